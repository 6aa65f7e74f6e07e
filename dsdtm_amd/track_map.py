"""libdsdtm_amd_trackmap.so (include/dsdtm_amd_trackmap.h) from Python: the track map resident on the device and
dsdtm_trackmap_local — the selection of Tracking::UpdateLocalMap plus dsdtm_track_desc's local-map columns (what
tracking.flatten_local_map builds by walking the objects) for n trackers in one submission. Restated in track_map_restatement.py.

    ctx = TrackMapContext()                  # one per calling thread
    store = TrackMapStore(ctx)               # mirrors keyframe / map-point objects into a device map
    store.add_keyframe(kf)                   # its map points are added on the way
    r = store.local(cam, T_cur_w)            # r["flat"]: pw, found, bad, off, okf, opx, olv, ob — tracking.TrackCall's `flat=`

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon
from .local_map import Camera, Params, camera_struct

LIB_NAME = "libdsdtm_amd_trackmap.so"
# every symbol include/dsdtm_amd_trackmap.h declares
SYMBOLS = ["dsdtm_trackmap_create", "dsdtm_trackmap_destroy", "dsdtm_trackmap_last_error", "dsdtm_trackmap_map_create",
           "dsdtm_trackmap_map_destroy", "dsdtm_trackmap_points_write", "dsdtm_trackmap_found_write", "dsdtm_trackmap_keyframe_add",
           "dsdtm_trackmap_keyframe_write", "dsdtm_trackmap_map_read", "dsdtm_trackmap_local"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MAX_LOCAL_POINTS, MAX_CALL_BYTES = 4096, 2147483648
FILL = 0xA5          # what local()'s output arrays hold before the call: entries the call does not write keep it


class Desc(C.Structure):
    """dsdtm_trackmap_desc"""
    _fields_ = [("map", C.c_void_p), ("T_cur_w", C.c_void_p), ("point_capacity", C.c_int32), ("obs_capacity", C.c_int32), ("kf", C.c_void_p),
                ("kf_dist", C.c_void_p), ("point", C.c_void_p), ("point_kf", C.c_void_p), ("mp_world", C.c_void_p), ("mp_found", C.c_void_p),
                ("mp_bad", C.c_void_p), ("obs_offset", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_px", C.c_void_p), ("obs_level", C.c_void_p),
                ("obs_bearing", C.c_void_p)]


class Result(C.Structure):
    """dsdtm_trackmap_result"""
    _fields_ = [("n_close", C.c_int32), ("n_kf", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("overflow_points", C.c_int32),
                ("overflow_obs", C.c_int32)]


class Image(C.Structure):
    """dsdtm_trackmap_image"""
    _fields_ = [("n_points", C.c_int32), ("n_keyframes", C.c_int32), ("n_slots_total", C.c_int64), ("complete", C.c_int32), ("reserved", C.c_int32),
                ("point_capacity", C.c_int32), ("keyframe_capacity", C.c_int32), ("slot_capacity", C.c_int64), ("p_world", C.c_void_p),
                ("bad", C.c_void_p), ("found", C.c_void_p), ("T_kf_w", C.c_void_p), ("n_slots", C.c_void_p), ("slot_offset", C.c_void_p),
                ("point_of_slot", C.c_void_p), ("observes", C.c_void_p), ("px_xy", C.c_void_p), ("level", C.c_void_p), ("bearing", C.c_void_p)]


class TrackMapError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_trackmap.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_trackmap"),
        "dsdtm_trackmap_map_create": (i, [vp, C.POINTER(vp)]),
        "dsdtm_trackmap_map_destroy": (None, [vp, vp]),
        "dsdtm_trackmap_points_write": (i, [vp, vp, i, i, vp, vp, vp]),
        "dsdtm_trackmap_found_write": (i, [vp, vp, i, vp, vp]),
        "dsdtm_trackmap_keyframe_add": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, C.POINTER(i)]),
        "dsdtm_trackmap_keyframe_write": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "dsdtm_trackmap_map_read": (i, [vp, vp, C.POINTER(Image)]),
        "dsdtm_trackmap_local": (i, [vp, C.POINTER(Camera), C.POINTER(Params), i, C.POINTER(Desc), C.POINTER(Result)])}, _not_built)


def _arr(a, dtype, shape):
    return np.ascontiguousarray(np.asarray(a, dtype).reshape(shape))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _filled(n, dtype):
    return np.full(max(int(n), 1) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


class TrackMapContext(_addon.AddonContext):
    """A dsdtm_trackmap_ctx: its own stream and staging blocks on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_trackmap", TrackMapError, staticmethod(load)

    def new_map(self) -> "DeviceTrackMap":
        return DeviceTrackMap(self)

    def local(self, cam, queries, n_local: int = 10, boundary: int = 0) -> list:
        """dsdtm_trackmap_local: `queries` is a list of (DeviceTrackMap, T_cur_w, point_capacity, obs_capacity). One submission.
        Returns one dict per query (LocalCall.answers)."""
        call = LocalCall(self, cam, queries, n_local, boundary)
        self.check(call.run_raw())
        return call.answers()


class LocalCall:
    """One prepared dsdtm_trackmap_local call: descriptors and output arrays are built once, run_raw() is the C call alone."""
    OUT = (("kf", np.int32, 1), ("kf_dist", np.float64, 1), ("point", np.int32, 1), ("point_kf", np.int32, 1), ("mp_world", np.float64, 3),
           ("mp_found", np.int32, 1), ("mp_bad", np.uint8, 1), ("obs_offset", np.int32, 1), ("obs_kf", np.int32, 1), ("obs_px", np.float32, 2),
           ("obs_level", np.int32, 1), ("obs_bearing", np.float64, 3))

    def __init__(self, ctx: TrackMapContext, cam, queries, n_local: int = 10, boundary: int = 0):
        self.ctx, self.n = ctx, len(queries)
        self.cam, self.prm = camera_struct(cam), Params(int(n_local), int(boundary))
        self.descs = (Desc * max(self.n, 1))()
        self.results = (Result * max(self.n, 1))()
        C.memset(self.results, FILL, C.sizeof(self.results))
        self.keep = []
        nl = max(int(n_local), 1)
        for k, (dmap, T, cap, ocap) in enumerate(queries):
            T, cap, ocap = _arr(T, np.float64, 12), int(cap), int(ocap)
            rows = dict(kf=nl, kf_dist=nl, obs_offset=max(cap, 0) + 1)
            raw = {name: _filled(rows.get(name, ocap if name.startswith("obs_") else cap) * width, dt) for name, dt, width in self.OUT}
            self.keep.append((dmap, T, cap, ocap, raw))
            d = self.descs[k]
            d.map, d.T_cur_w, d.point_capacity, d.obs_capacity = dmap.handle, T.ctypes.data, cap, ocap
            for name, _, _ in self.OUT:
                setattr(d, name, raw[name].ctypes.data)

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_trackmap_local(self.ctx.handle, C.byref(self.cam), C.byref(self.prm), self.n, self.descs, self.results)

    def answers(self) -> list:
        """Per query: kf, kf_dist, point, point_kf (lists), n_close, n_kf, n_points, n_obs, overflow_points, overflow_obs, `flat` (the
        columns under the keys of tracking.flatten_local_map: pw, found, bad, off, okf, opx, olv, ob — copies, cut to what the call
        wrote) and `raw` (the twelve output arrays whole: entries the call did not write hold FILL bytes)."""
        out = []
        for k, (_, _, cap, ocap, raw) in enumerate(self.keep):
            r = self.results[k]
            m, no = min(r.n_points, cap), min(r.n_obs, ocap)
            flat = dict(pw=raw["mp_world"][:3 * m].reshape(m, 3).copy(), found=raw["mp_found"][:m].copy(), bad=raw["mp_bad"][:m].copy(),
                        off=raw["obs_offset"][:m + 1].copy(), okf=raw["obs_kf"][:no].copy(), opx=raw["obs_px"][:2 * no].reshape(no, 2).copy(),
                        olv=raw["obs_level"][:no].copy(), ob=raw["obs_bearing"][:3 * no].reshape(no, 3).copy())
            out.append(dict(kf=raw["kf"][:r.n_kf].tolist(), kf_dist=raw["kf_dist"][:r.n_kf].tolist(), point=raw["point"][:m].tolist(),
                            point_kf=raw["point_kf"][:m].tolist(), n_close=r.n_close, n_kf=r.n_kf, n_points=r.n_points, n_obs=r.n_obs,
                            overflow_points=r.overflow_points, overflow_obs=r.overflow_obs, flat=flat, raw=raw))
        return out


class DeviceTrackMap:
    """A dsdtm_trackmap: one tracker's (or one rig's) map on the device. Updates return at once; they hold for every later call on
    the context, in call order."""

    def __init__(self, ctx: TrackMapContext):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_trackmap_map_create(ctx.handle, C.byref(h)))
        self.handle = h

    def points_write(self, first: int, p_world, bad=None, found=None):
        p = _arr(p_world, np.float64, (-1, 3))
        b = None if bad is None else _arr(bad, np.uint8, -1)
        f = None if found is None else _arr(found, np.int32, -1)
        for a, what in ((b, "flags"), (f, "found counts")):
            if a is not None and len(a) != len(p):
                raise ValueError(f"{len(a)} {what} for {len(p)} points")
        self.ctx.check(self.ctx.lib.dsdtm_trackmap_points_write(self.ctx.handle, self.handle, int(first), len(p), _ptr(p), _ptr(b), _ptr(f)))

    def found_write(self, index, found):
        i, f = _arr(index, np.int32, -1), _arr(found, np.int32, -1)
        if len(i) != len(f):
            raise ValueError(f"{len(f)} found counts for {len(i)} indices")
        self.ctx.check(self.ctx.lib.dsdtm_trackmap_found_write(self.ctx.handle, self.handle, len(i), _ptr(i), _ptr(f)))

    def keyframe_add(self, T_kf_w, point_of_slot, observes, px, level, bearing) -> int:
        T, s = _arr(T_kf_w, np.float64, 12), _arr(point_of_slot, np.int32, -1)
        o, x, l, b = _arr(observes, np.uint8, -1), _arr(px, np.float32, (-1, 2)), _arr(level, np.int32, -1), _arr(bearing, np.float64, (-1, 3))
        if not len(s) == len(o) == len(x) == len(l) == len(b):
            raise ValueError("the slot columns differ in length")
        k = C.c_int(-1)
        self.ctx.check(self.ctx.lib.dsdtm_trackmap_keyframe_add(self.ctx.handle, self.handle, T.ctypes.data, len(s), _ptr(s), _ptr(o), _ptr(x), _ptr(l),
                                                                _ptr(b), C.byref(k)))
        return k.value

    def keyframe_write(self, kf: int, T_kf_w=None, first_slot: int = 0, point_of_slot=(), observes=()):
        T = None if T_kf_w is None else _arr(T_kf_w, np.float64, 12)
        s, o = _arr(point_of_slot, np.int32, -1), _arr(observes, np.uint8, -1)
        if len(s) != len(o):
            raise ValueError(f"{len(o)} flags for {len(s)} slots")
        self.ctx.check(self.ctx.lib.dsdtm_trackmap_keyframe_write(self.ctx.handle, self.handle, int(kf), _ptr(T), int(first_slot), len(s), _ptr(s), _ptr(o)))

    def read(self) -> dict:
        """dsdtm_trackmap_map_read: the whole map as the restatement takes it (a world of track_map_restatement)."""
        im = Image()
        self.ctx.check(self.ctx.lib.dsdtm_trackmap_map_read(self.ctx.handle, self.handle, C.byref(im)))
        P, K, S = im.n_points, im.n_keyframes, im.n_slots_total
        p, b, f = np.zeros((P, 3), np.float64), np.zeros(P, np.uint8), np.zeros(P, np.int32)
        T, ns, off = np.zeros((K, 12), np.float64), np.zeros(K, np.int32), np.zeros(K, np.int64)
        sl, ob, px, lv, be = np.zeros(S, np.int32), np.zeros(S, np.uint8), np.zeros((S, 2), np.float32), np.zeros(S, np.int32), np.zeros((S, 3), np.float64)
        im.point_capacity, im.keyframe_capacity, im.slot_capacity = P, K, S
        (im.p_world, im.bad, im.found, im.T_kf_w, im.n_slots, im.slot_offset, im.point_of_slot, im.observes, im.px_xy, im.level,
         im.bearing) = (_ptr(a) for a in (p, b, f, T, ns, off, sl, ob, px, lv, be))
        self.ctx.check(self.ctx.lib.dsdtm_trackmap_map_read(self.ctx.handle, self.handle, C.byref(im)))
        assert im.complete == 1 and (im.n_points, im.n_keyframes, im.n_slots_total) == (P, K, S)
        cut = lambda a: [a[off[k]:off[k] + ns[k]].copy() for k in range(K)]
        return dict(p_world=p, bad=b, found=f, T_kf_w=T, slots=cut(sl), observes=cut(ob), px=cut(px), level=cut(lv), bearing=cut(be))

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.dsdtm_trackmap_map_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrackMapStore:
    """Mirrors keyframe / map-point objects into a DeviceTrackMap and keeps the index <-> object tables. The objects are the ones
    tracking.flatten_local_map walks: a map point has Get_Pose(), IsBad(), Get_FoundNums() and mObservations (keyframe index -> slot,
    the keyframe index being the one add_keyframe returned); a keyframe has Get_Pose(), mvMapPoints (a point or None per feature) and its
    features' px, level and bearing columns. A slot observes when its point's mObservations holds (this keyframe, this slot). The map's
    owner calls, where the reference's classes change what the call reads:
        add_keyframe(kf)        Tracking::CraeteKeyframe / Map::AddKeyFrame (its map points are added first, in slot order)
        update_point(mp)        MapPoint::Set_Pose (after local BA), MapPoint::SetBadFlag
        update_found(mps)       MapPoint::IncreaseFound / EraseFound (a tracked frame's matches)
        update_keyframe(kf)     KeyFrame::Set_Pose (after local BA), Add_MapPoint / Add_Observation, Erase_MapPointMatch, Erase_Observation
    """

    def __init__(self, ctx: TrackMapContext | None = None):
        self.ctx = ctx or TrackMapContext()
        self.map = self.ctx.new_map()
        self.points, self.keyframes = [], []            # index -> object
        self._point_index, self._kf_index = {}, {}      # id(object) -> index
        self.capacity_hint = (MAX_LOCAL_POINTS, 8192)   # local()'s remembered (point_capacity, obs_capacity)

    def point_index(self, mp) -> int:
        return self._point_index[id(mp)]

    def keyframe_index(self, kf) -> int:
        return self._kf_index[id(kf)]

    def add_points(self, mps):
        new = [mp for mp in {id(mp): mp for mp in mps}.values() if id(mp) not in self._point_index]      # (by identity: objects need no hash)
        if not new:
            return
        self.map.points_write(len(self.points), [mp.Get_Pose() for mp in new], [1 if mp.IsBad() else 0 for mp in new], [mp.Get_FoundNums() for mp in new])
        for mp in new:
            self._point_index[id(mp)] = len(self.points)
            self.points.append(mp)

    def update_point(self, mp):
        self.map.points_write(self._point_index[id(mp)], [mp.Get_Pose()], [1 if mp.IsBad() else 0], [mp.Get_FoundNums()])

    def update_found(self, mps):
        mps = list({id(mp): mp for mp in mps}.values())
        if mps:
            self.map.found_write([self._point_index[id(mp)] for mp in mps], [mp.Get_FoundNums() for mp in mps])

    def _slots(self, kf, k):
        slots = np.array([-1 if mp is None else self._point_index[id(mp)] for mp in kf.mvMapPoints], np.int32)
        observes = np.array([0 if mp is None else int(mp.mObservations.get(k, -1) == s) for s, mp in enumerate(kf.mvMapPoints)], np.uint8)
        return slots, observes

    def add_keyframe(self, kf) -> int:
        self.add_points([mp for mp in kf.mvMapPoints if mp is not None])
        k = len(self.keyframes)
        slots, observes = self._slots(kf, k)
        got = self.map.keyframe_add(np.asarray(kf.Get_Pose(), np.float64).reshape(12), slots, observes, np.asarray(kf.px, np.float32)[:len(slots)],
                                    np.asarray(kf.level, np.int32)[:len(slots)], np.asarray(kf.bearing, np.float64)[:len(slots)])
        assert got == k
        self._kf_index[id(kf)] = k
        self.keyframes.append(kf)
        return k

    def add_keyframe_columns(self, kf, new_points, point_of_slot, observes) -> int:
        """add_keyframe from the columns dsdtm_newkf_make returned (keyframe_creation.create_keyframes): `new_points` are appended as
        points [len(points), ...) in that order — the numbering point_of_slot was made with — and the keyframe's slots are written as
        given, without a walk over the objects. The caller enters the observations into the points afterwards."""
        first = len(self.points)
        if any(id(mp) in self._point_index for mp in new_points):
            raise ValueError("a new point is already in the map")
        if new_points:
            self.map.points_write(first, [mp.Get_Pose() for mp in new_points], [1 if mp.IsBad() else 0 for mp in new_points],
                                  [mp.Get_FoundNums() for mp in new_points])
        k = len(self.keyframes)
        try:
            got = self.map.keyframe_add(np.asarray(kf.Get_Pose(), np.float64).reshape(12), point_of_slot, observes, kf.px, kf.level, kf.bearing)
        finally:
            for mp in new_points:                           # (the points are in the device map whether or not the keyframe followed)
                self._point_index[id(mp)] = len(self.points)
                self.points.append(mp)
        assert got == k
        self._kf_index[id(kf)] = k
        self.keyframes.append(kf)
        return k

    def update_keyframe(self, kf, pose: bool = True, slots: bool = True):
        k = self._kf_index[id(kf)]
        if slots:
            self.add_points([mp for mp in kf.mvMapPoints if mp is not None])
        s, o = self._slots(kf, k) if slots else ((), ())
        self.map.keyframe_write(k, np.asarray(kf.Get_Pose(), np.float64).reshape(12) if pose else None, 0, s, o)

    def mirror(self) -> dict:
        """The map as the objects hold it now, as a world of track_map_restatement (what the device map equals when every change was
        reported)."""
        so = [self._slots(kf, k) for k, kf in enumerate(self.keyframes)]
        n = [len(s) for s, _ in so]
        return dict(p_world=np.array([mp.Get_Pose() for mp in self.points], np.float64).reshape(-1, 3),
                    bad=np.array([1 if mp.IsBad() else 0 for mp in self.points], np.uint8),
                    found=np.array([mp.Get_FoundNums() for mp in self.points], np.int32),
                    T_kf_w=np.array([np.asarray(kf.Get_Pose(), np.float64).reshape(12) for kf in self.keyframes], np.float64).reshape(-1, 12),
                    slots=[s for s, _ in so], observes=[o for _, o in so],
                    px=[np.asarray(kf.px, np.float32)[:c].reshape(c, 2) for kf, c in zip(self.keyframes, n)],
                    level=[np.asarray(kf.level, np.int32)[:c] for kf, c in zip(self.keyframes, n)],
                    bearing=[np.asarray(kf.bearing, np.float64)[:c].reshape(c, 3) for kf, c in zip(self.keyframes, n)])

    def local(self, cam, T_cur_w, n_local: int = 10, point_capacity: int | None = None, obs_capacity: int | None = None) -> dict:
        """One pose: the answer of TrackMapContext.local plus `keyframes` (mvpLocalKeyFrames) and `map_points` (the local points, in
        the order of the columns) as objects. r["flat"] goes to tracking.TrackCall as `flat=`, with keyframes = self.keyframes."""
        return local_maps(self.ctx, cam, [self], [T_cur_w], n_local, point_capacity, obs_capacity)[0]


def local_maps(ctx: TrackMapContext, cam, stores, Ts, n_local: int = 10, point_capacity: int | None = None, obs_capacity: int | None = None) -> list:
    """One dsdtm_trackmap_local for n stores of one context. The read-back is sized by the capacities, so a capacity left None is the
    store's REMEMBERED one: what its last call needed plus a quarter and 256 (at first 4096 points, 8192 observations). A list that does
    not fit is asked for again with room for all of it; more local points than dsdtm_track_desc takes (4096) raise — a result that
    overflows never reaches the tracker."""
    if len(stores) != len(Ts):
        raise ValueError(f"{len(stores)} stores, {len(Ts)} poses")
    caps = [[s.capacity_hint[0] if point_capacity is None else int(point_capacity), s.capacity_hint[1] if obs_capacity is None else int(obs_capacity)] for s in stores]
    for attempt in range(3):
        rs = ctx.local(cam, [(s.map, T, c[0], c[1]) for s, T, c in zip(stores, Ts, caps)], n_local, 0)
        over = [r for r in rs if r["overflow_points"] or r["overflow_obs"]]
        if not over:
            break
        for r, c in zip(rs, caps):
            if r["overflow_points"]:
                if c[0] == MAX_LOCAL_POINTS:
                    raise TrackMapError(ERR_INVALID, f"{r['n_points']} local points exceed the {MAX_LOCAL_POINTS} a dsdtm_track_desc takes")
                c[0], c[1] = MAX_LOCAL_POINTS, max(c[1], 2 * r["n_obs"] + 256)      # (n_obs was the cut list's)
            elif r["overflow_obs"]:
                c[1] = r["n_obs"]
    else:
        raise TrackMapError(ERR_INVALID, "the local map did not fit after two enlargements")
    for s, r in zip(stores, rs):
        s.capacity_hint = (min(MAX_LOCAL_POINTS, r["n_points"] + r["n_points"] // 4 + 256), r["n_obs"] + r["n_obs"] // 4 + 256)
        r["keyframes"], r["map_points"] = [s.keyframes[k] for k in r["kf"]], [s.points[p] for p in r["point"]]
    return rs
