"""libdsdtm_amd_localmap.so (include/dsdtm_amd_localmap.h) from Python: the map resident on the device and
dsdtm_localmap_select — Tracking::GetCloseKeyFrames and the keyframe and point selection of Tracking::UpdateLocalMap
(reference src/Tracking.cpp:258-345) for n trackers in one submission. The rules are restated in local_map_restatement.py.

    ctx = LocalMapContext()                  # one per calling thread
    store = LocalMapStore(ctx)               # mirrors mapping.KeyFrame / MapPoint objects into a device map
    store.add_keyframe(kf)                   # its map points are added on the way
    keyframes, map_points = store.update_local_map(cam, T_cur_w)      # what Tracker.TrackFrame takes

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_localmap.so"
# every symbol include/dsdtm_amd_localmap.h declares
SYMBOLS = ["dsdtm_localmap_create", "dsdtm_localmap_destroy", "dsdtm_localmap_last_error", "dsdtm_localmap_map_create",
           "dsdtm_localmap_map_destroy", "dsdtm_localmap_points_write", "dsdtm_localmap_keyframe_add", "dsdtm_localmap_keyframe_write",
           "dsdtm_localmap_map_read", "dsdtm_localmap_select"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MAX_POINTS, MAX_KEYFRAMES, MAX_SLOTS, MAX_LOCAL, MAX_DESCS = 1048576, 16384, 4096, 64, 1024
# what a map's device arrays start with (csrc/localmap.h): each doubles when an update needs more
INITIAL_POINTS, INITIAL_KEYFRAMES, INITIAL_SLOTS = 4096, 64, 16384
FILL = 0xA5          # what select()'s output arrays hold before the call: entries the call does not write keep it


class Camera(C.Structure):
    """dsdtm_camera (include/dsdtm_amd.h)"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("f", C.c_float), ("width", C.c_int), ("height", C.c_int)]


class Params(C.Structure):
    """dsdtm_localmap_params"""
    _fields_ = [("n_local", C.c_int32), ("boundary", C.c_int32)]


class Desc(C.Structure):
    """dsdtm_localmap_desc"""
    _fields_ = [("map", C.c_void_p), ("T_cur_w", C.c_void_p), ("kf", C.c_void_p), ("kf_dist", C.c_void_p), ("point_capacity", C.c_int32),
                ("reserved", C.c_int32), ("point", C.c_void_p), ("point_kf", C.c_void_p)]


class Result(C.Structure):
    """dsdtm_localmap_result"""
    _fields_ = [("n_close", C.c_int32), ("n_kf", C.c_int32), ("n_points", C.c_int32), ("overflow", C.c_int32)]


class Image(C.Structure):
    """dsdtm_localmap_image"""
    _fields_ = [("n_points", C.c_int32), ("n_keyframes", C.c_int32), ("n_slots_total", C.c_int64), ("complete", C.c_int32), ("reserved", C.c_int32),
                ("point_capacity", C.c_int32), ("keyframe_capacity", C.c_int32), ("slot_capacity", C.c_int64), ("p_world", C.c_void_p),
                ("bad", C.c_void_p), ("T_kf_w", C.c_void_p), ("n_slots", C.c_void_p), ("slot_offset", C.c_void_p), ("point_of_slot", C.c_void_p)]


class LocalMapError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_localmap.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_localmap"),
        "dsdtm_localmap_map_create": (i, [vp, C.POINTER(vp)]),
        "dsdtm_localmap_map_destroy": (None, [vp, vp]),
        "dsdtm_localmap_points_write": (i, [vp, vp, i, i, vp, vp]),
        "dsdtm_localmap_keyframe_add": (i, [vp, vp, vp, i, vp, C.POINTER(i)]),
        "dsdtm_localmap_keyframe_write": (i, [vp, vp, i, vp, i, i, vp]),
        "dsdtm_localmap_map_read": (i, [vp, vp, C.POINTER(Image)]),
        "dsdtm_localmap_select": (i, [vp, C.POINTER(Camera), C.POINTER(Params), i, C.POINTER(Desc), C.POINTER(Result)])}, _not_built)


def camera_struct(cam) -> Camera:
    if isinstance(cam, Camera):
        return cam
    return Camera(float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), float(getattr(cam, "f", cam.fx)), int(cam.width), int(cam.height))


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class LocalMapContext(_addon.AddonContext):
    """A dsdtm_localmap_ctx: its own stream and staging blocks on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_localmap", LocalMapError, staticmethod(load)

    def new_map(self) -> "DeviceMap":
        return DeviceMap(self)

    def select(self, cam, queries, n_local: int = 10, boundary: int = 0) -> list:
        """dsdtm_localmap_select: `queries` is a list of (DeviceMap, T_cur_w, point_capacity). One submission. Returns one dict per
        query: kf, kf_dist (n_kf), point, point_kf (min(n_points, point_capacity)), n_close, n_kf, n_points, overflow, and `raw`:
        the four output arrays whole (entries the call did not write hold FILL bytes)."""
        call = SelectCall(self, cam, queries, n_local, boundary)
        self.check(call.run_raw())
        return call.answers()


class SelectCall:
    """One prepared dsdtm_localmap_select call: descriptors and output arrays are built once, run_raw() is the C call alone."""

    def __init__(self, ctx: LocalMapContext, cam, queries, n_local: int = 10, boundary: int = 0):
        self.ctx, self.n = ctx, len(queries)
        self.cam, self.prm = camera_struct(cam), Params(int(n_local), int(boundary))
        self.descs = (Desc * max(self.n, 1))()
        self.results = (Result * max(self.n, 1))()
        C.memset(self.results, FILL, C.sizeof(self.results))
        self.keep = []
        nl = max(int(n_local), 1)
        for k, (dmap, T, cap) in enumerate(queries):
            T = _f64(T, 12)
            kf, dist = np.full(nl, FILL, np.uint8).repeat(4).view(np.int32), np.full(nl * 8, FILL, np.uint8).view(np.float64)
            point, point_kf = (np.full(max(int(cap), 1) * 4, FILL, np.uint8).view(np.int32) for _ in range(2))
            self.keep.append((dmap, T, kf, dist, point, point_kf, int(cap)))
            d = self.descs[k]
            d.map, d.T_cur_w, d.kf, d.kf_dist = dmap.handle, T.ctypes.data, kf.ctypes.data, dist.ctypes.data
            d.point_capacity, d.point, d.point_kf = int(cap), point.ctypes.data, point_kf.ctypes.data

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_localmap_select(self.ctx.handle, C.byref(self.cam), C.byref(self.prm), self.n, self.descs, self.results)

    def answers(self) -> list:
        out = []
        for k, (_, _, kf, dist, point, point_kf, cap) in enumerate(self.keep):
            r = self.results[k]
            m = min(r.n_points, cap)
            out.append(dict(kf=kf[:r.n_kf].tolist(), kf_dist=dist[:r.n_kf].tolist(), point=point[:m].tolist(), point_kf=point_kf[:m].tolist(),
                            n_close=r.n_close, n_kf=r.n_kf, n_points=r.n_points, overflow=r.overflow,
                            raw=dict(kf=kf, kf_dist=dist, point=point, point_kf=point_kf)))
        return out


class DeviceMap:
    """A dsdtm_localmap: one tracker's (or one rig's) map on the device. Updates return at once; they hold for every later call on
    the context, in call order."""

    def __init__(self, ctx: LocalMapContext):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_localmap_map_create(ctx.handle, C.byref(h)))
        self.handle = h

    def points_write(self, first: int, p_world, bad=None):
        p = _f64(p_world, (-1, 3))
        b = None if bad is None else np.ascontiguousarray(np.asarray(bad, np.uint8).reshape(-1))
        if b is not None and len(b) != len(p):
            raise ValueError(f"{len(b)} flags for {len(p)} points")
        self.ctx.check(self.ctx.lib.dsdtm_localmap_points_write(self.ctx.handle, self.handle, int(first), len(p), _ptr(p), _ptr(b)))

    def keyframe_add(self, T_kf_w, point_of_slot) -> int:
        T, s = _f64(T_kf_w, 12), np.ascontiguousarray(np.asarray(point_of_slot, np.int32).reshape(-1))
        k = C.c_int(-1)
        self.ctx.check(self.ctx.lib.dsdtm_localmap_keyframe_add(self.ctx.handle, self.handle, T.ctypes.data, len(s), _ptr(s), C.byref(k)))
        return k.value

    def keyframe_write(self, kf: int, T_kf_w=None, first_slot: int = 0, point_of_slot=()):
        T = None if T_kf_w is None else _f64(T_kf_w, 12)
        s = np.ascontiguousarray(np.asarray(point_of_slot, np.int32).reshape(-1))
        self.ctx.check(self.ctx.lib.dsdtm_localmap_keyframe_write(self.ctx.handle, self.handle, int(kf), _ptr(T), int(first_slot), len(s), _ptr(s)))

    def read(self) -> dict:
        """dsdtm_localmap_map_read: the whole map as the restatement takes it (p_world, bad, T_kf_w, slots)."""
        im = Image()
        self.ctx.check(self.ctx.lib.dsdtm_localmap_map_read(self.ctx.handle, self.handle, C.byref(im)))
        P, K, S = im.n_points, im.n_keyframes, im.n_slots_total
        p, b = np.zeros((P, 3), np.float64), np.zeros(P, np.uint8)
        T, ns, off, sl = np.zeros((K, 12), np.float64), np.zeros(K, np.int32), np.zeros(K, np.int64), np.zeros(S, np.int32)
        im.point_capacity, im.keyframe_capacity, im.slot_capacity = P, K, S
        im.p_world, im.bad, im.T_kf_w, im.n_slots, im.slot_offset, im.point_of_slot = (_ptr(a) for a in (p, b, T, ns, off, sl))
        self.ctx.check(self.ctx.lib.dsdtm_localmap_map_read(self.ctx.handle, self.handle, C.byref(im)))
        assert im.complete == 1 and (im.n_points, im.n_keyframes, im.n_slots_total) == (P, K, S)
        return dict(p_world=p, bad=b, T_kf_w=T, slots=[sl[off[k]:off[k] + ns[k]].copy() for k in range(K)])

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.dsdtm_localmap_map_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LocalMapStore:
    """Mirrors mapping.KeyFrame / MapPoint objects (Get_Pose(), IsBad(), mvMapPoints) into a DeviceMap and keeps the index <-> object
    tables. The map's owner calls, where the reference's classes change what the selection reads:
        add_keyframe(kf)        Map::AddKeyFrame (its map points are added first, in slot order)
        update_point(mp)        MapPoint::Set_Pose (after local BA), MapPoint::SetBadFlag
        update_keyframe(kf)     KeyFrame::Set_Pose (after local BA), KeyFrame::Add_MapPoint, KeyFrame::Erase_MapPointMatch
    """

    def __init__(self, ctx: LocalMapContext | None = None):
        self.ctx = ctx or LocalMapContext()
        self.map = self.ctx.new_map()
        self.points, self.keyframes = [], []            # index -> object
        self._point_index, self._kf_index = {}, {}      # id(object) -> index

    def point_index(self, mp) -> int:
        return self._point_index[id(mp)]

    def keyframe_index(self, kf) -> int:
        return self._kf_index[id(kf)]

    def add_points(self, mps):
        new = [mp for mp in {id(mp): mp for mp in mps}.values() if id(mp) not in self._point_index]      # (by identity: objects need no hash)
        if not new:
            return
        first = len(self.points)
        self.map.points_write(first, [mp.Get_Pose() for mp in new], [1 if mp.IsBad() else 0 for mp in new])
        for mp in new:
            self._point_index[id(mp)] = len(self.points)
            self.points.append(mp)

    def update_point(self, mp):
        self.map.points_write(self._point_index[id(mp)], [mp.Get_Pose()], [1 if mp.IsBad() else 0])

    def _slots(self, kf):
        return [-1 if mp is None else self._point_index[id(mp)] for mp in kf.mvMapPoints]

    def add_keyframe(self, kf) -> int:
        self.add_points([mp for mp in kf.mvMapPoints if mp is not None])
        k = self.map.keyframe_add(np.asarray(kf.Get_Pose(), np.float64).reshape(12), self._slots(kf))
        assert k == len(self.keyframes)
        self._kf_index[id(kf)] = k
        self.keyframes.append(kf)
        return k

    def update_keyframe(self, kf, pose: bool = True, slots: bool = True):
        if slots:
            self.add_points([mp for mp in kf.mvMapPoints if mp is not None])
        self.map.keyframe_write(self._kf_index[id(kf)], np.asarray(kf.Get_Pose(), np.float64).reshape(12) if pose else None, 0,
                                self._slots(kf) if slots else ())

    def mirror(self) -> dict:
        """The map as the objects hold it now, in the restatement's form (what the device map equals when every change was reported)."""
        return dict(p_world=np.array([mp.Get_Pose() for mp in self.points], np.float64).reshape(-1, 3),
                    bad=np.array([1 if mp.IsBad() else 0 for mp in self.points], np.uint8),
                    T_kf_w=np.array([np.asarray(kf.Get_Pose(), np.float64).reshape(12) for kf in self.keyframes], np.float64).reshape(-1, 12),
                    slots=[np.array(self._slots(kf), np.int32) for kf in self.keyframes])

    def update_local_map(self, cam, T_cur_w, n_local: int = 10, point_capacity: int | None = None):
        """(keyframes, map_points): mvpLocalKeyFrames and the local points in the order the reference hands them to ReprojectPoint."""
        return update_local_maps(self.ctx, cam, [self], [T_cur_w], n_local, point_capacity)[0]


def update_local_maps(ctx: LocalMapContext, cam, stores, Ts, n_local: int = 10, point_capacity: int | None = None) -> list:
    """One dsdtm_localmap_select for n stores of one context: [(keyframes, map_points)] as objects."""
    if len(stores) != len(Ts):
        raise ValueError(f"{len(stores)} stores, {len(Ts)} poses")
    caps = [min(n_local * MAX_SLOTS, max(1, len(s.points))) if point_capacity is None else int(point_capacity) for s in stores]
    rs = ctx.select(cam, [(s.map, T, c) for s, T, c in zip(stores, Ts, caps)], n_local, 0)
    out = []
    for s, r in zip(stores, rs):
        if r["overflow"]:
            raise LocalMapError(ERR_INVALID, f"{r['n_points']} local points exceed point_capacity")
        out.append(([s.keyframes[k] for k in r["kf"]], [s.points[p] for p in r["point"]]))
    return out
