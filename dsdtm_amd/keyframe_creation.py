"""libdsdtm_amd_newkf.so (include/dsdtm_amd_newkf.h) from Python: dsdtm_newkf_make / dsdtm_newkf_make_batch — the walk of
Feature_detector::detect behind the image work and the slots of Tracking::CraeteKeyframe (reference src/Tracking.cpp:412-464) for n
trackers in one submission. The rules are restated in keyframe_creation_restatement.py.

    ctx = NewKeyframeContext()               # one per calling thread
    out = ctx.make(cam, params, inp)         # inp: a NewKeyframeInput; out: the dict create_keyframe() of the restatement returns
    outs = ctx.make_batch(cam, params, [inp0, inp1, ...])

The cell arrays, the depth image and the dynamic mask of an input may each be a numpy array (host memory) or a DeviceArray (an address
in this device's memory or in pinned host memory, e.g. a torch tensor's data_ptr()).

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _addon
from .keyframe_creation_restatement import COLUMNS, NewKeyframeInput, NewKeyframeParams  # noqa: F401  (re-exported)

LIB_NAME = "libdsdtm_amd_newkf.so"
# every symbol include/dsdtm_amd_newkf.h declares
SYMBOLS = ["dsdtm_newkf_create", "dsdtm_newkf_destroy", "dsdtm_newkf_last_error", "dsdtm_newkf_make", "dsdtm_newkf_make_batch"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MAX_TRACKERS, MAX_CELLS, MAX_EXISTING, MAX_RADIUS, MAX_SIDE = 1024, 4096, 4096, 127, 16384
FILL = 0xA5          # what the output arrays hold before the call: entries the call does not write keep it


class Camera(C.Structure):
    """dsdtm_camera (include/dsdtm_amd.h)"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("f", C.c_float), ("width", C.c_int), ("height", C.c_int)]


class Params(C.Structure):
    """dsdtm_newkf_params"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("cell_size", C.c_int32), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32),
                ("max_fts", C.c_int32), ("min_dist", C.c_int32), ("score_floor", C.c_float)]


class Desc(C.Structure):
    """dsdtm_newkf_desc"""
    _fields_ = [("cell_score", C.c_void_p), ("cell_x", C.c_void_p), ("cell_y", C.c_void_p), ("cell_level", C.c_void_p),
                ("n_existing", C.c_int32), ("first_point_index", C.c_int32), ("px_xy", C.c_void_p), ("level", C.c_void_p),
                ("bearing", C.c_void_p), ("has_point", C.c_void_p), ("initial", C.c_void_p), ("point_index", C.c_void_p),
                ("depth", C.c_void_p), ("depth_stride", C.c_int32), ("depth_scale", C.c_float),
                ("dyn_stride", C.c_int32), ("dyn_mask", C.c_void_p), ("T_c2w", C.c_void_p),
                ("slot_capacity", C.c_int32), ("point_capacity", C.c_int32), ("bad_capacity", C.c_int32), ("reserved", C.c_int32)]


class Result(C.Structure):
    """dsdtm_newkf_result"""
    _fields_ = [("n_new", C.c_int32), ("n_slots", C.c_int32), ("n_new_points", C.c_int32), ("overflow", C.c_int32),
                ("point_of_slot", C.c_void_p), ("observes", C.c_void_p), ("px_xy", C.c_void_p), ("level", C.c_void_p), ("bearing", C.c_void_p),
                ("depth_of_slot", C.c_void_p), ("new_p_world", C.c_void_p), ("new_bad", C.c_void_p)]


class NewKeyframeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


@dataclass
class DeviceArray:
    """An array the library reads where it is: `ptr` is an address in this device's memory or in pinned host memory; `stride` is the
    row pitch of an image (depth: in elements, dyn_mask: in bytes). `keep` holds whatever owns the memory."""
    ptr: int
    stride: int = 0
    keep: object = None


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_newkf.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_newkf"),
        "dsdtm_newkf_make": (i, [vp, C.POINTER(Camera), C.POINTER(Params), C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_newkf_make_batch": (i, [vp, C.POINTER(Camera), C.POINTER(Params), i, C.POINTER(Desc), C.POINTER(Result)])}, _not_built)


def camera_struct(cam) -> Camera:
    if isinstance(cam, Camera):
        return cam
    if isinstance(cam, (tuple, list)):
        fx, fy, cx, cy = (float(v) for v in cam)
        return Camera(fx, fy, cx, cy, fx, 0, 0)
    return Camera(float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), float(getattr(cam, "f", cam.fx)), int(cam.width), int(cam.height))


def params_struct(p) -> Params:
    if isinstance(p, Params):
        return p
    return Params(int(p.width), int(p.height), int(p.cell_size), int(p.grid_cols), int(p.grid_rows), int(p.max_fts), int(p.min_dist), float(p.score_floor))


class MakeCall:
    """One prepared dsdtm_newkf_make_batch call: descriptors and output arrays are built once, run_raw() is the C call alone.
    `capacities`: per input (slot_capacity, point_capacity), or None for what always fits."""

    def __init__(self, ctx, cam, params, inputs, capacities=None, single=False):
        self.ctx, self.single = ctx, single
        self.cam, self.prm = camera_struct(cam), params_struct(params)
        n = len(inputs)
        G = self.prm.grid_cols * self.prm.grid_rows
        self.descs, self.results = (Desc * n)(), (Result * n)()
        self.keep, self.out = [], []
        for t, inp in enumerate(inputs):
            d = self.descs[t]
            ne = inp.n_existing
            for name, dt in (("cell_score", np.float32), ("cell_x", np.int32), ("cell_y", np.int32), ("cell_level", np.int32)):
                setattr(d, name, self._array(getattr(inp, name), dt)[0])
            d.n_existing, d.first_point_index = ne, int(inp.first_point_index)
            for name, dt in (("px_xy", np.float32), ("level", np.int32), ("bearing", np.float64), ("has_point", np.uint8),
                             ("initial", np.uint8), ("point_index", np.int32)):
                a = np.ascontiguousarray(np.asarray(getattr(inp, name), dt))
                self.keep.append(a)
                setattr(d, name, a.ctypes.data if ne else None)
            d.depth, stride = self._array(inp.depth, np.uint16)
            d.depth_stride, d.depth_scale = stride, float(inp.depth_scale)
            if inp.dyn_mask is not None:
                d.dyn_mask, d.dyn_stride = self._array(inp.dyn_mask, np.uint8)
            T = np.ascontiguousarray(np.asarray(inp.T_c2w, np.float64).reshape(12))
            self.keep.append(T)
            d.T_c2w = T.ctypes.data
            if capacities is None:
                slots = ne + min(G, max(0, self.prm.max_fts - ne))
                points = slots
            else:
                slots, points = capacities[t]
            d.slot_capacity, d.point_capacity, d.bad_capacity = slots, points, points
            o = {"point_of_slot": np.empty(max(slots, 1), np.int32), "observes": np.empty(max(slots, 1), np.uint8),
                 "px_xy": np.empty((max(slots, 1), 2), np.float32), "level": np.empty(max(slots, 1), np.int32),
                 "bearing": np.empty((max(slots, 1), 3), np.float64), "depth_of_slot": np.empty(max(slots, 1), np.float32),
                 "new_p_world": np.empty((max(points, 1), 3), np.float64), "new_bad": np.empty(max(points, 1), np.uint8)}
            for name, a in o.items():
                a.view(np.uint8).fill(FILL)
                setattr(self.results[t], name, a.ctypes.data)
            self.out.append(o)

    def _array(self, a, dt):
        """(address, row stride in elements) of a caller's array: a DeviceArray as it is, anything else as a contiguous numpy array."""
        if isinstance(a, DeviceArray):
            self.keep.append(a)
            return a.ptr, int(a.stride)
        a = np.asarray(a)
        if a.dtype != dt or a.ndim == 0 or a.strides[-1] != a.itemsize or (a.ndim == 2 and a.strides[0] % a.itemsize):
            a = np.ascontiguousarray(a, dt)
        self.keep.append(a)
        return a.ctypes.data, (a.strides[0] // a.itemsize if a.ndim == 2 else 0)

    def run_raw(self) -> int:
        lib, h = self.ctx.lib, self.ctx.handle
        if self.single:
            return lib.dsdtm_newkf_make(h, C.byref(self.cam), C.byref(self.prm), self.descs, self.results)
        return lib.dsdtm_newkf_make_batch(h, C.byref(self.cam), C.byref(self.prm), len(self.descs), self.descs, self.results)

    def answers(self) -> list:
        """One dict per input: the counts, `overflow`, the COLUMNS cut to their counts (empty on overflow) and `raw`: the output arrays whole."""
        outs = []
        for r, o in zip(self.results, self.out):
            ns, npnt = (0, 0) if r.overflow else (r.n_slots, r.n_new_points)
            a = {"n_new": r.n_new, "n_slots": r.n_slots, "n_new_points": r.n_new_points, "overflow": r.overflow, "raw": o}
            for name in COLUMNS:
                a[name] = o[name][:npnt] if name == "new_p_world" else o[name][:ns]
            a["new_bad"] = o["new_bad"][:npnt]
            outs.append(a)
        return outs


class NewKeyframeContext(_addon.AddonContext):
    """A dsdtm_newkf_ctx: its own stream and staging blocks on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_newkf", NewKeyframeError, staticmethod(load)

    def make(self, cam, params, inp, capacity=None) -> dict:
        """dsdtm_newkf_make for one NewKeyframeInput."""
        call = MakeCall(self, cam, params, [inp], None if capacity is None else [capacity], single=True)
        self.check(call.run_raw())
        return call.answers()[0]

    def make_batch(self, cam, params, inputs, capacities=None) -> list:
        """dsdtm_newkf_make_batch: one submission for all inputs."""
        call = MakeCall(self, cam, params, inputs, capacities)
        self.check(call.run_raw())
        return call.answers()


# ---- the adapter: Tracking::CraeteKeyframe / CreateInitialMapRGBD on frame, keyframe and map-point objects -------------------------
class NewMapPoint:
    """A map point CraeteKeyframe makes (src/Tracking.cpp:444), with what track_map.TrackMapStore reads from a point."""

    def __init__(self, pos):
        self._pos = np.asarray(pos, np.float64).reshape(3).copy()
        self._bad, self._found = False, 0
        self.mObservations = {}                     # keyframe index of the store -> slot

    def Get_Pose(self):
        return self._pos.copy()

    def Set_Pose(self, p):
        self._pos = np.asarray(p, np.float64).reshape(3).copy()

    def IsBad(self):
        return self._bad

    def SetBadFlag(self):
        self._bad = True

    def Get_FoundNums(self):
        return self._found

    def IncreaseFound(self, n: int = 1):
        self._found += n

    def EraseFound(self, n: int = 1):
        self._found -= n


class NewKeyFrame:
    """KeyFrame(mCurrentFrame) (src/Tracking.cpp:420): the frame's pose and its features' columns, fixed from here on, and mvMapPoints."""

    def __init__(self, T_c2w, px, level, bearing, map_points):
        self._T = np.asarray(T_c2w, np.float64).reshape(3, 4).copy()
        self.px, self.level, self.bearing = np.array(px, np.float32), np.array(level, np.int32), np.array(bearing, np.float64)
        self.mvMapPoints = list(map_points)
        self.mOrderedCovGraph = []                  # [(weight, keyframe index)] ascending, as dsdtm_mapping_covisibility lists it

    def Get_Pose(self):
        return self._T.copy()

    def Set_Pose(self, T):
        self._T = np.asarray(T, np.float64).reshape(3, 4).copy()


def create_keyframes(gpu_ctx, nctx, cam, frames, stores, depths, depth_scale: float = 5000.0, detection_threshold: float = 5.0,
                     min_points: int = 0) -> list:
    """Tracking::CraeteKeyframe (src/Tracking.cpp:412-464) for n trackers: Set_ExistingFeatures and dsdtm_detect_cells_frame per frame,
    ONE dsdtm_newkf_make_batch, then per store points_write + keyframe_add with the returned columns, then KeyFrame::UpdateConnection
    through dsdtm_mapping_covisibility where the stores' context is a ba_window.MappingContext (one call for all). The new features and
    points are appended to the frame objects. frames[i]: a frame.Frame with its pyramid or a resident _device_frame, and mvMapPoints
    (absent: no feature has a point); stores[i]: a track_map.TrackMapStore that knows every map point of the frame; depths[i]: the
    frame's uint16 depth image (host array or DeviceArray). min_points: CreateInitialMapRGBD's test (:182) — a tracker that makes
    fewer new points is left untouched and answers None. Returns one dict per tracker: keyframe, kf (its index), new_points, n_new,
    cov (the covisibility answer, or None)."""
    from .feature_detection import Feature_detector
    from .frame import Config
    n = len(frames)
    if not (n == len(stores) == len(depths)):
        raise ValueError(f"{n} frames, {len(stores)} stores, {len(depths)} depth images")
    if n == 0:
        return []
    h, w = int(cam.height), int(cam.width)
    det = Feature_detector(w, h, ctx=gpu_ctx)
    prm = NewKeyframeParams(w, h, det.mCell_size, det.mGrid_cols, det.mGrid_rows, det.mMax_fts, int(Config.Get("Camera.Min_dist")), 20.0)
    inputs = []
    for fr, store, depth in zip(frames, stores, depths):
        ne = fr.n_features
        mps = list(getattr(fr, "mvMapPoints", [None] * ne))
        det.Set_ExistingFeatures(fr.px if ne else np.zeros((0, 2), np.float32))                     # :415
        s, x, y, l = (a.copy() for a in det.detect_cells(fr, detection_threshold))                  # the image work of :416
        det.ResetGrid()
        inp = NewKeyframeInput(s, x, y, l, depth, depth_scale, np.asarray(fr.Get_Pose(), np.float64).reshape(12), len(store.points),
                               px_xy=fr.px if ne else np.zeros((0, 2), np.float32), level=fr.level if ne else np.zeros(0, np.int32),
                               bearing=fr.bearing if ne else np.zeros((0, 3)),
                               has_point=np.array([mp is not None for mp in mps], np.uint8), initial=np.asarray(fr.initial, np.uint8) if ne else np.zeros(0, np.uint8),
                               point_index=np.array([-1 if mp is None else store.point_index(mp) for mp in mps], np.int32))
        inputs.append((inp, mps))
    # trackers that share a store (a rig): their point numbers follow each other, so they are made one after the other
    shared = len({id(s) for s in stores}) < n
    if shared:
        outs = []
        for (inp, _), store in zip(inputs, stores):
            inp.first_point_index = len(store.points) + sum(o["n_new_points"] for o, st in zip(outs, stores) if st is store)
            outs.append(nctx.make(cam, prm, inp))
    else:
        for (inp, _), store in zip(inputs, stores):
            inp.first_point_index = len(store.points)
        outs = nctx.make_batch(cam, prm, [i for i, _ in inputs])
    answers, pairs = [], []
    for fr, store, (inp, mps), o in zip(frames, stores, inputs, outs):
        if o["n_new_points"] < min_points:
            answers.append(None)
            continue
        ne, S = inp.n_existing, o["n_slots"]
        new_points = [NewMapPoint(p) for p in o["new_p_world"]]
        slot_points = mps + [None] * o["n_new"]
        for i in range(S):
            p = int(o["point_of_slot"][i])
            if p >= inp.first_point_index and not (i < ne and inp.initial[i]):
                slot_points[i] = new_points[p - inp.first_point_index]                               # :446-451
        kf = NewKeyFrame(fr.Get_Pose(), o["px_xy"], o["level"], o["bearing"], slot_points)
        k = store.add_keyframe_columns(kf, new_points, o["point_of_slot"], o["observes"])            # :421, :453
        for i in range(S):
            if o["observes"][i]:
                slot_points[i].mObservations.setdefault(k, i)                                        # :431, :448
        # the frame object: the new features, and the points the lifted features got (:450-451)
        m = o["n_new"]
        p_world = np.zeros((S, 3))
        p_world[:ne] = fr.p_world if ne else np.zeros((0, 3))
        for i in range(S):
            if slot_points[i] is not None and not (i < ne and inp.initial[i]):
                p_world[i] = slot_points[i].Get_Pose()
        fr.set_features(o["px_xy"].copy(), o["bearing"].copy(), p_world, np.concatenate([inp.initial, np.zeros(m, np.uint8)]), o["level"].copy())
        fr.mvMapPoints = list(slot_points)
        answers.append(dict(keyframe=kf, kf=k, new_points=new_points, n_new=m, cov=None))
        if hasattr(store.ctx, "covisibility"):
            pairs.append((len(answers) - 1, store, k))
    by_ctx = {}
    for at, store, k in pairs:
        by_ctx.setdefault(id(store.ctx), (store.ctx, []))[1].append((at, store, k))
    for mctx, items in by_ctx.values():                                                              # :459 tKFrame->UpdateConnection()
        for (at, store, k), cov in zip(items, mctx.covisibility([(store.map, k, max(len(store.keyframes), 1)) for _, store, k in items])):
            answers[at]["cov"] = cov
            answers[at]["keyframe"].mOrderedCovGraph = list(zip(cov["cov_weight"], cov["cov_kf"]))
    return answers
