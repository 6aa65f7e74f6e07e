"""libdsdtm_amd_slam.so (include/dsdtm_amd_slam.h) from Python: ONE resident map for the whole per-frame loop — the track map and its
local-map columns, the mapping thread's covisibility list, window and commit, and dsdtm_slam_track_commit: a tracked frame's effects on
the map (IncreaseFound, the EraseFound walk, the SetBadFlag cascade). Restated in aftertrack_restatement.py.

    ctx = SlamContext()                      # one per calling thread; a ba_window.MappingContext and more
    store = track_map.TrackMapStore(ctx)     # mirrors keyframe / map-point objects into the resident map
    r = store.local(cam, T_cur_w)            # the local map of the frame
    ... dsdtm_track_frame ...
    out = ctx.track_commit(thresh, [(store.map, [r["point"][i] for i in matches["point"]], residual_norm)])

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon, ba_window, capi, track_map
from .capi import LocalBaProblem
from .local_map import Camera, Params

LIB_NAME = "libdsdtm_amd_slam.so"
# every symbol include/dsdtm_amd_slam.h declares
SYMBOLS = ["dsdtm_slam_" + s[len("dsdtm_mapping_"):] for s in ba_window.SYMBOLS] + ["dsdtm_slam_track_commit", "dsdtm_slam_need_keyframes"]
MAX_MATCHES, MAX_DESCS = 256, 1024
FILL = 0xA5


class CommitDesc(C.Structure):
    """dsdtm_slam_commit_desc"""
    _fields_ = [("map", C.c_void_p), ("n_matches", C.c_int32), ("reserved", C.c_int32), ("point", C.c_void_p), ("residual_norm", C.c_void_p),
                ("found_after", C.c_void_p)]


class CommitResult(C.Structure):
    """dsdtm_slam_commit_result"""
    _fields_ = [("n_erased", C.c_int32), ("n_bad", C.c_int32), ("overflow_bad", C.c_int32), ("reserved", C.c_int32)]


class KeyframeDesc(C.Structure):
    """dsdtm_slam_keyframe_desc"""
    _fields_ = [("map", C.c_void_p), ("T_cur_w", C.c_void_p), ("n_valid", C.c_int32), ("n_cur_points", C.c_int32), ("cur_point", C.c_void_p),
                ("kf", C.c_int32), ("n_local_kf", C.c_int32), ("local_kf", C.c_void_p)]


class SlamError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_slam.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_slam"),
        "dsdtm_slam_map_create": (i, [vp, C.POINTER(vp)]),
        "dsdtm_slam_map_destroy": (None, [vp, vp]),
        "dsdtm_slam_points_write": (i, [vp, vp, i, i, vp, vp, vp]),
        "dsdtm_slam_found_write": (i, [vp, vp, i, vp, vp]),
        "dsdtm_slam_keyframe_add": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, C.POINTER(i)]),
        "dsdtm_slam_keyframe_write": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "dsdtm_slam_map_read": (i, [vp, vp, C.POINTER(track_map.Image)]),
        "dsdtm_slam_local": (i, [vp, C.POINTER(Camera), C.POINTER(Params), i, C.POINTER(track_map.Desc), C.POINTER(track_map.Result)]),
        "dsdtm_slam_covisibility": (i, [vp, i, C.POINTER(ba_window.CovDesc), C.POINTER(ba_window.CovResult)]),
        "dsdtm_slam_ba_window": (i, [vp, i, C.POINTER(ba_window.WindowDesc), C.POINTER(ba_window.WindowArrays), C.POINTER(LocalBaProblem),
                                     C.POINTER(ba_window.WindowResult)]),
        "dsdtm_slam_ba_commit": (i, [vp, i, C.POINTER(ba_window.WindowDesc), C.POINTER(LocalBaProblem), C.POINTER(ba_window.WindowResult),
                                     C.POINTER(ba_window.WindowArrays), vp, vp, i, vp, C.POINTER(ba_window.CommitResult)]),
        "dsdtm_slam_track_commit": (i, [vp, C.c_double, i, C.POINTER(CommitDesc), i, vp, C.POINTER(CommitResult)]),
        "dsdtm_slam_need_keyframes": (i, [vp, C.POINTER(capi.Camera), C.POINTER(capi.KeyframeParams), i, C.POINTER(KeyframeDesc), vp])}, _not_built)


class _SlamNames:
    """The library as track_map's and ba_window's classes address it: dsdtm_trackmap_<entry> and dsdtm_mapping_<entry> are this
    library's dsdtm_slam_<entry> (one implementation each, the same layouts), so track_map.DeviceTrackMap, LocalCall and TrackMapStore,
    ba_window.MappingContext.covisibility and ba_window.WindowCall work on a SlamContext unchanged."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        for prefix in ("dsdtm_trackmap_", "dsdtm_mapping_"):
            if name.startswith(prefix):
                name = "dsdtm_slam_" + name[len(prefix):]
        return getattr(self._lib, name)


class CommitCall:
    """One prepared dsdtm_slam_track_commit call: `frames` is a list of (map, point, residual_norm) — point: the MAP index of every
    match. Descriptors and output arrays are built once, run_raw() is the C call alone. found_after and bad_points are filled with FILL
    bytes before the call: entries the call does not write keep them."""

    def __init__(self, ctx: "SlamContext", outlier_threshold: float, frames, bad_capacity: int | None = None, want_found_after: bool = True):
        self.ctx, self.n, self.threshold = ctx, len(frames), float(outlier_threshold)
        self.descs, self.results = (CommitDesc * max(self.n, 1))(), (CommitResult * max(self.n, 1))()
        C.memset(self.results, FILL, C.sizeof(self.results))
        self.keep = []
        for d, (m, point, norm) in zip(self.descs, frames):
            p = np.ascontiguousarray(np.asarray(point, np.int32).reshape(-1))
            r = np.ascontiguousarray(np.asarray(norm, np.float64).reshape(-1))
            if len(p) != len(r):
                raise ValueError(f"{len(r)} norms for {len(p)} matches")
            fa = _filled(len(p), np.int32) if want_found_after else None
            self.keep.append((p, r, fa))
            d.map, d.n_matches, d.point, d.residual_norm = m.handle, len(p), p.ctypes.data if len(p) else None, r.ctypes.data if len(r) else None
            d.found_after = fa.ctypes.data if fa is not None else None
        self.bad_capacity = max([len(p) for p, _, _ in self.keep] + [0]) if bad_capacity is None else int(bad_capacity)
        self.bad = _filled(max(self.n, 1) * max(self.bad_capacity, 1), np.int32)

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_slam_track_commit(self.ctx.handle, self.threshold, self.n, self.descs, self.bad_capacity, self.bad.ctypes.data, self.results)

    def answers(self) -> list:
        """Per frame: n_erased, n_bad, overflow_bad, bad_points (cut to what was written), found_after (a list, or None), raw (the
        frame's bad_points row whole and found_after whole)."""
        out = []
        for t, (p, _, fa) in enumerate(self.keep):
            r, cap = self.results[t], self.bad_capacity
            row = self.bad[t * cap:(t + 1) * cap]
            out.append(dict(n_erased=r.n_erased, n_bad=r.n_bad, overflow_bad=r.overflow_bad, reserved=r.reserved, bad_points=row[:min(max(r.n_bad, 0), cap)].tolist(),
                            found_after=None if fa is None else fa[:len(p)].tolist(), raw=(row, fa)))
        return out


class KeyframeCall:
    """One prepared dsdtm_slam_need_keyframes call: `trackers` is a list of dicts with map (a DeviceTrackMap), T_cur_w, n_valid,
    cur_point (map indices, feature order), kf (the last keyframe's map index), local_kf (map keyframe indices). The verdicts are
    filled with FILL bytes before the call."""

    def __init__(self, ctx: "SlamContext", cam, params, trackers):
        self.ctx, self.n = ctx, len(trackers)
        self.cam, self.prm = capi.camera_struct(cam), capi.keyframe_params_struct(params)
        self.descs, self.keep = (KeyframeDesc * max(self.n, 1))(), []
        for d, t in zip(self.descs, trackers):
            T = np.ascontiguousarray(np.asarray(t["T_cur_w"], np.float64).reshape(12))
            cur = np.ascontiguousarray(np.asarray(t["cur_point"], np.int32).reshape(-1))
            lk = np.ascontiguousarray(np.asarray(t["local_kf"], np.int32).reshape(-1))
            self.keep.append((T, cur, lk))
            d.map, d.T_cur_w, d.n_valid, d.n_cur_points, d.cur_point = t["map"].handle, T.ctypes.data, int(t["n_valid"]), len(cur), cur.ctypes.data if len(cur) else None
            d.kf, d.n_local_kf, d.local_kf = int(t["kf"]), len(lk), lk.ctypes.data if len(lk) else None
        self.verdicts = np.full(max(1, self.n) * capi.KEYFRAME_VERDICT_DTYPE.itemsize, FILL, np.uint8).view(capi.KEYFRAME_VERDICT_DTYPE)

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_slam_need_keyframes(self.ctx.handle, C.byref(self.cam), C.byref(self.prm), self.n, self.descs, self.verdicts.ctypes.data)

    def answers(self) -> list:
        names = [k for k in capi.KEYFRAME_VERDICT_DTYPE.names if k != "reserved"]
        return [{k: self.verdicts[k][t].item() for k in names} for t in range(self.n)]


def _filled(n, dtype):
    return np.full(max(int(n), 1) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


class SlamContext(ba_window.MappingContext):
    """A dsdtm_slam_ctx: its own stream and staging blocks on one device, serving ONE resident map to the tracker and to the mapping
    thread's entries (everything a ba_window.MappingContext does: new_map, local, covisibility; ba_window.WindowCall takes it as its
    context) and the tracked frame's commit. One per calling thread."""
    PREFIX, ERROR = "dsdtm_slam", SlamError

    @staticmethod
    def load():
        return _SlamNames(load())

    def track_commit(self, outlier_threshold: float, frames, bad_capacity: int | None = None) -> list:
        """dsdtm_slam_track_commit: `frames` is a list of (DeviceTrackMap, point, residual_norm). One submission, synchronous; the
        next call on this context sees the new counts and flags. Returns one dict per frame (CommitCall.answers)."""
        call = CommitCall(self, outlier_threshold, frames, bad_capacity)
        self.check(call.run_raw())
        return call.answers()

    def need_keyframes(self, cam, params, trackers) -> list:
        """dsdtm_slam_need_keyframes: Tracking::NeedKeyframe on the resident map for len(trackers) trackers in one submission
        (KeyframeCall's dicts). Returns one verdict dict per tracker, as capi.need_keyframes does."""
        call = KeyframeCall(self, cam, params, trackers)
        self.check(call.run_raw())
        return call.answers()


def outlier_threshold(cam) -> float:
    """tOutlineThres of Optimizer::PoseOptimization (src/Optimizer.cpp:22-24) as tracking.apply_tracked_frame computes it."""
    from .frame import Config
    return float(np.float32(Config.Get("Optimization.LocalBAthreshhold"))) / float(np.float32(cam.f))


def commit_tracked_frames(ctx: SlamContext, cam, stores, results, point_lists, threshold: float | None = None) -> list:
    """The commit of n tracked frames in ONE call: results[i] is sequence i's track_frame / track_frames result, point_lists[i] the
    `point` list its store's local() returned (r["point"]: the map index of every local map point, in the order the tracker saw them).
    The objects are not touched here: tracking.apply_tracked_frame has applied the same rules to them (the keyframe side of
    SetBadFlag, which it leaves out, is the caller's: bad_points names the points). A lost frame commits nothing; a match without a
    residual block (none today: every feature of a tracked frame has one) is committed with a NaN norm, which erases nothing. Returns
    the answers, each with `points` (the map index of every match)."""
    frames = []
    for s, r, pl in zip(stores, results, point_lists):
        pts = [] if r["lost"] else [int(pl[int(i)]) for i in r["matches"]["point"]]
        norm = np.full(len(pts), np.nan)
        if pts:
            rn = np.asarray(r["residual_norm"], np.float64)[:len(pts)]
            norm[:len(rn)] = rn
        frames.append((s.map, pts, norm))
    out = ctx.track_commit(outlier_threshold(cam) if threshold is None else threshold, frames)
    for (_, pts, _), a in zip(frames, out):
        a["points"] = pts
    return out
