"""libdsdtm_amd_mapping.so (include/dsdtm_amd_mapping.h) from Python: the resident track map served to the mapping thread, the
covisibility list of KeyFrame::UpdateConnection, the window of Optimizer::LocalBundleAdjustment in the layout
dsdtm_local_ba_batch_device takes, and the commit of its solve. Restated in ba_window_restatement.py.

    ctx = MappingContext()                   # one per calling thread
    m = ctx.new_map()                        # a track_map.DeviceTrackMap served by this library: points_write, keyframe_add, read ...
    cov = ctx.covisibility([(m, kf, 64)])
    call = WindowCall(ctx, [(m, kf, cov[0]["cov_kf"], origin_kf, 80, 4096, 32768)])      # device arrays come from torch
    call.run(); ...solve on call.tensors...; call.commit(outlier_tensor, stream)

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon, track_map
from .capi import LocalBaProblem
from .local_map import Camera, Params

LIB_NAME = "libdsdtm_amd_mapping.so"
# every symbol include/dsdtm_amd_mapping.h declares
MAP_SYMBOLS = ["dsdtm_mapping_" + s[len("dsdtm_trackmap_"):] for s in track_map.SYMBOLS]
SYMBOLS = MAP_SYMBOLS + ["dsdtm_mapping_covisibility", "dsdtm_mapping_ba_window", "dsdtm_mapping_ba_commit"]
COV_THRESHOLD, MAX_PAIRS, MAX_WINDOWS, MAX_COV = 15, 1024, 256, 255
FILL = 0xA5
RESULT_FIELDS = ("n_local", "n_fixed", "n_points", "n_obs", "over_free_kf", "over_const_kf", "over_points", "over_obs", "over_keyframe_capacity",
                 "over_point_capacity", "over_observation_capacity", "usable")
# the device arrays of a window call: name, dtype, columns, which capacity sizes it
DEVICE_ARRAYS = (("T_c2w", np.float64, 12, "kf"), ("kf_constant", np.uint8, 1, "kf"), ("points", np.float64, 3, "point"), ("obs_kf", np.int32, 1, "obs"),
                 ("obs_point", np.int32, 1, "obs"), ("obs_bearing", np.float64, 3, "obs"), ("obs_level", np.int32, 1, "obs"), ("kf_index", np.int32, 1, "kf"),
                 ("point_index", np.int32, 1, "point"), ("obs_slot", np.int64, 1, "obs"))


class CovDesc(C.Structure):
    """dsdtm_mapping_cov_desc"""
    _fields_ = [("map", C.c_void_p), ("kf", C.c_int32), ("capacity", C.c_int32), ("cov_kf", C.c_void_p), ("cov_weight", C.c_void_p)]


class CovResult(C.Structure):
    """dsdtm_mapping_cov_result"""
    _fields_ = [("n_cov", C.c_int32), ("n_connected", C.c_int32), ("overflow", C.c_int32), ("reserved", C.c_int32)]


class WindowDesc(C.Structure):
    """dsdtm_mapping_window_desc"""
    _fields_ = [("map", C.c_void_p), ("kf", C.c_int32), ("n_cov", C.c_int32), ("cov_kf", C.c_void_p), ("origin_kf", C.c_int32),
                ("keyframe_capacity", C.c_int32), ("point_capacity", C.c_int32), ("observation_capacity", C.c_int32)]


class WindowArrays(C.Structure):
    """dsdtm_mapping_window_arrays"""
    _fields_ = [(name, C.c_void_p) for name, _, _, _ in DEVICE_ARRAYS] + [("h_kf_index", C.c_void_p), ("h_point_index", C.c_void_p), ("h_obs_slot", C.c_void_p)]


class WindowResult(C.Structure):
    """dsdtm_mapping_window_result"""
    _fields_ = [(f, C.c_int32) for f in RESULT_FIELDS]


class CommitResult(C.Structure):
    """dsdtm_mapping_commit_result"""
    _fields_ = [("n_outliers", C.c_int32), ("n_bad", C.c_int32), ("overflow_bad", C.c_int32), ("reserved", C.c_int32)]


class MappingError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_mapping.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_mapping"),
        "dsdtm_mapping_map_create": (i, [vp, C.POINTER(vp)]),
        "dsdtm_mapping_map_destroy": (None, [vp, vp]),
        "dsdtm_mapping_points_write": (i, [vp, vp, i, i, vp, vp, vp]),
        "dsdtm_mapping_found_write": (i, [vp, vp, i, vp, vp]),
        "dsdtm_mapping_keyframe_add": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, C.POINTER(i)]),
        "dsdtm_mapping_keyframe_write": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "dsdtm_mapping_map_read": (i, [vp, vp, C.POINTER(track_map.Image)]),
        "dsdtm_mapping_local": (i, [vp, C.POINTER(Camera), C.POINTER(Params), i, C.POINTER(track_map.Desc), C.POINTER(track_map.Result)]),
        "dsdtm_mapping_covisibility": (i, [vp, i, C.POINTER(CovDesc), C.POINTER(CovResult)]),
        "dsdtm_mapping_ba_window": (i, [vp, i, C.POINTER(WindowDesc), C.POINTER(WindowArrays), C.POINTER(LocalBaProblem), C.POINTER(WindowResult)]),
        "dsdtm_mapping_ba_commit": (i, [vp, i, C.POINTER(WindowDesc), C.POINTER(LocalBaProblem), C.POINTER(WindowResult), C.POINTER(WindowArrays), vp, vp, i, vp,
                                        C.POINTER(CommitResult)])}, _not_built)


class _MapNames:
    """The library as track_map's classes address it: dsdtm_trackmap_<entry> is this library's dsdtm_mapping_<entry> (one implementation,
    the same layouts), so track_map.DeviceTrackMap, LocalCall and TrackMapStore work on a MappingContext unchanged."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name.replace("dsdtm_trackmap_", "dsdtm_mapping_", 1))


def _filled(n, dtype):
    return np.full(max(int(n), 1) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


class MappingContext(_addon.AddonContext):
    """A dsdtm_mapping_ctx: its own stream and staging blocks on one device. One per calling thread."""
    PREFIX, ERROR = "dsdtm_mapping", MappingError

    @staticmethod
    def load():
        return _MapNames(load())

    def new_map(self) -> track_map.DeviceTrackMap:
        return track_map.DeviceTrackMap(self)

    def local(self, cam, queries, n_local: int = 10, boundary: int = 0) -> list:
        """dsdtm_mapping_local: as track_map.TrackMapContext.local."""
        call = track_map.LocalCall(self, cam, queries, n_local, boundary)
        self.check(call.run_raw())
        return call.answers()

    def covisibility(self, pairs) -> list:
        """dsdtm_mapping_covisibility: `pairs` is a list of (map, kf, capacity). One dict per pair: cov_kf, cov_weight (cut to what was
        written), n_cov, n_connected, overflow, raw (the two arrays whole: entries the call did not write hold FILL bytes)."""
        n = len(pairs)
        descs, results, keep = (CovDesc * max(n, 1))(), (CovResult * max(n, 1))(), []
        for d, (m, kf, cap) in zip(descs, pairs):
            a, b = _filled(cap, np.int32), _filled(cap, np.int32)
            keep.append((a, b))
            d.map, d.kf, d.capacity, d.cov_kf, d.cov_weight = m.handle, int(kf), int(cap), a.ctypes.data, b.ctypes.data
        self.check(self.lib.dsdtm_mapping_covisibility(self.handle, n, descs, results))
        out = []
        for (a, b), (_, _, cap), r in zip(keep, pairs, results):
            m = min(r.n_cov, cap)
            out.append(dict(cov_kf=a[:m].tolist(), cov_weight=b[:m].tolist(), n_cov=r.n_cov, n_connected=r.n_connected, overflow=r.overflow, raw=(a, b)))
        return out


class WindowCall:
    """One dsdtm_mapping_ba_window call and the dsdtm_mapping_ba_commit that follows it. `windows` is a list of
    (map, kf, cov_kf, origin_kf, keyframe_capacity, point_capacity, observation_capacity). The device arrays are torch tensors
    (self.tensors, by the names of dsdtm_mapping_window_arrays), filled with FILL bytes before the call."""

    def __init__(self, ctx: MappingContext, windows, device: str = "cuda:0"):
        import torch
        self.ctx, self.n, self.windows = ctx, len(windows), windows
        self.descs, self.problems, self.results = (WindowDesc * max(self.n, 1))(), (LocalBaProblem * max(self.n, 1))(), (WindowResult * max(self.n, 1))()
        self.keep = []
        total = dict(kf=0, point=0, obs=0)
        self.offsets = []
        for d, (m, kf, cov, origin, kcap, pcap, ocap) in zip(self.descs, windows):
            cov = np.ascontiguousarray(np.asarray(cov, np.int32).reshape(-1))
            self.keep.append(cov)
            d.map, d.kf, d.n_cov, d.cov_kf, d.origin_kf = m.handle, int(kf), len(cov), cov.ctypes.data if len(cov) else None, int(origin)
            d.keyframe_capacity, d.point_capacity, d.observation_capacity = int(kcap), int(pcap), int(ocap)
            self.offsets.append(dict(total))
            total["kf"] += int(kcap); total["point"] += int(pcap); total["obs"] += int(ocap)
        self.total = total
        self.tensors, self.arrays = {}, WindowArrays()
        for name, dt, width, by in DEVICE_ARRAYS:
            t = torch.full((max(total[by], 1) * width * np.dtype(dt).itemsize,), FILL, dtype=torch.uint8, device=device)
            self.tensors[name] = t
            setattr(self.arrays, name, t.data_ptr())
        self.host = dict(h_kf_index=_filled(total["kf"], np.int32), h_point_index=_filled(total["point"], np.int32), h_obs_slot=_filled(total["obs"], np.int64))
        for name, a in self.host.items():
            setattr(self.arrays, name, a.ctypes.data)
        torch.cuda.synchronize()

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_mapping_ba_window(self.ctx.handle, self.n, self.descs, C.byref(self.arrays), self.problems, self.results)

    def run(self) -> list:
        self.ctx.check(self.run_raw())
        return self.answers()

    def column(self, name) -> np.ndarray:
        """A device array whole, on the host, as (rows, columns)."""
        dt, width = {n: (d, w) for n, d, w, _ in DEVICE_ARRAYS}[name]
        return self.tensors[name].cpu().numpy().view(dt).reshape(-1, width)

    def answers(self) -> list:
        """Per window: the result's fields, `problem` (counts and offsets) and, when usable, its segment of every array (copies), plus
        the host copies of the three index arrays under h_kf_index, h_point_index, h_obs_slot."""
        cols = {name: self.column(name) for name, _, _, _ in DEVICE_ARRAYS}
        out = []
        for w in range(self.n):
            r, p, at = self.results[w], self.problems[w], self.offsets[w]
            a = {f: getattr(r, f) for f in RESULT_FIELDS}
            a["problem"] = dict(n_keyframes=p.n_keyframes, n_points=p.n_points, n_observations=p.n_observations, keyframe_offset=p.keyframe_offset,
                                point_offset=p.point_offset, observation_offset=p.observation_offset)
            if r.usable:
                cnt = dict(kf=r.n_local + r.n_fixed, point=r.n_points, obs=r.n_obs)
                for name, _, width, by in DEVICE_ARRAYS:
                    seg = cols[name][at[by]:at[by] + cnt[by]].copy()
                    a[name] = seg if width > 1 else seg.reshape(-1)
                for name, by in (("h_kf_index", "kf"), ("h_point_index", "point"), ("h_obs_slot", "obs")):
                    a[name] = self.host[name][at[by]:at[by] + cnt[by]].copy()
            out.append(a)
        return out

    def commit(self, outlier, hip_stream=None, bad_capacity: int = 64):
        """dsdtm_mapping_ba_commit on this call's windows; `outlier` is a torch uint8 tensor over the observation segments. Returns the
        status and one dict per window (n_outliers, n_bad, overflow_bad, bad_points)."""
        bad = _filled(max(self.n, 1) * max(bad_capacity, 1), np.int32)
        res = (CommitResult * max(self.n, 1))()
        st = self.ctx.lib.dsdtm_mapping_ba_commit(self.ctx.handle, self.n, self.descs, self.problems, self.results, C.byref(self.arrays), outlier.data_ptr(),
                                                  hip_stream, int(bad_capacity), bad.ctypes.data, res)
        out = [dict(n_outliers=r.n_outliers, n_bad=r.n_bad, overflow_bad=r.overflow_bad,
                    bad_points=bad[w * bad_capacity:w * bad_capacity + min(r.n_bad, bad_capacity)].tolist()) for w, r in zip(range(self.n), res)]
        return st, out
