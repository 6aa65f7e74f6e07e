"""ctypes binding of the C ABI in include/dsdtm_amd.h (the drop-in boundary).

The shared library is built in-tree by `dsdtm_amd/csrc/build.py` (hipcc, gfx950) and is
the ONLY compute path: there is no CPU fallback. Loading fails loudly when the library
is missing; compute calls fail with DSDTM_ERR_NO_DEVICE when no MI355X is visible.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _addon

MAX_LEVELS = 8
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4

u8p = C.POINTER(C.c_uint8)


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("f", C.c_float), ("width", C.c_int), ("height", C.c_int)]


class Pyramid(C.Structure):
    _fields_ = [("levels", C.c_int), ("data", C.c_void_p * MAX_LEVELS),
                ("width", C.c_int * MAX_LEVELS), ("height", C.c_int * MAX_LEVELS),
                ("stride", C.c_int * MAX_LEVELS)]


class AlignParams(C.Structure):
    _fields_ = [("max_level", C.c_int), ("min_level", C.c_int), ("max_iters", C.c_int),
                ("min_fts", C.c_int)]


class AlignStats(C.Structure):
    _fields_ = [("iters", C.c_int32 * MAX_LEVELS), ("n_ref", C.c_int32 * MAX_LEVELS),
                ("n_vis", C.c_int32 * MAX_LEVELS), ("exit_code", C.c_int32 * MAX_LEVELS),
                ("chi2", C.c_double * MAX_LEVELS)]

    def as_dict(self):
        return {k: list(getattr(self, k)) for k, _ in self._fields_}


STATS_DTYPE = np.dtype([("iters", "<i4", MAX_LEVELS), ("n_ref", "<i4", MAX_LEVELS),
                        ("n_vis", "<i4", MAX_LEVELS), ("exit_code", "<i4", MAX_LEVELS),
                        ("chi2", "<f8", MAX_LEVELS)])
assert STATS_DTYPE.itemsize == C.sizeof(AlignStats)


class BatchDesc(C.Structure):
    _fields_ = [("n_pairs", C.c_int), ("max_features", C.c_int), ("levels", C.c_int),
                ("width", C.c_int * MAX_LEVELS), ("height", C.c_int * MAX_LEVELS),
                ("stride", C.c_int * MAX_LEVELS), ("level_offset", C.c_size_t * MAX_LEVELS),
                ("pyr_pitch", C.c_size_t),
                ("ref_pyr", C.c_void_p), ("cur_pyr", C.c_void_p), ("px_xy", C.c_void_p),
                ("bearing", C.c_void_p), ("p_world", C.c_void_p), ("initial", C.c_void_p),
                ("n_features", C.c_void_p), ("T_ref_w", C.c_void_p), ("T_cur_w", C.c_void_p),
                ("n_tracked", C.c_void_p), ("stats", C.c_void_p)]


class StreamDesc(C.Structure):
    """dsdtm_stream_desc: a host sequence of level-0 images + feature columns for dsdtm_sparse_align_batch_streamed."""
    _fields_ = [("n_pairs", C.c_int32), ("max_features", C.c_int32), ("levels", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("row_stride", C.c_int32), ("image_pitch", C.c_size_t),
                ("ref_image", C.c_void_p), ("cur_image", C.c_void_p), ("px_xy", C.c_void_p),
                ("bearing", C.c_void_p), ("p_world", C.c_void_p), ("initial", C.c_void_p),
                ("n_features", C.c_void_p), ("T_ref_w", C.c_void_p), ("T_cur_w", C.c_void_p),
                ("n_tracked", C.c_void_p), ("stats", C.c_void_p)]


class ImageDesc(C.Structure):
    _fields_ = [("levels", C.c_int), ("width", C.c_int * MAX_LEVELS),
                ("height", C.c_int * MAX_LEVELS), ("stride", C.c_int * MAX_LEVELS),
                ("level_offset", C.c_size_t * MAX_LEVELS), ("bytes", C.c_size_t),
                ("data", C.c_void_p)]


def camera_struct(cam) -> Camera:
    return Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.f, cam.width, cam.height)


def pyramid_struct(levels) -> tuple[Pyramid, list]:
    """levels: list of 2-D uint8 arrays (rows may be strided). Returns (struct, keepalive)."""
    p = Pyramid()
    p.levels = len(levels)
    keep = []
    for i, a in enumerate(levels):
        if a.dtype != np.uint8 or a.ndim != 2 or a.strides[1] != 1:
            a = np.ascontiguousarray(a, dtype=np.uint8)
        keep.append(a)
        p.data[i] = a.ctypes.data
        p.width[i] = a.shape[1]
        p.height[i] = a.shape[0]
        p.stride[i] = a.strides[0]
    return p, keep


def pyramid_layout(width: int, height: int, levels: int, align: int = 64):
    """Packed-pyramid geometry used by the *_device entry points: per level
    (w, h, stride=w, offset); offsets aligned to `align` bytes, pitch too."""
    ws, hs, offs = [], [], []
    off = 0
    w, h = width, height
    for _ in range(levels):
        ws.append(w)
        hs.append(h)
        offs.append(off)
        off += (w * h + align - 1) // align * align
        w, h = (w + 1) // 2, (h + 1) // 2
    return ws, hs, list(ws), offs, off


def declare_signatures(lib, prefix: str, with_ctx: bool):
    """Attach argtypes for the entry points shared by the product library (prefix 'dsdtm_',
    ctx first) and the oracle (prefix 'oracle_', no ctx)."""
    ctx = [C.c_void_p] if with_ctx else []
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f = getattr(lib, prefix + "sparse_align")
    f.restype = C.c_int
    f.argtypes = ctx + [C.POINTER(Pyramid), C.POINTER(Pyramid), C.POINTER(Camera), fp, dp, dp, u8p,
                        C.c_int, dp, dp, C.POINTER(AlignParams), C.POINTER(C.c_int),
                        C.POINTER(AlignStats)]
    f = getattr(lib, prefix + "align2d_batch")
    f.restype = C.c_int
    f.argtypes = ctx + [C.POINTER(Pyramid), u8p, u8p, ip, dp, u8p, C.c_int, C.c_int]
    f = getattr(lib, prefix + "warp_patches")
    f.restype = C.c_int
    f.argtypes = ctx + [C.POINTER(Pyramid), C.c_int, C.POINTER(Camera), dp, dp, ip, fp, ip, dp, dp,
                        C.c_int, C.c_int, dp, ip, u8p, u8p]


# every symbol include/dsdtm_amd.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "dsdtm_create", "dsdtm_destroy", "dsdtm_last_error", "dsdtm_version", "dsdtm_device_count",
    "dsdtm_sparse_align", "dsdtm_sparse_align_batch_device", "dsdtm_sparse_align_check", "dsdtm_sparse_align_workspace_bytes",
    "dsdtm_reserve", "dsdtm_align2d_batch", "dsdtm_align2d_batch_device",
    "dsdtm_pyrdown_batch_device", "dsdtm_pyrdown", "dsdtm_warp_patches",
    "dsdtm_frame_create", "dsdtm_frame_create_from_image", "dsdtm_frame_destroy", "dsdtm_sparse_align_frames",
    "dsdtm_detect_cells", "dsdtm_detect_cells_frame", "dsdtm_match_candidates_frames",
    "dsdtm_pose_optimization", "dsdtm_pose_optimization_batch_device",
    "dsdtm_sparse_align_batch_sharded", "dsdtm_sparse_align_batch_streamed", "dsdtm_shard_range", "dsdtm_detect_cells_batch_device",
    "dsdtm_match_candidates_batch_device", "dsdtm_match_candidates_scratch_bytes", "dsdtm_track_frame",
    "dsdtm_track_frames", "dsdtm_local_ba", "dsdtm_local_ba_batch_device",
    "dsdtm_frame_prefetch", "dsdtm_frame_wait", "dsdtm_track_frame_on", "dsdtm_frame_lift",
]
# every symbol include/dsdtm_amd_keyframe.h declares: the add-on library (Tracking::NeedKeyframe for n trackers), loaded on first use
KEYFRAME_SYMBOLS = ["dsdtm_keyframe_create", "dsdtm_keyframe_destroy", "dsdtm_keyframe_last_error", "dsdtm_need_keyframe",
                    "dsdtm_need_keyframes"]
KEYFRAME_LIB_NAME = "libdsdtm_amd_keyframe.so"


class DetectParams(C.Structure):
    _fields_ = [("cell_size", C.c_int32), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("levels", C.c_int32),
                ("barrier", C.c_int32), ("detection_threshold", C.c_float)]


class PoseOptParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class PoseOptSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("successful_steps", C.c_int32), ("termination", C.c_int32),
                ("n_residual_blocks", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("x", C.c_double * 6)]

    def as_dict(self):
        return dict(iterations=self.iterations, successful_steps=self.successful_steps, termination=self.termination,
                    n_residual_blocks=self.n_residual_blocks, initial_cost=self.initial_cost,
                    final_cost=self.final_cost, x=np.array(list(self.x)))


class LocalBaParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved", C.c_int32), ("delta", C.c_double)]


class LocalBaSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("successful_steps", C.c_int32), ("termination", C.c_int32),
                ("n_residual_blocks", C.c_int32), ("n_outliers", C.c_int32), ("n_free_keyframes", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


LBA_SUMMARY_DTYPE = np.dtype([("iterations", "<i4"), ("successful_steps", "<i4"), ("termination", "<i4"),
                              ("n_residual_blocks", "<i4"), ("n_outliers", "<i4"), ("n_free_keyframes", "<i4"),
                              ("initial_cost", "<f8"), ("final_cost", "<f8")])
assert LBA_SUMMARY_DTYPE.itemsize == C.sizeof(LocalBaSummary)


class LocalBaProblem(C.Structure):
    _fields_ = [("n_keyframes", C.c_int32), ("n_points", C.c_int32), ("n_observations", C.c_int32), ("reserved", C.c_int32),
                ("keyframe_offset", C.c_int64), ("point_offset", C.c_int64), ("observation_offset", C.c_int64)]


LBA_MAX_FREE_KF, LBA_MAX_CONST_KF, LBA_MAX_POINTS, LBA_MAX_OBSERVATIONS = 16, 64, 16384, 131072


class TrackDesc(C.Structure):
    """dsdtm_track_desc: one tracked frame (new image, Run against the last frame, the local map) for dsdtm_track_frame."""
    _fields_ = [("image", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("levels", C.c_int32),
                ("ref", C.c_void_p), ("ref_px_xy", C.c_void_p), ("ref_bearing", C.c_void_p), ("ref_p_world", C.c_void_p),
                ("ref_initial", C.c_void_p), ("n_ref_features", C.c_int32), ("T_ref_w", C.c_void_p), ("T_seed", C.c_void_p),
                ("align", AlignParams), ("min_tracked", C.c_int32),
                ("kf", C.c_void_p), ("n_kf", C.c_int32), ("T_kf_w", C.c_void_p), ("n_points", C.c_int32),
                ("mp_world", C.c_void_p), ("mp_found", C.c_void_p), ("mp_bad", C.c_void_p), ("obs_offset", C.c_void_p),
                ("obs_kf", C.c_void_p), ("obs_px", C.c_void_p), ("obs_level", C.c_void_p), ("obs_bearing", C.c_void_p),
                ("mask", C.c_void_p), ("mask_stride", C.c_int32), ("cell_size", C.c_int32), ("max_pyr_levels", C.c_int32),
                ("max_matches", C.c_int32), ("align2d_iters", C.c_int32), ("pose_opt", PoseOptParams)]


class FrameImage(C.Structure):
    """dsdtm_frame_image: what a frame is constructed from (gray image, optional 16-bit depth map) for dsdtm_frame_prefetch."""
    _fields_ = [("gray", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("levels", C.c_int32),
                ("depth", C.c_void_p), ("depth_stride", C.c_int32), ("depth_scale", C.c_float)]


LIFT_MAX = 16384
KF_MAX_POINTS, KF_MAX_LOCAL_KF, TRACK_FRAMES_MAX = 4096, 64, 1024


class KeyframeParams(C.Structure):
    """dsdtm_keyframe_params: the thresholds of Tracking::NeedKeyframe (src/Tracking.cpp:347-410)."""
    _fields_ = [("min_valid", C.c_int32), ("max_valid", C.c_int32), ("px_samples", C.c_int32), ("reserved", C.c_int32),
                ("min_px_median", C.c_double), ("min_rot", C.c_double), ("min_trans", C.c_double)]


class KeyframeDesc(C.Structure):
    """dsdtm_keyframe_desc: one tracker's inputs of dsdtm_need_keyframes."""
    _fields_ = [("T_cur_w", C.c_void_p), ("T_kf_w", C.c_void_p), ("n_valid", C.c_int32),
                ("n_cur_points", C.c_int32), ("cur_p_world", C.c_void_p), ("cur_bad", C.c_void_p),
                ("n_kf_points", C.c_int32), ("kf_p_world", C.c_void_p), ("kf_bad", C.c_void_p),
                ("n_local_kf", C.c_int32), ("local_kf_centre", C.c_void_p)]


class KeyframeVerdict(C.Structure):
    _fields_ = [("need", C.c_int32), ("reason", C.c_int32), ("rule_mask", C.c_int32), ("undefined", C.c_int32),
                ("n_px", C.c_int32), ("n_depth", C.c_int32), ("svo_kf", C.c_int32), ("reserved", C.c_int32),
                ("median_px", C.c_double), ("rot", C.c_double), ("trans", C.c_double),
                ("min_depth", C.c_double), ("median_depth", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


KEYFRAME_VERDICT_DTYPE = np.dtype([("need", "<i4"), ("reason", "<i4"), ("rule_mask", "<i4"), ("undefined", "<i4"),
                                   ("n_px", "<i4"), ("n_depth", "<i4"), ("svo_kf", "<i4"), ("reserved", "<i4"),
                                   ("median_px", "<f8"), ("rot", "<f8"), ("trans", "<f8"), ("min_depth", "<f8"),
                                   ("median_depth", "<f8")])
assert KEYFRAME_VERDICT_DTYPE.itemsize == C.sizeof(KeyframeVerdict)


class TrackMatch(C.Structure):
    _fields_ = [("cell", C.c_int32), ("point", C.c_int32), ("px", C.c_float * 2), ("level", C.c_int32)]


TRACK_MATCH_DTYPE = np.dtype([("cell", "<i4"), ("point", "<i4"), ("px", "<f4", 2), ("level", "<i4")])
assert TRACK_MATCH_DTYPE.itemsize == C.sizeof(TrackMatch)


class TrackResult(C.Structure):
    _fields_ = [("frame", C.c_void_p), ("T_run", C.c_double * 12), ("n_tracked", C.c_int32), ("lost", C.c_int32),
                ("stats", AlignStats), ("n_in_grid", C.c_int32), ("n_matches", C.c_int32), ("replay_full_scan", C.c_int32), ("reserved", C.c_int32),
                ("T_opt", C.c_double * 12),
                ("summary", PoseOptSummary)]


# dsdtm_pose_opt_termination
PO_FUNCTION_TOLERANCE, PO_PARAMETER_TOLERANCE, PO_GRADIENT_TOLERANCE, PO_MAX_ITERATIONS = 0, 1, 2, 3
PO_MIN_RADIUS, PO_INVALID_STEPS, PO_NO_RESIDUALS, PO_EVALUATION_FAILED = 4, 5, 6, 7

_LIBS = {}
LIB_NAME = "libdsdtm_amd.so"             # the release library: the product (exactly the header's symbols, no switches)
DIAG_LIB_NAME = "libdsdtm_amd_diag.so"   # the diagnostic build (build.py --diag): + dsdtm_debug_*, environment switches


def lib_path(diag: bool | None = False) -> str:
    diag = _DIAG_DEFAULT if diag is None else bool(diag)
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", DIAG_LIB_NAME if diag else LIB_NAME)


class DsdtmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"dsdtm_amd status {status}: {msg}")
        self.status = status


# Which library a Context is created from when the caller does not say: the release one. tools/ (A/B scripts that set
# DSDTM_* switches in the environment — only the diagnostic library reads them) export DSDTM_PY_DIAG=1; tests use
# `with capi.diag_default():`. This is the PYTHON binding's choice of file; the release library itself reads no environment.
_DIAG_DEFAULT = os.environ.get("DSDTM_PY_DIAG") == "1"


class diag_default:
    """`with capi.diag_default(): ...` — contexts created inside the block without an explicit `diag=` come from the
    diagnostic library (for code that builds its own Context, e.g. tools/ modules driven by a `diag` test)."""

    def __init__(self, flag: bool = True):
        self.flag = bool(flag)

    def __enter__(self):
        global _DIAG_DEFAULT
        self.old, _DIAG_DEFAULT = _DIAG_DEFAULT, self.flag
        return self

    def __exit__(self, *exc):
        global _DIAG_DEFAULT
        _DIAG_DEFAULT = self.old
        return False


def load(diag: bool | None = None):
    """Load libdsdtm_amd.so — or, diag=True, the diagnostic build beside it (tools/ and the tests marked `diag`: fault
    injection and A/B switches the release library does not have). No fallback: raises if it has not been built."""
    diag = _DIAG_DEFAULT if diag is None else bool(diag)
    if diag in _LIBS:
        return _LIBS[diag]
    path = lib_path(diag)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "dsdtm_amd has no CPU fallback.")
    lib = C.CDLL(path)
    declare_signatures(lib, "dsdtm_", with_ctx=True)
    lib.dsdtm_create.restype = C.c_int
    lib.dsdtm_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.dsdtm_destroy.restype = None
    lib.dsdtm_destroy.argtypes = [C.c_void_p]
    lib.dsdtm_last_error.restype = C.c_char_p
    lib.dsdtm_last_error.argtypes = [C.c_void_p]
    lib.dsdtm_version.restype = C.c_char_p
    lib.dsdtm_device_count.restype = C.c_int
    lib.dsdtm_sparse_align_batch_device.restype = C.c_int
    lib.dsdtm_sparse_align_batch_device.argtypes = [C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Camera),
                                                    C.POINTER(AlignParams), C.c_void_p]
    lib.dsdtm_sparse_align_check.restype = C.c_int
    lib.dsdtm_sparse_align_check.argtypes = [C.c_void_p, C.c_void_p]
    lib.dsdtm_sparse_align_workspace_bytes.restype = C.c_size_t
    lib.dsdtm_sparse_align_workspace_bytes.argtypes = [C.POINTER(BatchDesc)]
    lib.dsdtm_reserve.restype = C.c_int
    lib.dsdtm_reserve.argtypes = [C.c_void_p, C.c_size_t]
    lib.dsdtm_align2d_batch_device.restype = C.c_int
    lib.dsdtm_align2d_batch_device.argtypes = [C.c_void_p, C.POINTER(ImageDesc), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p]
    lib.dsdtm_pyrdown_batch_device.restype = C.c_int
    lib.dsdtm_pyrdown_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                               C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.POINTER(C.c_size_t), C.c_void_p]
    lib.dsdtm_pyrdown.restype = C.c_int
    lib.dsdtm_pyrdown.argtypes = [C.c_void_p, u8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    lib.dsdtm_frame_create.restype = C.c_int
    lib.dsdtm_frame_create.argtypes = [C.c_void_p, C.POINTER(Pyramid), C.POINTER(C.c_void_p)]
    lib.dsdtm_frame_create_from_image.restype = C.c_int
    lib.dsdtm_frame_create_from_image.argtypes = [C.c_void_p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.dsdtm_frame_destroy.restype = None
    lib.dsdtm_frame_destroy.argtypes = [C.c_void_p, C.c_void_p]
    lib.dsdtm_sparse_align_frames.restype = C.c_int
    lib.dsdtm_sparse_align_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Camera), fp, dp, dp, u8p, C.c_int,
                                              dp, dp, C.POINTER(AlignParams), C.POINTER(C.c_int), C.POINTER(AlignStats)]
    ip32 = C.POINTER(C.c_int32)
    lib.dsdtm_detect_cells.restype = C.c_int
    lib.dsdtm_detect_cells.argtypes = [C.c_void_p, C.POINTER(Pyramid), u8p, C.POINTER(DetectParams), fp, ip32, ip32, ip32]
    lib.dsdtm_detect_cells_frame.restype = C.c_int
    lib.dsdtm_detect_cells_frame.argtypes = [C.c_void_p, C.c_void_p, u8p, C.POINTER(DetectParams), fp, ip32, ip32, ip32]
    lib.dsdtm_match_candidates_batch_device.restype = C.c_int
    lib.dsdtm_match_candidates_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_int,
                                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                                        C.POINTER(Camera)] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.dsdtm_match_candidates_scratch_bytes.restype = C.c_size_t
    lib.dsdtm_match_candidates_scratch_bytes.argtypes = [C.c_int]
    lib.dsdtm_detect_cells_batch_device.restype = C.c_int
    lib.dsdtm_detect_cells_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.c_void_p,
                                                    C.POINTER(DetectParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dsdtm_match_candidates_frames.restype = C.c_int
    lib.dsdtm_match_candidates_frames.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(Camera), dp, dp,
                                                  ip32, fp, ip32, dp, dp, C.c_int, C.c_int, C.c_int, dp, ip32, u8p]
    lib.dsdtm_sparse_align_batch_sharded.restype = C.c_int
    lib.dsdtm_sparse_align_batch_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(BatchDesc), C.POINTER(Camera),
                                                     C.POINTER(AlignParams)]
    lib.dsdtm_sparse_align_batch_streamed.restype = C.c_int
    lib.dsdtm_sparse_align_batch_streamed.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(StreamDesc), C.c_int, C.POINTER(Camera),
                                                      C.POINTER(AlignParams)]
    lib.dsdtm_track_frame.restype = C.c_int
    lib.dsdtm_track_frame.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(TrackDesc), C.POINTER(TrackResult), C.c_void_p, C.c_void_p]
    lib.dsdtm_track_frames.restype = C.c_int
    lib.dsdtm_track_frames.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.POINTER(TrackDesc), C.POINTER(TrackResult), C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    lib.dsdtm_frame_prefetch.restype = C.c_int
    lib.dsdtm_frame_prefetch.argtypes = [C.c_void_p, C.POINTER(FrameImage), C.POINTER(C.c_void_p)]
    lib.dsdtm_frame_wait.restype = C.c_int
    lib.dsdtm_frame_wait.argtypes = [C.c_void_p, C.c_void_p]
    lib.dsdtm_track_frame_on.restype = C.c_int
    lib.dsdtm_track_frame_on.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(TrackDesc), C.c_void_p, C.POINTER(TrackResult),
                                         C.c_void_p, C.c_void_p]
    lib.dsdtm_frame_lift.restype = C.c_int
    lib.dsdtm_frame_lift.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.dsdtm_shard_range.restype = None
    lib.dsdtm_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if diag:
        lib.dsdtm_debug_set_option.restype = C.c_int
        lib.dsdtm_debug_set_option.argtypes = [C.c_char_p, C.c_int]
        lib.dsdtm_debug_get_option.restype = C.c_int
        lib.dsdtm_debug_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    _LIBS[diag] = lib
    return lib


class debug_options:
    """`with capi.debug_options(no_team=1): ...` — diagnostic switches of the DIAGNOSTIC library (kernels.h: Options) for
    the duration of a block; they act on contexts of that library only (Context(device, diag=True)). The release library
    has no switches. The diagnostic library reads the environment once, when its first context is created; tests and A/B
    tools change a switch afterwards through this."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        lib = load(diag=True)
        for k, v in self.kv.items():
            cur = C.c_int()
            if lib.dsdtm_debug_get_option(k.encode(), C.byref(cur)) != OK:
                raise KeyError(k)
            self.old[k] = cur.value
            lib.dsdtm_debug_set_option(k.encode(), int(v))
        return self

    def __exit__(self, *exc):
        lib = load(diag=True)
        for k, v in self.old.items():
            lib.dsdtm_debug_set_option(k.encode(), v)
        return False


def track_frames(ctx, cam, n, descs, results, matches, residual_norm, in_grid, frames=None) -> int:
    """dsdtm_track_frames; returns its status. `descs` / `results`: ctypes arrays of n TrackDesc / TrackResult; `matches`,
    `residual_norm`, `in_grid`: addresses (in_grid may be None). frames=[DeviceFrame, ...] (n of them) is the resident mode: the
    frames are already on the device, or on their way there (DeviceFrame.prefetch) — every descriptor's image is set to NULL and
    results[f].frame names frame f on entry; it is the same handle on return, and the frame stays the caller's."""
    if frames is not None:
        if len(frames) != n:
            raise ValueError(f"{len(frames)} resident frames for {n} descriptors")
        for f, df in enumerate(frames):
            descs[f].image = None
            results[f].frame = df.handle.value if isinstance(df.handle, C.c_void_p) else df.handle
    return ctx.lib.dsdtm_track_frames(ctx.handle, C.byref(cam) if isinstance(cam, Camera) else C.byref(camera_struct(cam)), n, descs,
                                      results, matches, residual_norm, in_grid)


def keyframe_lib_path() -> str:
    return _addon.lib_path(KEYFRAME_LIB_NAME)


def _keyframe_not_built(path):
    return ImportError(f"{path} not found: the HIP extension is not built. Run "
                       "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). dsdtm_amd has no CPU fallback.")


def load_keyframe():
    """Load libdsdtm_amd_keyframe.so (include/dsdtm_amd_keyframe.h). No fallback: raises if it has not been built."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(KEYFRAME_LIB_NAME, {
        **_addon.context_signatures("dsdtm_keyframe"),
        "dsdtm_need_keyframe": (i, [vp, C.POINTER(Camera), C.POINTER(KeyframeParams), C.POINTER(KeyframeDesc), vp]),
        "dsdtm_need_keyframes": (i, [vp, C.POINTER(Camera), C.POINTER(KeyframeParams), i, C.POINTER(KeyframeDesc), vp])},
        _keyframe_not_built)


class KeyframeContext(_addon.AddonContext):
    """A dsdtm_keyframe_ctx: the add-on library's own context (stream + staging block) on one device."""
    PREFIX, ERROR, load = "dsdtm_keyframe", DsdtmError, staticmethod(load_keyframe)


def keyframe_context_of(ctx) -> KeyframeContext:
    """The keyframe context that goes with a Context (same device; created on first use, kept on the Context); a
    KeyframeContext is returned as it is."""
    if isinstance(ctx, KeyframeContext):
        return ctx
    kc = getattr(ctx, "_keyframe_ctx", None)
    if kc is None or kc.handle is None:
        kc = ctx._keyframe_ctx = KeyframeContext(getattr(ctx, "device", 0))
    return kc


def keyframe_params_struct(params=None) -> KeyframeParams:
    """dsdtm_keyframe_params from a keyframe_decision.KeyframeParams (or anything with its attributes); None: the defaults."""
    if isinstance(params, KeyframeParams):
        return params
    g = (lambda k, d: d) if params is None else (lambda k, d: getattr(params, k, d))
    return KeyframeParams(int(g("min_valid", 30)), int(g("max_valid", 50)), int(g("px_samples", 31)), 0,
                          float(g("min_px_median", 40.0)), float(g("min_rot", 0.08)), float(g("min_trans", 0.08)))


class KeyframeCall:
    """One prepared dsdtm_need_keyframes call: the descriptors and every array they point at are built once, `run_raw()` is the
    library call alone. `descs`: one dict per tracker with T_cur_w, T_kf_w (12 doubles or 3x4), n_valid, cur_p_world (n x 3),
    cur_bad (n bytes or None = none bad), kf_p_world, kf_bad, local_kf_centre (n x 3)."""

    def __init__(self, ctx, cam, params, descs, single: bool = False):
        self.ctx, self.n, self.single = keyframe_context_of(ctx), len(descs), single
        self.cs = cam if isinstance(cam, Camera) else camera_struct(cam)
        self.prm = keyframe_params_struct(params)
        self.descs = (KeyframeDesc * max(1, self.n))()
        self._keep = []

        def arr(v, dtype, cols):
            if v is None:
                return None, 0
            a = np.ascontiguousarray(v, dtype).reshape((-1, cols) if cols else (-1,))
            self._keep.append(a)
            return (a.ctypes.data if a.size else None), len(a)

        for t, d in enumerate(descs):
            k = self.descs[t]
            k.T_cur_w, _ = arr(np.asarray(d["T_cur_w"], np.float64).reshape(12), np.float64, 0)
            k.T_kf_w, _ = arr(np.asarray(d["T_kf_w"], np.float64).reshape(12), np.float64, 0)
            k.n_valid = int(d["n_valid"])
            k.cur_p_world, k.n_cur_points = arr(d["cur_p_world"], np.float64, 3)
            k.cur_bad, nb = arr(d.get("cur_bad"), np.uint8, 0)
            if d.get("cur_bad") is not None and nb != k.n_cur_points:
                raise ValueError(f"tracker {t}: {nb} cur_bad flags for {k.n_cur_points} points")
            k.kf_p_world, k.n_kf_points = arr(d["kf_p_world"], np.float64, 3)
            k.kf_bad, nb = arr(d.get("kf_bad"), np.uint8, 0)
            if d.get("kf_bad") is not None and nb != k.n_kf_points:
                raise ValueError(f"tracker {t}: {nb} kf_bad flags for {k.n_kf_points} points")
            k.local_kf_centre, k.n_local_kf = arr(d["local_kf_centre"], np.float64, 3)
        self.verdicts = np.zeros(max(1, self.n), KEYFRAME_VERDICT_DTYPE)

    def run_raw(self) -> int:
        if self.single:
            return self.ctx.lib.dsdtm_need_keyframe(self.ctx.handle, C.byref(self.cs), C.byref(self.prm), self.descs, self.verdicts.ctypes.data)
        return self.ctx.lib.dsdtm_need_keyframes(self.ctx.handle, C.byref(self.cs), C.byref(self.prm), self.n, self.descs,
                                                 self.verdicts.ctypes.data)

    def run(self) -> list:
        self.ctx.check(self.run_raw())
        return [{k: self.verdicts[k][t].item() for k in KEYFRAME_VERDICT_DTYPE.names if k != "reserved"} for t in range(self.n)]


def need_keyframes(ctx, cam, params, descs) -> list:
    """dsdtm_need_keyframes: Tracking::NeedKeyframe (src/Tracking.cpp:347-410) for len(descs) independent trackers in one
    submission (`ctx`: a Context, whose keyframe context is made on first use, or a KeyframeContext). Returns one dict per tracker: need, reason, rule_mask, undefined, n_px, n_depth, svo_kf, median_px, rot, trans,
    min_depth, median_depth (the fields of dsdtm_keyframe_verdict)."""
    if not descs:
        return []
    return KeyframeCall(ctx, cam, params, descs).run()


def need_keyframe(ctx, cam, params, desc) -> dict:
    """dsdtm_need_keyframe: the batch entry with n = 1."""
    return KeyframeCall(ctx, cam, params, [desc], single=True).run()[0]


def device_frame_of(ctx, frame):
    """The frame's pyramid on the device (uploaded on first use, cached on the Frame object)."""
    df = getattr(frame, "_device_frame", None)
    if df is None or df.ctx is not ctx or df.handle is None:
        df = frame._device_frame = DeviceFrame.from_pyramid(ctx, frame.mvImg_Pyr)
    return df


class DeviceFrame:
    """A frame's image pyramid kept on the device (dsdtm_frame): uploaded once, used by every Run the
    frame takes part in. `from_image` sends level 0 only and builds the pyramid with the library's
    bit-exact pyrDown (Frame::ComputeImagePyramid, reference src/Frame.cpp:74-81)."""

    def __init__(self, ctx: "Context", handle):
        self.ctx, self.handle = ctx, handle

    @classmethod
    def from_pyramid(cls, ctx: "Context", img_pyr):
        pyr, keep = pyramid_struct(img_pyr)
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_frame_create(ctx.handle, C.byref(pyr), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_image(cls, ctx: "Context", level0, levels: int):
        import numpy as np
        img = np.ascontiguousarray(level0, dtype=np.uint8)
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_frame_create_from_image(ctx.handle, img.ctypes.data_as(u8p), img.shape[1], img.shape[0],
                                                        img.strides[0], levels, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def prefetch(cls, ctx: "Context", gray, levels: int, depth=None, depth_scale: float = 5000.0):
        """dsdtm_frame_prefetch: the frame is enqueued on the context's prefetch stream and the call returns at once.
        `gray`: a 2-D uint8 array (rows may be padded) or a (pointer, width, height, stride) tuple for pinned / device memory;
        `depth`: a 2-D uint16 array (rows may be padded), a (pointer, stride_in_elements) tuple, or None. An array in
        pageable memory is staged before the call returns; anything else is read in place and must stay unchanged until
        `.wait()` or the first call that uses the frame has returned (the frame keeps a reference to the arrays)."""
        import numpy as np
        im = FrameImage()
        keep = []
        if isinstance(gray, tuple):
            ptr, w, h, stride = gray
        else:
            if gray.dtype != np.uint8 or gray.ndim != 2 or gray.strides[1] != 1:
                gray = np.ascontiguousarray(gray, dtype=np.uint8)
            keep.append(gray)
            ptr, w, h, stride = gray.ctypes.data, gray.shape[1], gray.shape[0], gray.strides[0]
        im.gray, im.width, im.height, im.stride, im.levels = ptr, w, h, stride, levels
        if depth is not None:
            if isinstance(depth, tuple):
                im.depth, im.depth_stride = depth
            else:
                if depth.dtype != np.uint16 or depth.ndim != 2 or depth.strides[1] != 2 or depth.strides[0] % 2:
                    depth = np.ascontiguousarray(depth, dtype=np.uint16)
                if depth.shape != (h, w):
                    raise ValueError(f"depth map {depth.shape} does not match the image {(h, w)}")
                keep.append(depth)
                im.depth, im.depth_stride = depth.ctypes.data, depth.strides[0] // 2
            im.depth_scale = depth_scale
        hnd = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_frame_prefetch(ctx.handle, C.byref(im), C.byref(hnd)))
        df = cls(ctx, hnd)
        df._keep = keep
        return df

    def wait(self):
        """dsdtm_frame_wait: the host waits until the frame is resident (buffers read in place are the caller's again)."""
        self.ctx.check(self.ctx.lib.dsdtm_frame_wait(self.ctx.handle, self.handle))
        self._keep = []
        return self

    def lift(self, cam, T_c2w, px_xy):
        """dsdtm_frame_lift: Frame::Get_FeatureDetph + Frame::UnProject for n pixels -> (depth[n] f32, -1 = none; p_world[n, 3])."""
        import numpy as np
        px = np.ascontiguousarray(px_xy, np.float32).reshape(-1, 2)
        T = np.ascontiguousarray(np.asarray(T_c2w, np.float64).reshape(-1)[:12])
        n = px.shape[0]
        d = np.empty(n, np.float32)
        p = np.empty((n, 3), np.float64)
        c = cam if isinstance(cam, Camera) else camera_struct(cam)
        self.ctx.check(self.ctx.lib.dsdtm_frame_lift(self.ctx.handle, self.handle, C.byref(c), T.ctypes.data, px.ctypes.data, n,
                                                     d.ctypes.data, p.ctypes.data))
        return d, p

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.dsdtm_frame_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns one dsdtm_ctx (one per calling thread, as the reference classes are single-threaded)."""

    def __init__(self, device: int = 0, diag: bool | None = None):
        diag = _DIAG_DEFAULT if diag is None else bool(diag)
        self.lib = load(diag)
        self.diag = diag
        h = C.c_void_p()
        st = self.lib.dsdtm_create(device, C.byref(h))
        if st != OK:
            msg = self.lib.dsdtm_last_error(None)
            raise DsdtmError(st, msg.decode() if msg else "dsdtm_create failed")
        self.handle = h
        self.device = device

    def check(self, st: int):
        if st != OK:
            msg = self.lib.dsdtm_last_error(self.handle)
            raise DsdtmError(st, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.dsdtm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT_CTX = {}


def default_context(device: int = 0, diag: bool | None = None) -> Context:
    diag = _DIAG_DEFAULT if diag is None else bool(diag)
    ctx = _DEFAULT_CTX.get((device, diag))
    if ctx is None:
        ctx = _DEFAULT_CTX[(device, diag)] = Context(device, diag)
    return ctx
