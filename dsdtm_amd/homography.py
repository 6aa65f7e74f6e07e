"""libdsdtm_amd_homography.so (include/dsdtm_amd_homography.h) from Python: the ctypes binding of dsdtm_find_homographies — RANSAC
homographies for n trackers in one launch, the H that dsdtm_motion_step (dsdtm_amd/motion.py) takes as an argument. It keeps the
documented shape of cv::findHomography(A, B, CV_RANSAC) at its default arguments; everything else is this project's definition
(dsdtm_amd/homography_restatement.py), and parity with OpenCV is unpinned.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_homography.so"
# every symbol include/dsdtm_amd_homography.h declares
SYMBOLS = ["dsdtm_homography_create", "dsdtm_homography_destroy", "dsdtm_homography_last_error", "dsdtm_find_homographies",
           "dsdtm_find_homography"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MAX_POINTS, MAX_PROBLEMS, MAX_HYPOTHESES, DEFAULT_HYPOTHESES = 2048, 1024, 4096, 2048
DEFAULT_THRESHOLD, DEFAULT_CONFIDENCE, DEFAULT_SEED = 3.0, 0.995, 0x2545F491
FILL = 0xA5          # what the outputs hold before the call: a refused call, and a problem with found = 0, leave it there


class Desc(C.Structure):
    """dsdtm_homography_desc"""
    _fields_ = [("points_a", C.c_void_p), ("points_b", C.c_void_p), ("mask", C.c_void_p), ("m", C.c_int32), ("max_hypotheses", C.c_int32),
                ("reproj_threshold", C.c_double), ("confidence", C.c_double), ("seed", C.c_uint32), ("reserved", C.c_uint32)]


class Result(C.Structure):
    """dsdtm_homography_result"""
    _fields_ = [("H", C.c_double * 9), ("cost_before", C.c_double), ("cost_after", C.c_double), ("found", C.c_int32),
                ("n_inliers", C.c_int32), ("best_hypothesis", C.c_int32), ("rounds", C.c_int32), ("refit_iterations", C.c_int32),
                ("reserved", C.c_int32)]


class HomographyError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_homography.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_homography"),
        "dsdtm_find_homographies": (i, [vp, i, C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_find_homography": (i, [vp, i, vp, vp, vp, C.POINTER(Result)])}, _not_built)


def _answer(res: Result, mask):
    """A result as the restatement reports it; found = 0 carries nothing else."""
    if res.found != 1:
        return dict(found=int(res.found))
    return dict(found=1, H=np.array(res.H[:], np.float64), mask=mask, n_inliers=res.n_inliers, best_hypothesis=res.best_hypothesis,
                rounds=res.rounds, refit_iterations=res.refit_iterations, cost_before=res.cost_before, cost_after=res.cost_after)


class HomographyContext(_addon.AddonContext):
    """A dsdtm_homography_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_homography", HomographyError, staticmethod(load)

    def prepare(self, problems) -> "PreparedProblems":
        """A dsdtm_find_homographies call built once (descriptors, output arrays), to be run any number of times."""
        return PreparedProblems(self, problems)

    def find_homographies(self, problems) -> list:
        """dsdtm_find_homographies: `problems` is a list of (A, B) or (A, B, params), A and B m x 2 (float32), params a dict of
        thr / confidence / max_hypotheses / seed (absent: the defaults). One submission. Returns one dict per problem: found and, with
        found = 1, H (9,), mask (m,), n_inliers, best_hypothesis, rounds, refit_iterations, cost_before, cost_after."""
        p = PreparedProblems(self, problems)
        self.check(p.run_raw())
        return p.answers()

    def find_homography(self, A, B) -> dict:
        """dsdtm_find_homography (the single entry, default parameters)."""
        A, B = _points(A), _points(B)
        if len(A) != len(B):
            raise ValueError("A and B differ in length")
        mask, res = np.full(max(len(A), 1), FILL, np.uint8), Result()
        C.memset(C.byref(res), FILL, C.sizeof(res))
        self.check(self.lib.dsdtm_find_homography(self.handle, len(A), A.ctypes.data, B.ctypes.data, mask.ctypes.data, C.byref(res)))
        return _answer(res, mask[:len(A)])


def _points(p):
    return np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 2))


class PreparedProblems:
    """The descriptors of one dsdtm_find_homographies call and every array they point at; run_raw() is the C call alone."""

    def __init__(self, ctx, problems):
        self.ctx, self.n = ctx, len(problems)
        self.descs = (Desc * max(self.n, 1))()
        self.results = (Result * max(self.n, 1))()
        C.memset(self.results, FILL, C.sizeof(self.results))
        self.keep, self.masks = [], []
        for k, prob in enumerate(problems):
            A, B = _points(prob[0]), _points(prob[1])
            if len(A) != len(B):
                raise ValueError(f"problem {k}: A and B differ in length")
            params = prob[2] if len(prob) > 2 and prob[2] else {}
            mask = np.full(max(len(A), 1), FILL, np.uint8)
            self.keep.append((A, B))
            self.masks.append(mask)
            d = self.descs[k]
            d.points_a, d.points_b, d.mask, d.m = A.ctypes.data, B.ctypes.data, mask.ctypes.data, len(A)
            d.reproj_threshold, d.confidence = params.get("thr", 0.0), params.get("confidence", 0.0)
            d.max_hypotheses, d.seed = params.get("max_hypotheses", 0), params.get("seed", 0)

    def run_raw(self) -> int:
        return self.ctx.lib.dsdtm_find_homographies(self.ctx.handle, self.n, self.descs, self.results)

    def answers(self) -> list:
        return [_answer(self.results[k], self.masks[k][:len(self.keep[k][0])].copy()) for k in range(self.n)]
