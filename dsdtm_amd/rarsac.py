"""libdsdtm_amd_rarsac.so (include/dsdtm_amd_rarsac.h) from Python: the ctypes binding of dsdtm_rarsac_reject_batch / dsdtm_rarsac_check —
Rarsac_base::RejectFundamental, the grid-guided RANSAC for the fundamental matrix, for n trackers in one launch — and a Python twin of
the reference's class. Which samples are drawn and how the 8-point system is solved are this project's definition
(dsdtm_amd/rarsac_restatement.py); parity with OpenCV is unpinned.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_rarsac.so"
# every symbol include/dsdtm_amd_rarsac.h declares
SYMBOLS = ["dsdtm_rarsac_create", "dsdtm_rarsac_destroy", "dsdtm_rarsac_last_error", "dsdtm_rarsac_reject_batch", "dsdtm_rarsac_reject",
           "dsdtm_rarsac_check"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
GRID, MIN_POINTS, MAX_POINTS, MAX_PROBLEMS, MAX_ITERATIONS = 100, 8, 2048, 1024, 16384
DEFAULT_ITERATIONS, DEFAULT_TERMINATE, DEFAULT_SIGMA, DEFAULT_SEED = 1000, 0.001, 0.5, 0x2545F491
FILL = 0xA5          # what the outputs hold before the call: a refused call, and a problem with found = 0, leave it there


class Desc(C.Structure):
    """dsdtm_rarsac_desc"""
    _fields_ = [("cur", C.c_void_p), ("prev", C.c_void_p), ("status", C.c_void_p), ("F", C.c_void_p), ("grid_probability_in", C.c_double * GRID),
                ("terminate_threshold", C.c_double), ("sigma", C.c_float), ("seed", C.c_uint32), ("m", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("max_iterations", C.c_int32)]


class Result(C.Structure):
    """dsdtm_rarsac_result"""
    _fields_ = [("grid_probability_out", C.c_double * GRID), ("score", C.c_double), ("F", C.c_float * 9), ("found", C.c_int32),
                ("best_hypothesis", C.c_int32), ("iterations_run", C.c_int32), ("n_inliers", C.c_int32), ("reserved", C.c_int32 * 3)]


class RarsacError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_rarsac.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_rarsac"),
        "dsdtm_rarsac_reject_batch": (i, [vp, i, C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_rarsac_check": (i, [vp, i, C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_rarsac_reject": (i, [vp, i, vp, vp, i, i, vp, vp, C.POINTER(Result)])}, _not_built)


def _answer(res: Result, status):
    """A result as the restatement reports it; found = 0 carries nothing else."""
    if res.found != 1:
        return dict(found=int(res.found))
    return dict(found=1, status=status, F=np.array(res.F[:], np.float32), grid=np.array(res.grid_probability_out[:], np.float64), score=float(res.score),
                best_hypothesis=res.best_hypothesis, iterations_run=res.iterations_run, n_inliers=res.n_inliers)


def _points(p):
    return np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 2))


class PreparedProblems:
    """The descriptors of one dsdtm_rarsac_reject_batch / dsdtm_rarsac_check call and every array they point at; run_raw() is the C call
    alone. A problem is a dict: cur, prev, and optionally width, height (640 x 480), prior, max_iterations, terminate, sigma, seed, F."""

    def __init__(self, ctx, problems, check=False):
        self.ctx, self.n, self.check = ctx, len(problems), check
        self.descs = (Desc * max(self.n, 1))()
        self.results = (Result * max(self.n, 1))()
        C.memset(self.results, FILL, C.sizeof(self.results))
        self.keep, self.status = [], []
        for k, prob in enumerate(problems):
            cur, prev = _points(prob["cur"]), _points(prob["prev"])
            if len(cur) != len(prev):
                raise ValueError(f"problem {k}: cur and prev differ in length")
            status = np.full(max(len(cur), 1), FILL, np.uint8)
            F = np.ascontiguousarray(prob["F"], np.float32).reshape(9) if prob.get("F") is not None else None
            self.keep.append((cur, prev, F))
            self.status.append(status)
            d = self.descs[k]
            d.cur, d.prev, d.status, d.m = cur.ctypes.data, prev.ctypes.data, status.ctypes.data, len(cur)
            d.F = F.ctypes.data if F is not None else None
            d.width, d.height = prob.get("width", 640), prob.get("height", 480)
            prior = prob.get("prior")
            d.grid_probability_in[:] = [0.5] * GRID if prior is None else [float(v) for v in np.asarray(prior, np.float64).reshape(GRID)]
            d.max_iterations, d.terminate_threshold = prob.get("max_iterations", 0), prob.get("terminate", 0.0)
            d.sigma, d.seed = prob.get("sigma", 0.0), prob.get("seed", 0)

    def run_raw(self) -> int:
        fn = self.ctx.lib.dsdtm_rarsac_check if self.check else self.ctx.lib.dsdtm_rarsac_reject_batch
        return fn(self.ctx.handle, self.n, self.descs, self.results)

    def answers(self) -> list:
        return [_answer(self.results[k], self.status[k][:len(self.keep[k][0])].copy()) for k in range(self.n)]


class RarsacContext(_addon.AddonContext):
    """A dsdtm_rarsac_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_rarsac", RarsacError, staticmethod(load)

    def prepare(self, problems, check=False) -> PreparedProblems:
        return PreparedProblems(self, problems, check)

    def reject_batch(self, problems) -> list:
        """dsdtm_rarsac_reject_batch: one submission. One dict per problem: found and, with found = 1, status (m,), F (9,), grid (100,),
        score, best_hypothesis, iterations_run, n_inliers."""
        p = PreparedProblems(self, problems)
        self.check(p.run_raw())
        return p.answers()

    def check_batch(self, problems) -> list:
        """dsdtm_rarsac_check: R5-R6 alone for each problem's F."""
        p = PreparedProblems(self, problems, check=True)
        self.check(p.run_raw())
        return p.answers()

    def reject(self, cur, prev, width=640, height=480, prior=None) -> dict:
        """dsdtm_rarsac_reject (the single entry, default parameters)."""
        cur, prev = _points(cur), _points(prev)
        if len(cur) != len(prev):
            raise ValueError("cur and prev differ in length")
        status, res = np.full(max(len(cur), 1), FILL, np.uint8), Result()
        C.memset(C.byref(res), FILL, C.sizeof(res))
        grid = None if prior is None else np.ascontiguousarray(prior, np.float64).reshape(GRID)
        self.check(self.lib.dsdtm_rarsac_reject(self.handle, len(cur), cur.ctypes.data, prev.ctypes.data, width, height,
                                                grid.ctypes.data if grid is not None else None, status.ctypes.data, C.byref(res)))
        return _answer(res, status[:len(cur)])


class Rarsac_base:
    """The reference's class (include/Rarsac_base.h): Rarsac_base(frame_grid_probability, pts1, pts2).RejectFundamental() returns the status
    vector and writes the frame's grid (a mutable sequence of 100 doubles) back when a hypothesis won, as src/Rarsac_base.cpp:250 does."""

    def __init__(self, frame_grid_probability, pts1, pts2, width=640, height=480, ctx=None):
        self.grid, self.cur, self.prev, self.width, self.height = frame_grid_probability, _points(pts1), _points(pts2), width, height
        self.ctx, self.result = ctx, None

    def RejectFundamental(self):
        ctx = self.ctx or RarsacContext(0)
        try:
            self.result = ctx.reject(self.cur, self.prev, self.width, self.height, np.asarray(self.grid, np.float64))
        finally:
            if self.ctx is None:
                ctx.close()
        if self.result["found"] != 1:
            return np.zeros(0, np.uint8)
        if self.result["best_hypothesis"] >= 0:
            self.grid[:] = self.result["grid"]
        return self.result["status"]
