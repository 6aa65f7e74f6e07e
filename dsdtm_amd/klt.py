"""libdsdtm_amd_klt.so (include/dsdtm_amd_klt.h) from Python: the ctypes binding of dsdtm_klt_steps / dsdtm_klt_flow — KLTWrapper::RunTrack
(the pyramidal Lucas-Kanade flow of a grid of points and the RANSAC homography of the survivors) for n trackers in one submission: the
H that dsdtm_motion_step and dsdtm_mcd_step take as an argument, from images alone. The rules are this project's definition
(dsdtm_amd/klt_restatement.py, K1-K9 of the header); parity with OpenCV is unpinned.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_klt.so"
# every symbol include/dsdtm_amd_klt.h declares
SYMBOLS = ["dsdtm_klt_create", "dsdtm_klt_destroy", "dsdtm_klt_last_error", "dsdtm_klt_model_create", "dsdtm_klt_model_destroy",
           "dsdtm_klt_model_reset", "dsdtm_klt_model_pyramid", "dsdtm_klt_steps", "dsdtm_klt_step", "dsdtm_klt_flow"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MAX_STEPS, MAX_FLOW_POINTS, MAX_LEVELS, MIN_WINDOW, MAX_WINDOW = 1024, 16384, 5, 3, 21
SOURCE_IDENTITY, SOURCE_RANSAC, SOURCE_KEPT = 0, 1, 2
FILL = 0xA5          # what the outputs hold before the call: a refused call leaves it there


class Desc(C.Structure):
    """dsdtm_klt_desc"""
    _fields_ = [("model", C.c_void_p), ("image", C.c_void_p), ("stride", C.c_int32), ("grid_w", C.c_int32), ("grid_h", C.c_int32),
                ("reserved", C.c_int32), ("prev_points", C.c_void_p), ("points", C.c_void_p), ("status", C.c_void_p),
                ("iterations", C.c_void_p), ("mask", C.c_void_p)]


class Result(C.Structure):
    """dsdtm_klt_result"""
    _fields_ = [("H", C.c_double * 9), ("cost_before", C.c_double), ("cost_after", C.c_double), ("source", C.c_int32), ("n_points", C.c_int32),
                ("n_tracked", C.c_int32), ("n_inliers", C.c_int32), ("best_hypothesis", C.c_int32), ("rounds", C.c_int32),
                ("refit_iterations", C.c_int32), ("frame", C.c_int32)]


class FlowDesc(C.Structure):
    """dsdtm_klt_flow_desc"""
    _fields_ = [("prev", C.c_void_p), ("cur", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("prev_stride", C.c_int32),
                ("cur_stride", C.c_int32), ("n_points", C.c_int32), ("window", C.c_int32), ("levels", C.c_int32), ("iterations", C.c_int32),
                ("epsilon", C.c_double), ("min_eig", C.c_double), ("points", C.c_void_p), ("guesses", C.c_void_p), ("out_points", C.c_void_p),
                ("status", C.c_void_p), ("iterations_used", C.c_void_p), ("residual", C.c_void_p)]


class KltError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_klt.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_klt"),
        "dsdtm_klt_model_create": (i, [vp, i, i, i, C.POINTER(vp)]),
        "dsdtm_klt_model_destroy": (None, [vp, vp]),
        "dsdtm_klt_model_reset": (i, [vp, vp]),
        "dsdtm_klt_model_pyramid": (i, [vp, vp, i, vp, i]),
        "dsdtm_klt_steps": (i, [vp, i, C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_klt_step": (i, [vp, vp, vp, i, C.POINTER(Result)]),
        "dsdtm_klt_flow": (i, [vp, i, C.POINTER(FlowDesc)])}, _not_built)


def _image_pointer(image, width, height, stride=None):
    """(pointer, stride, what to keep alive) of a gray image: a uint8 numpy array (rows may be strided), anything with data_ptr() /
    stride() (a torch tensor, on the host or on this device), or a raw pointer with `stride`."""
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim != 2 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, np.uint8)
        if image.shape != (height, width):
            raise ValueError(f"image is {image.shape[1]} x {image.shape[0]}, not {width} x {height}")
        return image.ctypes.data, image.strides[0], image
    if hasattr(image, "data_ptr"):
        if tuple(image.shape) != (height, width):
            raise ValueError(f"image is {tuple(image.shape)}, not ({height}, {width})")
        return image.data_ptr(), int(image.stride(0)), image
    return int(image), int(stride), None


class KltContext(_addon.AddonContext):
    """A dsdtm_klt_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_klt", KltError, staticmethod(load)

    def steps(self, steps) -> list:
        """dsdtm_klt_steps: `steps` is a list of dicts(model, image, want=True, stride=None, grid_w=0, grid_h=0). One submission.
        Returns one dict per entry: H (9,), source, n_points, n_tracked, n_inliers, frame, cost_before, cost_after, best_hypothesis,
        rounds, refit_iterations and, with want, prev_points, points, status, iterations, mask (the first n_tracked bytes)."""
        n = len(steps)
        descs, results = (Desc * max(n, 1))(), (Result * max(n, 1))()
        C.memset(results, FILL, C.sizeof(results))
        keep, outs = [], []
        for k, s in enumerate(steps):
            m = s["model"]
            ptr, stride, hold = _image_pointer(s["image"], m.width, m.height, s.get("stride"))
            d = descs[k]
            d.model, d.image, d.stride, d.grid_w, d.grid_h = m.handle, ptr, stride, s.get("grid_w", 0), s.get("grid_h", 0)
            out = None
            if s.get("want", True):
                cap = max(1, max(0, m.width // (d.grid_w or 32) - 1) * max(0, m.height // (d.grid_h or 24) - 1))
                out = dict(prev_points=np.full((cap, 2), np.nan, np.float32), points=np.full((cap, 2), np.nan, np.float32),
                           status=np.full(cap, FILL, np.uint8), iterations=np.full(cap, -1, np.int32), mask=np.full(cap, FILL, np.uint8))
                d.prev_points, d.points, d.status = out["prev_points"].ctypes.data, out["points"].ctypes.data, out["status"].ctypes.data
                d.iterations, d.mask = out["iterations"].ctypes.data, out["mask"].ctypes.data
            keep.append(hold)
            outs.append(out)
        self.check(self.lib.dsdtm_klt_steps(self.handle, n, descs, results))
        del keep
        return [_answer(results[k], outs[k]) for k in range(n)]

    def flow(self, pairs) -> list:
        """dsdtm_klt_flow: `pairs` is a list of dicts(prev, cur, points, guesses=None, window=0, levels=0, iterations=0, epsilon=0.0,
        min_eig=0.0) (0: the default). One submission. Returns one dict(points, status, iterations, residual) per pair."""
        n = len(pairs)
        descs = (FlowDesc * max(n, 1))()
        keep, outs = [], []
        for k, p in enumerate(pairs):
            h, w = int(p["prev"].shape[0]), int(p["prev"].shape[1])
            p0, s0, k0 = _image_pointer(p["prev"], w, h)
            p1, s1, k1 = _image_pointer(p["cur"], w, h)
            pts = np.ascontiguousarray(np.asarray(p["points"], np.float32).reshape(-1, 2))
            g = p.get("guesses")
            g = None if g is None else np.ascontiguousarray(np.asarray(g, np.float32).reshape(-1, 2))
            m = len(pts)
            out = dict(points=np.full((max(m, 1), 2), np.nan, np.float32), status=np.full(max(m, 1), FILL, np.uint8),
                       iterations=np.full(max(m, 1), -1, np.int32), residual=np.full(max(m, 1), np.nan, np.float32))
            d = descs[k]
            d.prev, d.cur, d.width, d.height, d.prev_stride, d.cur_stride = p0, p1, w, h, s0, s1
            d.n_points, d.window, d.levels, d.iterations = m, p.get("window", 0), p.get("levels", 0), p.get("iterations", 0)
            d.epsilon, d.min_eig = p.get("epsilon", 0.0), p.get("min_eig", 0.0)
            d.points, d.guesses = pts.ctypes.data, (g.ctypes.data if g is not None else None)
            d.out_points, d.status, d.iterations_used, d.residual = (out["points"].ctypes.data, out["status"].ctypes.data,
                                                                     out["iterations"].ctypes.data, out["residual"].ctypes.data)
            keep.append((k0, k1, pts, g))
            outs.append({name: a[:m] for name, a in out.items()})
        self.check(self.lib.dsdtm_klt_flow(self.handle, n, descs))
        del keep
        return outs


def _answer(res: Result, out):
    r = dict(H=np.array(res.H[:], np.float64), source=int(res.source), n_points=int(res.n_points), n_tracked=int(res.n_tracked),
             n_inliers=int(res.n_inliers), frame=int(res.frame), cost_before=res.cost_before, cost_after=res.cost_after,
             best_hypothesis=int(res.best_hypothesis), rounds=int(res.rounds), refit_iterations=int(res.refit_iterations))
    if out is not None:
        n = r["n_points"]
        r.update(prev_points=out["prev_points"][:n], points=out["points"][:n], status=out["status"][:n], iterations=out["iterations"][:n],
                 mask=out["mask"][:r["n_tracked"]] if r["source"] == SOURCE_RANSAC else np.zeros(0, np.uint8))
    return r


class KltModel:
    """A dsdtm_klt_model: the device-resident pyramid of one tracker's previous image, its previous H and frame counter."""

    def __init__(self, ctx: KltContext, width: int, height: int, levels: int = 0):
        self.ctx, self.width, self.height, self.levels = ctx, int(width), int(height), int(levels) or 4
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_klt_model_create(ctx.handle, self.width, self.height, int(levels), C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.dsdtm_klt_model_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(self.ctx.lib.dsdtm_klt_model_reset(self.ctx.handle, self.handle))

    def pyramid(self) -> list:
        """The pyramid of the last image the model was stepped with (what the next step tracks from)."""
        out, w, h = [], self.width, self.height
        for l in range(self.levels):
            a = np.full((h, w), FILL, np.uint8)
            self.ctx.check(self.ctx.lib.dsdtm_klt_model_pyramid(self.ctx.handle, self.handle, l, a.ctypes.data, w))
            out.append(a)
            w, h = (w + 1) // 2, (h + 1) // 2
        return out

    def step(self, image, want=True, stride=None, grid_w=0, grid_h=0) -> dict:
        return self.ctx.steps([dict(model=self, image=image, want=want, stride=stride, grid_w=grid_w, grid_h=grid_h)])[0]

    def step_single(self, image) -> dict:
        """dsdtm_klt_step (the single entry: the result alone)."""
        ptr, stride, hold = _image_pointer(image, self.width, self.height)
        res = Result()
        C.memset(C.byref(res), FILL, C.sizeof(res))
        st = self.ctx.lib.dsdtm_klt_step(self.ctx.handle, self.handle, ptr, stride, C.byref(res))
        del hold
        self.ctx.check(st)
        return _answer(res, None)


class KLTWrapper:
    """KLTWrapper (Thirdparty/fastMCD/src/KLTWrapper.h) over the C ABI: Init(image) seeds the model, RunTrack(image) tracks the grid from
    the last image and fits H, GetHomography() returns it (3 x 3, maps the current frame to the last one)."""

    def __init__(self, ctx: KltContext | None = None, device: int = 0):
        self.ctx = ctx or KltContext(device)
        self.model, self.last = None, None
        self.H = np.eye(3)

    def Init(self, image):
        self.model = KltModel(self.ctx, int(image.shape[1]), int(image.shape[0]))
        self.last = self.model.step(image, want=False)
        self.H = self.last["H"].reshape(3, 3).copy()

    def RunTrack(self, image, want=False) -> dict:
        if self.model is None:
            self.Init(image)
            return self.last
        self.last = self.model.step(image, want=want)
        self.H = self.last["H"].reshape(3, 3).copy()
        return self.last

    def GetHomography(self) -> np.ndarray:
        return self.H.copy()
