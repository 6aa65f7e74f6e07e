"""libdsdtm_amd_framediff.so (include/dsdtm_amd_framediff.h) from Python: the ctypes binding of dsdtm_framediff_steps / _step / _warp —
Moving_Detecter::Mod_FrameDiff (warp the other frame by H, subtract, threshold, open, dilate) and the feature test of
Frame::Motion_Removal on its mask, for n independent pairs in one submission. The rules are this project's definition
(dsdtm_amd/framediff_restatement.py, F1-F8 of the header); parity with OpenCV is unpinned.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_framediff.so"
# every symbol include/dsdtm_amd_framediff.h declares
SYMBOLS = ["dsdtm_framediff_create", "dsdtm_framediff_destroy", "dsdtm_framediff_last_error", "dsdtm_framediff_steps", "dsdtm_framediff_step",
           "dsdtm_framediff_warp"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MIN_SIDE, MAX_SIDE, MAX_FEATURES, MAX_STEPS, THRESHOLD, MAXVAL, INVERSE_MAP = 16, 4096, 16384, 1024, 50, 200, 1
FILL = 0xA5          # what the outputs hold before the call: a refused call leaves it there


class Desc(C.Structure):
    """dsdtm_framediff_desc"""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("a_stride", C.c_int32), ("b_stride", C.c_int32),
                ("H", C.c_double * 9), ("flags", C.c_int32), ("threshold", C.c_int32), ("maxval", C.c_int32), ("mask_stride", C.c_int32),
                ("mask", C.c_void_p), ("warped", C.c_void_p), ("warped_stride", C.c_int32), ("n_features", C.c_int32),
                ("feature_px", C.c_void_p), ("feature_on_mask", C.c_void_p)]


class Result(C.Structure):
    """dsdtm_framediff_result"""
    _fields_ = [("M", C.c_double * 9), ("n_foreground", C.c_int32), ("n_flagged", C.c_int32)]


class FrameDiffError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_framediff.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_framediff"),
        "dsdtm_framediff_steps": (i, [vp, i, C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_framediff_step": (i, [vp, C.POINTER(Desc), C.POINTER(Result)]),
        "dsdtm_framediff_warp": (i, [vp, i, C.POINTER(Desc)])}, _not_built)


def _image(image):
    """(pointer, width, height, stride, what to keep alive) of a gray image: a 2-d uint8 numpy array (rows may be strided) or anything
    with data_ptr() / stride() (a torch tensor, on the host or on this device)."""
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim != 2 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, np.uint8)
        return image.ctypes.data, image.shape[1], image.shape[0], image.strides[0], image
    if image.dim() != 2 or image.stride(1) != 1:
        raise ValueError("an image must be 2-d with contiguous rows")
    return image.data_ptr(), int(image.shape[1]), int(image.shape[0]), int(image.stride(0)), image


def _output(want, width, height):
    """(array or tensor the caller reads, pointer, stride): want True -> a fresh host array prefilled with FILL; an array / tensor of
    the caller (host or this device) -> written in place; None / False -> not wanted."""
    if want is None or want is False:
        return None, None, 0
    if want is True:
        out = np.full((height, width), FILL, np.uint8)
        return out, out.ctypes.data, width
    if isinstance(want, np.ndarray) and (want.dtype != np.uint8 or want.ndim != 2 or want.strides[1] != 1 or not want.flags.writeable):
        raise ValueError("an output must be a writeable 2-d uint8 array with contiguous rows (it is written in place)")
    ptr, w, h, stride, hold = _image(want)
    if (w, h) != (width, height):
        raise ValueError(f"an output is {w} x {h}, not {width} x {height}")
    return want, ptr, stride


class Prepared:
    """The descriptors of one dsdtm_framediff_steps / _warp call and every array they point at; run_raw() is the C call alone."""

    def __init__(self, ctx, pairs, warp_only=False):
        self.ctx, self.n, self.warp_only = ctx, len(pairs), warp_only
        self.descs, self.res = (Desc * max(self.n, 1))(), (Result * max(self.n, 1))()
        C.memset(self.res, FILL, C.sizeof(self.res))
        self.keep, self.outs = [], []
        for k, p in enumerate(pairs):
            d = self.descs[k]
            bp, w, h, bs, bk = _image(p["b"])
            a = p.get("a")
            ap, aw, ah, as_, ak = (bp, w, h, bs, bk) if a is p["b"] else _image(a) if a is not None else (None, w, h, 0, None)
            if (aw, ah) != (w, h):
                raise ValueError("a and b differ in size")
            d.a, d.b, d.width, d.height, d.a_stride, d.b_stride = ap, bp, w, h, as_, bs
            d.H[:] = [float(v) for v in np.asarray(p["H"], np.float64).reshape(9)]
            d.flags, d.threshold, d.maxval = p.get("flags", 0), p.get("threshold", THRESHOLD), p.get("maxval", 0)
            mask, d.mask, d.mask_stride = _output(p.get("mask", not warp_only), w, h)
            warped, d.warped, d.warped_stride = _output(p.get("warped", warp_only), w, h)
            f = p.get("features")
            f = None if f is None else np.ascontiguousarray(np.asarray(f, np.float32).reshape(-1, 2))
            flags = None if f is None else np.full(len(f), FILL, np.uint8)
            d.n_features = 0 if f is None else len(f)
            d.feature_px = f.ctypes.data if f is not None and len(f) else None
            d.feature_on_mask = flags.ctypes.data if flags is not None and len(flags) else None
            self.keep.append((ak, bk, f))
            self.outs.append((mask, warped, flags))

    def run_raw(self) -> int:
        if self.warp_only:
            return self.ctx.lib.dsdtm_framediff_warp(self.ctx.handle, self.n, self.descs)
        return self.ctx.lib.dsdtm_framediff_steps(self.ctx.handle, self.n, self.descs, self.res)

    def results(self) -> list:
        if self.warp_only:
            return [o[1] for o in self.outs]
        return [dict(M=np.array(self.res[k].M[:], np.float64), n_foreground=int(self.res[k].n_foreground), n_flagged=int(self.res[k].n_flagged),
                     mask=o[0], warped=o[1], flags=o[2]) for k, o in enumerate(self.outs)]


class FrameDiffContext(_addon.AddonContext):
    """A dsdtm_framediff_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_framediff", FrameDiffError, staticmethod(load)

    def prepare(self, pairs, warp_only=False) -> Prepared:
        return Prepared(self, pairs, warp_only)

    def steps(self, pairs) -> list:
        """dsdtm_framediff_steps: `pairs` is a list of dicts(a, b, H, flags=0, threshold=50, maxval=0, mask=True, warped=None,
        features=None); mask / warped: True (a fresh host array), an array or tensor of the caller's (host or device), None (not
        wanted). One submission. Returns one dict(M, n_foreground, n_flagged, mask, warped, flags) per pair."""
        p = Prepared(self, pairs)
        self.check(p.run_raw())
        return p.results()

    def step(self, a, b, H, **kw) -> dict:
        """dsdtm_framediff_step (the single entry)."""
        p = Prepared(self, [dict(a=a, b=b, H=H, **kw)])
        self.check(self.lib.dsdtm_framediff_step(self.handle, p.descs, p.res))
        return p.results()[0]

    def warp(self, images) -> list:
        """dsdtm_framediff_warp: `images` is a list of dicts(b, H, flags=0, warped=True). One submission. Returns the warped images."""
        p = Prepared(self, images, warp_only=True)
        self.check(p.run_raw())
        return p.results()
