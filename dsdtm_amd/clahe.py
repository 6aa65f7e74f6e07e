"""libdsdtm_amd_clahe.so (include/dsdtm_amd_clahe.h) from Python: the ctypes binding of dsdtm_clahe_apply_batch / _apply / _luts —
cv::createCLAHE(3.0, cv::Size(8, 8))->apply of the reference's drivers, n frames of mixed sizes in one submission — and createCLAHE(),
the object those drivers use. The rules E1-E7 are this project's definition (dsdtm_amd/clahe_restatement.py); parity with OpenCV
binaries is unpinned.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon

LIB_NAME = "libdsdtm_amd_clahe.so"
# every symbol include/dsdtm_amd_clahe.h declares
SYMBOLS = ["dsdtm_clahe_create", "dsdtm_clahe_destroy", "dsdtm_clahe_last_error", "dsdtm_clahe_apply_batch", "dsdtm_clahe_apply", "dsdtm_clahe_luts"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MIN_SIDE, MAX_SIDE, MAX_TILES, DEFAULT_TILES, DEFAULT_CLIP_LIMIT, MAX_FRAMES = 16, 4096, 16, 8, 3.0, 1024


class Desc(C.Structure):
    """dsdtm_clahe_desc"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("lut_out", C.c_void_p), ("clip_limit", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("src_stride", C.c_int32), ("dst_stride", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32)]


class ClaheError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_clahe.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_clahe"),
        "dsdtm_clahe_apply_batch": (i, [vp, i, C.POINTER(Desc)]),
        "dsdtm_clahe_apply": (i, [vp, C.POINTER(Desc)]),
        "dsdtm_clahe_luts": (i, [vp, C.POINTER(Desc)])}, _not_built)


def _image(a):
    """(address, width, height, stride in bytes, keep-alive) of a gray image: a 2-D uint8 numpy array (host memory), a 2-D uint8 torch
    tensor (device or pinned host memory), rows contiguous, or a tuple (address, width, height, stride) for anything else."""
    if isinstance(a, tuple):
        return int(a[0]), int(a[1]), int(a[2]), int(a[3]), None
    if isinstance(a, np.ndarray):
        assert a.ndim == 2 and a.dtype == np.uint8 and a.strides[1] == 1, "an image is 2-D uint8 with contiguous rows"
        return a.ctypes.data, a.shape[1], a.shape[0], a.strides[0], a
    assert a.dim() == 2 and a.element_size() == 1 and a.stride(1) == 1, "an image is 2-D uint8 with contiguous rows"       # a torch tensor
    return a.data_ptr(), a.shape[1], a.shape[0], a.stride(0), a


class ClaheContext(_addon.AddonContext):
    """A dsdtm_clahe_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_clahe", ClaheError, staticmethod(load)

    def descs(self, frames):
        """The dsdtm_clahe_desc array of `frames`: dicts of src, dst and, optionally, clip_limit (default 3.0), tiles_x, tiles_y (default
        8), lut_out (a C-contiguous uint8 numpy array of tiles_y * tiles_x * 256 bytes). Returns (array, what must stay alive)."""
        arr = (Desc * max(len(frames), 1))()
        keep = []
        for k, f in enumerate(frames):
            d = arr[k]
            d.src, d.width, d.height, d.src_stride, alive = _image(f["src"])
            keep.append(alive)
            if f.get("dst") is not None:
                d.dst, w, h, d.dst_stride, alive = _image(f["dst"])
                assert (w, h) == (d.width, d.height), "dst has the size of src"
                keep.append(alive)
            d.clip_limit = float(f.get("clip_limit", DEFAULT_CLIP_LIMIT))
            d.tiles_x, d.tiles_y = int(f.get("tiles_x", DEFAULT_TILES)), int(f.get("tiles_y", DEFAULT_TILES))
            lut = f.get("lut_out")
            if lut is not None:
                assert isinstance(lut, np.ndarray) and lut.dtype == np.uint8 and lut.flags.c_contiguous
                assert lut.size == (d.tiles_x or DEFAULT_TILES) * (d.tiles_y or DEFAULT_TILES) * 256, "lut_out holds tiles_y * tiles_x * 256 bytes"
                d.lut_out = lut.ctypes.data
                keep.append(lut)
        return arr, keep

    def apply_batch_raw(self, n, arr) -> int:
        return self.lib.dsdtm_clahe_apply_batch(self.handle, n, arr)

    def apply_batch(self, frames):
        """dsdtm_clahe_apply_batch: one submission, synchronous. Destinations (and lut_out) are written in place."""
        arr, keep = self.descs(frames)
        self.check(self.apply_batch_raw(len(frames), arr))
        del keep

    def apply(self, src, dst=None, clip_limit=DEFAULT_CLIP_LIMIT, tiles_x=DEFAULT_TILES, tiles_y=DEFAULT_TILES, lut_out=None):
        """dsdtm_clahe_apply. dst None: a new array of src's kind (numpy: numpy; torch: torch.empty_like). Returns dst."""
        if dst is None:
            if isinstance(src, np.ndarray):
                dst = np.empty(src.shape, np.uint8)
            else:
                import torch
                dst = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
                if dst.is_cuda:
                    torch.cuda.synchronize(dst.device)          # (the tensor exists; the add-on's stream is its own)
        arr, keep = self.descs([dict(src=src, dst=dst, clip_limit=clip_limit, tiles_x=tiles_x, tiles_y=tiles_y, lut_out=lut_out)])
        self.check(self.lib.dsdtm_clahe_apply(self.handle, arr))
        del keep
        return dst

    def luts(self, src, clip_limit=DEFAULT_CLIP_LIMIT, tiles_x=DEFAULT_TILES, tiles_y=DEFAULT_TILES) -> np.ndarray:
        """dsdtm_clahe_luts: (tiles_y, tiles_x, 256) uint8, the tables of E5."""
        out = np.empty((tiles_y or DEFAULT_TILES, tiles_x or DEFAULT_TILES, 256), np.uint8)
        arr, keep = self.descs([dict(src=src, clip_limit=clip_limit, tiles_x=tiles_x, tiles_y=tiles_y, lut_out=out)])
        self.check(self.lib.dsdtm_clahe_luts(self.handle, arr))
        del keep
        return out


class CLAHE:
    """What cv::createCLAHE returns, over a ClaheContext (made at the first apply and kept)."""

    def __init__(self, clipLimit=DEFAULT_CLIP_LIMIT, tileGridSize=(DEFAULT_TILES, DEFAULT_TILES), device=0):
        self.clipLimit, self.tileGridSize, self.device, self._ctx = float(clipLimit), (int(tileGridSize[0]), int(tileGridSize[1])), device, None

    def apply(self, img, dst=None):
        """cv::CLAHE::apply(src, dst): the equalised image (tileGridSize is (columns, rows), as cv::Size)."""
        if self._ctx is None:
            self._ctx = ClaheContext(self.device)
        return self._ctx.apply(img, dst, self.clipLimit, self.tileGridSize[0], self.tileGridSize[1])


def createCLAHE(clipLimit=DEFAULT_CLIP_LIMIT, tileGridSize=(DEFAULT_TILES, DEFAULT_TILES), device=0) -> CLAHE:
    """cv::createCLAHE(clipLimit, tileGridSize) in the shape the reference's drivers use: createCLAHE(3.0, (8, 8)).apply(img)."""
    return CLAHE(clipLimit, tileGridSize, device)
