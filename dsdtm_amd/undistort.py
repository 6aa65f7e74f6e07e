"""libdsdtm_amd_undistort.so (include/dsdtm_amd_undistort.h) from Python: the ctypes binding of dsdtm_undistort_frames (cv::undistort of
raw gray / depth frames, n frames in one launch) and dsdtm_undistort_points (Frame::UndistortFeatures). The rules U1-U5 are this
project's definition (dsdtm_amd/undistort_restatement.py); parity with OpenCV's fixed-point remap is unpinned.

No fallback: loading raises if the library has not been built, a context raises without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon
from .local_map import Camera, camera_struct

LIB_NAME = "libdsdtm_amd_undistort.so"
# every symbol include/dsdtm_amd_undistort.h declares
SYMBOLS = ["dsdtm_undistort_create", "dsdtm_undistort_destroy", "dsdtm_undistort_last_error", "dsdtm_undistort_map_create",
           "dsdtm_undistort_map_destroy", "dsdtm_undistort_map_read", "dsdtm_undistort_frames", "dsdtm_undistort_points"]
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
MIN_SIDE, MAX_SIDE, MAX_FRAMES, MAX_POINTS, OUTSIDE = 8, 4096, 1024, 16384, -2**31


class Desc(C.Structure):
    """dsdtm_undistort_desc"""
    _fields_ = [("map", C.c_void_p), ("gray_src", C.c_void_p), ("gray_dst", C.c_void_p), ("depth_src", C.c_void_p), ("depth_dst", C.c_void_p),
                ("gray_src_stride", C.c_int32), ("gray_dst_stride", C.c_int32), ("depth_src_stride", C.c_int32), ("depth_dst_stride", C.c_int32)]


class UndistortError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"status {status}: {message}")
        self.status, self.message = status, message


def lib_path() -> str:
    return _addon.lib_path(LIB_NAME)


def _not_built(path):
    return FileNotFoundError(f"{path} has not been built (python dsdtm_amd/csrc/build.py --all); there is no fallback")


def load():
    """Load libdsdtm_amd_undistort.so. Raises if it has not been built (dsdtm_amd/csrc/build.py --all)."""
    vp, i = C.c_void_p, C.c_int
    return _addon.load_addon(LIB_NAME, {
        **_addon.context_signatures("dsdtm_undistort"),
        "dsdtm_undistort_map_create": (i, [vp, C.POINTER(Camera), vp, C.POINTER(vp)]),
        "dsdtm_undistort_map_destroy": (None, [vp]),
        "dsdtm_undistort_map_read": (i, [vp, vp, vp]),
        "dsdtm_undistort_frames": (i, [vp, i, C.POINTER(Desc)]),
        "dsdtm_undistort_points": (i, [vp, C.POINTER(Camera), vp, i, vp, vp, vp, vp])}, _not_built)


def _dist(dist):
    d = np.ascontiguousarray(np.asarray(dist, np.float32).reshape(5))
    return d


def _ptr_stride(a, itemsize):
    """(address, stride in elements, keep-alive) of an image: a numpy array (host), a torch tensor (device or pinned host), or a tuple
    (address, stride in elements) for anything else."""
    if a is None:
        return None, 0, None
    if isinstance(a, tuple):
        return int(a[0]), int(a[1]), None
    if isinstance(a, np.ndarray):
        assert a.ndim == 2 and a.itemsize == itemsize and a.strides[1] == itemsize, "an image is 2-D with contiguous rows"
        return a.ctypes.data, a.strides[0] // itemsize, a
    assert a.dim() == 2 and a.element_size() == itemsize and a.stride(1) == 1, "an image is 2-D with contiguous rows"       # a torch tensor
    return a.data_ptr(), a.stride(0), a


class UndistortMap:
    """A dsdtm_undistort_map: U1 for one camera, resident on the context's device."""

    def __init__(self, ctx, cam, dist):
        self.ctx, self.cam, self.dist = ctx, camera_struct(cam), _dist(dist)
        self.width, self.height = self.cam.width, self.cam.height
        h = C.c_void_p()
        ctx.check(ctx.lib.dsdtm_undistort_map_create(ctx.handle, C.byref(self.cam), self.dist.ctypes.data, C.byref(h)))
        self.handle = h

    def read(self) -> np.ndarray:
        """(height, width, 2) int32: the pairs (X, Y) at 1/32 pixel."""
        out = np.empty((self.height, self.width, 2), np.int32)
        self.ctx.check(self.ctx.lib.dsdtm_undistort_map_read(self.ctx.handle, self.handle, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.dsdtm_undistort_map_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UndistortContext(_addon.AddonContext):
    """A dsdtm_undistort_ctx: its own stream and staging block on one device. One per calling thread."""
    PREFIX, ERROR, load = "dsdtm_undistort", UndistortError, staticmethod(load)

    def make_map(self, cam, dist) -> UndistortMap:
        """dsdtm_undistort_map_create: cam has fx fy cx cy width height, dist = (k1, k2, p1, p2, k3)."""
        return UndistortMap(self, cam, dist)

    def descs(self, frames):
        """The dsdtm_undistort_desc array of `frames`: dicts of map, gray_src, gray_dst and, optionally, depth_src, depth_dst; an image is
        a 2-D numpy array (host memory), a 2-D torch tensor (device or pinned host memory) or (address, stride in elements).
        Returns (array, what must stay alive)."""
        arr = (Desc * max(len(frames), 1))()
        keep = []
        for k, f in enumerate(frames):
            d = arr[k]
            d.map = f["map"].handle if f.get("map") is not None else None
            for name, size in (("gray_src", 1), ("gray_dst", 1), ("depth_src", 2), ("depth_dst", 2)):
                p, s, alive = _ptr_stride(f.get(name), size)
                setattr(d, name, p)
                setattr(d, name + "_stride", s)
                keep.append(alive)
            keep.append(f.get("map"))
        return arr, keep

    def undistort_frames_raw(self, n, arr) -> int:
        return self.lib.dsdtm_undistort_frames(self.handle, n, arr)

    def undistort_frames(self, frames):
        """dsdtm_undistort_frames: one submission, synchronous. Destinations are written in place."""
        arr, keep = self.descs(frames)
        self.check(self.undistort_frames_raw(len(frames), arr))
        del keep

    def undistort_points(self, cam, dist, px_in, skip=None, bearing_out=None):
        """dsdtm_undistort_points: (px_out (n, 2) float32, bearing_out (n, 3) float64); rows of bearing_out of skipped pixels keep what
        they held (zeros if none is given)."""
        px_in = np.ascontiguousarray(np.asarray(px_in, np.float32).reshape(-1, 2))
        n = len(px_in)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip, np.uint8).reshape(n))
        out = np.empty((n, 2), np.float32)
        b = np.zeros((n, 3), np.float64) if bearing_out is None else bearing_out
        assert b.dtype == np.float64 and b.shape == (n, 3) and b.flags.c_contiguous
        cs, d = camera_struct(cam), _dist(dist)
        self.check(self.lib.dsdtm_undistort_points(self.handle, C.byref(cs), d.ctypes.data, n, px_in.ctypes.data, None if sk is None else sk.ctypes.data,
                                                   out.ctypes.data, b.ctypes.data))
        return out, b
