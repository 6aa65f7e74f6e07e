"""The worlds of tests/test_klt_cpu.py and tests/test_klt_gpu.py: small gray image pairs whose motion is known, and the helpers that run
klt_flow_host (dsdtm_amd/host/dsdtm_klt_host.hpp, behind tests/klt_host/shim.cpp) on them. Each world is checked with the restatement on
the CPU (test_klt_cpu.py) before the GPU tests trust it."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from dsdtm_amd import klt_restatement as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = [(0, 0), (3, -2), (6, 5)]
SIZES = {"160x120": (160, 120), "171x123": (171, 123), "640x480": (640, 480)}
MARGIN = 16
_LIBS = {}


@functools.lru_cache(maxsize=None)
def canvas(width, height, seed=7, sigma=3.0):
    """A smooth band-limited random texture, float64 in [0, 255], MARGIN pixels larger than the image on every side: white noise under
    a Gaussian low-pass of `sigma` pixels (in the frequency domain), stretched to the full range."""
    h, w = height + 2 * MARGIN, width + 2 * MARGIN
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    spec = np.fft.rfft2(rng.standard_normal((h, w))) * np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))
    t = np.fft.irfft2(spec, s=(h, w))
    t = (t - t.min()) / (t.max() - t.min())
    return 255.0 * t


def crop(c, width, height, dx=0, dy=0):
    """The image whose content lies (dx, dy) pixels further right / down than in crop(c, w, h): integer shifts, no resampling."""
    return np.ascontiguousarray(np.clip(np.rint(c[MARGIN - dy:MARGIN - dy + height, MARGIN - dx:MARGIN - dx + width]), 0, 255).astype(np.uint8))


def shift_world(size, shift):
    w, h = SIZES[size]
    c = canvas(w, h)
    return crop(c, w, h), crop(c, w, h, *shift)


def sample_bilinear(c, x, y):
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    return (c[y0, x0] * (1 - fx) * (1 - fy) + c[y0, x0 + 1] * fx * (1 - fy) + c[y0 + 1, x0] * (1 - fx) * fy + c[y0 + 1, x0 + 1] * fx * fy)


WARP_H = np.array([[1.004, -0.006, 1.2], [0.006, 1.004, -0.9], [4e-6, -3e-6, 1.0]])      # small rotation + scale + perspective: current -> previous


def warp_world(size="160x120"):
    """(prev, cur, H): the pixel x of cur shows what prev shows at H x, so the truth of K9 (A = current -> B = previous) is H."""
    w, h = SIZES[size]
    c = canvas(w, h)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d = WARP_H[2, 0] * xs + WARP_H[2, 1] * ys + WARP_H[2, 2]
    u = (WARP_H[0, 0] * xs + WARP_H[0, 1] * ys + WARP_H[0, 2]) / d
    v = (WARP_H[1, 0] * xs + WARP_H[1, 1] * ys + WARP_H[1, 2]) / d
    cur = np.clip(np.rint(sample_bilinear(c, u + MARGIN, v + MARGIN)), 0, 255).astype(np.uint8)
    return crop(c, w, h), np.ascontiguousarray(cur), WARP_H.copy()


def flat_world():
    """A shift of (3, -2) with the left third of both images flat (one gray value): the grid points there fail the eigenvalue test (K5)."""
    prev, cur = shift_world("160x120", (3, -2))
    prev, cur = prev.copy(), cur.copy()
    prev[:, :56] = 128
    cur[:, :56] = 128
    return prev, cur


BLOCK = (192, 120, 416, 360)        # x0, y0, x1, y1 of the pasted block in the previous image of the moving-block world


def block_world():
    """640 x 480: the background moves by (6, 0); a block of another texture, covering about a third of the grid, moves by (-5, 0).
    -> (prev, cur, flags): flags[k] = 1 where grid point k's window lies on the block in both images, 0 where it lies on the background
    in both, 2 where it touches the block's edge (neither is asserted)."""
    w, h = SIZES["640x480"]
    c, c2 = canvas(w, h), canvas(w, h, seed=11)
    prev, cur = crop(c, w, h), crop(c, w, h, 6, 0)
    x0, y0, x1, y1 = BLOCK
    blk = crop(c2, w, h)
    prev[y0:y1, x0:x1] = blk[y0:y1, x0:x1]
    cur[y0:y1, x0 - 5:x1 - 5] = blk[y0:y1, x0:x1]
    g = KR.grid_points(w, h)
    flags = np.full(len(g), 2, np.uint8)
    for k, (x, y) in enumerate(g):
        if x0 + 12 <= x <= x1 - 18 and y0 + 8 <= y <= y1 - 8:
            flags[k] = 1
        elif x < x0 - 20 or x > x1 + 14 or y < y0 - 8 or y > y1 + 8:
            flags[k] = 0
    return prev, cur, flags


def border_points(width, height):
    """Points for dsdtm_klt_flow at 160 x 120 with 4 levels: windows that leave level 0, that leave only coarse levels, and that come
    within a pixel of the border, beside interior ones."""
    return np.array([(80, 60), (40.25, 30.75), (3, 60), (80, 2), (width - 3, 60), (80, height - 3),          # leave level 0
                     (6.5, 60), (6.4, 6.4), (width - 8.5, height - 8.5), (width - 7.6, 60),                # within a pixel of level 0's border
                     (12, 12), (20, 100), (140, 20), (30.5, 60.5), (width - 14, height - 14),              # leave only coarse levels
                     (100.125, 50.875), (60, 90)], np.float32)


def host_library(tmp_dir):
    """klt_flow_host / klt_pyramid_host / klt_grid_host behind C entries (tests/klt_host/shim.cpp)."""
    key = str(tmp_dir)
    if key not in _LIBS:
        so = os.path.join(key, "libklt_host.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-o", so, os.path.join(ROOT, "tests", "klt_host", "shim.cpp")], check=True)
        lib = C.CDLL(so)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        lib.klt_flow_host_c.restype, lib.klt_flow_host_c.argtypes = i, [vp, i, vp, i, i, i, i, i, vp, vp, i, i, d, d, vp, vp, vp, vp]
        lib.klt_pyramid_host_c.restype, lib.klt_pyramid_host_c.argtypes = i, [vp, i, i, i, i, vp]
        lib.klt_grid_host_c.restype, lib.klt_grid_host_c.argtypes = i, [i, i, i, i, vp, i]
        lib.klt_step_host_c.restype, lib.klt_step_host_c.argtypes = i, [vp, vp, i, i, i, i, i, i, vp, vp, vp, i, vp]
        _LIBS[key] = lib
    return _LIBS[key]


def host_flow(lib, prev, cur, points, guesses=None, window=10, levels=4, iterations=20, eps=0.03, min_eig=1e-4):
    prev, cur = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(cur, np.uint8)
    h, w = prev.shape
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 2))
    g = None if guesses is None else np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(-1, 2))
    n = len(pts)
    out = dict(points=np.zeros((n, 2), np.float32), status=np.zeros(n, np.uint8), iterations=np.zeros(n, np.int32), residual=np.zeros(n, np.float32))
    rc = lib.klt_flow_host_c(prev.ctypes.data, prev.strides[0], cur.ctypes.data, cur.strides[0], w, h, levels, n, pts.ctypes.data,
                             g.ctypes.data if g is not None else None, window, iterations, eps, min_eig, out["points"].ctypes.data,
                             out["status"].ctypes.data, out["iterations"].ctypes.data, out["residual"].ctypes.data)
    assert rc == 0
    return out


def host_step(lib, prev, cur, levels=4, gw=0, gh=0):
    """klt_step_host: dict(a, b, status, n_points, n_tracked)."""
    prev, cur = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(cur, np.uint8)
    h, w = prev.shape
    cap = 2048
    a, b, st, n = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32), np.zeros(cap, np.uint8), C.c_int(0)
    m = lib.klt_step_host_c(prev.ctypes.data, cur.ctypes.data, w, h, prev.strides[0], levels, gw, gh, a.ctypes.data, b.ctypes.data, st.ctypes.data, cap, C.byref(n))
    assert m >= 0
    return dict(a=a[:m], b=b[:m], status=st[:n.value], n_points=n.value, n_tracked=m)


def same_flow(a, b):
    """Bit for bit: points and residual compared as their 32-bit patterns."""
    return (np.array_equal(a["points"].view(np.uint32), b["points"].view(np.uint32)) and np.array_equal(a["status"], b["status"])
            and np.array_equal(a["iterations"], b["iterations"]) and np.array_equal(a["residual"].view(np.uint32), b["residual"].view(np.uint32)))


def apply_h(H, pts):
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    d = H[2, 0] * p[:, 0] + H[2, 1] * p[:, 1] + H[2, 2]
    return np.stack([(H[0, 0] * p[:, 0] + H[0, 1] * p[:, 1] + H[0, 2]) / d, (H[1, 0] * p[:, 0] + H[1, 1] * p[:, 1] + H[1, 2]) / d], 1)
