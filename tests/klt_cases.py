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


# ---- saturated contrast: window sums past 2^31 (integer totals) and 2^32 (right-hand sides) ------------------------------------------

def checker_world(shift=(1, 0)):
    """160 x 120: a checkerboard of 2 x 2 blocks of 0 / 255, the current image `shift` pixels further right / down. Every Scharr value on
    it is 0 or +-2550; at window 21 a tracked point's s11 = s22 = 2 867 602 500 > 2^31 and its first t1 is -+4 806 648 000 (the sign is
    the shift's): beyond 32 bits both ways with (1, 0) and (-1, 0) together (test_klt_cpu.py asserts these)."""
    ys, xs = np.mgrid[0:120 + 2 * MARGIN, 0:160 + 2 * MARGIN]
    c = 255.0 * ((xs // 2 + ys // 2) % 2)
    return crop(c, 160, 120), crop(c, 160, 120, *shift)


def block_noise_world(seed=3, shift=(1, 0)):
    """160 x 120: random 2 x 2 blocks of 0 / 255, shifted. Its gradients reach the largest value K2 allows, |dx| = 4080."""
    b = np.random.default_rng(seed).integers(0, 2, (60 + MARGIN, 80 + MARGIN))
    c = 255.0 * np.kron(b, np.ones((2, 2)))
    return crop(c, 160, 120), crop(c, 160, 120, *shift)


def saturated_worlds():
    return [("checker (1, 0)", *checker_world()), ("checker (-1, 0)", *checker_world((-1, 0))),
            ("noise (1, 0)", *block_noise_world()), ("noise (-1, 1)", *block_noise_world(shift=(-1, 1)))]


def saturated_points(window, width=160, height=120):
    """Points for one level-0 window size. The first tap is q - (window - 1) / 2, so which points have a zero fraction depends on the
    window's parity: whole and half positions are both here (fx = 0 / fy = 0 / both for either parity), both fractions at 31 / 32 for
    either parity, an unrelated fraction, and the border of K4 on level 0: the first and the last admissible positions (the last is
    1 / 32 before the bound: floor), and the first positions K4 rejects on each side."""
    half, e = (window - 1) * 0.5, 0.03125
    x0, y0, x1, y1 = 1 + half, 1 + half, width - 1 - window + half, height - 1 - window + half          # admissible: x0 <= x < x1
    return np.array([(80, 60), (80.5, 60.5), (80, 60.5), (80.5, 60), (40.96875, 30.96875), (40.46875, 30.46875), (100.25, 44.75),
                     (x0, y0), (x1 - e, y1 - e), (x1 - e, y0), (x0, y1 - e), (x0 - e, 60), (x1, 60), (80, y0 - e), (80, y1)], np.float32)


class _Observed(np.ndarray):
    """A window array of the restatement whose sums go through a function of the test's."""
    fn = None

    def sum(self, *a, **kw):
        return _Observed.fn(np.asarray(self))


class observed_sums:
    """with observed_sums(fn): every window array KR.bilinear returns, and so every product and difference of them, answers .sum() with
    fn(values). This is how a test sees what the restatement sums without the restatement knowing: the lanes' partial sums, and the
    mutant that wraps the totals to 32 bits. `gradients` collects the largest |value| of the gradient windows (shift W_BITS)."""

    def __init__(self, fn):
        self.fn, self.gradient_max = fn, 0

    def __enter__(self):
        self.saved = KR.bilinear

        def bilinear(img, ix, iy, n, w, shift):
            v = self.saved(img, ix, iy, n, w, shift)
            if shift == KR.W_BITS and v.size:
                self.gradient_max = max(self.gradient_max, int(np.abs(v).max()))
            return v.view(_Observed)
        KR.bilinear, _Observed.fn = bilinear, staticmethod(self.fn)
        return self

    def __exit__(self, *exc):
        KR.bilinear, _Observed.fn = self.saved, None
        return False


def lane_partials(values):
    """A window's values summed the way klt_kernel spreads them: pixel i (row major) belongs to lane i % 64. -> 64 Python-int partials."""
    flat = values.ravel().astype(np.int64)
    out = np.zeros(64, np.int64)
    np.add.at(out, np.arange(flat.size) % 64, flat)
    return out


# ---- every exit of the level loop and the iteration loop ----------------------------------------------------------------------------

EPS_ZERO = 1e-170        # its square is 0.0 in double: the step test fires on an exactly zero step alone. (An epsilon of 0 means the
#                          default to dsdtm_klt_flow; the restatement and klt_flow_host square what they are given, like the device.)
EXITS = ("prev_outside", "eigen", "cur_outside", "eps", "oscillation", "cap")


def exit_world():
    """-> (prev, cur, points, guesses, parameter sets). The flat world (a shift of (3, -2), the left third flat) with border_points,
    points on the flat third (eigen on every level), points whose previous window leaves the coarse levels only, and guesses that put
    the current window outside every level from the first iteration (+-1e5, the bound the entry admits, and just past the border) or
    let it drift out after one or more steps. Over the parameter sets every exit is taken on a coarse level and on level 0, and K7's
    last look fails (test_klt_cpu.py asserts it from the trace)."""
    prev, cur = flat_world()
    own = [(20, 60), (30, 20), (150.4, 60), (150.6, 60), (151.2, 60), (80, 6.6), (80, 7.4), (80, 8.2), (149, 100), (148, 30),
           (80, 60), (100, 50), (80, 60), (100, 50), (80, 60), (100, 50), (90, 70), (90, 70), (120, 40), (120, 40)]
    far = [(1e5, 1e5), (-1e5, -1e5), (1e5, 60), (100, -1e5), (152, 60), (100, 3), (148, 70), (90, 9), (150, 40), (140, 12)]
    pts = np.concatenate([border_points(160, 120), np.array(own, np.float32)])
    g = pts.copy()
    g[len(pts) - len(far):] = np.array(far, np.float32)
    sets = [dict(iterations=1), dict(iterations=2), dict(eps=EPS_ZERO), dict(), dict(iterations=3, eps=EPS_ZERO)]
    return prev, cur, pts, g, sets


# ---- windows on both sides of a pass of 64 lanes; one submission of unlike pairs ------------------------------------------------------

SWEEP_WINDOWS = (5, 7, 8, 9, 11, 12, 15, 16, 17, 20)        # areas 64 and 256 fill a pass, 81 and 289 put one pixel into a new one


def deepest_levels(window, width=160, height=120):
    """The most levels dsdtm_klt_flow accepts: the coarsest level holds one window and its ring (window + 3 pixels), five at the most."""
    levels = 1
    while levels < 5 and min((width - 1 >> levels) + 1, (height - 1 >> levels) + 1) >= window + 3:
        levels += 1
    return levels


def mixed_pairs():
    """Seven pairs for ONE dsdtm_klt_flow call: windows 4, 9, 16 and 21, one to five levels, 1, 3, 2048, 4, 5, 64 and 65 points (the
    largest, a 64 x 32 lattice on the smooth world, in the middle: the launch is sized by it, every other pair's waves leave early)."""
    smooth, far = shift_world("160x120", (3, -2)), shift_world("160x120", (6, 5))
    lattice = np.array([(12 + 2.125 * i, 10 + 3.0625 * j) for j in range(32) for i in range(64)], np.float32)
    b = border_points(160, 120)
    return [dict(prev=checker_world()[0], cur=checker_world()[1], points=saturated_points(21)[:1], window=21, levels=1),
            dict(prev=block_noise_world()[0], cur=block_noise_world()[1], points=saturated_points(16)[:3], window=16, levels=3),
            dict(prev=smooth[0], cur=smooth[1], points=lattice, window=9, levels=4),
            dict(prev=far[0], cur=far[1], points=b[:4], guesses=b[:4] + np.float32(4.5), window=9, levels=2, iterations=3),
            dict(prev=smooth[0], cur=smooth[1], points=b[6:11], window=4, levels=5),
            dict(prev=far[0], cur=far[1], points=KR.grid_points(160, 120, 17, 13), window=21, levels=2),
            dict(prev=smooth[0], cur=smooth[1], points=KR.grid_points(160, 120, 11, 20), window=16, levels=1, eps=EPS_ZERO)]


def restated(pair, klt=None, trace=None):
    """A pair of mixed_pairs() / a parameter set through the restatement."""
    kw = {k: v for k, v in pair.items() if k not in ("prev", "cur", "points")}
    return (klt or KR.Klt()).flow(pair["prev"], pair["cur"], pair["points"], trace=trace, **kw)


def device_pair(pair):
    """The same pair as dsdtm_amd.klt.KltContext.flow spells it (`epsilon`, not `eps`)."""
    d = dict(pair)
    if "eps" in d:
        d["epsilon"] = d.pop("eps")
    return d


# ---- klt_compact_kernel's edges: whole ballot rounds, the threshold of 10 survivors ---------------------------------------------------

def painted_world(rects, shift=(2, 1)):
    """160 x 120, a shift world with the rectangles (x0, y0, x1, y1) of both images painted one gray value: grid points there fail K5.
    (The shift goes right and down so that the grid's first row and column, a pixel or two inside K4's border, can survive.)"""
    w, h = SIZES["160x120"]
    c = canvas(w, h)
    prev, cur = crop(c, w, h), crop(c, w, h, *shift)
    for x0, y0, x1, y1 in rects:
        prev[y0:y1, x0:x1] = 128
        cur[y0:y1, x0:x1] = 128
    return prev, cur


# name -> (painted rectangles, grid_w, grid_h, n_points, n_tracked of the second step): the claims test_klt_cpu.py asserts.
# A grid of 128 points on 160 x 120 is 16 x 8 with grid_w = 9: its first column (x = 4) lies outside K4's border for a 10 x 10 window,
# so point 0 cannot survive there (a grid whose point 0 can needs grid_w, grid_h >= 12: 12 x 9 = 108 points at most). The pattern
# "survivors at lanes 0 and 63, holes between" is therefore on the one round of the 64-point grid (8 x 8, grid_w = 17) and on the SECOND
# round of a 128-point grid, behind a first round that is partly filled, so that a `base` that is not carried moves every survivor.
COMPACTION = {
    "64 points": ([], 17, 13, 64, None),
    "64 points, lanes 0 and 63 and holes": ([(0, 25, 160, 80)], 17, 13, 64, None),
    "65 points": ([], 11, 20, 65, None),
    "128 points, second round full": ([(0, 28, 70, 60)], 9, 13, 128, None),
    "128 points, second round empty": ([(70, 0, 160, 120)], 9, 13, 128, None),
    "128 points, second round lanes 0 and 63 and holes": ([(0, 25, 160, 80)], 9, 13, 128, None),
    "9 survivors": ([(0, 0, 52, 120), (96, 0, 160, 120)], 16, 30, 27, 9),
    "10 survivors": ([(0, 0, 64, 120), (96, 0, 160, 120)], 16, 20, 45, 10),
    "0 survivors": ([(0, 0, 160, 120)], 17, 13, 64, 0),
}


def compaction_step(name):
    """-> (prev, cur, grid_w, grid_h, the restatement's second step)."""
    rects, gw, gh, _, _ = COMPACTION[name]
    prev, cur = painted_world(rects)
    m = KR.KltModel(160, 120, gw=gw, gh=gh)
    m.step(prev)
    return prev, cur, gw, gh, m.step(cur)
