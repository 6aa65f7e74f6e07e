"""The worlds of tests/test_framediff_cpu.py and tests/test_framediff_gpu.py: seeded pairs of gray images with an H, a threshold, a
maxval and features, at the smallest sizes that can still go wrong — 64x16 (one word of the bit-plane, one band), 70x37 and 129x45
(ragged last words of 6 and 1 pixels), 127x20 (63), 200x80 (bands of 32 rows: seams at rows 32 and 64; of 16: 16, 32, 48, 64) and
640x480 once — and the helper that runs frame_diff_host (dsdtm_amd/host/dsdtm_framediff_host.hpp, behind tests/framediff_host/shim.cpp)
on them. Each world is held to the restatement on the CPU (test_framediff_cpu.py) before the GPU tests trust it."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from dsdtm_amd import framediff_restatement as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.eye(3).reshape(9)
_LIBS = {}


def texture(width, height, seed):
    """Noise under a 3x3 box: neighbouring pixels differ by tens of gray values, so a 1/32-pixel step of the map shows."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 256, (height + 2, width + 2)).astype(np.int64)
    s = sum(n[dy:dy + height, dx:dx + width] for dy in range(3) for dx in range(3))
    lo, hi = s.min(), s.max()
    return ((s - lo) * 255 // (hi - lo)).astype(np.uint8)


def drawn(width, height, rects):
    """H identity and b = 0: t IS the drawn pattern (a = 255 inside the rectangles (x0, y0, x1, y1), x1 and y1 exclusive)."""
    a = np.zeros((height, width), np.uint8)
    for x0, y0, x1, y1 in rects:
        a[y0:y1, x0:x1] = 255
    return a, np.zeros((height, width), np.uint8)


def _features(width, height, seed, n=24):
    rng = np.random.default_rng(seed)
    f = np.stack([rng.uniform(0, width - 1, n), rng.uniform(0, height - 1, n)], 1).astype(np.float32)
    f[0], f[1], f[2] = (0, 0), (width - 1, height - 1), (width - 1.5, height - 1.5)
    return f


def _case(name, a, b, H=IDENTITY, flags=0, threshold=FR.THRESHOLD, maxval=0, features=None, same=False):
    h, w = a.shape
    return dict(name=name, a=a, b=a if same else b, H=np.asarray(H, np.float64).reshape(9).copy(), flags=flags, threshold=threshold, maxval=maxval,
                features=_features(w, h, len(name)) if features is None else np.asarray(features, np.float32).reshape(-1, 2), same=same)


def edge_rects(w, h):
    """3-wide strips along the four edges (clear of the corners) and 3x3 blocks in the four corners."""
    strips = [(0, 8, 3, h - 8), (w - 3, 8, w, h - 8), (8, 0, w - 8, 3), (8, h - 3, w - 8, h)]
    corners = [(0, 0, 3, 3), (w - 3, 0, w, 3), (0, h - 3, 3, h), (w - 3, h - 3, w, h)]
    return strips, corners


def translation(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty, 0, 0, 1], np.float64)


ROTATION = np.array([1.02 * np.cos(0.05), -1.02 * np.sin(0.05), 1.7, 1.02 * np.sin(0.05), 1.02 * np.cos(0.05), -2.3, 0, 0, 1], np.float64)
PERSPECTIVE = np.array([1, 0.01, 0.5, -0.02, 1, 0.25, -0.025, 0.001, 1], np.float64)        # as M: W = 1 - x / 40 + y / 1000 crosses 0 at x = 40
FAR = translation(10000.0, -10000.0)
HUGE = translation(1e300, -1e300)
NAN_M = np.array([1e308, 0, 0, 0, 1, 0, 1, 0, -20], np.float64)      # as M: W = 0 at x = 20 where X0 is infinite: 0 * inf, "outside"
SIZES = [(64, 16), (70, 37), (129, 45), (200, 80)]


@functools.lru_cache(maxsize=None)
def _built():
    out = []
    # ---- morphology edges: t is drawn
    out.append(_case("blocks 4x4 5x5 6x6", *drawn(200, 80, [(10, 10, 14, 14), (40, 8, 45, 13), (70, 8, 76, 14)])))
    for w, h in SIZES:
        strips, corners = edge_rects(w, h)
        out.append(_case(f"edge strips {w}x{h}", *drawn(w, h, strips)))
        out.append(_case(f"corner blocks {w}x{h}", *drawn(w, h, corners)))
    out.append(_case("band seams", *drawn(200, 80, [(10, 30, 15, 35), (30, 62, 35, 67), (50, 14, 55, 19), (70, 46, 75, 51), (90, 28, 96, 38)])))
    out.append(_case("word seams", *drawn(200, 80, [(62, 10, 67, 15), (126, 30, 131, 35), (60, 60, 70, 66), (190, 62, 195, 67)])))
    out.append(_case("word seam 129x45", *drawn(129, 45, [(62, 20, 67, 25), (124, 30, 129, 35), (126, 4, 129, 14)])))
    # ---- ragged width: foreground ending exactly at width - 1
    for w, h in ((129, 45), (70, 37), (127, 20)):
        out.append(_case(f"ragged row {w}x{h}", *drawn(w, h, [(w - 20, 6, w, 11), (w - 9, h - 5, w, h)])))
    # ---- warp: each H direct and as the inverse map
    hs = [("translation 37/32 -13/32", translation(37 / 32, -13 / 32)), ("translation 1.3 0.77", translation(1.3, 0.77)),
          ("halves 1/64 3/64", translation(1 / 64, 3 / 64)), ("rotation with scale", ROTATION), ("perspective through W = 0", PERSPECTIVE),
          ("everything outside", FAR), ("entries of 1e300", HUGE)]
    for k, (w, h) in enumerate(((70, 37), (129, 45))):
        a, b = texture(w, h, 11 + k), texture(w, h, 23 + k)
        for name, H in hs:
            for flags in (0, FR.INVERSE_MAP):
                # (the perspective world is written as M: its direct variant passes the inverse, so that F1 arrives at a W that crosses 0)
                Hd = FR.invert(H) if name.startswith("perspective") and not flags else H
                out.append(_case(f"{name} {w}x{h} {'inverse' if flags else 'direct'}", a, b, Hd, flags, threshold=30))
    out.append(_case("nan in the map 70x37 inverse", texture(70, 37, 5), texture(70, 37, 6), NAN_M, FR.INVERSE_MAP, threshold=30))
    # ---- threshold, maxval, features
    a, b = np.full((37, 70), 100, np.uint8), np.full((37, 70), 100, np.uint8)
    a[8:16, 40:48] = 150            # d = 50: not above the threshold
    a[8:16, 17:25] = 151            # d = 51: t on 17..24 x 8..15, f on 15..26 x 6..17
    feats = [(26.5, 10), (27.5, 10), (14.5, 10), (13.5, 10), (20, 17.5), (20, 16.5), (20, 5.5), (44, 12), (-0.4, -0.5), (69.49, 36.5)]
    out.append(_case("threshold 50 and 51 maxval 200", a, b, features=feats))
    out.append(_case("threshold 50 and 51 maxval 255", a, b, maxval=255, features=feats))
    out.append(_case("threshold 0 maxval 1", texture(64, 16, 3), texture(64, 16, 4), threshold=0, maxval=1))
    out.append(_case("threshold 254", *drawn(64, 16, [(20, 4, 30, 12)]), threshold=254, maxval=255))
    # ---- the literal line 45: b = a, the same pointer
    out.append(_case("literal line 45", texture(129, 45, 9), None, translation(3, 2), threshold=20, maxval=255, same=True))
    # ---- 640x480 once
    a, b = texture(640, 480, 1).copy(), texture(640, 480, 1).copy()
    a[200:260, 300:380] = np.minimum(a[200:260, 300:380].astype(np.int64) + 90, 255).astype(np.uint8)
    out.append(_case("640x480", a, b, ROTATION, threshold=40, maxval=255, features=_features(640, 480, 77, 300)))
    return out


def all_cases():
    return _built()


def names():
    return [c["name"] for c in _built()]


def by_name(name):
    return next(c for c in _built() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's answer for a case: computed once, shared, never changed."""
    c = by_name(name)
    return FR.FrameDiff().step(c["a"], c["b"], c["H"], c["flags"], c["threshold"], c["maxval"], c["features"])


def run_with(model, c):
    return model.step(c["a"], c["b"], c["H"], c["flags"], c["threshold"], c["maxval"], c["features"])


STAGES = ("warped", "t", "e", "o", "f", "mask", "flags")


def same_answer(x, y):
    return (all(np.array_equal(x[s], y[s]) for s in STAGES) and np.array_equal(x["M"].view(np.uint64), y["M"].view(np.uint64))
            and x["n_foreground"] == y["n_foreground"] and x["n_flagged"] == y["n_flagged"])


# ---- frame_diff_host behind a C entry

def host_library(tmp_dir):
    key = str(tmp_dir)
    if key not in _LIBS:
        so = os.path.join(key, "libframediff_host.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-o", so, os.path.join(ROOT, "tests", "framediff_host", "shim.cpp")], check=True)
        lib = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        lib.frame_diff_host_c.restype, lib.frame_diff_host_c.argtypes = i, [vp, i, vp, i, i, i, vp, i, i, i, vp, i, i, vp, vp, vp, vp, vp]
        lib.warp_perspective_host_c.restype, lib.warp_perspective_host_c.argtypes = i, [vp, i, i, i, vp, i, vp, i, vp]
        _LIBS[key] = lib
    return _LIBS[key]


def host_step(lib, c):
    """frame_diff_host on a case: the dict of FR.FrameDiff.step, or None where F1 refuses."""
    a, b = np.ascontiguousarray(c["a"]), np.ascontiguousarray(c["b"])
    h, w = a.shape
    H = np.ascontiguousarray(c["H"], np.float64)
    f = np.ascontiguousarray(c["features"], np.float32)
    mask, flags = np.full((h, w), 0xA5, np.uint8), np.full(len(f), 0xA5, np.uint8)
    stages = np.zeros((5, h, w), np.uint8)
    M, counts = np.zeros(9, np.float64), np.zeros(2, np.int32)
    ok = lib.frame_diff_host_c(a.ctypes.data, a.strides[0], b.ctypes.data, b.strides[0], w, h, H.ctypes.data, c["flags"], c["threshold"], c["maxval"],
                               mask.ctypes.data, w, len(f), f.ctypes.data, flags.ctypes.data, stages.ctypes.data, M.ctypes.data, counts.ctypes.data)
    if not ok:
        return None
    return dict(M=M, warped=stages[0], t=stages[1].astype(bool), e=stages[2].astype(bool), o=stages[3].astype(bool), f=stages[4].astype(bool),
                mask=mask, flags=flags, n_foreground=int(counts[0]), n_flagged=int(counts[1]))
