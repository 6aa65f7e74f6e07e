"""The cases the contour-box tests share (tests/test_mcd_cpu.py, tests/test_mcd_gpu.py): hand-made masks with their expected results
(computed by hand, not by any implementation), random masks, the larger shapes of the GPU tests, the loaders of the C twin
(tests/contour_restatement.c) and of mcd_box_host (dsdtm_amd/host/dsdtm_mcd_host.hpp), and the whole-Run chain over the worlds of
tests/motion_cases.py (which this module does not modify).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from dsdtm_amd import contour_restatement as CR
from tests import motion_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((16, 16), (23, 17), (37, 29), (48, 40))          # width, height
DENSITIES = (0.05, 0.3, 0.45, 0.6)                         # 0.45: near the 8-connected percolation point


def _blank(w=16, h=16):
    return np.zeros((h, w), np.uint8)


def hand_cases():
    """name -> (mask 16x16, dict(area2, box, n_components)). Every expectation is worked out by hand in the comment beside it."""
    cases = {}

    def add(name, m, area2, box, n):
        cases[name] = (m, dict(area2=area2, box=list(box), n_components=n))

    m = _blank(); m[4:9, 3:10] = 255                       # filled 7 x 5: the border runs through the pixel centres, (7 - 1)(5 - 1) = 24
    add("rectangle", m, 2 * 6 * 4, (3, 4, 7, 5), 1)
    m = _blank(); m[5, 5] = 255
    add("pixel", m, 0, (0, 0, 0, 0), 1)
    m = _blank(); m[3, 2:10] = 255
    add("line_horizontal", m, 0, (0, 0, 0, 0), 1)
    m = _blank(); m[2:13, 7] = 255
    add("line_vertical", m, 0, (0, 0, 0, 0), 1)
    m = _blank(); m[np.arange(2, 11), np.arange(2, 11)] = 255
    add("line_diagonal", m, 0, (0, 0, 0, 0), 1)
    m = _blank(); m[np.arange(2, 11), 12 - np.arange(2, 11)] = 255
    add("line_antidiagonal", m, 0, (0, 0, 0, 0), 1)
    m = _blank(); m[4, 4] = m[5, 4] = m[5, 5] = 7; m[12, 12] = 3      # the triangle (4,4) (4,5) (5,5): area 1/2; a dot elsewhere keeps its byte
    add("l3", m, 1, (4, 4, 2, 2), 2)
    m = _blank(); m[6, 5:8] = 255; m[5:8, 6] = 255           # the diamond through the four arms: diagonals 2 x 2, area 2
    add("plus5", m, 4, (5, 5, 3, 3), 1)
    m = _blank(); m[2:12, 2:12] = 255; m[4:10, 4:10] = 0; m[6:8, 6:8] = 255      # the ring's OUTER border: 9 x 9
    add("ring_with_block", m, 2 * 9 * 9, (2, 2, 10, 10), 2)
    m = _blank(); m[1:5, 1:5] = 255; m[9:13, 9:13] = 255     # 3 x 3 each: the raster-first one
    add("two_equal_squares", m, 2 * 3 * 3, (1, 1, 4, 4), 2)
    m = _blank(); m[2:5, 2:5] = 255; m[5:8, 5:8] = 255       # joined at (4,4)-(5,5) only: one component, the link walked twice: 2 x 2 + 2 x 2
    add("diagonal_join", m, 2 * (4 + 4), (2, 2, 6, 6), 1)
    m = _blank(); m[0, :] = m[15, :] = 255; m[:, 0] = m[:, 15] = 255
    add("frame_on_all_edges", m, 2 * 15 * 15, (0, 0, 16, 16), 1)
    add("empty", _blank(), 0, (0, 0, 0, 0), 0)
    add("full", np.full((16, 16), 255, np.uint8), 2 * 15 * 15, (0, 0, 16, 16), 1)
    return cases


def expected_boxed(mask, box):
    """C5 by hand: the mask with box = x, y, w, h set to 255."""
    out = mask.copy()
    x, y, w, h = box
    out[y:y + h, x:x + w] = 255
    return out


def random_masks():
    """[(name, mask)]: every size at every density, bytes 255 / 0."""
    out = []
    for k, (w, h) in enumerate(SIZES):
        for j, d in enumerate(DENSITIES):
            rng = np.random.default_rng(1000 + 10 * k + j)
            out.append((f"random_{w}x{h}_{d}", np.where(rng.random((h, w)) < d, 255, 0).astype(np.uint8)))
    return out


def serpentine(w=131, h=67):
    """One component that winds through every even row: it crosses every block of pixels and its labels merge in long chains."""
    m = np.zeros((h, w), np.uint8)
    m[0::2, :] = 255
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 255
    return m


def checkerboard(n=64):
    yy, xx = np.mgrid[0:n, 0:n]
    return (((xx + yy) % 2 == 0) * 255).astype(np.uint8)


def u_trap(w=48, h=40):
    """A U of 2-pixel walls (bounding box 20 x 20: the larger bound, the smaller area) before a compact 12 x 12 square, which wins."""
    m = np.zeros((h, w), np.uint8)
    m[2:22, 2:4] = 255; m[2:22, 20:22] = 255; m[20:22, 2:22] = 255
    m[24:36, 30:42] = 255
    return m


def blob_with_salt(w=640, h=480, seed=9):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((((xx - 300) / 90.0) ** 2 + ((yy - 220) / 60.0) ** 2 + 0.15 * np.sin(xx / 7.0) * np.cos(yy / 5.0)) < 1.0)
    m = m | (rng.random((h, w)) < 0.01)
    m[100:103, 500:560] = True
    return (m * 255).astype(np.uint8)


# ---- the C twin and the host function, compiled into a scratch directory ----
_LIBS = {}


def c_twin(tmp_dir):
    key = ("twin", str(tmp_dir))
    if key not in _LIBS:
        so = os.path.join(str(tmp_dir), "libcontour_restatement.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=c11", "-Wall", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "contour_restatement.c")], check=True)
        lib = C.CDLL(so)
        lib.contour_box.restype, lib.contour_box.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIBS[key] = lib
    return _LIBS[key]


def host_function(tmp_dir):
    """mcd_box_host behind a C entry (tests/mcd_host/shim.cpp)."""
    key = ("host", str(tmp_dir))
    if key not in _LIBS:
        so = os.path.join(str(tmp_dir), "libmcd_box_host.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", so,
                        os.path.join(ROOT, "tests", "mcd_host", "shim.cpp")], check=True)
        lib = C.CDLL(so)
        lib.mcd_box_host_c.restype, lib.mcd_box_host_c.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIBS[key] = lib
    return _LIBS[key]


def run_c(fn, mask):
    """A C implementation (contour_box or mcd_box_host_c) on a mask: dict(box, area2, n_components, boxed)."""
    mask = np.ascontiguousarray(mask, np.uint8)
    h, w = mask.shape
    boxed = np.full((h, w), 0xA5, np.uint8)
    box, area2, n = (C.c_int32 * 4)(), C.c_int64(), C.c_int32()
    rc = fn(mask.ctypes.data, w, h, w, boxed.ctypes.data, w, C.cast(box, C.c_void_p), C.cast(C.pointer(area2), C.c_void_p), C.cast(C.pointer(n), C.c_void_p))
    assert rc == 0
    return dict(box=list(box), area2=int(area2.value), n_components=int(n.value), boxed=boxed)


def same(a, b):
    """Bit-equality of two results: box, area2, count and every byte of the boxed mask."""
    return a["box"] == b["box"] and a["area2"] == b["area2"] and a["n_components"] == b["n_components"] and np.array_equal(a["boxed"], b["boxed"])


_RESTATED = {}


def restated(name, mask):
    """The restatement's result for a named mask, computed once and never modified."""
    if name not in _RESTATED:
        _RESTATED[name] = CR.ContourRestatement().run(mask)
    return _RESTATED[name]


# ---- the whole Run over the worlds of tests/motion_cases.py ----
_CHAINS = {}


def step_features(wd, mask, n=200, seed=77):
    """n feature positions around the mask's set pixels (the four corners and exact halves among them), as motion_cases.features places them."""
    w, h = wd["width"], wd["height"]
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(mask == 255)
    if len(xs) == 0:
        xs, ys = np.array([0, w - 1]), np.array([0, h - 1])
    x0, x1, y0, y1 = max(xs.min() - 3, 0), min(xs.max() + 3, w - 1), max(ys.min() - 3, 0), min(ys.max() + 3, h - 1)
    px = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], axis=1).astype(np.float32)
    px[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    half = np.floor(px[8:n // 2]) + 0.5
    px[8:n // 2] = np.minimum(half, [w - 1.5, h - 1.5])
    return px


def chain_of(name):
    """Per step of a world: the motion restatement's trace entry `t`, the features `px`, the contour restatement `c` on t["mask"], and the
    flags on the raw and on the boxed mask."""
    if name not in _CHAINS:
        wd, out = mc.world(name), []
        for s, t in enumerate(mc.trace_of(name)):
            px = step_features(wd, t["mask"])
            c = CR.ContourRestatement().run(t["mask"])
            out.append(dict(t=t, px=px, c=c, flags_raw=CR.features_on_mask(t["mask"], px), flags=CR.features_on_mask(c["boxed"], px)))
        _CHAINS[name] = out
    return _CHAINS[name]


def rectangle_steps(name):
    """The steps of a world at which a rectangle is drawn AND at least one feature's flag differs between the boxed and the raw mask."""
    return [s for s, e in enumerate(chain_of(name)) if e["c"]["area2"] > 0 and (e["flags"] != e["flags_raw"]).any()]
