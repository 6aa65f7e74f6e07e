"""The cases of tests/test_newkf_cpu.py and tests/test_newkf_gpu.py: small trackers for dsdtm_newkf_make (rules K1-K6 of
include/dsdtm_amd_newkf.h), each aimed at one branch, on the two smallest shapes at which the kernel can still go wrong: 96x64 with
cell 16 (24 cells: not a multiple of a wavefront) and 176x100 with cell 12 (a ragged last column and row). Built once (seeded) and
never changed by a test; the restated answers are computed once per session (answers())."""
import functools
import math
import struct

import numpy as np

from dsdtm_amd.keyframe_creation_restatement import NewKeyframeInput, NewKeyframeParams, create_keyframe
from tests.detector_restatement import circle_spans

CAM = (525.0, 525.5, 87.25, 49.5)          # fx, fy, cx, cy


def params(width, height, cell, max_fts, min_dist):
    return NewKeyframeParams(width, height, cell, int(math.ceil(width / cell)), int(math.ceil(height / cell)), max_fts, min_dist, 20.0)


SMALL = dict(width=96, height=64, cell=16)
RAGGED = dict(width=176, height=100, cell=12)


def pose(rng):
    """A rotation that is not the identity and a translation: [R|t], 12 doubles."""
    a, b = rng.uniform(-0.4, 0.4, 2)
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    return np.concatenate([Rz @ Ry, rng.uniform(-1, 1, (3, 1))], axis=1).reshape(12)


def random_cells(rng, prm, scores=(0.0, 5.0, 20.0, 20.5, 25.0, 25.0, 30.0, 30.0, 41.5, 77.0), nan=False):
    """One corner per cell inside its cell (clipped to the image), scores from a short list (ties; 20 itself does not pass)."""
    G = prm.grid_cols * prm.grid_rows
    k = np.arange(G)
    x = np.minimum((k % prm.grid_cols) * prm.cell_size + rng.integers(0, prm.cell_size, G), prm.width - 1).astype(np.int32)
    y = np.minimum((k // prm.grid_cols) * prm.cell_size + rng.integers(0, prm.cell_size, G), prm.height - 1).astype(np.int32)
    s = rng.choice(np.asarray(scores, np.float32), G).astype(np.float32)
    if nan:
        s[rng.integers(0, G, 3)] = np.nan
    return s, x, y, rng.integers(0, 3, G).astype(np.int32)


def random_depth(rng, prm, zeros=0.3):
    d = rng.integers(300, 60000, (prm.height, prm.width)).astype(np.uint16)
    d[rng.random((prm.height, prm.width)) < zeros] = 0
    return d


def random_existing(rng, prm, n, first_point_index):
    """n features: pixels on halves too (cvRound to even), some without a point, some initial (those have a point index)."""
    px = np.stack([rng.uniform(-3, prm.width + 3, n), rng.uniform(-3, prm.height + 3, n)], axis=1)
    px[::3] = np.floor(px[::3]) + 0.5
    px = px.astype(np.float32)
    initial = (rng.random(n) < 0.5).astype(np.uint8)
    has_point = np.maximum(initial, (rng.random(n) < 0.5).astype(np.uint8))
    point_index = np.where(has_point, rng.integers(0, max(first_point_index, 1), n), -1).astype(np.int32)
    b = rng.normal(size=(n, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return dict(px_xy=px, level=rng.integers(0, 4, n).astype(np.int32), bearing=b, has_point=has_point, initial=initial, point_index=point_index)


def _case(name, prm, inp, detect_comparable):
    return dict(name=name, prm=prm, inp=inp, detect_comparable=detect_comparable)


def _random_case(name, seed, shape, n_existing, max_fts, min_dist, dyn=False, nan=False, zeros=0.3):
    rng = np.random.default_rng(seed)
    prm = params(shape["width"], shape["height"], shape["cell"], max_fts, min_dist)
    s, x, y, l = random_cells(rng, prm, nan=nan)
    first = 1000 + seed
    inp = NewKeyframeInput(s, x, y, l, random_depth(rng, prm, zeros), 5000.0, pose(rng), first, **random_existing(rng, prm, n_existing, first))
    if dyn:
        inp.dyn_mask = rng.choice(np.asarray([0, 199, 200, 201, 255], np.uint8), (prm.height, prm.width))
    # tests/detector_restatement.detect knows neither the dynamic mask (it only matters with existing features) nor a NaN score
    return _case(name, prm, inp, detect_comparable=not nan and not (dyn and n_existing > 0))


def _edge_case():
    """One existing feature with a point in the middle; corners ON the rim of its disc (|dx| = hw) and one pixel outside (hw + 1), for
    several |dy|, and corners on the rim of an ACCEPTED corner's disc. All scores differ: the walk's order is the list's."""
    prm = params(**RAGGED, max_fts=400, min_dist=9)
    G = prm.grid_cols * prm.grid_rows
    cx, cy = 60, 50
    hw = circle_spans(prm.min_dist)
    pts = []
    for dy in (0, 3, 6, 8, 9):
        pts += [(cx + hw[dy], cy + dy), (cx + hw[dy] + 1, cy - dy), (cx - hw[dy], cy - dy), (cx - hw[dy] - 1, cy + dy)]
    pts += [(cx, cy + 10), (cx, cy - 9)]
    hc = circle_spans(prm.cell_size)
    ax, ay = 140, 50                                  # the first corner of the walk; the next ones sit on / off its rim
    rim = [(ax, ay)]
    for dy in (0, 5, 11, 12):
        rim += [(ax + hc[dy], ay + dy), (ax - hc[dy] - 1, ay - dy)]
    rim += [(ax, ay + 13)]
    s = np.zeros(G, np.float32)
    x, y = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for i, (px, py) in enumerate(rim + pts):
        s[i], x[i], y[i] = 500.0 - i, px, py
    rng = np.random.default_rng(7)
    ex = dict(px_xy=np.asarray([[cx + 0.25, cy - 0.25], [20.0, 20.0]], np.float32), level=np.zeros(2, np.int32),
              bearing=np.asarray([[0, 0, 1.0], [0, 0, 1.0]]), has_point=np.asarray([1, 0], np.uint8), initial=np.asarray([1, 0], np.uint8),
              point_index=np.asarray([5, -1], np.int32))
    inp = NewKeyframeInput(s, x, y, np.zeros(G, np.int32), random_depth(rng, prm, 0.0), 5000.0, pose(rng), 40, **ex)
    return _case("disc_edges", prm, inp, True)


def _border_case():
    """Existing features whose discs are clipped by every border (centres at and outside the corners of the image), corners next to them."""
    prm = params(**SMALL, max_fts=400, min_dist=10)
    rng = np.random.default_rng(11)
    s, x, y, l = random_cells(rng, prm, scores=(21.0, 22.0, 23.0, 24.0, 90.0))
    x[:6], y[:6] = [0, 95, 0, 95, 7, 88], [0, 0, 63, 63, 7, 56]
    s[:6] = [100, 99, 98, 97, 96, 95]
    px = np.asarray([[-2.0, -2.0], [97.0, 1.0], [0.0, 66.0], [95.0, 63.0], [48.0, -9.0]], np.float32)
    ex = dict(px_xy=px, level=np.zeros(5, np.int32), bearing=np.tile([0, 0, 1.0], (5, 1)), has_point=np.ones(5, np.uint8),
              initial=np.zeros(5, np.uint8), point_index=np.arange(5, dtype=np.int32))
    inp = NewKeyframeInput(s, x, y, l, random_depth(rng, prm), 1000.0, pose(rng), 5, **ex)
    return _case("discs_clipped_by_border", prm, inp, True)


def _depth_case():
    """The lift's branches: a corner whose own depth is 0 with each of the four neighbours as the FIRST non-zero one, one with all five 0,
    one on each border of the image (neighbours outside), and existing features that are not initial (lifted) beside initial ones."""
    prm = params(**RAGGED, max_fts=400, min_dist=3)
    G = prm.grid_cols * prm.grid_rows
    rng = np.random.default_rng(13)
    depth = rng.integers(300, 60000, (prm.height, prm.width)).astype(np.uint16)
    order = [(-1, 0), (0, -1), (1, 0), (0, 1)]
    corners = []
    for first in range(4):                            # the neighbours before `first` are 0 too
        px, py = 20 + 30 * first, 20
        depth[py, px] = 0
        for ddx, ddy in order[:first]:
            depth[py + ddy, px + ddx] = 0
        corners.append((px, py))
    depth[60, 20] = depth[60, 19] = depth[59, 20] = depth[60, 21] = depth[61, 20] = 0
    corners.append((20, 60))
    for px, py in ((0, 50), (175, 50), (80, 0), (80, 99), (0, 0), (175, 99)):      # borders and corners of the image: own depth 0
        depth[py, px] = 0
        corners.append((px, py))
    # ... and the neighbours inside the image that come BEFORE the one outside, so that the walk reaches it
    depth[0, 79] = 0                                    # (80, 0): (-1, 0) is 0, (0, -1) is outside, (1, 0) decides
    depth[50, 174] = depth[49, 175] = 0                 # (175, 50): (1, 0) is outside, (0, 1) decides
    depth[99, 79] = depth[98, 80] = depth[99, 81] = 0   # (80, 99): (0, 1) is outside: none
    depth[99, 174] = depth[98, 175] = 0                 # (175, 99): the other two are outside: none
    depth[80, 140] = 0                                  # an ordinary one: its left neighbour decides
    corners.append((140, 80))
    s = np.zeros(G, np.float32)
    x, y = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for i, (px, py) in enumerate(corners):
        s[3 * i], x[3 * i], y[3 * i] = 100.0 + i, px, py
    depth[70, 110] = 0                                  # an existing non-initial feature on a zero: neighbour (-1, 0)
    depth[30, 150] = depth[30, 149] = depth[29, 150] = depth[30, 151] = depth[31, 150] = 0      # ... and one that finds none
    ex = dict(px_xy=np.asarray([[110.4, 69.6], [150.0, 30.0], [50.5, 80.5], [120.0, 40.0], [-4.0, 200.0]], np.float32),
              level=np.asarray([0, 1, 2, 3, 0], np.int32), bearing=np.tile([0.6, 0, 0.8], (5, 1)),
              has_point=np.asarray([0, 0, 0, 1, 0], np.uint8), initial=np.asarray([0, 0, 0, 1, 0], np.uint8),
              point_index=np.asarray([-1, -1, -1, 17, -1], np.int32))
    inp = NewKeyframeInput(s, x, y, (np.arange(G) % 3).astype(np.int32), depth, 5000.0, pose(rng), 123, **ex)
    return _case("depth_branches", prm, inp, True)


def _outside_case():
    """Corners outside the image and a level outside 0..15 are skipped (cells in host memory would be refused when negative: these are
    too LARGE, which only the walk sees)."""
    prm = params(**SMALL, max_fts=400, min_dist=5)
    rng = np.random.default_rng(17)
    s, x, y, l = random_cells(rng, prm, scores=(30.0, 31.0, 32.0))
    x[2], y[5], l[7] = 96, 64, 16
    s[[2, 5, 7]] = 99.0
    inp = NewKeyframeInput(s, x, y, l, random_depth(rng, prm), 5000.0, pose(rng), 0)
    return _case("outside_corners_skipped", prm, inp, False)


@functools.lru_cache(maxsize=None)
def all_cases():
    return (
        _random_case("ties_small", 1, SMALL, 5, 400, 6),
        _random_case("ties_ragged", 2, RAGGED, 20, 400, 8),
        _random_case("ties_ragged_nan", 3, RAGGED, 9, 400, 8, nan=True),
        _edge_case(),
        _border_case(),
        _random_case("cap_mid_walk", 4, RAGGED, 12, 12 + 7, 4),
        _random_case("cap_after_first", 5, SMALL, 3, 4, 4),
        _random_case("n_existing_at_cap", 6, SMALL, 10, 10, 6),
        _random_case("n_existing_over_cap", 7, RAGGED, 14, 9, 6),
        _random_case("empty_frame_dyn_ignored", 8, RAGGED, 0, 400, 6, dyn=True),
        _random_case("dyn_mask_with_existing", 9, RAGGED, 15, 400, 6, dyn=True),
        _random_case("all_depth_zero", 10, SMALL, 4, 400, 6, zeros=1.1),
        _depth_case(),
        _outside_case(),
    )


@functools.lru_cache(maxsize=None)
def answers():
    """The restated answer of every case, by name (computed once)."""
    return {c["name"]: create_keyframe(CAM, c["prm"], c["inp"]) for c in all_cases()}


def pack(cases) -> bytes:
    """The cases as tests/newkf_host/driver.cpp reads them."""
    out = [struct.pack("<i", len(cases))]
    for c in cases:
        p, i = c["prm"], c["inp"]
        out.append(struct.pack("<7if4f", p.width, p.height, p.cell_size, p.grid_cols, p.grid_rows, p.max_fts, p.min_dist, p.score_floor, *CAM))
        for a, dt in ((i.cell_score, np.float32), (i.cell_x, np.int32), (i.cell_y, np.int32), (i.cell_level, np.int32)):
            out.append(np.ascontiguousarray(a, dt).tobytes())
        out.append(struct.pack("<2i", i.n_existing, i.first_point_index))
        for a, dt in ((i.px_xy, np.float32), (i.level, np.int32), (i.bearing, np.float64), (i.has_point, np.uint8), (i.initial, np.uint8),
                      (i.point_index, np.int32)):
            out.append(np.ascontiguousarray(a, dt).tobytes())
        out.append(np.ascontiguousarray(i.depth, np.uint16).tobytes())
        out.append(struct.pack("<fi", i.depth_scale, 0 if i.dyn_mask is None else 1))
        if i.dyn_mask is not None:
            out.append(np.ascontiguousarray(i.dyn_mask, np.uint8).tobytes())
        out.append(np.ascontiguousarray(i.T_c2w, np.float64).tobytes())
    return b"".join(out)


def unpack(blob: bytes, n_cases: int) -> list:
    """The driver's answers: per case n_new, n_slots, n_new_points and the columns."""
    outs, o = [], 0

    def take(dt, count, shape=None):
        nonlocal o
        a = np.frombuffer(blob, dt, count, o).copy()
        o += a.nbytes
        return a if shape is None else a.reshape(shape)
    for _ in range(n_cases):
        n_new, S, P = (int(v) for v in take(np.int32, 3))
        outs.append({"n_new": n_new, "n_slots": S, "n_new_points": P, "point_of_slot": take(np.int32, S), "observes": take(np.uint8, S),
                     "px_xy": take(np.float32, 2 * S, (S, 2)), "level": take(np.int32, S), "bearing": take(np.float64, 3 * S, (S, 3)),
                     "depth_of_slot": take(np.float32, S), "new_p_world": take(np.float64, 3 * P, (P, 3))})
    assert o == len(blob)
    return outs


def assert_same(got: dict, want: dict, what: str):
    """Counts equal, every column bit-equal."""
    for k in ("n_new", "n_slots", "n_new_points"):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in ("point_of_slot", "observes", "px_xy", "level", "bearing", "depth_of_slot", "new_p_world"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])
