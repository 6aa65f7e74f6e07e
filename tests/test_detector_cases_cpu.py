"""Holds the cases of tests/detector_cases.py to their conditions, with the oracle alone: each case reaches the kernels it names,
its table is one the batch entry accepts, and the inputs have the property the case exists for (ties that the two tie mutants of
the oracle decide differently, a threshold that equals a cell's score, corners outside a short grid). The device runs the same
cases in tests/test_detector_paths_gpu.py."""
import numpy as np
import pytest

from tests import detector_cases as DC
from tests import oracle_lib


@pytest.mark.parametrize("name", DC.NAMES)
def test_case_reaches_the_kernels_it_names(name):
    case = DC.get(name)
    assert DC.table_is_valid(case) and case.occ.shape == (case.n, case.cells)
    assert all(w < (1 << 14) and h < (1 << 14) for w, h in zip(case.width, case.height))
    assert DC.kernel_paths(case.width, case.stride, case.offset, case.pitch, case.n) == (case.score, case.select)
    if case.sub_n is not None:
        assert 0 < case.sub_n < case.n
        assert DC.kernel_paths(case.width, case.stride, case.offset, case.pitch, case.sub_n) == (case.score, case.sub_select)
    if case.twin is not None:
        twin = DC.get(case.twin)
        assert twin.images is case.images and np.array_equal(twin.occ, case.occ) and (twin.grid_cols, twin.grid_rows) == (case.grid_cols, case.grid_rows)
        assert (twin.stride, twin.offset) != (case.stride, case.offset)


@pytest.mark.parametrize("name", [n for n in DC.NAMES if n != "kinds_128x80"])
def test_every_level_decides_cells(oracle, name):
    """a path that no winning corner went through would be compared with nothing: over the batch every level wins cells (in the tie
    cases level 1 repeats level 0 and loses every tie to it by construction: levels 0 and 2 there)"""
    case = DC.get(name)
    won = np.zeros(case.levels, np.int64)
    for i in range(case.n):
        sc, _, _, lv = DC.oracle_cells(oracle, case, i)
        won += np.bincount(lv[sc > np.float32(case.threshold)], minlength=case.levels)
    need = [0, 2] if name.startswith("ties_") else range(case.levels)
    assert all(won[l] >= 3 for l in need), won


def test_the_layout_cases_are_what_they_are_for():
    mixed = DC.get("mixed_180x100")
    assert mixed.width == (180, 90, 45) and mixed.n == 8 and mixed.sub_n == 7
    assert (mixed.width[2] + 3) // 4 * 4 > mixed.width[2]                                # a ragged last task of 4 pixels
    assert DC.get("mixed_188x120").width == (188, 94, 47, 24)
    assert DC.get("production_752x480").width == (752, 376, 188, 94) and DC.get("production_752x480").n == 8
    for (w, h), groups in DC.GRID_SIZES.items():
        case = DC.get(f"grid_{w}x{h}")
        assert case.n == 9 and case.sub_n == 3 and DC.strip_workgroups(w, h) == groups
        assert all(DC.strip_workgroups(*s) <= groups for s in zip(case.width, case.height))
        assert case.stride == case.width and all(o % 64 == 0 for o in case.offset)
    assert DC.get("grid_176x100").height == (100, 50, 25) and DC.get("grid_240x150").height == (150, 75, 38)   # 4-row chunks end inside
    pad = DC.get("stride_aligned_padding")
    assert pad.stride == (184, 96, 48) and all(o % 4 == 0 and o % 64 != 0 for o in pad.offset)
    assert DC.get("stride_odd").stride == (176, 91, 44)
    odd = DC.get("offset_odd")
    assert odd.stride == odd.width and odd.offset[1] % 4 == 2 and odd.offset[0] % 4 == 0 and odd.offset[2] % 4 == 0
    tight = DC.get("tight_pitch")
    assert tight.offset[2] + tight.stride[2] * (tight.height[2] - 1) + tight.width[2] == tight.pitch and tight.pitch % 8 == 4
    big = DC.get("larger_pixel_level")
    assert (big.width, big.height, big.stride) == ((64, 150), (60, 90), (64, 151))
    strip = DC.get("larger_strip_level")
    assert strip.width[1] > strip.width[0] and strip.height[1] > strip.height[0]
    assert DC.strip_workgroups(strip.width[1], strip.height[1]) > DC.strip_workgroups(strip.width[0], strip.height[0])


def test_packing_fills_everything_outside_the_levels_with_random_bytes():
    case = DC.get("stride_aligned_padding")
    a, b = DC.pack(case, 2, seed=1), DC.pack(case, 2, seed=2)
    inside = np.zeros(case.pitch, bool)
    for l in range(case.levels):
        w, h, s, o = case.width[l], case.height[l], case.stride[l], case.offset[l]
        for y in range(h):
            inside[o + y * s:o + y * s + w] = True
            assert np.array_equal(a[1, o + y * s:o + y * s + w], case.images[1][l][y])
    assert np.array_equal(a[:, inside], b[:, inside]) and 0 < (~inside).sum()
    outside = a[:, ~inside]
    assert (outside != b[:, ~inside]).mean() > 0.9 and len(np.unique(outside)) > 200      # padding, gaps and the tail: noise


def _differing(a, b):
    return (a[1] != b[1]) | (a[2] != b[2]) | (a[3] != b[3]) | (a[0] != b[0])


@pytest.mark.parametrize("name", ["ties_176x100", "ties_180x100"])
def test_tie_frames_are_decided_differently_by_the_tie_mutants(oracle, name):
    """In every tie frame: MUT_D_CELLMAX (the LAST of equal scores keeps the cell) moves the winner of >= 10 cells, in >= 3 of them
    to another level; MUT_D_NMS_TIE (equal neighbours do not suppress) changes >= 10 survivors of level 0 — and the cells."""
    case = DC.get(name)
    assert DC.TIE_FRAMES[0] is not None and DC.TIE_FRAMES[1] is None                     # a tie frame and a plain frame side by side
    for i, t in enumerate(DC.TIE_FRAMES):
        if t is None:
            continue
        assert 8 <= t[0] <= 16 and np.array_equal(case.images[i][1], DC.tiling(case.height[1], case.width[1], *t))
        faithful = DC.oracle_cells(oracle, case, i)
        nms = oracle.fast10_list(case.images[i][0], case.barrier)
        with oracle_lib.mutant("MUT_D_CELLMAX"):
            last = DC.oracle_cells(oracle_lib, case, i)
        with oracle_lib.mutant("MUT_D_NMS_TIE"):
            nms_tie = oracle_lib.fast10_list(case.images[i][0], case.barrier)
            loose = DC.oracle_cells(oracle_lib, case, i)
        moved = _differing(faithful, last)
        assert moved.sum() >= 10 and (moved & (faithful[3] != last[3])).sum() >= 3, (i, moved.sum())
        assert np.array_equal(faithful[0], last[0])                                      # equal scores: only the place differs
        assert np.array_equal(nms[:, :3], nms_tie[:, :3]) and (nms[:, 3] != nms_tie[:, 3]).sum() >= 10, i
        assert _differing(faithful, loose).sum() >= 1, i
        # the two mutants' cells are two results, not one looked up twice
        assert loose is not last and _differing(last, loose).any(), i


@pytest.mark.parametrize("name", DC.THRESHOLD_CASES)
def test_threshold_equal_to_a_score_drops_that_corner(oracle, name):
    case = DC.get(name)
    k, s, below = DC.threshold_pair(oracle, case)
    at, under = DC.oracle_cells(oracle, case, 0, s), DC.oracle_cells(oracle, case, 0, below)
    assert below < s and under[0][k] == s and (under[1][k], under[2][k]) != (0, 0)       # just below: the corner is still there
    assert at[0][k] == s and (at[1][k], at[2][k], at[3][k]) == (0, 0, 0)                 # at s: `>` fails, the cell is empty (:74)
    base = DC.oracle_cells(oracle, case, 0)[0]
    assert (at[0] > s).sum() >= 3 and ((base > np.float32(case.threshold)) & (base < s)).sum() >= 3   # winners on both sides of s
    others = np.arange(case.cells) != k
    assert all(np.array_equal(a[others], b[others]) for a, b in zip(at[1:], under[1:]))  # the same corners everywhere else


def test_frames_of_different_kinds(oracle):
    case = DC.get("kinds_128x80")
    thr = np.float32(case.threshold)
    flat, chk = DC.oracle_cells(oracle, case, 0), DC.oracle_cells(oracle, case, 1)
    assert len(np.unique(case.images[0][0])) == 1 and (flat[0] == thr).all() and not (flat[1] | flat[2] | flat[3]).any()
    assert set(np.unique(case.images[1][0])) == {0, 255} and np.array_equal(case.images[1][0][:4, :8], np.repeat([[0, 255]], 4, 0).repeat(4, 1))
    # (a plain checkerboard has no FAST-10 corner — no 10 contiguous ring pixels of the other colour — so its cells are empty as
    # well; the frame of 0 / 255 blocks behind the textures is the one whose corners all have margin 255 and score 254)
    assert (chk[0] == thr).all()
    blocks = oracle.fast10_list(case.images[5][0], case.barrier)
    assert len(blocks) > 50 and set(blocks[:, 2].tolist()) == {254} and (DC.oracle_cells(oracle, case, 5)[0] > thr).sum() >= 10
    assert case.images[2] is case.images[3] is case.images[4]
    assert case.occ[2].all() and not case.occ[3].any() and 0 < case.occ[4].sum() < case.cells and not case.occ[[0, 1, 5, 6, 7]].any()
    full, none, some = (DC.oracle_cells(oracle, case, i) for i in (2, 3, 4))
    assert (full[0] == thr).all() and (none[0] > thr).sum() >= 15
    free = case.occ[4] == 0
    assert (some[0][~free] == thr).all() and all(np.array_equal(a[free], b[free]) for a, b in zip(some, none))
    assert ((none[0] > thr) & ~free).sum() >= 3                                          # the occupancy of frame 4 hides winners of frame 3


def test_corners_outside_a_short_grid(oracle):
    """176x100 at cell size 25 is covered by 8 x 4 cells. With fewer columns the corners on the right compute a column index equal to
    grid_cols and land in the next row's first cell, as the reference's expression (:97-98) does; with 3 rows the corners at the
    bottom compute k >= G and are dropped. (The right-most candidate column of level 0 is 172 < 175, and the other levels reach
    less far: with 7 columns no corner has column index 7 — that run only checks a grid narrower than the image — and the wrap
    is held at 6 columns.)"""
    def kinds(case):
        wrap = drop = 0
        for l, x, y in DC.survivors(oracle, case, 0):
            col, row = (x << l) // case.cell_size, (y << l) // case.cell_size
            k = row * case.grid_cols + col
            drop += k >= case.cells
            wrap += col >= case.grid_cols and k < case.cells
        return wrap, drop
    assert kinds(DC.get("stride_packed")) == (0, 0)
    assert kinds(DC.get("grid_7x4_on_176x100")) == (0, 0)
    wrap, drop = kinds(DC.get("grid_6x4_on_176x100"))
    assert wrap >= 5 and drop >= 5                                                       # the last row's wrapped corners leave the grid
    wrap, drop = kinds(DC.get("grid_8x3_on_176x100"))
    assert wrap == 0 and drop >= 5
