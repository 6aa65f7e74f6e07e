"""KLTWrapper::RunTrack without a GPU: the restatement dsdtm_amd/klt_restatement.py (rules K1-K9 of include/dsdtm_amd_klt.h) against
klt_flow_host (dsdtm_amd/host/dsdtm_klt_host.hpp) bit for bit on every world of tests/klt_cases.py, against hand cases whose answer
needs no implementation, the properties of the worlds, the mutants of the restatement, and the surface of libdsdtm_amd_klt.so.

Measured here with the restatement (asserted at twice the value): the recovered flow of the integer-shift worlds errs by at most
2.6e-3 px (171x123, shift (3, -2)); on the warp world the returned H maps the grid points to within 3.6e-2 px of the true one.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import capi, homography, klt, mcd
from dsdtm_amd import klt_restatement as KR
from dsdtm_amd.csrc import build as hip_build
from tests import klt_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW_BOUND = 2.6e-3        # px, measured: the largest error of a grid point's flow on the 160x120 and 171x123 shift worlds
WARP_BOUND = 3.6e-2        # px, measured: the largest distance between H_returned p and H_true p over the grid of the warp world
K = KR.Klt()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cases.host_library(tmp_path_factory.mktemp("klt"))


@pytest.fixture(scope="module")
def block_step():
    prev, cur, flags = cases.block_world()
    m = KR.KltModel(640, 480)
    m.step(prev)
    return m, m.step(cur), flags, (prev, cur)


@pytest.mark.parametrize("size", ["160x120", "171x123"])
@pytest.mark.parametrize("shift", cases.SHIFTS)
def test_shift_worlds_restatement_host_and_flow(host, size, shift):
    """Every grid point keeps status 1, the flow is the shift to within 2x the measured bound, host function = restatement bit for bit."""
    w, h = cases.SIZES[size]
    prev, cur = cases.shift_world(size, shift)
    pts = KR.grid_points(w, h)
    assert len(pts) == 16
    f = K.flow(prev, cur, pts)
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts), f)
    assert f["status"].all()
    err = np.abs(f["points"].astype(np.float64) - pts - np.array(shift, np.float64)).max()
    print(size, shift, "flow error", err, "iterations", f["iterations"].tolist())
    assert err <= 2 * FLOW_BOUND
    if shift == (0, 0):
        assert err == 0.0 and (f["residual"] == 0).all()


def test_grid_is_what_init_features_fills(host):
    """K8: 361 points at 640x480, not the reference's count of 400; i major; the host function's grid is the same."""
    g = KR.grid_points(640, 480)
    assert len(g) == 19 * 19 == 361 and 640 // 32 * (480 // 24) == 400
    assert g[0].tolist() == [16, 12] and g[1].tolist() == [16, 36] and g[19].tolist() == [48, 12] and g[-1].tolist() == [18 * 32 + 16, 18 * 24 + 12]
    buf = np.zeros((400, 2), np.float32)
    for (w, h, gw, gh) in ((640, 480, 0, 0), (171, 123, 0, 0), (160, 120, 80, 8), (160, 120, 16, 12)):
        n = host.klt_grid_host_c(w, h, gw, gh, buf.ctypes.data, 400)
        assert n == len(KR.grid_points(w, h, gw, gh)) and np.array_equal(buf[:n], KR.grid_points(w, h, gw, gh))


def test_pyramid_of_the_host_function_is_the_restatements(host):
    img = cases.shift_world("171x123", (0, 0))[0]
    pyr = KR.build_pyramid(img, 4)
    assert [p.shape for p in pyr] == [(123, 171), (62, 86), (31, 43), (16, 22)]
    for l in range(4):
        out = np.zeros(pyr[l].shape, np.uint8)
        assert host.klt_pyramid_host_c(img.ctypes.data, 171, 123, img.strides[0], l, out.ctypes.data) == 0
        assert np.array_equal(out, pyr[l])


def test_640x480_shift_world_once(host):
    prev, cur = cases.shift_world("640x480", (6, 5))
    pts = KR.grid_points(640, 480)
    f = cases.host_flow(host, prev, cur, pts)
    assert len(pts) == 361 and f["status"].all()
    assert np.abs(f["points"].astype(np.float64) - pts - (6, 5)).max() <= 2 * FLOW_BOUND
    assert cases.same_flow(K.flow(prev, cur, pts), f)          # all 361 points


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------

def test_hand_scharr_of_a_ramp():
    """I(x, y) = 3 x + 2 y: gx = (3 + 10 + 3) * 2 * 3 = 96 and gy = 16 * 2 * 2 = 64 at every interior pixel."""
    ys, xs = np.mgrid[0:9, 0:11]
    gx, gy = K.gradients((3 * xs + 2 * ys).astype(np.uint8))
    assert (gx[1:-1, 1:-1] == 96).all() and (gy[1:-1, 1:-1] == 64).all()


def test_hand_fixed_point_bilinear_at_the_corners_of_a_cell():
    img = np.array([[10, 20], [30, 40]], np.int64)
    for (fx, fy), w, v in (((0.0, 0.0), (16384, 0, 0, 0), 10), ((1.0, 0.0), (0, 16384, 0, 0), 20), ((0.0, 1.0), (0, 0, 16384, 0), 30), ((1.0, 1.0), (0, 0, 0, 16384), 40)):
        assert KR.weights(fx, fy) == w
        assert KR.bilinear(img, 0, 0, 1, w, 9)[0, 0] == v * 32 and KR.bilinear(img, 0, 0, 1, w, 14)[0, 0] == v
    assert KR.weights(0.5, 0.5) == (4096, 4096, 4096, 4096) and KR.bilinear(img, 0, 0, 1, KR.weights(0.5, 0.5), 9)[0, 0] == 25 * 32
    assert sum(KR.weights(0.3, 0.7)) == 16384


def test_hand_zero_shift_converges_in_one_iteration_with_a_zero_step(host):
    """Equal images: b = 0, so the step is exactly 0 and `<=` stops every level after one iteration, even at epsilon 0. (48, 36) is row
    36 / 8 - 4.5 = 0 on the coarsest level: its ring leaves that level, which is skipped (K4): three iterations, not four."""
    img = cases.shift_world("160x120", (0, 0))[0]
    pts = np.array([(80, 60), (48, 36)], np.float32)
    f = K.flow(img, img, pts, eps=0.0)
    assert f["iterations"].tolist() == [4, 3] and np.array_equal(f["points"], pts) and f["status"].tolist() == [1, 1]
    assert cases.same_flow(cases.host_flow(host, img, img, pts, eps=0.0), f)


def test_hand_constant_image_fails_the_eigenvalue_test_everywhere(host):
    img = np.full((120, 160), 77, np.uint8)
    pts = KR.grid_points(160, 120)
    f = K.flow(img, img, pts)
    assert not f["status"].any() and not f["iterations"].any() and np.array_equal(f["points"], pts)
    assert cases.same_flow(cases.host_flow(host, img, img, pts), f)


# ---- the other worlds ---------------------------------------------------------------------------------------------------------------

def test_flat_region_exits_by_the_eigenvalue_test(host):
    prev, cur = cases.flat_world()
    pts = KR.grid_points(160, 120)
    f = K.flow(prev, cur, pts)
    assert f["status"].tolist() == [0] * 8 + [1] * 8            # the two grid columns on the flat third
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts), f)


@pytest.mark.parametrize("window,levels", [(4, 1), (10, 4), (21, 3), (10, 5)])
def test_border_points_windows_and_levels(host, window, levels):
    prev, cur = cases.shift_world("160x120", (3, -2))
    pts = cases.border_points(160, 120)
    f = K.flow(prev, cur, pts, window=window, levels=levels)
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts, window=window, levels=levels), f)
    assert f["status"][:2].all() and not f["status"][3:6].any()          # interior points live; windows that leave level 0 do not
    if (window, levels) == (10, 4):
        assert f["status"].tolist() == [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]


def test_initial_guesses(host):
    prev, cur = cases.shift_world("160x120", (6, 5))
    pts = KR.grid_points(160, 120)
    g = pts + np.array([5.5, 4.5], np.float32)
    f = K.flow(prev, cur, pts, guesses=g, levels=1)
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts, guesses=g, levels=1), f)
    assert f["status"].all() and np.abs(f["points"] - pts - (6, 5)).max() <= 2 * FLOW_BOUND


def test_warp_world_returns_the_homography():
    prev, cur, H = cases.warp_world()
    m = KR.KltModel(160, 120)
    first = m.step(prev)
    assert first["source"] == KR.SOURCE_IDENTITY and first["n_tracked"] == 0 and np.array_equal(first["H"], KR.IDENTITY)
    r = m.step(cur)
    assert r["source"] == KR.SOURCE_RANSAC and r["n_tracked"] == 16 and r["n_inliers"] == 16
    err = np.abs(cases.apply_h(r["H"], m.grid) - cases.apply_h(H, m.grid)).max()
    print("warp error", err)
    assert err <= 2 * WARP_BOUND


def test_moving_block_is_rejected_by_the_ransac(block_step):
    m, r, flags, _ = block_step
    assert r["source"] == KR.SOURCE_RANSAC and r["n_points"] == 361
    keep = np.flatnonzero(r["status"])
    fl = flags[keep]
    assert (fl == 1).sum() >= 50 and (fl == 0).sum() >= 250
    assert not r["mask"][fl == 1].any()               # every point on the block is an outlier
    assert r["mask"][fl == 0].all()                   # every background point an inlier
    assert flags[r["status"] == 0].tolist() == [] or (flags[r["status"] == 0] == 2).all()
    H = r["H"].reshape(3, 3)
    assert abs(H[0, 2] + 6.0) < 0.05 and abs(H[1, 2]) < 0.05          # current -> previous: the background came from 6 px to the left


def test_fewer_than_ten_survivors_give_the_identity():
    prev, cur = cases.flat_world()
    m = KR.KltModel(160, 120)
    m.step(prev)
    r = m.step(cur)
    assert r["n_tracked"] == 8 and r["source"] == KR.SOURCE_IDENTITY and np.array_equal(r["H"], KR.IDENTITY)


def test_collinear_grid_finds_nothing_and_keeps_the_previous_h():
    """One grid column: every sample is collinear, the RANSAC finds nothing, and K9 keeps the H of the step before."""
    a, b = cases.shift_world("160x120", (3, -2))
    m = KR.KltModel(160, 120)
    m.step(a)
    r1 = m.step(b)
    r2 = m.step(a, gw=80, gh=8)
    assert r1["source"] == KR.SOURCE_RANSAC and r2["n_points"] == 14 and r2["n_tracked"] >= 10
    assert r2["source"] == KR.SOURCE_KEPT and np.array_equal(r2["H"], r1["H"]) and not np.array_equal(r2["H"], KR.IDENTITY)


def _same_step_host(host, prev, cur, r, grid, **kw):
    """klt_step_host against KltModel.step: the grid's status and the survivors in ascending index, A = current, B = previous."""
    hs = cases.host_step(host, prev, cur, **kw)
    keep = np.flatnonzero(r["status"])
    assert hs["n_points"] == r["n_points"] and hs["n_tracked"] == r["n_tracked"] == len(keep) and np.array_equal(hs["status"], r["status"])
    assert np.array_equal(hs["a"].view(np.uint32), r["points"][keep].view(np.uint32)) and np.array_equal(hs["b"], grid[keep])
    assert not np.array_equal(hs["a"], hs["b"])


def test_host_functions_on_the_warp_world(host):
    prev, cur, _ = cases.warp_world()
    pts = KR.grid_points(160, 120)
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts), K.flow(prev, cur, pts))
    m = KR.KltModel(160, 120)
    m.step(prev)
    _same_step_host(host, prev, cur, m.step(cur), m.grid)


def test_host_functions_on_the_moving_block_world(host, block_step):
    m, r, _, (prev, cur) = block_step
    f = cases.host_flow(host, prev, cur, m.grid)
    assert np.array_equal(f["points"].view(np.uint32), r["points"].view(np.uint32)) and np.array_equal(f["status"], r["status"])
    assert np.array_equal(f["iterations"], r["iterations"])
    _same_step_host(host, prev, cur, r, m.grid)


def test_step_host_on_the_flat_world_and_another_grid(host):
    """Survivors are fewer than the grid (the compaction moves them), and a grid of the caller."""
    prev, cur = cases.flat_world()
    m = KR.KltModel(160, 120)
    m.step(prev)
    r = m.step(cur)
    assert r["n_tracked"] == 8
    _same_step_host(host, prev, cur, r, m.grid)
    m2 = KR.KltModel(160, 120, gw=16, gh=12)
    m2.step(prev)
    _same_step_host(host, prev, cur, m2.step(cur), m2.grid, gw=16, gh=12)


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    from tests import fake_hip_build as fhb
    here = os.path.join(ROOT, "tests", "fake_hip_klt")
    there = os.path.join(ROOT, "tests", "fake_hip_homography")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_klt.cpp"), os.path.join(there, "fake_homography.cpp")],
                           ["klt_api.cpp"], include_dirs=[here, there])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok answers_and_memory_kinds", "ok refusals", "ok call_failures", "ok create_failures"], lines


# ---- mutants: each is told apart by a named case -------------------------------------------------------------------------------------

class Sobel(KR.Klt):
    KERNEL = (1, 2, 1)


class NoHalving(KR.Klt):
    def halves_on_oscillation(self):
        return False


class StrictStop(KR.Klt):
    def stops(self, d2, eps2):
        return d2 < eps2


class RingMayLeave(KR.Klt):
    def ring(self):
        return 0


class Swapped(KR.Klt):
    def oriented(self, cur, prev):
        return prev, cur


class StaleFixed(KR.Klt):
    def keeps_stale_h(self):
        return False


def test_mutant_sobel_on_the_shift_world():
    prev, cur = cases.shift_world("160x120", (3, -2))
    pts = KR.grid_points(160, 120)
    assert not cases.same_flow(Sobel().flow(prev, cur, pts), K.flow(prev, cur, pts))


def test_mutant_strict_stop_on_the_zero_shift_case():
    img = cases.shift_world("160x120", (0, 0))[0]
    f = StrictStop().flow(img, img, [(80, 60)], eps=0.0)
    # (every step is 0: the mutant never stops by the step test, and leaves each level by the oscillation test at its second iteration)
    assert f["iterations"].tolist() == [8] and K.flow(img, img, [(80, 60)], eps=0.0)["iterations"].tolist() == [4]


def test_mutant_no_halving_on_an_oscillating_point():
    """The oscillation exit is reached on the warp world at epsilon 0 (no step is ever small enough to stop first)."""
    prev, cur, _ = cases.warp_world()
    pts = KR.grid_points(160, 120)
    base, mut = K.flow(prev, cur, pts, eps=0.0), NoHalving().flow(prev, cur, pts, eps=0.0)
    assert (base["iterations"] < 80).any() and (mut["iterations"] > base["iterations"]).any()
    assert not np.array_equal(base["points"], mut["points"])


def test_mutant_ring_on_the_border_points():
    prev, cur = cases.shift_world("160x120", (0, 0))
    pts = np.array([(4.5, 60), (80, 4.5)], np.float32)          # first tap at column / row 0: the window fits, its ring does not
    assert K.flow(prev, cur, pts, levels=1)["status"].tolist() == [0, 0]
    assert RingMayLeave().flow(prev, cur, pts, levels=1)["status"].tolist() == [1, 1]


def test_mutant_swapped_on_the_moving_block(block_step):
    m, r, _, (prev, cur) = block_step
    s = KR.KltModel(640, 480, klt=Swapped())          # the mutant through step(): the same flow, the fit the other way round
    s.step(prev)
    got = s.step(cur)
    assert got["source"] == KR.SOURCE_RANSAC and np.array_equal(got["points"], r["points"])
    assert abs(got["H"][2] - 6.0) < 0.05 and abs(r["H"][2] + 6.0) < 0.05


class NothingFound:
    def find(self, A, B, thr=None):
        return dict(found=0)


def test_mutant_stale_h_fixed():
    a, b = cases.shift_world("160x120", (3, -2))
    for klt_, source in ((KR.Klt(), KR.SOURCE_KEPT), (StaleFixed(), KR.SOURCE_IDENTITY)):
        m = KR.KltModel(160, 120, klt=klt_)
        m.step(a)
        r1 = m.step(b)
        m.ransac = NothingFound()
        r2 = m.step(a)
        assert r1["source"] == KR.SOURCE_RANSAC and r2["n_tracked"] == 16 and r2["source"] == source
        assert np.array_equal(r2["H"], r1["H"] if source == KR.SOURCE_KEPT else KR.IDENTITY)


# ---- the worlds of the device's edge tests, held to their claims ---------------------------------------------------------------------
# (saturated contrast, windows around a pass of 64 lanes, every exit of the two loops, the compaction's edges: tests/test_klt_gpu.py
#  runs them on the device; here the restatement's trace says what they reach, and klt_flow_host agrees with it bit for bit. The host
#  function takes every parameter these worlds use — any window, level count, iteration cap and epsilon, guesses — so nothing is left out
#  of that comparison; klt_step_host has the defaults of RunTrack built in, which are the compaction worlds' parameters.)

SATURATED_WINDOWS = (21, 16, 10, 4)


def _plain_sum(v):
    return int(v.sum())


def test_saturated_worlds_carry_past_31_and_32_bits(host):
    """Window 21, from the trace, over points with status 1: an s11 or s22 above 2^31 on every world, a t1 / t2 above 2^32 in magnitude
    with both signs over the worlds, and |dx| = 4080 on the block noise."""
    beyond = []
    for name, prev, cur in cases.saturated_worlds():
        pts = cases.saturated_points(21)
        tr = []
        f = K.flow(prev, cur, pts, window=21, levels=1, trace=tr)
        assert cases.same_flow(cases.host_flow(host, prev, cur, pts, window=21, levels=1), f)
        ok = [e for e in tr if e["status"] == 1]
        assert f["status"][:7].all() and ok, name                  # the interior points track
        assert max(max(e["s11"], e["s22"]) for e in ok) > 2 ** 31, name
        beyond += [e["t1_min"] for e in ok] + [e["t1_max"] for e in ok] + [e["t2_min"] for e in ok] + [e["t2_max"] for e in ok]
        with cases.observed_sums(_plain_sum) as seen:
            again = K.flow(prev, cur, pts[f["status"] == 1], window=21, levels=1)
        assert again["status"].all()
        print(name, "s max", max(max(e["s11"], e["s22"]) for e in ok), "t1", min(e["t1_min"] for e in ok), max(e["t1_max"] for e in ok), "|dx|", seen.gradient_max)
        assert seen.gradient_max == (4080 if name.startswith("noise") else 2550), (name, seen.gradient_max)
    assert min(beyond) < -2 ** 32 and max(beyond) > 2 ** 32, (min(beyond), max(beyond))
    tr = []
    K.flow(*cases.checker_world(), [(80, 60)], window=21, levels=1, trace=tr)          # the figures of the world's docstring
    assert (tr[0]["s11"], tr[0]["s22"], tr[0]["t1_min"], tr[0]["steps"], tr[0]["status"]) == (2867602500, 2867602500, -4806648000, 8, 1)


@pytest.mark.parametrize("window", SATURATED_WINDOWS)
def test_a_lanes_partial_sum_fits_32_bits_on_the_saturated_worlds(window):
    """klt_kernel keeps a lane's partial of dx dx, dx dy, dy dy, d dx, d dy and |d| in an int: pixel i of the window belongs to lane
    i % 64, seven pixels at the most. By arithmetic no image gets past 7 x 4080^2 = 1.17e8 and 7 x 8160 x 4080 = 2.33e8; asserted all
    the same on the worlds that come closest, from the arrays the restatement sums (a condition on the inputs, not on the device)."""
    worst = [0]

    def fn(v):
        worst[0] = max(worst[0], int(np.abs(cases.lane_partials(v)).max()))
        return int(v.sum())

    for name, prev, cur in cases.saturated_worlds():
        pts = cases.saturated_points(window)
        with cases.observed_sums(fn):
            f = K.flow(prev, cur, pts, window=window, levels=4)
        assert cases.same_flow(f, K.flow(prev, cur, pts, window=window, levels=4)), name          # observing changes nothing
    print("window", window, "largest lane partial", worst[0])
    assert 0 < worst[0] < 2 ** 31 and worst[0] <= 7 * 8160 * 4080
    assert np.array_equal(cases.lane_partials(np.arange(130).reshape(10, 13))[:3], [0 + 64 + 128, 1 + 65 + 129, 2 + 66])


@pytest.mark.parametrize("window", SATURATED_WINDOWS)
@pytest.mark.parametrize("levels", [1, 4])
def test_saturated_worlds_host_function(host, window, levels):
    for name, prev, cur in cases.saturated_worlds():
        pts = cases.saturated_points(window)
        f = K.flow(prev, cur, pts, window=window, levels=levels)
        assert cases.same_flow(cases.host_flow(host, prev, cur, pts, window=window, levels=levels), f), name
        assert f["status"][:7].all() or levels == 4, name
        if levels == 1:          # K4 on level 0: the first and last admissible positions pass, the first outside fail
            assert not f["status"][11:].any(), (name, f["status"].tolist())
            tr = []
            K.flow(prev, cur, pts[7:11], window=window, levels=1, trace=tr)
            assert all(e["exit"] != "prev_outside" for e in tr), name


@pytest.mark.parametrize("window", cases.SWEEP_WINDOWS)
def test_window_sweep_host_function(host, window):
    """Windows whose area fills a pass of 64 lanes (8, 16), starts a new one with one pixel (9, 17), and the other parities."""
    levels = cases.deepest_levels(window)
    assert levels == {5: 5, 7: 4, 8: 4, 9: 4, 11: 4, 12: 4, 15: 3, 16: 3, 17: 3, 20: 3}[window]
    prev, cur = cases.shift_world("160x120", (3, -2))
    pts = cases.border_points(160, 120)
    f = K.flow(prev, cur, pts, window=window, levels=levels)
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts, window=window, levels=levels), f)
    assert f["status"][:2].all() and not f["status"][3:6].any()


def test_exit_world_takes_every_exit_on_a_coarse_level_and_on_level_0(host):
    """From the trace, over the parameter sets: each of the six ways out of a level on a level above 0 and on level 0, K7's last look,
    a current window that is outside before the first step and one that drifts out after one or more steps (each on a coarse
    level and on level 0), a step that is exactly zero at an epsilon whose square is 0. No combination is missing."""
    prev, cur, pts, g, sets = cases.exit_world()
    seen, drift = set(), set()
    for kw in sets:
        tr = []
        f = K.flow(prev, cur, pts, guesses=g, trace=tr, **kw)
        assert cases.same_flow(cases.host_flow(host, prev, cur, pts, guesses=g, **kw), f), kw
        here = {(e["exit"], e["level"] > 0) for e in tr}
        print(kw, sorted(here))
        seen |= here
        drift |= {(min(e["steps"], 1), e["level"] > 0) for e in tr if e["exit"] == "cur_outside"}
        cap = kw.get("iterations", 20)
        assert all(e["steps"] <= cap for e in tr) and all(e["steps"] == cap for e in tr if e["exit"] == "cap")
        if kw.get("eps") == cases.EPS_ZERO:
            assert cases.EPS_ZERO ** 2 == 0.0 and cases.same_flow(K.flow(prev, cur, pts, guesses=g, **dict(kw, eps=0.0)), f)
    assert seen == {(name, coarse) for name in cases.EXITS for coarse in (False, True)} | {("final_outside", False)}, sorted(seen)
    assert drift == {(steps, coarse) for steps in (0, 1) for coarse in (False, True)}, sorted(drift)          # 1: one step or more
    n = len(pts)
    assert np.abs(g[n - 10:n - 6]).max() == 1e5          # the bound dsdtm_klt_flow admits


def test_exit_world_oscillating_point_of_the_warp_world(host):
    """The point test_mutant_no_halving_on_an_oscillating_point relies on, as the device test runs it."""
    prev, cur, _ = cases.warp_world()
    pts = KR.grid_points(160, 120)
    tr = []
    f = K.flow(prev, cur, pts, eps=cases.EPS_ZERO, trace=tr)
    assert {(e["exit"], e["level"] > 0) for e in tr} >= {("oscillation", False), ("oscillation", True)}
    assert cases.same_flow(cases.host_flow(host, prev, cur, pts, eps=cases.EPS_ZERO), f) and cases.same_flow(K.flow(prev, cur, pts, eps=0.0), f)


def test_trace_is_opt_in_and_changes_nothing():
    prev, cur, pts, g, sets = cases.exit_world()
    tr = []
    assert cases.same_flow(K.flow(prev, cur, pts, guesses=g), K.flow(prev, cur, pts, guesses=g, trace=tr))
    assert len(tr) >= 4 * len(pts) and {e["point"] for e in tr} == set(range(len(pts)))
    assert [e["level"] for e in tr if e["point"] == 0 and e["exit"] != "final_outside"] == [3, 2, 1, 0]


def test_mixed_pairs_host_function(host):
    pairs = cases.mixed_pairs()
    assert [len(p["points"]) for p in pairs] == [1, 3, 2048, 4, 5, 64, 65]
    assert sorted({p["window"] for p in pairs}) == [4, 9, 16, 21] and sorted({p["levels"] for p in pairs}) == [1, 2, 3, 4, 5]
    for k, p in enumerate(pairs):
        kw = {a: b for a, b in p.items() if a not in ("prev", "cur", "points")}
        assert cases.same_flow(cases.host_flow(host, p["prev"], p["cur"], p["points"], **kw), cases.restated(p)), k


@pytest.mark.parametrize("name", list(cases.COMPACTION))
def test_compaction_worlds_are_what_they_claim(host, name):
    rects, gw, gh, n_points, n_tracked = cases.COMPACTION[name]
    prev, cur, gw, gh, r = cases.compaction_step(name)
    s = r["status"]
    print(name, r["n_tracked"], "".join(map(str, s.tolist())))
    assert r["n_points"] == n_points == len(s) and r["n_tracked"] == int(s.sum())
    if n_tracked is not None:
        assert r["n_tracked"] == n_tracked
        assert r["source"] == (KR.SOURCE_RANSAC if n_tracked >= 10 else KR.SOURCE_IDENTITY)
    if "lanes 0 and 63" in name:
        last = s[-64:]
        assert last[0] == 1 and last[63] == 1 and 0 < last[1:63].sum() < 62
    if "second round" in name:
        assert 0 < s[:64].sum() < 64          # the first round is partly filled: `base` is neither 0 nor 64 when it is carried
    if "second round full" in name:
        assert s[64:].all()
    if "second round empty" in name:
        assert not s[64:].any()
    if name == "64 points":
        assert s.all()                        # one whole round, every lane a survivor
    if r["n_tracked"]:
        _same_step_host(host, prev, cur, r, KR.grid_points(160, 120, gw, gh), gw=gw, gh=gh)
    else:
        hs = cases.host_step(host, prev, cur, gw=gw, gh=gh)
        assert hs["n_tracked"] == 0 and hs["n_points"] == n_points and not hs["status"].any()


def test_mutant_totals_wrapped_to_32_bits_on_the_checker_world():
    """A device that summed a window in 32 bits: told apart by the checker world at window 21, and by no world the suite had before."""
    def wrapped(v):
        return (int(v.sum()) + 2 ** 31) % 2 ** 32 - 2 ** 31

    prev, cur = cases.checker_world()
    pts = cases.saturated_points(21)
    with cases.observed_sums(wrapped):
        mut = K.flow(prev, cur, pts, window=21, levels=1)
    base = K.flow(prev, cur, pts, window=21, levels=1)
    assert not cases.same_flow(mut, base) and not np.array_equal(mut["status"], base["status"])
    a, b = cases.shift_world("160x120", (3, -2))
    with cases.observed_sums(wrapped):
        mut = K.flow(a, b, cases.border_points(160, 120), window=21, levels=3)
    assert cases.same_flow(mut, K.flow(a, b, cases.border_points(160, 120), window=21, levels=3))


def test_mutant_more_than_ten_on_the_ten_survivor_world(monkeypatch):
    """`n_tracked > 10` written for `>= 10`: told apart by the world with exactly ten survivors, and not by 8, 9 or 16."""
    want = {name: cases.compaction_step(name)[4] for name in ("9 survivors", "10 survivors", "64 points")}
    monkeypatch.setattr(KR, "MIN_TRACKED", 11)          # (>= 11 is > 10)
    got = {name: cases.compaction_step(name)[4] for name in want}
    assert want["10 survivors"]["source"] == KR.SOURCE_RANSAC and got["10 survivors"]["source"] == KR.SOURCE_IDENTITY
    assert np.array_equal(got["10 survivors"]["H"], KR.IDENTITY) and not np.array_equal(want["10 survivors"]["H"], KR.IDENTITY)
    for name in ("9 survivors", "64 points"):
        assert got[name]["source"] == want[name]["source"] and np.array_equal(got[name]["H"], want[name]["H"])


# ---- the surface --------------------------------------------------------------------------------------------------------------------

def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_and_exported():
    """libdsdtm_amd_klt.so exports exactly the 10 symbols its header declares and reads no environment; libdsdtm_amd.so,
    libdsdtm_amd_homography.so and libdsdtm_amd_mcd.so export what they exported; the main library's source hash covers nothing of this."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_klt.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(klt.SYMBOLS) and len(klt.SYMBOLS) == 10 and len(set(klt.SYMBOLS)) == 10
    assert _exported(klt.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", klt.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    assert _exported(capi.lib_path(False)) == set(capi.EXPORTED_SYMBOLS) and len(capi.EXPORTED_SYMBOLS) == 38
    assert _exported(homography.lib_path()) == set(homography.SYMBOLS) and len(homography.SYMBOLS) == 5
    assert _exported(mcd.lib_path()) == set(mcd.SYMBOLS) and len(mcd.SYMBOLS) == 11
    assert hip_build.MORE_ADDONS["klt"][0] == ["klt_api.cpp", "klt.hip", "homography.hip", "pyrdown.hip"] and "klt" not in hip_build.ADDONS
    assert hip_build.ADDONS["homography"][0] == ["homography_api.cpp", "homography.hip"]
    assert not {"klt.hip", "klt.h", "klt_api.cpp"} & set(hip_build.SOURCES + hip_build.HEADERS)


@pytest.mark.parametrize("struct,name", [(klt.Desc, "dsdtm_klt_desc"), (klt.Result, "dsdtm_klt_result"), (klt.FlowDesc, "dsdtm_klt_flow_desc")])
def test_desc_layout(tmp_path, struct, name):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_klt.h"', 'int main(void) {', f'  printf("%zu", sizeof({name}));']
    src += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in struct._fields_] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(struct)] + [getattr(struct, f[0]).offset for f in struct._fields_]


def test_header_documents_the_rules_and_the_parity():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_klt.h")).read()
    for needle in ("KLTWrapper.cpp:125-126", "KLTWrapper.cpp:102-107", ":138-145", ":180-184", "Test/test_Optimizer.cpp:91", "THIS PROJECT'S DEFINITION",
                   "unpinned and stays unpinned", "SUPERSEDES", "QUIRK NOT KEPT", "441 x 4080^2", *[f"K{i} " for i in range(1, 10)]):
        assert needle in hdr, needle
    for name, value in (("WINDOW", 10), ("LEVELS", 4), ("ITERATIONS", 20), ("MIN_TRACKED", 10), ("MAX_STEPS", 1024), ("MAX_FLOW_POINTS", 16384)):
        assert re.search(rf"#define DSDTM_KLT_{name} {value}\b", hdr), name
