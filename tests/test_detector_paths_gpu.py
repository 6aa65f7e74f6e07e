"""The detector's batch entry on the kernel paths, layouts and inputs that tests/test_detector_gpu.py does not reach: the cases of
tests/detector_cases.py (held to their conditions by tests/test_detector_cases_cpu.py) against the oracle, cell by cell and bit
for bit. Every byte of the pyramid outside a level's pixels is random, the score scratch is 0xA5 before the first call and is
used again as that call left it by the second."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi
from tests import detector_cases as DC
from tests import oracle_lib

pytestmark = pytest.mark.gpu

FIELDS = ("score", "x", "y", "level")


@pytest.fixture(scope="module")
def device_cells(gpu_ctx):
    """device_cells(case, n=None, threshold=None): run_batch, once per (case, n, threshold) for the tests of this module"""
    done = {}

    def get(case, n=None, threshold=None):
        key = (case.name, case.n if n is None else n, None if threshold is None else float(threshold))
        if key not in done:
            done[key] = run_batch(gpu_ctx, case, key[1], threshold)
        return done[key]
    return get


def run_batch(ctx, case, n, threshold=None):
    """(score, x, y, level), each (n, cells), of the first n frames of the case through dsdtm_detect_cells_batch_device — two calls
    on the same scratch, which must agree. Read-only arrays."""
    import torch
    dev = torch.device("cuda", 0)
    G, L = case.cells, case.levels
    prm = DC.params(case, threshold)
    d_pyr = torch.from_numpy(DC.pack(case, n)).to(dev)                       # n frames back to back in one allocation
    d_occ = torch.from_numpy(np.array(case.occ[:n])).to(dev)
    d_score = torch.full((n, case.pitch), 0xA5, dtype=torch.uint8, device=dev)
    d_key = torch.full((n, G), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    d_s = torch.full((n, G), -1.0, dtype=torch.float32, device=dev)
    d_x, d_y, d_l = (torch.full((n, G), -1, dtype=torch.int32, device=dev) for _ in range(3))
    wa, ha, sa = (C.c_int * L)(*case.width), (C.c_int * L)(*case.height), (C.c_int * L)(*case.stride)
    oa = (C.c_size_t * L)(*case.offset)
    runs = []
    for rep in range(2):
        ctx.check(ctx.lib.dsdtm_detect_cells_batch_device(
            ctx.handle, d_pyr.data_ptr(), case.pitch, n, L, wa, ha, sa, oa, d_occ.data_ptr(), C.byref(prm), d_score.data_ptr(),
            d_key.data_ptr(), d_s.data_ptr(), d_x.data_ptr(), d_y.data_ptr(), d_l.data_ptr(), None))
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in (d_s, d_x, d_y, d_l)])
    for a, b, name in zip(runs[0], runs[1], FIELDS):
        assert np.array_equal(a, b), (case.name, n, "second call on the same scratch", name)
    for a in runs[0]:
        a.setflags(write=False)
    return tuple(runs[0])


def assert_equals_oracle(oracle, case, got, n, threshold=None):
    for i in range(n):
        want = DC.oracle_cells(oracle, case, i, threshold)
        for g, wv, name in zip(got, want, FIELDS):
            assert np.array_equal(g[i], wv), (case.name, n, i, name, np.nonzero(g[i] != wv)[0][:5], g[i][g[i] != wv][:5], wv[g[i] != wv][:5])


@pytest.mark.parametrize("name", DC.NAMES)
def test_batch_equals_the_oracle_on_every_path(gpu_ctx, device_cells, oracle, name):
    """The whole batch (the select kernel the case names), then its first sub_n frames alone (another select kernel, the same score
    kernels): both equal the oracle frame by frame, hence each other; a case with a twin — the same images in the packed layout —
    returns the twin's cells (padding content is invisible)."""
    case = DC.get(name)
    for n in (case.n, case.sub_n):
        if n is None:
            continue
        got = device_cells(case, n)
        assert_equals_oracle(oracle, case, got, n)
        if n != case.n:
            assert all(np.array_equal(g, f[:n]) for g, f in zip(got, device_cells(case)))
        if case.twin is not None:
            assert all(np.array_equal(g, t) for g, t in zip(got, device_cells(DC.get(case.twin), n)))


@pytest.mark.parametrize("name", DC.THRESHOLD_CASES)
def test_threshold_equal_to_a_score(gpu_ctx, device_cells, oracle, name):
    """detection_threshold exactly a cell's winning score, and the float below it: `>` (:104 against the initial score of :74)"""
    case = DC.get(name)
    k, s, below = DC.threshold_pair(oracle, case)
    for n in (case.n, case.sub_n):
        at, under = device_cells(case, n, s), device_cells(case, n, below)
        assert_equals_oracle(oracle, case, at, n, s)
        assert_equals_oracle(oracle, case, under, n, below)
        assert at[0][0, k] == s and (at[1][0, k], at[2][0, k], at[3][0, k]) == (0, 0, 0)
        assert under[0][0, k] == s and (under[1][0, k], under[2][0, k]) != (0, 0)


@pytest.mark.parametrize("name", DC.SINGLE_FRAME)
def test_single_frame_entry_returns_the_same_cells(gpu_ctx, device_cells, oracle, name):
    """dsdtm_detect_cells on frame 0 as a host pyramid: packed by the library, keys decoded on the host — a second copy of the
    device's decode (ties are where the two could disagree)."""
    case = DC.get(name)
    pyr, keep = capi.pyramid_struct(case.images[0])
    G = case.cells
    prm = DC.params(case)
    occ = np.array(case.occ[0])
    score, cx, cy, cl = np.full(G, -1, np.float32), np.full(G, -1, np.int32), np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    ip = C.POINTER(C.c_int32)
    gpu_ctx.check(gpu_ctx.lib.dsdtm_detect_cells(gpu_ctx.handle, C.byref(pyr), occ.ctypes.data_as(capi.u8p), C.byref(prm),
                                                 score.ctypes.data_as(C.POINTER(C.c_float)), cx.ctypes.data_as(ip), cy.ctypes.data_as(ip),
                                                 cl.ctypes.data_as(ip)))
    batch = device_cells(case)
    for g, wv, b, field in zip((score, cx, cy, cl), DC.oracle_cells(oracle, case, 0), batch, FIELDS):
        assert np.array_equal(g, wv) and np.array_equal(g, b[0]), (name, field, np.nonzero(g != wv)[0][:5])


@pytest.mark.parametrize("name", ["ties_176x100", "ties_180x100"])
def test_tie_frames_differ_from_both_tie_mutants(gpu_ctx, device_cells, oracle, name):
    """the device equals the faithful oracle (above), so in every tie frame it is neither the oracle that lets the last of equal scores
    keep a cell nor the one whose equal neighbours do not suppress each other"""
    case = DC.get(name)
    for n in (case.n, case.sub_n):
        got = device_cells(case, n)
        for i in [i for i, t in enumerate(DC.TIE_FRAMES) if t is not None and i < n]:
            seen = []
            for mut in ("MUT_D_CELLMAX", "MUT_D_NMS_TIE"):
                with oracle_lib.mutant(mut):
                    wrong = DC.oracle_cells(oracle_lib, case, i)
                assert any(not np.array_equal(g[i], wv) for g, wv in zip(got, wrong)), (n, i, mut)
                seen.append(wrong)
            assert seen[0] is not seen[1] and any(not np.array_equal(a, b) for a, b in zip(*seen)), (n, i)   # two mutants, two results


def test_frames_of_different_kinds_keep_their_own_cells(gpu_ctx, device_cells, oracle):
    case = DC.get("kinds_128x80")
    got = device_cells(case)
    thr = np.float32(case.threshold)
    for i in (0, 1, 2):                                                      # flat, checkerboard, every cell occupied: threshold and 0, 0, 0
        assert (got[0][i] == thr).all() and not (got[1][i] | got[2][i] | got[3][i]).any(), i
    assert (got[0][3] > thr).sum() >= 15 and (got[0][4][case.occ[4] == 1] == thr).all()
