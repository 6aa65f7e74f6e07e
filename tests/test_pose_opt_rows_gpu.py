"""The batch kernels of pose refinement that carry several frames per wavefront — pose_opt_rows_kernel<2> (4096 to 8191
frames, 32 lanes a frame) and pose_opt_rows_kernel<4> (8192 frames and more, one 16-lane row a frame) — against the CPU
restatement (normal-equation form), through dsdtm_pose_optimization_batch_device as pose_opt_launch picks them by the
frame count. What these kernels have and the one-frame-per-wave kernel has not: a trust-region loop in divergent
control flow beside rows in other states, row results cut out of whole-wave ballots, column sums per row, dead rows
in the last wavefront and feature strides of 16 / 32. The cases (tests/pose_opt_rows_cases.py, held to their
conditions by tests/test_pose_opt_rows_cpu.py) put every problem in every row, beside varying neighbours.

Every frame of a launch is compared: the frames of one problem are reduced to their distinct result bytes (pose,
summary, the whole residual-norm row) and every distinct result goes through assert_same of tests/test_pose_opt_gpu.py,
with its tolerances."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi
from tests import pose_opt_rows_cases as cases
from tests.test_pose_opt_gpu import assert_same

pytestmark = pytest.mark.gpu

FRAME_COUNTS = (4095, 4096, 4097, 8191, 8192, 8193, 8195)
SETS = {"main": cases.problems, "33": cases.problems33}

_REF = {}


@pytest.fixture(scope="module")
def ref(oracle):
    """The restatement of one problem under one iteration cap, computed once."""
    def get(name, k, cap=100):
        key = (name, k, cap)
        if key not in _REF:
            P = SETS[name]()[k]
            _REF[key] = oracle.pose_optimization(P.bearing, P.p_world, P.level, P.use, P.T_seed, cap, 1)
        return _REF[key]
    return get


class Result:
    pass


def launch(ctx, pk, cap=100, pass_counts=True):
    """One call on a stream of its own; returns the three in/out arrays with their guard frames."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)
    d_b, d_p, d_l, d_u, d_n = t(pk.bearing), t(pk.p_world), t(pk.level), t(pk.use), t(pk.n_features)
    d_T, d_rn, d_sm = t(pk.T_cur_w), t(pk.residual_norm), t(pk.summary)
    prm = capi.PoseOptParams(cap, 0)
    f = ctx.lib.dsdtm_pose_optimization_batch_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.POINTER(capi.PoseOptParams), C.c_void_p, C.c_void_p, C.c_void_p]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.check(f(ctx.handle, pk.n_frames, pk.max_features, d_n.data_ptr() if pass_counts else None, d_b.data_ptr(), d_p.data_ptr(),
                    d_l.data_ptr(), d_u.data_ptr(), d_T.data_ptr(), C.byref(prm), d_rn.data_ptr(), d_sm.data_ptr(), s.cuda_stream))
    s.synchronize()
    r = Result()
    r.T, r.rn, r.sm = d_T.cpu().numpy(), d_rn.cpu().numpy(), d_sm.cpu().numpy()
    return r


def frame_bytes(pk, r):
    """(n_frames, bytes): everything the kernel may write for a frame."""
    F = pk.n_frames
    return np.concatenate([np.ascontiguousarray(r.T[:F]).view(np.uint8), r.sm[:F], np.ascontiguousarray(r.rn[:F]).view(np.uint8)], axis=1)


def assert_guards_untouched(pk, r):
    F = pk.n_frames
    for got, was in ((r.T, pk.T_cur_w), (r.sm, pk.summary), (r.rn, pk.residual_norm)):
        assert got.shape == was.shape and got[F:].tobytes() == was[F:].tobytes()
        assert set(got[F:].tobytes()) == {cases.SENTINEL}


def assert_batch_equals_the_restatement(pk, r, ref, name, cap=100):
    """Every frame against the restatement of its problem; returns the number of distinct results per problem."""
    F, M = pk.n_frames, pk.max_features
    assert_guards_untouched(pk, r)
    rows = frame_bytes(pk, r)
    nT, nS = 12 * 8, r.sm.shape[1]
    compared = 0
    variants = {}
    for p in np.unique(pk.frame_to_problem):
        idx = np.nonzero(pk.frame_to_problem == p)[0]
        uniq = np.unique(rows[idx], axis=0)
        variants[int(p)] = len(uniq)
        cpu = ref(name, int(p), cap)
        for u in uniq:
            what = f"problem {p}: frames {idx[(rows[idx] == u).all(1)][:8]}"
            T = u[:nT].view(np.float64).reshape(3, 4)
            sm = capi.PoseOptSummary.from_buffer_copy(u[nT:nT + nS].tobytes()).as_dict()
            rn = u[nT + nS:].view(np.float64)
            nb = sm["n_residual_blocks"]
            assert 0 <= nb <= M, (what, sm)
            assert_same((T, rn[:nb], sm), cpu, what)
            assert np.all(rn[nb:] == -1.0), what                    # nothing written past the block count
        compared += len(idx)
    assert compared == F                                            # no frame left out
    return variants


def packed_main(n_frames, **kw):
    return cases.pack(cases.problems(), cases.layout(n_frames), cases.MAX_FEATURES, **kw)


@pytest.mark.parametrize("n_frames", FRAME_COUNTS)
def test_frame_counts(gpu_ctx, ref, n_frames):
    """4095: the last count of the one-wave kernel; 4096 / 8192: the first of each rows kernel; 4097, 8191, 8193, 8195: last
    wavefronts with 1 of 2, 1 of 2, 1 of 4 and 3 of 4 live rows. Ragged feature counts (0..48 of 48), cap 100."""
    pk = packed_main(n_frames)
    assert_batch_equals_the_restatement(pk, launch(gpu_ctx, pk), ref, "main")


@pytest.mark.parametrize("n_frames", [4097, 8195])
def test_nothing_crosses_a_row(gpu_ctx, n_frames):
    """All copies of a problem — in every row, beside different neighbours — give the same bits, and so does a second launch."""
    pk = packed_main(n_frames)
    r1 = launch(gpu_ctx, pk)
    rows = frame_bytes(pk, r1)
    for p in range(cases.K):
        idx = np.nonzero(pk.frame_to_problem == p)[0]
        assert len(idx) >= 8
        differ = idx[(rows[idx] != rows[idx[0]]).any(1)]
        assert len(differ) == 0, (p, idx[0], differ)
    r2 = launch(gpu_ctx, pk)
    assert r1.T.tobytes() == r2.T.tobytes() and r1.sm.tobytes() == r2.sm.tobytes() and r1.rn.tobytes() == r2.rn.tobytes()
    assert_guards_untouched(pk, r1)


@pytest.mark.parametrize("n_frames", [4096, 8192])
def test_all_features_used(gpu_ctx, ref, n_frames):
    """n_features == NULL, max_features = 33: every frame takes all 33 columns, one lane is live in the last trip of both strides."""
    pk = cases.pack(cases.problems33(), cases.layout(n_frames, cases.K33), 33)
    assert_batch_equals_the_restatement(pk, launch(gpu_ctx, pk, pass_counts=False), ref, "33")


@pytest.mark.parametrize("cap", [4, 0])
def test_iteration_caps(gpu_ctx, ref, cap):
    """Cap 4: rows that converged at 3 or 4 iterations beside rows the cap stops; cap 0: norms at the seed pose."""
    pk = packed_main(8195)
    assert_batch_equals_the_restatement(pk, launch(gpu_ctx, pk, cap), ref, "main", cap)
    its = [ref("main", p, cap)[2]["iterations"] for p in range(cases.K)]
    assert max(its) == cap


@pytest.mark.parametrize("n_frames", [4097, 8195])
def test_feature_count_above_max_features_is_clamped(gpu_ctx, ref, n_frames):
    """n_features[f] = 60 with max_features = 48 gives the result of 48 — also in the batch's last frame, where column 48 on
    is the guard space behind the arrays' last frame."""
    i48 = cases.planted_index("n48")
    f2p = cases.layout(n_frames)
    f2p[-1] = i48
    pk = cases.pack(cases.problems(), f2p, cases.MAX_FEATURES, over_count=(i48, 60))
    assert np.all(pk.n_features[:n_frames][f2p == i48] == 60) and np.count_nonzero(f2p == i48) >= 8
    assert_batch_equals_the_restatement(pk, launch(gpu_ctx, pk), ref, "main")
