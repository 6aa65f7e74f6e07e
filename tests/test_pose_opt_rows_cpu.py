"""The case set of tests/pose_opt_rows_cases.py, held to what tests/test_pose_opt_rows_gpu.py relies on — on the CPU,
with the restatement alone: (1) no problem sits near a decision threshold (the restatement's two linear solvers take
the same decisions on every one), (2) the set reaches the solver's exits, rejected steps and the whole range of
iteration counts, (3) the layout moves every problem through every row of a wavefront and puts frames that stop early
beside frames that go on."""
import numpy as np
import pytest

from dsdtm_amd import capi
from tests import pose_opt_rows_cases as cases

EXACT = ("iterations", "successful_steps", "termination", "n_residual_blocks")
FRAME_COUNTS = (4095, 4096, 4097, 8191, 8192, 8193, 8195)


def _solve(oracle, probs, linear_solver):
    return [oracle.pose_optimization(P.bearing, P.p_world, P.level, P.use, P.T_seed, linear_solver=linear_solver) for P in probs]


@pytest.fixture(scope="module")
def solved(oracle):
    return {name: (probs, _solve(oracle, probs, 1), _solve(oracle, probs, 0))
            for name, probs in (("main", cases.problems()), ("33", cases.problems33()))}


def test_the_set_is_what_the_issue_describes():
    probs = cases.problems()
    assert len(probs) == cases.K == 512 and cases.K % 4 == 0
    n = np.array([len(P.use) for P in probs])
    assert n[:cases.N_RANDOM].min() == 1 and n[:cases.N_RANDOM].max() == 48 and n.max() == cases.MAX_FEATURES
    keys = {(P.bearing.tobytes(), P.p_world.tobytes(), P.use.tobytes(), P.level.tobytes(), P.T_seed.tobytes()) for P in probs}
    assert len(keys) == cases.K                                     # distinct
    pl = {name: probs[cases.planted_index(name)] for name in cases.PLANTED}
    assert len(pl["zero_features"].use) == 0
    assert len(pl["nothing_used"].use) > 0 and not pl["nothing_used"].use.any()
    for name, cnt in (("n1", 1), ("n16", 16), ("n17", 17), ("n32", 32), ("n33", 33), ("n48", 48)):
        assert len(pl[name].use) == cnt and pl[name].use.all()
    assert len(pl["only_47"].use) == 48 and list(np.nonzero(pl["only_47"].use)[0]) == [47]
    P = pl["evaluation_failure"]
    assert np.array_equal(P.T_seed, np.eye(4)[:3]) and np.any((P.p_world[:, 2] == 0.0) & (P.use != 0))
    for P in cases.problems33():
        assert len(P.use) == 33
    u32 = [int(P.use[32]) for P in cases.problems33()]
    assert 0 in u32 and 1 in u32                                    # the one lane of the last trip: live and not
    again = cases.pack(probs, cases.layout(9), cases.MAX_FEATURES)  # deterministic
    assert again.bearing.tobytes() == cases.pack(probs, cases.layout(9), cases.MAX_FEATURES).bearing.tobytes()


@pytest.mark.parametrize("name", ["main", "33"])
def test_no_problem_sits_on_a_threshold(solved, name):
    probs, ne, qr = solved[name]
    for k, ((Ta, ra, sa), (Tb, rb, sb)) in enumerate(zip(ne, qr)):
        for q in EXACT:
            assert sa[q] == sb[q], (k, q, sa, sb)
        assert np.abs(Ta - Tb).max() <= 1e-10, k
        assert ra.shape == rb.shape and np.allclose(ra, rb, rtol=0, atol=1e-10), k      # (equal infinities pass, a NaN does not)


def test_the_set_covers_the_decisions(solved):
    _, ne, _ = solved["main"]
    sm = [s for _, _, s in ne]
    rnd = sm[:cases.N_RANDOM]
    term = [s["termination"] for s in rnd]
    for t in (capi.PO_FUNCTION_TOLERANCE, capi.PO_PARAMETER_TOLERANCE, capi.PO_GRADIENT_TOLERANCE, capi.PO_MAX_ITERATIONS):
        assert term.count(t) >= 1, (t, term.count(t))
    assert sm[cases.planted_index("zero_features")]["termination"] == capi.PO_NO_RESIDUALS
    assert sm[cases.planted_index("nothing_used")]["termination"] == capi.PO_NO_RESIDUALS
    assert sm[cases.planted_index("evaluation_failure")]["termination"] == capi.PO_EVALUATION_FAILED
    for name, cnt in (("n1", 1), ("n16", 16), ("n17", 17), ("n32", 32), ("n33", 33), ("n48", 48), ("only_47", 1)):
        assert sm[cases.planted_index(name)]["n_residual_blocks"] == cnt
    assert sum(s["successful_steps"] < s["iterations"] - 1 for s in sm) >= 100
    its = [s["iterations"] for s in sm]
    assert min(its) == 0 and max(its) == 100
    # every count an iteration cap of 4 tells apart: ended by itself at 3, at 4, and stopped by the cap
    assert its.count(3) >= 10 and its.count(4) >= 10 and sum(i > 4 for i in its) >= 100


def test_pack_poisons_and_guards():
    probs = cases.problems()
    f2p = cases.layout(37)
    i48 = cases.planted_index("n48")
    pk = cases.pack(probs, f2p, cases.MAX_FEATURES, guard_frames=4, over_count=(i48, 60))
    F, M = 37, cases.MAX_FEATURES
    assert pk.bearing.shape == (F + 4, M, 3) and pk.summary.shape[0] == F + 4 and pk.n_features.dtype == np.int32
    for f in range(F):
        P = probs[f2p[f]]
        n = len(P.use)
        assert pk.n_features[f] == (60 if f2p[f] == i48 else n)
        assert np.array_equal(pk.bearing[f, :n], P.bearing) and np.array_equal(pk.use[f, :n], P.use)
        assert np.array_equal(pk.p_world[f, :n], P.p_world) and np.array_equal(pk.level[f, :n], P.level)
        assert np.isnan(pk.bearing[f, n:]).all() and np.isnan(pk.p_world[f, n:]).all()
        assert (pk.level[f, n:] == 40).all() and (pk.use[f, n:] == 1).all()
        assert np.array_equal(pk.T_cur_w[f], P.T_seed.reshape(12))
    assert (pk.residual_norm[:F] == -1.0).all()
    for a in (pk.T_cur_w, pk.summary, pk.residual_norm):
        assert set(a[F:].tobytes()) == {cases.SENTINEL}
    assert set(pk.summary.tobytes()) == {cases.SENTINEL}


@pytest.mark.parametrize("group", [2, 4])
def test_the_layout_mixes_neighbours(solved, group):
    _, ne, _ = solved["main"]
    its = np.array([s["iterations"] for _, _, s in ne])
    term = np.array([s["termination"] for _, _, s in ne])
    solving = its > 0
    n_frames = 4097 if group == 2 else 8195
    f2p = cases.layout(n_frames)
    at_row = np.zeros((cases.K, group), bool)
    at_row[f2p, np.arange(n_frames) % group] = True
    assert at_row.all()                                             # every problem at every row index
    full = n_frames // group * group
    w = f2p[:full].reshape(-1, group)                               # the problems of every full wavefront
    for stops in (capi.PO_NO_RESIDUALS, capi.PO_EVALUATION_FAILED):
        assert np.any((term[w] == stops).any(1) & solving[w].any(1)), stops
    assert np.any(np.abs(np.diff(its[w], axis=1)) >= 50)                  # side by side
    # the same problem beside different neighbours
    mates = {}
    for row in w:
        for p in row:
            mates.setdefault(int(p), set()).add(tuple(int(q) for q in row if q != p))
    assert min(len(m) for m in mates.values()) >= 2


def test_every_problem_occurs_often_enough():
    for n_frames in FRAME_COUNTS:
        cnt = np.bincount(cases.layout(n_frames), minlength=cases.K)
        assert cnt.min() >= (8 if n_frames >= 4096 else 7), (n_frames, cnt.min())
