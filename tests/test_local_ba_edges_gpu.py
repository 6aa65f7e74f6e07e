"""dsdtm_local_ba / dsdtm_local_ba_batch_device at the exits of the trust-region loop and at the edges of the problem's
structure (the worlds of tests/local_ba_edges.py), held to the numpy restatement as tests/test_local_ba_gpu.py holds the grid:
termination, iteration and step counts, residual blocks and outlier flags identical, poses / points / costs within TOL_DEFAULT.
Every world is decidable (tests/test_local_ba_cpu.py asserts it, and again here), so no termination or count is left out.
A problem in a batch gives the bits of its single call, whatever lies beside it; a duplicate observation is refused by both
entries with nothing written."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi
from dsdtm_amd.optimizer import local_bundle_adjustment
from tests import local_ba_edges as E
from tests import local_ba_restatement as R
from tests.test_local_ba_gpu import TOL, TOL_DEFAULT, _batch, _pack, _summaries, compare, cost_rounding, decidable, device

pytestmark = pytest.mark.gpu


def _run(ctx, name):
    """The device against the restatement on one edge world: the compare() assertions; returns (world, device, reference)."""
    w, ref, tr = E.reference(name)
    with np.errstate(all="ignore"):
        ok = decidable(w, ref[0], ref[1], tr, TOL.get(name, TOL_DEFAULT))
    dev = device(ctx, w, E.MAX_ITERATIONS.get(name, 10))
    # the two worlds without noise: their residuals are the rounding of their own subtraction (and, with one point moved by
    # 1e-7, eight digits above it), so their costs are held to what that rounding can do, not to 1e-10 of themselves
    exact = name in ("gradient", "parameter_no_step")
    compare(w, dev, ref, name, ok, atol_initial=cost_rounding(w, w.T, w.points) if exact else 0.0,
            atol_final=cost_rounding(w, ref[0], ref[1]) if exact else 0.0)
    return w, dev, ref


@pytest.mark.parametrize("name", list(E.EXITS))
def test_every_exit_equals_the_restatement(gpu_ctx, name):
    _, _, termination, iterations, successful = E.EXITS[name]
    w, (T, X, out, sm), (Tr, Xr, outr, smr) = _run(gpu_ctx, name)
    assert (sm["termination"], sm["iterations"], sm["successful_steps"]) == (termination, iterations, successful)
    if name in ("parameter_no_step", "parameter_and_function"):       # the candidate is evaluated, not accepted
        assert np.array_equal(X, w.points)
    # ("parameter_and_function": both tolerances hold at iteration 1, so the termination asserted above is the ORDER of the
    # two tests; tests/test_local_ba_cpu.py shows that the other order ends on FUNCTION_TOLERANCE)
    if name in ("parameter_long", "function_long"):         # x, not the candidate the loop ended on (compare() holds X to Xr)
        assert np.array_equal(out, outr)
    if name == "evaluation_failed":
        assert sm["initial_cost"] == 0.0 and sm["final_cost"] == 0.0
        assert np.array_equal(X, w.points)
        assert np.abs(T - w.T).max() < 1e-12                # re-normalised, nothing else
        assert np.array_equal(out, outr) and sm["n_outliers"] == smr["n_outliers"] == 216
    if name == "no_residuals":
        assert sm["n_outliers"] == 0 and sm["n_free_keyframes"] == 0 and len(out) == 0
        assert sm["initial_cost"] == 0.0 and sm["final_cost"] == 0.0
        assert np.array_equal(X, w.points) and np.abs(T - w.T).max() < 1e-12
    if name == "cap0":                                       # the outlier pass at the input poses
        assert np.array_equal(out, outr) and np.array_equal(X, w.points) and np.abs(T - w.T).max() < 1e-12
        assert sm["final_cost"] == sm["initial_cost"]


def test_no_residuals_with_no_point_and_null_pointers(gpu_ctx):
    """n_points == 0, n_observations == 0 and NULL for every array they size: legal in the single entry."""
    w = E.world("no_residuals")
    T = w.T.reshape(-1).copy()
    kc = np.ascontiguousarray(w.constant, np.uint8)
    prm = capi.LocalBaParams(10, 0, w.delta)
    sm = capi.LocalBaSummary()
    # a prototype of its own from the symbol's address (every array as void*, so that None is NULL): the shared function
    # object of the binding keeps its declared types
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.POINTER(capi.LocalBaParams), C.c_void_p, C.POINTER(capi.LocalBaSummary))
    f = proto(C.cast(gpu_ctx.lib.dsdtm_local_ba, C.c_void_p).value)
    gpu_ctx.check(f(gpu_ctx.handle, len(w.T), T.ctypes.data, kc.ctypes.data, 0, None, 0, None, None, None, None, C.byref(prm),
                    None, C.byref(sm)))
    d = sm.as_dict()
    assert d["termination"] == R.NO_RESIDUALS and d["iterations"] == 0 and d["successful_steps"] == 0
    assert d["n_residual_blocks"] == 0 and d["n_outliers"] == 0 and d["n_free_keyframes"] == 0
    assert d["initial_cost"] == 0.0 and d["final_cost"] == 0.0
    assert np.abs(T.reshape(-1, 3, 4) - w.T).max() < 1e-12


@pytest.mark.parametrize("name", list(E.STRUCTURE))
def test_every_structure_edge_equals_the_restatement(gpu_ctx, name):
    w, (T, X, out, sm), (Tr, Xr, outr, smr) = _run(gpu_ctx, name)
    seen_p = np.bincount(w.obs_pt, minlength=len(w.points)) > 0
    seen_k = np.bincount(w.obs_kf, minlength=len(w.T)) > 0
    assert sm["n_free_keyframes"] == int((seen_k & ~w.constant).sum())
    assert np.array_equal(X[~seen_p], w.points[~seen_p])     # a point nobody observes comes back bit for bit
    still = ~(seen_k & ~w.constant)                          # constant or unobserved: only re-normalised
    assert np.abs(T[still] - w.T[still]).max() < 1e-12
    assert np.abs(X[seen_p] - w.points[seen_p]).max() > 1e-6
    if (~still).any():
        assert np.abs(T[~still] - w.T[~still]).max() > 1e-6
    if name == "unobserved_points":
        assert list(np.nonzero(~seen_p)[0]) == list(E.UNOBSERVED_POINTS)
    if name == "unobserved_keyframe":
        assert sm["n_free_keyframes"] == 3 and still[E.UNOBSERVED_KF]
    if name == "no_pose_block":
        assert sm["n_free_keyframes"] == 0 and sm["successful_steps"] > 0 and (~seen_p).any()
        assert np.abs(X - w.points)[seen_p].max() > 1e-3    # the points move, as in the restatement (compare())
    if name == "one_observation":
        assert sm["n_residual_blocks"] == 1 and sm["n_free_keyframes"] == 1
    if name == "free11":
        assert sm["n_free_keyframes"] == 11
    if name == "kf80":
        assert len(w.T) == 80 and sm["n_free_keyframes"] == 16
    if name == "dense_pairs":
        assert sm["n_free_keyframes"] == 16 and sm["n_residual_blocks"] >= 16 * 40


def _empty():
    """A problem of keyframes alone: no point, no observation."""
    w = E.world("no_residuals")
    w.points = np.zeros((0, 3))
    return w


# one batch per iteration cap (a batch shares it); the problems that end before the loop lie between ordinary ones
BATCHES = {
    10: ["unobserved_points", "evaluation_failed", "free11", "no_residuals", "kf80", "<empty>", "gradient", "dense_pairs",
         "parameter_no_step", "one_observation", "parameter_and_function", "no_pose_block", "all_levels",
         "unobserved_keyframe"],
    0: ["unobserved_points", "cap0", "no_pose_block"],
    1: ["no_pose_block", "cap1", "evaluation_failed", "unobserved_points"],
    100: ["unobserved_keyframe", "parameter_long", "no_residuals", "all_levels"],
    300: ["one_observation", "function_long", "unobserved_points"],
}


def test_every_edge_world_is_in_a_batch():
    assert {n for names in BATCHES.values() for n in names} == set(E.EXITS) | set(E.STRUCTURE) | {"<empty>"}
    for name in ("cap0", "cap1", "parameter_long", "function_long"):      # in the batch of their own iteration cap
        assert name in BATCHES[E.MAX_ITERATIONS[name]]


@pytest.mark.parametrize("max_iterations", list(BATCHES))
def test_batch_of_edge_worlds_equals_the_single_calls_bit_for_bit(gpu_ctx, max_iterations):
    names = BATCHES[max_iterations]
    worlds = [_empty() if n == "<empty>" else E.reference(n)[0] for n in names]
    delta = worlds[0].delta
    assert all(w.delta == delta for w in worlds)
    probs, a = _pack(worlds)
    assert _batch(gpu_ctx, probs, a, delta, max_iterations=max_iterations) == capi.OK
    sms = _summaries(a, len(worlds))
    T, X, out = a["T"].cpu().numpy(), a["X"].cpu().numpy(), a["out"].cpu().numpy()
    ko = po = oo = 0
    for j, w in enumerate(worlds):
        Ts, Xs, outs, sm = device(gpu_ctx, w, max_iterations)
        K, P, N = len(w.T), len(w.points), len(w.obs_kf)
        assert np.array_equal(T[12 * ko:12 * (ko + K)], Ts.reshape(-1)), names[j]
        assert np.array_equal(X[3 * po:3 * (po + P)], Xs.reshape(-1)), names[j]
        assert np.array_equal(out[oo:oo + N], outs), names[j]
        for k in capi.LBA_SUMMARY_DTYPE.names:
            assert sms[j][k] == sm[k], (names[j], k)
        if names[j] in E.EXITS and E.MAX_ITERATIONS[names[j]] == max_iterations:
            assert (sm["termination"], sm["iterations"], sm["successful_steps"]) == E.EXITS[names[j]][2:], names[j]
        ko += K; po += P; oo += N
    assert oo == 0 or (out[oo:] == 7).all()


def _with_duplicate(w):
    """Observation 11 repeated: its keyframe observes its point twice (the order by point holds)."""
    idx = np.sort(np.concatenate([np.arange(len(w.obs_kf)), [11]]))
    return R.keep_observations(w, idx)


def test_a_duplicate_observation_is_refused_by_both_entries(gpu_ctx):
    import torch
    good = E.reference("unobserved_points")[0]
    bad = _with_duplicate(good)
    # the single entry: checked on the host, nothing copied, nothing written
    T, X = bad.T.reshape(-1).copy(), bad.points.reshape(-1).copy()
    with pytest.raises(capi.DsdtmError) as e:
        local_bundle_adjustment(gpu_ctx, T, bad.constant, X, bad.obs_kf, bad.obs_pt, bad.bearing, bad.level, bad.delta)
    assert e.value.status == capi.ERR_INVALID
    msg = str(e.value)
    assert f"keyframe {bad.obs_kf[11]} observes point {bad.obs_pt[11]} twice" in msg, msg
    assert np.array_equal(T, bad.T.reshape(-1)) and np.array_equal(X, bad.points.reshape(-1))
    # the batch entry: checked by a kernel, one bad problem and no problem is written
    for worlds in ([good, bad, good], [bad], [good, good, bad]):
        probs, a = _pack(worlds)
        T0, X0 = a["T"].clone(), a["X"].clone()
        assert _batch(gpu_ctx, probs, a, good.delta) == capi.ERR_INVALID
        msg = gpu_ctx.lib.dsdtm_last_error(gpu_ctx.handle).decode()
        assert "a keyframe observes a point twice" in msg and f"problem {worlds.index(bad)}" in msg, msg
        assert torch.equal(a["T"], T0) and torch.equal(a["X"], X0)
        assert (a["out"] == 7).all() and (a["sm"] == 0x5A).all()
    probs, a = _pack([good, good])                           # and a valid batch after the refused ones runs
    assert _batch(gpu_ctx, probs, a, good.delta) == capi.OK
    assert (_summaries(a, 2)["n_residual_blocks"] == len(good.obs_kf)).all()
