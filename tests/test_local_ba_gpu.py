"""dsdtm_local_ba / dsdtm_local_ba_batch_device — Optimizer::LocalBundleAdjustment on the device, held to the numpy
restatement (tests/local_ba_restatement.py, Schur form) on a grid of worlds: the decisions (iterations, successful steps,
termination, residual blocks, every outlier flag) must be identical, poses and points within the tolerance of
DESIGN.md §3.7, costs within rtol 1e-10. A problem in a batch gives the bits of its single call, two launches give the same
bits, the checks write nothing, and Optimizer.LocalBundleAdjustment runs end to end on an object-graph map."""
import ctypes as C
import threading

import numpy as np
import pytest

from dsdtm_amd import capi
from dsdtm_amd.optimizer import Optimizer, local_bundle_adjustment
from tests import local_ba_restatement as R

pytestmark = pytest.mark.gpu

# per world, (keyframe poses m / rad, points m, final-cost rtol). Well-conditioned worlds agree to ~1e-11.
# After 10 weakly damped LM iterations, worlds with points seen over short baselines carry rounding amplified by their
# condition number (measured on the device: "f10" 4e-7 / 8e-7 / 7e-8, "f16_16k" points 3e-7, "far" points 1e-6).
TOL = {"f4": (1e-6, 1e-6, 1e-8), "f10": (1e-6, 2e-6, 2e-7), "f16": (1e-9, 1e-6, 1e-10), "f16_16k": (1e-9, 1e-6, 1e-10),
       "far": (1e-9, 1e-5, 1e-10), "outliers": (1e-9, 1e-7, 1e-10)}
TOL_DEFAULT = (1e-9, 1e-9, 1e-10)
TOL_ONCE = 1e-6        # m: points seen ONCE (depth set by the damping alone)
RTOL_COST = 1e-10      # initial cost

# name -> make_world arguments; the grid of the issue (free keyframes 1/4/10/16, fixed 0..40, points 50..16 384, a point seen
# once, a free keyframe with mlId == 0, heavy outliers, a start far enough out that steps are rejected)
WORLDS = {
    "f1": dict(seed=11, n_free=1, n_fixed=3, n_points=50),
    "f4": dict(seed=12, n_free=4, n_fixed=8, n_points=400),
    "f4_nofixed": dict(seed=13, n_free=4, n_fixed=0, n_points=300),
    "f10": dict(seed=14, n_free=10, n_fixed=20, n_points=3000),
    "f16": dict(seed=15, n_free=16, n_fixed=40, n_points=2000),
    "f16_16k": dict(seed=16, n_free=16, n_fixed=0, n_points=16384, max_obs=3),
    "once": dict(seed=17, n_free=4, n_fixed=4, n_points=200, once_frac=0.3),
    "mlid0": dict(seed=18, n_free=4, n_fixed=4, n_points=300, zero_id=0),
    "outliers": dict(seed=19, n_free=4, n_fixed=6, n_points=400, outlier_frac=0.3),
    "far": dict(seed=21, n_free=4, n_fixed=4, n_points=300, pose_noise=(0.15, 0.5), point_noise=0.6),
}


def world(name):
    kw = dict(WORLDS[name])
    return R.make_world(kw.pop("seed"), **kw)


def device(ctx, w, max_iterations=10):
    T = w.T.reshape(-1).copy()
    X = w.points.reshape(-1).copy()
    out, sm = local_bundle_adjustment(ctx, T, w.constant, X, w.obs_kf, w.obs_pt, w.bearing, w.level, w.delta, max_iterations)
    return T.reshape(-1, 3, 4), X.reshape(-1, 3), out, sm


ROUND0 = 1e-6         # relative: far above (condition number of one damped solve) x 2^-53, see exits_decidable


def exits_decidable(w, trace, tol):
    """The three tolerance tests of the loop, held to the reasoning of the acceptance ratio: at every test the restatement
    made, the quantity must lie farther from its bound than a deviation of the size the world is tolerated to have (tol) can
    move it, or the termination and the counts would not be decided. The margins, two times what the deviation can do:
      function   |cost - candidate cost| against 1e-6 cost: both costs within rtol cost, the bound moves by 1e-6 of that;
      parameter  |x - candidate| against 1e-8 (|x| + 1e-8): iterates that differ by d give steps that differ by no more than
                 about |d| (a weakly damped Gauss-Newton step towards the same minimum),
                 |d| <= sqrt(6 F tol_pose^2 + 3 Q tol_pt^2), and the bound moves by 1e-8 |d|;
      gradient   max |x - Plus(x, -g)| against 1e-10. Below the bound: dg = J^T J d, bounded column by column with absolute
                 values (trace: sens_pose, sens_point). Above it: the test can only flip where EVERY component of g
                 vanishes, at a stationary point, and the step the loop takes next is the distance to it (to first order,
                 the damping being weak): that step must be longer than 2 |d|.
    Before the first accepted step the iterate IS the input, bit for bit on both sides, and only rounding separates them:
    the gradient by the rounding of the residuals' own subtraction (trace: ground; in a world without noise the residuals
    are nothing else), the step and the cost change by far less than ROUND0 of themselves."""
    tol_pose, tol_pt, rtol = tol
    seen_k = np.bincount(w.obs_kf, minlength=len(w.T)) > 0
    F = int((seen_k & ~w.constant).sum())
    Q = int((np.bincount(w.obs_pt, minlength=len(w.points)) > 0).sum())
    d = np.sqrt(6.0 * F * tol_pose ** 2 + 3.0 * Q * tol_pt ** 2)
    for j, t in enumerate(trace):
        if t[0] == "gradient":
            gmax, bound, accepted, ground, sens_pose, sens_pt = t[2:8]
            if not accepted:
                ok = abs(gmax - bound) > 2.0 * ground
            elif gmax <= bound:
                ok = bound - gmax > 2.0 * (tol_pose * sens_pose + tol_pt * sens_pt)
            else:
                nxt = [u[2] for u in trace[j + 1:] if u[0] == "parameter"][:1]
                ok = not nxt or nxt[0] > 2.0 * d
            assert ok, ("world sits on a gradient-tolerance near-tie", t[1], gmax)
        elif t[0] == "parameter":
            step, bound, accepted = t[2:5]
            margin = 2.0 * d * (1.0 + 1e-8) if accepted else ROUND0 * step
            assert abs(step - bound) > margin, ("world sits on a parameter-tolerance near-tie", t[1], step, bound, margin)
        elif t[0] == "function":
            change, bound, accepted, cost = t[2:6]
            margin = 4.0 * rtol * cost * (1.0 + 1e-6) if accepted else ROUND0 * change
            assert abs(change - bound) > margin, ("world sits on a function-tolerance near-tie", t[1], change, bound, margin)


def decidable(w, ref_T, ref_X, trace, tol):
    """Near ties, with margins sized from the tolerance the world is held to. The step decisions: no step ratio may sit closer
    to the acceptance bound 1e-3 than a cost deviation of rtol moves it (the world would be excluded: none of the grid is).
    The outlier flags: an observation whose error lies closer to delta^2 than a pose / point deviation within the tolerance
    can move it has no decided flag; returns the mask of the observations whose flag is decided (the others, < 1 %, are not
    compared)."""
    tol_pose, tol_pt, rtol = tol
    for t in trace:
        if t[0] == "ratio":
            rho, cost, model_change = t[2], t[3], t[4]
            assert abs(rho - 1e-3) > 4.0 * rtol * cost / model_change, "world sits on an acceptance near-tie"
    exits_decidable(w, trace, tol)
    once = (np.bincount(w.obs_pt, minlength=len(w.points)) == 1)[w.obs_pt]
    pc = np.einsum("nij,nj->ni", ref_T[w.obs_kf, :, :3], ref_X[w.obs_pt]) + ref_T[w.obs_kf, :, 3]
    u = pc[:, :2] / pc[:, 2:3]
    e = w.bearing[:, :2] / w.bearing[:, 2:3] - u
    err = (e * e).sum(1)
    # |d pc| <= tol_pose (1 + |X|) + tol_pt (rotation, translation, point); |d u| <= (1 + |u|) |d pc| / z per coordinate
    dpc = tol_pose * (1.0 + np.linalg.norm(ref_X[w.obs_pt], axis=1)) + np.where(once, max(tol_pt, TOL_ONCE), tol_pt)
    du = (1.0 + np.abs(u).max(1)) * dpc / np.abs(pc[:, 2])
    margin = 2.0 * np.sqrt(2.0 * err) * du + 2.0 * du * du
    ok = np.abs(err - w.delta * w.delta) > margin
    assert (~ok).sum() <= 0.01 * len(ok), ("too many outlier near-ties", int((~ok).sum()))
    return ok


_REF = {}


def reference(name):
    if name not in _REF:
        w = world(name)
        tr = []
        _REF[name] = (w, R.solve(w, trace=tr), tr)
    return _REF[name]


def cost_rounding(w, T, X):
    """What the rounding of the residuals' own subtraction can move the cost at poses T and points X by: every residual
    component r = (observed - projected) / 2^level carries an absolute error of rho = 2^-50 (|observed| + |projected|) / 2^level
    (8 ulp of the larger operand: the division of the bearing, the projection and the subtraction), and the cost
    1/2 sum loss(r^2), loss' <= 1, moves by no more than sum (|r| rho + rho^2 / 2). Some 1e-14 of the cost of a world with
    pixel noise; all there is to the cost of a world without, whose residuals are nothing but that rounding."""
    pc = np.einsum("nij,nj->ni", T[w.obs_kf, :, :3], X[w.obs_pt]) + T[w.obs_kf, :, 3]
    obs, proj = w.bearing[:, :2] / w.bearing[:, 2:3], pc[:, :2] / pc[:, 2:3]
    scale = (1 << w.level).astype(np.float64)[:, None]
    rho = 2.0 ** -50 * (np.abs(obs) + np.abs(proj)) / scale
    return float((np.abs(obs - proj) / scale * rho + 0.5 * rho * rho).sum())


def compare(w, dev, ref, what="", decided=None, atol_initial=0.0, atol_final=0.0):
    """atol_*: an absolute allowance beside the relative one, for worlds whose cost is at the rounding of its own residuals
    (cost_rounding); the worlds of this file have none."""
    T, X, out, sm = dev
    Tr, Xr, outr, smr = ref
    tol_pose, tol_pt, rtol_final = TOL.get(what, TOL_DEFAULT)
    for k in ("iterations", "successful_steps", "termination", "n_residual_blocks"):
        assert sm[k] == smr[k], (what, k, sm[k], smr[k])
    assert sm["n_outliers"] == int(out.sum())
    d = np.ones(len(out), bool) if decided is None else decided
    assert np.array_equal(out[d], outr[d]), (what, "outlier flags", np.nonzero((out != outr) & d)[0][:10])
    assert np.allclose(sm["initial_cost"], smr["initial_cost"], rtol=RTOL_COST, atol=atol_initial), what
    assert np.allclose(sm["final_cost"], smr["final_cost"], rtol=rtol_final, atol=atol_final), what
    assert np.abs(T - Tr).max() <= tol_pose, (what, np.abs(T - Tr).max())
    once = np.bincount(w.obs_pt, minlength=len(w.points)) == 1
    dX = np.abs(X - Xr).max(1)
    assert (dX[~once].max(initial=0) <= tol_pt), (what, dX[~once].max(initial=0))
    assert (dX[once].max(initial=0) <= TOL_ONCE), (what, dX[once].max(initial=0))


@pytest.mark.parametrize("name", list(WORLDS))
def test_device_equals_the_restatement(gpu_ctx, name):
    w, ref, tr = reference(name)
    ok = decidable(w, ref[0], ref[1], tr, TOL.get(name, TOL_DEFAULT))
    dev = device(gpu_ctx, w)
    compare(w, dev, ref, name, ok)
    if name == "far":
        assert ref[3]["successful_steps"] < ref[3]["iterations"], "the far start must reject a step"
    if name == "mlid0":                                       # the mlId == 0 keyframe is constant: only re-normalised
        assert np.abs(dev[0][0] - w.T[0]).max() < 1e-12
    if name == "outliers":
        assert dev[3]["n_outliers"] > 0.2 * len(w.obs_kf)


def _mutant_differs(w, dev, mut):
    T, X, out, sm = dev
    Tm, Xm, outm, smm = mut
    return (sm["iterations"] != smm["iterations"] or sm["termination"] != smm["termination"] or not np.array_equal(out, outm)
            or np.abs(T - Tm).max() > 1e-3)


@pytest.mark.parametrize("m", R.MUTANTS)
def test_device_agrees_with_no_mutant(gpu_ctx, m):
    for name in ("mlid0", "f4", "outliers"):
        w, _, _ = reference(name)
        dev = device(gpu_ctx, w)
        if _mutant_differs(w, dev, R.solve(w, mutants=(m,))):
            return
    pytest.fail(f"the device agrees with mutant {m}")


def _pack(worlds):
    """The worlds back to back as torch device tensors + the host descriptors."""
    import torch
    dev = torch.device("cuda:0")
    probs = (capi.LocalBaProblem * len(worlds))()
    ko = po = oo = 0
    for j, w in enumerate(worlds):
        probs[j] = capi.LocalBaProblem(len(w.T), len(w.points), len(w.obs_kf), 0, ko, po, oo)
        ko += len(w.T); po += len(w.points); oo += len(w.obs_kf)
    cat = lambda xs, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs), dt)).to(dev)
    a = dict(T=cat([w.T.reshape(-1) for w in worlds], np.float64), kc=cat([w.constant for w in worlds], np.uint8),
             X=cat([w.points.reshape(-1) for w in worlds], np.float64), okf=cat([w.obs_kf for w in worlds], np.int32),
             opt=cat([w.obs_pt for w in worlds], np.int32), b=cat([w.bearing.reshape(-1) for w in worlds], np.float64),
             lev=cat([w.level for w in worlds], np.int32))
    a["out"] = torch.full((max(oo, 1),), 7, dtype=torch.uint8, device=dev)
    a["sm"] = torch.full((len(worlds) * capi.LBA_SUMMARY_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device=dev)
    return probs, a


def _batch(ctx, probs, a, delta, n=None, max_iterations=10):
    import torch
    f = ctx.lib.dsdtm_local_ba_batch_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 7 + [C.POINTER(capi.LocalBaParams), C.c_void_p, C.c_void_p, C.c_void_p]
    prm = capi.LocalBaParams(max_iterations, 0, delta)
    s = torch.cuda.current_stream()
    st = f(ctx.handle, len(probs) if n is None else n, C.cast(probs, C.c_void_p), a["T"].data_ptr(), a["kc"].data_ptr(),
           a["X"].data_ptr(), a["okf"].data_ptr(), a["opt"].data_ptr(), a["b"].data_ptr(), a["lev"].data_ptr(), C.byref(prm),
           a["out"].data_ptr(), a["sm"].data_ptr(), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return st


def _summaries(a, n):
    return np.frombuffer(a["sm"].cpu().numpy().tobytes(), capi.LBA_SUMMARY_DTYPE)[:n]


def test_batch_of_mixed_sizes_equals_the_single_calls_bit_for_bit(gpu_ctx):
    names = ["f1", "f4", "once", "f10", "mlid0", "far", "f4_nofixed", "outliers"]
    worlds = [reference(n)[0] for n in names]
    delta = worlds[0].delta
    assert all(w.delta == delta for w in worlds)
    probs, a = _pack(worlds)
    assert _batch(gpu_ctx, probs, a, delta) == capi.OK
    sms = _summaries(a, len(worlds))
    T, X, out = a["T"].cpu().numpy(), a["X"].cpu().numpy(), a["out"].cpu().numpy()
    ko = po = oo = 0
    for j, w in enumerate(worlds):
        Ts, Xs, outs, sm = device(gpu_ctx, w)
        K, P, N = len(w.T), len(w.points), len(w.obs_kf)
        assert np.array_equal(T[12 * ko:12 * (ko + K)], Ts.reshape(-1)), names[j]
        assert np.array_equal(X[3 * po:3 * (po + P)], Xs.reshape(-1)), names[j]
        assert np.array_equal(out[oo:oo + N], outs), names[j]
        for k in capi.LBA_SUMMARY_DTYPE.names:
            assert sms[j][k] == sm[k], (names[j], k)
        ko += K; po += P; oo += N


def test_two_launches_are_bit_identical(gpu_ctx):
    w, _, _ = reference("f10")
    a, b = device(gpu_ctx, w), device(gpu_ctx, w)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3]


def _host_call(ctx, w, T=None, kc=None, okf=None, opt=None, lev=None):
    T = (w.T.reshape(-1).copy() if T is None else T)
    X = w.points.reshape(-1).copy()
    out0 = np.full(len(w.obs_kf), 9, np.uint8)
    args = (T, w.constant if kc is None else kc, X, w.obs_kf if okf is None else okf, w.obs_pt if opt is None else opt,
            w.bearing, w.level if lev is None else lev)
    T0, X0 = T.copy(), X.copy()
    with pytest.raises(capi.DsdtmError) as e:
        local_bundle_adjustment(ctx, *args, w.delta)
    assert e.value.status == capi.ERR_INVALID
    assert np.array_equal(T, T0) and np.array_equal(X, X0) and (out0 == 9).all()
    return str(e.value)


def test_argument_checks_write_nothing(gpu_ctx):
    w = R.make_world(30, n_free=4, n_fixed=4, n_points=100)
    msg = _host_call(gpu_ctx, w, kc=np.ones(len(w.T), np.uint8))
    assert "free" in msg
    okf = w.obs_kf.astype(np.int32).copy(); okf[5] = len(w.T)
    assert "keyframe index" in _host_call(gpu_ctx, w, okf=okf)
    opt = w.obs_pt.astype(np.int32).copy(); opt[-1] = len(w.points)
    assert "point index" in _host_call(gpu_ctx, w, opt=opt)
    lev = w.level.astype(np.int32).copy(); lev[3] = capi.MAX_LEVELS
    assert "level" in _host_call(gpu_ctx, w, lev=lev)
    big = R.make_world(31, n_free=17, n_fixed=2, n_points=60)
    assert "free keyframes over the limit of 16" in _host_call(gpu_ctx, big)
    many = R.make_world(32, n_free=2, n_fixed=65, n_points=60)
    assert "constant keyframes over the limit of 64" in _host_call(gpu_ctx, many)


def test_batch_checks_are_all_or_nothing(gpu_ctx):
    import torch
    worlds = [reference("f1")[0], reference("f4")[0]]
    probs, a = _pack(worlds)
    assert _batch(gpu_ctx, probs, a, worlds[0].delta, n=0) == capi.OK          # n_problems == 0: nothing happens
    probs[1].n_points = capi.LBA_MAX_POINTS + 1                                  # over the limit: nothing enqueued
    T0, X0 = a["T"].clone(), a["X"].clone()
    assert _batch(gpu_ctx, probs, a, worlds[0].delta) == capi.ERR_INVALID
    assert torch.equal(a["T"], T0) and torch.equal(a["X"], X0)
    assert (a["out"] == 7).all() and (a["sm"] == 0x5A).all()
    # what lives in device memory (indices, levels, order, constant flags) is checked by a kernel before the solve is enqueued:
    # one bad problem and the call fails with every problem unwritten
    K0, N0 = len(worlds[0].T), len(worlds[0].obs_kf)
    breakers = {
        "keyframe index": lambda a: a["okf"].__setitem__(N0 + 2, 1000),
        "point index": lambda a: a["opt"].__setitem__(N0 + 5, -1),
        "level": lambda a: a["lev"].__setitem__(N0 + 1, capi.MAX_LEVELS),
        "point index decreases": lambda a: a["opt"].__setitem__(N0 + 7, 0),
        "no free keyframe": lambda a: a["kc"][K0:].fill_(1),
    }
    for reason, brk in breakers.items():
        probs, a = _pack(worlds)
        brk(a)
        T0, X0 = a["T"].clone(), a["X"].clone()
        assert _batch(gpu_ctx, probs, a, worlds[0].delta) == capi.ERR_INVALID, reason
        assert reason in gpu_ctx.lib.dsdtm_last_error(gpu_ctx.handle).decode(), reason
        assert torch.equal(a["T"], T0) and torch.equal(a["X"], X0), reason
        assert (a["out"] == 7).all() and (a["sm"] == 0x5A).all(), reason
    # and a valid batch after a refused one runs
    probs, a = _pack(worlds)
    assert _batch(gpu_ctx, probs, a, worlds[0].delta) == capi.OK
    assert (_summaries(a, 2)["n_residual_blocks"] == [len(w.obs_kf) for w in worlds]).all()


def test_local_ba_beside_a_tracked_frame_on_two_threads(gpu_ctx):
    """The LocalMapping / Tracking split: dsdtm_local_ba on context B while dsdtm_track_frame runs on context A."""
    from dsdtm_amd import tracking
    from tests.test_track_frames_gpu import ALIGN, _last_with, _set_config
    from tests.test_search_gpu import make_world
    _set_config()
    cam, kfs, cur, mps = make_world(500, n_points=900)
    last = _last_with(kfs[0], cam, 300)

    def track(ctx):
        g = tracking.track_frame(ctx, cam, cur.mvImg_Pyr[0], 5, last, last.Get_Pose(), ALIGN, 20, kfs, mps)
        r = (g["T_opt"].copy(), g["matches"].copy())
        g["frame"].close()
        return r

    w, _, _ = reference("f10")
    solo_t = track(gpu_ctx)
    solo_b = device(gpu_ctx, w)
    A, B = capi.Context(0), capi.Context(0)
    res = {}

    def run_t():
        res["t"] = [track(A) for _ in range(4)]

    def run_b():
        res["b"] = [device(B, w) for _ in range(4)]

    th = [threading.Thread(target=run_t), threading.Thread(target=run_b)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for T, m in res["t"]:
        assert np.array_equal(T, solo_t[0]) and np.array_equal(m, solo_t[1])
    for b in res["b"]:
        for x, y in zip(b[:3], solo_b[:3]):
            assert np.array_equal(x, y)
        assert b[3] == solo_b[3]
    A.close(); B.close()


def test_optimizer_local_bundle_adjustment_end_to_end(gpu_ctx):
    from tests.test_local_ba_cpu import object_map
    tKF, kfs, mps, w = object_map(seed=40)
    sm = Optimizer.LocalBundleAdjustment(tKF, None, ctx=gpu_ctx)
    assert sm["n_residual_blocks"] == len(w.obs_kf) and sm["termination"] in (0, 1, 2, 3)
    Tr, Xr, outr, smr = R.solve(w)
    assert sm["iterations"] == smr["iterations"] and sm["n_outliers"] == smr["n_outliers"]
    for k, kf in enumerate(kfs):
        assert np.abs(kf.Get_Pose() - Tr[k]).max() <= 1e-6   # residual order of the object graph differs
    for q, mp in enumerate(mps):
        assert np.abs(mp.Get_Pose() - Xr[q]).max() <= TOL_ONCE
