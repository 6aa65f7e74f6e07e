"""Independent numpy restatement of Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:103-282), the solve and the
outlier pass, used to check dsdtm_local_ba. Test infrastructure only: it shares no code with the kernel
(rotations through scipy's Rotation, 3x3 inverses and the reduced solve through LAPACK).

Two forms of the same minimiser (Ceres 1.13 TrustRegionMinimizer + LevenbergMarquardtStrategy):
  form="schur": the step the kernel computes — points eliminated per 3x3 block (D^2 added first), the reduced
                camera matrix solved by Cholesky, the points recovered by back-substitution;
  form="dense": the full (J^T J + D^2) system of every free parameter solved at once (small worlds only).
Both take the model decrease from J * step. Mutant flags each "fix" one quirk of the reference:
  L1  Jacobians divided by 1 << level            L2  CauchyLoss(1.0) (the commented-out :164) instead of Huber(delta)
  L3  outlier threshold delta instead of delta^2  L4  outlier error divided by (1 << level)^2 (the residual's scale)
  L5  the keyframe with mlId == 0 left free       L6  max_num_iterations = 100
  L7  PoseLocalParameterization::Plus as a vector sum
"""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation

MUTANTS = ("L1", "L2", "L3", "L4", "L5", "L6", "L7")
# dsdtm_pose_opt_termination
FUNCTION_TOL, PARAMETER_TOL, GRADIENT_TOL, MAX_ITER, MIN_RADIUS, INVALID_STEPS, NO_RESIDUALS, EVAL_FAILED = range(8)


def x_of_T(T):
    T = np.asarray(T, np.float64).reshape(3, 4)
    return np.concatenate([T[:, 3], Rotation.from_matrix(T[:, :3]).as_rotvec()])


def T_of_x(x):
    return np.concatenate([Rotation.from_rotvec(x[3:]).as_matrix(), x[:3, None]], 1)


def plus(x, d, mutants=()):
    """PoseLocalParameterization::Plus (include/Optimizer.h:222-236): SE3(exp(d)) * SE3(exp(x))."""
    if "L7" in mutants:
        return x + d
    Ro, Rd = Rotation.from_rotvec(x[3:]).as_matrix(), Rotation.from_rotvec(d[3:]).as_matrix()
    return np.concatenate([Rd @ x[:3] + d[:3], Rotation.from_matrix(Rd @ Ro).as_rotvec()])


def loss(s, delta, mutants=()):
    """rho(s), rho'(s) of ceres::HuberLoss(delta) (or CauchyLoss(1) under L2); rho'' <= 0 for both."""
    if "L2" in mutants:
        return np.log1p(s), np.maximum(1.0 / (1.0 + s), np.finfo(float).tiny)
    b = delta * delta
    r = np.sqrt(s)
    out = s > b
    rho = np.where(out, 2.0 * delta * r - b, s)
    rho1 = np.where(out, np.maximum(np.finfo(float).tiny, delta / np.where(out, r, 1.0)), 1.0)
    return rho, rho1


class Problem:
    """The host arrays of one dsdtm_local_ba call."""

    def __init__(self, T, constant, points, obs_kf, obs_pt, bearing, level, delta):
        self.T = np.asarray(T, np.float64).reshape(-1, 3, 4)
        self.constant = np.asarray(constant, bool)
        self.points = np.asarray(points, np.float64).reshape(-1, 3)
        self.obs_kf = np.asarray(obs_kf, np.int64)
        self.obs_pt = np.asarray(obs_pt, np.int64)
        self.bearing = np.asarray(bearing, np.float64).reshape(-1, 3)
        self.level = np.asarray(level, np.int64)
        self.delta = float(delta)


def _evaluate(xk, xp, P, mutants, jac=True):
    """FullBA_Problem::Evaluate of every residual block (include/Optimizer.h:139-197) + the Huber corrector."""
    R = Rotation.from_rotvec(xk[:, 3:]).as_matrix()          # (K, 3, 3)
    k, p = P.obs_kf, P.obs_pt
    pc = np.einsum("nij,nj->ni", R[k], xp[p]) + xk[k, :3]
    inv = (1 << P.level).astype(np.float64)
    obs = P.bearing[:, :2] / P.bearing[:, 2:3]
    r = (obs - pc[:, :2] / pc[:, 2:3]) / inv[:, None]
    s = (r * r).sum(1)
    rho, rho1 = loss(s, P.delta, mutants)
    cost = 0.5 * rho.sum()
    if not jac:
        return cost
    x, y, zi = pc[:, 0], pc[:, 1], 1.0 / pc[:, 2]
    zi2 = zi * zi
    Jc = np.zeros((len(k), 2, 6))
    Jc[:, 0, 0] = -zi
    Jc[:, 0, 2] = x * zi2
    Jc[:, 0, 3] = y * Jc[:, 0, 2]
    Jc[:, 0, 4] = -(1.0 + x * Jc[:, 0, 2])
    Jc[:, 0, 5] = y * zi
    Jc[:, 1, 1] = -zi
    Jc[:, 1, 2] = y * zi2
    Jc[:, 1, 3] = 1.0 + y * Jc[:, 1, 2]
    Jc[:, 1, 4] = -x * Jc[:, 1, 2]
    Jc[:, 1, 5] = -x * zi
    M = np.zeros((len(k), 2, 3))
    M[:, 0, 0] = zi
    M[:, 0, 2] = -x * zi2
    M[:, 1, 1] = zi
    M[:, 1, 2] = -y * zi2
    Jp = -np.einsum("nij,njk->nik", M, R[k])
    if "L1" in mutants:
        Jc = Jc / inv[:, None, None]
        Jp = Jp / inv[:, None, None]
    w = np.sqrt(rho1)
    return cost, r * w[:, None], Jc * w[:, None, None], Jp * w[:, None, None]


def _reduce(idx, vals, n):
    out = np.zeros((n,) + vals.shape[1:])
    np.add.at(out, idx, vals)
    return out


def solve(P: Problem, max_iterations=10, form="schur", mutants=(), trace=None, function_tolerance=1e-6,
          parameter_tolerance=1e-8):
    """Returns (T (K,3,4), points (P,3), outlier (N,) u8, summary dict). L5 needs a World (its `fixed` flags).
    `trace` (a list) receives, in order of execution: ("step", it, radius, model_change), ("ratio", it, rho, cost,
    model_change), and one record per tolerance test, each with the quantity and the bound it was compared with and the
    number of steps accepted before it:
      ("gradient", it, gmax, 1e-10, accepted, ground, sens_pose, sens_point)  ground = max_i sum_o |J_oi| rho_o with
          rho_o = 2^-50 (|observed| + |projected|) / 2^level, what the rounding of a residual's own subtraction moves a
          gradient component by; sens_* = max_i sum_o |J_oi| sum_j |J_oj| over the pose / point columns j: a deviation
          of d_pose / d_point per parameter moves no gradient component by more than d_pose sens_pose + d_point sens_point
      ("parameter", it, step_norm, 1e-8 (x_norm + 1e-8), accepted)
      ("function", it, |cost change|, 1e-6 cost, accepted, cost)
    function_tolerance / parameter_tolerance: Ceres' defaults, which the reference leaves alone; the tests set one to 0 to
    polish a start, or to ask what the OTHER test would have said at the iteration the first one ended."""
    mutants = tuple(mutants)
    if "L6" in mutants:
        max_iterations = 100
    const = P.constant.copy()
    if "L5" in mutants and hasattr(P, "fixed"):
        const = np.asarray(P.fixed, bool).copy()            # only the keyframes outside the window stay constant
    K, NP, N = len(P.T), len(P.points), len(P.obs_kf)
    xk = np.stack([x_of_T(T) for T in P.T]) if K else np.zeros((0, 6))
    xp = P.points.copy()
    # the reduced program: constant blocks and blocks without residuals are removed
    seen_k = np.bincount(P.obs_kf, minlength=K) > 0
    seen_p = np.bincount(P.obs_pt, minlength=NP) > 0
    free_k = np.nonzero(~const & seen_k)[0]
    free_p = np.nonzero(seen_p)[0]
    F, Q = len(free_k), len(free_p)
    col_k = -np.ones(K, np.int64); col_k[free_k] = np.arange(F)
    col_p = -np.ones(NP, np.int64); col_p[free_p] = np.arange(Q)
    ok_k = col_k[P.obs_kf] >= 0                                # the observation's keyframe is free
    summ = dict(iterations=0, successful_steps=0, termination=NO_RESIDUALS, n_residual_blocks=N,
                initial_cost=0.0, final_cost=0.0)

    def flat(xk_, xp_):
        return np.concatenate([xk_[free_k].reshape(-1), xp_[free_p].reshape(-1)])

    def ev(xk_, xp_):
        cost, r, Jc, Jp = _evaluate(xk_, xp_, P, mutants)
        Jc = Jc * ok_k[:, None, None]
        return cost, r, Jc, Jp

    def gradient(r, Jc, Jp):
        gk = _reduce(col_k[P.obs_kf][ok_k], np.einsum("nij,ni->nj", Jc[ok_k], r[ok_k]), F)
        gp = _reduce(col_p[P.obs_pt], np.einsum("nij,ni->nj", Jp, r), Q)
        return gk, gp

    def trace_gradient(it, gmax, succ, xk_, xp_, Jc, Jp):
        aJc, aJp = np.abs(Jc), np.abs(Jp)
        Rm = Rotation.from_rotvec(xk_[:, 3:]).as_matrix()
        pc = np.einsum("nij,nj->ni", Rm[P.obs_kf], xp_[P.obs_pt]) + xk_[P.obs_kf, :3]
        rho = 2.0 ** -50 * (np.abs(P.bearing[:, :2] / P.bearing[:, 2:3]) + np.abs(pc[:, :2] / pc[:, 2:3]))
        rho = rho / (1 << P.level).astype(np.float64)[:, None]
        ck, cp = col_k[P.obs_kf][ok_k], col_p[P.obs_pt]

        def worst(row_weight):                                   # max over the columns i of sum_o |J_oi| . weight_o
            a = _reduce(ck, np.einsum("nij,ni->nj", aJc[ok_k], row_weight[ok_k]), F)
            b = _reduce(cp, np.einsum("nij,ni->nj", aJp, row_weight), Q)
            return max(a.max(initial=0.0), b.max(initial=0.0))
        trace.append(("gradient", it, gmax, 1e-10, succ, worst(rho), worst(aJc.sum(2)), worst(aJp.sum(2))))

    def gmax_of(xk_, xp_, gk, gp):
        m = 0.0
        for a in range(F):
            x = xk_[free_k[a]]
            m = max(m, np.abs(x - plus(x, -gk[a], mutants)).max())
        if Q:
            x = xp_[free_p]
            m = max(m, np.abs(x - (x + -gp)).max())
        return m

    if N:
        cost, r, Jc, Jp = ev(xk, xp)
        if not (np.isfinite(cost) and np.isfinite(r).all() and np.isfinite(Jc).all() and np.isfinite(Jp).all()):
            summ["termination"] = EVAL_FAILED
        else:
            summ["initial_cost"] = cost
            dk = _reduce(col_k[P.obs_kf][ok_k], (Jc[ok_k] ** 2).sum(1), F)
            dp = _reduce(col_p[P.obs_pt], (Jp ** 2).sum(1), Q)
            sk, sp = 1.0 / (1.0 + np.sqrt(dk)), 1.0 / (1.0 + np.sqrt(dp))    # Jacobi scaling, fixed at iteration 0
            gk, gp = gradient(r, Jc, Jp)
            gmax = gmax_of(xk, xp, gk, gp)
            x_norm = np.linalg.norm(flat(xk, xp))
            radius, dec, reuse, invalid, it, succ = 1e4, 2.0, False, 0, 0, 0
            diag = None
            while True:
                if it >= max_iterations:
                    term = MAX_ITER; break
                if trace is not None:
                    trace_gradient(it, gmax, succ, xk, xp, Jc, Jp)
                if gmax <= 1e-10:
                    term = GRADIENT_TOL; break
                if radius <= 1e-32:
                    term = MIN_RADIUS; break
                it += 1
                # (no free keyframe observed: F == 0, Jc is all zero and there is no pose scale to gather)
                Jcs = Jc * sk[np.maximum(col_k[P.obs_kf], 0)][:, None, :] if F else Jc
                Jps = Jp * sp[col_p[P.obs_pt]][:, None, :]
                if not reuse:
                    diag = (np.clip(_reduce(col_k[P.obs_kf][ok_k], (Jcs[ok_k] ** 2).sum(1), F), 1e-6, 1e32),
                            np.clip(_reduce(col_p[P.obs_pt], (Jps ** 2).sum(1), Q), 1e-6, 1e32))
                Dk2, Dp2 = diag[0] / radius, diag[1] / radius
                yk, yp = _step(P, form, F, Q, col_k, col_p, ok_k, r, Jcs, Jps, Dk2, Dp2)
                reuse = True
                step_k, step_p = -yk, -yp
                valid = np.isfinite(step_k).all() and np.isfinite(step_p).all()
                mr = np.zeros_like(r)
                if valid:
                    mr = (np.einsum("nij,nj->ni", Jcs[ok_k], step_k[col_k[P.obs_kf][ok_k]]) if F else 0) * 1.0
                    full = np.zeros_like(r); full[ok_k] = mr if F else 0.0
                    mr = full + np.einsum("nij,nj->ni", Jps, step_p[col_p[P.obs_pt]])
                model_change = -(mr.reshape(-1) @ (r.reshape(-1) + mr.reshape(-1) / 2.0)) if valid else 0.0
                if trace is not None:
                    trace.append(("step", it, radius, model_change))
                if not (valid and model_change > 0):
                    invalid += 1
                    if invalid >= 5:
                        term = INVALID_STEPS; break
                    radius /= dec; dec *= 2
                    continue
                invalid = 0
                ck, cp = xk.copy(), xp.copy()
                for a in range(F):
                    ck[free_k[a]] = plus(xk[free_k[a]], step_k[a] * sk[a], mutants)
                cp[free_p] = xp[free_p] + step_p * sp
                ccost = _evaluate(ck, cp, P, mutants, jac=False)
                if not np.isfinite(ccost):
                    ccost = np.finfo(float).max
                step_norm = np.linalg.norm(flat(xk, xp) - flat(ck, cp))
                if trace is not None:
                    trace.append(("parameter", it, step_norm, parameter_tolerance * (x_norm + 1e-8), succ))
                if step_norm <= parameter_tolerance * (x_norm + 1e-8):
                    term = PARAMETER_TOL; break
                change = cost - ccost
                if trace is not None:
                    trace.append(("function", it, abs(change), function_tolerance * cost, succ, cost))
                if abs(change) <= function_tolerance * cost:
                    term = FUNCTION_TOL; break
                rho = change / model_change
                if trace is not None:
                    trace.append(("ratio", it, rho, cost, model_change))
                if rho > 1e-3:
                    xk, xp = ck, cp
                    cost, r, Jc, Jp = ev(xk, xp)
                    if not (np.isfinite(r).all() and np.isfinite(Jc).all() and np.isfinite(Jp).all()):
                        succ += 1
                        term = EVAL_FAILED; break                 # Ceres ends the solve: the Jacobian failed at the new point
                    gk, gp = gradient(r, Jc, Jp)
                    gmax = gmax_of(xk, xp, gk, gp)
                    x_norm = np.linalg.norm(flat(xk, xp))
                    succ += 1
                    radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                    dec, reuse = 2.0, False
                else:
                    radius /= dec; dec *= 2; reuse = True
            summ.update(iterations=it, successful_steps=succ, termination=term, final_cost=cost)
    # write-back: Set_Pose(SE3(SO3::exp(x.tail), x.head)) for every keyframe (:236-242), every point (:244-248)
    Tn = np.stack([T_of_x(x) for x in xk]) if K else np.zeros((0, 3, 4))
    # outlier pass (:250-271): squared 2-D error at the new poses, against delta^2
    out = np.zeros(N, np.uint8)
    if N:
        pc = np.einsum("nij,nj->ni", Tn[P.obs_kf, :, :3], xp[P.obs_pt]) + Tn[P.obs_kf, :, 3]
        e = P.bearing[:, :2] / P.bearing[:, 2:3] - pc[:, :2] / pc[:, 2:3]
        err = (e * e).sum(1)
        if "L4" in mutants:
            err = err / (1 << P.level).astype(np.float64) ** 2
        thr = P.delta if "L3" in mutants else P.delta * P.delta
        out = (err > thr).astype(np.uint8)
    summ["n_outliers"] = int(out.sum())
    return Tn, xp, out, summ


def _step(P, form, F, Q, col_k, col_p, ok_k, r, Jc, Jp, Dk2, Dp2):
    """y solving (J^T J + D^2) y = J^T r over the free blocks (the step is -y); NaN when the solve fails."""
    ck, cp = col_k[P.obs_kf], col_p[P.obs_pt]
    if form == "dense":
        n = 6 * F + 3 * Q
        N = len(ck)
        J = np.zeros((2 * N, n))
        for i in range(N):
            if ok_k[i]:
                J[2 * i:2 * i + 2, 6 * ck[i]:6 * ck[i] + 6] = Jc[i]
            J[2 * i:2 * i + 2, 6 * F + 3 * cp[i]:6 * F + 3 * cp[i] + 3] = Jp[i]
        A = J.T @ J + np.diag(np.concatenate([Dk2.reshape(-1), Dp2.reshape(-1)]))
        g = J.T @ r.reshape(-1)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return np.full((F, 6), np.nan), np.full((Q, 3), np.nan)
        y = np.linalg.solve(L.T, np.linalg.solve(L, g))
        return y[:6 * F].reshape(F, 6), y[6 * F:].reshape(Q, 3)
    # Schur: points are the e-blocks, free keyframe poses the f-blocks
    V = _reduce(cp, np.einsum("nji,njk->nik", Jp, Jp), Q) + np.einsum("qi,ij->qij", Dp2, np.eye(3))
    gp = _reduce(cp, np.einsum("nij,ni->nj", Jp, r), Q)
    try:
        Vi = np.linalg.inv(V)
    except np.linalg.LinAlgError:
        return np.full((F, 6), np.nan), np.full((Q, 3), np.nan)
    S = np.zeros((6 * F, 6 * F))
    b = np.zeros(6 * F)
    if F:
        U = _reduce(ck[ok_k], np.einsum("nji,njk->nik", Jc[ok_k], Jc[ok_k]), F)
        gk = _reduce(ck[ok_k], np.einsum("nij,ni->nj", Jc[ok_k], r[ok_k]), F)
        for a in range(F):
            S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = U[a] + np.diag(Dk2[a])
        b = gk.reshape(-1).copy()
        W = np.einsum("nji,njk->nik", Jc, Jp)                          # (N, 6, 3)
        idx = np.nonzero(ok_k)[0]
        by_pt = {}
        for i in idx:
            by_pt.setdefault(cp[i], []).append(i)
        for q, obs in by_pt.items():
            for i in obs:
                Fi = W[i] @ Vi[q]
                a = ck[i]
                b[6 * a:6 * a + 6] -= Fi @ gp[q]
                for j in obs:
                    c = ck[j]
                    S[6 * a:6 * a + 6, 6 * c:6 * c + 6] -= Fi @ W[j].T
    try:
        L = np.linalg.cholesky(S) if F else np.zeros((0, 0))
    except np.linalg.LinAlgError:
        return np.full((F, 6), np.nan), np.full((Q, 3), np.nan)
    yk = np.linalg.solve(L.T, np.linalg.solve(L, b)) if F else np.zeros(0)
    yk = yk.reshape(F, 6)
    rhs = gp.copy()
    if F:
        np.add.at(rhs, cp[ok_k], -np.einsum("nji,nj->ni", np.einsum("nji,njk->nik", Jc[ok_k], Jp[ok_k]), yk[ck[ok_k]]))
    yp = np.einsum("qij,qj->qi", Vi, rhs)
    return yk, yp


# ---- synthetic local-BA worlds -------------------------------------------------------------------------------------
class World(Problem):
    """A LocalMapping window: n_free local keyframes (kf 0 is the new keyframe), n_fixed keyframes outside the window
    that observe local points, points in front of them; bearings with pixel noise at levels 0..4 and planted outliers."""


def make_world(seed, n_free=4, n_fixed=4, n_points=200, f=500.0, noise_px=0.5, outlier_frac=0.05, pose_noise=(0.003, 0.01),
               point_noise=0.02, once_frac=0.05, max_obs=6, zero_id=None, thresh=2.0, all_free=False):
    """all_free: every point is observed by ALL free keyframes (besides the constant ones it drew): the densest pair lists."""
    rng = np.random.default_rng(seed)
    K = n_free + n_fixed
    Tt = np.zeros((K, 3, 4))
    for k in range(K):                               # cameras on an arc, looking at the scene around z = 5
        ang = -0.5 + 1.0 * k / max(K - 1, 1) + rng.normal(0, 0.02)
        c = np.array([3.0 * np.sin(ang), rng.normal(0, 0.1), 5.0 - 3.0 * np.cos(ang)])
        Rwc = Rotation.from_rotvec([rng.normal(0, 0.02), ang, rng.normal(0, 0.02)]).as_matrix()
        R = Rwc.T
        Tt[k, :, :3] = R
        Tt[k, :, 3] = -R @ c
    pts = np.column_stack([rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.8, 1.8, n_points), rng.uniform(4.0, 7.0, n_points)])
    obs_kf, obs_pt, bearing, level = [], [], [], []
    for q in range(n_points):
        if rng.random() < once_frac:
            ks = [int(rng.integers(0, n_free))]
        else:
            m = int(rng.integers(2, min(max_obs, K) + 1))
            ks = [int(rng.integers(0, n_free))] + [int(k) for k in rng.choice(K, m, replace=False)]
            ks = list(dict.fromkeys(ks))
        if all_free:
            ks = list(range(n_free)) + [k for k in ks if k >= n_free]
        rng.shuffle(ks)                              # std::map<KeyFrame*> order: not keyframe order
        for k in ks:
            pc = Tt[k, :, :3] @ pts[q] + Tt[k, :, 3]
            lev = int(rng.choice(5, p=[0.5, 0.2, 0.15, 0.1, 0.05]))
            uv = pc[:2] / pc[2] + rng.normal(0, noise_px / f, 2)
            if rng.random() < outlier_frac:
                uv = uv + rng.choice([-1, 1], 2) * rng.uniform(15, 40, 2) / f
            b = np.array([uv[0], uv[1], 1.0])
            obs_kf.append(k); obs_pt.append(q); bearing.append(b / np.linalg.norm(b)); level.append(lev)
    T0 = Tt.copy()
    for k in range(n_free):                          # the local window starts off its optimum
        dR = Rotation.from_rotvec(rng.normal(0, pose_noise[0], 3)).as_matrix()
        T0[k, :, :3] = dR @ Tt[k, :, :3]
        T0[k, :, 3] = Tt[k, :, 3] + rng.normal(0, pose_noise[1], 3)
    p0 = pts + rng.normal(0, point_noise, pts.shape)
    kf_id = np.arange(K) + 1
    if zero_id is not None:
        kf_id[zero_id] = 0
    fixed = np.arange(K) >= n_free
    const = fixed | (kf_id == 0)
    delta = float(np.float32(thresh)) / float(np.float32(f))
    w = World(T0, const, p0, obs_kf, obs_pt, bearing, level, delta)
    w.fixed, w.kf_id, w.T_true, w.p_true, w.seed = fixed, kf_id, Tt, pts, seed
    return w


def keep_observations(w, keep, levels=None):
    """The world with the observations of the mask / index list `keep` only (keyframes and points stay, so some may lose
    every observation), optionally with other levels. The arrays are copies: the source world is left as it is."""
    keep = np.asarray(keep)
    idx = np.nonzero(keep)[0] if keep.dtype == bool else keep.astype(np.int64)
    lev = w.level if levels is None else np.asarray(levels, np.int64)
    v = World(w.T.copy(), w.constant.copy(), w.points.copy(), w.obs_kf[idx], w.obs_pt[idx], w.bearing[idx], lev[idx], w.delta)
    for k in ("fixed", "kf_id", "T_true", "p_true", "seed"):
        if hasattr(w, k):
            setattr(v, k, getattr(w, k))
    return v
