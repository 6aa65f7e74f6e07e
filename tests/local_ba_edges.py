"""The edge worlds of dsdtm_local_ba (tests/test_local_ba_cpu.py checks the restatement on them, tests/test_local_ba_edges_gpu.py
the device): one world per exit of the trust-region loop that finite, small inputs reach, and one per edge of the problem's
structure (blocks without residuals, no pose block, the largest and the densest problems, every pyramid level). Test
infrastructure only; built from tests/local_ba_restatement.py, no code shared with the kernel."""
import numpy as np

from tests import local_ba_restatement as R

SMALL = dict(n_free=3, n_fixed=3, n_points=60)
EXACT = dict(noise_px=0, outlier_frac=0, pose_noise=(0, 0), point_noise=0)


def _gradient():
    # seed 55, not 51: in a world without noise the residuals are the rounding of their own subtraction, and on seed 51 that
    # rounding can move gmax (8.4e-11) across 1e-10 (exits_decidable of tests/test_local_ba_gpu.py): an undecided world is
    # replaced by another seed. Here gmax = 1.1e-11 and the rounding moves it by 5e-12.
    return R.make_world(55, **SMALL, **EXACT)


def _parameter_no_step():
    w = _gradient()
    w.points[5] += 1e-7
    return w


def _parameter_and_function():
    """A world with pixel noise started a hair from its minimum, where BOTH the parameter and the function tolerance hold in
    the first iteration while the gradient is still far above its own (the order of the two tests decides the termination).
    The start: the restatement run to GRADIENT_TOLERANCE with the two other tolerances off (212 iterations; every point is
    seen at least twice and none is an outlier, so the minimum is sharp), then one point moved by 1e-7: the step back is
    1.4e-7 against a bound of 3.7e-7, the cost change 5.5e-12 against 5.0e-11, gmax 5.8e-7 against 1e-10. The 1e-7 is eight
    digits above what the rounding of the polish can differ by from one LAPACK to another."""
    w = R.make_world(56, n_free=2, n_fixed=4, n_points=40, once_frac=0, outlier_frac=0)
    T, X, _, sm = R.solve(w, max_iterations=300, function_tolerance=0.0, parameter_tolerance=0.0)
    assert sm["termination"] == R.GRADIENT_TOL, sm
    w.T, w.points = T.copy(), X.copy()
    w.points[5] += 1e-7
    return w


def _no_residuals():
    w = R.make_world(50, **SMALL)
    return R.keep_observations(w, np.zeros(len(w.obs_kf), bool))


def _evaluation_failed():
    w = R.make_world(54, **SMALL)
    w.bearing[7] = (1.0, 0.0, 0.0)
    return w


# name -> (builder, max_iterations, termination, iterations, successful steps): the exits, as the restatement ends them
EXITS = {
    "gradient": (_gradient, 10, R.GRADIENT_TOL, 0, 0),
    "parameter_no_step": (_parameter_no_step, 10, R.PARAMETER_TOL, 1, 0),
    "parameter_and_function": (_parameter_and_function, 10, R.PARAMETER_TOL, 1, 0),
    "parameter_long": (lambda: R.make_world(52, n_free=2, n_fixed=2, n_points=20, noise_px=0, outlier_frac=0), 100,
                       R.PARAMETER_TOL, 66, 65),
    # seed 109, not 50: on seed 50 (142 iterations) the restatement's own two forms end at different iteration counts and
    # differ by 5e-6 in the points, so its counts are decided by rounding; here they agree to 3e-15 and ten steps are rejected
    "function_long": (lambda: R.make_world(109, **SMALL), 300, R.FUNCTION_TOL, 38, 28),
    "cap0": (lambda: R.make_world(50, **SMALL), 0, R.MAX_ITER, 0, 0),
    "cap1": (lambda: R.make_world(50, **SMALL), 1, R.MAX_ITER, 1, 1),
    "no_residuals": (_no_residuals, 10, R.NO_RESIDUALS, 0, 0),
    "evaluation_failed": (_evaluation_failed, 10, R.EVAL_FAILED, 0, 0),
}

# ---- structure: 4 free + 4 fixed keyframes, 120 points, the default cap of 10 iterations, unless the name says otherwise
BASE = dict(n_free=4, n_fixed=4, n_points=120)
UNOBSERVED_POINTS = (0, 1, 57, 58, 119)            # the front, the middle and the end of the point array
UNOBSERVED_KF = 2


def _base(seed):
    return R.make_world(seed, **BASE)


def _unobserved_points():
    w = _base(60)
    return R.keep_observations(w, ~np.isin(w.obs_pt, UNOBSERVED_POINTS))


def _unobserved_keyframe():
    w = _base(61)
    return R.keep_observations(w, w.obs_kf != UNOBSERVED_KF)


def _no_pose_block():
    w = _base(62)
    return R.keep_observations(w, w.constant[w.obs_kf])


def _one_observation():
    w = _base(63)
    # observation 2, the second one of a free keyframe: with the first, the solve ends after 3 iterations on gmax = 1.18e-10
    # against 1e-10, a near tie; with this one the 9 free parameters of 2 residuals run to the cap
    i = np.nonzero(~w.constant[w.obs_kf])[0][1]
    assert i == 2
    return R.keep_observations(w, [i])


def all_levels(clip=None):
    """The 120-point world with the levels cycling through 0..7 (clip: the same world with the levels cut at `clip`)."""
    w = _base(64)
    lev = np.arange(len(w.obs_kf)) % 8
    return R.keep_observations(w, np.ones(len(lev), bool), levels=lev if clip is None else np.minimum(lev, clip))


STRUCTURE = {
    "unobserved_points": _unobserved_points,
    "unobserved_keyframe": _unobserved_keyframe,
    "no_pose_block": _no_pose_block,
    "one_observation": _one_observation,
    "free11": lambda: R.make_world(65, n_free=11, n_fixed=4, n_points=120),                 # n = 66: the first size with y1
    "kf80": lambda: R.make_world(66, n_free=16, n_fixed=64, n_points=120),                  # K = 80: the keyframe limit
    # seed 81, not 67: on seed 67 the restatement's own two forms differ by 1e-8 / 3e-8 (poses / points), above TOL_DEFAULT;
    # here by 5e-14 / 9e-14
    "dense_pairs": lambda: R.make_world(81, n_free=16, n_fixed=4, n_points=40, all_free=True),
    "all_levels": all_levels,
}

MAX_ITERATIONS = {name: e[1] for name, e in EXITS.items()}
_CACHE = {}


def world(name):
    return (EXITS[name][0] if name in EXITS else STRUCTURE[name])()


def reference(name):
    """(world, solve(world) in the Schur form, its trace), computed once and shared; nobody writes to it."""
    if name not in _CACHE:
        w = world(name)
        tr = []
        with np.errstate(all="ignore"):                      # the non-finite evaluation of "evaluation_failed" is the point
            ref = R.solve(w, max_iterations=MAX_ITERATIONS.get(name, 10), trace=tr)
        _CACHE[name] = (w, ref, tr)
    return _CACHE[name]
