"""The local-BA checker checked (tests/local_ba_restatement.py): its Schur form and its dense normal-equations form agree on
small worlds, every mutant changes a named output on a committed world seed, and the Python host mirror of
Optimizer::LocalBundleAdjustment (set construction, write-back, outlier bookkeeping with its quirk) behaves as the reference
with the solve stubbed. No GPU."""
import numpy as np
import pytest

from dsdtm_amd import mapping
from dsdtm_amd.optimizer import Optimizer
from tests import local_ba_restatement as R


@pytest.mark.parametrize("seed,kw", [(1, dict(n_free=2, n_fixed=2, n_points=30)),
                                     (2, dict(n_free=3, n_fixed=3, n_points=40, zero_id=0)),
                                     (3, dict(n_free=3, n_fixed=1, n_points=40, outlier_frac=0.3)),
                                     (4, dict(n_free=2, n_fixed=2, n_points=30, pose_noise=(0.08, 0.3), point_noise=0.4))])
def test_schur_and_dense_forms_agree(seed, kw):
    w = R.make_world(seed, **kw)
    ta, tb = [], []
    Ta, Xa, oa, sa = R.solve(w, form="schur", trace=ta)
    Tb, Xb, ob, sb = R.solve(w, form="dense", trace=tb)
    for k in ("iterations", "successful_steps", "termination", "n_residual_blocks", "n_outliers"):
        assert sa[k] == sb[k], k
    assert [t[0] for t in ta] == [t[0] for t in tb]                       # the same accept / reject sequence
    assert [t[2] > 1e-3 for t in ta if t[0] == "ratio"] == [t[2] > 1e-3 for t in tb if t[0] == "ratio"]
    assert np.array_equal(oa, ob)
    once = np.bincount(w.obs_pt, minlength=len(w.points)) == 1
    assert np.abs(Ta - Tb).max() <= 1e-9
    assert np.abs(Xa - Xb)[~once].max() <= 1e-6                         # point depths: DESIGN.md §3.7
    if "pose_noise" in kw:
        assert sa["successful_steps"] < sa["iterations"]                  # the far start rejects a step


# mutant -> (world seed, the output it changes on that world)
MUTANT_WORLDS = {
    "L1": (21, "pose"), "L2": (21, "pose"), "L3": (21, "outliers"), "L4": (21, "outliers"),
    "L5": (22, "pose"), "L6": (21, "iterations"), "L7": (21, "pose"),
}


def _mutant_world(seed):
    return R.make_world(seed, n_free=3, n_fixed=3, n_points=60, zero_id=0 if seed == 22 else None)


@pytest.mark.parametrize("m", R.MUTANTS)
def test_every_mutant_changes_a_named_output(m):
    seed, what = MUTANT_WORLDS[m]
    w = _mutant_world(seed)
    T, X, out, sm = R.solve(w)
    Tm, Xm, outm, smm = R.solve(w, mutants=(m,))
    if what == "pose":
        assert np.abs(T - Tm).max() > 1e-6
    elif what == "outliers":
        assert not np.array_equal(out, outm)
    else:
        assert sm["iterations"] != smm["iterations"]


def object_map(seed=40, **kw):
    """A world as KeyFrame / MapPoint objects: keyframe 0 is the new keyframe, the other free ones its covisible keyframes,
    the fixed ones observe local points only. Returns (tKFrame, keyframes, map points, the world)."""
    kw = dict(dict(n_free=3, n_fixed=2, n_points=60), **kw)
    w = R.make_world(seed, **kw)
    cam = mapping.Camera(500.0)
    feats = [[] for _ in w.T]
    for i, (k, q) in enumerate(zip(w.obs_kf, w.obs_pt)):
        feats[k].append(i)
    kfs = [mapping.KeyFrame(w.kf_id[k], w.T[k], [mapping.Feature(w.bearing[i], w.level[i]) for i in feats[k]], cam)
           for k in range(len(w.T))]
    mps = [mapping.MapPoint(q + 100, w.points[q]) for q in range(len(w.points))]
    slot = {}
    for k in range(len(w.T)):
        for j, i in enumerate(feats[k]):
            slot[i] = j
    for i, (k, q) in enumerate(zip(w.obs_kf, w.obs_pt)):     # observations in residual order: the map's order
        mps[q].Add_Observation(kfs[k], slot[i])
        kfs[k].Add_MapPoint(mps[q], slot[i])
    n_free = int((~w.fixed).sum())
    kfs[0].mOrderedCovGraph = [(10, kfs[k]) for k in range(1, n_free)]
    return kfs[0], kfs, mps, w


def test_host_mirror_builds_the_reference_problem():
    tKF, kfs, mps, w = object_map(seed=41, zero_id=1)
    seen = {}

    def stub(T, kc, X, okf, opt, b, lev, delta):
        seen.update(T=T.copy(), kc=kc.copy(), X=X.copy(), okf=okf.copy(), opt=opt.copy(), delta=delta)
        return np.zeros(len(okf), np.uint8), dict(n_outliers=0)
    Optimizer.LocalBundleAdjustment(tKF, None, solve=stub)
    assert seen["delta"] == float(np.float32(2.0)) / float(np.float32(500.0))
    assert len(seen["okf"]) == len(w.obs_kf)
    kc = seen["kc"].astype(bool)
    n_free = int((~w.fixed).sum())
    assert not kc[0] and kc[1]                                # local keyframe with mlId == 0 is constant
    assert kc[n_free:].all()                                 # the fixed keyframes
    assert (np.diff(seen["opt"]) >= 0).all()                 # residual-block order: point by point


def test_host_mirror_outlier_bookkeeping_keeps_the_match():
    """Erase_Observation runs before Erase_MapPointMatch, so the keyframe keeps the point in mvMapPoints; a point left with
    <= 1 observation is bad. The solve is stubbed: observation 0 (point A, kf 0) and both of point B's are outliers."""
    cam = mapping.Camera(500.0)
    f = lambda: mapping.Feature([0.0, 0.0, 1.0], 0)
    k0 = mapping.KeyFrame(1, np.eye(3, 4), [f(), f()], cam)
    k1 = mapping.KeyFrame(2, np.eye(3, 4), [f(), f()], cam)
    k2 = mapping.KeyFrame(3, np.eye(3, 4), [f()], cam)
    A, B = mapping.MapPoint(10, [0, 0, 5]), mapping.MapPoint(11, [1, 0, 5])
    for kf, mp, j in ((k0, A, 0), (k1, A, 0), (k2, A, 0), (k0, B, 1), (k1, B, 1)):
        mp.Add_Observation(kf, j)
        kf.Add_MapPoint(mp, j)
    k0.mOrderedCovGraph = [(5, k1)]

    def stub(T, kc, X, okf, opt, b, lev, delta):
        assert list(opt) == [0, 0, 0, 1, 1] and list(kc) == [0, 0, 1]
        T.reshape(-1, 3, 4)[:, 0, 3] += 1.0                  # a visible write-back
        X.reshape(-1, 3)[:, 1] += 2.0
        return np.array([1, 0, 0, 1, 1], np.uint8), dict(n_outliers=3)
    Optimizer.LocalBundleAdjustment(k0, None, solve=stub)
    assert k0 not in A.Get_Observations() and A.mObsNum == 2 and not A.IsBad()
    assert k0.mvMapPoints[0] is A                            # the quirk: the match is NOT cleared
    assert B.Get_Observations() == {} and B.IsBad()          # <= 1 observation left: bad
    assert k0.mvMapPoints[1] is B and k1.mvMapPoints[1] is B
    assert k2.Get_Pose()[0, 3] == 1.0 and A.Get_Pose()[1] == 2.0   # every keyframe, fixed ones included, and every point
