"""dsdtm_find_homography / dsdtm_find_homographies (libdsdtm_amd_homography.so: csrc/homography.hip, csrc/homography_api.cpp) against the
numpy restatement dsdtm_amd/homography_restatement.py, which tests/test_homography_cpu.py holds to its C twin, to the worlds' truth and
to its mutants. Comparison rule: EVERY output is bit-equal to the restatement's — H, both costs, the mask, n_inliers, best_hypothesis,
rounds, refit_iterations — and a problem with found = 0 leaves its outputs as the caller filled them."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import homography, motion
from dsdtm_amd import motion_restatement as MR
from tests import homography_cases as hc
from tests import motion_cases as mc

pytestmark = pytest.mark.gpu

BATCH = ["H", "s64", "s65", "s257", "s2048", "D", "G"]          # sizes 5, 64, 65, 257, 2048, the collinear world and m = 4


@pytest.fixture(scope="module")
def hctx():
    ctx = homography.HomographyContext(0)
    yield ctx
    ctx.close()


def _report(name, got, want):
    if want["found"] and got["found"]:
        print(f"[homography] {name}: n_inliers {got['n_inliers']} / {want['n_inliers']}, best {got['best_hypothesis']} / {want['best_hypothesis']}, "
              f"rounds {got['rounds']} / {want['rounds']}, refit {got['refit_iterations']} / {want['refit_iterations']}, "
              f"max |dH| {np.abs(got['H'] - want['H']).max():.3e}, costs {got['cost_before']!r} {got['cost_after']!r} / "
              f"{want['cost_before']!r} {want['cost_after']!r}")
    else:
        print(f"[homography] {name}: found {got['found']} / {want['found']}")


@pytest.mark.parametrize("name", hc.NAMES)
def test_world_single_call(hctx, name):
    wd, want = hc.world(name), hc.expected(name)
    got = hctx.find_homography(wd["A"], wd["B"])
    _report(name, got, want)
    assert hc.same(got, want), name


def _untouched(prepared, k):
    raw = bytes(prepared.results[k])
    found = C.sizeof(homography.Result) - 24
    return (all(b == homography.FILL for b in raw[:found] + raw[found + 4:]) and (prepared.masks[k] == homography.FILL).all())


def test_batch_equals_single_calls_and_is_deterministic(hctx):
    probs = [(hc.world(n)["A"], hc.world(n)["B"]) for n in BATCH]
    p = hctx.prepare(probs)
    hctx.check(p.run_raw())
    first = p.answers()
    for k, n in enumerate(BATCH):
        assert hc.same(first[k], hctx.find_homography(*probs[k])) and hc.same(first[k], hc.expected(n)), n
    for k in (5, 6):          # found = 0: the outputs are as the caller filled them
        assert first[k]["found"] == 0 and _untouched(p, k), BATCH[k]
    again = hctx.find_homographies(probs)
    rev = hctx.find_homographies(probs[::-1])[::-1]
    for k, n in enumerate(BATCH):
        assert hc.same(first[k], again[k]) and hc.same(first[k], rev[k]), n


@pytest.mark.parametrize("name,params", [("B", dict(thr=1.0)), ("C", dict(max_hypotheses=256)), ("B", dict(seed=12345)),
                                         ("N", dict(thr=1.0, max_hypotheses=700, seed=9)), ("N", dict(thr=3.0686867580216677)), ("E", dict(seed=1))])
def test_non_default_parameters(hctx, name, params):
    wd, want = hc.world(name), hc.expected(name, **params)
    got = hctx.find_homographies([(wd["A"], wd["B"], params)])[0]
    _report(f"{name} {params}", got, want)
    assert hc.same(got, want), (name, params)
    if "max_hypotheses" in params and want["found"]:
        assert got["rounds"] <= -(-params["max_hypotheses"] // 256)


def test_argument_errors_name_index_and_field(hctx):
    b, h = hc.world("B"), hc.world("H")
    bad = b["A"].copy()
    bad[17, 1] = np.nan
    cases = [([(h["A"], h["B"]), (bad, b["B"])], "problem 1", "points_a is not finite at index 17"),
             ([(h["A"], h["B"]), (b["A"], b["B"], dict(confidence=1.0))], "problem 1", "confidence"),
             ([(b["A"], b["B"], dict(max_hypotheses=4097)), (h["A"], h["B"])], "problem 0", "max_hypotheses"),
             ([(h["A"], h["B"]), (h["A"], h["B"]), (np.zeros((2049, 2)), np.zeros((2049, 2)))], "problem 2", "m out of range")]
    for probs, index, field in cases:
        p = hctx.prepare(probs)
        assert p.run_raw() == homography.ERR_INVALID
        msg = hctx.last_error()
        assert index in msg and field in msg, msg
        raw = bytes(p.results)[:p.n * C.sizeof(homography.Result)]
        assert all(x == homography.FILL for x in raw) and all((m == homography.FILL).all() for m in p.masks)
    p = hctx.prepare([(h["A"], h["B"])])
    assert hctx.lib.dsdtm_find_homographies(hctx.handle, 1025, p.descs, p.results) == homography.ERR_INVALID and "n =" in hctx.last_error()
    assert hctx.lib.dsdtm_find_homographies(hctx.handle, 0, None, None) == homography.OK
    assert hc.same(hctx.find_homography(h["A"], h["B"]), hc.expected("H"))          # and the context still works


def test_chained_with_the_motion_step(hctx):
    """H of world B, as the device found it, fed to dsdtm_motion_step on a 64x48 model: the masks equal motion_restatement's run with
    the restatement's H."""
    wd = hc.world("B")
    got, want = hctx.find_homography(wd["A"], wd["B"]), hc.expected("B")
    assert got["found"] == 1 and np.array_equal(got["H"].view(np.uint64), want["H"].view(np.uint64))
    mw = mc.world("A")
    rs = MR.MotionRestatement(mw["width"], mw["height"])
    mctx = motion.MotionContext(0)
    model = motion.MotionModel(mctx, mw["width"], mw["height"])
    fired = 0
    for s in range(3):
        ref = rs.step(mc.image_of(mw, s), want["H"])
        assert not (ref["exp_arg"] != 0.0).any()          # exp is only ever handed 0: the device must be bit-equal
        mask, _ = model.step(mc.image_of(mw, s), got["H"])
        assert np.array_equal(mask, ref["mask"]), s
        assert np.array_equal(model.read().view(np.uint32), rs.model.state.view(np.uint32)), s
        fired += int((mask == 255).sum())
    model.close()
    mctx.close()
