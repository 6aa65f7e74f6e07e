"""dsdtm_rarsac_reject / dsdtm_rarsac_reject_batch / dsdtm_rarsac_check (libdsdtm_amd_rarsac.so: csrc/rarsac.hip, csrc/rarsac_api.cpp) against
the restatement dsdtm_amd/rarsac_restatement.py (m = 2048: its C twin), which tests/test_rarsac_cpu.py holds to the twin, to the host
function and to the worlds' truth. Comparison rule: EVERY output is bit-equal — status, F, the grid, the score, best_hypothesis,
iterations_run, n_inliers — and a problem with found = 0 leaves its outputs as the caller filled them."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import rarsac
from dsdtm_amd import rarsac_restatement as R
from tests import rarsac_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = rarsac.RarsacContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return rc.c_twin(tmp_path_factory.mktemp("rarsac_twin"))


def problem(c, **over):
    return dict(cur=c["cur"], prev=c["prev"], width=c["width"], height=c["height"], **dict(c["params"], **over))


def want(name, twin):
    return rc.run_native(twin, rc.world(name)) if name == "m2048" else rc.expected(name)


def _report(name, got, exp):
    if got["found"] and exp["found"]:
        print(f"[rarsac] {name}: best {got['best_hypothesis']} / {exp['best_hypothesis']}, run {got['iterations_run']} / {exp['iterations_run']}, "
              f"inliers {got['n_inliers']} / {exp['n_inliers']}, score {got['score']!r} / {exp['score']!r}, differing {rc.differences(got, exp)}")
    else:
        print(f"[rarsac] {name}: found {got['found']} / {exp['found']}")


def _untouched(prepared, k):
    raw = bytes(prepared.results[k])
    at = rarsac.Result.found.offset
    return all(b == rarsac.FILL for b in raw[:at] + raw[at + 4:]) and (prepared.status[k] == rarsac.FILL).all()


@pytest.mark.parametrize("name", rc.NAMES)
def test_world_single_problem(ctx, twin, name):
    """m = 8 in 8 bins, m = 8 in 7 bins (found = 0, outputs untouched), 300 clean and with 40 % outliers, 2048 against the C twin, the
    round edges 1 / 255 / 256 / 257 / 1000, a stop on the last hypothesis of a round and on the first of the next, the worlds R4
    refuses, a peaked prior and another image size."""
    c, exp = rc.world(name), want(name, twin)
    p = ctx.prepare([problem(c)])
    ctx.check(p.run_raw())
    got = p.answers()[0]
    _report(name, got, exp)
    assert rc.same(got, exp), (name, rc.differences(got, exp))
    if not exp["found"]:
        assert _untouched(p, 0)


def test_what_the_worlds_exercise(ctx, twin):
    """The expectations themselves: the stop indices, the exact iteration counts, the refusals of R4."""
    assert rc.expected("m8 in 7 bins")["found"] == 0
    assert rc.expected("clean300")["iterations_run"] < R.ROUND and rc.expected("clean300")["best_hypothesis"] >= 0
    for n in (1, 255, 256, 257, 1000):
        assert rc.expected("noise64 x%d" % n)["iterations_run"] == n
    assert rc.expected("stop at 255")["iterations_run"] == 256 and rc.expected("stop at 256")["iterations_run"] == 257
    for name in ("coincident", "collinear"):
        e = rc.expected(name)
        assert e["found"] == 1 and e["best_hypothesis"] == -1 and e["iterations_run"] == 300 and not e["status"].any() and e["score"] == R.DBL_MIN
    assert not rc.same(rc.expected("peaked prior"), rc.expected("outliers300"))


def test_default_entry_and_refusals(ctx):
    c = rc.world("outliers300")
    assert rc.same(ctx.reject(c["cur"], c["prev"]), rc.expected("outliers300"))
    seven = rc.world("m8")
    p = ctx.prepare([problem(dict(seven, cur=seven["cur"][:7], prev=seven["prev"][:7]))])
    assert p.run_raw() == rarsac.ERR_INVALID and "problem 0" in ctx.last_error() and "m out of range" in ctx.last_error()
    w = rc.world("480x640")
    cur = w["cur"].copy()
    cur[41] = (100.0, 500.0)                      # row 500 / 48 = 10: bin 102
    p = ctx.prepare([problem(rc.world("m8")), problem(dict(w, cur=cur))])
    assert p.run_raw() == rarsac.ERR_INVALID
    assert "problem 1" in ctx.last_error() and "index 41" in ctx.last_error() and "R1" in ctx.last_error(), ctx.last_error()
    assert _untouched(p, 0) and bytes(p.results[1]) == bytes([rarsac.FILL]) * C.sizeof(rarsac.Result)
    with pytest.raises(R.Refused) as e:
        rc.restate(dict(w, cur=cur))
    assert e.value.index == 41
    cur[41] = (np.nan, 5.0)
    p = ctx.prepare([problem(dict(w, cur=cur))])
    assert p.run_raw() == rarsac.ERR_INVALID and "cur is not finite at index 41" in ctx.last_error()
    assert rc.same(ctx.reject(c["cur"], c["prev"]), rc.expected("outliers300"))          # and the context still works


def test_mixed_batch_equals_single_calls_in_two_orders(ctx, twin):
    names = list(rc.NAMES)
    probs = [problem(rc.world(n)) for n in names]
    p = ctx.prepare(probs)
    ctx.check(p.run_raw())
    first = p.answers()
    for k, n in enumerate(names):
        assert rc.same(first[k], want(n, twin)), (n, rc.differences(first[k], want(n, twin)))
    assert _untouched(p, names.index("m8 in 7 bins"))
    order = np.random.default_rng(26).permutation(len(names))
    shuffled = ctx.reject_batch([probs[i] for i in order])
    rev = ctx.reject_batch(probs[::-1])[::-1]
    for k, n in enumerate(names):
        assert rc.same(first[k], rev[k]), n
        assert rc.same(first[k], shuffled[list(order).index(k)]), n


def test_check_on_the_winning_F_returns_status_and_grid(ctx, twin):
    for name in ("outliers300", "clean300", "480x640", "m2048"):
        c, exp = rc.world(name), want(name, twin)
        got = ctx.check_batch([dict(problem(c), F=exp["F"])])[0]
        assert np.array_equal(got["status"], exp["status"]) and np.array_equal(got["grid"].view(np.uint64), exp["grid"].view(np.uint64)), name
        assert got["score"] == exp["score"] and got["n_inliers"] == exp["n_inliers"] and got["best_hypothesis"] == -1 and got["iterations_run"] == 0
        assert rc.same(got, R.check_fundamental(c["cur"], c["prev"], exp["F"], c["width"], c["height"])), name


def test_klt_flow_then_rarsac_reject(ctx):
    """The pipeline of Test/test_Optimizer.cpp:91-106 on a synthetic image pair: dsdtm_klt_flow, then dsdtm_rarsac_reject on what it
    tracked; the device's answer is the restatement's on the same correspondences."""
    from dsdtm_amd import klt
    h, w = 480, 640
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)

    def image(dx, dy):
        x, y = xs - dx, ys - dy
        v = 128 + 50 * np.sin(x * 0.11 + y * 0.07) + 40 * np.cos(y * 0.13 - x * 0.05) + 30 * np.sin(x * 0.31) * np.cos(y * 0.29)
        return np.clip(v, 0, 255).astype(np.uint8)
    prev_img, cur_img = image(0.0, 0.0), image(2.0, 1.0)
    gx, gy = np.meshgrid(np.arange(40, 600, 40), np.arange(40, 440, 40))
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
    kctx = klt.KltContext(0)
    try:
        flow = kctx.flow([dict(prev=prev_img, cur=cur_img, points=pts)])[0]
    finally:
        kctx.close()
    ok = flow["status"].astype(bool)
    cur, prev = np.asarray(flow["points"], np.float32)[ok], pts[ok]          # tracked from the previous image into the current one
    inside = (cur[:, 0] >= 0) & (cur[:, 0] < w) & (cur[:, 1] >= 0) & (cur[:, 1] < h)
    cur, prev = cur[inside], prev[inside]
    assert len(cur) >= 100 and np.abs(np.median(cur - prev, axis=0) - (2.0, 1.0)).max() < 0.25
    got = ctx.reject(cur, prev)
    exp = R.reject_fundamental(cur, prev)
    print(f"[rarsac] klt chain: {len(cur)} tracked, best {got.get('best_hypothesis')}, run {got.get('iterations_run')}, inliers {got.get('n_inliers')}")
    assert got["found"] == 1 and rc.same(got, exp), rc.differences(got, exp)
