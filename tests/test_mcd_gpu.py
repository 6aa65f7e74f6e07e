"""dsdtm_mcd_boxes / dsdtm_mcd_steps (libdsdtm_amd_mcd.so: csrc/contour.hip, csrc/mcd_api.cpp) against the restatement
dsdtm_amd/contour_restatement.py, which tests/test_mcd_cpu.py holds to hand-computed cases, its C twin, mcd_box_host and its mutants.
The contour step is integer-only: every comparison is bit-equality. The motion part of a whole Run is held exactly as
tests/test_motion_gpu.py holds dsdtm_motion_step (its compare(), its excused-pixel rule, MAX_EXCUSED_SHARE).
"""
import numpy as np
import pytest

from dsdtm_amd import contour_restatement as CR
from dsdtm_amd import mcd
from tests import mcd_cases as cases
from tests import motion_cases as mc
from tests.test_motion_gpu import _bits, compare

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()
SMALL = [(n, m) for n, (m, _) in HAND.items()] + cases.random_masks() + [
    ("width_37x29", np.where(np.random.default_rng(5).random((29, 37)) < 0.4, 255, 0).astype(np.uint8)),
    ("serpentine", cases.serpentine()), ("checkerboard", cases.checkerboard()), ("u_trap", cases.u_trap())]


@pytest.fixture(scope="module")
def ctx():
    c = mcd.McdContext(0)
    yield c
    c.close()


def _same(got, want, where):
    assert got["box"] == want["box"] and got["area2"] == want["area2"] and got["n_components"] == want["n_components"], \
        (where, got["box"], got["area2"], got["n_components"], want["box"], want["area2"], want["n_components"])
    assert np.array_equal(got["boxed"], want["boxed"]), (where, np.argwhere(got["boxed"] != want["boxed"])[:5].tolist())


def test_boxes_against_the_restatement(ctx):
    """Every small mask in ONE submission (mixed sizes), and each hand case against its hand-computed answer as well."""
    outs = ctx.boxes([m for _, m in SMALL])
    for (name, mask), got in zip(SMALL, outs):
        _same(got, cases.restated(name, mask), name)
        if name in HAND:
            want = HAND[name][1]
            assert got["box"] == want["box"] and got["area2"] == want["area2"] and got["n_components"] == want["n_components"], name
    u = cases.restated("u_trap", cases.u_trap())
    by_bound = sorted(u["components"], key=lambda c: -(c["maxx"] - c["minx"]) * (c["maxy"] - c["miny"]))
    assert by_bound[0]["area2"] < by_bound[1]["area2"] == u["area2"], "the prune's trap: the larger bound has the smaller area"
    assert cases.restated("serpentine", cases.serpentine())["n_components"] == 1 and cases.restated("checkerboard", cases.checkerboard())["n_components"] == 1


def test_boxes_strided_device_mask_is_read_in_place(ctx):
    import torch
    rng = np.random.default_rng(11)
    buf = rng.integers(1, 256, size=(24, 64)).astype(np.uint8)          # bytes beyond the width are non-zero: reading them is caught
    buf[:, :40] = np.where(rng.random((24, 40)) < 0.35, 255, 0)
    buf[5:15, 8:20] = 255
    dev = torch.from_numpy(buf).cuda()[:, :40]
    torch.cuda.synchronize()
    assert dev.stride(0) == 64
    got = ctx.boxes([dev])[0]
    _same(got, CR.ContourRestatement().run(buf[:, :40]), "device mask")
    assert np.array_equal(dev.cpu().numpy(), buf[:, :40]), "the source is not modified"
    host = ctx.boxes([buf[:, :40]])[0]                                   # the same view from host memory
    _same(host, got, "host view")


def test_boxes_640x480_twice_and_without_the_boxed_mask(ctx):
    mask = cases.blob_with_salt()
    want = cases.restated("blob_with_salt", mask)
    assert want["n_components"] > 1000 and want["box"][2] > 150
    first, second = ctx.boxes([mask])[0], ctx.boxes([mask])[0]
    _same(first, want, "640x480")
    _same(second, first, "the same call twice")
    bare = ctx.boxes([mask], want_boxed=False)[0]
    assert bare["boxed"] is None and (bare["box"], bare["area2"], bare["n_components"]) == (want["box"], want["area2"], want["n_components"])


def test_boxes_batch_of_eight_equals_eight_single_calls(ctx):
    picks = [m for _, m in SMALL[-8:]]
    batch = ctx.boxes(picks)
    for k, m in enumerate(picks):
        _same(ctx.boxes([m])[0], batch[k], k)


def test_boxes_limits(ctx):
    assert ctx.boxes([]) == []
    big = np.zeros((1024, 1025), np.uint8)
    with pytest.raises(mcd.McdError) as err:
        ctx.boxes([cases.u_trap(), big], want_boxed=False)
    assert err.value.status == mcd.ERR_INVALID and "mask 1" in err.value.message and "1025 x 1024" in err.value.message
    edge = np.zeros((1024, 1024), np.uint8)                             # the largest size the step takes
    edge[3:1020, 5:1000] = 255
    got = ctx.boxes([edge], want_boxed=False)[0]
    assert (got["box"], got["area2"], got["n_components"]) == ([5, 3, 995, 1017], 2 * 994 * 1016, 1)


def _run_step(model, wd, s, e, **kw):
    model.write(e["t"]["before"])
    return model.step(mc.image_of(wd, s), wd["H"][s], want_raw=True, features=e["px"], **kw)


@pytest.mark.parametrize("name", ["A", "C"])
def test_whole_run_step_by_step(ctx, name):
    wd, chain = mc.world(name), cases.chain_of(name)
    model = mcd.McdModel(ctx, wd["width"], wd["height"])
    assert np.array_equal(_bits(model.read()), _bits(chain[0]["t"]["before"])), "ProbModel::init"
    excused, exact = 0, []
    for s, e in enumerate(chain):
        r = _run_step(model, wd, s, e)
        # (a) the motion part, as tests/test_motion_gpu.py holds dsdtm_motion_step
        excused += compare(wd, e["t"], model.read(), r["mask_raw"], f"step {s}")[1]
        # (b) the contour part against the restatement applied to the mask the device returned
        c = CR.ContourRestatement().run(r["mask_raw"])
        _same(dict(r, boxed=r["mask"]), c, (name, s))
        assert np.array_equal(r["flags"], CR.features_on_mask(c["boxed"], e["px"])), (name, s)
        # (c) where the device's detect_img is the restated one, everything is the full restated chain
        if np.array_equal(r["mask_raw"], e["t"]["mask"]):
            exact.append(s)
            _same(dict(r, boxed=r["mask"]), e["c"], (name, s, "chain"))
            assert np.array_equal(r["flags"], e["flags"]), (name, s)
    assert excused <= mc.MAX_EXCUSED_SHARE * len(chain) * wd["width"] * wd["height"]
    drawn = cases.rectangle_steps(name)
    assert drawn and set(drawn) <= set(exact), (drawn, exact)
    model.close()


def test_whole_run_real_image_640x480(ctx):
    wd, e = mc.world("real"), cases.chain_of("real")[2]
    model = mcd.McdModel(ctx, 640, 480)
    r = _run_step(model, wd, 2, e)
    _, excused = compare(wd, e["t"], model.read(), r["mask_raw"], "step 2")
    assert excused <= mc.MAX_EXCUSED_SHARE * 640 * 480
    c = CR.ContourRestatement().run(r["mask_raw"])
    _same(dict(r, boxed=r["mask"]), c, "real")
    assert c["area2"] > 0 and np.array_equal(r["flags"], CR.features_on_mask(c["boxed"], e["px"]))
    # flags only: nothing but the flags and the box crosses the link
    model.write(e["t"]["before"])
    bare = model.step(mc.image_of(wd, 2), wd["H"][2], want_mask=False, features=e["px"])
    assert bare["mask"] is None and bare["mask_raw"] is None and np.array_equal(bare["flags"], r["flags"]) and bare["box"] == r["box"]
    model.close()


def test_single_step_equals_the_same_desc_in_a_batch_of_four(ctx):
    picks = (("A", 3), ("C", 2), ("A", 5), ("C", 3))
    entries, singles = [], []
    for name, s in picks:
        wd, e = mc.world(name), cases.chain_of(name)[s]
        m = mcd.McdModel(ctx, wd["width"], wd["height"])
        singles.append((_run_step(m, wd, s, e), m.read()))
        m.write(e["t"]["before"])
        entries.append(dict(model=m, image=mc.image_of(wd, s), H=wd["H"][s], features=e["px"], want_raw=True))
    for e, r, (one, state) in zip(entries, ctx.steps(entries), singles):
        assert np.array_equal(_bits(e["model"].read()), _bits(state))
        _same(dict(r, boxed=r["mask"]), dict(one, boxed=one["mask"]), "batch")
        assert np.array_equal(r["mask_raw"], one["mask_raw"]) and np.array_equal(r["flags"], one["flags"])
        e["model"].close()
    assert ctx.steps([]) == []


def test_a_refused_step_leaves_outputs_and_model_as_they_were(ctx):
    wd, chain = mc.world("A"), cases.chain_of("A")
    models = [mcd.McdModel(ctx, 64, 48) for _ in range(2)]
    for m in models:
        m.write(chain[3]["t"]["before"])
    before = [m.read() for m in models]
    bad_H = list(wd["H"][3])
    bad_H[5] = float("inf")
    p = ctx.prepare([dict(model=models[0], image=mc.image_of(wd, 3), H=wd["H"][3], features=chain[3]["px"], want_raw=True),
                     dict(model=models[1], image=mc.image_of(wd, 3), H=bad_H, features=chain[3]["px"], want_raw=True)])
    assert p.run_raw() == mcd.ERR_INVALID and "model 1: H is not finite" in ctx.last_error()
    for (mask, raw, flags), r in zip(p.outs, p.results()):
        assert (mask == 0xA5).all() and (raw == 0xA5).all() and (flags == 0xA5).all()
        assert r["box"] == [-1, -1, -1, -1] and r["area2"] == -1 and r["n_components"] == -1
    for m, b in zip(models, before):
        assert np.array_equal(_bits(m.read()), _bits(b))
    with pytest.raises(mcd.McdError) as err:
        mcd.McdModel(ctx, 1025, 1024).step(np.zeros((1024, 1025), np.uint8), mc.translation(0, 0))
    assert err.value.status == mcd.ERR_INVALID and "1025 x 1024" in err.value.message
    twin = dict(model=models[0], image=mc.image_of(wd, 3), H=wd["H"][3])
    with pytest.raises(mcd.McdError) as err:
        ctx.steps([twin, dict(twin)])
    assert "model 1" in err.value.message and "model 0" in err.value.message
    for m in models:
        m.close()


def test_motion_detector_runs_the_whole_run(ctx):
    wd, chain = mc.world("A"), cases.chain_of("A")
    det = mcd.MotionDetector(ctx, required_rows=48)
    for s, e in enumerate(chain):
        mask = det.Run(mc.image_of(wd, s), wd["H"][s], features=e["px"], want_raw=True)
        assert np.array_equal(det.mask_raw, e["t"]["mask"]) and np.array_equal(mask, e["c"]["boxed"]) and det.box == e["c"]["box"], s
    keep, rebuilt = det.motion_removal(chain[-1]["px"])
    assert np.array_equal(keep, 1 - chain[-1]["flags"]) and rebuilt[:200] == list(range(200))
    assert (chain[-1]["flags"] != chain[-1]["flags_raw"]).any(), "the box removes features the raw mask keeps"
