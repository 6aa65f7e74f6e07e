"""dsdtm_motion_step / dsdtm_motion_steps (libdsdtm_amd_motion.so: csrc/motion.hip, csrc/motion_api.cpp) against the numpy restatement
dsdtm_amd/motion_restatement.py, which tests/test_motion_cpu.py holds to its C twin, to a brute-force median and to its mutants.

Comparison rule. Every step of every world starts from the restatement's state (model_write before the step), so a difference cannot
compound; one extra run of world A carries the device's own state through all its steps.
 - Per cell and array the float bit patterns are EQUAL wherever the restatement handed exp an argument of exactly 0 — every cell of
   worlds A-C (asserted in tests/test_motion_cpu.py and again here).
 - In a cell that takes the exp branch the device's double exp may differ from the host libm's in its last place; there m_Age_Temp,
   m_Age, m_Mean and m_Var may differ by at most EXP_ULP_BOUND float ulps. The bound is TWICE the largest distance measured on the
   first GPU run of these worlds against this restatement (EXP_ULP_MEASURED; profiles/r15_motion_mask.txt), because libm versions
   differ; m_Mean_Temp and m_Var_Temp do not depend on exp and stay bit-equal.
 - The mask is equal everywhere except at pixels in an exp-branch cell where the restatement's |dist - 2 var| < 1e-4 dist; the share of
   pixels excused this way is capped at 0.5 % per world.
"""
import numpy as np
import pytest

from dsdtm_amd import motion
from dsdtm_amd import motion_restatement as R
from tests import motion_cases as mc

pytestmark = pytest.mark.gpu

EXP_ULP_MEASURED = 0            # the first GPU run: worlds D (1421 exp cells over its steps) and real (2546): every entry bit-equal
EXP_ULP_BOUND = 2 * EXP_ULP_MEASURED
ULP_ROWS = (R.MEAN, R.MEAN + 1, R.VAR, R.VAR + 1, R.AGE, R.AGE + 1, R.AGE_T, R.AGE_T + 1)      # what exp reaches


@pytest.fixture(scope="module")
def mctx():
    ctx = motion.MotionContext(0)
    yield ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(wd, t, state, mask, where=""):
    """One step of the device (state 12 x cells, mask) against the restatement's step t. Returns (largest ulp distance in exp cells,
    pixels excused)."""
    exp = mc.exp_cells(t)
    same = _bits(state) == _bits(t["after"])
    assert same[:, ~exp].all(), (wd["name"], where, "cells without exp differ", np.argwhere(~same & ~exp[None, :])[:5].tolist())
    worst = 0
    if exp.any():
        print(f"[motion] world {wd['name']} {where}: {int(exp.sum())} exp cells, {int((~same[:, exp]).sum())} entries differ", end="")
        ulp = mc.ulp_distance(state[:, exp], t["after"][:, exp])
        rest = [k for k in range(12) if k not in ULP_ROWS]
        assert (ulp[rest] == 0).all(), (wd["name"], where, "an array exp does not reach differs")
        worst = int(ulp.max())
        print(f", largest distance {worst} ulp")
        assert worst <= EXP_ULP_BOUND, (wd["name"], where, worst)
    differ = mask != t["mask"]
    excusable = mc.excusable_pixels(wd, t)
    assert not (differ & ~excusable).any(), (wd["name"], where, "mask differs", np.argwhere(differ & ~excusable)[:5].tolist())
    return worst, int(differ.sum())


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_world_step_by_step(mctx, name):
    wd, trace = mc.world(name), mc.trace_of(name)
    model = motion.MotionModel(mctx, wd["width"], wd["height"])
    assert np.array_equal(_bits(model.read()), _bits(trace[0]["before"])), "ProbModel::init"
    excused = 0
    for s, t in enumerate(trace):
        if name in "ABC":
            assert not mc.exp_cells(t).any()
        model.write(t["before"])
        mask, _ = model.step(mc.image_of(wd, s), wd["H"][s])
        excused += compare(wd, t, model.read(), mask, f"step {s}")[1]
    assert excused <= mc.MAX_EXCUSED_SHARE * len(trace) * wd["width"] * wd["height"]
    if name == "B":
        assert trace[1]["stale"].any() and (trace[1]["stale"] & trace[2]["stale"]).any()
    if name == "C":
        assert wd["stride"] == 80 and not mask[48:].any() and not mask[:, 68:].any()
    if name == "D":
        assert sum(int(mc.exp_cells(t).sum()) for t in trace) >= 0.05 * len(trace) * trace[0]["stale"].size
    model.close()


def test_world_a_carried_on_the_device(mctx):
    """The device's own state through all six steps (two generations swapped per step, the _Temp arrays persisting): bit-equal."""
    wd, trace = mc.world("A"), mc.trace_of("A")
    model = motion.MotionModel(mctx, wd["width"], wd["height"])
    model.write(np.full((12, 192), 3.0, np.float32))
    model.reset()
    for s, t in enumerate(trace):
        mask, _ = model.step(mc.image_of(wd, s), wd["H"][s])
        assert np.array_equal(_bits(model.read()), _bits(t["after"])) and np.array_equal(mask, t["mask"]), s
    model.close()


def _real_step(mctx, image):
    wd, t = mc.world("real"), mc.trace_of("real")[2]
    model = motion.MotionModel(mctx, 640, 480)
    model.write(t["before"])
    mask, _ = model.step(image, wd["H"][2])
    state = model.read()
    model.close()
    return state, mask


def test_real_image_from_host_and_from_device_memory(mctx):
    import torch
    wd, t = mc.world("real"), mc.trace_of("real")[2]
    view = mc.image_of(wd, 2)                                   # 480 x 640 inside the 752-wide buffer
    assert view.strides == (752, 1)
    s_host, m_host = _real_step(mctx, view)
    dev = torch.from_numpy(np.ascontiguousarray(wd["images"][2])).cuda()[:, 60:700]
    torch.cuda.synchronize()
    assert dev.stride(0) == 752 and dev.data_ptr() % 4 == 0
    s_dev, m_dev = _real_step(mctx, dev)
    assert np.array_equal(_bits(s_host), _bits(s_dev)) and np.array_equal(m_host, m_dev)
    assert (t["mask"] == 255).mean() > 0.01
    _, excused = compare(wd, t, s_host, m_host, "step 2")
    assert excused <= mc.MAX_EXCUSED_SHARE * 640 * 480


def _batch_entries(mctx):
    picks = (("A", 3), ("C", 3), ("real", 2))
    entries = []
    for name, s in picks:
        wd, t = mc.world(name), mc.trace_of(name)[s]
        m = motion.MotionModel(mctx, wd["width"], wd["height"])
        m.write(t["before"])
        px = mc.features(name)[0] if name == "A" and s == 5 else None
        entries.append(dict(model=m, image=mc.image_of(wd, s), H=wd["H"][s], features=px, world=wd, t=t))
    return entries


def test_batch_of_three_sizes_equals_the_single_steps(mctx):
    entries = _batch_entries(mctx)
    assert [(e["world"]["width"], e["world"]["height"]) for e in entries] == [(64, 48), (70, 50), (640, 480)]
    feats = np.array([[3.5, 2.5], [40.25, 30.0], [63.0, 47.0]], np.float32)
    entries[0]["features"] = feats
    outs = mctx.steps(entries)
    for e, (mask, flags) in zip(entries, outs):
        state = e["model"].read()
        e["model"].write(e["t"]["before"])
        mask1, flags1 = e["model"].step(e["image"], e["H"], features=e["features"])
        assert np.array_equal(_bits(state), _bits(e["model"].read())) and np.array_equal(mask, mask1)
        assert (flags is None and flags1 is None) or np.array_equal(flags, flags1)
        compare(e["world"], e["t"], state, mask, "batch")
        e["model"].close()
    assert mctx.steps([]) == []


def test_batch_refuses_the_same_model_twice(mctx):
    entries = _batch_entries(mctx)[:2]
    twin = dict(entries[0])
    before = [e["model"].read() for e in entries]
    with pytest.raises(motion.MotionError) as err:
        mctx.steps([entries[0], entries[1], twin])
    assert err.value.status == motion.ERR_INVALID and "model 2" in err.value.message and "model 0" in err.value.message
    for e, b in zip(entries, before):
        assert np.array_equal(_bits(e["model"].read()), _bits(b))
        e["model"].close()


def test_features_round_half_to_even(mctx):
    wd, trace = mc.world("A"), mc.trace_of("A")
    px, want = mc.features("A")
    assert len(px) == 200 and (px[8:100] % 1 == 0.5).all() and 0 < want.sum() < 200
    model = motion.MotionModel(mctx, 64, 48)
    model.write(trace[-1]["before"])
    mask, flags = model.step(mc.image_of(wd, 5), wd["H"][5], features=px)
    assert np.array_equal(mask, trace[-1]["mask"]) and np.array_equal(flags, want)
    # the same flags without asking for the mask: the lookup is made against the mask where it lies
    model.write(trace[-1]["before"])
    none, flags = model.step(mc.image_of(wd, 5), wd["H"][5], want_mask=False, features=px)
    assert none is None and np.array_equal(flags, want)
    # one feature outside the image: refused, named, nothing done
    bad = px.copy()
    bad[17] = [64.0, 10.0]
    before = model.read()
    with pytest.raises(motion.MotionError) as err:
        model.step(mc.image_of(wd, 5), wd["H"][5], features=bad)
    assert err.value.status == motion.ERR_INVALID and "feature 17" in err.value.message
    assert np.array_equal(_bits(model.read()), _bits(before))
    # n = 0 features
    mask, flags = model.step(mc.image_of(wd, 5), wd["H"][5], features=np.zeros((0, 2), np.float32))
    assert len(flags) == 0
    model.close()


def test_moving_detector_has_the_reference_shape(mctx):
    wd, trace = mc.world("A"), mc.trace_of("A")
    px, want = mc.features("A")
    det = motion.MovingDetector(mctx, required_rows=48)
    for s in range(6):
        mask = det.Mod_FastMCD(mc.image_of(wd, s), wd["H"][s], features=px if s == 5 else None)
        assert np.array_equal(mask, trace[s]["mask"]), s
    keep, rebuilt = det.motion_removal(px)
    assert np.array_equal(keep, 1 - want)
    assert rebuilt[:200] == list(range(200)) and rebuilt[200:] == [int(k) for k in np.flatnonzero(keep)]      # src/Frame.cpp:346-356
    with pytest.raises(ValueError):
        motion.MovingDetector(mctx, required_rows=480).Mod_FastMCD(mc.image_of(wd, 0), wd["H"][0])


def test_argument_errors_name_the_field(mctx):
    wd = mc.world("A")
    model = motion.MotionModel(mctx, 64, 48)
    img, before = mc.image_of(wd, 0), model.read()

    def refused(what, **kw):
        args = dict(image=img, H=mc.translation(0, 0))
        args.update(kw)
        with pytest.raises(motion.MotionError) as err:
            model.step(**args)
        assert err.value.status == motion.ERR_INVALID and what in err.value.message, err.value.message

    refused("H is not finite", H=[1, 0, 0, 0, 1, 0, 0, float("nan"), 1])
    refused("denominator", H=[1, 0, 0, 0, 1, 0, -1.0 / 61.0, 0, 1])          # positive at the left corner cells only
    refused("denominator", H=[1, 0, 0, 0, 1, 0, 0, 0, 0])
    refused("image is NULL", image=0, stride=64)
    for w, h, what in ((15, 48, "width"), (64, 12, "height")):
        with pytest.raises(motion.MotionError) as err:
            motion.MotionModel(mctx, w, h)
        assert err.value.status == motion.ERR_INVALID and what in err.value.message
    assert np.array_equal(_bits(model.read()), _bits(before))
    model.close()
