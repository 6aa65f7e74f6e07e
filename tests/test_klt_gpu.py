"""dsdtm_klt_steps / dsdtm_klt_flow (libdsdtm_amd_klt.so: csrc/klt.hip, csrc/klt_api.cpp) against the restatement
dsdtm_amd/klt_restatement.py, which tests/test_klt_cpu.py holds to hand cases, klt_flow_host and its mutants. Window sums are integers and
the scalar tail is uncontracted double in one order: every comparison is bit-equality (points and residual as 32-bit patterns, H as
64-bit patterns)."""
import numpy as np
import pytest

from dsdtm_amd import klt, mcd
from dsdtm_amd import contour_restatement as CR
from dsdtm_amd import klt_restatement as KR
from dsdtm_amd import synth
from tests import klt_cases as cases

pytestmark = pytest.mark.gpu
K = KR.Klt()


@pytest.fixture(scope="module")
def ctx():
    c = klt.KltContext(0)
    yield c
    c.close()


def _same_step(got, want, where):
    for f in ("source", "n_points", "n_tracked", "n_inliers"):
        assert got[f] == want[f], (where, f, got[f], want[f])
    assert np.array_equal(got["H"].view(np.uint64), np.asarray(want["H"], np.float64).view(np.uint64)), (where, got["H"], want["H"])
    if "points" in got:
        assert np.array_equal(got["prev_points"], want["prev_points"]), where
        assert np.array_equal(got["points"].view(np.uint32), want["points"].view(np.uint32)), (where, np.abs(got["points"] - want["points"]).max())
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"]), where
        assert np.array_equal(got["mask"], want["mask"]), where
    if want["ransac"] is not None and want["source"] == KR.SOURCE_RANSAC:
        for f in ("best_hypothesis", "rounds", "refit_iterations", "cost_before", "cost_after"):
            assert got[f] == want["ransac"][f], (where, f)


def _pairs():
    out = [(f"{size} {shift}", *cases.shift_world(size, shift)) for size in ("160x120", "171x123") for shift in cases.SHIFTS]
    out.append(("warp", *cases.warp_world()[:2]))
    out.append(("flat", *cases.flat_world()))
    return out


def test_every_small_world_against_the_restatement(ctx):
    """Two steps per world (the first seeds), all worlds' second steps in ONE submission of mixed sizes."""
    worlds = _pairs()
    models = [klt.KltModel(ctx, a.shape[1], a.shape[0]) for _, a, _ in worlds]
    firsts = ctx.steps([dict(model=m, image=a) for m, (_, a, _) in zip(models, worlds)])
    seconds = ctx.steps([dict(model=m, image=b) for m, (_, _, b) in zip(models, worlds)])
    for (name, a, b), m, f, s in zip(worlds, models, firsts, seconds):
        r = KR.KltModel(a.shape[1], a.shape[0])
        _same_step(f, r.step(a), name + " first")
        assert f["frame"] == 0 and s["frame"] == 1
        _same_step(s, r.step(b), name)
        for got, want in zip(m.pyramid(), synth.build_pyramid(b, 4)):          # the pyramid the library built: dsdtm_pyrdown's bytes
            assert np.array_equal(got, want), name
        m.close()
    assert seconds[-1]["source"] == klt.SOURCE_IDENTITY and seconds[-1]["n_tracked"] == 8          # flat: fewer than 10 survivors


def test_moving_block_world_and_the_hand_over_to_mcd_step(ctx):
    """640x480, 361 points: the RANSAC's H follows the background; KLTWrapper.RunTrack -> dsdtm_mcd_step equals the restated chain."""
    prev, cur, flags = cases.block_world()
    w = klt.KLTWrapper(ctx)
    w.Init(prev)
    got = w.RunTrack(cur, want=True)
    r = KR.KltModel(640, 480)
    r.step(prev)
    want = r.step(cur)
    _same_step(got, want, "block")
    fl = flags[np.flatnonzero(got["status"])]
    assert not got["mask"][fl == 1].any() and got["mask"][fl == 0].all()
    assert np.array_equal(w.GetHomography().ravel(), want["H"])
    mctx = mcd.McdContext(0)
    a, b = mcd.McdModel(mctx, 640, 480), mcd.McdModel(mctx, 640, 480)
    a.step(prev, KR.IDENTITY)
    b.step(prev, KR.IDENTITY)
    x, y = a.step(cur, w.GetHomography(), want_raw=True), b.step(cur, want["H"], want_raw=True)
    assert np.array_equal(x["mask"], y["mask"]) and x["box"] == y["box"] and x["area2"] == y["area2"]
    boxed = CR.ContourRestatement().run(x["mask_raw"])
    assert np.array_equal(x["mask"], boxed["boxed"]) and x["box"] == boxed["box"]
    for m in (a, b):
        m.close()
    mctx.close()


def test_a_model_over_five_frames_with_the_kept_h(ctx):
    """Frame by frame against the restatement's chain: the swap of the pyramids, and in frame 4 a one-column grid whose points are
    collinear, so the RANSAC finds nothing and the H of frame 3 is kept (K9)."""
    w, h = cases.SIZES["171x123"]
    c = cases.canvas(w, h)
    frames = [cases.crop(c, w, h, dx, dy) for dx, dy in ((0, 0), (3, -2), (5, 1), (5, 1), (2, 3))]
    grids = [(0, 0), (0, 0), (0, 0), (85, 8), (0, 0)]
    m, r = klt.KltModel(ctx, w, h), KR.KltModel(w, h)
    sources = []
    for k, (img, (gw, gh)) in enumerate(zip(frames, grids)):
        padded = np.zeros((h, w + 5), np.uint8)          # an odd stride of the caller
        padded[:, :w] = img
        got = m.step(padded[:, :w], grid_w=gw, grid_h=gh)
        want = r.step(img, gw=gw or None, gh=gh or None)
        _same_step(got, want, f"frame {k}")
        assert got["frame"] == k
        sources.append(got["source"])
    assert sources == [klt.SOURCE_IDENTITY, klt.SOURCE_RANSAC, klt.SOURCE_RANSAC, klt.SOURCE_KEPT, klt.SOURCE_RANSAC]
    m.reset()
    assert m.step(frames[1])["source"] == klt.SOURCE_IDENTITY          # after a reset the next step is a first step
    m.close()


def test_batch_of_eight_equals_eight_single_calls(ctx):
    """Mixed sizes, strides, memory kinds (pageable, pinned and device images), a first step and a step with fewer than 10 survivors."""
    import torch
    worlds = [("160x120", (3, -2)), ("171x123", (6, 5)), ("160x120", (6, 5)), ("171x123", (0, 0)), ("160x120", (0, 0)), ("171x123", (3, -2))]
    pairs = [cases.shift_world(*wd) for wd in worlds] + [cases.flat_world(), cases.warp_world()[:2]]

    def image(k, img):
        if k % 3 == 1:
            return torch.from_numpy(img).cuda()
        if k % 3 == 2:
            t = torch.zeros((img.shape[0], img.shape[1] + 3), dtype=torch.uint8).pin_memory()
            t[:, :img.shape[1]] = torch.from_numpy(img)
            return t[:, :img.shape[1]]
        return img

    def run(batched):
        models = [klt.KltModel(ctx, a.shape[1], a.shape[0]) for a, _ in pairs]
        seeds = [dict(model=m, image=image(k, a)) for k, (m, (a, _)) in enumerate(zip(models, pairs)) if k != 4]      # model 4: its first step is in the batch
        steps = [dict(model=m, image=image(k, b)) for k, (m, (_, b)) in enumerate(zip(models, pairs))]
        if batched:
            ctx.steps(seeds)
            out = ctx.steps(steps)
        else:
            for s in seeds:
                ctx.steps([s])
            out = [ctx.steps([s])[0] for s in steps]
        torch.cuda.synchronize()
        for m in models:
            m.close()
        return out

    single, batch = run(False), run(True)
    for k, (s, b) in enumerate(zip(single, batch)):
        _same_step(b, dict(s, ransac=None), f"model {k}")
        for f in ("best_hypothesis", "rounds", "refit_iterations", "cost_before", "cost_after", "frame"):
            assert s[f] == b[f], (k, f)
    assert batch[4]["frame"] == 0 and batch[4]["source"] == klt.SOURCE_IDENTITY and batch[6]["n_tracked"] == 8
    r = KR.KltModel(160, 120)
    r.step(pairs[0][0])
    _same_step(batch[0], r.step(pairs[0][1]), "model 0 against the restatement")


@pytest.mark.parametrize("window,levels", [(4, 1), (10, 4), (21, 3)])
def test_flow_border_points_windows_and_levels(ctx, window, levels):
    prev, cur = cases.shift_world("160x120", (3, -2))
    pts = cases.border_points(160, 120)
    got = ctx.flow([dict(prev=prev, cur=cur, points=pts, window=window, levels=levels)])[0]
    assert cases.same_flow(got, K.flow(prev, cur, pts, window=window, levels=levels))


def test_flow_five_levels_guesses_and_a_batch(ctx):
    """Five levels need a larger image (320x240: 20x15 at the top); initial guesses at one level; both pairs in one submission."""
    c = cases.canvas(320, 240)
    a, b = cases.crop(c, 320, 240), cases.crop(c, 320, 240, 6, 5)
    pts5 = np.array([(160, 120), (100.5, 80.25), (40, 40), (300, 200), (8, 8), (250.75, 60.5)], np.float32)
    prev, cur = cases.shift_world("160x120", (6, 5))
    pts = KR.grid_points(160, 120)
    g = pts + np.array([5.5, 4.5], np.float32)
    got = ctx.flow([dict(prev=a, cur=b, points=pts5, levels=5), dict(prev=prev, cur=cur, points=pts, guesses=g, levels=1)])
    assert cases.same_flow(got[0], K.flow(a, b, pts5, levels=5))
    assert cases.same_flow(got[1], K.flow(prev, cur, pts, guesses=g, levels=1)) and got[1]["status"].all()


# ---- the edges tests/test_klt_cpu.py holds to their claims: saturated contrast, pass boundaries, every exit, the compaction ------------

@pytest.mark.parametrize("levels", [1, 4])
def test_flow_saturated_contrast(ctx, levels):
    """Totals above 2^31 and right-hand sides beyond +-2^32 through wave_sum's two 32-bit halves; |dx| = 4080. One submission per level
    count: four worlds x windows 21, 16, 10 and 4. At 160 x 120 the entry refuses four levels for windows 21 and 16 (the coarsest level,
    20 x 15, cannot hold window + 3 pixels): that refusal is asserted, and those windows run at the three levels it accepts."""
    def depth(window):
        return min(levels, cases.deepest_levels(window))

    assert [depth(w) for w in (21, 16, 10, 4)] == ([1, 1, 1, 1] if levels == 1 else [3, 3, 4, 4])
    pairs = [dict(prev=prev, cur=cur, points=cases.saturated_points(window), window=window, levels=depth(window))
             for _, prev, cur in cases.saturated_worlds() for window in (21, 16, 10, 4)]
    got = ctx.flow(pairs)
    for p, g in zip(pairs, got):
        assert cases.same_flow(g, cases.restated(p)), (p["window"], p["levels"])
    assert got[0]["status"][:7].all()
    for p in pairs[:2]:
        with pytest.raises(klt.KltError) as e:
            ctx.flow([dict(p, levels=4)])
        assert e.value.status == klt.ERR_INVALID and "coarsest" in e.value.message


def test_flow_window_sweep_around_a_pass_of_64_lanes(ctx):
    """Areas 64 and 256 fill a pass, 81 and 289 start the next with one pixel; as many levels as the entry accepts per window."""
    prev, cur = cases.shift_world("160x120", (3, -2))
    pts = cases.border_points(160, 120)
    pairs = [dict(prev=prev, cur=cur, points=pts, window=w, levels=cases.deepest_levels(w)) for w in cases.SWEEP_WINDOWS]
    for p, g in zip(pairs, ctx.flow(pairs)):
        assert cases.same_flow(g, cases.restated(p)), p["window"]
        assert g["status"][:2].all()


def test_flow_exit_world(ctx):
    """One call per parameter set. (The Python binding always passes a residual array, and dsdtm_klt_flow gives the kernel a device
    residual whatever the caller wants: a run without one cannot be made from here and is left out.)"""
    prev, cur, pts, g, sets = cases.exit_world()
    for kw in sets:
        pair = dict(prev=prev, cur=cur, points=pts, guesses=g, **kw)
        got = ctx.flow([cases.device_pair(pair)])[0]
        want = cases.restated(pair)
        for f in ("iterations", "status"):
            assert np.array_equal(got[f], want[f]), (kw, f, got[f].tolist(), want[f].tolist())
        assert cases.same_flow(got, want), kw
    a, b, _ = cases.warp_world()                                       # the oscillating point of test_mutant_no_halving_on_an_oscillating_point
    pair = dict(prev=a, cur=b, points=KR.grid_points(160, 120), eps=cases.EPS_ZERO)
    assert cases.same_flow(ctx.flow([cases.device_pair(pair)])[0], cases.restated(pair))


def test_flow_mixed_submission(ctx):
    """Unlike windows, level counts and point counts (1 to 2048) in one launch = the pairs one by one = the restatement."""
    pairs = cases.mixed_pairs()
    dev = [cases.device_pair(p) for p in pairs]
    together = ctx.flow(dev)
    for k, (p, d, g) in enumerate(zip(pairs, dev, together)):
        assert len(g["status"]) == len(p["points"])
        assert cases.same_flow(g, ctx.flow([d])[0]), k
        assert cases.same_flow(g, cases.restated(p)), k


def test_compaction_edges(ctx):
    """klt_compact_kernel: 64, 65 and 128 points, rounds that are full, empty, or hold lanes 0 and 63 with holes between, and 9 / 10 / 0
    survivors around `base >= min_tracked`; as one batch and as single calls. After the step with no survivor the model goes on."""
    names = list(cases.COMPACTION)
    worlds = [cases.compaction_step(name) for name in names]

    def run(batched):
        models = [klt.KltModel(ctx, 160, 120) for _ in names]
        seeds = [dict(model=m, image=w[0], grid_w=w[2], grid_h=w[3]) for m, w in zip(models, worlds)]
        steps = [dict(model=m, image=w[1], grid_w=w[2], grid_h=w[3]) for m, w in zip(models, worlds)]
        if batched:
            ctx.steps(seeds)
            out = ctx.steps(steps)
        else:
            for s in seeds:
                ctx.steps([s])
            out = [ctx.steps([s])[0] for s in steps]
        return models, out

    for batched in (True, False):
        models, out = run(batched)
        for name, w, got in zip(names, worlds, out):
            _same_step(got, w[4], (name, batched))
            assert got["n_points"] == cases.COMPACTION[name][3]
        by = dict(zip(names, out))
        assert by["9 survivors"]["source"] == klt.SOURCE_IDENTITY and by["9 survivors"]["n_tracked"] == 9
        assert by["0 survivors"]["source"] == klt.SOURCE_IDENTITY and by["0 survivors"]["n_tracked"] == 0
        assert by["10 survivors"]["n_tracked"] == 10 and by["10 survivors"]["source"] == worlds[names.index("10 survivors")][4]["source"] == klt.SOURCE_RANSAC
        if batched:          # the chain after no survivor at all: the next step on a textured frame
            k = names.index("0 survivors")
            a, b = cases.painted_world([])
            r = KR.KltModel(160, 120, gw=17, gh=13)
            for img in worlds[k][:2]:
                r.step(img)
            want = r.step(b)
            _same_step(models[k].step(b, grid_w=17, grid_h=13), want, "after 0 survivors")
            assert want["n_tracked"] == 0          # (tracked from the flat frame: nothing again)
            want = r.step(a)
            _same_step(models[k].step(a, grid_w=17, grid_h=13), want, "a textured pair after 0 survivors")
            assert want["source"] == KR.SOURCE_RANSAC and want["n_tracked"] > 10
        for m in models:
            m.close()


def test_refusals_leave_every_output_and_model_untouched(ctx):
    prev, cur = cases.shift_world("160x120", (3, -2))
    m = klt.KltModel(ctx, 160, 120)
    m.step(prev)
    for bad, needle in ((dict(model=m, image=cur, grid_w=2, grid_h=2), "more than 2048"), (dict(model=m, image=cur, stride=100), "stride")):
        if "stride" in bad:
            bad["image"] = cur.ctypes.data
        with pytest.raises(klt.KltError) as e:
            ctx.steps([bad])
        assert e.value.status == klt.ERR_INVALID and needle in e.value.message, e.value.message
    with pytest.raises(klt.KltError) as e:
        ctx.steps([dict(model=m, image=cur), dict(model=m, image=cur)])
    assert "twice" in e.value.message
    for size, levels, needle in (((40, 120), 4, "width"), ((160, 90), 4, "height"), ((160, 120), 6, "levels")):
        with pytest.raises(klt.KltError) as e:
            klt.KltModel(ctx, *size, levels)
        assert e.value.status == klt.ERR_INVALID and needle in e.value.message
    for kw, needle in ((dict(window=2), "window"), (dict(window=22), "window"), (dict(levels=6), "levels"), (dict(levels=5), "coarsest")):
        with pytest.raises(klt.KltError) as e:
            ctx.flow([dict(prev=prev, cur=cur, points=[(80, 60)], **kw)])
        assert needle in e.value.message
    r = KR.KltModel(160, 120)                           # the refused calls changed nothing: the model still tracks from `prev`
    r.step(prev)
    _same_step(m.step(cur), r.step(cur), "after refusals")
    assert m.step_single(prev)["frame"] == 2
    m.close()


def test_motion_detector_without_an_h_argument(ctx):
    """MotionDetector.RunTrack(image) = KLTWrapper.RunTrack followed by Run(image, H): the second adapter."""
    prev, cur, _ = cases.block_world()
    det, ref, w = mcd.MotionDetector(), mcd.MotionDetector(), klt.KLTWrapper(ctx)
    feats = np.array([(300, 200), (50, 50)], np.float32)
    for img in (prev, cur):
        got = det.RunTrack(img, features=feats)
        w.RunTrack(img)
        want = ref.Run(img, w.GetHomography().reshape(9), features=feats)
        assert np.array_equal(got, want) and det.box == ref.box and np.array_equal(det._pending, ref._pending)
    assert det.klt.last["source"] == klt.SOURCE_RANSAC and np.array_equal(det.klt.GetHomography(), w.GetHomography())


def test_cpp_adapters_and_the_linked_example(tmp_path):
    """dsdtm_amd/host/example_klt.cpp linked and run: DSDTM::KLTWrapper in front of DSDTM::MotionDetector on a scene that moves 3 px per
    frame; it exits with 0 only when every H is that translation and the device tracks as many points as klt_step_host."""
    import os
    import subprocess
    from dsdtm_amd import motion
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsdtm_amd", "host")
    exe = str(tmp_path / "example_klt")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "example_klt.cpp"), klt.lib_path(), mcd.lib_path(),
                    motion.lib_path(), "-Wl,-rpath," + os.path.dirname(klt.lib_path()), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and r.stdout.count("source 1") == 3, (r.stdout, r.stderr)
