"""dsdtm_framediff_steps / _step / _warp (libdsdtm_amd_framediff.so: csrc/framediff.hip, csrc/framediff_api.cpp) against the restatement
dsdtm_amd/framediff_restatement.py, which tests/test_framediff_cpu.py holds to hand cases, frame_diff_host and its mutants. The map is
uncontracted double in one order and everything behind it is integer: every comparison is equality of bytes (M as 64-bit patterns)."""
import os
import subprocess

import numpy as np
import pytest

from dsdtm_amd import framediff, mcd, motion
from dsdtm_amd import framediff_restatement as FR
from tests import framediff_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = framediff.FrameDiffContext(0)
    yield c
    c.close()


def _pair(c, **kw):
    return dict(a=c["a"], b=c["b"], H=c["H"], flags=c["flags"], threshold=c["threshold"], maxval=c["maxval"], features=c["features"], mask=True,
                warped=True, **kw)


def _same(got, want, where):
    assert np.array_equal(got["M"].view(np.uint64), want["M"].view(np.uint64)), (where, got["M"], want["M"])
    for s in ("warped", "mask", "flags"):
        if got[s] is not None:
            assert np.array_equal(np.asarray(got[s]), want[s]), (where, s, int((np.asarray(got[s]) != want[s]).sum()))
    assert got["n_foreground"] == want["n_foreground"] and got["n_flagged"] == want["n_flagged"], (where, got["n_foreground"], want["n_foreground"])


@pytest.fixture(scope="module")
def singles(ctx):
    """Every case through the single entry, once."""
    return {c["name"]: ctx.step(c["a"], c["b"], c["H"], flags=c["flags"], threshold=c["threshold"], maxval=c["maxval"], features=c["features"],
                                mask=True, warped=True) for c in cases.all_cases()}


@pytest.mark.parametrize("name", cases.names())
def test_device_is_the_restatement(singles, name):
    _same(singles[name], cases.restated(name), name)


def test_one_batch_of_all_cases_in_every_memory_kind_equals_the_single_calls(ctx, singles):
    """Mixed sizes in one submission; a, b and mask rotate through pageable, pinned and device memory (warped: host)."""
    import torch
    pairs, held = [], []
    for k, c in enumerate(cases.all_cases()):
        kind = k % 3
        h, w = c["a"].shape

        def place(img):
            if kind == 0:
                return img
            t = torch.from_numpy(np.ascontiguousarray(img))
            return t.pin_memory() if kind == 1 else t.cuda()
        a = place(c["a"])
        b = a if c["same"] else place(c["b"])
        full = None if kind == 0 else torch.full((h, w + 3), 0xA5, dtype=torch.uint8)
        full = full if kind == 0 else full.pin_memory() if kind == 1 else full.cuda()
        mask = True if kind == 0 else full[:, :w]
        held.append((a, b, mask, full))
        pairs.append(dict(_pair(c), a=a, b=b, mask=mask))
    torch.cuda.synchronize()
    out = ctx.steps(pairs)
    for c, r, (a, b, mask, full) in zip(cases.all_cases(), out, held):
        got = dict(r, mask=r["mask"] if mask is True else mask.cpu().numpy())
        _same(got, cases.restated(c["name"]), c["name"] + " in the batch")
        one = singles[c["name"]]
        assert np.array_equal(got["mask"], one["mask"]) and np.array_equal(r["warped"], one["warped"]) and r["n_foreground"] == one["n_foreground"]
        assert np.array_equal(r["M"].view(np.uint64), one["M"].view(np.uint64)) and np.array_equal(r["flags"], one["flags"])
        if full is not None:
            assert (full.cpu().numpy()[:, c["a"].shape[1]:] == 0xA5).all(), c["name"]          # the gap between rows is not touched


def test_strided_outputs_keep_their_gaps(ctx):
    c = cases.by_name("rotation with scale 129x45 direct")
    mask, warped = np.full((45, 140), 0xA5, np.uint8), np.full((45, 131), 0xA5, np.uint8)
    r = ctx.step(c["a"], c["b"], c["H"], flags=c["flags"], threshold=c["threshold"], maxval=c["maxval"], mask=mask[:, :129], warped=warped[:, :129])
    want = cases.restated(c["name"])
    assert np.array_equal(mask[:, :129], want["mask"]) and (mask[:, 129:] == 0xA5).all() and np.array_equal(warped[:, :129], want["warped"]) and (warped[:, 129:] == 0xA5).all()
    assert r["n_foreground"] == want["n_foreground"]


def test_flags_alone_without_a_mask(ctx):
    """mask == NULL: the feature test reads a mask that never leaves the device."""
    for name in ("threshold 50 and 51 maxval 255", "threshold 50 and 51 maxval 200", "640x480"):
        c, want = cases.by_name(name), cases.restated(name)
        r = ctx.step(c["a"], c["b"], c["H"], flags=c["flags"], threshold=c["threshold"], maxval=c["maxval"], features=c["features"], mask=None)
        assert r["mask"] is None and r["warped"] is None
        assert np.array_equal(r["flags"], want["flags"]) and r["n_flagged"] == want["n_flagged"] and r["n_foreground"] == want["n_foreground"]
    assert cases.restated("threshold 50 and 51 maxval 255")["n_flagged"] == 3 and cases.restated("threshold 50 and 51 maxval 200")["n_flagged"] == 0
    c = cases.by_name("blocks 4x4 5x5 6x6")
    r = ctx.step(c["a"], c["b"], c["H"], mask=None)                      # neither mask nor features: the counter alone
    assert r["n_foreground"] == cases.restated(c["name"])["n_foreground"] == 181


def test_warp_alone(ctx):
    import torch
    picked = [cases.by_name(n) for n in ("rotation with scale 129x45 direct", "perspective through W = 0 70x37 inverse", "halves 1/64 3/64 70x37 direct",
                                         "entries of 1e300 129x45 direct", "nan in the map 70x37 inverse", "640x480")]
    dev = torch.full((480, 640), 0xA5, dtype=torch.uint8, device="cuda")
    out = ctx.warp([dict(b=c["b"], H=c["H"], flags=c["flags"], warped=dev if c["name"] == "640x480" else True) for c in picked])
    for c, w in zip(picked, out):
        got = w.cpu().numpy() if c["name"] == "640x480" else w
        assert np.array_equal(got, cases.restated(c["name"])["warped"]), c["name"]


def test_refusals_leave_the_outputs(ctx):
    c = cases.by_name("threshold 50 and 51 maxval 255")
    for kw, needle in ((dict(H=np.arange(1.0, 10.0)), "singular"), (dict(threshold=255), "threshold"), (dict(maxval=256), "maxval"),
                       (dict(features=[(69.5, 3)]), "rounds outside the image at feature 0"), (dict(H=cases.NAN_M), "singular")):
        p = framediff.Prepared(ctx, [_pair(cases.by_name("blocks 4x4 5x5 6x6")), dict(_pair(c), **kw)])
        assert p.run_raw() == framediff.ERR_INVALID and "desc 1" in ctx.last_error() and needle in ctx.last_error(), ctx.last_error()
        for mask, warped, flags in p.outs:
            assert (mask == framediff.FILL).all() and (warped == framediff.FILL).all() and (flags is None or (flags == framediff.FILL).all())


def _block_frames():
    """Two 320x240 frames: a smooth background (the texture of tests/klt_cases.py, dimmed) that moves by (3, 0) and a bright 50x50
    block that jumps by 33."""
    from tests import klt_cases
    c = klt_cases.canvas(320, 240)
    prev, cur = klt_cases.crop(c, 320, 240) // 2 + 20, klt_cases.crop(c, 320, 240, 3, 0) // 2 + 20
    prev[90:140, 100:150] = 250
    cur[90:140, 133:183] = 250
    return prev.astype(np.uint8), cur.astype(np.uint8)


def test_mod_framediff_klt_flags_the_moved_block():
    prev, cur = _block_frames()
    on_block = np.array([(170, 100), (178.5, 130.5), (160, 115)], np.float32)          # the block's new place, clear of its old one
    static = np.array([(40, 40), (280, 200), (60, 180), (250, 30)], np.float32)
    feats = np.concatenate([on_block, static])
    det = mcd.MotionDetector()
    assert det.Mod_FrameDiff_KLT(prev, features=feats, maxval=255) is None          # the first image seeds the tracker
    mask = det.Mod_FrameDiff_KLT(cur, features=feats, maxval=255)
    H = det.klt.GetHomography()
    assert det.klt.last["source"] == 1 and abs(H[0, 2] + 3.0) < 0.1 and abs(H[1, 2]) < 0.1, H
    want = FR.FrameDiff().step(cur, prev, H.reshape(9), FR.INVERSE_MAP, 50, 255, feats)
    assert np.array_equal(mask, want["mask"]) and np.array_equal(det._pending, want["flags"])
    assert det._pending.tolist() == [1, 1, 1, 0, 0, 0, 0]
    keep, _ = det.motion_removal(feats)
    assert keep.tolist() == [0, 0, 0, 1, 1, 1, 1]
    det200 = mcd.MotionDetector(ctx=det.ctx)
    buf = prev.copy()                                                                # one buffer refilled per frame, as a camera's is
    det200.Mod_FrameDiff_KLT(buf, features=feats)
    buf[:] = cur
    m200 = det200.Mod_FrameDiff_KLT(buf, features=feats)                             # the reference's 200: QUIRK 2, nothing is removed
    assert np.array_equal(m200 == 200, mask == 255) and not det200._pending.any()


def test_mod_framediff_from_points():
    prev, cur = _block_frames()
    rng = np.random.default_rng(3)
    pb = np.stack([rng.uniform(10, 300, 40), rng.uniform(10, 230, 40)], 1).astype(np.float32)
    pa = pb + np.array([3, 0], np.float32)
    det = mcd.MotionDetector()
    assert det.Mod_FrameDiff(cur, prev, pa[:3], pb[:3]) is None                        # fewer than 4 points
    mask = det.Mod_FrameDiff(cur, prev, pa, pb, features=[(170, 100), (40, 40)], maxval=255)
    H = det.last_framediff["M"]
    want = FR.FrameDiff().step(cur, prev, det.homography.find_homography(pb, pa)["H"], 0, 50, 255, [(170, 100), (40, 40)])
    assert np.array_equal(H.view(np.uint64), want["M"].view(np.uint64)) and np.array_equal(mask, want["mask"]) and det._pending.tolist() == [1, 0]


def test_cpp_example(tmp_path):
    """dsdtm_amd/host/example_framediff.cpp linked and run: DSDTM::MotionDetector::Mod_FrameDiff on the device and with frame_diff_host, the
    same bytes; the block's features flagged at 255 and none at 200."""
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsdtm_amd", "host")
    exe = str(tmp_path / "example_framediff")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "example_framediff.cpp"), framediff.lib_path(),
                    mcd.lib_path(), motion.lib_path(), "-Wl,-rpath," + os.path.dirname(framediff.lib_path()), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "2 flagged" in r.stdout, (r.stdout, r.stderr)
