"""libdsdtm_amd_clahe.so on the MI355X: the equalised image AND the tables (lut_out and dsdtm_clahe_luts) byte-equal to the restatement
(dsdtm_amd/clahe_restatement.py) on every case of tests/clahe_cases.py, so that a failure says which kernel is wrong; one batch of all
cases over every memory kind byte-equal to its single calls; 64 frames at the smallest tile; Tracker.prefetch_equalized; the C++ adapter
and example. Every comparison is equality of bytes."""
import os
import subprocess

import numpy as np
import pytest

from dsdtm_amd import capi, clahe, tracking
from tests import clahe_cases as cc

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def cctx():
    ctx = clahe.ClaheContext(0)
    yield ctx
    ctx.close()


def _padded(h, w, extra):
    buf = np.full((h, w + extra), FILL, np.uint8)
    return buf, buf[:, :w]


@pytest.mark.parametrize("name", cc.NAMES)
def test_single_call_equals_the_restatement(cctx, name):
    """A pageable source with the case's stride into a padded host destination: tables (both ways) and image byte-equal, padding untouched."""
    c = cc.case(name)
    want, want_luts = cc.expected(name)
    h, w = c["img"].shape
    params = dict(clip_limit=c["clip_limit"], tiles_x=c["tiles_x"], tiles_y=c["tiles_y"])
    luts = cctx.luts(c["img"], **params)
    assert np.array_equal(luts, want_luts), ("dsdtm_clahe_luts", name, int((luts != want_luts).sum()))
    buf, dst = _padded(h, w, 7)
    lut_out = np.zeros_like(want_luts)
    cctx.apply(c["img"], dst, lut_out=lut_out, **params)
    assert np.array_equal(lut_out, want_luts), ("lut_out", name, int((lut_out != want_luts).sum()))
    assert np.array_equal(dst, want), ("image", name, int((dst != want).sum()))
    assert (buf[:, w:] == FILL).all()


def _in_memory(torch, img, kind, extra):
    """`img` in pageable (numpy), pinned or device memory (torch), rows `extra` bytes apart beyond the width"""
    h, w = img.shape
    if kind == "pageable":
        buf = np.full((h, w + extra), 0xEE, np.uint8)
        buf[:, :w] = img
        return buf[:, :w]
    t = torch.full((h, w + extra), 0xEE, dtype=torch.uint8)
    t[:, :w] = torch.from_numpy(np.array(img))
    t = t.pin_memory() if kind == "pinned" else t.cuda()
    return t[:, :w]


def _dst(torch, h, w, kind, extra):
    """(whole buffer, view of w columns) filled with the guard pattern"""
    if kind == "device":
        t = torch.full((h, w + extra), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t, t[:, :w]
    if kind == "pinned":
        t = torch.full((h, w + extra), FILL, dtype=torch.uint8).pin_memory()
        return t, t[:, :w]
    return _padded(h, w, extra)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def test_batch_of_all_cases_over_every_memory_kind(cctx):
    """All cases in ONE call, sources rotating through pageable / pinned / device memory and destinations through device / pageable /
    pinned, destination strides wider than the width with a guard pattern in the slack, tables asked for on every other frame: each
    frame byte-equal to the restatement (which the single calls equal too) and the slack untouched."""
    import torch
    kinds_src, kinds_dst = ("pageable", "pinned", "device"), ("device", "pageable", "pinned", "device")
    frames, held = [], []
    for k, name in enumerate(cc.NAMES):
        c = cc.case(name)
        h, w = c["img"].shape
        src = _in_memory(torch, c["img"], kinds_src[k % 3], 1 + k % 5)
        whole, dst = _dst(torch, h, w, kinds_dst[k % 4], 3 + k % 7)
        f = dict(src=src, dst=dst, clip_limit=c["clip_limit"], tiles_x=c["tiles_x"], tiles_y=c["tiles_y"])
        if k % 2 == 0:
            f["lut_out"] = np.zeros_like(cc.expected(name)[1])
        frames.append(f)
        held.append((name, whole, dst, f.get("lut_out")))
    torch.cuda.synchronize()
    cctx.apply_batch(frames)
    for name, whole, dst, lut_out in held:
        want, want_luts = cc.expected(name)
        w = want.shape[1]
        assert lut_out is None or np.array_equal(lut_out, want_luts), ("lut_out", name)
        assert np.array_equal(_np(dst), want), ("image", name, int((_np(dst) != want).sum()))
        assert (_np(whole)[:, w:] == FILL).all(), ("slack", name)


def test_batch_of_64_small_frames_equals_64_single_calls(cctx):
    """64 frames of 64 x 48 (tiles of 8 x 6, the smallest of the cases): 4096 (frame, tile) workgroups in one launch."""
    rng = np.random.default_rng(64)
    imgs = [np.clip(rng.normal(90 + k, 20 + k % 9, (48, 64)), 0, 255).astype(np.uint8) for k in range(64)]
    batch = [np.full((48, 64), FILL, np.uint8) for _ in imgs]
    cctx.apply_batch([dict(src=s, dst=d) for s, d in zip(imgs, batch)])
    singles = [cctx.apply(s) for s in imgs]
    assert all(np.array_equal(b, s) for b, s in zip(batch, singles))
    from dsdtm_amd import clahe_restatement as R
    for k in (0, 31, 63):
        assert np.array_equal(batch[k], R.clahe(imgs[k]))
    assert len({b.tobytes() for b in batch}) == 64


def test_refusals_on_the_device(cctx):
    """What the sanitizer driver cannot reach on the fake runtime, and that a refused batch writes nothing."""
    img = np.array(cc.case("64x48")["img"])
    good, bad = np.full((48, 64), FILL, np.uint8), np.full((48, 64), FILL, np.uint8)
    with pytest.raises(clahe.ClaheError) as e:
        cctx.apply_batch([dict(src=img, dst=good), dict(src=img, dst=bad, tiles_x=17)])
    assert e.value.status == clahe.ERR_INVALID and "desc 1" in e.value.message and "tiles_x" in e.value.message and (good == FILL).all()
    with pytest.raises(clahe.ClaheError) as e:
        cctx.apply(img, img)
    assert "overlaps" in e.value.message
    cctx.apply_batch([])


def test_prefetch_equalized(gpu_ctx):
    """Tracker.prefetch_equalized: the returned device tensor is the restatement's image, TrackFrame picks the prefetched frame up and
    returns the bytes a plain Tracker returns on the host-equalised image."""
    from dsdtm_amd import clahe_restatement as R
    from tests.test_undistort_gpu import _track_world
    cam, kfs, mps, last, raw = _track_world()
    want = R.clahe(raw)
    trk = tracking.Tracker(cam, gpu_ctx, max_level=5, min_level=0, max_iters=8)
    df, g = trk.prefetch_equalized(raw)
    assert np.array_equal(g.cpu().numpy(), want) and not np.array_equal(want, raw)
    cur, n, matches = trk.TrackFrame(raw, last, kfs, mps)
    assert trk._prefetched == [] and trk.last_result["frame"] is df
    cam2, kfs2, mps2, last2, _ = _track_world()
    plain = tracking.Tracker(cam2, gpu_ctx, max_level=5, min_level=0, max_iters=8)
    plain.prefetch(want)
    cur2, n2, matches2 = plain.TrackFrame(want, last2, kfs2, mps2)
    assert n == n2 and len(matches) == len(matches2)
    assert np.asarray(cur.Get_Pose()).tobytes() == np.asarray(cur2.Get_Pose()).tobytes()
    assert cur.px.tobytes() == cur2.px.tobytes() and cur.bearing.tobytes() == cur2.bearing.tobytes()
    trk.last_result["frame"].close(); plain.last_result["frame"].close()


def test_create_clahe_is_the_drivers_object():
    img = np.array(cc.case("752x480 real")["img"])
    out = clahe.createCLAHE(3.0, (8, 8)).apply(img)
    assert isinstance(out, np.ndarray) and np.array_equal(out, cc.expected("752x480 real")[0])
    import torch
    t = torch.from_numpy(img).cuda()
    out_t = clahe.createCLAHE(clipLimit=3.0, tileGridSize=(8, 8)).apply(t)
    assert out_t.is_cuda and np.array_equal(out_t.cpu().numpy(), out)


def test_cpp_adapter_and_example_on_the_device(tmp_path):
    """dsdtm_amd/host/example_clahe.cpp linked and run: DSDTM::CLAHE equalises a pageable frame into device memory (bit-equal to
    clahe_host), dsdtm_frame_prefetch reads it in place and dsdtm_detect_cells_frame detects on it."""
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsdtm_amd", "host")
    exe = str(tmp_path / "example_clahe")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "example_clahe.cpp"), clahe.lib_path(),
                    capi.lib_path(False), "-Wl,-rpath," + os.path.dirname(clahe.lib_path()), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "device == host" in r.stdout and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)
