"""dsdtm_track_frames on resident frames without a GPU: the capability adds no symbol (header, ctypes layer and release library
still carry exactly the set of symbols they carried before it), the ctypes binding fills the in/out frame handles, and the host
side of the resident mode — ownership of the frames on success and on every failure, the argument checks, no slab, the
device-side wait for pending prefetches, teardown — runs against the unmodified fake HIP runtime of tests/fake_hip as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer) and, with two contexts on two threads,
under ThreadSanitizer (scenarios: tests/fake_hip_frames_resident/driver.cpp; the rgbd.hip launches are the faked ones of
tests/fake_hip_prefetch)."""
import ctypes as C
import os
import re
import subprocess

from dsdtm_amd import capi
from tests import fake_hip_build as fhb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGBD = os.path.join(ROOT, "tests", "fake_hip_prefetch")
DRIVER = os.path.join(ROOT, "tests", "fake_hip_frames_resident", "driver.cpp")

# the C ABI before resident frames entered dsdtm_track_frames: they came in through an argument combination, not a symbol
SYMBOLS = {
    "dsdtm_align2d_batch", "dsdtm_align2d_batch_device", "dsdtm_create", "dsdtm_destroy", "dsdtm_detect_cells",
    "dsdtm_detect_cells_batch_device", "dsdtm_detect_cells_frame", "dsdtm_device_count", "dsdtm_frame_create",
    "dsdtm_frame_create_from_image", "dsdtm_frame_destroy", "dsdtm_frame_lift", "dsdtm_frame_prefetch", "dsdtm_frame_wait",
    "dsdtm_last_error", "dsdtm_local_ba", "dsdtm_local_ba_batch_device", "dsdtm_match_candidates_batch_device",
    "dsdtm_match_candidates_frames", "dsdtm_match_candidates_scratch_bytes", "dsdtm_pose_optimization",
    "dsdtm_pose_optimization_batch_device", "dsdtm_pyrdown", "dsdtm_pyrdown_batch_device", "dsdtm_reserve", "dsdtm_shard_range",
    "dsdtm_sparse_align", "dsdtm_sparse_align_batch_device", "dsdtm_sparse_align_batch_sharded", "dsdtm_sparse_align_batch_streamed",
    "dsdtm_sparse_align_check", "dsdtm_sparse_align_frames", "dsdtm_sparse_align_workspace_bytes", "dsdtm_track_frame",
    "dsdtm_track_frame_on", "dsdtm_track_frames", "dsdtm_version", "dsdtm_warp_patches"}


def test_no_symbol_was_added():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == SYMBOLS, declared ^ SYMBOLS
    assert set(capi.EXPORTED_SYMBOLS) == SYMBOLS and len(capi.EXPORTED_SYMBOLS) == len(SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (dsdtm_\w+)$", out, re.M)) == SYMBOLS


def test_header_describes_both_modes():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    block = hdr[hdr.index("n independent tracked frames in ONE submission"):hdr.index("#define DSDTM_TRACK_FRAMES_MAX")]
    assert "resident mode" in block and "image mode" in block and "IN/OUT" in block


class _FakeLib:
    def __init__(self):
        self.seen = None

    def dsdtm_track_frames(self, ctx, cam, n, descs, results, matches, rn, grid):
        self.seen = [(descs[f].image, results[f].frame) for f in range(n)]
        return capi.OK


class _FakeCtx:
    handle = C.c_void_p(1)

    def __init__(self):
        self.lib = _FakeLib()


class _FakeFrame:
    def __init__(self, h):
        self.handle = C.c_void_p(h)


def test_binding_fills_the_frame_handles_and_clears_the_images():
    ctx = _FakeCtx()
    descs, res = (capi.TrackDesc * 3)(), (capi.TrackResult * 3)()
    buf = (C.c_uint8 * 16)()
    for d in descs:
        d.image = C.addressof(buf)
    cam = capi.Camera(1, 1, 0, 0, 1, 4, 4)
    assert capi.track_frames(ctx, cam, 3, descs, res, None, None, None) == capi.OK
    assert [s[0] for s in ctx.lib.seen] == [C.addressof(buf)] * 3                        # image mode: passed through as it is
    frames = [_FakeFrame(0x1000), _FakeFrame(0x2000), _FakeFrame(0x3000)]
    assert capi.track_frames(ctx, cam, 3, descs, res, None, None, None, frames=frames) == capi.OK
    assert ctx.lib.seen == [(None, 0x1000), (None, 0x2000), (None, 0x3000)]
    try:
        capi.track_frames(ctx, cam, 3, descs, res, None, None, None, frames=frames[:2])
    except ValueError:
        pass
    else:
        raise AssertionError("two frames for three descriptors")


def _build(tmp_path, san):
    return fhb.build_driver(tmp_path, san, [DRIVER, os.path.join(RGBD, "fake_rgbd.cpp")], fhb.API_SOURCES, include_dirs=[RGBD])


def test_resident_mode_under_address_and_ub_sanitizers(tmp_path):
    r, lines = fhb.run_driver(_build(tmp_path, "asan"), "asan")
    assert lines == ["ok resident_call", "ok resident_failures", "ok resident_arguments", "ok destroy_with_resident_frames",
                     "ok two_contexts_two_threads"], lines


def test_two_contexts_in_lockstep_under_thread_sanitizer(tmp_path):
    r, lines = fhb.run_driver(_build(tmp_path, "tsan"), "tsan", ["two_contexts_two_threads"])
    assert "ok two_contexts_two_threads" in r.stdout
