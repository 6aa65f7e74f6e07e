"""dsdtm_frame_prefetch / _wait / dsdtm_track_frame_on / dsdtm_frame_lift without a GPU: the entries are declared, exported and
mirrored by the ctypes layer; and their host side — the staging ring, the frame pool with pending buffers, every failure path,
teardown with a prefetch pending — runs against the unmodified fake HIP runtime of tests/fake_hip as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer) and, with two contexts on two threads, under ThreadSanitizer
(scenarios: tests/fake_hip_prefetch/driver.cpp; the two rgbd.hip launches are faked in tests/fake_hip_prefetch/fake_rgbd.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dsdtm_amd import capi, tum
from tests import fake_hip_build as fhb
from tests import rgbd_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "fake_hip_prefetch")
NEW = ["dsdtm_frame_prefetch", "dsdtm_frame_wait", "dsdtm_track_frame_on", "dsdtm_frame_lift"]


def test_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    assert re.search(r"#define DSDTM_LIFT_MAX 16384\b", hdr) and capi.LIFT_MAX == 16384
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    lib = capi.load()
    for sym in NEW:
        assert re.search(r"\bint %s\(dsdtm_ctx\*" % sym, hdr), sym
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
        assert re.search(r"\bT %s$" % sym, out, re.M), sym
    assert len(lib.dsdtm_frame_prefetch.argtypes) == 3 and len(lib.dsdtm_track_frame_on.argtypes) == 7
    assert len(lib.dsdtm_frame_lift.argtypes) == 8 and len(capi.EXPORTED_SYMBOLS) == 38


def test_frame_image_layout_matches_the_compiled_header(tmp_path):
    fields = ["gray", "width", "height", "stride", "levels", "depth", "depth_stride", "depth_scale"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd.h"', 'int main(void) {',
           '  printf("%zu", sizeof(dsdtm_frame_image));']
    src += [f'  printf(" %zu", offsetof(dsdtm_frame_image, {f}));' for f in fields]
    src += ['  printf(" %zu\\n", sizeof(dsdtm_track_desc));', '  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(tmp_path / "layout.c")], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.FrameImage)] + [getattr(capi.FrameImage, f).offset for f in fields] + [C.sizeof(capi.TrackDesc)]


def test_lift_restatement_on_a_hand_made_case():
    """tests/rgbd_restatement.py against values worked out by hand: identity rotation, t = (1, 2, 3): p_w = p_c - t."""
    class Cam:
        fx, fy, cx, cy = 2.0, 4.0, 1.0, 1.0
    plane = tum.depth_to_metres(np.array([[0, 0, 0], [0, 0, 10000], [0, 0, 0]], np.uint16), 5000.0)
    T = np.array([[1.0, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]])
    d, p = R.lift(plane, Cam, T, np.array([[1.4, 0.6], [0.0, 0.0], [2.5, 1.0]], np.float32))
    assert d[0] == 2.0 and d[1] == -1.0 and d[2] == 2.0           # the right-hand neighbour of (1, 1); nothing; cvRound(2.5) = 2
    x = np.float32(np.float32(2.0) * np.float32(np.float32(1.4) - np.float32(1.0))) / np.float32(2.0)
    assert np.array_equal(p[0], [np.float64(x) - 1.0, np.float64(np.float32(2.0 * (np.float32(0.6) - np.float32(1.0))) / np.float32(4.0)) - 2.0, -1.0])
    assert np.all(p[1] == 0)


def _build(tmp_path, san):
    return fhb.build_driver(tmp_path, san, [os.path.join(HERE, "driver.cpp"), os.path.join(HERE, "fake_rgbd.cpp")], fhb.API_SOURCES, include_dirs=[HERE])


def test_prefetch_path_under_address_and_ub_sanitizers(tmp_path):
    r, lines = fhb.run_driver(_build(tmp_path, "asan"), "asan")
    assert lines == ["ok prefetch_failures", "ok ring_slot_reuse", "ok pooled_pending_buffer", "ok destroy_with_a_prefetch_pending",
                     "ok prefetch_then_track", "ok two_contexts_two_threads"], lines


def test_two_contexts_prefetching_under_thread_sanitizer(tmp_path):
    r, lines = fhb.run_driver(_build(tmp_path, "tsan"), "tsan", ["two_contexts_two_threads"])
    assert "ok two_contexts_two_threads" in r.stdout
