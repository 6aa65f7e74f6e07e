"""dsdtm_track_frames without a GPU: the entry is declared, exported and mirrored by the ctypes layer; and its host side — packing,
the slab of frames, the frame pool, every failure path — runs against the unmodified fake HIP runtime of tests/fake_hip under
AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer) and, with two contexts on two threads, under ThreadSanitizer
(scenarios: tests/fake_hip_batch/driver.cpp)."""
import os
import re
import subprocess

import pytest

from dsdtm_amd import capi
from tests import fake_hip_build as fhb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "fake_hip_batch", "driver.cpp")


def test_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    assert re.search(r"#define DSDTM_TRACK_FRAMES_MAX 1024\b", hdr)
    assert re.search(r"int dsdtm_track_frames\(dsdtm_ctx\* ctx, const dsdtm_camera\* cam, int n_frames, const dsdtm_track_desc\* descs,", hdr)
    assert "dsdtm_track_frames" in capi.EXPORTED_SYMBOLS
    lib = capi.load()
    assert hasattr(lib, "dsdtm_track_frames") and len(lib.dsdtm_track_frames.argtypes) == 8


def test_release_library_exports_the_entry_and_reads_no_environment():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT dsdtm_track_frames$", out, re.M)
    und = subprocess.run(["nm", "-D", "--undefined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bgetenv\b", und)


def _build(tmp_path, san):
    return fhb.build_driver(tmp_path, san, [DRIVER], fhb.API_SOURCES, defines=["DSDTM_DIAG=1"])


def test_batch_entry_under_address_and_ub_sanitizers(tmp_path):
    r, lines = fhb.run_driver(_build(tmp_path, "asan"), "asan")
    assert lines == ["ok batch_failures", "ok batch_image_arrivals", "ok two_contexts_two_threads"], lines


def test_two_contexts_running_batches_under_thread_sanitizer(tmp_path):
    r, lines = fhb.run_driver(_build(tmp_path, "tsan"), "tsan", ["two_contexts_two_threads"])
    assert "ok two_contexts_two_threads" in r.stdout
