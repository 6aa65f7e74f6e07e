"""dsdtm_track_frames without a GPU: the entry is declared, exported and mirrored by the ctypes layer; and its host side — packing,
the slab of frames, the frame pool, every failure path — runs against the unmodified fake HIP runtime of tests/fake_hip under
AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer) and, with two contexts on two threads, under ThreadSanitizer
(scenarios: tests/fake_hip_batch/driver.cpp)."""
import os
import re
import subprocess

import pytest

from dsdtm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
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
    exe = str(tmp_path / f"driver_{san}")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DDSDTM_DIAG=1", "-Wall", "-Wno-unused-function", "-pthread"]
    flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san == "asan" else ["-fsanitize=thread"]
    subprocess.run([os.environ.get("CXX", "g++"), *flags, "-I", FAKE, "-I", os.path.join(ROOT, "dsdtm_amd", "csrc"), DRIVER,
                    os.path.join(FAKE, "fake_hip.cpp"), os.path.join(ROOT, "dsdtm_amd", "csrc", "api.cpp"), "-o", exe], check=True)
    return exe


def test_batch_entry_under_address_and_ub_sanitizers(tmp_path):
    exe = _build(tmp_path, "asan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok ", "FAILED "))]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert lines == ["ok batch_failures", "ok batch_image_arrivals", "ok two_contexts_two_threads"], lines
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr


def test_two_contexts_running_batches_under_thread_sanitizer(tmp_path):
    exe = _build(tmp_path, "tsan")
    r = subprocess.run([exe, "two_contexts_two_threads"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ok two_contexts_two_threads" in r.stdout and "ThreadSanitizer" not in r.stderr
