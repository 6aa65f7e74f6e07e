"""dsdtm_need_keyframes without a GPU: the host side of the add-on library (dsdtm_amd/csrc/keyframe_api.cpp) — the context,
the argument checks, the packing of n trackers into one blob, the one upload / one launch / one read-back, every failure path — runs against the unmodified fake HIP runtime of
tests/fake_hip as a stand-alone program (its own main) under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer).
Scenarios: tests/fake_hip_keyframe/driver.cpp; the keyframe.hip launch is faked in tests/fake_hip_keyframe/fake_keyframe.cpp.
Nothing is loaded into Python and nothing is preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
HERE = os.path.join(ROOT, "tests", "fake_hip_keyframe")


def _build(tmp_path):
    exe = str(tmp_path / "driver_asan")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-pthread",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([os.environ.get("CXX", "g++"), *flags, "-I", FAKE, "-I", HERE, "-I", os.path.join(ROOT, "dsdtm_amd", "csrc"),
                    os.path.join(HERE, "driver.cpp"), os.path.join(HERE, "fake_keyframe.cpp"), os.path.join(FAKE, "fake_hip.cpp"),
                    os.path.join(ROOT, "dsdtm_amd", "csrc", "keyframe_api.cpp"), "-o", exe], check=True)
    return exe


def test_need_keyframes_host_side_under_address_and_ub_sanitizers(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok ", "FAILED "))]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert lines == ["ok keyframe_failures", "ok keyframe_limits", "ok rejected_in_the_middle"], lines
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr
