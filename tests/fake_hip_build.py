"""The stand-alone sanitizer programs over the fake HIP runtime of tests/fake_hip: how each is built and how each is run.

A program is a driver (its own main, scenarios printed as `ok <name>` / `FAILED <name>`), the fake's sources and the host sources of
dsdtm_amd/csrc under test (a list: the main library's host files, or an add-on's single one), compiled by g++ with AddressSanitizer +
UndefinedBehaviorSanitizer (+ LeakSanitizer) or with ThreadSanitizer. Nothing is loaded into Python and nothing is preloaded."""
import os
import subprocess

from dsdtm_amd.csrc import build as hip_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
CSRC = os.path.join(ROOT, "dsdtm_amd", "csrc")
# The host files of libdsdtm_amd.so that every `api` driver links: all of them (api.cpp, api_track.cpp) but the local-BA one, whose launches
# no driver fakes and whose entries no driver calls
API_SOURCES = [s for s in hip_build.SOURCES if s.endswith(".cpp") and s != "api_local_ba.cpp"]
COMMON_FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-pthread"]
SAN_FLAGS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
SAN_ENV = {"asan": {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"},
           "tsan": {"TSAN_OPTIONS": "halt_on_error=1"}}
SAN_REPORTS = {"asan": ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer"), "tsan": ("ThreadSanitizer",)}


def build_driver(out_dir, san, sources, api_sources, include_dirs=(), defines=()):
    """Compile `sources` (the driver and its own fakes), tests/fake_hip/fake_hip.cpp and every dsdtm_amd/csrc/<file> of `api_sources` into
    <out_dir>/driver_<san>; san: "asan" (address + undefined, no recovery from undefined) or "tsan". Returns the program's path."""
    exe = os.path.join(str(out_dir), f"driver_{san}")
    includes = [a for d in (FAKE, *include_dirs, CSRC) for a in ("-I", d)]
    subprocess.run([os.environ.get("CXX", "g++"), *COMMON_FLAGS, *["-D" + d for d in defines], *SAN_FLAGS[san], *includes, *sources,
                    os.path.join(FAKE, "fake_hip.cpp"), *[os.path.join(CSRC, s) for s in api_sources], "-o", exe], check=True)
    return exe


def run_driver(exe, san, scenarios=()):
    """Run the program (every scenario, or the named ones): it must exit with 0 and the sanitizer must have reported nothing.
    Returns (completed process, the `ok ` / `FAILED ` lines)."""
    r = subprocess.run([exe, *scenarios], capture_output=True, text=True, timeout=900, env=dict(os.environ, **SAN_ENV[san]))
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok ", "FAILED "))]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    for report in SAN_REPORTS[san]:
        assert report not in r.stderr, r.stderr[-4000:]
    return r, lines
