"""Rarsac_base::RejectFundamental without a GPU: the restatement (dsdtm_amd/rarsac_restatement.py, rules R1-R9 of
include/dsdtm_amd_rarsac.h) against its C twin (tests/rarsac_restatement.c) and the host function (dsdtm_amd/host/dsdtm_rarsac_host.hpp)
bit for bit on every world of tests/rarsac_cases.py, the worlds' truth as conditions, mutants of the restatement each told apart by a
world, the surface of libdsdtm_amd_rarsac.so, and the host side of the library under sanitizers (tests/fake_hip_rarsac/driver.cpp, a
stand-alone program against the fake HIP runtime of tests/fake_hip; nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import rarsac
from dsdtm_amd import rarsac_restatement as R
from dsdtm_amd.csrc import build as hip_build
from tests import fake_hip_build as fhb
from tests import rarsac_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def natives(tmp_path_factory):
    d = tmp_path_factory.mktemp("rarsac")
    return rc.c_twin(d), rc.host_library(d)


@pytest.mark.parametrize("name", rc.NAMES)
def test_restatement_twin_and_host_function_are_bit_equal(natives, name):
    """status, F, grid, score, best_hypothesis, iterations_run (and n_inliers). m = 2048: the twin against the host function, and the
    restatement on the hypotheses up to the first win (the whole run costs the restatement too long)."""
    twin, host = natives
    c = rc.world(name)
    t, h = rc.run_native(twin, c), rc.run_native(host, c)
    assert rc.same(t, h), (name, rc.differences(t, h))
    if name == "m2048":
        short = rc.restate(c, max_iterations=40)
        assert rc.same(short, rc.run_native(twin, c, max_iterations=40)) and short["best_hypothesis"] >= 0
        return
    e = rc.expected(name)
    assert rc.same(t, e), (name, rc.differences(t, e))


def test_worlds_are_what_they_claim():
    assert [len(rc.world(n)["cur"]) for n in ("m8", "m8 in 7 bins", "clean300", "outliers300", "m2048", "coincident")] == [8, 8, 300, 300, 2048, 8]
    bins = lambda c: {R.bin_of(x, y, c["height"] // 10, c["width"] // 10) for x, y in c["cur"]}
    assert len(bins(rc.world("m8"))) == 8 and len(bins(rc.world("m8 in 7 bins"))) == 7 and len(bins(rc.world("coincident"))) == 8
    assert rc.expected("m8 in 7 bins") == dict(found=0)
    e = rc.expected("clean300")
    assert e["iterations_run"] < R.ROUND and e["best_hypothesis"] >= 0          # stops in the first round
    for n in (1, 255, 256, 257, 1000):                                          # never stops early: the round edges
        assert rc.expected("noise64 x%d" % n)["iterations_run"] == n
    assert rc.expected("stop at 255")["iterations_run"] == 256 and rc.expected("stop at 256")["iterations_run"] == 257
    for name in ("coincident", "collinear"):                                    # R4 refuses every hypothesis
        e = rc.expected(name)
        assert e["found"] == 1 and e["best_hypothesis"] == -1 and e["iterations_run"] == 300 and not e["status"].any() and e["score"] == R.DBL_MIN
        assert not e["F"].any() and np.array_equal(e["grid"], np.full(100, 0.5))
    assert (rc.world("coincident")["prev"] == rc.world("coincident")["prev"][0]).all()
    assert not rc.same(rc.expected("peaked prior"), rc.expected("outliers300"))          # R3's weights change what is drawn
    w = rc.world("480x640")
    assert (w["width"], w["height"]) == (480, 640) and R.bin_of(100.0, 500.0, 64, 48) == -1 and R.bin_of(100.0, 479.0, 64, 48) == 91


def test_forty_percent_outliers_are_rejected():
    """At least 90 % of the true inliers kept, at most 10 % of the planted outliers: the restatement alone, then the others by equality."""
    for name in ("outliers300", "peaked prior"):
        c, e = rc.world(name), rc.expected(name)
        assert (c["truth"] == 0).sum() == 120
        kept, passed = e["status"][c["truth"] == 1].mean(), e["status"][c["truth"] == 0].mean()
        print(f"[rarsac] {name}: {kept:.3f} of the inliers kept, {passed:.3f} of the outliers passed")
        assert kept >= 0.9 and passed <= 0.1, (name, kept, passed)


def test_quirk_first_valid_hypothesis_that_does_not_win_stops_the_run():
    """R8: q is 0 before the first win. A world whose every score is NaN (F of all NaN cannot come out of R4, so: a mutant whose wins()
    is never true) stops at its first valid hypothesis with best_hypothesis = -1."""
    class NeverWins(R.Rarsac):
        def wins(self, score, best):
            return False
    c = rc.world("clean300")
    e = NeverWins(c["cur"], c["prev"]).reject()
    assert e["found"] == 1 and e["best_hypothesis"] == -1 and e["iterations_run"] == 1 and not e["status"].any() and e["score"] == R.DBL_MIN


def test_hash_and_sampling():
    def h(seed, k, c):
        x = (seed + k * 0x9E3779B9 + c * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    assert all(R.hash3(R.DEFAULT_SEED, k, c) == h(R.DEFAULT_SEED, k, c) for k in (0, 1, 255, 256, 4095) for c in (0, 7, 63, 71))
    c = rc.world("outliers300")
    r = R.Rarsac(c["cur"], c["prev"])
    for k in range(0, 600, 7):
        at = r.draw_sample(k)
        assert at is not None
        b = [int(np.searchsorted(r.start, a, side="right")) - 1 for a in at]
        assert len(set(b)) == 8 and all(r.a[x] > 0 for x in b)
    # the peaked prior draws its bin far more often: weight 1024 against 204
    flat, peak = R.Rarsac(c["cur"], c["prev"]), R.Rarsac(c["cur"], c["prev"], prior=rc.PEAK)
    assert peak.weight(1.0) == 1024 and peak.weight(0.2) == 204 and peak.weight(0.0) == 1
    hit = lambda r: sum(34 in [int(np.searchsorted(r.start, a, side="right")) - 1 for a in r.draw_sample(k)] for k in range(300))
    assert r.a[34] > 0 and hit(peak) > 2 * hit(flat)


class StrictNaNRejects(R.Rarsac):
    def rejects(self, chi, th):
        return ~(chi <= th)


class FloorAtZero(R.Rarsac):
    def floor(self):
        return 0.0


class NoPivotFloor(R.Rarsac):
    def pivot_floor(self):
        return 0.0


class UnweightedBins(R.Rarsac):
    def weight(self, prior):
        return 1


MUTANTS = {FloorAtZero: "outliers300", NoPivotFloor: "collinear", UnweightedBins: "peaked prior"}


@pytest.mark.parametrize("mutant", list(MUTANTS), ids=lambda m: m.__name__)
def test_mutant_is_told_apart(mutant):
    c = rc.world(MUTANTS[mutant])
    got = R.reject_fundamental(c["cur"], c["prev"], c["width"], c["height"], c["params"].get("prior"), c["params"].get("max_iterations", 0), cls=mutant)
    assert not rc.same(got, rc.expected(MUTANTS[mutant])), mutant.__name__


def test_check_is_the_stateless_check_fundamental(natives):
    twin, host = natives
    for name in ("outliers300", "480x640"):
        c, e = rc.world(name), rc.expected(name)
        k = R.check_fundamental(c["cur"], c["prev"], e["F"], c["width"], c["height"])
        assert np.array_equal(k["status"], e["status"]) and np.array_equal(k["grid"].view(np.uint64), e["grid"].view(np.uint64)) and k["score"] == e["score"]
        assert rc.same(rc.run_native_check(twin, c, e["F"]), k) and rc.same(rc.run_native_check(host, c, e["F"]), k)
    # a NaN distance does not reject (chiSquare > th as written): F = 0 makes every distance 0 / 0
    c = rc.world("m8")
    assert R.check_fundamental(c["cur"], c["prev"], np.zeros(9))["status"].all()
    assert not StrictNaNRejects(c["cur"], c["prev"]).check_fundamental(np.zeros(9))["status"].any()


def test_r1_refusals(natives):
    twin, host = natives
    w = rc.world("480x640")
    for bad, index in (((100.0, 500.0), 41), ((np.nan, 5.0), 3), ((5.0, np.inf), 0), ((3e30, 5.0), 119)):
        cur = w["cur"].copy()
        cur[index] = bad
        for run in (lambda c: rc.restate(c), lambda c: rc.run_native(twin, c), lambda c: rc.run_native(host, c)):
            with pytest.raises(R.Refused) as e:
                run(dict(w, cur=cur))
            assert e.value.index == index


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_rarsac")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_rarsac.cpp")], ["rarsac_api.cpp"], include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    assert [l for l in lines if not l.startswith("ok refusal: ")] == ["ok call_failures", "ok batch_rules", "ok refusals", "ok create_failures"], lines
    refusals = {l[len("ok refusal: "):] for l in lines if l.startswith("ok refusal: ")}
    for needle in ("m out of range", "cur is NULL", "prev is NULL", "width out of range", "height out of range", "sigma", "cur is not finite at index 100",
                   "prev is not finite at index 64", "cur lies outside the 10x10 grid (R1) at index 17", "F is NULL", "F is not finite at entry 4",
                   "max_iterations out of range", "terminate_threshold", "grid_probability_in outside 0..1 at bin 33", "grid_probability_in sums to 0"):
        assert needle in refusals, (needle, refusals)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_and_exported():
    """libdsdtm_amd_rarsac.so exports exactly the symbols its header declares and reads no environment; the row stands in MORE_ADDONS."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_rarsac.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(rarsac.SYMBOLS) == {"dsdtm_rarsac_create", "dsdtm_rarsac_destroy", "dsdtm_rarsac_last_error", "dsdtm_rarsac_reject_batch",
                                               "dsdtm_rarsac_reject", "dsdtm_rarsac_check"}
    assert _exported(rarsac.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", rarsac.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    assert "rarsac" in hip_build.MORE_ADDONS and "rarsac" not in hip_build.ADDONS
    assert hip_build.MORE_ADDONS["rarsac"][0] == ["rarsac_api.cpp", "rarsac.hip"]
    assert not {"rarsac.hip", "rarsac.h", "rarsac_api.cpp"} & set(hip_build.SOURCES + hip_build.HEADERS)
    for k, v in (("GRID", 100), ("MIN_POINTS", 8), ("MAX_POINTS", 2048), ("MAX_PROBLEMS", 1024), ("MAX_ITERATIONS", 16384), ("DEFAULT_ITERATIONS", 1000)):
        assert re.search(r"#define DSDTM_RARSAC_%s %d\b" % (k, v), hdr) and getattr(rarsac, k) == v and getattr(R, k, v) == v
    assert re.search(r"#define DSDTM_RARSAC_DEFAULT_SEED 0x%Xu" % R.DEFAULT_SEED, hdr) and rarsac.DEFAULT_SEED == R.DEFAULT_SEED
    assert "DSDTM_RARSAC_DEFAULT_TERMINATE 0.001" in hdr and "DSDTM_RARSAC_DEFAULT_SIGMA 0.5" in hdr


def test_desc_and_result_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_rarsac.h"', 'int main(void) {']
    for ctype, mirror in (("dsdtm_rarsac_desc", rarsac.Desc), ("dsdtm_rarsac_result", rarsac.Result)):
        src += [f'  printf("%zu", sizeof({ctype}));'] + [f'  printf(" %zu", offsetof({ctype}, {f[0]}));' for f in mirror._fields_] + ['  printf("\\n");']
    src += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, mirror in zip(lines, (rarsac.Desc, rarsac.Result)):
        assert [int(v) for v in line.split()] == [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]


def test_header_documents_the_rules_the_quirk_and_the_parity():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_rarsac.h")).read()
    for needle in ("src/Rarsac_base.cpp", "include/Tracking.h:127", "Test/test_Optimizer.cpp:91-106", "cv::SVDecomp and std::random_shuffle cannot be restated",
                   "THIS PROJECT'S DEFINITION", "unpinned and stays unpinned", "SWAPPED DIVISORS", "src/Camera.cpp:70-78", "COMPLETE PIVOTING", "QUIRK",
                   "a NaN distance", "DBL_MIN", *["R%d " % i for i in range(1, 10)]):
        assert needle in hdr, needle


def test_example_and_adapter_build(tmp_path):
    """dsdtm_amd/host/dsdtm_rarsac_host.hpp's Rarsac_base on the host path: the status vector and the grid written back."""
    src = tmp_path / "adapter.cpp"
    src.write_text('#include "dsdtm_rarsac_host.hpp"\n#include <cstdio>\nint main() {\n  std::vector<DSDTM::RarsacPoint2f> a, b;\n'
                   '  for (int i = 0; i < 120; ++i) { float x = 10.f + (i * 97 % 600), y = 10.f + (i * 131 % 440); a.push_back({x, y}); b.push_back({x + 2.f + 0.01f * (i % 7), y + 1.f}); }\n'
                   '  std::vector<double> grid(100, 0.5);\n  DSDTM::Rarsac_base r(grid, a, b, 640, 480, false);\n  std::vector<uint8_t> st = r.RejectFundamental();\n'
                   '  std::vector<DSDTM::RarsacPoint2f> kept = a; DSDTM::ReduceFeatures(kept, st);\n'
                   '  std::printf("%zu %d %d %zu %d\\n", st.size(), r.result.found, r.result.best_hypothesis >= 0 ? 1 : 0, kept.size(), grid[0] != 0.5 || grid[11] != 0.5 ? 1 : 0);\n  return 0;\n}\n')
    exe = tmp_path / "adapter"
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-DDSDTM_RARSAC_HOST_ONLY=1", "-I", os.path.join(ROOT, "dsdtm_amd", "host"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "120" and out[1] == "1" and int(out[3]) <= 120
    if out[2] == "1":          # a hypothesis won: the frame's grid was written back
        assert out[4] == "1"
