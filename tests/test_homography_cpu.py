"""The RANSAC homography without a GPU: the numpy restatement (dsdtm_amd/homography_restatement.py) against its C twin
(tests/homography_restatement.c) bit for bit on every committed world, the worlds' truth as conditions, mutants of the restatement each
told apart by a committed world, the surface of libdsdtm_amd_homography.so, and the host side of the library under sanitizers
(tests/fake_hip_homography/driver.cpp, a stand-alone program against the fake HIP runtime of tests/fake_hip; nothing is loaded into
Python)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import capi, homography, motion
from dsdtm_amd import homography_restatement as R
from tests import fake_hip_build as fhb
from tests import homography_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NON_DEFAULT = [("B", dict(thr=1.0)), ("C", dict(max_hypotheses=256)), ("B", dict(seed=12345)), ("N", dict(thr=1.0, max_hypotheses=700, seed=9)),
               ("N", dict(confidence=0.5)), ("C", dict(max_hypotheses=4096))]


@pytest.mark.parametrize("name", hc.NAMES)
def test_numpy_and_c_restatements_are_bit_equal(tmp_path_factory, name):
    lib = hc.c_twin(tmp_path_factory.getbasetemp())
    wd = hc.world(name)
    assert hc.same(hc.run_c(lib, wd["A"], wd["B"]), hc.expected(name)), name


@pytest.mark.parametrize("name,params", NON_DEFAULT + [hc.MUTANTS[m] for m in (hc.StrictThreshold, hc.NoRedraw)])
def test_bit_equal_with_other_parameters(tmp_path_factory, name, params):
    lib = hc.c_twin(tmp_path_factory.getbasetemp())
    wd = hc.world(name)
    assert hc.same(hc.run_c(lib, wd["A"], wd["B"], **params), hc.expected(name, **params)), (name, params)


@pytest.mark.parametrize("name", hc.NAMES)
def test_worlds_are_what_they_claim(name):
    wd, e = hc.world(name), hc.expected(name)
    assert len(wd["A"]) == len(wd["B"]) == len(wd["truth"]) and wd["A"].dtype == np.float32
    assert wd["exact"] == (name in ("A", "B", "H"))
    hc.check_truth(name, wd, e)
    if wd["exact"]:      # the outliers lie at least 20 px off their transfer, so no share of the mask is excused
        off = np.hypot(*(hc.transfer(hc.H_TRUE, wd["A"]) - wd["B"].astype(np.float64)).T)
        assert (off[wd["truth"] == 0] >= 20.0 - 1e-3).all() and (off[wd["truth"] == 1] < 2.0).all()
        assert np.array_equal(e["mask"], wd["truth"])


def test_world_sizes_and_shapes():
    sizes = {n: len(hc.world(n)["A"]) for n in hc.NAMES}
    assert sizes["A"] == 60 and sizes["B"] == 200 and sizes["C"] == 120 and sizes["G"] == 4 and sizes["E"] == sizes["H"] == 5
    assert [sizes[n] for n in ("s64", "s65", "s256", "s257", "s2048")] == [64, 65, 256, 257, 2048]
    e = hc.world("E")
    assert np.array_equal(e["A"][3], e["A"][1]) and np.array_equal(e["B"][3], e["B"][1])
    d = hc.world("D")
    assert (d["A"][:, 1] == 2 * d["A"][:, 0] + 3).all()
    assert hc.expected("C")["rounds"] == 8 and hc.expected("C", max_hypotheses=4096)["rounds"] == 16
    assert hc.expected("C", max_hypotheses=257)["rounds"] == 2          # rounded UP to whole rounds
    f = hc.expected("F")                                                # two planes tie at 40: the lowest index wins
    tied = hc.TieToHighestIndex().find(hc.world("F")["A"], hc.world("F")["B"])
    assert f["n_inliers"] == tied["n_inliers"] == 40 and f["best_hypothesis"] < tied["best_hypothesis"]


def test_hash_and_sampling():
    # the hash by hand: plain Python integers
    def h(seed, k, c):
        x = (seed + k * 0x9E3779B9 + c * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    ks = np.array([0, 1, 255, 256, 4095], np.uint64)
    for c in (0, 7, 15):
        assert [int(v) for v in R.hash3(R.DEFAULT_SEED, ks, c)] == [h(R.DEFAULT_SEED, int(k), c) for k in ks]
    # a sample never repeats an index; with m = 5 most samples redraw, and 16 draws may not suffice
    s, ok = R.Ransac().samples(R.DEFAULT_SEED, np.arange(4096, dtype=np.uint64), 5)
    assert all(len(set(s[:, k])) == 4 for k in np.flatnonzero(ok)) and ok.sum() > 4000
    first4 = np.stack([(R.hash3(R.DEFAULT_SEED, np.arange(4096, dtype=np.uint64), c) * np.uint64(5)) >> np.uint64(32) for c in range(4)])
    assert (np.array([len(set(first4[:, k])) for k in range(4096)]) < 4).mean() > 0.5
    # hypothesis k is the same whichever round evaluates it
    s2, _ = R.Ransac().samples(R.DEFAULT_SEED, np.arange(256, 512, dtype=np.uint64), 5)
    assert np.array_equal(s2, s[:, 256:512])


@pytest.mark.parametrize("mutant", list(hc.MUTANTS), ids=lambda m: m.__name__)
def test_mutant_is_told_apart(mutant):
    assert hc.mutant_differs(mutant), (mutant.__name__, hc.MUTANTS[mutant])


def test_declared_and_exported():
    """libdsdtm_amd_homography.so exports exactly what its header declares and reads no environment; the other libraries are untouched."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_homography.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(homography.SYMBOLS) and len(homography.SYMBOLS) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", homography.lib_path()], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.strip()} == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", homography.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    for k, v in (("MAX_POINTS", 2048), ("MAX_PROBLEMS", 1024), ("MAX_HYPOTHESES", 4096), ("DEFAULT_HYPOTHESES", 2048)):
        assert re.search(r"#define DSDTM_HOMOGRAPHY_%s %d\b" % (k, v), hdr) and getattr(homography, k) == v
    assert re.search(r"#define DSDTM_HOMOGRAPHY_DEFAULT_SEED 0x%Xu" % R.DEFAULT_SEED, hdr) and homography.DEFAULT_SEED == R.DEFAULT_SEED
    assert "DSDTM_HOMOGRAPHY_DEFAULT_THRESHOLD 3.0" in hdr and "DSDTM_HOMOGRAPHY_DEFAULT_CONFIDENCE 0.995" in hdr
    assert (R.MAX_POINTS, R.MAX_HYPOTHESES_CAP, R.DEFAULT_MAX_HYPOTHESES) == (2048, 4096, 2048)
    main = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path(False)], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in main.splitlines() if l.strip()}
    assert len(names) == 38 and names == set(capi.EXPORTED_SYMBOLS) and not any("homograph" in n for n in names)
    mot = subprocess.run(["nm", "-D", "--defined-only", motion.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in mot.splitlines() if l.strip()}
    assert len(names) == 10 and names == set(motion.SYMBOLS)
    lib = homography.load()
    assert len(lib.dsdtm_find_homographies.argtypes) == 4 and len(lib.dsdtm_find_homography.argtypes) == 6


def test_desc_and_result_layout(tmp_path):
    """dsdtm_homography_desc / _result as a C compiler lays them out, against the ctypes mirrors."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_homography.h"', 'int main(void) {']
    for ctype, mirror in (("dsdtm_homography_desc", homography.Desc), ("dsdtm_homography_result", homography.Result)):
        src += [f'  printf("%zu", sizeof({ctype}));'] + [f'  printf(" %zu", offsetof({ctype}, {f[0]}));' for f in mirror._fields_] + ['  printf("\\n");']
    src += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, mirror in zip(lines, (homography.Desc, homography.Result)):
        assert [int(v) for v in line.split()] == [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]


def test_header_documents_the_parity_and_the_definitions():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_homography.h")).read()
    for needle in ("src/Moving_Detection.cpp:28", ":47", "KLTWrapper.cpp:180", "OpenCV is not available to this project, in source or binary",
                   "neither cv::findHomography's random sequence nor its", "final refinement can be restated faithfully", "findContours",
                   "4-point samples", "forward reprojection error against 3 px", "confidence 0.995", "about 2000 hypotheses at most",
                   "a refit on the inliers of the best model", "the mask of the RANSAC model returned", "THIS PROJECT'S DEFINITION",
                   "which samples are drawn, how ties fall, when the loop stops and how the refit iterates",
                   "Parity with OpenCV is unpinned and stays unpinned", "TIES GO TO THE LOWEST HYPOTHESIS INDEX",
                   "NOT RE-EVALUATED AFTER THE REFIT", "m <= 4: found = 0", "H maps A to B", "EMPTY matrix", "dereferences unchecked"):
        assert needle in hdr, needle


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_homography")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_homography.cpp")],
                           ["homography_api.cpp"], include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok call_failures", "ok batch_rules", "ok argument_checks", "ok create_failures"], lines
