"""Moving_Detecter::Mod_FrameDiff without a GPU: the restatement dsdtm_amd/framediff_restatement.py (rules F1-F8 of
include/dsdtm_amd_framediff.h) against hand-derived answers, frame_diff_host (dsdtm_amd/host/dsdtm_framediff_host.hpp) against it bit
for bit on every world of tests/framediff_cases.py and at every stage, the library's host side over the fake HIP runtime under
ASan / UBSan, the mutants of the restatement each told apart by a named case, and the surface of libdsdtm_amd_framediff.so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import framediff
from dsdtm_amd import framediff_restatement as FR
from dsdtm_amd.csrc import build as hip_build
from tests import framediff_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = FR.FrameDiff()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cases.host_library(tmp_path_factory.mktemp("framediff"))


# ---- hand cases: answers that need no implementation -----------------------------------------------------------------------------------

def _drawn_f(w, h, rects):
    a, b = cases.drawn(w, h, rects)
    return F.step(a, b, cases.IDENTITY)


def test_hand_interior_blocks():
    """F6's consequences: a 4x4 block vanishes, a 5x5 block comes out 9x9 (its eroded centre pixel dilated twice), a 6x6 block 10x10."""
    r = _drawn_f(200, 80, [(10, 10, 14, 14)])
    assert r["t"].sum() == 16 and not r["e"].any() and not r["f"].any() and r["n_foreground"] == 0
    r = _drawn_f(200, 80, [(40, 8, 45, 13)])
    want = np.zeros((80, 200), bool)
    want[6:15, 38:47] = True
    assert r["e"].sum() == 1 and r["e"][10, 42] and r["o"].sum() == 25 and np.array_equal(r["f"], want) and r["n_foreground"] == 81
    r = _drawn_f(200, 80, [(70, 8, 76, 14)])
    assert r["e"].sum() == 4 and r["f"].sum() == 100
    assert set(np.unique(r["mask"])) == {0, 200}


def test_hand_edge_strips_survive_and_come_out_5_wide():
    """A 3-wide strip along an edge survives the erosion at the edge column only (the window's outside part takes no part) and comes
    out 5 wide: 1 + 2 + 2."""
    for w, h in cases.SIZES[1:]:
        r = _drawn_f(w, h, [(0, 8, 3, h - 8)])
        assert r["e"][:, 0].sum() == h - 16 - 4 and not r["e"][:, 1:].any()
        assert r["f"][:, :5].any(axis=0).all() and not r["f"][:, 5:].any()
        r = _drawn_f(w, h, [(w - 3, 8, w, h - 8)])
        assert r["e"][:, w - 1].sum() == h - 20 and not r["e"][:, :w - 1].any() and r["f"][:, w - 5:].any(axis=0).all() and not r["f"][:, :w - 5].any()
        r = _drawn_f(w, h, [(8, 0, w - 8, 3)])
        assert r["e"][0].sum() == w - 20 and not r["e"][1:].any() and r["f"][:5].any(axis=1).all() and not r["f"][5:].any()
        r = _drawn_f(w, h, [(8, h - 3, w - 8, h)])
        assert r["e"][h - 1].sum() == w - 20 and not r["e"][:h - 1].any() and r["f"][h - 5:].any(axis=1).all() and not r["f"][:h - 5].any()


def test_hand_corner_blocks_come_out_5x5():
    r = _drawn_f(70, 37, cases.edge_rects(70, 37)[1])
    want = np.zeros((37, 70), bool)
    want[:5, :5] = want[:5, -5:] = want[-5:, :5] = want[-5:, -5:] = True
    assert r["e"].sum() == 4 and np.array_equal(r["f"], want)


def test_hand_one_pixel_translation():
    """H = a shift by (1, 0): warped(x, y) = b(x - 1, y), the first column reads outside: 0. Both directions of F1."""
    b = cases.texture(70, 37, 2)
    want = np.zeros_like(b)
    want[:, 1:] = b[:, :-1]
    w1, M = F.warp(b, cases.translation(1, 0))
    assert np.array_equal(w1, want) and M.tolist() == [1, 0, -1, 0, 1, 0, 0, 0, 1]
    w2, M2 = F.warp(b, cases.translation(-1, 0), FR.INVERSE_MAP)
    assert np.array_equal(w2, want) and M2.tolist() == [1, 0, -1, 0, 1, 0, 0, 0, 1]
    assert np.array_equal(F.warp(b, cases.IDENTITY)[0], b)
    half, _ = F.warp(b, cases.translation(-0.5, 0))          # X = 32 x + 16: the mean of two neighbours, + 512 >> 10
    assert np.array_equal(half[:, :-1], ((b[:, :-1].astype(int) + b[:, 1:].astype(int)) * 512 + 512) >> 10)


def test_hand_inverse_times_h_is_the_identity():
    for H in (cases.ROTATION, cases.PERSPECTIVE, cases.translation(37 / 32, -13 / 32), np.array([2, 1, 3, -1, 4, 5, 0.001, 0.002, 1.0])):
        M = FR.invert(H)
        assert np.abs(M.reshape(3, 3) @ H.reshape(3, 3) - np.eye(3)).max() <= 1e-12
    for bad in (np.arange(1.0, 10.0), np.zeros(9), [1, 0, 0, 0, 1, 0, 0, 0, np.nan], [1e-300, 0, 0, 0, 1e-300, 0, 0, 0, 1]):
        with pytest.raises(ValueError):
            FR.invert(bad)


def test_hand_threshold_is_strict_and_the_quirk_of_200():
    lo, hi = cases.restated("threshold 50 and 51 maxval 200"), cases.restated("threshold 50 and 51 maxval 255")
    want = np.zeros((37, 70), bool)
    want[8:16, 17:25] = True                                  # d = 51 only; the block with d = 50 is not there
    assert np.array_equal(lo["t"], want) and np.array_equal(hi["t"], want)
    f = np.zeros((37, 70), bool)
    f[6:18, 15:27] = True
    assert np.array_equal(lo["f"], f) and set(np.unique(lo["mask"])) == {0, 200} and set(np.unique(hi["mask"])) == {0, 255}
    # features: 26.5 -> 26 (on), 27.5 -> 28, 14.5 -> 14, 13.5 -> 14 (off: f starts at 15), y 17.5 -> 18 (off), 16.5 -> 16 (on), 5.5 -> 6 (on)
    assert hi["flags"].tolist() == [1, 0, 0, 0, 0, 1, 1, 0, 0, 0] and hi["n_flagged"] == 3
    assert not lo["flags"].any() and lo["n_flagged"] == 0 and lo["n_foreground"] == hi["n_foreground"] == 144      # QUIRK 2: no flag at 200
    c = cases.by_name("threshold 50 and 51 maxval 255")
    for bad in ([(69.5, 10)], [(10, 37)], [(-0.6, 3)], [(np.nan, 3)]):
        with pytest.raises(ValueError):
            F.step(c["a"], c["b"], c["H"], features=bad)


def test_hand_map_saturates_and_nan_is_outside():
    X, Y = F.map(cases.HUGE.copy(), 70, 37)                   # as M: x + 1e300 and y - 1e300
    assert (X == 2 ** 31 - 1).all() and (Y == -2 ** 31).all()
    X, Y = F.map(cases.NAN_M, 70, 37)
    assert X[5, 20] == FR.OUTSIDE and X[5, 0] == 0 and X[5, 19] == -2 ** 31 and X[5, 21] == 2 ** 31 - 1 and Y[5, 20] == 0
    for name in ("everything outside 70x37 direct", "entries of 1e300 70x37 direct", "entries of 1e300 129x45 inverse"):
        r, c = cases.restated(name), cases.by_name(name)
        assert not r["warped"].any() and np.array_equal(r["t"], c["a"] > c["threshold"])
    for name in cases.names():                                # the perspective worlds' W changes sign inside the image, direct AND inverse
        if name.startswith("perspective"):
            M, (h, w) = cases.restated(name)["M"], cases.by_name(name)["a"].shape
            ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
            W = (M[6] * xs + M[7] * ys) + M[8]
            assert W.min() < -0.5 and W.max() > 0.5, (name, W.min(), W.max())
    assert sum(n.startswith("perspective") for n in cases.names()) == 4


# ---- the host function, on every case and every stage -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.names())
def test_host_function_is_the_restatement(host, name):
    c, want = cases.by_name(name), cases.restated(name)
    got = cases.host_step(host, c)
    assert got is not None
    for s in cases.STAGES:
        assert np.array_equal(got[s], want[s]), s
    assert cases.same_answer(got, want)


def test_host_warp_and_refusals(host):
    c = cases.by_name("rotation with scale 129x45 direct")
    out, M = np.full((45, 133), 0xA5, np.uint8), np.zeros(9)
    b = np.ascontiguousarray(c["b"])
    assert host.warp_perspective_host_c(b.ctypes.data, b.strides[0], 129, 45, c["H"].ctypes.data, 0, out.ctypes.data, 133, M.ctypes.data) == 1
    want = cases.restated(c["name"])
    assert np.array_equal(out[:, :129], want["warped"]) and (out[:, 129:] == 0xA5).all() and np.array_equal(M.view(np.uint64), want["M"].view(np.uint64))
    for bad in (np.arange(1.0, 10.0), np.array([1, 0, 0, 0, 1, 0, 0, 0, np.inf])):
        assert cases.host_step(host, dict(c, H=bad)) is None
    assert cases.host_step(host, dict(c, H=cases.NAN_M, flags=0)) is None          # its determinant overflows


def test_cases_cover_what_they_claim():
    names = cases.names()
    assert len(names) == len(set(names))
    assert {c["a"].shape[::-1] for c in cases.all_cases()} >= {(64, 16), (70, 37), (129, 45), (127, 20), (200, 80), (640, 480)}
    assert sorted({c["a"].shape[1] % 64 for c in cases.all_cases() if c["name"].startswith("ragged")}) == [1, 6, 63]
    for name in names:
        if name.startswith("ragged"):
            r = cases.restated(name)
            assert r["t"][:, -1].any() and r["f"][:, -1].any()
    for name, seams in (("band seams", (16, 32, 48, 64)),):
        f = cases.restated(name)["f"]
        assert all(f[s - 1].any() and f[s].any() for s in seams)          # a blob on either side of every seam of 16- and 32-row bands
    f = cases.restated("word seams")["f"]
    assert f[:, 63].any() and f[:, 64].any() and f[:, 127].any() and f[:, 128].any()
    assert cases.by_name("literal line 45")["a"] is cases.by_name("literal line 45")["b"]
    assert any(cases.restated(n)["n_foreground"] > 0 for n in names if n.startswith("rotation"))
    assert cases.restated("640x480")["n_flagged"] > 0 and cases.restated("nan in the map 70x37 inverse")["n_foreground"] >= 0


# ---- mutants: each a one-line variant of the restatement, each told apart by at least one case -------------------------------------------

class ErodeOutsideIsZero(FR.FrameDiff):
    ERODE_OUTSIDE = 0


class DilateOutsideIsOne(FR.FrameDiff):
    DILATE_OUTSIDE = 1


class ThresholdNotStrict(FR.FrameDiff):
    def exceeds(self, d, threshold):
        return d >= threshold


class HalvesUp(FR.FrameDiff):
    def round(self, v):
        return np.floor(v + 0.5)


class Uninverted(FR.FrameDiff):
    def matrix(self, H, flags):
        return np.asarray(H, np.float64).reshape(9).copy()


MUTANTS = {"outside counts as 0 in the erosion": (ErodeOutsideIsZero, "edge strips 70x37"),
           "outside counts as 1 in a dilation": (DilateOutsideIsOne, "blocks 4x4 5x5 6x6"),
           "threshold >=": (ThresholdNotStrict, "threshold 50 and 51 maxval 255"),
           "halves rounded up in F2": (HalvesUp, "halves 1/64 3/64 70x37 direct"),
           "H used uninverted": (Uninverted, "translation 1.3 0.77 129x45 direct")}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_told_apart(mutant):
    cls, name = MUTANTS[mutant]
    got, want = cases.run_with(cls(), cases.by_name(name)), cases.restated(name)
    assert not np.array_equal(got["mask"], want["mask"]) or not np.array_equal(got["warped"], want["warped"]), (mutant, name)
    assert not cases.same_answer(got, want)


def test_mutants_that_must_change_the_mask():
    """The morphology and threshold mutants show in the MASK (not only in an inner stage) on their named case."""
    for mutant in ("outside counts as 0 in the erosion", "outside counts as 1 in a dilation", "threshold >="):
        cls, name = MUTANTS[mutant]
        assert not np.array_equal(cases.run_with(cls(), cases.by_name(name))["mask"], cases.restated(name)["mask"]), mutant


# ---- the library's host side: refusals and atomicity, as a stand-alone program under the sanitizers ----------------------------------------

def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    from tests import fake_hip_build as fhb
    here = os.path.join(ROOT, "tests", "fake_hip_framediff")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_framediff.cpp")], ["framediff_api.cpp"], include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    scenarios = [l for l in lines if not l.startswith("ok refusal: ")]
    assert scenarios == ["ok answers_and_memory_kinds", "ok refusals", "ok call_failures", "ok create_failures"], lines
    refusals = [l[len("ok refusal: "):] for l in lines if l.startswith("ok refusal: ")]
    for needle in ("desc 0: H is singular", "desc 0: H is not finite", "desc 0: width out of range", "desc 0: height out of range",
                   "desc 0: threshold outside 0..254", "desc 0: maxval outside 0..255", "desc 3: threshold"):
        assert needle in refusals, (needle, refusals)


# ---- the surface ------------------------------------------------------------------------------------------------------------------------

def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_and_exported():
    """libdsdtm_amd_framediff.so exports exactly the symbols its header declares and reads no environment; the row stands in MORE_ADDONS."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_framediff.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(framediff.SYMBOLS) == {"dsdtm_framediff_create", "dsdtm_framediff_destroy", "dsdtm_framediff_last_error", "dsdtm_framediff_steps",
                                                  "dsdtm_framediff_step", "dsdtm_framediff_warp"}
    assert _exported(framediff.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", framediff.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    assert "framediff" in hip_build.MORE_ADDONS and "framediff" not in hip_build.ADDONS
    assert hip_build.MORE_ADDONS["framediff"][0] == ["framediff_api.cpp", "framediff.hip"]
    assert not {"framediff.hip", "framediff.h", "framediff_api.cpp"} & set(hip_build.SOURCES + hip_build.HEADERS)


@pytest.mark.parametrize("struct,name", [(framediff.Desc, "dsdtm_framediff_desc"), (framediff.Result, "dsdtm_framediff_result")])
def test_desc_layout(tmp_path, struct, name):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_framediff.h"', 'int main(void) {', f'  printf("%zu", sizeof({name}));']
    src += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in struct._fields_] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(struct)] + [getattr(struct, f[0]).offset for f in struct._fields_]


def test_header_documents_the_rules_the_quirks_and_the_parity():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_framediff.h")).read()
    for needle in ("src/Moving_Detection.cpp:36-63", "src/Frame.cpp:352", "QUIRK 1", "QUIRK 2", "tImgB = tframeA->mColorImg", "THIS PROJECT'S DEFINITION",
                   "unpinned and stays unpinned", "SUPERSEDES", *[f"F{i} " for i in range(1, 9)]):
        assert needle in hdr, needle
    for name, value in (("THRESHOLD", 50), ("MAXVAL", 200), ("MIN_SIDE", 16), ("MAX_SIDE", 4096), ("MAX_STEPS", 1024), ("MAX_FEATURES", 16384), ("INVERSE_MAP", 1)):
        assert re.search(rf"#define DSDTM_FRAMEDIFF_{name} {value}\b", hdr), name
    assert (FR.THRESHOLD, FR.MAXVAL, FR.INVERSE_MAP) == (framediff.THRESHOLD, framediff.MAXVAL, framediff.INVERSE_MAP) == (50, 200, 1)


def test_binding_refuses_outputs_it_could_not_write_in_place():
    ok = np.zeros((37, 80), np.uint8)[:, :70]
    assert framediff._output(ok, 70, 37)[0] is ok and framediff._output(ok, 70, 37)[2] == 80
    for bad in (np.zeros((37, 70), np.int32), np.zeros((37, 140), np.uint8)[:, ::2], np.zeros(37 * 70, np.uint8)):
        with pytest.raises(ValueError):
            framediff._output(bad, 70, 37)
    with pytest.raises(ValueError):
        framediff._output(np.zeros((37, 71), np.uint8), 70, 37)
