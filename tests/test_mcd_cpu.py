"""The contour box of MCDWrapper::Run without a GPU: the restatement dsdtm_amd/contour_restatement.py (rules C1-C6 of
include/dsdtm_amd_mcd.h) against hand-computed cases, its plain-C twin tests/contour_restatement.c and mcd_box_host
(dsdtm_amd/host/dsdtm_mcd_host.hpp), bit for bit; the invariants of the definition on random masks; its mutants; the surface of
libdsdtm_amd_mcd.so; the host side under ASan/UBSan over the fake HIP runtime; which steps of the motion worlds draw a rectangle.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import capi, mcd, motion
from dsdtm_amd import contour_restatement as CR
from dsdtm_amd.csrc import build as hip_build
from tests import fake_hip_build as fhb
from tests import mcd_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = cases.hand_cases()
RANDOM = cases.random_masks()
LARGER = [("serpentine", cases.serpentine()), ("checkerboard", cases.checkerboard()), ("u_trap", cases.u_trap())]


@pytest.fixture(scope="module")
def impls(tmp_path_factory):
    d = tmp_path_factory.mktemp("mcd")
    return cases.c_twin(d).contour_box, cases.host_function(d).mcd_box_host_c


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(impls, name):
    mask, want = HAND[name]
    want = dict(want, boxed=cases.expected_boxed(mask, want["box"]))
    got = cases.restated(name, mask)
    assert cases.same(got, want), (name, got["box"], got["area2"], got["n_components"])
    for fn in impls:
        assert cases.same(cases.run_c(fn, mask), want), name
    assert not np.array_equal(mask, 0 * mask) or got["n_components"] == 0


def test_hand_cases_say_what_the_issue_lists():
    assert HAND["rectangle"][1]["area2"] == 2 * (7 - 1) * (5 - 1) and HAND["l3"][1]["area2"] == 1 and HAND["plus5"][1]["area2"] == 4
    for line in ("pixel", "line_horizontal", "line_vertical", "line_diagonal", "line_antidiagonal"):
        assert HAND[line][1]["area2"] == 0 and HAND[line][1]["box"] == [0, 0, 0, 0]
    m = HAND["frame_on_all_edges"][0]
    assert m[0].all() and m[-1].all() and m[:, 0].all() and m[:, -1].all()
    assert HAND["l3"][0].max() == 7            # C1: any non-zero byte; C5: other bytes unchanged (the dot of value 3)


@pytest.mark.parametrize("name,mask", RANDOM + LARGER, ids=[n for n, _ in RANDOM + LARGER])
def test_restatement_twin_and_host_function_bit_equal(impls, name, mask):
    got = cases.restated(name, mask)
    for fn in impls:
        assert cases.same(cases.run_c(fn, mask), got), name
    for c in got["components"]:                # the bound the device prunes by
        assert c["area2"] <= 2 * (c["maxx"] - c["minx"]) * (c["maxy"] - c["miny"]), (name, c)
    assert np.array_equal(got["boxed"] != mask, (got["boxed"] == 255) & (mask != 255))


def _summary(r, swap=False):
    return sorted((c["area2"], *((c["maxy"] - c["miny"], c["maxx"] - c["minx"]) if swap else (c["maxx"] - c["minx"], c["maxy"] - c["miny"]))) for c in r["components"])


@pytest.mark.parametrize("name,mask", RANDOM, ids=[n for n, _ in RANDOM])
def test_invariants_under_transpose_and_flips(name, mask):
    """area2 and the extents of EVERY component, the count and the winner's area2 map under transpose and both flips (a wrong
    direction table or stop rule breaks this). The box maps too wherever the winning area2 is held by one component only: between
    equals the raster-first one wins (C4), and which one that is changes with the transform."""
    r = cases.restated(name, mask)
    h, w = mask.shape
    x, y, bw, bh = r["box"]
    unique = sum(1 for c in r["components"] if c["area2"] == r["area2"]) == 1
    run = CR.ContourRestatement().run
    for what, other, box, swap in (("transpose", run(np.ascontiguousarray(mask.T)), [y, x, bh, bw], True),
                                   ("flip x", run(np.ascontiguousarray(mask[:, ::-1])), [w - x - bw, y, bw, bh], False),
                                   ("flip y", run(np.ascontiguousarray(mask[::-1])), [x, h - y - bh, bw, bh], False)):
        assert other["area2"] == r["area2"] and other["n_components"] == r["n_components"], (name, what)
        assert _summary(other, swap) == _summary(r), (name, what)
        if r["area2"] > 0 and unique:
            assert other["box"] == box, (name, what)


class FourConnected(CR.ContourRestatement):
    CONNECTIVITY = 4


class TiesToTheLast(CR.ContourRestatement):
    def beats(self, area2, best):
        return area2 >= best


class ExclusiveRectangle(CR.ContourRestatement):
    def rect(self, minx, miny, maxx, maxy):
        return slice(miny, maxy), slice(minx, maxx)


@pytest.mark.parametrize("mutant,case", [(FourConnected, "diagonal_join"), (TiesToTheLast, "two_equal_squares"), (TiesToTheLast, "pixel"),
                                         (ExclusiveRectangle, "plus5")])
def test_mutants_are_told_apart(mutant, case):
    mask, want = HAND[case]
    want = dict(want, boxed=cases.expected_boxed(mask, want["box"]))
    assert cases.same(CR.ContourRestatement().run(mask), want)
    assert not cases.same(mutant().run(mask), want), (mutant.__name__, case)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_and_exported():
    """libdsdtm_amd_mcd.so exports exactly the 11 symbols its header declares and reads no environment; libdsdtm_amd.so and
    libdsdtm_amd_motion.so export what they exported; the main library's source hash covers nothing of this."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_mcd.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(mcd.SYMBOLS) and len(mcd.SYMBOLS) == 11 and len(set(mcd.SYMBOLS)) == 11
    assert _exported(mcd.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", mcd.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    assert _exported(motion.lib_path()) == set(motion.SYMBOLS) and len(motion.SYMBOLS) == 10
    assert _exported(capi.lib_path(False)) == set(capi.EXPORTED_SYMBOLS) and len(capi.EXPORTED_SYMBOLS) == 38
    assert re.search(r"#define DSDTM_MCD_MAX_PIXELS 1048576\b", hdr) and mcd.MAX_PIXELS == 1 << 20
    assert hip_build.MORE_ADDONS["mcd"][0] == ["mcd_api.cpp", "contour.hip", "motion.hip"] and "mcd" not in hip_build.ADDONS
    assert not {"contour.hip", "contour.h", "mcd_api.cpp", "motion_api_body.h"} & set(hip_build.SOURCES + hip_build.HEADERS)
    lib = mcd.load()
    assert len(lib.dsdtm_mcd_step.argtypes) == 15 and len(lib.dsdtm_mcd_steps.argtypes) == 3 and len(lib.dsdtm_mcd_boxes.argtypes) == 3


@pytest.mark.parametrize("struct,name", [(mcd.Desc, "dsdtm_mcd_desc"), (mcd.BoxDesc, "dsdtm_mcd_box_desc")])
def test_desc_layout(tmp_path, struct, name):
    """The descs as a C compiler lays them out, against the ctypes mirrors; dsdtm_mcd_desc begins as dsdtm_motion_desc does."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_mcd.h"', 'int main(void) {', f'  printf("%zu", sizeof({name}));']
    src += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in struct._fields_] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(struct)] + [getattr(struct, f[0]).offset for f in struct._fields_]
    if struct is mcd.Desc:
        for f, _ in motion.Desc._fields_:
            if f != "reserved":
                assert getattr(mcd.Desc, f).offset == getattr(motion.Desc, f).offset, f


def test_headers_document_the_rules_and_the_parity():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_mcd.h")).read()
    for needle in ("MCDWrapper.cpp:65-137", ":98-128", "src/Frame.cpp:352", "OpenCV 3.2", "THIS PROJECT'S DEFINITION", "unpinned and stays unpinned",
                   "C1 foreground", "C2 contour", "C3 area", "C4 winner", "C5 rectangle", "C6 features", "Suzuki", "never decide anything",
                   "contour ORDER", "INCLUSIVE", "DSDTM_MCD_MAX_PIXELS"):
        assert needle in hdr, needle
    assert "include/dsdtm_amd_mcd.h" in open(os.path.join(ROOT, "include", "dsdtm_amd_motion.h")).read()


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_mcd")
    there = os.path.join(ROOT, "tests", "fake_hip_motion")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_contour.cpp"), os.path.join(there, "fake_motion.cpp")],
                           ["mcd_api.cpp"], include_dirs=[here, there])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok step_failures", "ok boxes_failures", "ok argument_checks", "ok create_failures"], lines


def test_a_motion_world_draws_a_rectangle_that_changes_a_flag():
    """The GPU test of the whole Run (tests/test_mcd_gpu.py) needs a step at which the restated chain draws a rectangle and at least
    one feature's flag differs between the boxed and the raw mask; the bright-object worlds give one."""
    found = {name: cases.rectangle_steps(name) for name in ("A", "C")}
    print("[mcd] steps with a rectangle that changes a flag:", found)
    assert found["A"] and found["C"], found
    e = cases.chain_of("A")[found["A"][0]]
    assert e["c"]["box"][2] > 1 and e["c"]["box"][3] > 1 and (e["flags"] >= e["flags_raw"]).all()
