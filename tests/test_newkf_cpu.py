"""Tracking::CraeteKeyframe from the per-cell corners on (include/dsdtm_amd_newkf.h, rules K1-K6) without a GPU: the restatement
(dsdtm_amd/keyframe_creation_restatement.py, which paints a real mask) against tests/detector_restatement.detect on the walk, the host
function create_keyframe_host against the restatement through a compiled driver, the declaration / export / ctypes mirror of the add-on
library, and the host side of dsdtm_amd/csrc/newkf_api.cpp as a stand-alone program (its own main) over the unmodified fake HIP runtime
of tests/fake_hip under AddressSanitizer + UndefinedBehaviorSanitizer (+ LeakSanitizer). Nothing is loaded into Python under a
sanitizer and nothing is preloaded."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import keyframe_creation as kc
from dsdtm_amd import keyframe_creation_restatement as R
from tests import detector_restatement
from tests import fake_hip_build as fhb
from tests import newkf_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", [c for c in cases.all_cases() if c["detect_comparable"]], ids=lambda c: c["name"])
def test_walk_equals_the_detector_restatement(c):
    """K1-K4: the features the walk adds are those of tests/detector_restatement.detect (its own sort, mask and disc painting)."""
    p, i = c["prm"], c["inp"]
    want = detector_restatement.detect((i.cell_score, i.cell_x, i.cell_y, i.cell_level), p.width, p.height, p.cell_size, p.max_fts,
                                       np.asarray(i.px_xy, np.float32).reshape(-1, 2), i.has_point, p.min_dist)
    assert R.walk(p, i) == want
    a = cases.answers()[c["name"]]
    assert a["n_new"] == len(want) and a["n_slots"] == i.n_existing + len(want)
    assert [(int(x), int(y)) for x, y in a["px_xy"][i.n_existing:]] == [(x, y) for x, y, _ in want]
    assert a["level"][i.n_existing:].tolist() == [l for _, _, l in want]


def test_the_cases_reach_their_branches():
    a = cases.answers()
    by = {c["name"]: c for c in cases.all_cases()}
    assert a["n_existing_at_cap"]["n_new"] == 0 and a["n_existing_over_cap"]["n_new"] == 0                      # K1
    assert a["n_existing_over_cap"]["n_slots"] == 14 and a["n_existing_over_cap"]["n_new_points"] > 0            # ... K6 still lifts
    assert a["cap_mid_walk"]["n_new"] == 7 and a["cap_after_first"]["n_new"] == 1                               # K4's stop
    s = by["ties_ragged"]["inp"].cell_score
    assert len(np.unique(s[s > 20])) < int((s > 20).sum()) // 4                                                  # K2: many ties
    assert np.isnan(by["ties_ragged_nan"]["inp"].cell_score).sum() >= 2
    # K3's quirk: with no existing feature the dynamic mask is ignored — the same input without it gives the same answer, and WITH one
    # existing feature the mask removes corners
    inp = by["empty_frame_dyn_ignored"]["inp"]
    prm = by["empty_frame_dyn_ignored"]["prm"]
    assert (np.asarray(inp.dyn_mask) > 200).mean() > 0.3
    bare = R.NewKeyframeInput(inp.cell_score, inp.cell_x, inp.cell_y, inp.cell_level, inp.depth, inp.depth_scale, inp.T_c2w, inp.first_point_index)
    assert R.walk(prm, bare) == R.walk(prm, inp) and len(R.walk(prm, inp)) > 10
    d = by["dyn_mask_with_existing"]
    without = R.NewKeyframeInput(**{**d["inp"].__dict__, "dyn_mask": None})
    assert len(R.walk(d["prm"], without)) > len(R.walk(d["prm"], d["inp"])) > 0
    # the disc's rim: a corner ON the rim is never added; one pixel outside it is (where no accepted corner's disc reaches it first)
    e, ea = by["disc_edges"], a["disc_edges"]
    added = {(int(x), int(y)) for x, y in ea["px_xy"][2:]}
    hw, cx, cy = detector_restatement.circle_spans(9), 60, 50
    for dy in (0, 3, 6, 8, 9):
        assert (cx + hw[dy], cy + dy) not in added and (cx - hw[dy], cy - dy) not in added, dy
    assert (cx + hw[0] + 1, cy) in added and (cx - hw[0] - 1, cy) in added
    hc = detector_restatement.circle_spans(12)
    assert (140, 50) in added and (140 + hc[0], 50) not in added and (140 - hc[0] - 1, 50) in added      # ... and an accepted corner's
    assert e["inp"].n_existing == 2
    # the lift's branches
    dc, da = by["depth_branches"], a["depth_branches"]
    depth = dc["inp"].depth
    slot = {(int(x), int(y)): k for k, (x, y) in enumerate(da["px_xy"])}
    inv = np.float32(1.0) / np.float32(5000.0)
    for first, (ddx, ddy) in enumerate(((-1, 0), (0, -1), (1, 0), (0, 1))):
        x, y = 20 + 30 * first, 20
        assert da["depth_of_slot"][slot[(x, y)]] == np.float32(depth[y + ddy, x + ddx]) * inv != 0
    for x, y in ((20, 60), (80, 99), (175, 99)):
        k = slot[(x, y)]
        assert da["depth_of_slot"][k] == -1 and da["point_of_slot"][k] == -1 and da["observes"][k] == 0
    assert da["depth_of_slot"][slot[(80, 0)]] == np.float32(depth[0, 81]) * inv and da["depth_of_slot"][slot[(175, 50)]] == np.float32(depth[51, 175]) * inv
    assert da["depth_of_slot"][slot[(0, 0)]] == np.float32(depth[0, 1]) * inv and da["depth_of_slot"][slot[(0, 50)]] == np.float32(depth[49, 0]) * inv
    assert da["depth_of_slot"][0] == np.float32(depth[70, 109]) * inv and da["point_of_slot"][0] == 123           # an existing non-initial feature
    assert da["point_of_slot"][1] == -1 and da["point_of_slot"][3] == 17 and da["depth_of_slot"][3] == -1 and da["point_of_slot"][4] == -1
    new = da["point_of_slot"][(da["point_of_slot"] >= 123) & (np.arange(da["n_slots"]) != 3)]
    assert new.tolist() == list(range(123, 123 + da["n_new_points"]))                                           # numbered in slot order
    assert a["all_depth_zero"]["n_new_points"] == 0 and a["all_depth_zero"]["n_new"] > 0
    assert a["outside_corners_skipped"]["n_new"] > 0 and not {(96, int(by["outside_corners_skipped"]["inp"].cell_y[2]))} & {
        (int(x), int(y)) for x, y in a["outside_corners_skipped"]["px_xy"]}


def test_unprojected_points_are_the_inverse_pose_applied():
    """new_p_world against numpy's own R^T (p - t), to rounding: the restated order of operations is the reference's, the value the pose's."""
    c = [c for c in cases.all_cases() if c["name"] == "ties_ragged"][0]
    a = cases.answers()["ties_ragged"]
    T = np.asarray(c["inp"].T_c2w).reshape(3, 4)
    k = np.flatnonzero(a["depth_of_slot"] >= 0)
    assert len(k) == a["n_new_points"] > 10
    fx, fy, cx, cy = cases.CAM
    z = a["depth_of_slot"][k].astype(np.float64)
    pc = np.stack([z * (a["px_xy"][k, 0] - cx) / fx, z * (a["px_xy"][k, 1] - cy) / fy, z], axis=1)
    np.testing.assert_allclose(a["new_p_world"], (pc - T[:, 3]) @ T[:, :3], rtol=0, atol=1e-5)
    new = a["bearing"][c["inp"].n_existing:]
    np.testing.assert_allclose(np.linalg.norm(new, axis=1), 1.0, rtol=0, atol=1e-15)


def test_host_function_agrees_with_the_restatement(tmp_path):
    """create_keyframe_host (plain C++, no device call) through the compiled driver on every case: all columns, new_p_world and
    depth_of_slot bit-equal."""
    cs = cases.all_cases()
    exe = str(tmp_path / "newkf_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "newkf_host", "driver.cpp")], check=True)
    (tmp_path / "cases.bin").write_bytes(cases.pack(cs))
    subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], check=True)
    got = cases.unpack((tmp_path / "answers.bin").read_bytes(), len(cs))
    for c, g in zip(cs, got):
        cases.assert_same(g, cases.answers()[c["name"]], c["name"])


def test_declared_exported_and_mirrored(tmp_path):
    """The add-on library exports exactly the five symbols its header declares and reads no environment; the ctypes mirror has the
    header's layouts and limits; libdsdtm_amd.so is untouched."""
    from dsdtm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_newkf.h")).read()
    for name, val in (("MAX_TRACKERS", kc.MAX_TRACKERS), ("MAX_CELLS", kc.MAX_CELLS), ("MAX_EXISTING", kc.MAX_EXISTING), ("MAX_RADIUS", kc.MAX_RADIUS),
                      ("MAX_SIDE", kc.MAX_SIDE)):
        assert re.search(r"#define DSDTM_NEWKF_%s %d\b" % (name, val), hdr), name
    assert (kc.MAX_TRACKERS, kc.MAX_CELLS, kc.MAX_RADIUS) == (1024, 4096, 127)
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(kc.SYMBOLS) and len(kc.SYMBOLS) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", kc.lib_path()], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.strip()} == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", kc.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    lib = kc.load()
    for sym, nargs in (("dsdtm_newkf_create", 2), ("dsdtm_newkf_destroy", 1), ("dsdtm_newkf_last_error", 1), ("dsdtm_newkf_make", 5),
                       ("dsdtm_newkf_make_batch", 6)):
        decl = re.search(r"\b%s\(([^;]*?)\);" % sym, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib, sym).argtypes), sym
    main = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    assert "newkf" not in main and not set(kc.SYMBOLS) & set(capi.EXPORTED_SYMBOLS)
    structs = [("dsdtm_newkf_params", kc.Params), ("dsdtm_newkf_desc", kc.Desc), ("dsdtm_newkf_result", kc.Result), ("dsdtm_camera", kc.Camera)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_newkf.h"', 'int main(void) {']
    for cname, ct in structs:
        src.append(f'  printf("%zu", sizeof({cname}));')
        src += [f'  printf(" %zu", offsetof({cname}, {f}));' for f, _ in ct._fields_]
        src.append('  printf("\\n");')
    src += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (cname, ct), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], cname


def test_header_cites_the_reference_at_every_rule():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_newkf.h")).read()
    for needle in ("K1 (:71-72)", "K2 (:110", "Feature_detection.h:29-32", "K3 (:119-122, src/Frame.cpp:286-298)", "K4 (:124-150)",
                   "K5 (:145, src/Frame.cpp:139-149)", "K6 (src/Tracking.cpp:424-455)", "IGNORED on an empty", "unpinned", "OUT OF SCOPE",
                   "RECTIFIED", "(-1,0), (0,-1), (1,0), (0,1)"):
        assert needle in hdr, needle


def test_example_compiles():
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "dsdtm_amd", "host", "example_newkf.cpp")], check=True)
    src = open(os.path.join(ROOT, "dsdtm_amd", "host", "example_newkf.cpp")).read()
    assert "CraeteKeyframeOnDevice(" in src and "CreateInitialMapRGBDOnDevice(" in src          # the adapters are instantiated: the compiler sees them here


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_newkf")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_newkf.cpp")], ["newkf_api.cpp"],
                           include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok answers_and_memory_kinds", "ok refusals", "ok hip_failures", "ok overflow", "ok limits", "ok create_failures"], (lines, r.stderr[-3000:])
