"""dsdtm_trackmap_local (include/dsdtm_amd_trackmap.h) without a GPU: the restatement (dsdtm_amd/track_map_restatement.py) against
tracking.flatten_local_map walking the OBJECTS of every world — it is the yardstick of the device entry, so it must not be its own —,
the host function flatten_local_map_host against the restatement through a compiled driver, and the declaration / export / ctypes
mirror of the add-on library. No tolerance anywhere: every column is a copy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import local_map, track_map, tracking
from dsdtm_amd import track_map_restatement as TR
from tests import track_map_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", [c for c in cases.all_cases() if c["kfs"] is not None], ids=lambda c: c["name"])
def test_restatement_equals_flatten_local_map_on_the_objects(c):
    for q, want in enumerate(cases.expected(c)):
        yard = tracking.flatten_local_map(c["kfs"], [c["mps"][i] for i in want["point"]])
        assert want["n_obs"] == len(yard["okf"]) and want["overflow_obs"] == int(c["obs_capacity"] is not None and want["n_obs"] > c["obs_capacity"])
        cut = len(want["flat"]["okf"])
        assert cut == (want["n_obs"] if c["obs_capacity"] is None else min(want["n_obs"], c["obs_capacity"]))
        for k in ("okf", "opx", "olv", "ob"):
            yard[k] = yard[k][:cut]
        cases.same_columns(want["flat"], yard, (c["name"], q))


def test_the_worlds_reach_what_they_are_named_for():
    by = {c["name"]: (c, cases.expected(c)[0]) for c in cases.all_cases()}
    c, w = by["plain_trajectory"]
    assert w["n_kf"] == 4 and w["n_points"] > 40 and w["n_obs"] > w["n_points"] and not w["overflow_points"] and not w["overflow_obs"]
    c, w = by["observed_from_outside_the_local_set"]
    okf = set(w["flat"]["okf"].tolist())
    assert okf - set(w["kf"]) and max(okf) == len(c["kfs"]) - 1 > max(w["kf"])
    c, w = by["observation_erased_slot_still_set"]
    i = w["point"].index(c["quirk_point"])                    # listed through keyframe 0's slot ...
    assert w["kf"] == [0] and w["flat"]["okf"][w["flat"]["off"][i]:w["flat"]["off"][i + 1]].tolist() == [1, 2, 3]      # ... which does not observe it
    c, w = by["point_without_observation"]
    i = w["point"].index(c["lone_point"])
    assert w["flat"]["off"][i] == w["flat"]["off"][i + 1] and 0 < i < len(w["point"]) - 1
    c, w = by["bad_point_in_a_local_keyframe"]
    bad = [p for p in range(len(c["mps"])) if c["mps"][p].IsBad()]
    assert len(bad) == 2 and not set(bad) & set(w["point"]) and not w["flat"]["bad"].any() and w["point"][3] != bad[0]
    c, w = by["two_observing_slots_of_one_keyframe"]
    k, s_free, s_obs = c["twice"]
    i = w["point"].index(int(c["world"]["slots"][k][s_obs]))
    seg = slice(w["flat"]["off"][i], w["flat"]["off"][i + 1])
    at = [j for j in range(seg.start, seg.stop) if w["flat"]["okf"][j] == k]
    assert len(at) == 2 and at[1] == at[0] + 1                 # two observations of that keyframe, in slot order:
    for j, s in zip(at, (s_free, s_obs)):
        assert cases.same_bits(w["flat"]["opx"][j], c["world"]["px"][k][s]) and cases.same_bits(w["flat"]["ob"][j], c["world"]["bearing"][k][s])
    c, w = by["grows_past_the_initial_capacities"]
    assert len(c["mps"]) > local_map.INITIAL_POINTS and len(c["kfs"]) > local_map.INITIAL_KEYFRAMES
    assert sum(len(s) for s in c["world"]["slots"]) > local_map.INITIAL_SLOTS and w["n_points"] > 500
    first = c["first_part"]
    assert sum(len(s) for s in c["world"]["slots"][:first]) < local_map.INITIAL_SLOTS and first < local_map.INITIAL_KEYFRAMES
    assert by["emits_4096_points"][1]["n_points"] == 4096 and by["emits_4096_points"][1]["overflow_points"] == 0
    w = by["emits_4097_points"][1]
    assert w["n_points"] == 4097 and w["overflow_points"] == 1 and len(w["point"]) == 4096 and len(w["flat"]["off"]) == 4097
    w, full = by["emits_4096_points_one_observation_short"][1], by["emits_4096_points"][1]
    assert w["overflow_obs"] == 1 and w["n_obs"] == full["n_obs"] == len(w["flat"]["okf"]) + 1 and np.array_equal(w["flat"]["off"], full["flat"]["off"])
    assert cases.same_bits(w["flat"]["ob"], full["flat"]["ob"][:-1]) and np.array_equal(w["flat"]["okf"], full["flat"]["okf"][:-1])


def test_found_counts_follow_the_objects():
    c = cases.found_changes()                                 # (a copy of its own: the shared case stays unchanged)
    for p, v in c["found_updates"]:
        c["mps"][p].mnFound = v
    world = cases.world_of(c["kfs"], c["mps"])
    want = TR.track_map_local(cases.CAM, c["poses"][0], world, c["n_local"])
    cases.same_columns(want["flat"], tracking.flatten_local_map(c["kfs"], [c["mps"][i] for i in want["point"]]), "after the updates")
    assert not np.array_equal(want["flat"]["found"], cases.expected(cases.by_name("found_counts_change"))[0]["flat"]["found"])


def test_host_function_agrees_with_the_restatement(tmp_path):
    """select_local_map_host + flatten_local_map_host (plain C++, no device call) through the compiled driver on every world: integers
    equal, floats and doubles bit-equal."""
    cs = cases.all_cases()
    exe = str(tmp_path / "track_map_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "track_map_host", "driver.cpp")], check=True)
    cases.write_cases(tmp_path / "cases.bin", cs)
    subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], check=True)
    got = cases.read_answers(tmp_path / "answers.bin", cs)
    for c, per in zip(cs, got):
        for q, (g, want) in enumerate(zip(per, cases.expected(c))):
            cases.same_answer(g, want, (c["name"], q))


def _lib_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_exported_and_mirrored(tmp_path):
    """The add-on library exports exactly the eleven symbols its header declares and reads no environment; the ctypes mirror has the
    header's layouts and limits; the five older libraries export what they exported."""
    from dsdtm_amd import capi, homography, motion
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_trackmap.h")).read()
    assert re.search(r"#define DSDTM_TRACKMAP_MAX_LOCAL_POINTS %d\b" % track_map.MAX_LOCAL_POINTS, hdr) and track_map.MAX_LOCAL_POINTS == 4096 == TR.MAX_LOCAL_POINTS
    assert re.search(r"#define DSDTM_TRACKMAP_MAX_CALL_BYTES %dll\b" % track_map.MAX_CALL_BYTES, hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", code))
    assert declared == set(track_map.SYMBOLS) and len(track_map.SYMBOLS) == 11
    assert _lib_symbols(track_map.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", track_map.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    lib = track_map.load()
    for sym, nargs in (("dsdtm_trackmap_create", 2), ("dsdtm_trackmap_destroy", 1), ("dsdtm_trackmap_last_error", 1), ("dsdtm_trackmap_map_create", 2),
                       ("dsdtm_trackmap_map_destroy", 2), ("dsdtm_trackmap_points_write", 7), ("dsdtm_trackmap_found_write", 5),
                       ("dsdtm_trackmap_keyframe_add", 10), ("dsdtm_trackmap_keyframe_write", 8), ("dsdtm_trackmap_map_read", 3), ("dsdtm_trackmap_local", 6)):
        decl = re.search(r"\b%s\(([^;]*?)\);" % sym, code, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib, sym).argtypes), sym
    # the other libraries: each still exports its own binding's list, and none of them carries a symbol of this one
    assert _lib_symbols(local_map.lib_path()) == set(local_map.SYMBOLS)
    assert _lib_symbols(capi.lib_path()) == set(capi.EXPORTED_SYMBOLS)
    assert _lib_symbols(motion.lib_path()) == set(motion.SYMBOLS) and _lib_symbols(homography.lib_path()) == set(homography.SYMBOLS)
    kf_hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsdtm_amd_keyframe.h")).read(), flags=re.S)
    assert _lib_symbols(os.path.join(ROOT, "dsdtm_amd", "csrc", "libdsdtm_amd_keyframe.so")) == set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", kf_hdr))
    for older in ("dsdtm_amd.h", "dsdtm_amd_localmap.h", "dsdtm_amd_keyframe.h", "dsdtm_amd_motion.h", "dsdtm_amd_homography.h"):
        assert "trackmap" not in open(os.path.join(ROOT, "include", older)).read(), older
    structs = [("dsdtm_trackmap_desc", track_map.Desc), ("dsdtm_trackmap_result", track_map.Result), ("dsdtm_trackmap_image", track_map.Image),
               ("dsdtm_localmap_params", track_map.Params), ("dsdtm_camera", track_map.Camera)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_trackmap.h"', 'int main(void) {']
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


def test_example_and_adapter_compile():
    """example_trackmap.cpp uses DSDTM::TrackMap::UpdateLocalMapOnDevice and fills a dsdtm_track_desc: the compiler sees it here, the
    MI355X runs it (tests/test_track_map_gpu.py)."""
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "dsdtm_amd", "host", "example_trackmap.cpp")], check=True)
    src = open(os.path.join(ROOT, "dsdtm_amd", "host", "example_trackmap.cpp")).read()
    assert "UpdateLocalMapOnDevice(" in src and "dsdtm_track_desc" in src and "FillDesc(" in src


def test_header_states_the_duty_the_order_and_the_limits():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_trackmap.h")).read()
    for needle in ("src/Optimizer.cpp:266-267", "src/MapPoint.cpp:45-55", "src/MapPoint.cpp:149-161", "THE CALLER'S DUTY", "in slot order",
                   "ascending\n *   (keyframe index, slot index) order", "pointer values", "MUST NOT", "DSDTM_TRACKMAP_MAX_CALL_BYTES", "4096 keyframes"):
        assert needle in hdr, needle
