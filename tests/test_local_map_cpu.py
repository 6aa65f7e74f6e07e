"""The keyframe and point selection of Tracking::UpdateLocalMap (reference src/Tracking.cpp:258-345) without a GPU: the restatement
(dsdtm_amd/local_map_restatement.py) against an independent walk over KeyFrame / MapPoint OBJECTS written the way the reference is
written — it is the yardstick of the device entry, so it must not be its own —, the host function select_local_map_host against
the restatement through a compiled driver, and the declaration / export / ctypes mirror of the add-on library."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import local_map, mapping
from dsdtm_amd import local_map_restatement as R
from tests import local_map_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def objects_of(world):
    """The world as mapping.KeyFrame / MapPoint objects."""
    mps = [mapping.MapPoint(i, X) for i, X in enumerate(world["p_world"])]
    for mp, b in zip(mps, world["bad"]):
        if b:
            mp.SetBadFlag()
        mp.mLastProjectedFrameId = -1
    kfs = []
    for k, slots in enumerate(world["slots"]):
        kf = mapping.KeyFrame(k, np.asarray(world["T_kf_w"][k]).reshape(3, 4), [None] * len(slots), mapping.Camera(512.0))
        for i, p in enumerate(slots):
            if p >= 0:
                kf.Add_MapPoint(mps[p], i)
        kfs.append(kf)
    return kfs, mps


def reference_walk(cam, T_cur, kfs, frame_id, n_local, boundary):
    """GetCloseKeyFrames + UpdateLocalMap over objects: lists, sorted(key=) (stable), an mLastProjectedFrameId attribute. numpy does
    the arithmetic here (the restatement uses Python floats): float64, one operation at a time."""
    T = np.asarray(T_cur, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))

    def is_visible(X):
        with np.errstate(all="ignore"):
            pc = [T[r, 0] * X[0] + T[r, 1] * X[1] + T[r, 2] * X[2] + T[r, 3] for r in range(3)]
            if pc[2] < 0.0:
                return False
            u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
            if not (np.isfinite(u) and np.isfinite(v)) or abs(u) >= 1e9 or abs(v) >= 1e9:
                return False
            ur, vr = int(np.rint(np.float32(u))), int(np.rint(np.float32(v)))
        return boundary <= ur < cam.width - boundary and boundary <= vr < cam.height - boundary
    close = []
    for kf in kfs:
        for mp in kf.mvMapPoints:
            if mp is None:
                continue
            X = mp.Get_Pose()
            if not X.any():
                continue
            if is_visible(X):
                d = T[:, 3] - kf.Get_Pose()[:, 3]
                sq = d * d
                close.append((kf, float(np.sqrt(sq[0] + (sq[1] + sq[2])))))
                break
    close = sorted(close, key=lambda c: c[1])
    local_kfs, local_mps = [], []
    for kf, _ in close[:n_local]:
        local_kfs.append(kf)
        for mp in kf.mvMapPoints:
            if mp is None or mp.IsBad() or mp.mLastProjectedFrameId == frame_id:
                continue
            mp.mLastProjectedFrameId = frame_id
            local_mps.append((mp, kf))
    return close, local_kfs, local_mps


@pytest.mark.parametrize("c", cases.all_cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_object_graph_walk(c):
    kfs, mps = objects_of(c["world"])
    for q, (T, want) in enumerate(zip(c["poses"], cases.expected(c))):
        close, lk, lm = reference_walk(cases.CAM, T, kfs, q, c["n_local"], c["boundary"])
        cap = len(lm) if c["capacity"] is None else c["capacity"]
        assert (want["n_close"], want["n_kf"], want["n_points"], want["overflow"]) == (len(close), len(lk), len(lm), int(len(lm) > cap))
        assert want["kf"] == [kf.mlId for kf in lk]
        assert want["kf_dist"] == [d for _, d in close[:c["n_local"]]]
        assert want["point"] == [mp.mlID for mp, _ in lm][:cap]
        assert want["point_kf"] == [lk.index(kf) for _, kf in lm][:cap]


def test_the_cases_reach_what_they_are_named_for():
    by = {c["name"]: cases.expected(c)[0] for c in cases.all_cases()}
    assert by["empty_map"] == dict(kf=[], kf_dist=[], point=[], point_kf=[], n_close=0, n_kf=0, n_points=0, overflow=0)
    assert by["points_but_no_keyframe"]["n_close"] == 0
    assert by["keyframes_without_slots"]["kf"] == [1]
    for ns in (63, 64, 65, 129):
        assert by[f"only_visible_point_in_last_of_{ns}_slots"]["kf"] == [0]
    assert by["zero_position_pos"]["kf"] == [1] and by["zero_position_neg"]["kf"] == [1]
    assert by["only_visible_point_is_bad"]["kf"] == [0] and by["only_visible_point_is_bad"]["point"] == [1]
    assert by["depth_guards"]["kf"] == [2]
    for name in ("edges_u_boundary_0", "edges_v_boundary_0", "edges_u_boundary_8", "edges_v_boundary_8"):
        n = len([c for c in cases.all_cases() if c["name"] == name][0]["world"]["slots"])
        assert by[name]["n_close"] >= 8 and n - by[name]["n_close"] >= 4, name      # both sides of the edges are present
    assert by["two_identical_translations"]["kf"] == [1, 2, 0] and by["two_identical_translations"]["kf_dist"][:2] == [1.0, 1.0]
    assert by["tie_at_the_cut"]["kf"] == [5, 1, 3, 0] and by["tie_at_the_cut"]["n_close"] == 6
    assert by["tie_at_the_cut_negative_side"]["kf"] == [5, 1, 3, 0]
    assert by["exactly_n_local_close"]["kf"] == [3, 2, 0] and by["fewer_close_than_n_local"]["kf"] == [3, 2]
    assert by["more_close_than_n_local"]["kf"] == [5, 4, 3] and by["n_local_1"]["kf"] == [2]
    assert by["n_local_64_of_70"]["n_kf"] == 64 and by["n_local_64_of_300_with_ties"]["n_close"] == 200
    assert by["point_in_two_chosen_keyframes"] ["point"] == [0, 1, 2] and by["point_in_two_chosen_keyframes"]["point_kf"] == [0, 0, 1]
    d = by["duplicates_within_a_keyframe"]
    assert len(set(d["point"])) == len(d["point"]) and d["point"][:3] == [0, 1, 2] and d["point_kf"][-3:] == [1, 1, 1]
    assert by["capacity_one_short"]["overflow"] == 1 and len(by["capacity_one_short"]["point"]) == by["capacity_one_short"]["n_points"] - 1
    assert by["capacity_zero"]["overflow"] == 1 and by["capacity_zero"]["point"] == []
    rw = cases.expected(cases.all_cases()[-1])
    assert all(10 < r["n_close"] < 150 and r["n_kf"] == 10 and r["n_points"] > 300 for r in rw)


def test_cv_round_narrows_before_it_rounds():
    assert R.cv_round(10.5 - 1e-9) == 10 and R.cv_round(10.5 + 1e-9) == 10 and R.cv_round(11.5 - 1e-9) == 12      # float: exactly k + 0.5, to even
    assert R.cv_round(10.5 + 1e-4) == 11 and R.cv_round(-0.5) == 0 and R.cv_round(0.5) == 0 and R.cv_round(638.5) == 638
    assert not R.in_image(cases.CAM, math.inf, 0.0, 0) and not R.in_image(cases.CAM, math.nan, 0.0, 0) and not R.in_image(cases.CAM, 1e9, 0.0, 0)


def test_host_function_agrees_with_the_restatement(tmp_path):
    """select_local_map_host (plain C++, no device call) through the compiled driver on every case: lists equal, distances bit-equal."""
    cs = cases.all_cases()
    exe = str(tmp_path / "local_map_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "local_map_host", "driver.cpp")], check=True)
    cases.write_cases(tmp_path / "cases.bin", cs)
    out = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == sum(len(c["poses"]) for c in cs)
    for line in out:
        head, kf, dist, point, point_kf = [part.split() for part in line.split("|")]
        ci, q, n_close, n_kf, n_points, overflow = (int(v) for v in head)
        got = dict(n_close=n_close, n_kf=n_kf, n_points=n_points, overflow=overflow, kf=[int(v) for v in kf], point=[int(v) for v in point],
                   point_kf=[int(v) for v in point_kf], kf_dist=np.array([int(v, 16) for v in dist], np.uint64).view(np.float64).tolist())
        cases.same_answer(got, cases.expected(cs[ci])[q], (cs[ci]["name"], q))


def test_declared_exported_and_mirrored(tmp_path):
    """The add-on library exports exactly the ten symbols its header declares and reads no environment; the ctypes mirror has the
    header's layouts and limits; libdsdtm_amd.so is untouched."""
    from dsdtm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_localmap.h")).read()
    for name, val in (("MAX_POINTS", local_map.MAX_POINTS), ("MAX_KEYFRAMES", local_map.MAX_KEYFRAMES), ("MAX_SLOTS", local_map.MAX_SLOTS),
                      ("MAX_LOCAL", local_map.MAX_LOCAL), ("MAX_DESCS", local_map.MAX_DESCS)):
        assert re.search(r"#define DSDTM_LOCALMAP_%s %d\b" % (name, val), hdr), name
    assert (local_map.MAX_POINTS, local_map.MAX_KEYFRAMES, local_map.MAX_SLOTS, local_map.MAX_LOCAL, local_map.MAX_DESCS) == (1048576, 16384, 4096, 64, 1024)
    internal = open(os.path.join(ROOT, "dsdtm_amd", "csrc", "localmap.h")).read()
    for name, val in (("POINTS", local_map.INITIAL_POINTS), ("KEYFRAMES", local_map.INITIAL_KEYFRAMES), ("SLOTS", local_map.INITIAL_SLOTS)):
        assert re.search(r"LM_INITIAL_%s = %d;" % (name, val), internal), name
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(local_map.SYMBOLS) and len(local_map.SYMBOLS) == 10
    out = subprocess.run(["nm", "-D", "--defined-only", local_map.lib_path()], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.strip()} == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", local_map.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    lib = local_map.load()
    for sym, nargs in (("dsdtm_localmap_create", 2), ("dsdtm_localmap_destroy", 1), ("dsdtm_localmap_last_error", 1), ("dsdtm_localmap_map_create", 2),
                       ("dsdtm_localmap_map_destroy", 2), ("dsdtm_localmap_points_write", 6), ("dsdtm_localmap_keyframe_add", 6),
                       ("dsdtm_localmap_keyframe_write", 7), ("dsdtm_localmap_map_read", 3), ("dsdtm_localmap_select", 6)):
        decl = re.search(r"\b%s\(([^;]*?)\);" % sym, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib, sym).argtypes), sym
    main = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    assert "localmap" not in main and not set(local_map.SYMBOLS) & set(capi.EXPORTED_SYMBOLS)
    structs = [("dsdtm_localmap_params", local_map.Params), ("dsdtm_localmap_desc", local_map.Desc), ("dsdtm_localmap_result", local_map.Result),
               ("dsdtm_localmap_image", local_map.Image), ("dsdtm_camera", local_map.Camera)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_localmap.h"', 'int main(void) {']
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
    """example_localmap.cpp instantiates DSDTM::LocalMap::UpdateLocalMapOnDevice (a member template): the compiler sees it here, the
    MI355X runs it (tests/test_local_map_gpu.py)."""
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "dsdtm_amd", "host", "example_localmap.cpp")], check=True)
    src = open(os.path.join(ROOT, "dsdtm_amd", "host", "example_localmap.cpp")).read()
    assert "UpdateLocalMapOnDevice(" in src


def test_header_cites_the_reference_at_every_rule():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_localmap.h")).read()
    block = hdr[hdr.index("---- the selection"):hdr.index("typedef struct dsdtm_localmap_params")]
    for needle in ("src/Tracking.cpp:315-345", "src/Tracking.cpp:258-297", "src/Frame.cpp:300-311", "src/Camera.cpp:187-193", "isZero(0)", ":267-268",
                   "include/Map.h:60", "MAP INDEX ORDER", "mLastProjectedFrameId", "p0 + (p1 + p2)", "NOT the camera centres"):
        assert needle in block, needle
