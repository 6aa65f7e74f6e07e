"""Tracking::NeedKeyframe (reference src/Tracking.cpp:347-410) without a GPU: the numpy restatement
(dsdtm_amd/keyframe_decision.py) against answers worked out by hand — it is the yardstick of the device entry, so it must not
be its own — and the declaration / export / ctypes mirror of the add-on library that carries dsdtm_need_keyframe(s)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

from dsdtm_amd import capi
from dsdtm_amd import keyframe_decision as K
from tests import need_keyframe_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = cases.I34


def ref(**kw):
    return cases.run_reference(cases.make(**kw))


def test_pixel_distance_exactly_at_the_threshold_does_not_fire_and_one_step_more_does():
    c = cases.EXACT["k2_at_threshold"]()
    # exactly representable: 40 / 512 = 0.078125, 512 * 0.078125 / 1 = 40, 320 + 40 - 320 = 40
    assert 40.0 / 512.0 == 0.078125 and 512.0 * (0.5 + 0.078125) / 1.0 + 320.0 - (512.0 * 0.5 / 1.0 + 320.0) == 40.0
    r = cases.run_reference(c)
    assert r["px_dist"] == [40.0] * r["n_px"] and r["n_px"] == 31 and r["median_px"] == 40.0
    assert r["rule_mask"] == 0 and r["need"] == 0 and r["reason"] == 0          # strict > (:378); K3 silent (min_trans large)
    r = cases.run_reference(cases.EXACT["k2_above_threshold"]())
    assert r["median_px"] > 40.0 and r["median_px"] - 40.0 < 1e-9 and r["rule_mask"] == 2 and r["reason"] == 2 and r["need"] == 1


def test_count_rule_at_its_four_edges():
    for n_valid, fires in ((29, False), (30, True), (50, True), (51, False)):
        r = ref(n_valid=n_valid)
        assert bool(r["rule_mask"] & 1) == fires and r["need"] == int(fires) and r["reason"] == (1 if fires else 0), n_valid


def test_parallax_rule_fires_at_equality():
    r = cases.run_reference(cases.EXACT["k3_trans_equal"]())
    assert r["trans"] == 0.125 and r["rot"] == 0.0 and r["rule_mask"] == 4 and r["reason"] == 3      # >= (:387)
    c = cases.EXACT["k3_trans_equal"]()
    c["params"].min_trans = float(np.nextafter(0.125, 1.0))
    assert cases.run_reference(c)["rule_mask"] == 0


def test_scene_depth_rule_fires_at_equality():
    # depths all 2: m = 2; centre (4, 3.2, 5.2): 4 / 2 = 2 >= 2, 3.2 / 2 = 1.6 >= 0.8 * 2, 5.2 / 2 = 2.6 >= 1.3 * 2
    assert 4.0 / 2.0 == 2.0 and 3.2 / 2.0 >= 2.0 * 0.8 and 5.2 / 2.0 >= 2.0 * 1.3
    r = cases.run_reference(cases.EXACT["k4_equal"]())
    assert r["median_depth"] == 2.0 and r["min_depth"] == 2.0 and r["svo_kf"] == 0 and r["rule_mask"] == 8 and r["reason"] == 4


def test_fabs_of_a_boolean_is_the_boolean():
    """fabs(c.x / m >= m) (:398): a centre at x = -4 does NOT fire; a restatement that takes |c.x / m| would."""
    r = cases.run_reference(cases.EXACT["k4_fabs_quirk"]())
    assert r["svo_kf"] == -1 and r["rule_mask"] == 0 and r["need"] == 0
    assert abs(-4.0 / 2.0) >= 2.0          # the "fixed" rule would have fired


def test_the_walk_stops_after_31_samples_not_30():
    """40 keyframe points, displacements ~1, 2, .. 31 px and then nine huge ones: 31 samples ignore the tail (index 15 of the
    order: ~16 px); with px_samples = 40 the tail counts (index 20: ~21 px); 30 samples stop one earlier."""
    c = cases.EXACT["k2_31_stop"]()
    r = cases.run_reference(c)
    assert r["n_px"] == 31 and abs(r["median_px"] - 16.0) < 1e-9 and max(r["px_dist"]) < 32.0
    c["params"].px_samples = 40
    r = cases.run_reference(c)
    assert r["n_px"] == 40 and abs(r["median_px"] - 21.0) < 1e-9 and max(r["px_dist"]) == 4096.0
    c["params"].px_samples = 30
    r = cases.run_reference(c)
    assert r["n_px"] == 30 and abs(r["median_px"] - 16.0) < 1e-9


def test_with_40_samples_the_late_points_decide():
    c = cases.small_then_huge(20)                      # 20 of 8 px then 20 of 4096 px: the first 31 hold 20 small ones
    r = cases.run_reference(c)
    assert r["n_px"] == 31 and r["median_px"] == 8.0 and not r["rule_mask"] & 2
    c["params"].px_samples = 40                        # all 40: index 20 of the order is the first huge one
    r = cases.run_reference(c)
    assert r["n_px"] == 40 and r["median_px"] == 4096.0 and r["rule_mask"] & 2


def test_bad_flags_shift_the_window():
    c = cases.small_then_huge(20)
    bad = np.zeros(40, np.uint8)
    bad[:9] = 1                                        # 9 of the small ones are skipped: the window is points 9..39
    c["kf_bad"] = bad
    r = cases.run_reference(c)
    assert r["n_px"] == 31 and r["median_px"] == 4096.0 and r["rule_mask"] & 2          # 11 small, 20 huge


def test_median_is_the_upper_middle():
    assert [K.median_index(m) for m in (1, 2, 3, 4)] == [0, 1, 1, 2]
    assert K.get_median([7.0]) == 7.0 and K.get_median([2.0, 1.0]) == 2.0
    assert K.get_median([3.0, 1.0, 2.0]) == 2.0 and K.get_median([4.0, 1.0, 3.0, 2.0]) == 3.0
    assert K.get_median([-1.0, -3.0]) == -1.0
    for m, want in ((1, 1.0), (2, 2.0), (3, 2.0), (4, 3.0)):
        c = cases.make(cur_p=[[0.0, 0.0, float(z)] for z in range(m, 0, -1)])
        assert cases.run_reference(c)["median_depth"] == want and cases.run_reference(c)["min_depth"] == 1.0


def test_empty_lists_are_skipped_and_reported_as_zero_samples():
    r = ref(kf_p=np.zeros((0, 3)), cur_p=np.zeros((0, 3)), lkf=[[4.0, 3.2, 5.2]])
    assert r["n_px"] == 0 and r["n_depth"] == 0 and r["median_px"] == 0.0 and r["median_depth"] == 0.0 and r["min_depth"] == 0.0
    assert r["svo_kf"] == -1 and r["rule_mask"] == 0 and r["undefined"] == 0
    r = ref(kf_p=[[0.0, 0.0, 1.0]] * 3, kf_bad=[1, 1, 1], cur_p=[[0.0, 0.0, 2.0]] * 2, cur_bad=[1, 1], lkf=[[4.0, 3.2, 5.2]])
    assert r["n_px"] == 0 and r["n_depth"] == 0 and r["rule_mask"] == 0


def test_rotation_angle_of_a_known_rotation():
    a = 0.1
    T = np.array([[math.cos(a), -math.sin(a), 0, 0], [math.sin(a), math.cos(a), 0, 0], [0, 0, 1.0, 0]])
    r = ref(T_cur=T, params=K.KeyframeParams(min_rot=1.0, min_trans=1.0))
    assert abs(r["rot"] - 0.1) <= 4 * np.finfo(np.float64).eps and r["trans"] == 0.0 and r["rule_mask"] == 0
    r = ref(T_cur=T, params=K.KeyframeParams(min_rot=0.05, min_trans=1.0))
    assert r["rule_mask"] == 4


def test_a_point_at_the_camera_centre_is_undefined():
    r = ref(kf_p=[[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert r["undefined"] == 1


def test_negative_depths_order_below_positive_ones():
    r = ref(cur_p=[[0, 0, -3.0], [0, 0, 2.0], [0, 0, -1.0], [0, 0, 5.0], [0, 0, -7.0]])
    assert r["median_depth"] == -1.0 and r["min_depth"] == -7.0 and r["n_depth"] == 5


def test_declared_exported_and_mirrored(tmp_path):
    """The add-on library exports exactly what its own header declares, reads no environment; libdsdtm_amd.so is untouched."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_keyframe.h")).read()
    assert re.search(r"#define DSDTM_KF_MAX_POINTS 4096\b", hdr) and re.search(r"#define DSDTM_KF_MAX_LOCAL_KF 64\b", hdr)
    assert (capi.KF_MAX_POINTS, capi.KF_MAX_LOCAL_KF) == (4096, 64)
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(capi.KEYFRAME_SYMBOLS) and len(capi.KEYFRAME_SYMBOLS) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", capi.keyframe_lib_path()], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.strip()} == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", capi.keyframe_lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    strings = subprocess.run(["strings", "-n", "6", capi.keyframe_lib_path()], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bDSDTM_[A-Z0-9_]+", strings)
    lib = capi.load_keyframe()
    for sym, nargs in (("dsdtm_need_keyframe", 5), ("dsdtm_need_keyframes", 6)):
        assert re.search(r"\bint %s\(dsdtm_keyframe_ctx\*" % sym, hdr), sym
        assert len(getattr(lib, sym).argtypes) == nargs
    main = open(os.path.join(ROOT, "include", "dsdtm_amd.h")).read()
    assert "need_keyframe" not in main and not set(capi.KEYFRAME_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)
    # the layouts as a C compiler sees the header
    structs = [("dsdtm_keyframe_params", capi.KeyframeParams), ("dsdtm_keyframe_desc", capi.KeyframeDesc),
               ("dsdtm_keyframe_verdict", capi.KeyframeVerdict)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_keyframe.h"', 'int main(void) {']
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
    assert [n for n in capi.KEYFRAME_VERDICT_DTYPE.names] == [f for f, _ in capi.KeyframeVerdict._fields_]
    assert [capi.KEYFRAME_VERDICT_DTYPE.fields[f][1] for f, _ in capi.KeyframeVerdict._fields_] == \
        [getattr(capi.KeyframeVerdict, f).offset for f, _ in capi.KeyframeVerdict._fields_]


def test_header_documents_the_rules_and_quirks():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_keyframe.h")).read()
    block = hdr[hdr.index("---- Tracking::NeedKeyframe"):hdr.index("#define DSDTM_KF_MAX_POINTS")]
    for needle in ("src/Tracking.cpp:347-410", "floor(m / 2)", "31, not 30", "fabs of a", "include/Utils.h:34-40", "undefined"):
        assert needle in block, needle


def test_host_function_agrees_with_the_restatement(tmp_path):
    """need_keyframe_host (dsdtm_host.hpp: plain C++, no device call) through the compiled driver, on the exact-threshold cases and
    on random trackers of every shape class: the decisions equal, the medians bit-equal, the other quantities within 1e-9."""
    cs = [cases.EXACT[n]() for n in sorted(cases.EXACT)]
    shapes = [(1, 0, 0), (2, 30, 1), (63, 31, 10), (64, 32, 64), (65, 300, 10), (200, 300, 10), (4096, 300, 3)]
    for i, (a, b, l) in enumerate(shapes):
        for depth in ("positive", "negative", "mixed", "equal", "duplicates"):
            cs.append(cases.random_case(100 + i, a, b, l, depth=depth, bad="some" if i % 2 else "none", fire=(l - 1 if l and i % 2 else 0 if l else None)))
    got = cases.run_driver(tmp_path, cs, host_only=True)["host"]
    assert len(got) == len(cs)
    for i, (g, c) in enumerate(zip(got, cs)):
        want = cases.run_reference(c)
        if i >= len(cases.EXACT) and not want["undefined"]:
            assert min(cases.margins(c, want)) >= 1e-6, i
        cases.assert_same_verdict(g, want, i)
