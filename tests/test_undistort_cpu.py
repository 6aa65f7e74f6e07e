"""libdsdtm_amd_undistort.so without a GPU: the numpy restatement (dsdtm_amd/undistort_restatement.py) against the host functions of
dsdtm_amd/host/dsdtm_undistort_host.hpp (a stand-alone driver, tests/undistort_host/driver.cpp) bit for bit on every case, the map
included; the cases' own properties; two deliberately wrong variants of the restatement told apart by named cases; the round trip through
the forward model; the surface of the library; and its host side under sanitizers (tests/fake_hip_undistort/driver.cpp, a stand-alone
program over the fake HIP runtime of tests/fake_hip; nothing is loaded into Python)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import keyframe_creation_restatement as KR
from dsdtm_amd import undistort
from dsdtm_amd import undistort_restatement as R
from dsdtm_amd.csrc import build as hip_build
from tests import fake_hip_build as fhb
from tests import undistort_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_answers(tmp_path_factory):
    """Every case through undistort_map_host / undistort_frame_host / undistort_points_host, once."""
    d = tmp_path_factory.mktemp("undistort_host")
    exe = str(d / "driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "undistort_host", "driver.cpp")], check=True)
    (d / "cases.bin").write_bytes(uc.pack())
    subprocess.run([exe, str(d / "cases.bin"), str(d / "answers.bin")], check=True)
    frames, points = uc.unpack((d / "answers.bin").read_bytes())
    return dict(zip(uc.FRAME_NAMES, frames)), dict(zip(uc.POINT_NAMES, points))


def test_case_lists():
    assert [c["name"] for c in uc.frame_cases()] == uc.FRAME_NAMES and [c["name"] for c in uc.point_cases()] == uc.POINT_NAMES


@pytest.mark.parametrize("name", uc.FRAME_NAMES)
def test_host_frames_equal_the_restatement(host_answers, name):
    c, got, want = uc.frame_case(name), host_answers[0][name], uc.expected_frame(name)
    w = c["w"]
    assert uc.same_bits(got["map"], want["map"])
    assert uc.same_bits(got["gray"][:, :w], want["gray"]) and (got["gray"][:, w:] == 0xA5).all()          # nothing outside a row
    if c["depth"] is None:
        assert got["depth"] is None and want["depth"] is None
    else:
        assert uc.same_bits(got["depth"][:, :w], want["depth"]) and (got["depth"][:, w:] == 0xA5A5).all()


@pytest.mark.parametrize("name", uc.POINT_NAMES)
def test_host_points_equal_the_restatement(host_answers, name):
    got, want = host_answers[1][name], uc.expected_points(name)
    assert uc.same_bits(got["px"], want["px"]) and uc.same_bits(got["bearing"], want["bearing"])


def _outside_counts(name):
    c = uc.frame_case(name)
    return np.bincount(R.taps_outside(uc.expected_frame(name)["map"], c["w"], c["h"]).ravel(), minlength=5)


def test_cases_have_the_properties_they_are_named_for():
    # identity: dst == src, byte for byte
    c, e = uc.frame_case("identity"), uc.expected_frame("identity")
    assert np.array_equal(e["gray"], c["gray"]) and np.array_equal(e["depth"], c["depth"]) and c["dist"] == uc.ZERO
    xs, ys = np.meshgrid(np.arange(c["w"]), np.arange(c["h"]))
    assert np.array_equal(e["map"][..., 0], xs * 32) and np.array_equal(e["map"][..., 1], ys * 32)
    # tail_widths: all four remainders of the 4-pixel thread, strides above the width and all different
    tails = [uc.frame_case(f"tail_widths_{w}") for w in (37, 38, 39, 40)]
    assert sorted(t["w"] % 4 for t in tails) == [0, 1, 2, 3]
    for t in tails:
        strides = [t["gray"].base.shape[1], t["gd"], t["depth"].base.shape[1], t["zd"]]
        assert all(s > t["w"] for s in strides) and len(set(strides)) == 4
    # barrel_strong: the taps leave the image on all four sides; zeros at the border; partial taps. A 2 x 2 window meets a rectangle in
    # a rectangle of 4, 2, 1 or 0 pixels, so 2 (an edge) and 3 (a corner) taps outside are the partial counts that EXIST — exactly 1
    # outside cannot occur for any map, which the last line holds every case to.
    c, e = uc.frame_case("barrel_strong"), uc.expected_frame("barrel_strong")
    X, Y = e["map"][..., 0].astype(np.int64), e["map"][..., 1].astype(np.int64)
    assert (X >> 5).min() < -1 and (X >> 5).max() > c["w"] and (Y >> 5).min() < -1 and (Y >> 5).max() > c["h"]
    n_out = _outside_counts("barrel_strong")
    assert n_out[2] > 0 and n_out[3] > 0 and n_out[4] > 0 and n_out[0] > 0
    assert (e["gray"][0] == 0).all() and (e["gray"][-1] == 0).all() and (e["gray"][:, 0] == 0).all() and (e["gray"][:, -1] == 0).all()
    assert all(_outside_counts(n)[1] == 0 for n in uc.FRAME_NAMES)
    # pincushion: the sources compress (every tap inside, the source extent smaller than the image)
    e = uc.expected_frame("pincushion")
    assert _outside_counts("pincushion")[1:].sum() == 0 and (e["map"][..., 0] >> 5).min() > 2 and (e["map"][..., 0] >> 5).max() < 61
    # tangential_only: asymmetric — the map of the mirrored pixel is not the mirrored map
    c, e = uc.frame_case("tangential_only"), uc.expected_frame("tangential_only")
    assert c["dist"][0] == c["dist"][1] == c["dist"][4] == 0.0
    assert not np.array_equal(e["map"][:, ::-1, 0], (c["w"] - 1) * 32 - e["map"][..., 0])
    # kinect_yaml: the reference's numbers, held by a hash and 64 spot pixels
    c = uc.frame_case("kinect_yaml")
    assert (c["w"], c["h"]) == (640, 480) and c["dist"] == (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
    assert uc.kinect_digest() == uc.KINECT_SHA256 and uc.kinect_spots() == (uc.KINECT_SPOTS_GRAY, uc.KINECT_SPOTS_DEPTH)
    assert (uc.frame_case("min_side")["w"], uc.frame_case("min_side")["h"]) == (R.MIN_SIDE, R.MIN_SIDE)
    # depth_edges: nearest neighbour never invents a value
    c, e = uc.frame_case("depth_edges"), uc.expected_frame("depth_edges")
    assert set(np.unique(c["depth"]).tolist()) == {0, 1000, 3000, 65535}
    assert set(np.unique(e["depth"]).tolist()) <= {0, 1000, 3000, 65535} and {1000, 3000, 65535} <= set(np.unique(e["depth"]).tolist())
    assert uc.frame_case("gray_only")["depth"] is None and uc.frame_case("depth_given")["depth"] is not None
    # points: a 7 x 5 grid, alternating skips over more than one block, pixels at and outside the border
    assert len(uc.point_case("pts_grid")["px"]) == 35 and len(uc.point_case("pts_skip")["px"]) > 256
    assert uc.point_case("pts_skip")["skip"][:4].tolist() == [0, 1, 0, 1]
    b = uc.point_case("pts_border")["px"]
    assert (b.min(axis=0) < 0).all() and b[:, 0].max() > 640 and b[:, 1].max() > 480 and [0.0, 0.0] in b.tolist() and [639.0, 479.0] in b.tolist()


def test_points_rules():
    # skipped pixels are copied and their bearings stay; the others move
    c, e = uc.point_case("pts_skip"), uc.expected_points("pts_skip")
    sk = c["skip"] != 0
    assert uc.same_bits(e["px"][sk], c["px"][sk]) and (e["bearing"][sk] == uc.BEARING_FILL).all()
    assert (e["px"][~sk] != c["px"][~sk]).any(axis=1).mean() > 0.9 and np.allclose(np.linalg.norm(e["bearing"][~sk], axis=1), 1.0, atol=1e-15)
    # zero distortion: the output equals the input as float, the bearings are the newkf rule's
    c, e = uc.point_case("pts_zero_dist"), uc.expected_points("pts_zero_dist")
    assert uc.same_bits(e["px"], c["px"])
    want = np.array([KR.bearing_of(c["cam"][:4], float(p[0]), float(p[1])) for p in c["px"]], np.float64)
    assert uc.same_bits(e["bearing"], want)
    # the principal point does not move
    e, c = uc.expected_points("pts_border"), uc.point_case("pts_border")
    assert np.array_equal(e["px"][8], c["px"][8])


def test_round_trip_through_the_forward_model():
    """distort-then-undistort of pts_grid: the ideal pixel p goes through U1's forward model (steps 1-6, float64) to the distorted pixel,
    which is narrowed to float32 and handed to U5. Measured with the restatement: the largest |U5(forward(p)) - p| over the 35 pixels is
    4.49e-2 px (kinect_yaml coefficients, at the grid's corners, r2 = 0.5; the five fixed iterations leave it: with fifty the
    residual is float32 storage alone, one ulp at ~600 px being 6.1e-5). Asserted with a 2x margin."""
    c = uc.point_case("pts_grid")
    (fx, fy, cx, cy), _ = R.model(c["cam"], c["dist"])
    p = c["px"].astype(np.float64)
    mx, my = R.forward(c["cam"], c["dist"], (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy)
    back, _ = R.undistort_points(c["cam"], c["dist"], np.stack([mx, my], axis=1).astype(np.float32))
    err = np.abs(back.astype(np.float64) - p).max()
    print(f"round trip residual {err:.3e} px")
    assert err <= 2 * ROUND_TRIP_MEASURED, err
    # and it is the iteration count that leaves it: fifty iterations come back to float32 precision
    back50, _ = R.undistort_points(c["cam"], c["dist"], np.stack([mx, my], axis=1).astype(np.float32), iterations=50)
    assert np.abs(back50.astype(np.float64) - p).max() <= 2 * 6.2e-5


ROUND_TRIP_MEASURED = 4.49e-2         # px; see the test above and DESIGN 1.1k


# ---- non-vacuity: a wrong restatement is told apart by named cases
def test_truncation_instead_of_cvround_is_told_apart():
    for name in ("barrel_strong", "kinect_yaml", "tangential_only"):
        c = uc.frame_case(name)
        wrong = R.undistort_map(c["cam"], c["dist"], c["w"], c["h"], rounding=uc.truncating_round)
        assert not np.array_equal(wrong, uc.expected_frame(name)["map"]), name
        assert not np.array_equal(R.remap_gray(wrong, c["gray"]), uc.expected_frame(name)["gray"]), name


def test_no_rounding_bias_in_the_remap_is_told_apart():
    for name in ("barrel_strong", "pincushion", "kinect_yaml", "min_side"):
        c, e = uc.frame_case(name), uc.expected_frame(name)
        assert not np.array_equal(uc.remap_gray_no_bias(e["map"], c["gray"]), e["gray"]), name
    e = uc.expected_frame("identity")          # (where every weight is 0 or 32 the bias cannot show: the identity case does not tell)
    assert np.array_equal(uc.remap_gray_no_bias(e["map"], uc.frame_case("identity")["gray"]), e["gray"])


def test_rounding_and_saturation_of_the_map():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.0e9, -3.0e9, 2147483646.5, np.inf, -np.inf, np.nan])
    assert R.cv_round_sat(v).tolist() == [0, 2, 2, 0, -2, 2**31 - 1, -2**31, 2**31 - 2, R.OUTSIDE, R.OUTSIDE, R.OUTSIDE]
    # a sentinel and both saturated ends read as outside in U2 and U3, without overflow in (X + 16) >> 5
    m = np.array([[[R.OUTSIDE, 0], [2**31 - 1, 2**31 - 1], [-2**31, 40], [33, 2**31 - 1]]], np.int32)
    src = np.full((1, 4), 200, np.uint8)
    assert R.remap_gray(m, src).tolist() == [[0, 0, 0, 0]] and R.remap_depth(m, src.astype(np.uint16)).tolist() == [[0, 0, 0, 0]]


# ---- the surface
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_and_exported():
    """libdsdtm_amd_undistort.so exports exactly the 8 symbols its header declares, shares none with any other library and reads no
    environment; the other libraries export what they exported."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_undistort.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(undistort.SYMBOLS) and len(undistort.SYMBOLS) == 8 and len(set(undistort.SYMBOLS)) == 8
    assert _exported(undistort.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", undistort.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    counts = {"": 38, "keyframe": 5, "motion": 10, "homography": 5, "localmap": 10, "trackmap": 11, "mapping": 14, "newkf": 5, "slam": 16, "undistort": 8}
    assert list(hip_build.ADDONS) == [k for k in counts if k]
    for name, n in counts.items():
        names = _exported(hip_build.ADDONS[name][2] if name else hip_build.OUT)
        assert len(names) == n, (name, len(names))
        if name != "undistort":
            assert not (names & declared) and not any("undistort" in s for s in names), name
    for k, v in (("MIN_SIDE", 8), ("MAX_SIDE", 4096), ("MAX_FRAMES", 1024), ("MAX_POINTS", 16384)):
        assert re.search(r"#define DSDTM_UNDISTORT_%s %d\b" % (k, v), hdr) and getattr(undistort, k) == v and getattr(R, k) == v
    assert "#define DSDTM_UNDISTORT_OUTSIDE (-2147483647 - 1)" in hdr and undistort.OUTSIDE == R.OUTSIDE == -2**31
    lib = undistort.load()
    assert len(lib.dsdtm_undistort_frames.argtypes) == 3 and len(lib.dsdtm_undistort_points.argtypes) == 8 and len(lib.dsdtm_undistort_map_create.argtypes) == 4


def test_desc_layout(tmp_path):
    """dsdtm_undistort_desc as a C compiler lays it out, against the ctypes mirror."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_undistort.h"', 'int main(void) {', '  printf("%zu", sizeof(dsdtm_undistort_desc));']
    src += [f'  printf(" %zu", offsetof(dsdtm_undistort_desc, {f[0]}));' for f in undistort.Desc._fields_] + ['  printf("\\n");', '  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    line = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout
    assert [int(v) for v in line.split()] == [C.sizeof(undistort.Desc)] + [getattr(undistort.Desc, f[0]).offset for f in undistort.Desc._fields_]


def test_header_documents_the_parity_and_the_definitions():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_undistort.h")).read()
    for needle in ("src/Frame.cpp:57-61", "src/Frame.cpp:94-150", "src/Tracking.cpp:149", ":417", "src/Camera.cpp:62-67", "src/Frame.cpp:141-142",
                   "OpenCV is not available to this project, in source or binary", "THIS PROJECT'S DEFINITION", "unpinned and stays", "U1 the map",
                   "U2 gray", "U3 depth", "U4 frames", "U5 points", "the reference never remaps", "INTER_BITS = 5", "halves to even", "exactly FIVE times",
                   "include/dsdtm_amd_newkf.h", "is NOT restated", "defined for RECTIFIED images", "SYNCHRONOUS ON PURPOSE", "byte-equal to its single",
                   "NO CPU fallback"):
        assert needle in hdr, needle
    newkf = open(os.path.join(ROOT, "include", "dsdtm_amd_newkf.h")).read()          # that header's two sentences stay as they are
    assert "is NOT restated" in newkf and "RECTIFIED images" in newkf


def test_example_compiles():
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "dsdtm_amd", "host", "example_undistort.cpp")], check=True)
    src = open(os.path.join(ROOT, "dsdtm_amd", "host", "example_undistort.cpp")).read()
    assert "rectify(" in src and "dsdtm_frame_prefetch(" in src and "dsdtm_track_frame_on(" in src


def test_tracker_without_a_distortion_is_untouched():
    """The Python adapters: nothing happens unless a distortion is given."""
    from dsdtm_amd import synth, tracking
    from dsdtm_amd.frame import Frame

    class _Ctx:
        device = 0
    cam = synth.Camera.tum(64, 48)
    t = tracking.Tracker(cam, ctx=_Ctx(), max_level=3, min_level=0, max_iters=5)
    assert t.distortion is None
    f = Frame(cam, [np.zeros((48, 64), np.uint8)], np.eye(4)[:3])
    px = np.array([[10.5, 7.25], [40.0, 30.0]], np.float32)
    b = synth.bearing_from_px(cam, px)
    f.set_features(px.copy(), b.copy(), b * 2.0, np.array([0, 1], np.uint8))
    t.UndistortFeatures(f)
    assert uc.same_bits(f.px, px) and uc.same_bits(f.bearing, b)
    with pytest.raises(ValueError):
        t.prefetch_raw(np.zeros((48, 64), np.uint8))
    # product code does not import the tests' yardstick
    for mod in ("tracking.py", "undistort.py"):
        assert not re.search(r"^\s*(from|import)\b.*undistort_restatement", open(os.path.join(ROOT, "dsdtm_amd", mod)).read(), flags=re.M)


# ---- the host side under sanitizers
def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_undistort")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_undistort.cpp")],
                           ["undistort_api.cpp"], include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok answers_and_memory_kinds", "ok refusals", "ok call_failures", "ok create_failures"], lines
