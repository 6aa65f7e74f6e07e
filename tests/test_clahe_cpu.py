"""cv::CLAHE(3.0, 8x8) without a GPU: the restatement (dsdtm_amd/clahe_restatement.py, rules E1-E6 of include/dsdtm_amd_clahe.h) against
hand-computed tables, the host function (dsdtm_amd/host/dsdtm_clahe_host.hpp) bit for bit on every case of tests/clahe_cases.py, mutants of
the restatement each told apart by a named case, the surface of libdsdtm_amd_clahe.so, and the host side of the library under sanitizers
(tests/fake_hip_clahe/driver.cpp, a stand-alone program against the fake HIP runtime of tests/fake_hip; nothing is loaded into Python
under a sanitizer)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import clahe
from dsdtm_amd import clahe_restatement as R
from dsdtm_amd.csrc import build as hip_build
from tests import clahe_cases as cc
from tests import fake_hip_build as fhb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cc.host_library(tmp_path_factory.mktemp("clahe"))


def test_geometry_by_hand():
    """E1 with its quirk, E2 with its floor."""
    r = R.Clahe(3.0, 8, 8)
    assert r.padding(640, 480) == (0, 0) and r.padding(64, 50) == (8, 6) and r.padding(50, 64) == (6, 8) and r.padding(100, 50) == (4, 6)
    assert R.Clahe(3.0, 16, 16).padding(17, 16) == (15, 16)
    assert r.extended(cc.case("64x50")["img"]).shape == (56, 72)
    ext = R.Clahe(3.0, 16, 16).extended(cc.case("17x16 t16")["img"])
    img = cc.case("17x16 t16")["img"]
    assert ext.shape == (32, 32) and ext[0, 17] == img[0, 15] and ext[0, 31] == img[0, 1] and ext[16, 0] == img[14, 0] and ext[31, 0] == img[1, 0]   # 31 -> -1 -> 1
    assert r.clip(48) == 1 and int(3.0 * 48 / 256) == 0          # 64x48: the max(.., 1)
    assert r.clip(80 * 60) == 56 and r.clip(94 * 60) == 66 and R.Clahe(0.0).clip(4800) == 0 and R.Clahe(1e300).clip(4800) == 4800


def test_constant_tile_by_hand():
    """640x480 of 77: every tile holds 4800 pixels in bin 77. clip = 56, clipped = 4744, batch = 18, residual = 136: bins 0..135 hold 19,
    bin 77 holds 56 + 19 = 75, bins 136..255 hold 18. The cumulative sum at 77 is 78 * 19 + 56 = 1538, and 1538 * (255 / 4800) = 81.7 -> 82."""
    h = np.zeros(256, np.int32)
    h[77] = 4800
    got = R.Clahe().redistribute(h.copy(), 56)
    want = np.full(256, 18, np.int32)
    want[:136] += 1
    want[77] += 56
    assert (4800 - 56, 4744 // 256, 4744 - 18 * 256) == (4744, 18, 136) and np.array_equal(got, want) and got.sum() == 4800
    out, luts = cc.expected("640x480 constant")
    scale = F(255.0) / F(4800)
    by_hand = np.array([round(float(F(int(want[:i + 1].sum())) * scale)) for i in range(256)])          # (no product is near a half here)
    assert np.array_equal(luts[3, 5], by_hand) and luts[0, 0, 77] == 82 and luts[0, 0, 255] == 255 and (luts == luts[0, 0]).all()
    assert (out == 82).all()


def test_two_level_tile_by_hand():
    """A tile of 8 x 6 with 40 pixels of 10 and 8 of 200 under clip = 1 (64x48's floor): clipped = 39 + 7, batch = 0, residual = 46, so bins
    0..45 hold 1 (bin 10: 1 + 1), bin 200 holds 1. scale = 255 / 48 = 5.3125 exactly; cumsum 8 (at bin 6) gives 42.5 -> 42 (even) and
    cumsum 24 (bin 22) gives 127.5 -> 128: E5's halves."""
    img = np.full((48, 64), 10, np.uint8)
    img[:, 7::8] = 200          # the last column of every tile
    luts = R.clahe_luts(img, 3.0, 8, 8)
    h = np.zeros(256, np.int32)
    h[:46] = 1
    h[10] += 1
    h[200] += 1
    assert h.sum() == 48 and float(F(255.0) / F(48)) == 5.3125
    cum = np.cumsum(h)
    want = np.array([int(np.rint(c * 5.3125)) for c in cum])
    assert cum[6] == 7 and cum[7] == 8 and want[7] == 42 and 8 * 5.3125 == 42.5 and cum[22] == 24 and want[22] == 128 and 24 * 5.3125 == 127.5
    assert np.array_equal(luts[2, 3], want) and (luts == luts[0, 0]).all() and luts[0, 0, 255] == 255


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_function_is_bit_equal(host, name):
    out, luts = cc.expected(name)
    got, got_luts, got_luts2 = cc.run_host(host, cc.case(name))
    assert np.array_equal(got_luts, luts) and np.array_equal(got_luts2, luts), (name, int((got_luts != luts).sum()))
    assert np.array_equal(got, out), (name, int((got != out).sum()))


def test_cases_are_what_they_claim():
    shapes = {n: cc.case(n)["img"].shape for n in cc.NAMES}
    assert shapes["64x48"] == (48, 64) and shapes["17x16 t16"] == (16, 17) and shapes["752x480 real"] == (480, 752) and shapes["640x480 strided"] == (480, 640)
    assert cc.case("640x480 strided")["img"].strides[0] == 653 and cc.case("96x64 noclip")["clip_limit"] == 0.0
    # one tile: the interpolation is the identity over the table
    out, luts = cc.expected("96x64 t1")
    assert luts.shape == (1, 1, 256) and np.array_equal(out, luts[0, 0][cc.case("96x64 t1")["img"]])
    assert cc.expected("96x64 t3x5")[1].shape == (5, 3, 256)
    # the real image under the reference's parameters does something: the contrast of its darkest tile grows
    out, _ = cc.expected("752x480 real")
    img = cc.case("752x480 real")["img"]
    assert out.shape == img.shape and not np.array_equal(out, img) and int(out.max()) - int(out.min()) >= int(img.max()) - int(img.min())


class StridedResidual(R.Clahe):
    """OpenCV 3.x: the residual goes to every (256 / residual)-th bin"""
    def redistribute(self, h, clip):
        clipped = int(np.maximum(h - clip, 0).sum())
        h = np.minimum(h, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        h = h + batch
        if residual:
            step = max(256 // residual, 1)
            i = 0
            while i < 256 and residual > 0:
                h[i] += 1
                i += step
                residual -= 1
        return h


class TruncatedTable(R.Clahe):
    def table(self, h, area):
        return np.clip((np.cumsum(h, dtype=np.int32).astype(F) * (F(255.0) / F(area))).astype(np.int32), 0, 255).astype(np.uint8)


class TruncatedBlend(R.Clahe):
    def interpolate(self, img, luts):
        keep = self.round_u8
        self.round_u8 = lambda v: np.clip(v.astype(np.int32), 0, 255).astype(np.uint8)
        try:
            return super().interpolate(img, luts)
        finally:
            self.round_u8 = keep


class PadsOnlyTheSideThatDoesNotDivide(R.Clahe):
    def padding(self, width, height):
        return (self.tiles_x - width % self.tiles_x) % self.tiles_x, (self.tiles_y - height % self.tiles_y) % self.tiles_y


class NoHalfOffset(R.Clahe):
    def axis(self, n, tile, tiles):
        f = np.arange(n, dtype=F) * (F(1.0) / F(tile))
        fl = np.floor(f)
        i = fl.astype(np.int32)
        return np.minimum(np.maximum(i, 0), tiles - 1), np.minimum(i + 1, tiles - 1), f - fl


class NestedLerp(R.Clahe):
    def blend(self, p11, p12, p21, p22, xa, ya):
        one = F(1.0)
        top = p11 * (one - xa) + p12 * xa
        bottom = p21 * (one - xa) + p22 * xa
        return top * (one - ya) + bottom * ya


class ClipWithoutFloor(R.Clahe):
    def clip(self, area):
        return int(self.clip_limit * float(area) / 256.0) if self.clip_limit > 0 else 0          # 0 then reads as "no clipping"


# mutant -> the case that tells it apart
# (the constant image cannot tell the strided residual apart: its residual of 136 makes the stride 256 / 136 = 1)
MUTANTS = {StridedResidual: "640x480 two-level", TruncatedTable: "64x48", TruncatedBlend: "640x480 noise", PadsOnlyTheSideThatDoesNotDivide: "64x50",
           NoHalfOffset: "640x480 ramp", NestedLerp: "752x480 real", ClipWithoutFloor: "64x48"}


@pytest.mark.parametrize("mutant", list(MUTANTS), ids=lambda m: m.__name__)
def test_mutant_is_told_apart(mutant):
    c = cc.case(MUTANTS[mutant])
    got = R.clahe(c["img"], c["clip_limit"], c["tiles_x"], c["tiles_y"], cls=mutant)
    assert not np.array_equal(got, cc.expected(MUTANTS[mutant])[0]), mutant.__name__


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_clahe")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_clahe.cpp")], ["clahe_api.cpp"], include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    assert [l for l in lines if not l.startswith("ok refusal: ")] == ["ok answers_and_memory_kinds", "ok refusals", "ok call_failures", "ok create_failures"], lines
    refusals = {l[len("ok refusal: "):] for l in lines if l.startswith("ok refusal: ")}
    for needle in ("0..1024", "descs is NULL", "desc is NULL", "width out of range", "height out of range", "tiles_x out of range", "tiles_y out of range",
                   "clip_limit is not a finite number at or above 0", "src is NULL", "dst is NULL", "lut_out is NULL", "src_stride below width",
                   "dst_stride below width", "lut_out lies in device memory", "src of desc 2", "src of desc 4", "dst of desc", "lut_out overlaps dst of desc 0",
                   "lut_out of desc"):
        assert needle in refusals, (needle, refusals)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_and_exported():
    """libdsdtm_amd_clahe.so exports exactly the six symbols its header declares and reads no environment; the row stands in MORE_ADDONS;
    the library was cross-compiled by the build every test session runs."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_clahe.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(clahe.SYMBOLS) == {"dsdtm_clahe_create", "dsdtm_clahe_destroy", "dsdtm_clahe_last_error", "dsdtm_clahe_apply_batch",
                                              "dsdtm_clahe_apply", "dsdtm_clahe_luts"}
    assert os.path.exists(clahe.lib_path()) and not hip_build.addon_needs_build("clahe")
    assert _exported(clahe.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", clahe.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    assert "clahe" in hip_build.MORE_ADDONS and "clahe" not in hip_build.ADDONS
    assert hip_build.MORE_ADDONS["clahe"][0] == ["clahe_api.cpp", "clahe.hip"]
    assert not {"clahe.hip", "clahe.h", "clahe_api.cpp"} & set(hip_build.SOURCES + hip_build.HEADERS)
    for k, v in (("MIN_SIDE", 16), ("MAX_SIDE", 4096), ("MAX_TILES", 16), ("DEFAULT_TILES", 8), ("MAX_FRAMES", 1024)):
        assert re.search(r"#define DSDTM_CLAHE_%s %d\b" % (k, v), hdr) and getattr(clahe, k) == v and getattr(R, k) == v
    assert "#define DSDTM_CLAHE_DEFAULT_CLIP_LIMIT 3.0" in hdr and clahe.DEFAULT_CLIP_LIMIT == R.DEFAULT_CLIP_LIMIT == 3.0


def test_desc_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_clahe.h"', 'int main(void) {', '  printf("%zu", sizeof(dsdtm_clahe_desc));']
    src += [f'  printf(" %zu", offsetof(dsdtm_clahe_desc, {f[0]}));' for f in clahe.Desc._fields_] + ['  printf("\\n");', '  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    line = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout
    assert [int(v) for v in line.split()] == [C.sizeof(clahe.Desc)] + [getattr(clahe.Desc, f[0]).offset for f in clahe.Desc._fields_]


def test_header_and_readme_document_the_rules_and_the_parity():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_clahe.h")).read()
    for needle in ("Test/test_Feature_detection.cpp:85-86", "Test/test_Euroc.cpp:64-65", "Test/test_Optimizer.cpp:75-76", "THIS PROJECT'S DEFINITION",
                   "unpinned and stays unpinned", "QUIRK", "STRIDED RESIDUAL", "BORDER_REFLECT_101", "2^24", "halves to even", *["E%d " % i for i in range(1, 8)]):
        assert needle.strip() in hdr, needle
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "libdsdtm_amd_clahe.so" in readme and "unpinned" in readme[readme.index("libdsdtm_amd_clahe.so"):]


def test_adapter_builds_and_runs_on_the_host_path(tmp_path):
    """dsdtm_amd/host/dsdtm_clahe_host.hpp's DSDTM::CLAHE with on_device = false: the drivers' two lines, equal to clahe_host."""
    src = tmp_path / "adapter.cpp"
    src.write_text('#include "dsdtm_clahe_host.hpp"\n#include <cstdio>\nint main() {\n  const int W = 100, H = 50;\n  std::vector<uint8_t> a(W * H), b(W * H, 0), c(W * H, 1);\n'
                   '  for (int i = 0; i < W * H; ++i) a[i] = (uint8_t)((i * 7 + i / W * 13) % 200);\n'
                   '  DSDTM::CLAHE clahe(3.0, 8, 8, false);\n  clahe.apply(DSDTM::GrayImage{a.data(), W, H, W}, DSDTM::GrayImage{b.data(), W, H, W});\n'
                   '  DSDTM::clahe_host(a.data(), W, c.data(), W, W, H);\n  int bad = 0;\n  try { clahe.apply(DSDTM::GrayImage{a.data(), 8, 8, 8}, DSDTM::GrayImage{b.data(), 8, 8, 8}); } catch (const std::exception&) { bad = 1; }\n'
                   '  std::printf("%d %d %d\\n", b == c ? 1 : 0, b != a ? 1 : 0, bad);\n  return 0;\n}\n')
    exe = tmp_path / "adapter"
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-DDSDTM_CLAHE_HOST_ONLY=1", "-I", os.path.join(ROOT, "dsdtm_amd", "host"),
                    str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["1", "1", "1"]


def test_example_compiles(tmp_path):
    """dsdtm_amd/host/example_clahe.cpp against the headers (linking needs the libraries and a HIP runtime: the GPU test runs it)."""
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++14", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "dsdtm_amd", "host", "example_clahe.cpp")], check=True)
