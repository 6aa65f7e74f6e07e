"""The moving-object mask without a GPU: the numpy restatement (dsdtm_amd/motion_restatement.py) against its C twin
(tests/motion_restatement.c) bit for bit, the 5x5 median against a brute-force np.median, mutants of the restatement each told apart
by a committed world, the exports of libdsdtm_amd_motion.so, and the host side of the library under sanitizers
(tests/fake_hip_motion/driver.cpp, a stand-alone program against the fake HIP runtime of tests/fake_hip; nothing is loaded into
Python)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import capi, motion
from dsdtm_amd import motion_restatement as R
from tests import fake_hip_build as fhb
from tests import motion_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "real"])
def test_numpy_and_c_restatements_are_bit_equal(tmp_path_factory, name):
    lib = mc.c_twin(tmp_path_factory.getbasetemp())
    wd = mc.world(name)
    for s, (a, b) in enumerate(zip(mc.trace_of(name), mc.run_world_c(lib, wd))):
        assert np.array_equal(a["gray"], b["gray"]), (name, s)
        assert np.array_equal(_bits(a["after"]), _bits(b["after"])), (name, s)
        assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(_bits(a["dist"]), _bits(b["dist"])), (name, s)
        assert np.array_equal(a["exp_arg"], b["exp_arg"]) and int(a["stale"].sum()) == b["n_stale"], (name, s)


def test_init_is_zeros_then_one_step_on_a_zero_image(tmp_path_factory):
    m = R.ProbModel(64, 48)
    st = m.state.reshape(6, 2, -1)
    # By hand: compensation leaves every age 0 and var 900 (225 on the border); "oldest to 0" picks mode 1 (0 >= 0): mode 0 receives
    # it, mode 1 becomes (0, 225, 0); (0 - 0)^2 < 2 var: mode 0 matches, at age 0: mean = obs = 0, var = MAX(0, INIT_BG_VAR), age 1;
    # mode 1 keeps its _Temp entries (0, 225, 0)
    assert (st[0] == 0).all() and (st[1, 0] == 225).all() and (st[1, 1] == 225).all()
    assert (st[2, 0] == 1).all() and (st[2, 1] == 0).all()
    assert (st[3] == 0).all() and (st[4, 1] == 225).all() and (st[5] == 0).all()
    assert sorted(set(st[4, 0].tolist())) == [225.0, 900.0]                                      # border / interior
    lib = mc.c_twin(tmp_path_factory.getbasetemp())
    c = np.full((12, m.nc), 7, np.float32)
    lib.motion_model_init(c.ctypes.data, 64, 48)
    assert np.array_equal(_bits(c), _bits(m.state))


@pytest.mark.parametrize("shape", [(16, 16), (21, 19), (48, 64)])
def test_median_against_brute_force(tmp_path_factory, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    img = rng.integers(0, 256, size=shape).astype(np.uint8)
    img[:3, :3] = [[9, 200, 9], [200, 9, 200], [9, 200, 9]]         # make the four corners depend on the replication
    img[-2:, -2:] = [[255, 0], [0, 255]]
    img[0, -1], img[-1, 0] = 255, 0
    pad = np.pad(img, 2, mode="edge")
    want = np.empty_like(img)
    for y in range(shape[0]):
        for x in range(shape[1]):
            want[y, x] = int(np.median(pad[y:y + 5, x:x + 5]))        # 25 values: the median is an element
    got = R.median5(img)
    assert np.array_equal(got, want)
    for y, x in ((0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1)):
        assert got[y, x] == want[y, x]
    lib = mc.c_twin(tmp_path_factory.getbasetemp())
    strided = np.zeros((shape[0], shape[1] + 11), np.uint8) + 77
    strided[:, :shape[1]] = img
    out = np.zeros(shape, np.uint8)
    lib.motion_median5(strided.ctypes.data, shape[1], shape[0], strided.strides[0], out.ctypes.data)
    assert np.array_equal(out, want)


# ---- mutants: one deviation each; every one must be told apart from the faithful restatement by a committed world ----
class TempZeroedPerStep(R.ProbModel):
    def begin_step(self):
        self.state[6:] = 0


class CompensationReadsUpdatedModel(R.ProbModel):
    def run_cells(self, px, H, out):
        for c in range(self.nc):                      # row-major, in place: earlier cells are already updated
            self._cells(np.array([c]), self.state, px, H, out)


class StrictOldestPick(R.ProbModel):
    def mode1_is_oldest(self, age1, old_age):
        return age1 > old_age


class TrueSwap(R.ProbModel):
    def oldest_to_front(self, pick, t, cur_mean):
        for arr in (R.MEAN_T, R.VAR_T, R.AGE_T):
            a, b = t[arr].copy(), t[arr + 1].copy()
            t[arr], t[arr + 1] = np.where(pick, b, a), np.where(pick, a, b)


class MaskOnPostUpdateVariance(R.ProbModel):
    def mask_variance(self, var_temp0, var_new0):
        return var_new0


class PowRoundedToFloat(R.ProbModel):
    def square(self, d):
        return (d * d).astype(f32).astype(f64)


class BorderBelowZero(R.ProbModel):
    def on_border(self, iI, iJ):
        return (iI < 0) | (iI >= self.mw - 1) | (iJ < 0) | (iJ >= self.mh - 1)


# mutant -> the world that tells it apart
MUTANTS = {TempZeroedPerStep: "B", CompensationReadsUpdatedModel: "B", StrictOldestPick: "A", TrueSwap: "A",
           MaskOnPostUpdateVariance: "A", PowRoundedToFloat: "D", BorderBelowZero: "C"}


def _differs(a, b):
    return any(not np.array_equal(_bits(x["after"]), _bits(y["after"])) or not np.array_equal(x["mask"], y["mask"]) for x, y in zip(a, b))


@pytest.mark.parametrize("mutant", list(MUTANTS), ids=lambda m: m.__name__)
def test_mutant_is_told_apart(mutant):
    name = MUTANTS[mutant]
    assert _differs(mc.trace_of(name), mc.run_world(mc.world(name), model_class=mutant)), (mutant.__name__, name)


def test_truncation_instead_of_cvround_is_told_apart():
    px, want = mc.features("A")
    mask = mc.trace_of("A")[-1]["mask"]
    assert np.array_equal(R.MotionRestatement.features_on_mask(mask, px), want)
    trunc = R.MotionRestatement.features_on_mask(mask, px, round_fn=lambda v: np.asarray(v, f32).astype(np.int64))
    assert not np.array_equal(trunc, want)
    # half to even: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0
    assert list(R.cv_round([0.5, 1.5, 2.5, 3.5, 62.5])) == [0, 2, 2, 4, 62]


def test_worlds_are_what_they_claim():
    for name in "ABC":          # exp is only ever handed 0: the device must be bit-equal there
        assert all(not mc.exp_cells(t).any() for t in mc.trace_of(name)), name
    assert any((t["mask"] == 255).any() for t in mc.trace_of("A")) and any((t["mask"] == 255).any() for t in mc.trace_of("C"))
    b = mc.trace_of("B")
    assert b[1]["stale"].any() and (b[1]["stale"] & b[2]["stale"]).any()          # sumW == 0 twice running in the same cells
    c = mc.trace_of("C")[-1]["mask"]
    assert not c[48:, :].any() and not c[:, 68:].any()                            # beyond 4 * the model grid
    d, wd = mc.trace_of("D"), mc.world("D")
    assert sum(int(mc.exp_cells(t).sum()) for t in d) >= 0.05 * len(d) * d[0]["stale"].size
    excused = sum(int(mc.excusable_pixels(wd, t).sum()) for t in d)
    assert excused < mc.MAX_EXCUSED_SHARE * len(d) * wd["width"] * wd["height"], excused


def test_declared_and_exported():
    """libdsdtm_amd_motion.so exports exactly what its header declares and reads no environment; libdsdtm_amd.so is untouched."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_motion.h")).read()
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(motion.SYMBOLS) and len(motion.SYMBOLS) == 10
    out = subprocess.run(["nm", "-D", "--defined-only", motion.lib_path()], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.strip()} == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", motion.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    for k, v in (("MIN_SIDE", 16), ("MAX_SIDE", 4096), ("MAX_FEATURES", 16384), ("STEPS_MAX", 1024)):
        assert re.search(r"#define DSDTM_MOTION_%s %d\b" % (k, v), hdr) and getattr(motion, k) == v
    main = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path(False)], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in main.splitlines() if l.strip()}
    assert len(names) == 38 and names == set(capi.EXPORTED_SYMBOLS) and not any("motion" in n for n in names)
    lib = motion.load()
    assert len(lib.dsdtm_motion_step.argtypes) == 10 and len(lib.dsdtm_motion_steps.argtypes) == 3


def test_desc_layout(tmp_path):
    """dsdtm_motion_desc as a C compiler lays it out, against the ctypes mirror."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_motion.h"', 'int main(void) {',
           '  printf("%zu", sizeof(dsdtm_motion_desc));']
    src += [f'  printf(" %zu", offsetof(dsdtm_motion_desc, {f}));' for f, _ in motion.Desc._fields_] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(motion.Desc)] + [getattr(motion.Desc, f).offset for f, _ in motion.Desc._fields_]


def test_header_documents_the_scope_and_the_traps():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_motion.h")).read()
    for needle in ("MCDWrapper.cpp:65-137", "prob_model.h:121-167", "ZEROS ARE THIS PROJECT'S DEFINITION", "COMMENTED OUT (src/Tracking.cpp:230)",
                   "findHomography", ":98-128", "KLTWrapper", "Mod_FrameDiff", "HALVES TO EVEN", "2^30", "is not a swap", "src/Frame.cpp:352"):
        assert needle in hdr, needle


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "fake_hip_motion")
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_motion.cpp")], ["motion_api.cpp"],
                           include_dirs=[here])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok step_failures", "ok model_failures", "ok batch_rules", "ok argument_checks", "ok create_failures"], lines
