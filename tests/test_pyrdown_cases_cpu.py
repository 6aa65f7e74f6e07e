"""Holds the cases of tests/pyrdown_cases.py to their conditions, with the oracle alone: every layout is one
dsdtm_pyrdown_batch_device accepts, the bytes the call may write and level 0 are apart, the oracle's chain on the strided
buffer reads no padding, and the case list reaches every branch of dsdtm_amd/csrc/pyrdown.hip that depends on the caller's
layout (the restatements in pyrdown_cases classify; they are no oracle). The device runs the same cases in
tests/test_pyrdown_gpu.py."""
import numpy as np
import pytest

from dsdtm_amd import synth
from tests import pyrdown_cases as PC


@pytest.mark.parametrize("name", PC.NAMES)
def test_layout_buffer_and_oracle_chain(oracle, name):
    b = PC.build(name)
    c = b.case
    # the entry's own conditions: stride >= w, off + stride * h <= pitch, the child level is ((w + 1) / 2, (h + 1) / 2)
    assert PC.table_is_valid(b)
    assert (b.ws[0], b.hs[0]) == (c.w, c.h) and len(b.ws) == c.levels and 1 <= c.n
    assert b.host.size == b.base_shift + c.n * b.pitch + PC.SPARE and c.n * c.w * c.h <= 1200000
    # what may be written, level 0, and everything else
    assert not (b.writable & b.level0).any()
    assert b.writable.sum() == c.n * sum(w * h for w, h in zip(b.ws[1:], b.hs[1:])) and b.level0.sum() == c.n * c.w * c.h
    assert not b.writable[b.base_shift + c.n * b.pitch:].any() and not b.writable[:b.base_shift].any()
    free = ~b.writable & ~b.level0
    assert np.isin(b.host[free], (PC.POISON, 0x00, 0xFF)).all() and (b.host[b.writable] == PC.POISON).all()
    for i in range(c.n):
        assert np.array_equal(b.level(b.host, i, 0), b.images[i])
    if b.strides[0] >= c.w + 4 and c.h >= 3:                             # row padding: both guard values stand next to rows
        row = b.base_shift + b.offs[0]
        assert (b.host[row + c.w:row + c.w + 4] == 0x00).all() and (b.host[row + 2 * b.strides[0] - 4:row + 2 * b.strides[0]] == 0xFF).all()
        assert (b.host[row + b.strides[0] + c.w:row + 2 * b.strides[0] - 4] == PC.POISON).all()
    # the oracle on the strided buffer == the numpy restatement on contiguous copies: no padding byte is read
    want = PC.expected(oracle, name)
    assert np.array_equal(want[~b.writable], b.host[~b.writable])
    for i in range(c.n):
        for l in range(1, c.levels):
            assert np.array_equal(b.level(want, i, l), synth.pyrdown_u8(np.ascontiguousarray(b.level(want, i, l - 1)))), (i, l)
    if c.n >= 2:
        assert all((b.level(want, c.n - 1, l) == 255).all() for l in range(c.levels))


def test_every_path_of_the_strip_kernel_has_a_case():
    classes = {n: PC.strip_classes(PC.build(n)) for n in PC.NAMES}
    all_fast = [n for n, k in classes.items() if all(v == {"fast"} for v in k.values())]
    all_generic = [n for n, k in classes.items() if all(v == {"generic"} for v in k.values())]
    mixed = [n for n, k in classes.items() if any(v == {"fast", "generic"} for v in k.values())]
    assert "16x9_L2_packed" in all_fast and "24x12_L2_off4" in all_fast and "64x37_L3_padded4" in all_fast
    assert {"18x9_L2_packed", "20x12_L2_packed", "16x9_L2_odd_stride", "24x12_L2_off1", "16x3_L2_packed", "5x1_L2_packed",
            "636x38_L3_packed"} <= set(all_generic)                      # (packed 636: level 1 has a stride of 318)
    assert {"18x9_L2_rounded4", "20x9_L2_rounded4", "22x12_L2_rounded4", "30x9_L2_rounded4", "636x38_L3_rounded4", "642x21_L3_rounded4",
            "634x10_L3_rounded4"} <= set(mixed)
    # more than one wave of strips with both paths among them
    for n in ("636x38_L3_rounded4", "642x21_L3_rounded4", "634x10_L3_rounded4"):
        t = PC.fast_terms(PC.build(n), 0, 0)
        assert len(t) > 64 and all(all(x) for x in t[:-1]) and not all(t[-1])
    # images of one batch on different paths: an image base that is 2 modulo 4
    k = classes["64x37_L3_pitch2"]
    assert k[(0, 0)] == {"fast"} and k[(1, 0)] == {"generic"} and k[(2, 0)] == {"fast"}
    # the interior strip that loads columns sw and sw + 1 (width 2 modulo 8), the right strip that mirrors column sw (0 modulo 8)
    for n, sw in (("18x9_L2_rounded4", 18), ("24x12_L2_packed", 24)):
        x4 = max(4 * s for s, t in enumerate(PC.fast_terms(PC.build(n), 0, 0)) if all(t))
        assert 2 * x4 - 4 + 16 == sw + (2 if sw % 8 == 2 else 4)
    # image counts: 1, 3, 5, 9 and the batch of 32; workgroups x images both a multiple of 8 and not (the XCD renumbering)
    assert {1, 3, 5, 9, 32} <= {PC.CASES[n].n for n in PC.NAMES}
    assert 60 <= len(PC.NAMES) <= 85


# term -> (case, the exact set of false terms some strip of it has). For an even width `x4 + 3 < dw` and the right-edge rule are
# the same condition (2 x4 + 8 <= sw), so they are false together; the right-edge rule alone is false only at an odd width.
ISOLATED = {
    "sstride & 3": ("16x9_L2_stride2_l0", {"sstride & 3"}),
    "source alignment": ("16x9_L2_off1_l0", {"source alignment"}),
    "sw & 1": ("17x9_L2_rounded4", {"sw & 1"}),
    "sw >= 16": ("14x9_L2_rounded4", {"sw >= 16"}),
    "sh >= 4": ("16x3_L2_packed", {"sh >= 4"}),
    "x4 + 3 < dw": ("20x9_L2_rounded4", {"x4 + 3 < dw", "right edge"}),
    "right edge": ("23x9_L2_rounded4", {"sw & 1", "right edge"}),
    "destination alignment": ("16x9_L2_off1_l1", {"destination alignment"}),
    "dstride & 3": ("16x9_L2_stride2_l1", {"dstride & 3"}),
}


def test_every_term_of_the_fast_predicate_is_false_on_its_own_somewhere():
    assert set(ISOLATED) == set(PC.TERMS)
    for term, (name, false) in ISOLATED.items():
        assert term in false and frozenset(false) in PC.false_term_sets(PC.build(name)), (term, name)
    # the two terms that cannot be separated at an even width
    for n in PC.NAMES:
        b = PC.build(n)
        for l in range(b.case.levels - 1):
            if b.ws[l] % 2 == 0:
                assert all(t[5] == t[6] for t in PC.fast_terms(b, 0, l))


def test_the_one_launch_kernel_is_taken_and_refused_for_every_reason():
    why = {n: PC.fused_refusal(PC.build(n)) for n in PC.NAMES}
    assert {n for n, r in why.items() if r is None} >= {"64x37_L3_packed", "64x37_L3_padded4", "64x37_L3_padded12", "64x37_L3_off4",
                                                        "128x64_L5_packed", "128x64_L5_padded4", "128x64_L5_off4", "64x37_L3_mid_last",
                                                        PC.FUSED_256x4}
    assert why["16x9_L2_packed"] == "levels"
    assert why["64x37_L3_pitch2"] == "base or pitch"
    assert why["64x37_L3_off1"] == "stride or offset" and why["64x37_L3_odd_stride"] == "stride or offset"
    assert why["40x20_L3_packed"] == "width" and why["636x38_L3_rounded4"] == "width"
    assert why["64x6_L3_packed"] == "height"
    assert why["64x37_L3_reversed"] == "level 0 ends at the pitch" and why["128x64_L5_reversed"] == "level 0 ends at the pitch"


def test_a_source_level_ends_at_the_pitch():
    for n in ("16x9_L2_reversed", "24x12_L2_reversed", "20x12_L2_reversed", "64x37_L3_reversed", "128x64_L5_reversed"):
        b = PC.build(n)
        assert b.offs[0] + b.strides[0] * b.hs[0] == b.pitch and b.strides[0] == b.ws[0] and PC.tight(b, 0)
        assert all(b.offs[l] > b.offs[l + 1] for l in range(b.case.levels - 1))
        assert not any(PC.tight(b, l) for l in range(1, b.case.levels - 1))
    # the strips at the end of the last rows would load 4 bytes behind the pitch: 16-byte strips whose width is 0 modulo 8
    for n in ("16x9_L2_reversed", "24x12_L2_reversed", "64x37_L3_reversed"):
        t = PC.fast_terms(PC.build(n), 0, 0)
        assert all(t[-1]) and PC.build(n).ws[0] % 8 == 0
    b = PC.build("64x37_L3_mid_last")
    assert PC.tight(b, 1) and not PC.tight(b, 0) and b.offs[1] + b.strides[1] * b.hs[1] == b.pitch and b.offs[0] < b.offs[2] < b.offs[1]
    # no other case has a tight source level: the 4 bytes behind a level's last row are inside the pitch everywhere else
    others = [n for n in PC.NAMES if PC.CASES[n].layout not in ("reversed", "mid_last")]
    assert not any(PC.tight(PC.build(n), l) for n in others for l in range(PC.CASES[n].levels - 1))


def test_the_release_library_runs_the_256_thread_kernel_of_five_levels():
    b = PC.build(PC.FUSED_256x4)
    assert (b.case.w, b.case.h, b.case.levels, b.case.n) == (128, 288, 5, 32)
    assert all(w % 8 == 0 and w >= 16 for w in b.ws[:4]) and b.hs == [288, 144, 72, 36, 18]
    # ceil(2048 / 32) = 64 bands wanted -> 1 row each, but 32 x 18 rows > 256 -> bands of 2 rows: 9 bands, 288 workgroups > 256
    assert b.case.n * b.hs[4] == 576 and PC.fused_plan(b)[:2] == (2, 9) and 9 * b.case.n == 288
    assert PC.fused_plan(b)[2] <= 64 * 1024
    assert PC.release_kernel(b) == (4, 256)
    # every other pyramid of 5 levels stays on the 1024-thread variant, as the earlier tests' do; K = 2 runs as well
    for n in ("128x64_L5_packed", "128x64_L5_padded4", "128x64_L5_off4"):
        assert PC.release_kernel(PC.build(n)) == (4, 1024)
    assert PC.release_kernel(PC.build("64x37_L3_packed")) == (2, 256)
    assert PC.release_kernel(PC.build("64x37_L3_reversed")) == "per level"
