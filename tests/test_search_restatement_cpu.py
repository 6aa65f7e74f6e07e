"""The "round" search world (tests/quirk_fixtures.py) guarded against rot, on the CPU.

The reference rounds a pixel as a cv::Point2f: the double is narrowed to float and only then rounded half to even
(ReprojectPoint's IsInImage, src/Feature_alignment.cpp:58; the mask test, :96). The plants of the world sit within 1e-9..1e-6
of k + 0.5, where that and rounding the double part ways. If the world drifts (another texture, another pose draw, a plant
moved), the parity tests on it would still pass while no longer looking at the rounding: these tests fail first."""
import numpy as np
import pytest

from dsdtm_amd import search, synth
from tests import quirk_fixtures as Q
from tests import search_restatement as SR

N_BASE = Q.SEARCH_WORLDS["round"]["n_points"]          # the plants follow the std world's map points


@pytest.fixture(scope="module")
def runs():
    trace = []
    faithful = Q.search_restated("round", trace=trace)
    return dict(faithful=faithful, trace=trace, S1_ROUND_BORDER=Q.search_restated("round", "S1_ROUND_BORDER"),
                S1_ROUND_MASK=Q.search_restated("round", "S1_ROUND_MASK"))


def test_point2f_rounding_is_half_to_even_after_narrowing():
    assert SR.cv_round(100.5 + 1e-9) == 100 and SR.cv_round_double(100.5 + 1e-9) == 101
    assert SR.cv_round(101.5 - 1e-9) == 102 and SR.cv_round_double(101.5 - 1e-9) == 101
    assert SR.cv_round(100.5 + 1e-4) == 101 and SR.cv_round(7.25) == 7        # away from a half: the same as the double
    for x in (7.5 - 1e-9, 631.5 - 1e-7, 60.500001, 107.4999999, 3.5, 2.5):
        assert SR.cv_round(x) == search.cvRound_point2f(x)                   # the product's Python twin


def test_every_plant_sits_where_the_two_roundings_decide_differently(runs):
    cam = synth.Camera.tum(640, 480)
    at_mask_test = {t[1]: t for t in runs["trace"]}
    for i, (kind, x, y, decision) in enumerate(Q.ROUND_PLANTS):
        if kind == "border":
            f, d = SR.in_image(cam, x, y, 8), SR.in_image(cam, x, y, 8, rnd=SR.cv_round_double)
            assert f != d and f == (decision == "in"), (i, kind, x, y)
        else:
            # against the mask as it is when the restatement tests this candidate (a disc plant: after earlier cells painted)
            t = at_mask_test.get(N_BASE + i)
            assert t is not None, (i, kind, "never reaches the mask test")
            assert t[3] != t[4] and t[3] == (decision == "blocked"), (i, kind, x, y, t[3:])
    assert {p[0] for p in Q.ROUND_PLANTS} == {"border", "mask", "disc"}
    ins = sum(p[3] == "in" for p in Q.ROUND_PLANTS if p[0] == "border")
    outs = sum(p[3] == "out" for p in Q.ROUND_PLANTS if p[0] == "border")
    assert ins != outs and min(ins, outs) >= 1                              # the two directions do not cancel in the grid count


def test_the_faithful_restatement_and_each_rounding_mutant_differ(runs):
    f = runs["faithful"]
    assert len(f[0]) >= 150 and len(f[0]) < 200 and f[2] > 500
    for mutant in ("S1_ROUND_BORDER", "S1_ROUND_MASK"):
        assert Q.search_first_difference(f, runs[mutant]) is not None, mutant
    assert runs["S1_ROUND_BORDER"][2] != f[2]                               # a border flip moves the grid count


def test_each_kind_of_plant_changes_the_match_list(runs):
    """Not only the mask: for each kind, some plant is matched under one rounding and not under the other."""
    faithful = {m[1] for m in runs["faithful"][0]}
    for kind, mutant in (("border", "S1_ROUND_BORDER"), ("mask", "S1_ROUND_MASK"), ("disc", "S1_ROUND_MASK")):
        other = {m[1] for m in runs[mutant][0]}
        flipped = [i for i, p in enumerate(Q.ROUND_PLANTS) if p[0] == kind and ((N_BASE + i) in faithful) != ((N_BASE + i) in other)]
        assert flipped, kind
    for direction in ("in", "out"):                                         # a matchable plant on each side of the border
        assert any(p[0] == "border" and p[3] == direction and (((N_BASE + i) in faithful) != ((N_BASE + i) in {m[1] for m in runs["S1_ROUND_BORDER"][0]}))
                   for i, p in enumerate(Q.ROUND_PLANTS)), direction


def test_disc_plants_are_decided_by_a_disc_of_an_earlier_cell(runs):
    """A disc plant's cell comes after the cell whose match painted the disc edge it sits on: the device replay decides it through
    the discs (cp[] in track.hip), not through the caller's mask."""
    mask0 = Q.search_mask("round")
    cells = {t[1]: t[0] for t in runs["trace"]}
    for i, (kind, x, y, decision) in enumerate(Q.ROUND_PLANTS):
        if kind != "disc":
            continue
        for rnd in (SR.cv_round, SR.cv_round_double):
            assert mask0[rnd(y), rnd(x)] == 255                             # free at the start of the search
        assert any(m[0] < cells[N_BASE + i] for m in runs["faithful"][0])
