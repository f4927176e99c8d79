"""The inputs of the device tests of cup3d_compute_forces (tests/surface_forces_cases.py) take every path of KernelComputeForces::visit
(main.cpp:12273-12493): shown on the CPU by the instrumented restatement.  No GPU.  No path may be left out."""
import numpy as np
import pytest

import surface_forces_cases as SC
import surface_forces_restatement as R


@pytest.mark.parametrize("name", SC.SINGLE_RANK + ("uniform64",))
def test_every_path_is_taken(name):
    e = SC.expected(name)
    assert SC.ALL_PATHS - e.trace == set(), sorted(SC.ALL_PATHS - e.trace)
    assert e.trace - SC.ALL_PATHS <= {"forcePar=0"}, sorted(e.trace - SC.ALL_PATHS)   # obstacle B: velUnit = 0


@pytest.mark.parametrize("name", SC.SINGLE_RANK + ("uniform64",))
def test_shape_of_the_inputs(name):
    e = SC.expected(name)
    a, b = e.obstacles
    assert tuple(np.diff(a["first"])) == (1, 63, 64, 65, 200) and tuple(np.diff(b["first"])) == SC.COUNTS_B
    assert a["empty_slot"] not in a["slots"] or e.nb < 6   # the block without points is not listed (12280)
    assert set(b["slots"]) & set(a["slots"])               # the two obstacles share a block
    assert not b["vel"].any() and a["vel"].any()
    for o in (a, b):
        assert (np.sqrt((o["dchi"] ** 2).sum(axis=1)) >= 0.1).all()
        assert o["ijk"].min() >= 0 and o["ijk"].max() <= 7
    i65 = a["first"][3]
    assert np.array_equal(a["ijk"][i65], a["ijk"][i65 + 1]) and not np.array_equal(a["dchi"][i65], a["dchi"][i65 + 1])   # one cell, listed twice
    lo, hi = a["first"][4], a["first"][5]
    for ax in range(3):   # the six axis directions at ix / iy / iz in {0, 7}
        for sgn, cell in ((1, 7), (-1, 0)):
            on_axis = [(a["dchi"][i, ax] * sgn > 0) and not a["dchi"][i, [d for d in range(3) if d != ax]].any() and a["ijk"][i, ax] == cell
                       for i in range(lo, hi)]
            assert sum(on_axis) >= 1
    assert 0 <= e.chi.min() and e.chi.max() <= 0.05
    if name in SC.GOLDEN:
        assert len(set(e.hs.tolist())) >= 2   # h differs per block on these meshes


def test_the_two_point_branches_are_where_the_issue_says():
    """x = 10 with sx = +1, or x = -3 with sx = -1: the march has to carry the point three cells out of the block"""
    e = SC.expected("box222_wall")
    a = e.obstacles[0]
    i = 4
    lo, hi = a["first"][i], a["first"][i + 1]
    seen = set()
    for p in range(lo, hi):
        tr = set()
        R.visit(e.vel_tiles[a["slots"][i]], e.chi_tiles[a["slots"][i]], e.pres[a["slots"][i]], e.hs[a["slots"][i]], e.origins[a["slots"][i]], a["udef"][i],
                a["ijk"][p:p + 1], a["dchi"][p:p + 1], a["cm"], a["vel"], a["omega"], SC.NU, a["qoi"][i], tr)
        for ax in "xyz":
            if f"dveld{ax}_2" in tr:
                d = "xyz".index(ax)
                assert a["ijk"][p, d] in (0, 7) and a["dchi"][p, d] != 0
                seen.add((ax, int(np.sign(a["dchi"][p, d]))))
    assert seen == {(ax, s) for ax in "xyz" for s in (1, -1)}, seen


def test_the_second_call_carries_eight_sums_and_restarts_eleven():
    e = SC.expected("box222_wall")
    for o, (p1, q1), (p2, q2) in zip(e.obstacles, e.first_call, e.second_call):
        assert np.array_equal(p1, p2)
        zeroed = [R.QOI_NAMES.index(n) for n in R.ZEROED]
        carried = [R.QOI_NAMES.index(n) for n in R.CARRIED]
        assert len(zeroed) == 11 and len(carried) == 8
        assert np.array_equal(q1[:, zeroed], q2[:, zeroed])
        assert not np.array_equal(q1[:, carried], q2[:, carried])
