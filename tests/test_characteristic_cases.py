"""The cases of the cup3d_create_obstacles tests are not vacuous (no GPU): the inputs of tests/characteristic_cases.py take every path of
KernelCharacteristicFunction::operate (main.cpp:13298-13403) and of the udef momenta, as traced by the restatement
(tests/characteristic_restatement.py).

Every case: far cells of both signs, band cells, cells with sdf == +h and == -h exactly (band branch), an SDF with gradUSq != 1, accepted
points at index 0 and 7 on each axis, `< 1e-12` and `Delta <= EPS` rejections, a block with more than 64 points (the ordered compaction
crosses wavefront chunks; obstacle B has blocks with 256), a listed block with chi == 1 and no point, two obstacles that overlap with the
second listed in descending slot order, cells with chi <= 0 in blocks that have chi > 0 (skipped by the momenta).
Exception: a listed block with chi == 0 and no point exists on amr_periodic_l01 only (7 of them); on the two 8-block meshes sphere A
reaches every block."""
import numpy as np
import pytest

import characteristic_cases as CC

PATHS = {"far_inside", "far_outside", "band", "sdf==+h", "sdf==-h", "gradUSq!=1", "gradH<1e-12", "Delta<=EPS"} | {f"point_{a}{i}" for a in "xyz" for i in (0, 7)}
EMPTY_OUTSIDE = {"uniform8": 0, "f16_mixed": 0, "amr_periodic_l01": 7}


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_cases_take_every_path(name):
    c = CC.case(name)
    field, first, second, trace = CC.expected(name)
    assert trace == PATHS, sorted(PATHS ^ trace)
    a, b = first
    assert list(c.obstacles[1]["ids"]) == sorted(c.obstacles[1]["ids"], reverse=True) and len(c.obstacles[1]["ids"]) > 1
    counts = [np.diff(r.first) for r in first]
    print(name, "points per block:", [k.tolist() for k in counts])
    assert counts[0].max() > 64 and counts[1].max() > 192      # two and four chunks of 64
    assert ((counts[0] > 0) & (counts[0] < 64)).any()
    outside = [i for i in range(len(counts[0])) if (a.chi[i] == 0).all()]
    assert len(outside) == EMPTY_OUTSIDE[name] and all(counts[0][i] == 0 for i in outside)
    inside = [i for i in range(len(counts[1])) if (b.chi[i] == 1).all()]
    assert inside and all(counts[1][i] == 0 for i in inside)
    # the max into the field matters in both directions
    fa, fb = field[c.obstacles[0]["ids"]], field[c.obstacles[1]["ids"]]
    assert (fa > a.chi).any() and (fb > b.chi).any() and (fa >= a.chi).all() and (fb >= b.chi).all()
    for r in first:
        for i in range(len(r.chi)):
            if (r.chi[i] > 0).any() and (r.chi[i] <= 0).any():
                break
        else:
            raise AssertionError("no block with cells on both sides of chi <= 0")
        assert np.abs(r.transvel_correction).min() > 1e-2 and np.abs(r.angvel_correction).min() > 1e-2
        assert (r.ijk >= 0).all() and (r.ijk < 8).all() and (r.delta > 0).all()
    # oldCorrVel reaches the angular sums only (13470-13479)
    for r, s in zip(first, second):
        assert np.array_equal(r.udef_totals[:4], s.udef_totals[:4]) and np.array_equal(r.udef_totals[7:], s.udef_totals[7:])
    assert not np.array_equal(first[1].udef_totals[4:7], second[1].udef_totals[4:7])
    assert not np.array_equal(first[0].udef_totals[4:7], second[0].udef_totals[4:7])
