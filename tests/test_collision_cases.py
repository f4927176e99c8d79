"""The inputs of tests/collision_cases.py take the paths the cup3d_prevent_colliding_obstacles tests need them to take (no GPU)."""
import numpy as np
import pytest

import collision_cases as K

AB_CELLS = {"uniform8": 219, "f16_mixed": 219, "amr_periodic_l01": 378}
# scenario -> what the restatement's trace must hold, what it must not
PATHS = {"approach": ({"resolved"}, {"projVel<=0", "forced_mass_1e10"}),
         "apart": ({"projVel<=0"}, {"resolved"}),
         "A_forced": ({"resolved", "forced_mass_1e10"}, {"projVel<=0"}),
         "three": ({"positions_differ_by_more_than_0.2", "totals_run_on_across_j", "imagmax_restarts_per_j", "iMom_persists_across_an_empty_j"},
                   {"resolved", "projVel<=0", "iM<tolerance", "other_iM<tolerance"}),
         "A_and_C": ({"iM<tolerance"}, {"resolved", "projVel<=0", "positions_differ_by_more_than_0.2"})}


@pytest.mark.parametrize("name", K.NAMES)
def test_the_spheres_overlap_where_the_cases_say(name):
    o = K.obstacles(name)
    assert K.shared_cells(o["A"], o["B"]) == (AB_CELLS[name], 8)
    assert K.shared_cells(o["B"], o["C"])[0] == 83 and K.shared_cells(o["A"], o["C"]) == (0, 0)
    assert list(o["B"]["ids"]) == sorted(o["B"]["ids"], reverse=True) and list(o["A"]["ids"]) == sorted(o["A"]["ids"])
    r, _ = K.expected(name, "approach")
    a, b = np.array(r.sums)
    # the two CollisionInfo see the same cells: the 0.2 test compares a number with itself
    assert a[0] == b[0] == a[10] == b[10] == AB_CELLS[name] and np.array_equal(a[1:4], b[1:4])
    assert np.array_equal(a[0:4], b[10:14]) and np.array_equal(a[7:10], b[17:20]) and np.array_equal(a[4:7], b[14:17])


@pytest.mark.parametrize("name", K.NAMES)
@pytest.mark.parametrize("which", list(K.SCENARIOS))
def test_every_scenario_takes_its_path(name, which):
    r, trace = K.expected(name, which)
    must, must_not = PATHS[which]
    assert must <= trace and not (must_not & trace), sorted(trace)
    keys = K.SCENARIOS[which][0]
    before = K.scenario(name, which)[2]
    changed = [not (np.array_equal(b["vel"], a["vel"]) and np.array_equal(b["omega"], a["omega"])) for b, a in zip(before, r.bodies)]
    if "resolved" in must:
        assert r.collided == [0, 1] and r.any and all(changed)
        for b in r.bodies:
            assert b["collision_counter"] == 0.01 * K.DT and b["collision_vel"] == b["vel"] and b["collision_omega"] == b["omega"]
    else:
        assert not any(changed) and all(b["collision_counter"] == 0.0 for b in r.bodies)
        # `apart` is pushed onto bCollisionID BEFORE the projVel test (14249-14250), the others never get there
        assert (r.collided, r.any) == (([0, 1], True) if which == "apart" else ([], False))
    assert len(r.sums) == len(keys)


@pytest.mark.parametrize("name", K.NAMES)
def test_three_bodies_fail_the_position_test_pair_by_pair(name):
    r, _ = K.expected(name, "three")
    s = np.array(r.sums)
    assert (s[:, 0] > 0).all()   # every obstacle has cells: none stops at the tolerance test
    assert s[0, 0] == K.shared_cells(*[K.obstacles(name)[k] for k in "AB"])[0] and s[2, 0] == 83 and s[1, 0] == s[0, 0] + 83
    mean = s[:, 1:4] / s[:, 0:1]
    for i, j in ((0, 1), (0, 2), (1, 2)):
        d = np.abs(mean[i] - mean[j]).max()
        assert 0.3 < d < 2.1, (i, j, d)
