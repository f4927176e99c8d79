"""Where the order of the obstacles shows in Penalization and kernelUpdateTmpV on the scenario A, B, C of
tests/resident_obstacles_cases.py (no GPU).  The resident kernels walk a slot's obstacles inside one workgroup; these counts are why a
kernel that walks them in another order than the staged calls -- obstacles one after the other -- cannot pass
tests/test_gpu_resident_obstacles.py."""
import numpy as np
import pytest

import resident_obstacles_cases as RC

K = RC.K
TWICE = {"uniform8": 29, "f16_mixed": 29, "amr_periodic_l01": 99}        # cells penalised by two obstacles
ORDER = {"uniform8": 210, "f16_mixed": 210, "amr_periodic_l01": 211}    # cells whose tmpV differs between A,B,C and C,B,A


@pytest.mark.parametrize("name", RC.NAMES)
def test_cells_penalised_by_two_obstacles_of_one_slot(name):
    c = K.CC.case(name)
    obst = RC.obstacles(name, "ABC")
    field = RC.chi_field(c.nb, obst)
    hit = RC.per_slot(c.nb, obst, [RC.penalized(field, o) for o in obst])
    twice = hit.sum(axis=0) >= 2
    assert int(twice.sum()) == TWICE[name]
    assert int(twice.reshape(c.nb, -1).any(axis=1).sum()) == 7   # slots that hold such a cell
    # they are the ties inside A and B: both obstacles' chi equal the field's
    a, b = (np.zeros((c.nb, 8, 8, 8)) for _ in range(2))
    a[obst[0]["ids"]], b[obst[1]["ids"]] = obst[0]["chi"], obst[1]["chi"]
    assert (hit[0] & hit[1])[twice].all() and np.array_equal(a[twice], b[twice]) and np.array_equal(a[twice], field[twice])


def test_the_velocity_depends_on_the_order_of_two_obstacles():
    differs = 0
    for name in RC.NAMES:
        c = K.CC.case(name)
        obst = RC.obstacles(name, "ABC")
        field = RC.chi_field(c.nb, obst)
        ab = RC.penalize(RC.penalize(RC.vel_of(name).copy(), field, c.geom, obst[0]), field, c.geom, obst[1])
        ba = RC.penalize(RC.penalize(RC.vel_of(name).copy(), field, c.geom, obst[1]), field, c.geom, obst[0])
        twice = (RC.per_slot(c.nb, obst, [RC.penalized(field, o) for o in obst]).sum(axis=0) >= 2)
        assert np.array_equal(ab[~twice], ba[~twice])   # elsewhere a cell has one writer
        differs += int((ab != ba).any(axis=-1).sum())
    assert differs > 0


@pytest.mark.parametrize("name", RC.NAMES)
def test_tmpv_depends_on_the_order_of_the_obstacles(name):
    c = K.CC.case(name)
    obst = RC.obstacles(name, "ABC")
    field = RC.chi_field(c.nb, obst)
    adds = RC.per_slot(c.nb, obst, [RC.adds_udef(field, o) for o in obst])
    assert int((adds.sum(axis=0) == 3).sum()) == {"uniform8": 2397, "f16_mixed": 2397, "amr_periodic_l01": 2395}[name]
    abc, cba = np.zeros((c.nb, 8, 8, 8, 3)), np.zeros((c.nb, 8, 8, 8, 3))
    for o in obst:
        RC.update_tmpv(abc, field, o)
    for o in obst[::-1]:
        RC.update_tmpv(cba, field, o)
    assert int((abc != cba).any(axis=-1).sum()) == ORDER[name]


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_slot_major_lists_of_the_plan(name):
    obst = RC.obstacles(name, "ABC")
    lists = [o["ids"] for o in obst]
    row_base, row_obst, row_block, first, rows = RC.plan(lists)
    nb = K.CC.case(name).nb
    assert row_base.tolist() == [0, nb, 2 * nb, 3 * nb] and len(rows) == 3 * nb and len(first) == nb + 1
    sizes = np.diff(first)
    assert sizes.min() >= 1 and sizes.max() == 3
    for j in range(nb):   # the j-th distinct slot is slot j here; its rows ascend in k and point at that slot
        e = rows[first[j]:first[j + 1]]
        assert row_obst[e].tolist() == sorted(row_obst[e].tolist()) == [0, 1, 2]
        assert [int(lists[row_obst[r]][row_block[r]]) for r in e] == [j] * 3
    assert list(lists[1]) == sorted(lists[1], reverse=True)   # B's list descends: its rows are not in slot order
    # an obstacle that holds only some slots leaves shorter lists
    _, ro, _, f2, r2 = RC.plan([lists[0], lists[1][:3], lists[2][:0]])
    assert np.diff(f2).tolist() == [1] * (nb - 3) + [2] * 3 and ro[r2[-2:]].tolist() == [0, 1]
    assert RC.plan_bytes([lists[0], lists[1][:3], lists[2][:0]]) == 3 * 104 + (nb + 3) * 244 + (nb + 1) * 4 and RC.plan_bytes([[], []]) == 0
