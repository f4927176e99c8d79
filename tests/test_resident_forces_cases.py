"""The inputs of the cup3d_compute_forces_resident tests are not vacuous, and tests/resident_forces_cases.py restates the surface plan
consistently (no GPU).  Every mesh has all four properties, so none of the assertions is conditional."""
import numpy as np
import pytest

import resident_forces_cases as FC

K = FC.K


def lists_of(name, keys):
    first, obs = FC.firsts(name), K.obstacles(name)
    return [first[k] for k in keys], [obs[k]["ids"] for k in keys]


@pytest.mark.parametrize("name", FC.NAMES)
def test_the_spheres_take_every_path_of_the_plan(name):
    firsts, slots = lists_of(name, "ABC")
    per_block = [np.diff(f) for f in firsts]
    assert max(int(n.max()) for n in per_block) > 64                  # a block whose points span more than one chunk of 64
    assert all(int(n.max()) <= 512 for n in per_block)
    assert any(int((n == 0).sum()) > 0 for n in per_block)            # a listed block without points: it gets no row
    assert list(slots[1]) == sorted(slots[1], reverse=True)           # B's list descends: its rows are not in slot order
    p = FC.surface_plan(firsts, slots)
    rows, tiles = len(p["row_obst"]), len(p["tile_slots"])
    assert tiles < rows < sum(len(s) for s in slots)                   # a slot with points of two obstacles; fewer rows than listed blocks
    assert int(np.diff(p["sched_first"]).max()) == 3 and int(np.diff(p["sched_first"]).min()) == 1
    # AB, the other set of the GPU tests, shares slots too
    q = FC.surface_plan(*lists_of(name, "AB"))
    assert len(q["tile_slots"]) < len(q["row_obst"])


@pytest.mark.parametrize("name", FC.NAMES)
@pytest.mark.parametrize("keys", list(FC.SETS))
def test_the_tables_of_the_surface_plan(name, keys):
    firsts, slots = lists_of(name, keys)
    p = FC.surface_plan(firsts, slots)
    rows, points = len(p["row_obst"]), int(p["row_first"][-1])
    assert points == sum(int(f[-1]) for f in firsts) and p["row_base"][-1] == rows
    for r in range(rows):
        k, i = int(p["row_obst"][r]), int(p["row_block"][r])
        assert p["row_base"][k] <= r < p["row_base"][k + 1]
        assert int(slots[k][i]) == p["row_slot"][r] == p["tile_slots"][p["row_tile"][r]]
        assert p["row_first"][r + 1] - p["row_first"][r] == firsts[k][i + 1] - firsts[k][i] > 0
        # a row's points lie where the staged list of its obstacle has them: after the obstacle's earlier rows
        assert p["row_first"][r] - p["row_first"][p["row_base"][k]] == firsts[k][i]
    assert (np.diff(p["tile_slots"]) > 0).all()
    assert sorted(p["sched_rows"].tolist()) == list(range(rows))
    for j in range(len(p["tile_slots"])):   # the rows of the j-th slot: ascending obstacle, all of that slot
        e = p["sched_rows"][p["sched_first"][j]:p["sched_first"][j + 1]]
        assert len(e) >= 1 and (p["row_tile"][e] == j).all() and (np.diff(p["row_obst"][e]) > 0).all()
    # a chunk of tiles is a contiguous range of scheduled rows
    assert (np.diff(p["row_tile"][p["sched_rows"]]) >= 0).all()
    assert FC.surface_plan_bytes(firsts, slots) == len(slots) * 8 + rows * 172 + 4 + points * 36


def test_an_empty_rank_and_an_obstacle_without_blocks():
    assert FC.surface_plan_bytes([[0], [0]], [[], []]) == 0
    firsts, slots = lists_of("uniform8", "AB")
    p = FC.surface_plan([firsts[0], [0]], [slots[0], []])
    assert p["row_base"].tolist() == [0, len(p["row_obst"]), len(p["row_obst"])]
    assert FC.surface_plan_bytes([[0, 0, 0]], [[3, 1]]) == 0   # listed blocks, none with points


def test_totals_add_the_rows_in_ascending_slot_order():
    rng = np.random.default_rng(11)
    rows = rng.uniform(-1, 1, (6, 19)) * 10.0 ** rng.integers(-8, 8, (6, 19))
    slots = np.array([5, 2, 9, 0, 7, 3])
    want = np.zeros(19)
    for i in (3, 1, 5, 0, 4, 2):
        want = want + rows[i]
    assert np.array_equal(FC.totals(rows, slots), want)
    assert not np.array_equal(FC.totals(rows, slots), FC.totals(rows, slots[::-1].copy()))   # the order shows in the bits
    assert np.array_equal(FC.totals(np.zeros((0, 19)), []), np.zeros(19))
    # rows of zeros, which the resident call never sees, change no bit: the sum starts at +0 and a sum of doubles is -0 only from two -0
    with_zeros = np.concatenate([rows[:3], np.zeros((2, 19)), rows[3:]])
    assert np.array_equal(FC.totals(with_zeros, [5, 2, 9, 1, 4, 0, 7, 3]), want)
    assert not np.signbit(FC.totals(-0.0 * np.ones((2, 19)), [0, 1])).any()
    t = np.arange(19.0)
    pt, pd, e, eb = FC.derived(t, (3.0, 0.0, 4.0))
    assert (pt, pd) == (65.0, 60.0) and e == 65.0 / (65.0 + np.finfo(float).eps) and eb == 65.0 / (65.0 - 17.0 + np.finfo(float).eps)
    t[16] = -2.0
    assert FC.derived(t, (3.0, 0.0, 4.0))[2] == 65.0 / (65.0 + 2.0 + np.finfo(float).eps)
