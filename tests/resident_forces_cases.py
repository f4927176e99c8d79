"""Inputs of the cup3d_compute_forces_resident tests and a NumPy statement of its surface plan and of Obstacle::computeForces.
TEST INFRASTRUCTURE.

The meshes and the spheres A, B, C of tests/collision_cases.py (every sphere lists every block, B's list descends) with a seeded vel and
pres.  The GPU tests compare the resident entry point with the staged cup3d_compute_forces bit for bit, so nothing here has to
reproduce the device's per-point arithmetic: `surface_plan` restates the tables of SurfacePlan (csrc/obstacles.hpp), `surface_plan_bytes`
what they add to cup3d_sim_device_bytes (include/cup3d_hip.h), `totals` the loop of Obstacle::computeForces over obstacleBlocks
(main.cpp:13082-13086) and `derived` its last four lines (13108-13114)."""
import numpy as np

import resident_obstacles_cases as RC

K = RC.K
NAMES = RC.NAMES
SETS = RC.SETS
NU = 0.004
_pres, _first = {}, {}


def vel_of(name):
    """the velocity field every test starts from"""
    return RC.vel_of(name)


def pres_of(name):
    if name not in _pres:
        _pres[name] = np.random.default_rng(7).uniform(-1, 1, (K.CC.case(name).nb, 8, 8, 8))
    return _pres[name]


def firsts(name):
    """{"A" | "B" | "C": first [n+1]}: the CSR of every sphere's surface points over its listed blocks, as the restatement of
    CreateObstacles counts them"""
    if name not in _first:
        c = K.CC.case(name)
        _, created, _, _ = K.CC.expected(name)
        third = K.obstacles(name)["C"]
        _, (rc,) = K.CR.create(c.geom, c.nb, [{k: third[k] for k in ("ids", "sdf", "udef", "transvel_correction")}])
        _first[name] = {"A": np.asarray(created[0].first), "B": np.asarray(created[1].first), "C": np.asarray(rc.first)}
    return _first[name]


def surface_plan(first_lists, slot_lists):
    """dict of the plan's tables.  A surface row is a listed block with points, in obstacle order and then listed order: row_base [N+1],
    row_obst / row_block / row_slot [Rs], row_first [Rs+1] (where each row's points begin among all P).  tile_slots [S]: the distinct
    slots of the rows, ascending; row_tile [Rs]: the place of a row's slot among them; the slot-major schedule: the rows of the j-th
    slot, sched_rows[sched_first[j]:sched_first[j+1]], ascend in the obstacle."""
    row_obst, row_block, row_slot, row_first, row_base = [], [], [], [0], [0]
    for k, (first, slots) in enumerate(zip(first_lists, slot_lists)):
        first = np.asarray(first, dtype=np.int64) if len(slots) else np.zeros(1, dtype=np.int64)
        assert len(first) == len(slots) + 1
        for i, n in enumerate(np.diff(first)):
            if n > 0:
                row_obst.append(k)
                row_block.append(i)
                row_slot.append(int(slots[i]))
                row_first.append(row_first[-1] + int(n))
        row_base.append(len(row_obst))
    row_slot = np.array(row_slot, dtype=np.int64)
    sched_rows = np.argsort(row_slot, kind="stable").astype(np.int32)
    tile_slots = np.unique(row_slot)
    row_tile = np.searchsorted(tile_slots, row_slot).astype(np.int32)
    sched_first = np.searchsorted(row_slot[sched_rows], np.concatenate([tile_slots, [np.iinfo(np.int64).max]])).astype(np.int32)
    return dict(row_base=np.array(row_base), row_obst=np.array(row_obst, dtype=np.int32), row_block=np.array(row_block, dtype=np.int32),
                row_slot=row_slot.astype(np.int32), row_first=np.array(row_first, dtype=np.int32), tile_slots=tile_slots.astype(np.int32),
                row_tile=row_tile, sched_first=sched_first, sched_rows=sched_rows)


def surface_plan_bytes(first_lists, slot_lists):
    """what the surface plan adds to cup3d_sim_device_bytes: N * 8 + Rs * (5 * 4 + 19 * 8) + 4 + P * (3 * 4 + 3 * 8); nothing without rows"""
    p = surface_plan(first_lists, slot_lists)
    rows, points = len(p["row_obst"]), int(p["row_first"][-1])
    if rows == 0:
        return 0
    return len(slot_lists) * 8 + rows * (5 * 4 + 19 * 8) + 4 + points * (3 * 4 + 3 * 8)


def totals(qoi_rows, slots):
    """the nineteen sums of Obstacle::computeForces before the all-reduce: one row after the other in ascending slot (blockID) order onto
    zeros, in double precision"""
    qoi_rows = np.asarray(qoi_rows, dtype=np.float64).reshape(-1, 19)
    total = np.zeros(19)
    for i in np.argsort(np.asarray(slots), kind="stable"):
        total = total + qoi_rows[i]
    return total


def derived(total, vel):
    """(Pthrust, Pdrag, EffPDef, EffPDefBnd) as 13108-13114 write them; total in sumQoI order"""
    eps = np.finfo(np.float64).eps
    drag, thrust, def_power, def_power_bnd = (np.float64(total[q]) for q in (12, 13, 16, 17))
    v = np.asarray(vel, dtype=np.float64)
    vel_norm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    p_thrust, p_drag = thrust * vel_norm, drag * vel_norm
    with np.errstate(divide="ignore", invalid="ignore"):
        return p_thrust, p_drag, p_thrust / (p_thrust - min(def_power, np.float64(0)) + eps), p_thrust / (p_thrust - def_power_bnd + eps)
