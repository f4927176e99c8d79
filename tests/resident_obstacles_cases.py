"""Inputs of the resident obstacle operator tests (cup3d_update_obstacles_resident, cup3d_penalization_resident,
cup3d_update_tmpv_resident) and a short NumPy statement of what order means to them.  TEST INFRASTRUCTURE.

The meshes and the spheres A, B, C of tests/collision_cases.py; every sphere lists every block, B's list descends.  The GPU tests compare
the resident entry points with the staged ones bit for bit, so nothing here has to reproduce the device's bits: `penalize` and
`update_tmpv` state the per-cell rules of k_penalize / k_update_tmpv (csrc/obstacles_penalization.hip; KernelPenalization, main.cpp:13841-13912, and
kernelUpdateTmpV, 14948-14979) so that tests/test_resident_obstacles_cases.py can count where the order of the obstacles shows: a
slot-major kernel that visits a slot's obstacles in another order than the staged calls' cannot give the same bits there.
`plan` restates the plan of the retained set (ResidentPlan, csrc/obstacles.hpp)."""
import numpy as np

import collision_cases as K

NAMES = K.NAMES
DT, LAMBDA = K.DT, 1e4
SETS = {"AB": "approach", "ABC": "three"}   # obstacle set -> the scenario of collision_cases that holds its rigid state
_vel = {}


def vel_of(name):
    """the velocity field every test starts from"""
    if name not in _vel:
        _vel[name] = np.random.default_rng(3).uniform(-1, 1, (K.CC.case(name).nb, 8, 8, 8, 3))
    return _vel[name]


def obstacles(name, keys):
    """[dict(ids, chi, udef (corrected), cm, vel, omega)] of the set, with the rigid state of collision_cases.APPROACH"""
    obs = K.obstacles(name)
    return [dict(ids=obs[k]["ids"], chi=obs[k]["chi"], udef=obs[k]["udef_corrected"], cm=obs[k]["cm"], vel=np.array(K.APPROACH[k]["vel"]),
                 omega=np.array(K.APPROACH[k]["omega"])) for k in keys]


def chi_field(nb, obst):
    """the resident chi CreateObstacles leaves: the max over the obstacles (13301)"""
    field = np.zeros((nb, 8, 8, 8))
    for o in obst:
        for i, g in enumerate(o["ids"]):
            field[g] = np.maximum(field[g], o["chi"][i])
    return field


def penalized(field, o):
    """[nblocks][8][8][8] bool, in the obstacle's block order: the cells KernelPenalization changes (13871-13874)"""
    return np.array([~(field[g] > o["chi"][i]) & ~(o["chi"][i] <= 0) for i, g in enumerate(o["ids"])])


def adds_udef(field, o):
    """the cells kernelUpdateTmpV adds udef to (14969)"""
    return np.array([~(field[g] > o["chi"][i]) for i, g in enumerate(o["ids"])])


def penalize(vel, field, geom, o, dt=DT, lam=LAMBDA, implicit=False):
    """KernelPenalization of one obstacle on vel [nb][8][8][8][3], in place"""
    lam_fac = lam if implicit else 1.0 / dt
    c = np.arange(8) + 0.5
    mask = penalized(field, o)
    for i, g in enumerate(o["ids"]):
        h, org = geom[g, 0], geom[g, 1:4]
        z, y, x = np.meshgrid(org[2] + h * c, org[1] + h * c, org[0] + h * c, indexing="ij")
        p = np.stack([x, y, z], axis=-1) - o["cm"]
        ut = o["vel"] + np.cross(np.broadcast_to(o["omega"], p.shape), p) + o["udef"][i]
        chi = o["chi"][i]
        X = np.where(chi > 0.5, 1.0, 0.0) if implicit else chi
        fac = X * lam_fac / (1 + X * lam_fac * dt) if implicit else X * lam_fac
        new = vel[g] + dt * (fac[..., None] * (ut - vel[g]))
        vel[g] = np.where(mask[i][..., None], new, vel[g])
    return vel


def update_tmpv(tmpv, field, o):
    """kernelUpdateTmpV of one obstacle on tmpV [nb][8][8][8][3], in place"""
    mask = adds_udef(field, o)
    for i, g in enumerate(o["ids"]):
        tmpv[g] = np.where(mask[i][..., None], tmpv[g] + o["udef"][i], tmpv[g])
    return tmpv


def per_slot(nb, obst, masks):
    """[nobst][nb][8][8][8]: the obstacles' masks by slot instead of by listed block"""
    out = np.zeros((len(obst), nb, 8, 8, 8), dtype=bool)
    for k, (o, m) in enumerate(zip(obst, masks)):
        out[k, o["ids"]] = m
    return out


def plan(slot_lists):
    """(row_base [N+1], row_obst [R], row_block [R], sched_first [S+1], sched_rows [R]): row row_base[k] + i is block i of obstacle k; the
    distinct slots ascend, and the rows of the j-th of them, sched_rows[sched_first[j]:sched_first[j+1]], ascend in k"""
    row_base = np.concatenate([[0], np.cumsum([len(s) for s in slot_lists])]).astype(np.int64)
    row_obst = np.concatenate([np.full(len(s), k) for k, s in enumerate(slot_lists)] or [np.zeros(0)]).astype(np.int32)
    row_block = np.concatenate([np.arange(len(s)) for s in slot_lists] or [np.zeros(0)]).astype(np.int32)
    row_slot = np.concatenate([np.asarray(s) for s in slot_lists] or [np.zeros(0)]).astype(np.int64)
    sched_rows = np.argsort(row_slot, kind="stable").astype(np.int32)
    sorted_slots = row_slot[sched_rows]
    starts = np.where(np.concatenate([[True], sorted_slots[1:] != sorted_slots[:-1]]))[0] if len(sorted_slots) else np.zeros(0, dtype=np.int64)
    return row_base, row_obst, row_block, np.concatenate([starts, [len(row_slot)]]).astype(np.int32), sched_rows


def plan_bytes(slot_lists):
    """what the plan adds to cup3d_sim_device_bytes (include/cup3d_hip.h): N (32 + 72) + R (3 * 4 + 29 * 8) + (S + 1) * 4; nothing without rows"""
    n, rows = len(slot_lists), sum(len(s) for s in slot_lists)
    if rows == 0:
        return 0
    distinct = len(set(int(v) for s in slot_lists for v in s))
    return n * (32 + 72) + rows * (3 * 4 + 29 * 8) + (distinct + 1) * 4
