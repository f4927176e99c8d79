"""Inputs of the cup3d_prevent_colliding_obstacles tests and what tests/collision_restatement.py makes of them.  TEST INFRASTRUCTURE.

Built on tests/characteristic_cases.py: its three meshes, its spheres A (R = 1.3 at (3.3, 3.0, 3.2), blocks ascending) and B (R = 3.2 at
(1.6, 1.5, 1.7), blocks DESCENDING), which overlap, and a third sphere C (R = 0.9 at (1.0, 4.6, 1.2), blocks ascending) that lies inside
B and away from A.  chi, the corrected udef, the centre of mass, mass and J of every obstacle are what
characteristic_restatement.create makes of them -- what cup3d_create_obstacles leaves on the device.

A scenario is a tuple of obstacle names plus the rigid state of each (BODIES); the five of SCENARIOS take the five paths of the pair loop
(tests/test_collision_cases.py asserts which).  The restatement is evaluated once per (mesh, scenario) and its results are never
modified."""
import numpy as np

import characteristic_cases as CC
import characteristic_restatement as CR
import collision_restatement as R

NAMES = CC.NAMES
DT = 0.01
_obstacles, _expected = {}, {}

# rigid velocities under which A and B approach each other along the contact normal (projVel > 0); "apart" reverses them
APPROACH = {"A": dict(vel=(-0.30, -0.25, -0.20), omega=(0.05, -0.02, 0.03)),
            "B": dict(vel=(0.20, 0.25, 0.15), omega=(-0.01, 0.04, -0.02)),
            "C": dict(vel=(0.10, -0.30, 0.20), omega=(0.02, 0.01, -0.03))}
# scenario -> (obstacles, reversed?, the forced one)
SCENARIOS = {"approach": ("AB", False, None), "apart": ("AB", True, None), "A_forced": ("AB", False, "A"), "three": ("ABC", False, None),
             "A_and_C": ("AC", False, None)}


def obstacles(name):
    """{"A" | "B" | "C": dict(ids, sdf, udef (as the geometry wrote it), transvel_correction, chi, udef_corrected, cm, mass, J)} of the mesh"""
    if name in _obstacles:
        return _obstacles[name]
    c = CC.case(name)
    _, first, _, _ = CC.expected(name)
    out = {}
    ids = np.arange(c.nb, dtype=np.int64)
    rng = np.random.default_rng(41)
    sdf = CC.sdf_tiles(c.geom, ids, CC.sphere((1.0, 4.6, 1.2), 0.9))
    third = dict(ids=ids, sdf=sdf, udef=0.05 * rng.uniform(-1, 1, (c.nb, 8, 8, 8, 3)) + np.array([0.1, -0.2, 0.05]), transvel_correction=np.zeros(3))
    _, (rc,) = CR.create(c.geom, c.nb, [third])   # an obstacle's own arrays do not depend on the others of the call
    for key, o, r in (("A", c.obstacles[0], first[0]), ("B", c.obstacles[1], first[1]), ("C", third, rc)):
        out[key] = dict(o, chi=r.chi, udef_corrected=r.udef, cm=r.cm, mass=r.mass, J=r.J)
    _obstacles[name] = out
    return out


def body(o, key, reverse=False, forced=False):
    s = -1.0 if reverse else 1.0
    return dict(cm=o["cm"], mass=o["mass"], J=o["J"], forced=(1, 0, 0) if forced else (0, 0, 0), vel=s * np.array(APPROACH[key]["vel"]),
                omega=s * np.array(APPROACH[key]["omega"]), collision_vel=np.zeros(3), collision_omega=np.zeros(3), collision_counter=0.0)


def scenario(name, which):
    """(keys, obstacles as the restatement takes them, bodies)"""
    keys, reverse, forced = SCENARIOS[which]
    obs = obstacles(name)
    return keys, [dict(ids=obs[k]["ids"], sdf=obs[k]["sdf"], chi=obs[k]["chi"], udef=obs[k]["udef_corrected"]) for k in keys], \
        [body(obs[k], k, reverse, k == forced) for k in keys]


def expected(name, which):
    """(Result of collision_restatement.prevent, trace) on one rank"""
    if (name, which) not in _expected:
        _, obst, bodies = scenario(name, which)
        trace = set()
        _expected[name, which] = (R.prevent(CC.case(name).geom, obst, bodies, DT, trace), trace)
    return _expected[name, which]


def shared_cells(a, b):
    """(cells with chi > 0 in both, blocks that hold one)"""
    where = {int(g): i for i, g in enumerate(b["ids"])}
    cells = blocks = 0
    for i, g in enumerate(a["ids"]):
        if int(g) in where:
            n = int(((a["chi"][i] > 0) & (b["chi"][where[int(g)]] > 0)).sum())
            cells += n
            blocks += n > 0
    return cells, blocks
