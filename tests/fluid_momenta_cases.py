"""Inputs of the cup3d_update_obstacles tests and what tests/fluid_momenta_restatement.py makes of them.  TEST INFRASTRUCTURE.

Three meshes: `uniform8` (bpd 1,1,1 at level 1, a synthetic obstacle from oracle_lib.synthetic_obstacle), and the two goldens of
tests/golden/obstacle_ops.npz, `f16_mixed` (8 blocks) and `amr_periodic_l01` (15 blocks on two levels).  Each has two obstacles: A, the
fixture's own, and B, a different one on the same blocks listed in descending order.  The restatement is evaluated once per
(case, implicit, geometry) and its results are never modified."""
import os

import numpy as np

import fluid_momenta_restatement as R
import oracle_lib as O

NAMES = ("uniform8", "f16_mixed", "amr_periodic_l01")
EXT = 2 * np.pi
LAMBDA, DT = 1e4, 0.01
BCN = {0: "freespace", 1: "periodic", 2: "wall"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cases, _expected = {}, {}


class Case:
    """sim_kwargs (SimulationData arguments), nb, vel [nb][8][8][8][3], chi_field [nb][8][8][8], obstacles = [A, B]: dicts with
    ids, chi, udef, cm, vel, omega"""


def case(name):
    if name in _cases:
        return _cases[name]
    c = Case()
    c.name = name
    if name == "uniform8":
        bc = ("periodic", "wall", "freespace")
        c.bpd, c.lmax, c.bc, c.leaves = (1, 1, 1), 2, bc, None
        c.sim_kwargs = dict(bpdx=1, bpdy=1, bpdz=1, levelMax=2, levelStart=1, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
        c.nb = 8
        ob, c.chi_field = O.synthetic_obstacle(None, c.nb, 9)
        c.vel = np.random.default_rng(8).uniform(-1, 1, (c.nb, 8, 8, 8, 3))
        ids, chi, udef, rigid = ob["ids"], ob["chi"], ob["udef"], ob["rigid"]
    else:
        z, g = np.load(os.path.join(GOLDEN, "obstacle_ops.npz")), np.load(os.path.join(GOLDEN, name + ".npz"))
        t = g["tables"]
        bpd, bc = tuple(int(b) for b in g["bpd"]), tuple(BCN[int(b)] for b in g["bc"])
        c.bpd, c.lmax, c.bc, c.leaves = bpd, int(g["level_max"]), bc, (t[:, 0].astype(np.int32), t[:, 1].copy())
        c.sim_kwargs = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=c.lmax, levelStart=0, extent=float(g["extent"]), BC_x=bc[0], BC_y=bc[1],
                            BC_z=bc[2], leaves=c.leaves)
        c.tables, c.nb = t, len(t)
        c.vel, c.chi_field = z[name + "_vel_in"], z[name + "_chi_field"]
        ids, chi, udef, rigid = z[name + "_ids"], z[name + "_ochi"], z[name + "_oudef"], z[name + "_rigid"]
    a = dict(ids=np.asarray(ids, dtype=np.int64), chi=chi, udef=udef, cm=rigid[0:3], vel=rigid[3:6], omega=rigid[6:9])
    rng = np.random.default_rng(21)
    n = len(a["ids"])
    b = dict(ids=a["ids"][::-1].copy(), chi=rng.uniform(-0.6, 1.4, (n, 8, 8, 8)).clip(0.0, 1.0), udef=0.1 * rng.uniform(-1, 1, (n, 8, 8, 8, 3)),
             cm=rigid[0:3] + np.array([0.1, -0.05, 0.08]), vel=np.array([0.1, 0.2, -0.3]), omega=np.array([0.05, -0.02, 0.03]))
    c.obstacles = [a, b]
    assert (a["chi"] <= 0).any() and (a["chi"] > 0.5).any() and (b["chi"] <= 0).any() and (b["chi"] > 0.5).any()
    _cases[name] = c
    return c


def expected(name, implicit, geom, k=0, forced=(0, 0, 0), block_rotation=(0, 0, 0), vel_imposed=(0.0, 0.0, 0.0)):
    """the restatement's Result for obstacle k of the case on the whole mesh (geom [nb][4] from the grid tables)"""
    key = (name, int(implicit), k, tuple(forced), tuple(block_rotation), tuple(vel_imposed), np.asarray(geom).tobytes())
    if key not in _expected:
        c = case(name)
        o = c.obstacles[k]
        _expected[key] = R.update(c.vel, geom, o["ids"], o["chi"], o["udef"], o["cm"], LAMBDA, DT, implicit, forced, block_rotation, vel_imposed)
    return _expected[key]


def velocity_bound(r):
    """64 eps cond(A) max|x|: what two correct LU solves of the same 6 x 6 system may differ by; cond(A) < 100 for these inputs"""
    cond = float(np.linalg.cond(r.A))
    assert cond < 100, cond
    return 64 * np.finfo(float).eps * cond * max(np.abs(r.vel_computed).max(), np.abs(r.omega_computed).max())
