"""The cases, inputs and expected results of the cup3d_compute_dissipation / cup3d_fix_mass_flux tests, shared by
tests/test_dissipation_restatement.py (CPU: the mutation catalogue runs over exactly what the GPU tests use) and the test_gpu_*flow* /
test_gpu_compute_dissipation / test_gpu_fix_mass_flux files.  TEST INFRASTRUCTURE; works without a GPU.

A case is a mesh (a uniform grid is read as the one-level mesh of its blocks, which the oracle can build tiles of), seeded random vel and
pres, and chi either random in [0, 1] or left untouched (zero).  The yardstick is tests/dissipation_restatement.py fed with the ORACLE's
[-1,2) tiles.  Expected rows are computed once per case and never modified."""
import numpy as np

import cup3d_amd as cu
import dissipation_restatement as R
import multigrid_cases as K
import oracle_lib as O

EXT = 2 * np.pi
NU = 0.013
U = 2.0 ** -53

# name -> (bpd, levelMax, level or None for a multi-level mesh, bc, chi random?)
CASES = {
    "one_block": ((1, 1, 1), 1, 0, ("wall", "freespace", "periodic"), True),          # the reference's one-thread sum, bit for bit
    "three_blocks": ((3, 1, 1), 1, 0, ("periodic", "wall", "freespace"), False),      # 3 blocks in 8 workgroups: padding workgroups exist
    "sixteen_mixed": ((2, 1, 1), 2, 1, ("freespace", "wall", "periodic"), True),      # 16 blocks, mixed boundary conditions
    "l012_wall": (None, None, None, None, False),                                     # three levels: per-block h, coarse-fine ghosts
    "l012_periodic": (None, None, None, None, True),
    "uniform_222": ((2, 2, 2), 2, 1, ("periodic", "wall", "freespace"), True),          # 64 blocks: the uniform grid the over-ranks test shares out
    "blocks_1280": ((5, 4, 1), 3, 2, ("wall", "periodic", "freespace"), False),       # 1280 blocks: 20 chunks of the totals kernel
}
SMALL = tuple(n for n in CASES if n != "blocks_1280")
_cache = {}


class Case:
    """name, bpd, lmax, bc, leaves (levels, Zs), uniform_level (None: multi-level), sim_kwargs, extents, nb, tables [nb][6], geom [nb][4],
    vel, pres, chi (None: untouched), vel_labs [nb][10][10][10][3], pres_labs [nb][10][10][10]"""


def extents_of(bpd, lmax):
    """SimulationData's extents (_preprocessArguments, main.cpp:15394-15415)"""
    nfe = [b * (1 << (lmax - 1)) * 8 for b in bpd]
    return [n / max(nfe) * EXT for n in nfe]


def case(name):
    if name in _cache:
        return _cache[name]
    c = Case()
    c.name = name
    bpd, lmax, level, bc, with_chi = CASES[name]
    if bpd is None:
        bpd, lmax, bc, lv, zs = K.mesh_case(name)
        c.uniform_level = None
    else:
        og = O.OracleGrid(bpd, lmax, level, EXT, bc)
        lv, zs = og.tables[:, 0].astype(np.int32), og.tables[:, 1].copy()
        c.uniform_level = level
    c.bpd, c.lmax, c.bc, c.leaves = tuple(bpd), lmax, tuple(bc), (np.asarray(lv, dtype=np.int32), np.asarray(zs, dtype=np.int64))
    c.sim_kwargs = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=NU)
    if c.uniform_level is None:
        c.sim_kwargs.update(levelStart=0, leaves=c.leaves)
    else:
        c.sim_kwargs.update(levelStart=level)
    c.extents = extents_of(bpd, lmax)
    c.mesh = O.OracleMesh(bpd, lmax, EXT, bc, *c.leaves)
    grid = cu.operators.Grid(bpd, lmax, 0 if c.uniform_level is None else level, EXT, bc, leaves=c.leaves if c.uniform_level is None else None)
    assert np.array_equal(grid.tables, c.mesh.tables), "the oracle's mesh and the library's grid order their blocks differently"
    c.nb, c.tables, c.geom = grid.nblocks, grid.tables.copy(), grid.geom.copy()
    rng = np.random.default_rng(100 + len(name))
    c.vel, c.pres = rng.uniform(-1, 1, (c.nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (c.nb, 8, 8, 8))
    c.chi = rng.uniform(0, 1, (c.nb, 8, 8, 8)) if with_chi else None
    c.vel_labs = c.mesh.labs(c.vel, -1, 2)
    c.pres_labs = c.mesh.labs(c.pres, -1, 2)[..., 0]
    for a in (c.vel, c.pres, c.vel_labs, c.pres_labs, c.geom) + (() if c.chi is None else (c.chi,)):
        a.setflags(write=False)
    _cache[name] = c
    return c


def chi_of(c):
    return np.zeros((c.nb, 8, 8, 8)) if c.chi is None else c.chi


def rows(c, fast=True, mutation=None, pres_labs=None, blocks=None):
    """the restatement's block rows [n][20] of the listed blocks (all), from the oracle's tiles"""
    fn = R.block_sums_fast if fast else R.block_sums
    P, X = c.pres_labs if pres_labs is None else pres_labs, chi_of(c)
    return np.array([fn(c.vel_labs[b], P[b], X[b], c.geom[b], c.extents, NU, mutation) for b in (range(c.nb) if blocks is None else blocks)])


def expected(name):
    """(rows [nb][20], totals [20], abs_rows [nb][20] = sum |summand| per block and quantity): once per case, read-only.  The rows come
    from block_sums_fast, which tests/test_dissipation_restatement.py holds to the scalar block_sums bit for bit."""
    key = ("expected", name)
    if key not in _cache:
        c = case(name)
        r = rows(c)
        t = np.array(R.totals(r))
        X = chi_of(c)
        a = np.array([R.abs_sums(c.vel_labs[b], c.pres_labs[b], X[b], c.geom[b], c.extents, NU) for b in range(c.nb)])
        for v in (r, t, a):
            v.setflags(write=False)
        _cache[key] = (r, t, a)
    return _cache[key]


def gamma(n):
    return n * U / (1 - n * U)


def wall_faces(c):
    """[(block, axis, side)] of the faces that lie on a wall"""
    out = []
    for b, t in enumerate(c.tables):
        for d in range(3):
            if c.bc[d] != "wall":
                continue
            n = c.bpd[d] << int(t[0])
            if t[2 + d] == 0:
                out.append((b, d, 0))
            if t[2 + d] == n - 1:
                out.append((b, d, 1))
    return out


def pres_labs_with_negated_wall_ghosts(c):
    """the pres tiles as a velocity component's rule would fill them behind a wall: the ghost layer negated"""
    P = np.array(c.pres_labs)
    for b, d, side in wall_faces(c):
        sl = [slice(None)] * 3
        sl[2 - d] = 9 if side else 0   # tile axes are z, y, x
        P[(b,) + tuple(sl)] *= -1.0
    return P


MASS_FLUX_CASES = ("one_block", "sixteen_mixed", "l012_wall")   # (1,1,1) level 0; (2,1,1) level 1, walls in y; three levels
UMAX_FORCED, DT, UINF = 1.3, 0.0125, (0.21, -0.4, 0.15)


def expected_mass_flux(name):
    key = ("mass_flux", name)
    if key not in _cache:
        c = case(name)
        _cache[key] = R.fix_mass_flux(c.vel, c.geom, UMAX_FORCED, NU, DT, c.extents, UINF)
        _cache[key][1].setflags(write=False)
    return _cache[key]
