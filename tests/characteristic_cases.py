"""Inputs of the cup3d_create_obstacles tests and what tests/characteristic_restatement.py makes of them.  TEST INFRASTRUCTURE.

The three meshes of tests/fluid_momenta_cases.py: `uniform8` (16^3 cells in 8 blocks) and the goldens `f16_mixed` (8 blocks) and
`amr_periodic_l01` (15 blocks on two levels).  Each case has two obstacles whose signed distance is analytic, evaluated at the cell
centres of the blocks and of their one-cell ghost layer (sdfLab), and both list EVERY block of the mesh, so that blocks the body does not
reach (chi == 0, no point) and blocks it swallows (chi == 1, no point) are among them:

  A  a sphere, R = 1.3 at (3.3, 3.0, 3.2), with noise of 0.05 h on the distance (gradUSq != 1) and, in its first block, two band cells
     set to +h and -h exactly (they take the band branch: the test is `>`); blocks in ascending slot order; oldCorrVel = 0
  B  a sphere, R = 3.2 at (1.6, 1.5, 1.7), that overlaps A (the max into the chi field matters) and contains whole blocks; blocks in
     DESCENDING slot order; oldCorrVel != 0

udef is a rigid motion plus noise, so that both corrections are far from zero.  tests/test_characteristic_cases.py asserts the paths these
inputs take.  The restatement is evaluated once per (case, geometry) and its results are never modified."""
import numpy as np

import characteristic_restatement as R
import cup3d_amd as cu
import fluid_momenta_cases as FC

NAMES = FC.NAMES
EXT = FC.EXT
_cases, _expected = {}, {}


def sdf_tiles(geom, ids, dist):
    """sdfLab of the listed blocks: dist(x, y, z) at the centres of the cells -1..8, index [z+1][y+1][x+1]"""
    out = np.zeros((len(ids), 10, 10, 10))
    i = np.arange(-1, 9) + 0.5
    for n, b in enumerate(ids):
        h, o = geom[b, 0], geom[b, 1:4]
        z, y, x = np.meshgrid(o[2] + h * i, o[1] + h * i, o[0] + h * i, indexing="ij")
        out[n] = dist(x, y, z)
    return out


def sphere(c, radius):
    return lambda x, y, z: radius - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


def grid_of(name):
    """the mesh of the case as a host-side Grid (no GPU): its geom [nb][4] = h, origin is what the device operator uses"""
    c = FC.case(name)
    if c.leaves is None:
        return cu.operators.Grid(c.bpd, c.lmax, c.sim_kwargs["levelStart"], EXT, c.bc)
    return cu.operators.Grid(c.bpd, c.lmax, 0, EXT, c.bc, leaves=c.leaves)


class Case:
    """sim_kwargs, nb, geom [nb][4], obstacles = [A, B]: dicts with ids, sdf, udef, transvel_correction"""


def case(name):
    if name in _cases:
        return _cases[name]
    f = FC.case(name)
    c = Case()
    c.name, c.sim_kwargs, c.nb, c.bpd, c.lmax, c.bc, c.leaves = name, f.sim_kwargs, f.nb, f.bpd, f.lmax, f.bc, f.leaves
    c.tables = getattr(f, "tables", None)
    c.geom = grid_of(name).geom.copy()
    assert len(c.geom) == c.nb
    rng = np.random.default_rng(33)
    ids = np.arange(c.nb, dtype=np.int64)

    def udef(ids, seed):
        r = np.random.default_rng(seed)
        u = 0.05 * r.uniform(-1, 1, (len(ids), 8, 8, 8, 3))
        i = np.arange(8) + 0.5
        for n, b in enumerate(ids):
            h, o = c.geom[b, 0], c.geom[b, 1:4]
            z, y, x = np.meshgrid(o[2] + h * i, o[1] + h * i, o[0] + h * i, indexing="ij")
            u[n, ..., 0] += 0.3 + 0.2 * (z - 3.0) - 0.1 * (y - 3.0)
            u[n, ..., 1] += -0.2 + 0.1 * (x - 3.0) + 0.15 * (z - 3.0)
            u[n, ..., 2] += 0.1 - 0.15 * (y - 3.0) - 0.2 * (x - 3.0)
        return u

    sa = sdf_tiles(c.geom, ids, sphere((3.3, 3.0, 3.2), 1.3))
    sa += 0.05 * c.geom[ids, 0][:, None, None, None] * rng.uniform(-1, 1, sa.shape)
    # two band cells of the first block the sphere's surface crosses: +h and -h exactly
    first = next(n for n in range(len(ids)) if (np.abs(sa[n, 1:9, 1:9, 1:9]) < 0.5 * c.geom[ids[n], 0]).sum() >= 2)
    zz, yy, xx = np.where(np.abs(sa[first, 1:9, 1:9, 1:9]) < 0.5 * c.geom[ids[first], 0])
    sa[first, zz[0] + 1, yy[0] + 1, xx[0] + 1] = +c.geom[ids[first], 0]
    sa[first, zz[1] + 1, yy[1] + 1, xx[1] + 1] = -c.geom[ids[first], 0]
    a = dict(ids=ids, sdf=sa, udef=udef(ids, 34), transvel_correction=np.zeros(3))
    idb = ids[::-1].copy()
    b = dict(ids=idb, sdf=sdf_tiles(c.geom, idb, sphere((1.6, 1.5, 1.7), 3.2)), udef=udef(idb, 35), transvel_correction=np.array([0.01, -0.02, 0.03]))
    c.obstacles = [a, b]
    # a body of no volume anywhere (chi == 0): the reference's assert(com[0] > epsilon)
    c.nothing = dict(ids=ids, sdf=np.full((c.nb, 10, 10, 10), -10.0), udef=udef(ids, 36), transvel_correction=np.zeros(3))
    _cases[name] = c
    return c


def expected(name, geom=None):
    """(chi field, [Result A, Result B], [Result A, Result B] of a second call with the first one's transvel_correction, trace of the
    first call) on the given geometry (default: the case's own)"""
    c = case(name)
    geom = c.geom if geom is None else np.asarray(geom)
    key = (name, geom.tobytes())
    if key not in _expected:
        trace = set()
        field, first = R.create(geom, c.nb, c.obstacles, trace)
        again = [dict(o, transvel_correction=r.transvel_correction) for o, r in zip(c.obstacles, first)]
        field2, second = R.create(geom, c.nb, again)
        assert np.array_equal(field, field2)   # chi does not depend on udef
        _expected[key] = (field, first, second, trace)
    return _expected[key]
