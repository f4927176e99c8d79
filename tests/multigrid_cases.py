"""The cases, inputs and the tolerance of the V-cycle tests, shared by tests/test_multigrid_restatement.py (CPU: the mutation catalogue runs
over exactly what the GPU tests use), tests/test_gpu_multigrid_cycle.py and the over-ranks cases of tests/test_gpu_multirank.py.
TEST INFRASTRUCTURE."""
import numpy as np

import multigrid_restatement as R
import oracle_lib as O

EXT = 2 * np.pi
EPS = float(np.finfo(np.float64).eps)
MARGIN = 32         # FMA contraction in the kernels, the order of the 256-thread sum of the mean, over ranks the all-reduce
MUTATION_FACTOR = 1e6

# (bpd, level, bc): the smallest shapes at which each piece of the cycle can go wrong; none exceeds 128 blocks
UNIFORM = {
    "one_block_wall": ((1, 1, 1), 0, ("wall", "wall", "wall")),                  # 1 x 64 sweeps, every face a domain face
    "one_block_periodic": ((1, 1, 1), 0, ("periodic", "periodic", "periodic")),  # a block that is its own neighbour
    "one_level_8_blocks": ((2, 2, 2), 0, ("wall", "periodic", "freespace")),     # 16 x 4 launches, frozen ghosts, NO mean removal
    "two_levels": ((1, 1, 1), 1, ("wall", "wall", "wall")),                      # restrict, mean, prolong
    "three_levels_211": ((2, 1, 1), 2, ("freespace", "wall", "periodic")),       # non-cubic, parent / octant mapping
    "box_321": ((3, 2, 1), 1, ("periodic", "wall", "wall")),                     # a box that is not a power of two
}
MESHES = ("l012_wall", "l012_periodic", "l012_box322")
INPUTS = ("random", "constant", "impulses")
SCHEDULES = ((1, 3), (3, 1))                       # (mg_launches, mg_sweeps) beside the default (2, 2)
SCHEDULE_CASES = ("two_levels", "three_levels_211")
RANKS_CASE = ((1, 1, 1), 2, ("wall", "wall", "wall"))   # over 2 and 4 ranks: the hierarchy stops at level 1, 16 x 4 there


def mesh_case(name):
    if name == "l012_wall":
        bpd, lmax, bc = (2, 2, 2), 3, ("wall", "freespace", "wall")
        lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 0, 0, 0), (1, 0, 0, 0)])
    elif name == "l012_periodic":
        bpd, lmax, bc = (2, 2, 2), 3, ("periodic", "periodic", "periodic")
        lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 1, 1, 1), (1, 2, 2, 2), (1, 3, 3, 3)])
    else:  # a non-cubic box, mixed boundary conditions
        bpd, lmax, bc = (3, 2, 2), 3, ("periodic", "wall", "freespace")
        lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 2, 1, 0), (1, 4, 2, 1), (0, 0, 0, 1)])
    return bpd, lmax, bc, lv, zs


def uniform_input(kind, bpd, level, seed=31):
    """Dense (Z, Y, X) right-hand side of a uniform case."""
    shape = tuple(8 * (b << level) for b in bpd[::-1])
    if kind == "random":
        return np.random.default_rng(seed).uniform(-1, 1, shape)
    if kind == "constant":
        return np.full(shape, 0.75)
    # unit impulses at the eight corner cells of one block (the middle one: an interior block where the grid has one), distinct weights:
    # every face and octant of that block answers with its own number
    r = np.zeros(shape)
    o = [8 * ((s // 8) // 2) for s in shape]
    for q in range(8):
        r[o[0] + 7 * (q >> 2), o[1] + 7 * ((q >> 1) & 1), o[2] + 7 * (q & 1)] = 1.0 + 0.25 * q
    return r


def oracle_mesh(name):
    """(OracleMesh, restatement Mesh in the oracle's block order) of a multi-level case."""
    bpd, lmax, bc, lv, zs = mesh_case(name)
    m = O.OracleMesh(bpd, lmax, EXT, bc, lv, zs)
    return m, R.Mesh(bpd, bc, EXT / (8 * max(bpd)), m.tables[:, [0, 2, 3, 4]])


def mesh_input(nb, seed=37):
    return np.random.default_rng(seed).uniform(-1, 1, (nb, 8, 8, 8))


def tolerance(z64, zld):
    """max|z_dev - z_ld| may be MARGIN x the larger of: the float64 restatement's own distance from the longdouble one, 4 eps max|z_ld|."""
    return MARGIN * max(float(np.abs(z64 - zld).max()), 4 * EPS * float(np.abs(zld).max()))


_CACHE = {}


def restated(key, fn):
    """(z_f64, z_longdouble) of fn(dtype), computed once per key and shared (read-only) among the tests that need it."""
    if key not in _CACHE:
        pair = (fn(np.float64), fn(np.longdouble))
        for a in pair:
            a.setflags(write=False)
        _CACHE[key] = pair
    return _CACHE[key]


def restated_uniform(case, kind, launches=2, sweeps=2, **kw):
    bpd, level, bc = RANKS_CASE if case == "ranks" else UNIFORM[case]
    h = EXT / (8 * (max(bpd) << level))
    r = uniform_input(kind, bpd, level)
    return r, restated((case, kind, launches, sweeps), lambda dt: R.vcycle_uniform(r, bpd, level, bc, h, dtype=dt, launches=launches, sweeps=sweeps, **kw))
