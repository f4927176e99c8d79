"""The seeded inputs of the device tests of cup3d_compute_forces (tests/test_gpu_surface_forces.py, tests/test_gpu_surface_forces_over_ranks.py)
and what the restatement (tests/surface_forces_restatement.py) makes of them on the CPU oracle's tiles; tests/test_surface_forces_cases.py
(no GPU) shows that they take every path of the functor.  A helper module, not a test file.

Per mesh: vel and pres uniform in [-1, 1], chi uniform in [0, 0.05] (the march along the normal breaks at chi < 0.01: at random depths),
two obstacles.  Obstacle A has ObstacleBlocks with 1, 63, 64, 65 and 200 surface points and one with none, which is left out of the
slot list as main.cpp:12280 skips it; its normals are uniform in [-1, 1]^3 with |n| >= 0.1, plus, in the block of 200, the six axis
directions at ix / iy / iz in {0, 7} (the only way to the 2-point derivative branches and to the `continue` guards of the march); the
block of 65 lists one cell twice.  Obstacle B does not translate (vel = 0: vel_norm <= 1e-9) and shares a block with A."""
import os

import numpy as np

import oracle_lib as O
import surface_forces_restatement as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXT = 2 * np.pi
NU = 0.02
# name -> bpd, levelMax, level, bc: the uniform grids of tests/test_gpu_labs.py, and the 64-block grid of the over-ranks tests
UNIFORM = {
    "one_block_periodic": ((1, 1, 1), 1, 0, ("periodic", "periodic", "periodic")),
    "box321_every_bc": ((3, 2, 1), 1, 0, ("periodic", "wall", "freespace")),
    "box222_wall": ((2, 2, 2), 1, 0, ("wall", "wall", "wall")),
    "uniform64": ((2, 2, 2), 2, 1, ("periodic", "wall", "freespace")),
}
GOLDEN = ("amr_periodic_l01", "amr_mixed_l12")   # h differs per block, tiles have coarser and finer neighbours
SINGLE_RANK = ("one_block_periodic", "box321_every_bc", "box222_wall") + GOLDEN
COUNTS_A = (1, 63, 64, 65, 200)
COUNTS_B = (40, 30)

ALL_PATHS = {f"dveld{a}_{k}" for a in "xyz" for k in (6, 3, 2)} | {f"dveld{m}_{k}" for m in ("xdy", "ydz", "xdz") for k in ("full", "fallback")} | \
    {f"break_at_{k}" for k in range(5)} | {"no_break", "continue_x", "continue_y", "continue_z", "forcePar>0", "forcePar<0", "powOut<0", "powOut>=0",
                                           "powDef<0", "powDef>=0", "vel_norm>1e-9", "vel_norm<=1e-9"}


def mesh_recipe(name):
    """bpd, levelMax, level (None on a multi-level mesh), bc (names), extent, levels, Zs"""
    if name in UNIFORM:
        bpd, lmax, level, bc = UNIFORM[name]
        t = O.OracleGrid(bpd, lmax, level, EXT, bc).tables
        return bpd, lmax, level, bc, EXT, t[:, 0].astype(np.int32), t[:, 1].copy()
    g = np.load(os.path.join(GOLD, name + ".npz"))
    t = g["tables"]
    return (tuple(int(b) for b in g["bpd"]), int(g["level_max"]), None, tuple(O.BC_NAMES[int(b)] for b in g["bc"]), float(g["extent"]),
            t[:, 0].astype(np.int32), t[:, 1].copy())


def _normals(rng, n):
    out = np.zeros((n, 3))
    for i in range(n):
        while True:
            v = rng.uniform(-1, 1, 3)
            if np.sqrt((v * v).sum()) >= 0.1:
                break
        out[i] = v
    return out


def _block_points(rng, count, axis_points, twice):
    ijk = rng.integers(0, 8, (count, 3)).astype(np.int32)
    dchi = _normals(rng, count)
    if axis_points:   # the six axis directions where they run out of the tile: 8 points each, at the block face the normal leaves through
        k = 0
        for a in range(3):
            for sgn in (+1.0, -1.0):
                for _ in range(8):
                    ijk[k, a] = 7 if sgn > 0 else 0
                    dchi[k] = 0.0
                    dchi[k, a] = sgn * rng.uniform(0.5, 2.0)
                    k += 1
    if twice:
        ijk[1] = ijk[0]
    return ijk, dchi


def make_obstacles(nb, seed):
    """The two obstacles for a mesh of nb blocks (slots repeat when the mesh has fewer blocks than the obstacle): dicts with slots, first,
    ijk, dchi, udef, cm, vel, omega, qoi (the sums before the first call: random, so that a sum that should restart from zero and does
    not is seen), and `empty_slot`, the block of A that has no surface point."""
    rng = np.random.default_rng(seed)
    s0 = (nb // 2 - 2) % nb
    out = []
    for which, counts in (("A", COUNTS_A), ("B", COUNTS_B)):
        if which == "A":
            slots = [(s0 + j) % nb for j in range(len(counts))]
        else:
            slots = [out[0]["slots"][-1], (out[0]["slots"][-1] + 1) % nb]
        parts = [_block_points(rng, c, axis_points=(c == 200), twice=(c == 65)) for c in counts]
        o = dict(slots=np.array(slots, dtype=np.int32), first=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                 ijk=np.concatenate([p[0] for p in parts]), dchi=np.concatenate([p[1] for p in parts]),
                 udef=rng.uniform(-1, 1, (len(counts), 8, 8, 8, 3)), cm=rng.uniform(0, EXT, 3),
                 vel=rng.uniform(-1, 1, 3) if which == "A" else np.zeros(3), omega=rng.uniform(-1, 1, 3),
                 qoi=rng.uniform(-1, 1, (len(counts), 19)))
        if which == "A":
            o["empty_slot"] = (s0 + len(counts)) % nb
        out.append(o)
    return out


class Expected:
    """A mesh with its seeded fields and obstacles, the oracle's [-4,5) tiles and the restatement's results of two calls in a row (the
    second starts from the sums the first returned).  Built once per mesh, never modified."""

    def __init__(self, name):
        self.name = name
        self.bpd, self.lmax, self.level, self.bc, self.ext, lv, zs = mesh_recipe(name)
        self.m = O.OracleMesh(self.bpd, self.lmax, self.ext, self.bc, lv, zs)
        self.nb = nb = self.m.nb
        t = self.m.tables
        self.leaves = (t[:, 0].astype(np.int32), t[:, 1].copy())
        rng = np.random.default_rng(100 + len(name))
        self.vel, self.pres, self.chi = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8)), rng.uniform(0, 0.05, (nb, 8, 8, 8))
        self.hs = np.array([self.m.h(b) for b in range(nb)])
        self.origins = t[:, 2:5] * 8 * self.hs[:, None]   # Info::origin, main.cpp:1066-1068
        self.vel_tiles = self.m.labs(self.vel, -4, 5, True)
        self.chi_tiles = self.m.labs(self.chi, -4, 5, True)
        self.obstacles = make_obstacles(nb, 7 + len(name))
        self.trace = set()
        self.first_call = [R.compute_forces(self.vel_tiles, self.chi_tiles, self.pres, self.hs, self.origins, NU, o, trace=self.trace) for o in self.obstacles]
        self.second_call = [R.compute_forces(self.vel_tiles, self.chi_tiles, self.pres, self.hs, self.origins, NU, o, qoi_in=q)
                            for o, (_, q) in zip(self.obstacles, self.first_call)]

    def sim_kwargs(self):
        return dict(bpdx=self.bpd[0], bpdy=self.bpd[1], bpdz=self.bpd[2], levelMax=self.lmax, extent=self.ext, nu=NU, BC_x=self.bc[0], BC_y=self.bc[1],
                    BC_z=self.bc[2])


_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = Expected(name)
    return _expected[name]
