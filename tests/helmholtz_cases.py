"""The meshes, fields and operator callables of the implicit-diffusion tests (DiffusionSolver::solve, main.cpp:6896-7146, and
AdvectionDiffusionImplicit::euler, 10030-10118), shared by tests/test_helmholtz_restatement.py (CPU), tests/test_gpu_helmholtz_iteration.py,
tests/test_gpu_implicit_step.py and tests/test_gpu_multirank.py (MI355X): every case is built once per process and never edited afterwards.

  mixed16        uniform (1,1,1) level 1, 8 blocks, wall / freespace / periodic, dt 0.05, nu 100 (h^2 / (nu dt) = 0.03: close enough to
                 the Poisson operator for norms that rise within 8 iterations -- at nu = 2 none of 40 seeds gave that); one right-hand
                 side per direction (MIXED16_SEEDS)
  l012           the three-level mesh synthetic_l012 (22 blocks, wall / freespace / wall), dt 0.05, nu 2.0, rhs default_rng(3), x0
                 default_rng(4): 40 / 66 / 40 iterations at 1e-12 / 1e-11 for directions 0 / 1 / 2 on the oracle; directions 0 and 2
                 restart in loop pass k = 31, direction 1 restarts nowhere and passes the k = 50 refresh
  l012_fast      the same mesh with nu = 0.02: the solve is at its rounding floor after about four iterations and wanders from there
                 (the x_opt bookkeeping at work); one right-hand side per direction (FAST_SEEDS)
  uniform_mixed  the uniform grid of tests/test_gpu_amr.py's make_implicit: (2,1,2) level 1, freespace / wall / periodic
  grid1280       (5,4,1) level 2, wall / periodic / freespace: 1280 blocks, so every grid-stride loop of the step's pointwise passes
                 (2048 x 256 threads) takes a second trip; stencils only, no solve

Every case also carries the input of a whole step: vel = 0.5 default_rng(6) (pres drawn behind it), uinf = (0.1, -0.2, 0.3)."""
import numpy as np

import oracle_lib as O
from bicgstab_cases import EXT, U, gamma, synthetic_mesh  # noqa: F401  (gamma, U: for the tests that import this module as their cases)

UINF = (0.1, -0.2, 0.3)
UNBOUNDED = 2 ** 31 - 1   # hs.max_restarts of a Helmholtz solve: the reference's DiffusionSolver has no cap (7096)
# right-hand-side seeds per direction for which the oracle's norms over 8 iterations from x0 = 0 are not monotone, with no restart on the
# way (tests/test_helmholtz_restatement.py asserts it; the device sweeps assert their own).  mixed16: the first of 40 seeds that do
FAST_SEEDS = (0, 1, 0)
MIXED16_SEEDS = (37, 31, 37)
PER_DIRECTION = ("mixed16", "l012_fast")
_BUILT = {}


def uniform_leaves(bpd, level_max, level):
    """(levels, Zs) of the uniform grid at `level`"""
    sfc = O.lib().orc_sfc_create(int(bpd[0]), int(bpd[1]), int(bpd[2]), int(level_max))
    zs = [O.lib().orc_sfc_forward(sfc, level, i, j, k) for k in range(bpd[2] << level) for j in range(bpd[1] << level) for i in range(bpd[0] << level)]
    O.lib().orc_sfc_destroy(sfc)
    return np.full(len(zs), level, dtype=np.int32), np.array(zs, dtype=np.int64)


class Case:
    """oracle: OracleMesh; rhs, x0: [nb, 8, 8, 8] of a stand-alone solve; h: spacing per block; vel, pres: the input of a whole step;
    sim_kw: what cu.SimulationData takes to build the same mesh"""
    corner = 0

    def __init__(self, name, oracle, h, dt, nu, rhs, x0, sim_kw, uniform):
        self.name, self.oracle, self.h, self.dt, self.nu, self.rhs, self.x0, self.sim_kw, self.uniform = name, oracle, h, dt, nu, rhs, x0, sim_kw, uniform
        nb = oracle.nb
        rng = np.random.default_rng(6)
        self.vel = 0.5 * rng.uniform(-1, 1, (nb, 8, 8, 8, 3))
        self.pres = rng.uniform(-1, 1, (nb, 8, 8, 8))
        self.uinf = UINF
        self.h3 = (h * h * h).reshape(-1, 1, 1, 1) * np.ones((1, 8, 8, 8))
        # the block solve's centre coefficient as the kernel and tests/test_gpu_block_preconditioner.py evaluate it (10534-10579)
        self.centre = -6.0 - h * h / nu / dt
        for a in (self.rhs, self.x0, self.h, self.h3, self.vel, self.pres, self.centre):
            a.setflags(write=False)

    def A(self, direction):
        return lambda u: self.oracle.diff_lhs(np.ascontiguousarray(u), direction, self.dt, self.nu)

    def Minv(self, u):
        return self.oracle.diff_precond(u, self.dt, self.nu)

    def zero_corner(self, mc):
        return None   # no mean constraint in a Helmholtz solve

    def oracle_solve(self, direction, tol, tol_rel, rhs=None, x0=None):
        x, info = self.oracle.diff_solve(self.rhs if rhs is None else rhs, self.x0 if x0 is None else x0, direction, self.dt, self.nu, tol, tol_rel)
        return x, info.iters, info.restarts

    # ---- the callables of tests/implicit_step_restatement.py
    def advect(self, sequential=False):
        return lambda vel: self.oracle.advect_implicit(vel, self.dt, self.nu, self.uinf, sequential)

    def diffusion_rhs(self, vel):
        return self.oracle.diffusion_rhs(vel)

    def oracle_solver(self, tol, tol_rel):
        return lambda rhs, x0, direction: self.oracle.diff_solve(rhs, x0, direction, self.dt, self.nu, tol, tol_rel)[0]


def _uniform(name, bpd, lmax, level, bc, dt, nu, seed):
    lv, zs = uniform_leaves(bpd, lmax, level)
    m = O.OracleMesh(bpd, lmax, EXT, bc, lv, zs)
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    h = np.array([m.h(b) for b in range(m.nb)])
    assert np.ptp(h) == 0
    rhs = np.random.default_rng(seed).uniform(-1, 1, (m.nb, 8, 8, 8))
    return Case(name, m, h, dt, nu, rhs, np.zeros((m.nb, 8, 8, 8)), kw, True)


def case(name, direction=0):
    """mixed16 and l012_fast take the direction whose right-hand side they carry"""
    key = (name, direction if name in PER_DIRECTION else None)
    if key in _BUILT:
        return _BUILT[key]
    if name == "mixed16":
        c = _uniform(f"mixed16[{direction}]", (1, 1, 1), 2, 1, ("wall", "freespace", "periodic"), 0.05, 100.0, MIXED16_SEEDS[direction])
    elif name == "uniform_mixed":
        c = _uniform(name, (2, 1, 2), 3, 1, ("freespace", "wall", "periodic"), 0.05, 2.0, 3)
    elif name == "grid1280":
        c = _uniform(name, (5, 4, 1), 3, 2, ("wall", "periodic", "freespace"), 0.05, 2.0, 3)
    elif name in ("l012", "l012_fast"):
        bpd, lmax, bc, lv, zs = synthetic_mesh()
        m = O.OracleMesh(bpd, lmax, EXT, bc, lv, zs)
        kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], leaves=(lv, zs))
        h = np.array([m.h(b) for b in range(m.nb)])
        if name == "l012":
            rhs, x0, nu = np.random.default_rng(3).uniform(-1, 1, (m.nb, 8, 8, 8)), np.random.default_rng(4).uniform(-1, 1, (m.nb, 8, 8, 8)), 2.0
        else:
            rhs, x0, nu = np.random.default_rng(FAST_SEEDS[direction]).uniform(-1, 1, (m.nb, 8, 8, 8)), np.zeros((m.nb, 8, 8, 8)), 0.02
            name = f"l012_fast[{direction}]"
        c = Case(name, m, h, 0.05, nu, rhs, x0, kw, False)
    else:
        raise KeyError(name)
    _BUILT[key] = c
    return c
