"""Every BiCGSTAB iteration of the device's Helmholtz solves (cup3d_diffusion_solve <- DiffusionSolver::solve, main.cpp:6896-7146: the
routine of PoissonSolverAMR::solve on the operator of one velocity component) against tests/bicgstab_restatement.py, which
tests/test_helmholtz_restatement.py pins to the oracle's diff_solve bit for bit.  MI355X only (-m gpu), testing build.

The machinery is that of tests/test_gpu_bicgstab_iteration.py (its module docstring lists the checks per transition: eleven vector
updates bit for bit, every A u the oracle's diff_lhs(u, direction) bit for bit, every block solve inside
block_solve_exact.cg_bounds(rhs, h, centre) and equal to the stand-alone cup3d_diffusion_preconditioner, totals within
gamma sum|a_i b_i|, omega inside its interval, scalars = reference_step2 of the device's totals, init, pres = the x of the smallest norm),
run with the operator object below.  What differs from the pressure solver, and is asserted:
  * every iteration is host-driven (q.y and y.y are reported after each; t = A what is live in every state);
  * no mean constraint;
  * block solvers other than 2 are coerced to 0 (diffusion_params), and 1, 5 give the bits of 0;
  * io[11] reads 2^31 - 1 whatever params.max_restarts says: DiffusionSolver::solve has no cap (7096), so a solve asked for
    max_restarts = 0 still restarts.
Nothing here is a measured tolerance.  Worst observed ratios to the bounds are printed per sweep and recorded in tests/README.md."""
import ctypes as C

import numpy as np
import pytest

import cup3d_amd as cu
import helmholtz_cases as H
from cup3d_amd.capi import check, lib
from test_gpu_bicgstab_iteration import bits, check_sweep, read_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


class Helmholtz:
    """the operator object of check_sweep (class Poisson of tests/test_gpu_bicgstab_iteration.py) for the solve of one velocity component"""
    mc = 0
    restart_cap = H.UNBOUNDED

    def __init__(self, direction, block_solver=0, asked_block_solver=None, max_restarts=None):
        """block_solver: what the solve runs (0 or 2); asked_block_solver: what params.block_solver says (default: the same)"""
        self.direction, self.block_solver, self.max_restarts = direction, block_solver, max_restarts
        self.asked = block_solver if asked_block_solver is None else asked_block_solver
        self.label = f"direction {direction}, block solver {self.asked}" + ("" if max_restarts is None else f", max_restarts {max_restarts}")

    def sim(self, c, **kw):
        return cu.SimulationData(**{**c.sim_kw, **kw})

    def solve(self, c, sim, max_iter):
        p, r = cu.capi.PoissonParams(), cu.capi.PoissonResult()
        lib().cup3d_poisson_default_params(C.byref(p))
        p.tol, p.tol_rel, p.max_iter, p.block_solver = 0.0, 0.0, max_iter, self.asked
        if self.max_restarts is not None:
            p.max_restarts = self.max_restarts
        check(lib().cup3d_diffusion_solve(sim.handle, self.direction, c.dt, c.nu, C.byref(p), C.byref(r)))
        return r

    def A(self, c, u, mc=None):
        return c.oracle.diff_lhs(np.ascontiguousarray(u), self.direction, c.dt, c.nu)

    def centre(self, c):
        return c.centre

    def precondition(self, c, sim):
        """in place on pres; the sim evaluates the block CG as its last cup3d_preconditioner call or solve selected (0: production, 2: the
        reference's association), so that call comes first"""
        rhs = sim.download("pres")
        check(lib().cup3d_preconditioner(sim.handle, self.block_solver))
        sim.upload("pres", rhs)
        check(lib().cup3d_diffusion_preconditioner(sim.handle, c.dt, c.nu))

    def host_steps(self, k):
        return True


@pytest.mark.parametrize("block_solver", [0, 2])
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_eight_iterations_on_the_mixed_uniform_grid(direction, block_solver):
    """`mixed16`: 8 blocks, every one with wall, freespace and periodic faces; both associations of the block CG"""
    check_sweep(H.case("mixed16", direction), Helmholtz(direction, block_solver), 8)


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_twelve_iterations_on_the_three_level_mesh_from_a_nonzero_guess(direction):
    """`l012`: coarse/fine ghost slabs and the flux correction under the component's domain-face rule; the oracle's norm first rises
    at the 10th / 11th / 10th iteration (the device's own is asserted by the sweep)"""
    check_sweep(H.case("l012"), Helmholtz(direction), 12)


def test_x_opt_at_the_rounding_floor():
    """`l012_fast`: nu = 0.02, the solve is at its rounding floor after about four iterations and wanders"""
    check_sweep(H.case("l012_fast", 1), Helmholtz(1), 8)


def test_fifty_two_iterations_across_the_refresh():
    """`l012`, direction 1: k = 0, and 49 -> 50 -> 51 through the refresh form, all host-driven; no restart on the way"""
    check_sweep(H.case("l012"), Helmholtz(1), 52)


def test_a_solve_asked_for_no_restarts_restarts():
    """`l012`, direction 0 with params.max_restarts = 0: swept to the device's first restart + 2 (the oracle restarts in loop pass k = 31).
    The reference's Helmholtz solver has no cap, so the restart must happen, and io[10] counts it."""
    states = check_sweep(H.case("l012"), Helmholtz(0, max_restarts=0), 40, stop=lambda s: len(s) >= 3 and bool(s[-3]["io"][15]), need_restart=True)
    first = next(m for m, s in enumerate(states) if s["io"][15])
    print(f"    first restart at the end of iteration {first}")
    assert len(states) == first + 3
    assert [int(s["io"][10]) for s in states[first - 1:first + 2]] == [0, 1, 1]


def _solve_once(c, op, m):
    sim = op.sim(c)
    sim.upload("lhs", c.rhs)
    sim.upload("pres", c.x0)
    assert op.solve(c, sim, m).iterations == m
    return read_state(sim)


def _same_state(a, b):
    return set(a) == set(b) and all(bits(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_two_identical_solves_give_identical_bits():
    """what every sweep rests on: the state after m iterations is read from a solve of its own"""
    c = H.case("l012")
    a, b = _solve_once(c, Helmholtz(0), 12), _solve_once(c, Helmholtz(0), 12)
    assert _same_state(a, b), [k for k in a if not bits(np.asarray(a[k]), np.asarray(b[k]))]


@pytest.mark.parametrize("asked", [1, 5])
def test_other_block_solvers_are_coerced_to_the_block_cg(asked):
    """diffusion_params: the direct block solve and the multigrid are written for the Poisson coefficient"""
    c = H.case("mixed16", 1)
    a, b = _solve_once(c, Helmholtz(1, 0), 8), _solve_once(c, Helmholtz(1, 0, asked_block_solver=asked), 8)
    assert _same_state(a, b), [k for k in a if not bits(np.asarray(a[k]), np.asarray(b[k]))]


def test_four_iterations_over_two_ranks():
    """`l012` over two thread ranks (rank views of contiguous ranges): faces towards the other rank from ghost blocks, LHS split into
    inner and boundary blocks with the component's face rule carried over to the second ghost-fill pass, totals all-reduced before the
    scalars are stepped.  Four iterations are too few for the norms to rise (the one-rank sweeps above hold the x_opt bookkeeping)."""
    check_sweep(H.case("l012"), Helmholtz(1), 4, nranks=2, norms_must_rise=False)
