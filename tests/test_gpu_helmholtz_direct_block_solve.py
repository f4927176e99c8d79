"""The direct 8^3 block solve of the implicit diffusion's Helmholtz operator (k_precond_fdm_helm: fast diagonalisation with the eigenvalues
shifted by -h^2/(nu dt) per block), selected per sim with cup3d_diffusion_set_block_solver(sim, 1) / SimulationData(diffusionBlockSolver=1).
Runs on an MI355X only (-m gpu).

  exactness        cup3d_diffusion_preconditioner in mode 1 against tests/block_solve_exact.py block by block on the four grids of
                   tests/test_gpu_block_preconditioner.py, h^2/(nu dt) in {0.01, 1, 100} on the coarsest blocks:
                   max|z - z_exact| <= FDM_TOL max|z_exact| (5e-14, the project's bound for the worse-conditioned Poisson solve, not
                   re-fitted), skipped blocks exact zeros, nothing NaN; the assembled Green's function symmetric to the same bound
  mode 0           a sim that was in mode 1 and went back gives the bits of one that never left mode 0
  scale covariance z(2^k r) == 2^k z(r) bit for bit (IEEE operations only)
  solver           cup3d_diffusion_solve in mode 1 against the oracle's solve: the two-valid-iterates bound of tests/test_gpu_parity.py under the
                   oracle's Helmholtz operator, ||A (x_dev - x_oracle)|| <= 2.02 tau + 1e-13 max|x_oracle|, and iterations <= 1.1 oracle + 2
                   (iters_close for an exact block solve)
  step             cup3d_advect_diffuse_implicit in mode 1 is the restated passes around three stand-alone mode-1 solves, bit for bit
  over ranks       the block solve on two thread ranks is the one-rank bits; the solve meets the solver bound
  interface        other modes are refused; adapted() keeps the mode

Worst observed ratios are printed by each test.  On an MI355X (46 tests, 1.6 s in all): exactness 2.5e-15 ... 3.0e-15 of max|z_exact| on the
twelve grid x shift cases (medians 7e-16 ... 1.5e-15; bound 5e-14), Green's function asymmetry <= 6.7e-16, the adapted mesh 1.0e-15; solver
||A (x_dev - x_oracle)|| <= 0.351 tau (below 5e-4 tau at 1e-6 / 1e-4), iteration counts equal to the oracle's on 21 of the 24 solves and
15 / 16 / 15 against 16 / 15 / 16 for the three directions of `l012` at 1e-9 / 1e-7 (2 ... 21 iterations); over two ranks 0.213 tau, 16
iterations against 15; the mode-1 step 14 / 17 / 17 (`uniform_mixed`) and 23 / 21 / 21 (`l012`) iterations at 1e-12 / 1e-11, 6e-9 / 2.6e-8
away from the mode-0 step of a velocity change of 0.5.  DESIGN.md section 5b carries the same figures."""
import ctypes as C

import numpy as np
import pytest

import block_solve_exact as X
import cup3d_amd as cu
import helmholtz_cases as H
import test_gpu_block_preconditioner as B
from cup3d_amd.capi import PoissonParams, PoissonResult, check, lib
from test_gpu_bicgstab_iteration import bits
from test_gpu_block_preconditioner import FDM_TOL, GRIDS, case
from test_gpu_implicit_step import FIELDS, assert_step_without_iterations, device_step, params, restated_without_iterations
from test_gpu_parity import iters_close

pytestmark = pytest.mark.gpu
NU = 0.5
SHIFTS = [0.01, 1.0, 100.0]
SOLVER_CASES = ["mixed16", "uniform_mixed", "l012", "l012_fast"]
TOLS = [(1e-6, 1e-4), (1e-9, 1e-7)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)
    yield
    B._CASES.clear()
    _ORACLE.clear()


class direct:
    """mode 1 on a sim other tests share, for the body of the with-statement; the block CG behind it"""

    def __init__(self, sim):
        self.sim = sim

    def __enter__(self):
        check(lib().cup3d_diffusion_set_block_solver(self.sim.handle, 1))

    def __exit__(self, *a):
        check(lib().cup3d_diffusion_set_block_solver(self.sim.handle, 0))


def helm_precond(sim, rhs, dt, nu):
    """cup3d_diffusion_preconditioner, in place on pres, as the sim's mode says"""
    sim.upload("pres", rhs)
    check(lib().cup3d_diffusion_preconditioner(sim.handle, dt, nu))
    return sim.download("pres")


def assert_exact(z, rhs, h, centre, what, kinds=None):
    """the exactness bound per block; returns the worst ratio max|z - z_exact| / max|z_exact|"""
    assert np.isfinite(z).all(), what
    sk = X.skipped(rhs, h)
    assert (z[sk] == 0).all(), f"{what}: a block below the 1e-32 threshold is not exactly 0"
    zx = X.exact_block_solve(rhs, h, centre)
    n = len(z)
    d = np.abs(z - zx).reshape(n, -1).max(axis=1)
    m = np.abs(zx).reshape(n, -1).max(axis=1)
    ratio = (d / np.where(sk, 1.0, m))[~sk]
    print(f"{what}: max|z - z_exact| / max|z_exact| worst {ratio.max():.3e}, median {np.median(ratio):.3e} ({(~sk).sum()} solved blocks, {sk.sum()} skipped)")
    bad = np.where(~sk & (d > FDM_TOL * m))[0]
    assert not len(bad), f"{what}: blocks {bad[:8]} ({None if kinds is None else kinds[bad[:8]]}): worst {ratio.max():.3e} > {FDM_TOL}"
    return float(ratio.max())


# ------------------------------------------------------------------ 1. exactness
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("grid", GRIDS)
def test_direct_helmholtz_block_solve_is_exact(golden_dir, grid, shift):
    sim, rhs, h, kinds = case(grid, golden_dir)
    dt = h.max() ** 2 / NU / shift
    centre = -6.0 - h * h / NU / dt          # as the kernel evaluates it
    with direct(sim):
        z = helm_precond(sim, rhs, dt, NU)
    assert_exact(z, rhs, h, centre, f"{grid}: Helmholtz direct solve, shift {shift}", kinds)
    if grid == "green":
        G = z.reshape(512, 512)   # row b = h^-1 A^-1 e_b
        asym = np.abs(G - G.T).max() / np.abs(G).max()
        print(f"green: shift {shift}: |G - G^T| / max|G| = {asym:.3e}")
        assert asym <= FDM_TOL


# ------------------------------------------------------------------ 2. mode 0 is untouched
def _solve(c, sim, direction, tol, tol_rel, max_iter=None):
    sim.upload("lhs", c.rhs)
    sim.upload("pres", c.x0)
    p, r = params(tol, tol_rel, max_iter), PoissonResult()
    check(lib().cup3d_diffusion_solve(sim.handle, direction, c.dt, c.nu, C.byref(p), C.byref(r)))
    return sim.download("pres"), r


def test_mode_0_after_mode_1_is_the_block_cg_bit_for_bit():
    c = H.case("mixed16", 1)
    fresh, back = cu.SimulationData(**c.sim_kw), cu.SimulationData(**c.sim_kw)
    check(lib().cup3d_diffusion_set_block_solver(back.handle, 1))
    z1 = helm_precond(back, c.rhs, c.dt, c.nu)
    x1, _ = _solve(c, back, 1, 0.0, 0.0, max_iter=8)
    check(lib().cup3d_diffusion_set_block_solver(back.handle, 0))
    z0 = helm_precond(fresh, c.rhs, c.dt, c.nu)
    assert bits(helm_precond(back, c.rhs, c.dt, c.nu), z0)
    assert not bits(z1, z0), "mode 1 gave the block CG's bits: the setting does nothing"
    xa, ra = _solve(c, fresh, 1, 0.0, 0.0, max_iter=8)
    xb, rb = _solve(c, back, 1, 0.0, 0.0, max_iter=8)
    assert ra.iterations == 8 and bits(xa, xb) and not bits(xa, x1)
    for f in FIELDS:
        assert getattr(ra, f) == getattr(rb, f), f


# ------------------------------------------------------------------ 3. scale covariance
@pytest.mark.parametrize("shift", SHIFTS)
def test_scale_covariance(golden_dir, shift):
    """z(2^k r) for k in {-8, 8, 40} is exactly 2^k z(r): transforms by FMA and IEEE divisions only, on blocks clear of the 1e-32 threshold"""
    sim, _, h, _ = case("edge", golden_dir)
    rng = np.random.default_rng(9)
    blocks = []
    while len(blocks) < sim.nblocks:
        blocks += [b for _, b in X.edge_blocks(rng, kinds=("random", "constant", "spike", "lowest_mode"))]
    rhs = np.ascontiguousarray(blocks[:sim.nblocks])
    assert not X.skipped(rhs * 2.0 ** -8, h).any()
    dt = h.max() ** 2 / NU / shift
    with direct(sim):
        base = helm_precond(sim, rhs, dt, NU)
        assert_exact(base, rhs, h, -6.0 - h * h / NU / dt, f"edge: scale 1, shift {shift}")
        for k in (-8, 8, 40):
            s = 2.0 ** k
            z = helm_precond(sim, rhs * s, dt, NU)
            diff = np.where(z != base * s)
            assert not len(diff[0]), f"k = {k}: {len(diff[0])} cells differ, first block {diff[0][0]}"


# ------------------------------------------------------------------ 4. solver
_ORACLE = {}


def oracle_solve(name, direction, tol, tol_rel):
    """the oracle's solve of one case, computed once"""
    key = (name, direction, tol, tol_rel)
    if key not in _ORACLE:
        x, iters, restarts = H.case(name, direction).oracle_solve(direction, tol, tol_rel)
        x.setflags(write=False)
        _ORACLE[key] = (x, iters, restarts)
    return _ORACLE[key]


def assert_solver_bound(c, direction, tol, tol_rel, x_dev, r_dev, x_or, it_or, what):
    """two valid iterates under the oracle's operator, and the iteration rule of an exact block solve; prints both ratios"""
    tau = max(tol, tol_rel * r_dev.norm0)
    nrm = np.linalg.norm(c.A(direction)(x_dev - x_or).ravel())
    bound = 2.02 * tau + 1e-13 * np.abs(x_or).max()
    print(f"{what}: ||A (x_dev - x_oracle)|| / tau = {nrm / tau:.3f} (/ bound {nrm / bound:.3f}); iterations {r_dev.iterations} (oracle {it_or}), "
          f"restarts {r_dev.restarts}, norm0 {r_dev.norm0:.3e}, norm {r_dev.norm:.3e}")
    assert np.isfinite(x_dev).all()
    assert nrm <= bound, f"{what}: ||A (x_dev - x_oracle)|| = {nrm:.3e} > 2.02 tau + 1e-13 max|x| = {bound:.3e}"
    assert iters_close(r_dev.iterations, it_or, block_solver=1), f"{what}: {r_dev.iterations} iterations, oracle {it_or}"


@pytest.mark.parametrize("tol,tol_rel", TOLS)
@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("name", SOLVER_CASES)
def test_solve_with_the_direct_block_solve(name, direction, tol, tol_rel):
    c = H.case(name, direction)
    x_or, it_or, restarts = oracle_solve(name, direction, tol, tol_rel)
    assert restarts == 0, "condition of this test: the oracle's solve does not restart"
    sim = cu.SimulationData(diffusionBlockSolver=1, **c.sim_kw)
    x, r = _solve(c, sim, direction, tol, tol_rel)
    assert_solver_bound(c, direction, tol, tol_rel, x, r, x_or, it_or, f"{c.name}, direction {direction}, tol {tol:g} / {tol_rel:g}")


# ------------------------------------------------------------------ 5. step
@pytest.mark.parametrize("name", ["uniform_mixed", "l012"])
def test_step_is_its_three_stand_alone_direct_solves(name):
    """the pattern of tests/test_gpu_implicit_step.py::test_step_is_its_three_stand_alone_solves with the sim in mode 1"""
    c = H.case(name)
    sim = cu.SimulationData(nu=c.nu, uinf=c.uinf, diffusionBlockSolver=1, **c.sim_kw)
    assert np.array_equal(sim.grid.tables[:, :5], c.oracle.tables[:, :5])
    first, results0 = device_step(c, sim, params(0.0, 0.0, max_iter=0))
    assert_step_without_iterations(c, first, results0)     # tmpV and the guess are exact: what follows builds on them
    tight = params(1e-12, 1e-11)
    got, results = device_step(c, sim, tight)
    assert bits(got["tmpV"], first["tmpV"]) and bits(got["pres"], c.pres)
    change = np.abs(got["vel"] - c.vel).max()
    for comp in range(3):
        sim.upload("lhs", c.h3 * first["tmpV"][..., comp])
        sim.fill("pres", 0.0)
        alone = PoissonResult()
        check(lib().cup3d_diffusion_solve(sim.handle, comp, c.dt, c.nu, C.byref(tight), C.byref(alone)))
        x = sim.download("pres")
        want = restated_without_iterations(c)["guess"][..., comp] + x
        assert alone.iterations > 0 and np.abs(x).max() > 0
        for f in FIELDS:
            assert getattr(results[comp], f) == getattr(alone, f), (name, comp, f, getattr(results[comp], f), getattr(alone, f))
        assert bits(np.ascontiguousarray(got["vel"][..., comp]), want), \
            f"{name}: component {comp}: the step is not guess + the stand-alone solution, max |d| {np.abs(got['vel'][..., comp] - want).max():.3e} ({change:.3e} velocity change)"
    # the step did run the direct solve: in mode 0 the same sim gives other bits
    check(lib().cup3d_diffusion_set_block_solver(sim.handle, 0))
    cg, _ = device_step(c, sim, tight)
    assert not bits(cg["vel"], got["vel"])
    print(f"{name}: iterations per component, direct {[r.iterations for r in results]}; max |vel(direct) - vel(block CG)| = {np.abs(cg['vel'] - got['vel']).max():.3e} "
          f"of a velocity change of {change:.3e}")


# ------------------------------------------------------------------ 6. over ranks
def test_block_solve_and_solve_over_two_ranks():
    """`l012` over two thread ranks (rank views of contiguous ranges): the kernel runs over each rank's owned blocks only, with their h"""
    from test_gpu_multirank import VirtualComm, run_ranks
    c, nranks, direction, (tol, tol_rel) = H.case("l012"), 2, 1, TOLS[1]
    o, kw = c.oracle, c.sim_kw
    one = cu.SimulationData(diffusionBlockSolver=1, **kw)
    z_one = helm_precond(one, c.rhs, c.dt, c.nu)
    assert_exact(z_one, c.rhs, c.h, c.centre, "l012 on one rank")
    with VirtualComm(nranks):
        mesh = cu.operators.Grid((kw["bpdx"], kw["bpdy"], kw["bpdz"]), kw["levelMax"], 0, kw["extent"], (kw["BC_x"], kw["BC_y"], kw["BC_z"]), leaves=kw["leaves"])
        assert np.array_equal(mesh.tables, o.tables)
        owner = (np.arange(o.nb) * nranks // o.nb).astype(np.int32)
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(**{**kw, "leaves": None}, view=v, diffusionBlockSolver=1) for v in views]
        mine = [v.global_slot[:v.nlocal] for v in views]
        assert sum(s.nblocks for s in sims) == o.nb and all(s.nblocks for s in sims) and sum(v.nghost for v in views) > 0
        z, x, res = np.zeros_like(c.rhs), np.zeros_like(c.rhs), [None] * nranks

        def rank(r):
            s = sims[r]
            z[mine[r]] = helm_precond(s, c.rhs[mine[r]], c.dt, c.nu)
            s.upload("lhs", c.rhs[mine[r]])
            s.upload("pres", c.x0[mine[r]])
            p, res[r] = params(tol, tol_rel), PoissonResult()
            check(lib().cup3d_diffusion_solve(s.handle, direction, c.dt, c.nu, C.byref(p), C.byref(res[r])))
            x[mine[r]] = s.download("pres")

        run_ranks(rank, nranks)
        del sims, views
    assert bits(z, z_one), f"the block solve over ranks differs from one rank on blocks {np.where((z != z_one).reshape(o.nb, -1).any(axis=1))[0]}"
    for f in FIELDS:
        assert getattr(res[0], f) == getattr(res[1], f), f
    x_or, it_or, restarts = oracle_solve("l012", direction, tol, tol_rel)
    assert restarts == 0
    assert_solver_bound(c, direction, tol, tol_rel, x, res[0], x_or, it_or, f"l012 over {nranks} ranks, direction {direction}")


# ------------------------------------------------------------------ 7. interface
@pytest.mark.parametrize("mode", [2, -1])
def test_other_modes_are_refused(mode):
    c = H.case("mixed16", 0)
    sim = cu.SimulationData(**c.sim_kw)
    assert lib().cup3d_diffusion_set_block_solver(sim.handle, mode) == -1   # CUP3D_EINVAL
    text = lib().cup3d_last_error().decode()
    assert "cup3d_diffusion_set_block_solver" in text and str(mode) in text, text
    assert lib().cup3d_diffusion_set_block_solver(None, 1) == -1
    with pytest.raises(cu.capi.Cup3dError):
        cu.SimulationData(diffusionBlockSolver=mode, **c.sim_kw)
    # the refused call changed nothing: still the block CG
    assert bits(helm_precond(sim, c.rhs, c.dt, c.nu), helm_precond(cu.SimulationData(**c.sim_kw), c.rhs, c.dt, c.nu))


def test_adapted_keeps_the_mode():
    """SimulationData(diffusionBlockSolver=1).adapted(states) is in mode 1: the exactness bound on the adapted mesh, which a block CG result
    misses by seven orders"""
    c = H.case("l012")
    sim = cu.SimulationData(diffusionBlockSolver=1, **c.sim_kw)
    tags = np.zeros(c.oracle.nb, dtype=np.int8)
    tags[int(np.argmax(c.h))] = 1                           # refine one of the coarsest blocks
    st = c.oracle.valid_states(tags)
    assert (st == 1).any()
    new = sim.adapted(st)
    assert new.diffusionBlockSolver == 1 and new.nblocks > sim.nblocks
    h = new.grid.geom[:, 0].copy()
    rhs = np.random.default_rng(11).uniform(-1, 1, (new.nblocks, 8, 8, 8)) * h.reshape(-1, 1, 1, 1)
    dt = h.max() ** 2 / NU
    assert_exact(helm_precond(new, rhs, dt, NU), rhs, h, -6.0 - h * h / NU / dt, "adapted l012, shift 1")
