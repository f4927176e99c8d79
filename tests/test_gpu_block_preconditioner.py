"""The block preconditioner M^-1 on the device (cup3d_preconditioner, cup3d_diffusion_preconditioner) against the EXACT 8^3 block solve of
tests/block_solve_exact.py, block by block.  Runs on an MI355X only (-m gpu).

test_gpu_parity.py / test_gpu_amr.py compare M^-1 with the reference's own block CG at max|dz| <= 2e-5 max|z|; that cannot tell an exact
solver from one that is wrong in the seventh digit, nor a CG that obeys the reference's stopping rule from one that stops an iteration
early.  Asserted here, per block:
  block_solver 1 (fast diagonalisation)  max|z - z_exact| <= 5e-14 max|z_exact|; the assembled h^-1 A^-1 is symmetric to that bound
  block CG (0, 2, 3, 4; Helmholtz 0, 2)  ||A z - r/h|| <= 1.0001 max(1e-7 ||r/h||, 512e-16)  and  ||z - z_exact|| <= ||A^-1|| times that
                                         (block_solve_exact.cg_bounds: the stopping rule itself, no fitted tolerance)
  every solver                           blocks with ||r/h||^2/512^2 < 1e-32 come back as exact zeros; nothing is NaN
  iteration counts (0, 2)                within +-1 of the reference's block CG (oracle) on every block
  scale covariance                       z(2^k r) == 2^k z(r) bit for bit where only IEEE operations run (1, 2), the bounds at every scale
                                         where the division is v_rcp_f64 + Newton (0, 4) or for 3
and fast_div, the production CG's division, within 1 ulp of the correctly rounded quotient over the domain the CG reaches.
Grids: (a) the Green's function -- 512 blocks, block b holds a unit impulse at cell b; (b) the edge catalogue on 3 x 5 x 7 blocks (odd,
not a multiple of 8: the pair kernel's tail and the empty workgroups of block_slot); (c) two multi-level meshes (h differs per block).
"""
import numpy as np
import pytest

import block_solve_exact as X
import cup3d_amd as cu
import oracle_lib as O
from cup3d_amd.capi import check, lib

pytestmark = pytest.mark.gpu

EXT = 2 * np.pi
BCN = {0: "freespace", 1: "periodic", 2: "wall"}
GRIDS = ["green", "edge", "amr_mixed_l12", "random_3_levels"]
FDM_TOL = 5e-14


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)
    yield
    _CASES.clear()


def _need_testing_build(block_solver):
    if block_solver in (3, 4) and not hasattr(lib(), "cup3d_debug_set_option"):
        pytest.skip("A/B variant of the block CG: testing build only (this process runs the release library)")


def _mesh_sim(bpd, lmax, bc, lv, zs):
    return cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1],
                             BC_z=bc[2], leaves=(lv, zs))


_CASES = {}


def case(name, golden_dir):
    """(sim, rhs [nb, 8, 8, 8], h per block, kind per block) of one grid; built once per module."""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng({"green": 1, "edge": 2, "amr_mixed_l12": 3, "random_3_levels": 4}[name])
    if name == "green":
        sim = cu.SimulationData(bpdx=1, bpdy=1, bpdz=1, levelMax=4, levelStart=3, extent=EXT)
        assert sim.nblocks == 512
        rhs, kinds = np.eye(512).reshape(512, 8, 8, 8), np.array(["impulse"] * 512)
    else:
        if name == "edge":
            sim = cu.SimulationData(bpdx=3, bpdy=5, bpdz=7, levelMax=1, levelStart=0, extent=EXT, BC_x="wall", BC_y="periodic", BC_z="freespace")
            assert sim.nblocks == 105
        elif name == "amr_mixed_l12":
            g = np.load(f"{golden_dir}/{name}.npz")
            t = g["tables"]
            sim = _mesh_sim(tuple(int(b) for b in g["bpd"]), int(g["level_max"]), tuple(BCN[int(b)] for b in g["bc"]), t[:, 0].copy(), t[:, 1].copy())
        else:
            bc = tuple(str(b) for b in rng.choice(["periodic", "wall", "freespace"], 3))
            top = [int(v) for v in rng.integers(0, 2, 3)]
            refine = [(0, *top), (1, *(2 * t + int(v) for t, v in zip(top, rng.integers(0, 2, 3))))]   # a level-0 block, then one of its children
            lv, zs = O.build_balanced_mesh((2, 2, 2), 3, bc, refine)
            sim = _mesh_sim((2, 2, 2), 3, bc, lv, zs)
            assert set(sim.grid.tables[:, 0].tolist()) == {0, 1, 2}
        kinds, unit = X.edge_grid(rng, sim.nblocks, 1.0)
        rhs = unit * sim.grid.geom[:, 0].reshape(-1, 1, 1, 1)   # the catalogue's thresholds are per unit h
    h = sim.grid.geom[:, 0].copy()
    _CASES[name] = (sim, np.ascontiguousarray(rhs), h, kinds)
    return _CASES[name]


def precond(sim, rhs, block_solver, helmholtz=None, iterations=False):
    """M^-1 rhs on the device (in place on pres).  helmholtz = (dt, nu): the diffusion solver's block CG, evaluated as `block_solver` selects
    (0: production, 2: the reference's association) -- the sim takes that selection from the last cup3d_preconditioner call.
    iterations: also the per-block CG iteration counts (recorded while profiling is on)."""
    sim.upload("pres", rhs)
    if iterations:
        check(lib().cup3d_profile_enable(1))
    try:
        check(lib().cup3d_preconditioner(sim.handle, block_solver))
    finally:
        if iterations:
            check(lib().cup3d_profile_enable(0))
    if helmholtz is not None:
        sim.upload("pres", rhs)
        check(lib().cup3d_diffusion_preconditioner(sim.handle, helmholtz[0], helmholtz[1]))
    z = sim.download("pres")
    if not iterations:
        return z
    its = np.zeros(sim.nblocks, dtype=np.int32)
    check(lib().cup3d_debug_block_cg_iterations(sim.handle, its))
    return z, its


def assert_block_cg(z, rhs, h, centre, what):
    """The stopping rule's bounds per block (module docstring); returns the worst residual / ||r/h|| of the blocks the relative criterion
    ends."""
    assert np.isfinite(z).all(), what
    sk = X.skipped(rhs, h)
    assert (z[sk] == 0).all(), f"{what}: a block below the 1e-32 threshold is not exactly 0"
    rb, eb, bn = X.cg_bounds(rhs, h, centre)
    rn, _ = X.block_residual(z, rhs, h, centre)
    err = np.linalg.norm((z - X.exact_block_solve(rhs, h, centre)).reshape(len(z), -1), axis=1)
    s = ~sk
    relative = s & (X.BLOCK_REL * bn > 512 * X.BLOCK_ABS)   # blocks the relative criterion ends
    rel = (rn[relative] / bn[relative]).max() if relative.any() else 0.0
    print(f"{what}: residual / bound max {(rn / rb)[s].max():.4f}, error / bound max {(err / eb)[s].max():.4f}, "
          f"residual / ||r/h|| max {rel:.3e} ({s.sum()} solved blocks, {relative.sum()} of them ended by the relative criterion, {sk.sum()} skipped)")
    bad = np.where(s & (rn > rb))[0]
    assert not len(bad), f"{what}: residual above the stopping rule's bound on blocks {bad[:8]}: ratio {(rn / rb)[bad].max():.6f}"
    bad = np.where(s & (err > eb))[0]
    assert not len(bad), f"{what}: error above ||A^-1|| x residual bound on blocks {bad[:8]}: ratio {(err / eb)[bad].max():.4f}"
    return rel


@pytest.mark.parametrize("grid", GRIDS)
def test_direct_block_solve_is_exact(golden_dir, grid):
    """block_solver 1 (fdm_block: sine transforms with cQ, scaling by invD) is the exact solve to rounding: 5e-14 of the block's max|z|."""
    sim, rhs, h, kinds = case(grid, golden_dir)
    z = precond(sim, rhs, 1)
    assert np.isfinite(z).all()
    sk = X.skipped(rhs, h)
    assert (z[sk] == 0).all()
    zx = X.exact_block_solve(rhs, h)
    n = len(z)
    d = np.abs(z - zx).reshape(n, -1).max(axis=1)
    m = np.abs(zx).reshape(n, -1).max(axis=1)
    ratio = (d / np.where(sk, 1.0, m))[~sk]
    print(f"{grid}: block_solver 1: max|z - z_exact| / max|z_exact| worst {ratio.max():.3e}, median {np.median(ratio):.3e}")
    bad = np.where(~sk & (d > FDM_TOL * m))[0]
    assert not len(bad), f"blocks {bad[:8]} ({kinds[bad[:8]]}): worst {ratio.max():.3e} > {FDM_TOL}"
    if grid == "green":
        G = z.reshape(512, 512)   # row b = h^-1 A^-1 e_b
        asym = np.abs(G - G.T).max() / np.abs(G).max()
        print(f"green: |G - G^T| / max|G| = {asym:.3e}")
        assert asym <= FDM_TOL


@pytest.mark.parametrize("block_solver", [0, 2, 3, 4])
@pytest.mark.parametrize("grid", GRIDS)
def test_block_cg_meets_the_stopping_rule(golden_dir, grid, block_solver):
    _need_testing_build(block_solver)
    sim, rhs, h, _ = case(grid, golden_dir)
    assert_block_cg(precond(sim, rhs, block_solver), rhs, h, -6.0, f"{grid}: block_solver {block_solver}")


@pytest.mark.parametrize("shift", [0.01, 1.0, 100.0])
@pytest.mark.parametrize("block_solver", [0, 2])
@pytest.mark.parametrize("grid", GRIDS)
def test_helmholtz_block_cg_meets_the_stopping_rule(golden_dir, grid, block_solver, shift):
    """The diffusion solver's block CG (centre -6 - h^2/(nu dt)) with h^2/(nu dt) = shift on the grid's coarsest blocks (4x, 16x smaller
    on the finer levels of the meshes)."""
    sim, rhs, h, _ = case(grid, golden_dir)
    nu = 0.5
    dt = h.max() ** 2 / nu / shift
    centre = -6.0 - h * h / nu / dt          # as the kernel evaluates it
    z = precond(sim, rhs, block_solver, helmholtz=(dt, nu))
    assert_block_cg(z, rhs, h, centre, f"{grid}: Helmholtz, block_solver {block_solver}, shift {shift}")
    # the reference's block CG on the same blocks: the 2e-5 comparison of test_implicit_diffusion_solver, and the same bounds
    zo, _ = O.precond_blocks(rhs, h, centre)
    assert np.abs(z - zo).max() <= 2e-5 * np.abs(zo).max()


@pytest.mark.parametrize("block_solver", [0, 2])
@pytest.mark.parametrize("grid", GRIDS)
def test_block_cg_iterations_match_the_reference(golden_dir, grid, block_solver):
    """Per block, the device's CG runs as many iterations as the reference's block CG, +-1 (a block whose residual grazes the criterion
    may go either way under another summation order): catches a CG that stops short of the rule as well as one that runs past it."""
    sim, rhs, h, kinds = case(grid, golden_dir)
    z, its = precond(sim, rhs, block_solver, iterations=True)
    zo, ref = O.precond_blocks(rhs, h)
    eq = float((its == ref).mean())
    print(f"{grid}: block_solver {block_solver}: iteration counts equal to the reference's on {100 * eq:.1f} % of {len(its)} blocks "
          f"(device {its.sum()}, reference {ref.sum()}; max |d| {np.abs(its - ref).max()})")
    bad = np.where(np.abs(its - ref) > 1)[0]
    assert not len(bad), f"blocks {bad[:8]} ({kinds[bad[:8]]}): device {its[bad[:8]]}, reference {ref[bad[:8]]}"
    assert np.abs(z - zo).max() <= 2e-5 * np.abs(zo).max()


@pytest.mark.parametrize("block_solver", [1, 2, 0, 3, 4])
def test_scale_covariance(golden_dir, block_solver):
    """z(2^k r) for k in {-8, 8, 40}: exactly 2^k z(r) where the block solve is IEEE operations only (1: transforms, 2: the reference's
    association with IEEE divisions) -- on blocks clear of the 1e-32 thresholds and of the 1e-55 guards; the stopping rule's bounds at every
    scale for 0, 3 and 4."""
    _need_testing_build(block_solver)
    sim, _, h, _ = case("edge", golden_dir)
    rng = np.random.default_rng(9)
    blocks = []
    while len(blocks) < sim.nblocks:
        blocks += [b for _, b in X.edge_blocks(rng, kinds=("random", "constant", "spike", "lowest_mode"))]
    rhs = np.ascontiguousarray(blocks[:sim.nblocks])
    assert not X.skipped(rhs * 2.0 ** -8, h).any()
    base = precond(sim, rhs, block_solver)
    for k in (-8, 8, 40):
        s = 2.0 ** k
        z = precond(sim, rhs * s, block_solver)
        if block_solver in (1, 2):
            diff = np.where(z != base * s)
            assert not len(diff[0]), f"k = {k}: {len(diff[0])} cells differ, first block {diff[0][0]}"
        else:
            assert_block_cg(z, rhs * s, h, -6.0, f"block_solver {block_solver}, scale 2^{k}")


def _ulps_apart(a, b):
    """|a - b| in units in the last place (positive finite doubles: their bit patterns are ordered like the values)."""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_fast_div_within_one_ulp():
    """fast_div (v_rcp_f64, two Newton steps, one residual correction: the division of the production block CG, poisson.hip) against the
    correctly rounded IEEE quotient: within 1 ulp over d in [1e-55, 1e300], n in {0} and [1e-60, 1e300], normal quotients -- random,
    powers of two and exact quotients, the last returned exactly."""
    rng = np.random.default_rng(13)
    N = 1 << 20
    n = 10.0 ** rng.uniform(-60, 300, N)
    d = 10.0 ** rng.uniform(-55, 300, N)
    n[:4096] = 0.0
    d[4096:4200] = 1e-55                                 # the guard of rr / (a2 + 1e-55) alone
    # powers of two
    pn = np.ldexp(1.0, rng.integers(-199, 997, 8192))
    pd = np.ldexp(1.0, rng.integers(-182, 996, 8192))
    # exact quotients: d with a 32-bit significand times an integer below 2^20
    ed = np.ldexp(rng.integers(1 << 31, 1 << 32, 8192).astype(np.float64), rng.integers(-213, 965, 8192))
    en = ed * rng.integers(1, 1 << 20, 8192).astype(np.float64)
    n, d = np.concatenate([n, pn, en]), np.concatenate([d, pd, ed])
    exact = np.arange(len(n)) >= N                       # powers of two and exact quotients
    with np.errstate(over="ignore", under="ignore"):
        q = n / d
    fin = np.finfo(np.float64)
    keep = (n == 0) | ((q >= fin.tiny) & (q <= fin.max))
    keep &= (d >= 1e-55) & (d <= 1e300) & ((n == 0) | ((n >= 1e-60) & (n <= 1e300)))
    n, d, q, exact = np.ascontiguousarray(n[keep]), np.ascontiguousarray(d[keep]), q[keep], exact[keep]
    assert len(n) > N // 2
    out = np.empty_like(n)
    check(lib().cup3d_debug_cg_div(n, d, len(n), out))
    assert (out[n == 0] == 0).all()
    u = _ulps_apart(out, q)
    print(f"fast_div: {len(n)} quotients, correctly rounded {100 * float((u == 0).mean()):.4f} %, max {u.max()} ulp; "
          f"exact quotients returned exactly: {100 * float((u[exact] == 0).mean()):.2f} %")
    bad = np.where(u > 1)[0]
    assert not len(bad), f"n = {n[bad[:4]]}, d = {d[bad[:4]]}: {u[bad[:4]]} ulp"
    # a representable quotient comes back exactly: the residual correction q + y (n - d q) makes it so (n - d q is exact in the FMA)
    bad = np.where(exact & (u != 0))[0]
    assert not len(bad), f"exact quotients not returned exactly: n = {n[bad[:4]]}, d = {d[bad[:4]]}"
