"""ONE application of the multigrid V-cycle on the device (cup3d_preconditioner(sim, 5), in place on pres) against the dense NumPy restatement
of tests/multigrid_restatement.py evaluated in longdouble, cell by cell.  Runs on an MI355X only (-m gpu).

The solver tests compare converged pressures and iteration counts; BiCGSTAB converges with any reasonable preconditioner, so they cannot tell
this cycle from one with an averaged restriction, a swapped octant, unfrozen ghosts or a wrong coarse h.  Here the cycle is pinned as an
OPERATOR.  Tolerance (multigrid_cases.tolerance), both terms from the restatement and none from the device:
    max|z_dev - z_ld| <= 32 max(max|z_f64 - z_ld|, 4 eps max|z_ld|)
32 covers what legitimately differs: the order of the 256-thread sum of the coarsest level's mean, over ranks the all-reduce (the kernels
are built without FMA contraction, and the restatement keeps their association, the eight-child sum ((a+b)+(c+d))+((e+f)+(g+h)) included).
Every structural error moves the result by more than 1e6 x this bound (tests/test_multigrid_restatement.py, the mutation catalogue).
The ratio printed and recorded per case is max|z_dev - z_ld| / max(max|z_f64 - z_ld|, 4 eps max|z_ld|): it must stay <= 32.
"""
from contextlib import contextmanager

import numpy as np
import pytest

import cup3d_amd as cu
import multigrid_cases as K
import multigrid_restatement as R
import oracle_lib as O
from cup3d_amd.capi import check, lib

pytestmark = pytest.mark.gpu

_SIMS = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)
    yield
    _SIMS.clear()


@contextmanager
def options(**kw):
    """debug options for the duration of the block; every one is back at its default afterwards, whatever happens inside"""
    try:
        for k, v in kw.items():
            check(lib().cup3d_debug_set_option(k.encode(), int(v)))
        yield
    finally:
        for k in kw:
            check(lib().cup3d_debug_set_option(k.encode(), 0))


def uniform_sim(case):
    """(sim, oracle grid) of a uniform case, built once per module; the dense <-> block layout is the oracle's"""
    if case not in _SIMS:
        bpd, level, bc = K.UNIFORM[case]
        sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=level + 1, levelStart=level, extent=K.EXT, BC_x=bc[0], BC_y=bc[1],
                                BC_z=bc[2], blockSolver=5)
        o = O.OracleGrid(bpd, level + 1, level, K.EXT, bc)
        assert np.array_equal(sim.grid.index, o.index) and sim.grid.h == o.h
        _SIMS[case] = (sim, o)
    return _SIMS[case]


def mesh_sim(name):
    """(sim, restatement Mesh) of a multi-level case; the block order is the oracle's"""
    if name not in _SIMS:
        bpd, lmax, bc, lv, zs = K.mesh_case(name)
        m, M = K.oracle_mesh(name)
        sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=K.EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2],
                                leaves=(lv, zs), blockSolver=5)
        assert np.array_equal(sim.grid.tables, m.tables)
        _SIMS[name] = (sim, M)
    return _SIMS[name]


def apply_blocks(sim, blocks):
    """M^-1 of leaf blocks: one application through the public entry point, in place on pres"""
    sim.upload("pres", np.ascontiguousarray(blocks))
    check(lib().cup3d_preconditioner(sim.handle, 5))
    return sim.download("pres")


def apply_uniform(case, r):
    sim, o = uniform_sim(case)
    return o.to_global(apply_blocks(sim, o.to_blocks(r)))


def assert_cycle(what, z, z64, zld):
    assert np.isfinite(z).all(), what
    unit = K.tolerance(z64, zld) / K.MARGIN
    err = float(np.abs(z - zld).max())
    print(f"{what}: max|z_dev - z_ld| = {err:.3e} = {err / unit:.2f} x max(|z_f64 - z_ld|, 4 eps |z_ld|) (bound {K.MARGIN}); "
          f"equal to the float64 restatement in {100 * float((z == z64).mean()):.1f} % of the cells")
    assert err <= K.MARGIN * unit, f"{what}: {err / unit:.3g} x the unit, bound {K.MARGIN}"
    return err / unit


@pytest.mark.parametrize("kind", K.INPUTS)
@pytest.mark.parametrize("case", list(K.UNIFORM))
def test_uniform_cycle(case, kind):
    """Default V(2,2), production (wavefront) smoother, six uniform grids x three inputs.  Observed ratio on an MI355X (bound 32): one block
    0.16 - 1.00, 8 blocks on one level 0.61 - 1.00, two levels 0.23 - 1.00, three levels 0.40 - 1.00 and 3.45 for the constant field (the order
    of the mean's sum), box (3,2,1) 0.27 - 1.00; most cases equal the float64 restatement in every cell.  Before mg_vcycle staged an in-place
    input, every case except the two one-block ones failed here, by 1e15 ... 3e18 x the unit."""
    r, (z64, zld) = K.restated_uniform(case, kind)
    assert_cycle(f"{case}, {kind}", apply_uniform(case, r), z64, zld)


@pytest.mark.parametrize("launches,sweeps", K.SCHEDULES)
@pytest.mark.parametrize("case", K.SCHEDULE_CASES)
def test_uniform_cycle_other_schedules(case, launches, sweeps):
    """(mg_launches, mg_sweeps) = (1, 3) and (3, 1): the launch / sweep loops and the buffer alternation at odd counts.  Observed ratio 0.81 - 1.00.
    ((1, 3) is the one multi-block schedule that was right in place before the staging: its single launch per leg never reads the input after
    the output has been written.)"""
    r, (z64, zld) = K.restated_uniform(case, "random", launches, sweeps)
    with options(mg_launches=launches, mg_sweeps=sweeps):
        z = apply_uniform(case, r)
    assert_cycle(f"{case}, {launches} x {sweeps}", z, z64, zld)


@pytest.mark.parametrize("kind", K.INPUTS)
def test_uniform_cycle_workgroup_smoother(kind):
    """The LDS-tile form of the smoother (mg_smooth_workgroup) against the restatement, not only against the wavefront form.  Observed ratio
    1.00, 3.45, 0.40: the wavefront form's figures, bit for bit."""
    r, (z64, zld) = K.restated_uniform("three_levels_211", kind)
    with options(mg_smooth_workgroup=1):
        z = apply_uniform("three_levels_211", r)
    assert_cycle(f"three_levels_211, {kind}, workgroup smoother", z, z64, zld)


@pytest.mark.parametrize("launches,sweeps", [(2, 2), (1, 3)])
@pytest.mark.parametrize("name", K.MESHES)
def test_multilevel_cycle(name, launches, sweeps):
    """Three-level meshes on one rank: leaves and ancestors per level, zero coarse/fine ghosts on the way down, the containing coarse cell on
    the way up, the result on the leaves.  Observed ratio 0.83 - 1.00 on the three meshes and both schedules."""
    sim, M = mesh_sim(name)
    r = K.mesh_input(sim.nblocks)
    z64, zld = K.restated((name, launches, sweeps), lambda dt: R.vcycle_blocks(M, r, dtype=dt, launches=launches, sweeps=sweeps))
    with options(mg_launches=launches, mg_sweeps=sweeps):
        z = apply_blocks(sim, r)
    assert_cycle(f"{name}, {launches} x {sweeps}", z, z64, zld)


@pytest.mark.parametrize("case", ["three_levels_211", "l012_wall"])
def test_cycle_is_a_fixed_linear_operator_on_the_device(case):
    """What BiCGSTAB needs of M^-1: z(2^k r) == 2^k z(r) bit for bit (k = -3, 5), two applications of one input give the same bits, and
    z(r1 + r2) = z(r1) + z(r2) within the tolerance of the module docstring (taken for r1 + r2).  Observed: 7.1e-15 (three_levels_211) and 1.5e-14 (l012_wall)
    against a tolerance of 9.2e-13."""
    if case in K.UNIFORM:
        bpd, level, bc = K.UNIFORM[case]
        sim, o = uniform_sim(case)
        r1, r2 = o.to_blocks(K.uniform_input("random", bpd, level)), o.to_blocks(K.uniform_input("impulses", bpd, level))
        h = K.EXT / (8 * (max(bpd) << level))
        z64, zld = (np.stack([z[8 * k:8 * k + 8, 8 * j:8 * j + 8, 8 * i:8 * i + 8] for i, j, k in o.index])
                    for z in (R.vcycle_uniform(o.to_global(r1 + r2), bpd, level, bc, h, dtype=dt) for dt in (np.float64, np.longdouble)))
    else:
        sim, M = mesh_sim(case)
        r1, r2 = K.mesh_input(sim.nblocks), K.mesh_input(sim.nblocks, seed=41)
        z64, zld = (R.vcycle_blocks(M, r1 + r2, dtype=dt) for dt in (np.float64, np.longdouble))
    z1 = apply_blocks(sim, r1)
    assert np.array_equal(apply_blocks(sim, r1), z1), "two applications of one input differ"
    for k in (-3, 5):
        diff = np.where(apply_blocks(sim, r1 * 2.0 ** k) != z1 * 2.0 ** k)[0]
        assert not len(diff), f"k = {k}: {len(diff)} cells differ, first block {diff[0]}"
    z2, z12 = apply_blocks(sim, r2), apply_blocks(sim, r1 + r2)
    assert_cycle(f"{case}: z(r1 + r2)", z12, z64, zld)
    assert_cycle(f"{case}: z(r1) + z(r2)", z1 + z2, z64, zld)
    add = float(np.abs(z12 - (z1 + z2)).max())
    print(f"{case}: max|z(r1 + r2) - z(r1) - z(r2)| = {add:.3e}, tolerance {K.tolerance(z64, zld):.3e}")
    assert add <= K.tolerance(z64, zld)
