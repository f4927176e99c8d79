"""The pointwise passes of cup3d_advect_diffuse_implicit (k_imp_guess, k_imp_rhs, k_imp_load, k_imp_add, k_imp_copy of csrc/diffusion.hip
<- AdvectionDiffusionImplicit::euler, main.cpp:10030-10118) bit for bit against tests/implicit_step_restatement.py, which
tests/test_helmholtz_restatement.py pins to the oracle's advdiff_implicit.  MI355X only (-m gpu).

  max_iter = 0   every solve returns its zero guess, so no dot product touches a vector: vel is the restated guess + 0.0, tmpV the restated
                 right-hand side and pres what was uploaded, BIT FOR BIT -- on the uniform grids `mixed16` and `uniform_mixed`, on the
                 three-level mesh `l012` (per-block h) and on 1280 blocks, where every grid-stride loop of the passes (2048 x 256 threads:
                 the vector passes from 342 blocks, the scalar ones from 1025) takes its second trip.
  chained        the step at 1e-12 / 1e-11, then per component the stand-alone cup3d_diffusion_solve of h^3 tmpV_c from a zero guess with the
                 same parameters: vel_c of the step is guess_c + pres_c bit for bit and results[c] is the stand-alone result field by
                 field.  tests/test_gpu_helmholtz_iteration.py pins every iteration of the stand-alone solve, so the whole operator is
                 pinned.

The comparisons at solver tolerance of tests/test_gpu_amr.py stay as they are; tests/test_helmholtz_restatement.py lists the wrong steps
those cannot see and these cannot miss."""
import ctypes as C

import numpy as np
import pytest

import cup3d_amd as cu
import helmholtz_cases as H
import implicit_step_restatement as S
from cup3d_amd.capi import PoissonParams, PoissonResult, check, lib
from test_gpu_bicgstab_iteration import bits

pytestmark = pytest.mark.gpu
FIELDS = ("iterations", "restarts", "norm0", "norm", "used_xopt")


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def params(tol, tol_rel, max_iter=None):
    p = PoissonParams()
    lib().cup3d_poisson_default_params(C.byref(p))
    p.tol, p.tol_rel = tol, tol_rel
    if max_iter is not None:
        p.max_iter = max_iter
    return p


def make_sim(c):
    sim = cu.SimulationData(nu=c.nu, uinf=c.uinf, **c.sim_kw)
    assert np.array_equal(sim.grid.tables[:, :5], c.oracle.tables[:, :5])
    return sim


def device_step(c, sim, p):
    sim.upload("vel", c.vel)
    sim.upload("pres", c.pres)
    res = (PoissonResult * 3)()
    check(lib().cup3d_advect_diffuse_implicit(sim.handle, c.dt, c.nu, np.array(c.uinf, dtype=np.float64), C.byref(p), res))
    return dict(vel=sim.download("vel"), tmpV=sim.download("tmpV"), pres=sim.download("pres")), [res[i] for i in range(3)]


_RESTATED = {}


def restated_without_iterations(c):
    """the step whose every solve returns its guess (computed once per case, read-only)"""
    if c.name not in _RESTATED:
        r = S.euler(c.vel, c.pres, c.h, c.dt, c.nu, c.advect(False), c.diffusion_rhs, lambda rhs, x0, direction: x0.copy())
        for a in (r["vel"], r["tmpV"], r["pres"], r["guess"]):
            a.setflags(write=False)
        _RESTATED[c.name] = r
    return _RESTATED[c.name]


def assert_step_without_iterations(c, got, results):
    want = restated_without_iterations(c)
    assert bits(want["vel"], want["guess"] + 0.0)
    for k in ("tmpV", "vel", "pres"):
        if not bits(got[k], want[k]):
            d = np.abs(got[k] - want[k]).reshape(len(got[k]), -1).max(axis=1)
            raise AssertionError(f"{c.name}: {k} differs from the restated step on {int((d > 0).sum())} of {len(d)} blocks (first {int(np.argmax(d > 0))}), "
                                 f"max {d.max():.3e} = {d.max() / np.abs(want[k]).max():.1e} of max|{k}|")
    assert all(r.iterations == 0 and r.restarts == 0 for r in results)


@pytest.mark.parametrize("name", ["mixed16", "l012", "uniform_mixed"])
def test_step_without_iterations_is_the_restated_passes(name):
    c = H.case(name)
    got, results = device_step(c, make_sim(c), params(0.0, 0.0, max_iter=0))
    assert_step_without_iterations(c, got, results)


def test_step_without_iterations_on_1280_blocks():
    """(5,4,1) level 2, wall / periodic / freespace: the second trip of every grid-stride loop"""
    c = H.case("grid1280")
    assert c.oracle.nb == 1280 and 3 * 512 * c.oracle.nb > 2048 * 256 and 512 * c.oracle.nb > 2048 * 256
    got, results = device_step(c, make_sim(c), params(0.0, 0.0, max_iter=0))
    assert_step_without_iterations(c, got, results)


@pytest.mark.parametrize("name", ["l012", "mixed16"])
def test_step_is_its_three_stand_alone_solves(name):
    c = H.case(name)
    sim = make_sim(c)
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
        assert alone.iterations > 3 and np.abs(x).max() > 0
        for f in FIELDS:
            assert getattr(results[comp], f) == getattr(alone, f), (name, comp, f, getattr(results[comp], f), getattr(alone, f))
        assert bits(np.ascontiguousarray(got["vel"][..., comp]), want), \
            f"{name}: component {comp}: the step is not guess + the stand-alone solution, max |d| {np.abs(got['vel'][..., comp] - want).max():.3e} ({change:.3e} velocity change)"
