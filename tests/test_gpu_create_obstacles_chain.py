"""What cup3d_create_obstacles returns goes straight into the operators after it.  MI355X only (-m gpu).

CreateObstacles -> shape.data() / shape.surface() -> UpdateObstacles, Penalization, ComputeForces must give exactly what the same
operators give on the restatement's arrays (tests/characteristic_restatement.py) with its chi field uploaded; and
Simulation(sim, obstacle_operators=True) with sim.shapes must advance one step to the same fields as the chain called by hand."""
import numpy as np
import pytest

import characteristic_cases as CC
import cup3d_amd as cu

pytestmark = pytest.mark.gpu
DT, LAMBDA, NU = 0.01, 1e4, 0.01
MOTION = [((0.1, 0.2, -0.3), (0.05, -0.02, 0.03)), ((-0.2, 0.1, 0.15), (0.0, 0.04, -0.01))]


def fresh(c, **kw):
    sim = cu.SimulationData(nu=NU, **kw, **c.sim_kwargs)
    rng = np.random.default_rng(12)
    sim.upload("vel", rng.uniform(-1, 1, (c.nb, 8, 8, 8, 3)))
    sim.upload("pres", rng.uniform(-1, 1, (c.nb, 8, 8, 8)))
    sim.lambda_penal = LAMBDA
    return sim


def obstacle_step(sim):
    cu.UpdateObstacles(sim)(DT)
    cu.Penalization(sim)(DT)
    return cu.ComputeForces(sim)(DT)


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_results_feed_the_other_obstacle_operators(name):
    c = CC.case(name)
    sim = fresh(c)
    field, first, _, _ = CC.expected(name, sim.grid.geom)
    sim.shapes = [cu.ObstacleShape(o["ids"], o["sdf"], o["udef"], o["transvel_correction"]) for o in c.obstacles]
    cu.CreateObstacles(sim)(0.0)
    sim.obstacles = [s.data(v, w) for s, (v, w) in zip(sim.shapes, MOTION)]
    sim.surfaces = [s.surface(v, w) for s, (v, w) in zip(sim.shapes, MOTION)]
    for s, surf in zip(sim.shapes, sim.surfaces):
        assert 0 < len(surf.slots) <= len(s.slots) and (np.diff(surf.first) > 0).all()
    assert len(sim.surfaces[1].slots) < len(sim.shapes[1].slots)   # the blocks without points are left out
    got = obstacle_step(sim)
    # the same operators on the restatement's arrays
    ref = fresh(c)
    ref.upload("chi", field)
    ref.obstacles, ref.surfaces = [], []
    for o, r, (v, w) in zip(c.obstacles, first, MOTION):
        ref.obstacles.append(cu.ObstacleData(o["ids"], r.chi, r.udef, r.cm, v, w))
        keep = np.where(np.diff(r.first) > 0)[0]
        ref.surfaces.append(cu.ObstacleSurface(o["ids"][keep], np.concatenate([[0], np.cumsum(np.diff(r.first)[keep])]), r.ijk, r.dchi, r.udef[keep], r.cm, v, w))
    want = obstacle_step(ref)
    for a, b in zip(sim.obstacles, ref.obstacles):
        for f in ("totals", "block_sums", "vel", "omega", "force", "torque"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for (p, q), (rp, rq) in zip(got, want):
        assert np.array_equal(p, rp) and np.array_equal(q, rq) and p.shape[1] > 0
    assert np.array_equal(sim.download("vel"), ref.download("vel"))


def test_simulation_with_shapes_equals_the_chain_by_hand():
    c = CC.case("uniform8")
    kw = dict(uMax_forced=1.0, poissonTol=1e-12, poissonTolRel=1e-10)
    sims = [fresh(c, **kw), fresh(c, **kw)]
    for sim in sims:
        sim.shapes = [cu.ObstacleShape(o["ids"], o["sdf"], o["udef"], o["transvel_correction"]) for o in c.obstacles]
        sim.step = 4
    S = cu.Simulation(sims[0], obstacle_operators=True)
    assert [type(op).__name__ for op in S.pipeline] == ["CreateObstacles", "AdvectionDiffusion", "ExternalForcing", "UpdateObstacles", "Penalization",
                                                        "PressureProjection"]
    S.advance(DT)
    s = sims[1]
    cu.CreateObstacles(s)(DT)
    assert len(s.obstacles) == 2 and np.array_equal(s.obstacles[1].chi, s.shapes[1].chi)
    for op in (cu.AdvectionDiffusion, cu.ExternalForcing, cu.UpdateObstacles, cu.Penalization, cu.PressureProjection):
        op(s)(DT)
    for f in ("vel", "pres", "chi"):
        assert np.array_equal(sims[0].download(f), s.download(f)), f
    for a, b in zip(sims[0].obstacles, s.obstacles):
        assert np.array_equal(a.vel, b.vel) and np.array_equal(a.force, b.force) and np.abs(a.force).max() > 0
    # without sim.shapes the pipeline is the one it was
    plain = fresh(c, **kw)
    assert [type(op).__name__ for op in cu.Simulation(plain, obstacle_operators=True).pipeline] == ["AdvectionDiffusion", "ExternalForcing", "PressureProjection"]
    plain.obstacles = s.obstacles
    assert [type(op).__name__ for op in cu.Simulation(plain, obstacle_operators=True).pipeline] == ["AdvectionDiffusion", "ExternalForcing", "UpdateObstacles",
                                                                                                    "Penalization", "PressureProjection"]
