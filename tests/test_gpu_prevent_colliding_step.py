"""The resident obstacle step with the collision model: Simulation(sim, obstacle_operators=True, collisions=True) puts
PreventCollidingObstacles directly in front of Penalization, as Penalization::operator() begins with preventCollidingObstacles
(main.cpp:14329).  uniform8 with the spheres A and B of tests/collision_cases.py in a flow that carries A into B.  MI355X only (-m gpu)."""
import numpy as np
import pytest

import collision_cases as K
import cup3d_amd as cu

pytestmark = pytest.mark.gpu
DT, LAMBDA, NU = 0.01, 1e4, 0.01
ORDER = ["CreateObstacles", "AdvectionDiffusion", "ExternalForcing", "UpdateObstacles", "PreventCollidingObstacles", "Penalization", "PressureProjection"]


def flow(c):
    """APPROACH's velocity of A within 1.5 of A's centre, B's elsewhere: UpdateObstacles finds the two bodies approaching"""
    vel = np.zeros((c.nb, 8, 8, 8, 3))
    i = np.arange(8) + 0.5
    for b in range(c.nb):
        h, o = c.geom[b, 0], c.geom[b, 1:4]
        z, y, x = np.meshgrid(o[2] + h * i, o[1] + h * i, o[0] + h * i, indexing="ij")
        near_a = (x - 3.3) ** 2 + (y - 3.0) ** 2 + (z - 3.2) ** 2 < 1.5 ** 2
        for d in range(3):
            vel[b, ..., d] = np.where(near_a, K.APPROACH["A"]["vel"][d], K.APPROACH["B"]["vel"][d])
    return vel


def fresh(c):
    sim = cu.SimulationData(nu=NU, uMax_forced=1.0, poissonTol=1e-12, poissonTolRel=1e-10, **c.sim_kwargs)
    sim.upload("vel", flow(c))
    sim.upload("pres", np.random.default_rng(12).uniform(-1, 1, (c.nb, 8, 8, 8)))
    sim.lambda_penal, sim.step = LAMBDA, 4
    obs = K.obstacles("uniform8")
    sim.shapes = [cu.ObstacleShape(obs[k]["ids"], obs[k]["sdf"], obs[k]["udef"], obs[k]["transvel_correction"]) for k in "AB"]
    return sim


def test_two_steps_with_the_collision_model():
    c = K.CC.case("uniform8")
    auto, hand, without = fresh(c), fresh(c), fresh(c)
    S = cu.Simulation(auto, obstacle_operators=True, collisions=True)
    assert [type(op).__name__ for op in S.pipeline] == ORDER
    plain = cu.Simulation(without, obstacle_operators=True)
    assert [type(op).__name__ for op in plain.pipeline] == [n for n in ORDER if n != "PreventCollidingObstacles"]   # today's pipeline
    assert [type(op).__name__ for op in cu.Simulation(without, obstacle_operators=True, collisions=False).pipeline] == [type(op).__name__ for op in plain.pipeline]
    # ---- step 1
    S.advance(DT)
    plain.advance(DT)
    ops = {n: getattr(cu, n)(hand) for n in ORDER}
    for n in ORDER[:4]:
        ops[n](DT)
    updated = [(o.vel.copy(), o.omega.copy()) for o in hand.obstacles]
    ops["PreventCollidingObstacles"](DT)
    assert hand.bCollision and hand.bCollisionID == [0, 1]
    for o, (v, w) in zip(hand.obstacles, updated):   # the pair was resolved: both bodies move differently now
        assert not np.array_equal(o.vel, v) and not np.array_equal(o.omega, w)
        assert np.array_equal(o.collision_vel, o.vel) and np.array_equal(o.collision_omega, o.omega) and o.collision_counter == 0.01 * DT
    ops["Penalization"](DT)
    ops["PressureProjection"](DT)
    for a, b, p, (v, w) in zip(auto.obstacles, hand.obstacles, without.obstacles, updated):
        for f in ("vel", "omega", "force", "torque", "collision_vel", "collision_omega"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.collision_counter == b.collision_counter == 0.01 * DT
        # without the operator the bodies keep what UpdateObstacles gave them, and are penalised towards that
        assert np.array_equal(p.vel, v) and np.array_equal(p.omega, w) and p.collision_counter == 0.0
        assert not np.array_equal(a.force, p.force) and np.abs(a.force).max() > 0
    for f in ("vel", "pres", "chi"):
        assert np.array_equal(auto.download(f), hand.download(f)), f
    assert not np.array_equal(auto.download("vel"), without.download("vel"))
    assert auto.bCollision and auto.bCollisionID == [0, 1] and not getattr(without, "bCollision", False)
    # ---- step 2: while the counter runs, UpdateObstacles returns the stored collision velocities (13069-13077)
    stored = [(o.collision_vel.copy(), o.collision_omega.copy()) for o in hand.obstacles]
    hand.step += 1
    hand.time += DT
    for n in ORDER[:4]:
        ops[n](DT)
    for o, (v, w) in zip(hand.obstacles, stored):
        assert np.array_equal(o.vel, v) and np.array_equal(o.omega, w)
        assert not np.array_equal(o.vel_computed, v)   # ... and not what the fluid momenta give
        assert o.collision_counter == 0.01 * DT - DT
    for n in ORDER[4:]:
        ops[n](DT)
    S.advance(DT)
    for a, b in zip(auto.obstacles, hand.obstacles):
        for f in ("vel", "omega", "force", "torque"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.collision_counter == b.collision_counter
    for f in ("vel", "pres"):
        assert np.array_equal(auto.download(f), hand.download(f)), f
