"""The resident obstacle step on the blocks CreateObstacles leaves on the device: Simulation(sim, obstacle_operators=True,
collisions=True, resident_obstacles=True) runs the same pipeline as without the keyword, and UpdateObstacles, Penalization and
PressureProjection's tmpV update read the retained chi / udef instead of uploading them.  uniform8 with the spheres A and B in the flow of
tests/test_gpu_prevent_colliding_step.py, which carries A into B.  MI355X only (-m gpu)."""
import numpy as np
import pytest

import cup3d_amd as cu
from test_gpu_prevent_colliding_step import DT, ORDER, K, fresh

pytestmark = pytest.mark.gpu


def test_two_steps_equal_the_staged_run():
    c = K.CC.case("uniform8")
    staged, resident = fresh(c), fresh(c)
    S = cu.Simulation(staged, obstacle_operators=True, collisions=True, resident_obstacles=False)
    R = cu.Simulation(resident, obstacle_operators=True, collisions=True, resident_obstacles=True)
    assert [type(op).__name__ for op in R.pipeline] == [type(op).__name__ for op in S.pipeline] == ORDER
    assert resident.resident_obstacles is True and not getattr(staged, "resident_obstacles", False)
    for step in range(2):
        S.advance(DT)
        R.advance(DT)
        for f in ("vel", "pres", "chi"):
            assert np.array_equal(resident.download(f), staged.download(f)), (step, f)
        for a, b in zip(resident.obstacles, staged.obstacles):
            for f in ("vel", "omega", "force", "torque"):
                assert np.array_equal(getattr(a, f), getattr(b, f)), (step, f)
            assert a.collision_counter == b.collision_counter
        assert np.abs(staged.obstacles[0].force).max() > 0
    assert resident.bCollision and staged.bCollision


def test_the_keyword_needs_shapes():
    c = K.CC.case("uniform8")
    sim = fresh(c)
    sim.shapes = None
    with pytest.raises(ValueError, match="sim.shapes"):
        cu.Simulation(sim, obstacle_operators=True, resident_obstacles=True)
    assert not getattr(sim, "resident_obstacles", False)
    with pytest.raises(ValueError, match="obstacle_operators"):
        cu.Simulation(fresh(c), resident_obstacles=True)
    # without the keyword nothing is set
    plain = fresh(c)
    cu.Simulation(plain, obstacle_operators=True, collisions=True)
    assert not hasattr(plain, "resident_obstacles")
