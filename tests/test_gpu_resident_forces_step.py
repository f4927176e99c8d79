"""The whole resident obstacle step: Simulation(sim, obstacle_operators=True, collisions=True, resident_obstacles=True, forces=True) ends
with ComputeForces on the retained set, as setupOperators does (main.cpp:15244).  The twin runs the same step without the keyword and
then the staged ComputeForces on the surfaces its own CreateObstacles returned, with fresh sums -- every create restarts them.  uniform8
with the spheres A and B in the flow of tests/test_gpu_prevent_colliding_step.py.  MI355X only (-m gpu)."""
import numpy as np
import pytest

import cup3d_amd as cu
import resident_forces_cases as FC
from test_gpu_prevent_colliding_step import DT, ORDER, K, fresh

pytestmark = pytest.mark.gpu


def test_two_steps_equal_the_staged_run_and_its_forces():
    c = K.CC.case("uniform8")
    twin, resident = fresh(c), fresh(c)
    T = cu.Simulation(twin, obstacle_operators=True, collisions=True, resident_obstacles=True)
    R = cu.Simulation(resident, obstacle_operators=True, collisions=True, resident_obstacles=True, forces=True)
    assert [type(op).__name__ for op in T.pipeline] == ORDER and [type(op).__name__ for op in R.pipeline] == ORDER + ["ComputeForces"]
    totals = []
    for step in range(2):
        T.advance(DT)
        R.advance(DT)
        for f in ("vel", "pres", "chi"):
            assert np.array_equal(resident.download(f), twin.download(f)), (step, f)
        twin.surfaces = [s.surface(o.vel, o.omega) for s, o in zip(twin.shapes, twin.obstacles)]
        twin.resident_obstacles = False
        try:
            want = cu.ComputeForces(twin)(0.0)
        finally:
            twin.resident_obstacles = True
        for k, (o, surf, (points, qoi)) in enumerate(zip(resident.obstacles, twin.surfaces, want)):
            assert np.array_equal(o.force_points, points) and np.array_equal(o.force_rows, qoi), (step, k)
            t = FC.totals(qoi, surf.slots)
            assert np.array_equal(o.force_totals, t) and np.abs(t).max() > 0, (step, k)
            assert (o.Pthrust, o.Pdrag, o.EffPDef, o.EffPDefBnd) == tuple(float(v) for v in FC.derived(t, o.vel)), (step, k)
        totals.append(resident.obstacles[0].force_totals.copy())
    assert not np.array_equal(totals[0], totals[1])


def test_the_keyword_needs_the_retained_set():
    c = K.CC.case("uniform8")
    with pytest.raises(ValueError, match="resident_obstacles"):
        cu.Simulation(fresh(c), obstacle_operators=True, collisions=True, forces=True)
    # without the keyword the pipeline is what it was
    plain = cu.Simulation(fresh(c), obstacle_operators=True, collisions=True, resident_obstacles=True)
    assert [type(op).__name__ for op in plain.pipeline] == ORDER and plain.forces is False
    assert [type(op).__name__ for op in cu.Simulation(fresh(c), obstacle_operators=True, collisions=True).pipeline] == ORDER
