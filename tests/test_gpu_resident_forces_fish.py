"""cup3d_compute_forces_resident against the compiled reference's own fish, bit for bit.  MI355X only (-m gpu); fixtures only.

tests/golden/fish_one_*.npz (tests/fish_cases.py) holds what the unmodified reference, on one OpenMP thread, left after ComputeForces
for StefanFish, first and second call: the 19 per-point arrays, the blocks' nineteen sums and -- `f1.o0.totals`, `f2.o0.totals` -- what
Obstacle::computeForces (main.cpp:13079-13107) made of them.  The resident call reads nothing but what cup3d_create_obstacles left on
the device and the fixture's vel and pres, and must return all three; test_compute_forces_on_the_created_surface_first_and_second_call
(tests/test_gpu_fish_fixtures.py) makes no exception for any sum, and neither does this."""
import numpy as np
import pytest

import cup3d_amd as cu
import fish_cases as F
import surface_forces_restatement as SF
from test_gpu_fish_fixtures import create, same

pytestmark = pytest.mark.gpu
S = F.STATE


def test_two_resident_calls_on_the_created_fish():
    d, sim = create("fish_one")
    s = d["f1.in.o0.state"]
    sim.obstacles = [sim.shapes[0].data(s[S["vel"]], s[S["omega"]])]
    same(sim.obstacles[0].cm, s[S["cm"]], "the centre of mass the reference's call started from")
    sim.resident_obstacles = True
    try:
        for call in ("f1", "f2"):
            f = F.obstacle(d, call, 0)
            (points, qoi), = cu.ComputeForces(sim)(0.0)
            for a, name in enumerate(SF.POINT_NAMES):
                same(points[a], f["points"][a], (call, name))
            for a, name in enumerate(SF.QOI_NAMES):
                same(qoi[:, a], f["qoi"][:, a], (call, name))
            same(sim.obstacles[0].force_totals, d[f"{call}.o0.totals"], (call, "Obstacle::computeForces"))
    finally:
        sim.resident_obstacles = False
    assert not np.array_equal(d["f2.o0.totals"], d["f1.o0.totals"])
    assert len(F.obstacle(d, "f1", 0)["qoi"]) == 16 and F.obstacle(d, "f1", 0)["points"].shape[1] == 686
    same(sim.download("vel"), d["vel"], "vel is only read")
