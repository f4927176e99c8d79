"""How many all-reduces each obstacle operator issues on a grid spread over 2 ranks, on ONE GPU -- the ranks are host threads of this
process and the in-process communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_resident_obstacles_over_ranks.py,
whose two obstacles this test uses: A on both ranks, B on rank 1 only, so that rank 0 takes part in B's all-reduces with zeros.
MI355X only (-m gpu).

The operators share one host protocol (sums_over_ranks, csrc/obstacles_penalization.hip): n sums and an error flag in pieces of at most 16
values.  Per rank and per obstacle that is 1 all-reduce for the penalisation force (6 + flag), 2 for UpdateObstacles (29 + flag: 16 + 14)
and 2 for CreateObstacles (4 + flag, 13 + flag); the collision model of N obstacles takes ceil((2 N + 1) / 16) for the maxima and
ceil(20 N / 16) for the sums, 1 + 3 for N = 2.  cup3d_stats_read counts them process-wide, i.e. for both ranks."""
import ctypes as C
import gc

import pytest

import cup3d_amd as cu
import resident_obstacles_cases as RC
from cup3d_amd.capi import RunStats, check, lib
from test_gpu_create_obstacles_over_ranks import NRANKS, ranks_of, share
from test_gpu_labs_over_ranks import VirtualComm, run_ranks
from test_gpu_resident_obstacles_over_ranks import rigid, two_obstacles

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
NOBST = 2
PER_RANK = {"create": 2 * NOBST, "update": 2 * NOBST, "update_resident": 2 * NOBST, "penalization": NOBST, "penalization_resident": NOBST,
            "collisions": 1 + 3}


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def test_allreduces_per_operator():
    c, owner, make_sims = ranks_of("uniform8")
    obstacles = two_obstacles(c, owner)
    vel = RC.vel_of("uniform8")
    got = {}
    with VirtualComm(NRANKS):
        sims, views = make_sims()
        for r, s in enumerate(sims):
            s.upload("vel", vel[owner == r])
            s.lambda_penal, s.bImplicitPenalization = RC.LAMBDA, True
            s.shapes, s.obstacles = [share(o, owner, r)[0] for o in obstacles], []
        assert len(sims[0].shapes[1].slots) == 0 and len(sims[1].shapes[1].slots) > 0

        def counted(what, op, resident=False):
            def rank(r):
                sims[r].resident_obstacles = resident
                op(sims[r])(RC.DT)

            st = RunStats()
            check(lib().cup3d_stats_reset())
            run_ranks(rank, NRANKS)
            check(lib().cup3d_stats_read(C.byref(st)))
            got[what] = int(st.allreduces)

        counted("create", cu.CreateObstacles)
        for s in sims:
            rigid(s)
        counted("update", cu.UpdateObstacles)
        counted("update_resident", cu.UpdateObstacles, resident=True)
        counted("penalization", cu.Penalization)
        counted("penalization_resident", cu.Penalization, resident=True)
        counted("collisions", cu.PreventCollidingObstacles)
        del sims, views
        gc.collect()
    print("all-reduces of both ranks:", got)
    assert got == {what: NRANKS * n for what, n in PER_RANK.items()}
