"""cup3d_prevent_colliding_obstacles on a grid spread over 2 ranks, on ONE GPU -- the ranks are host threads of this process and the
in-process communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_create_obstacles_over_ranks.py, whose shares and
recombined restatement of cup3d_create_obstacles this test starts from.  MI355X only (-m gpu).

With two ranks each all-reduce is one max or one addition, so the totals are known exactly: the restatement's CollisionInfo of each
rank's blocks (tests/collision_restatement.py), combined as 14143-14207 combine them -- the momentum of the rank that does not hold the
maximum zeroed -- and then the pair loop.  Every rank returns those bits."""
import ctypes as C
import gc

import numpy as np
import pytest

import collision_cases as K
import collision_restatement as R
import cup3d_amd as cu
from cup3d_amd.capi import ObstacleCollision, check, lib
from test_gpu_create_obstacles_over_ranks import NRANKS, ranks_of, recombined, share
from test_gpu_labs_over_ranks import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
EINVAL, ECOMM, ESTATE = -1, -4, -5


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def raw_obstacles(name, keys):
    obs = K.obstacles(name)
    return [dict(ids=obs[k]["ids"], sdf=obs[k]["sdf"], udef=obs[k]["udef"], transvel_correction=obs[k]["transvel_correction"]) for k in keys]


@pytest.mark.parametrize("name", ["uniform8", "amr_periodic_l01"])
@pytest.mark.parametrize("which", ["approach", "three"])
def test_totals_over_ranks_and_the_same_motion_on_every_rank(name, which):
    c, owner, make_sims = ranks_of(name)
    keys, reverse, forced = K.SCENARIOS[which]
    obstacles = raw_obstacles(name, keys)
    # cup3d_create_obstacles over two ranks, by the restatement: chi per block, and cm, mass, J and the corrected udef from the recombined totals
    _, want_all = K.CR.create(c.geom, c.nb, obstacles)
    keeps = [[share(o, owner, r)[1] for r in range(NRANKS)] for o in obstacles]
    made = [recombined(c, o, w, kp) for o, w, kp in zip(obstacles, want_all, keeps)]
    bodies = [K.body(dict(cm=x["cm"], mass=x["mass"], J=x["J"]), k, reverse, k == forced) for x, k in zip(made, keys)]
    partials = []
    for r in range(NRANKS):
        mine = [dict(ids=o["ids"][kp[r]], sdf=o["sdf"][kp[r]], chi=w.chi[kp[r]], udef=x["udef"][kp[r]]) for o, w, x, kp in zip(obstacles, want_all, made, keeps)]
        partials.append(R.collision_info(c.geom, mine, bodies))
    trace = set()
    want = R.prevent(c.geom, None, bodies, K.DT, trace, partials=partials)
    assert ("resolved" in trace) == (which == "approach")
    # the ranks' partial maxima differ, so one rank's momentum is zeroed before the sum
    p = np.array(partials)
    assert (p[:, 0, 0] > 0).all()   # A and B touch on both sides of the rank boundary
    assert not np.array_equal((p[0, 0, 4:7] ** 2).sum(), (p[1, 0, 4:7] ** 2).sum())
    got = [None] * NRANKS
    with VirtualComm(NRANKS):
        sims, views = make_sims()
        for r, s in enumerate(sims):
            s.shapes = [share(o, owner, r)[0] for o in obstacles]
            s.obstacles = []
        before = [s.checksum("vel") for s in sims]

        def rank(r):
            s = sims[r]
            cu.CreateObstacles(s)(0.0)
            s.obstacles = [sh.data(b["vel"], b["omega"], forced=b["forced"]) for sh, b in zip(s.shapes, bodies)]
            for o, b in zip(s.obstacles, bodies):
                assert np.array_equal(o.cm, b["cm"]) and o.mass == b["mass"] and np.array_equal(o.J, b["J"])
            cu.PreventCollidingObstacles(s)(K.DT)
            got[r] = (s.obstacles, list(s.bCollisionID), bool(s.bCollision))

        run_ranks(rank, NRANKS)
        assert [s.checksum("vel") for s in sims] == before
        del sims, views
        gc.collect()
    for r in range(NRANKS):
        obst, ids, hit = got[r]
        assert ids == want.collided and hit == want.any, (r, ids, want.collided)
        for k, (o, b) in enumerate(zip(obst, want.bodies)):
            assert np.array_equal(o.collision_sums, np.array(want.sums[k])), (r, k, o.collision_sums, want.sums[k])
            for f in ("vel", "omega", "collision_vel", "collision_omega"):
                assert np.array_equal(getattr(o, f), np.array(b[f])), (r, k, f)
            assert o.collision_counter == b["collision_counter"]


def test_a_bad_argument_on_one_rank_is_an_error_on_both():
    """rank 1 passes dt = 0, then calls with nothing retained: it returns its own code, rank 0 CUP3D_ECOMM at the first all-reduce, nothing
    of the caller's is written on either, and neither is left waiting for the other"""
    c, owner, make_sims = ranks_of("uniform8")
    obstacles = raw_obstacles("uniform8", "AB")
    status, untouched = [[None] * NRANKS for _ in range(2)], [[None] * NRANKS for _ in range(2)]
    with VirtualComm(NRANKS):
        sims, _ = make_sims()
        for r, s in enumerate(sims):
            s.shapes = [share(o, owner, r)[0] for o in obstacles]
            s.obstacles = []

        def call(r, attempt, dt):
            arr = (ObstacleCollision * 2)()
            for a, sh in zip(arr, sims[r].shapes):
                a.mass = sh.mass
                for q in range(6):
                    a.J[q] = sh.J[q]
                for d in range(3):
                    a.cm[d], a.vel[d], a.collision_vel[d] = sh.cm[d], 0.25, 7.0
                for q in range(20):
                    a.sums[q] = 7.0
            ids = np.full(2, 7, dtype=np.int32)
            nids, hit = C.c_int(7), C.c_int(7)
            image = bytes(arr)
            status[attempt][r] = lib().cup3d_prevent_colliding_obstacles(sims[r].handle, dt, 2, arr, ids.ctypes.data_as(C.c_void_p), C.byref(nids), C.byref(hit))
            untouched[attempt][r] = bytes(arr) == image and (ids == 7).all() and nids.value == 7 and hit.value == 7

        def rank(r):
            cu.CreateObstacles(sims[r])(0.0)
            call(r, 0, 0.0 if r == 1 else K.DT)
            if r == 1:   # a refused cup3d_create_obstacles (not a collective: refused before anything is exchanged) drops the blocks
                assert lib().cup3d_create_obstacles(sims[r].handle, -1, None) == EINVAL
            call(r, 1, K.DT)

        run_ranks(rank, NRANKS)
        check(lib().cup3d_device_synchronize())
        del sims
        gc.collect()
    assert status[0] == [ECOMM, EINVAL] and status[1] == [ECOMM, ESTATE]
    assert all(untouched[0]) and all(untouched[1])
