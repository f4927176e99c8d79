"""The resident obstacle operators on a grid spread over 2 ranks, on ONE GPU -- the ranks are host threads of this process and the
in-process communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_update_obstacles_over_ranks.py.  MI355X only
(-m gpu).

On every rank cup3d_update_obstacles_resident, cup3d_penalization_resident and cup3d_update_tmpv_resident must give, bit for bit, what the
staged calls give there from the same state: the kernels share their bodies and the all-reduce protocol is the same one, per obstacle in
obstacle order, a rank without blocks of an obstacle taking part with zeros."""
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import resident_obstacles_cases as RC
from cup3d_amd.capi import ObstacleBody, ObstacleMotion, check, lib
from test_gpu_create_obstacles_over_ranks import NRANKS, ranks_of, share
from test_gpu_labs_over_ranks import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
K = RC.K
ESTATE, ECOMM = -5, -4
FIELDS = ("block_sums", "totals", "vel_computed", "omega_computed", "vel", "omega", "force", "torque")


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def two_obstacles(c, owner):
    """A, which lies on both sides of the rank boundary, and the part of A that rank 1 holds: rank 0 holds none of its blocks"""
    a = c.obstacles[0]
    assert set(owner[a["ids"]].tolist()) == {0, 1}
    only1 = [i for i, g in enumerate(a["ids"]) if owner[g] == 1]
    return [a, dict(a, ids=a["ids"][only1], sdf=a["sdf"][only1], udef=a["udef"][only1])]


def rigid(sim):
    sim.obstacles = [s.data(K.APPROACH[k]["vel"], K.APPROACH[k]["omega"]) for s, k in zip(sim.shapes, "AB")]


def sequence(sim, resident):
    sim.resident_obstacles = resident
    n = len(sim.obstacles)
    cu.UpdateObstacles(sim)(RC.DT)
    cu.Penalization(sim)(RC.DT)
    sim.fill("tmpV", 0.0)
    if resident:
        check(lib().cup3d_update_tmpv_resident(sim.handle, n))
    else:
        check(lib().cup3d_update_tmpv(sim.handle, n, cu.operators._obstacle_array(sim.obstacles)))
    out = dict(obstacles=[{f: np.array(getattr(o, f)).copy() for f in FIELDS} for o in sim.obstacles])
    for f in ("vel", "tmpV", "chi"):
        out[f] = sim.download(f)
    return out


@pytest.mark.parametrize("name", ["uniform8", "amr_periodic_l01"])
@pytest.mark.parametrize("implicit", [0, 1])
def test_resident_equals_staged_on_every_rank(name, implicit):
    c, owner, make_sims = ranks_of(name)
    obstacles = two_obstacles(c, owner)
    vel = RC.vel_of(name)
    staged, resident = [None] * NRANKS, [None] * NRANKS
    with VirtualComm(NRANKS):
        sims, views = make_sims()
        for r, s in enumerate(sims):
            s.upload("vel", vel[owner == r])
            s.lambda_penal, s.bImplicitPenalization = RC.LAMBDA, bool(implicit)
            s.shapes, s.obstacles = [share(o, owner, r)[0] for o in obstacles], []
        assert len(sims[0].shapes[1].slots) == 0 and len(sims[1].shapes[1].slots) > 0

        def first(r):
            cu.CreateObstacles(sims[r])(0.0)
            rigid(sims[r])
            staged[r] = sequence(sims[r], False)

        run_ranks(first, NRANKS)
        for r, s in enumerate(sims):   # the same state again: the blocks CreateObstacles left are still on the device
            s.upload("vel", vel[owner == r])
            rigid(s)

        def second(r):
            resident[r] = sequence(sims[r], True)

        run_ranks(second, NRANKS)
        del sims, views
        gc.collect()
    for r in range(NRANKS):
        for k, (g, w) in enumerate(zip(resident[r]["obstacles"], staged[r]["obstacles"])):
            for f in FIELDS:
                assert np.array_equal(g[f], w[f]), (r, k, f)
        for f in ("vel", "tmpV", "chi"):
            assert np.array_equal(resident[r][f], staged[r][f]), (r, f)
        assert not np.array_equal(staged[r]["vel"], vel[owner == r])
    for k in range(2):   # the totals, the velocities and the forces are the same bits on both ranks
        for f in FIELDS[1:]:
            assert np.array_equal(resident[0]["obstacles"][k][f], resident[1]["obstacles"][k][f]), (k, f)
        assert np.abs(resident[0]["obstacles"][k]["force"]).max() > 0
    assert resident[0]["obstacles"][1]["block_sums"].shape == (0, 29)


def test_nothing_retained_on_one_rank_is_an_error_on_both():
    """rank 0 has dropped its blocks: it returns CUP3D_ESTATE, rank 1 CUP3D_ECOMM at the first obstacle's all-reduce, nothing of the
    caller's is written on either, and neither is left waiting for the other"""
    c, owner, make_sims = ranks_of("uniform8")
    obstacles = two_obstacles(c, owner)
    status, untouched = {}, {}
    with VirtualComm(NRANKS):
        sims, _ = make_sims()
        for r, s in enumerate(sims):
            s.upload("vel", RC.vel_of("uniform8")[owner == r])
            s.shapes, s.obstacles = [share(o, owner, r)[0] for o in obstacles], []
        run_ranks(lambda r: cu.CreateObstacles(sims[r])(0.0), NRANKS)
        assert lib().cup3d_create_obstacles(sims[0].handle, -1, None) == -1   # a refused call drops what rank 0 held
        before = [s.checksum("vel") for s in sims]

        def rank(r):
            for which in ("update", "penalization"):
                body, mot = (ObstacleBody * 2)(), (ObstacleMotion * 2)()
                for k in range(2):
                    for d in range(3):
                        body[k].cm[d], body[k].vel[d], body[k].force[d] = sims[r].shapes[k].cm[d], 0.25, 7.0
                    for q in range(29):
                        mot[k].totals[q] = 7.0
                image = bytes(body), bytes(mot)
                if which == "update":
                    status[r, which] = lib().cup3d_update_obstacles_resident(sims[r].handle, RC.DT, RC.LAMBDA, 1, 2, body, mot)
                else:
                    status[r, which] = lib().cup3d_penalization_resident(sims[r].handle, RC.DT, RC.LAMBDA, 1, 2, body)
                untouched[r, which] = (bytes(body), bytes(mot)) == image

        run_ranks(rank, NRANKS)
        check(lib().cup3d_device_synchronize())
        assert [s.checksum("vel") for s in sims][0] == before[0]
        del sims
        gc.collect()
    for which in ("update", "penalization"):
        assert status[0, which] == ESTATE and status[1, which] == ECOMM, (which, status)
    assert all(untouched.values()), untouched
