"""cup3d_update_obstacles on a grid spread over 2 ranks, on ONE GPU -- the ranks are host threads of this process and the in-process
communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_labs_over_ranks.py, whose run_ranks / VirtualComm are used
here.  MI355X only (-m gpu).

A block's 29 sums do not depend on how the mesh is partitioned: each rank's block_sums must equal, bit for bit, the rows of the restatement
on the GLOBAL mesh (tests/fluid_momenta_cases.py) that belong to its blocks.  The totals are the same bits on both ranks and differ from the
one-rank totals by the reassociation of the block sum and nothing else: per entry at most nblocks eps sum_b |block sum_b|."""
import ctypes as C
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import fluid_momenta_cases as FC
import fluid_momenta_restatement as R
import labs_ranks_cases as LC
from cup3d_amd.capi import ObstacleMotion, check, lib
from test_gpu_labs_over_ranks import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
NRANKS = 2


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def ranks_of(name):
    """(case, owner [nb], geometry of the global mesh, make_sims) -- call make_sims() inside VirtualComm"""
    c = FC.case(name)
    if c.leaves is None:
        mesh, owner = cu.operators.uniform_share_mesh(c.bpd, c.lmax, c.sim_kwargs["levelStart"], FC.EXT, c.bc, NRANKS)

        def make_sims():
            return [cu.SimulationData(rank=r, nranks=NRANKS, **c.sim_kwargs) for r in range(NRANKS)], None
    else:
        mesh = cu.operators.Grid(c.bpd, c.lmax, 0, FC.EXT, c.bc, leaves=c.leaves)
        assert np.array_equal(mesh.tables, c.tables)
        owner = LC.owners(c.nb, "ranges", NRANKS, 0)

        def make_sims():
            views = [mesh.rank_view(owner, r, NRANKS) for r in range(NRANKS)]
            kw = {k: v for k, v in c.sim_kwargs.items() if k != "leaves"}
            return [cu.SimulationData(view=views[r], **kw) for r in range(NRANKS)], views
    return c, owner, mesh.geom.copy(), make_sims


def share(o, owner, r):
    """rank r's part of obstacle o: the blocks it owns, in the obstacle's order, with LOCAL slots; `keep` = their positions in o"""
    local = {int(g): i for i, g in enumerate(np.where(owner == r)[0])}
    keep = [i for i, g in enumerate(o["ids"]) if owner[g] == r]
    return cu.ObstacleData([local[int(o["ids"][i])] for i in keep], o["chi"][keep], o["udef"][keep].reshape(len(keep), 8, 8, 8, 3), o["cm"], o["vel"],
                           o["omega"]), keep


@pytest.mark.parametrize("name", ["uniform8", "amr_periodic_l01"])
@pytest.mark.parametrize("implicit", [0, 1])
def test_sums_per_rank_and_totals_over_ranks(name, implicit):
    c, owner, geom, make_sims = ranks_of(name)
    a = c.obstacles[0]
    assert set(owner[a["ids"]].tolist()) == {0, 1}          # obstacle A lies on both sides of the rank boundary
    only1 = [i for i, g in enumerate(a["ids"]) if owner[g] == 1]
    b = dict(a, ids=a["ids"][only1], chi=a["chi"][only1], udef=a["udef"][only1])   # ... and rank 0 holds none of this one's blocks
    obstacles = [a, b]
    want = [R.update(c.vel, geom, o["ids"], o["chi"], o["udef"], o["cm"], FC.LAMBDA, FC.DT, implicit) for o in obstacles]
    n = 29 if implicit else 13
    got = [None] * NRANKS
    with VirtualComm(NRANKS):
        sims, views = make_sims()
        for r, s in enumerate(sims):
            s.upload("vel", c.vel[owner == r])
            s.upload("chi", c.chi_field[owner == r])
            s.lambda_penal, s.bImplicitPenalization = FC.LAMBDA, bool(implicit)
            s.obstacles = [share(o, owner, r)[0] for o in obstacles]
        assert len(sims[0].obstacles[1].slots) == 0 and len(sims[1].obstacles[1].slots) > 0
        before = [s.checksum("vel") for s in sims]

        def rank(r):
            cu.UpdateObstacles(sims[r])(FC.DT)
            got[r] = sims[r].obstacles

        run_ranks(rank, NRANKS)
        assert [s.checksum("vel") for s in sims] == before
        del sims, views
        gc.collect()
    for k, (o, w) in enumerate(zip(obstacles, want)):
        for r in range(NRANKS):
            keep = share(o, owner, r)[1]
            assert got[r][k].block_sums.shape == (len(keep), 29)
            assert np.array_equal(got[r][k].block_sums[:, :n], w.rows[keep][:, :n]), f"obstacle {k}, rank {r}: block sums differ from the global restatement's rows"
        for f in ("totals", "vel", "omega", "vel_computed", "omega_computed"):
            assert np.array_equal(getattr(got[0][k], f), getattr(got[1][k], f)), (k, f)   # the same bits on both ranks
        bound = len(o["ids"]) * np.finfo(float).eps * np.abs(w.rows[:, :n]).sum(axis=0)
        d = np.abs(got[0][k].totals[:n] - w.M[:n])
        assert (d <= bound).all(), f"obstacle {k}: totals off by {d.max():.3g} in entries {np.where(d > bound)[0].tolist()}"
        assert (got[0][k].totals[n:] == 0).all()
        # the velocities are those of the restatement's solve from THESE totals
        q = R.Result()
        q.M = got[0][k].totals.tolist()
        R.finish(q, implicit)
        tol = FC.velocity_bound(q)
        assert np.abs(got[0][k].vel_computed - q.vel_computed).max() <= tol and np.abs(got[0][k].omega_computed - q.omega_computed).max() <= tol


def test_a_bad_slot_on_one_rank_is_an_error_on_both():
    """rank 1 lists a slot it does not have: both ranks return non-zero at the obstacle's all-reduce, nothing is written on either, and
    neither is left waiting for the other"""
    c, owner, geom, make_sims = ranks_of("uniform8")
    a = c.obstacles[0]
    status, untouched = [None] * NRANKS, [None] * NRANKS
    with VirtualComm(NRANKS):
        sims, _ = make_sims()
        parts = [share(a, owner, r)[0] for r in range(NRANKS)]
        for r, s in enumerate(sims):
            s.upload("vel", c.vel[owner == r])
        parts[1].slots[-1] = sims[1].nblocks

        def rank(r):
            arr = cu.operators._obstacle_array([parts[r]])
            mot = (ObstacleMotion * 1)()
            sums = np.full((len(parts[r].slots), 29), 7.0)
            mot[0].block_sums = sums.ctypes.data
            for q in range(29):
                mot[0].totals[q] = 5.0
            status[r] = lib().cup3d_update_obstacles(sims[r].handle, FC.DT, FC.LAMBDA, 1, 1, arr, mot)
            untouched[r] = bool((sums == 7.0).all()) and list(mot[0].totals) == [5.0] * 29 and list(arr[0].vel) == list(parts[r].vel)

        run_ranks(rank, NRANKS)
        check(lib().cup3d_device_synchronize())
        del sims
        gc.collect()
    assert status[1] == -1 and status[0] != 0   # CUP3D_EINVAL where the slot is bad, an error on the partner too
    assert all(untouched)
