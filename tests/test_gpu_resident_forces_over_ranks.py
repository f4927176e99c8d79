"""cup3d_compute_forces_resident_over_ranks on a grid spread over 2 ranks, on ONE GPU -- the ranks are host threads of this process and
the in-process communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_resident_obstacles_over_ranks.py, whose two
obstacles this module uses: A on both ranks, and the part of A that rank 1 holds, of which rank 0 holds no block.  MI355X only (-m gpu).
The module runs with `poison_ghosts`: every cell of the ghost pool that did not travel is NaN.

Neither a tile nor a block's points and sums depend on how the mesh is partitioned, so each rank's points and rows must be, bit for bit,
what the ONE-RANK staged cup3d_compute_forces gives for that rank's blocks on the whole mesh.  The one-rank call is handed the rank's own
surface -- the centre of mass and corrected udef of a CreateObstacles over ranks are sums of two rank partials and differ from the
one-rank ones in the last bits (tests/test_gpu_create_obstacles_over_ranks.py), which is CreateObstacles' business, not this call's.
The totals are each rank's rows added in ascending slot order, then ONE addition of the two partial sums, which commutes: known exactly."""
import ctypes as C
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import resident_forces_cases as FC
from cup3d_amd.capi import ObstacleForces, RunStats, check, lib
from test_gpu_create_obstacles_over_ranks import NRANKS, ranks_of, share
from test_gpu_labs_over_ranks import VirtualComm, run_ranks
from test_gpu_resident_obstacles_over_ranks import two_obstacles

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
K = FC.K
CC = K.CC
ESTATE, ECOMM = -5, -4


@pytest.fixture(scope="module", autouse=True)
def _poison_the_cells_that_are_not_shipped():
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 1))
    yield
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 0))


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def mesh_of(c):
    """the global mesh object every rank holds"""
    if c.leaves is None:
        return cu.operators.uniform_share_mesh(c.bpd, c.lmax, c.sim_kwargs["levelStart"], CC.EXT, c.bc, NRANKS)[0]
    return cu.operators.Grid(c.bpd, c.lmax, 0, CC.EXT, c.bc, leaves=c.leaves)


def prepare(sims, name, owner, obstacles):
    for r, s in enumerate(sims):
        s.upload("vel", FC.vel_of(name)[owner == r])
        s.upload("pres", FC.pres_of(name)[owner == r])
        s.nu = FC.NU
        s.shapes, s.obstacles = [share(o, owner, r)[0] for o in obstacles], []


def rigid(sim):
    sim.obstacles = [s.data(K.APPROACH[k]["vel"], K.APPROACH[k]["omega"]) for s, k in zip(sim.shapes, "AB")]


def two_rounds(owner):
    """a forces_chunk with which the largest share of a rank takes two rounds of tile calls"""
    most = int(np.bincount(owner).max())
    chunk = (most + 1) // 2
    assert -(-most // chunk) == 2
    return chunk


@pytest.mark.parametrize("name", ["uniform8", "amr_periodic_l01"])   # one rank's share of a uniform grid; rank views of a two-level mesh
def test_each_rank_gets_the_one_rank_rows_of_its_blocks(name):
    c, owner, make_sims = ranks_of(name)
    mesh = mesh_of(c)
    obstacles = two_obstacles(c, owner)
    got = [[None, None] for _ in range(NRANKS)]
    held = [[None, None] for _ in range(NRANKS)]
    surfaces = [None] * NRANKS
    check(lib().cup3d_debug_set_option(b"forces_chunk", two_rounds(owner)))
    try:
        with VirtualComm(NRANKS):
            sims, views = make_sims()
            prepare(sims, name, owner, obstacles)
            assert len(sims[0].shapes[1].slots) == 0 and len(sims[1].shapes[1].slots) > 0
            before = [tuple(s.checksum(f) for f in ("vel", "pres")) for s in sims]

            def rank(r):
                s = sims[r]
                cu.CreateObstacles(s)(0.0)
                rigid(s)
                surfaces[r] = [sh.surface(o.vel, o.omega) for sh, o in zip(s.shapes, s.obstacles)]
                s.resident_obstacles = True
                for call in range(2):
                    got[r][call] = cu.ComputeForces(s)(0, mesh=mesh, owner=owner)
                    held[r][call] = [{f: np.array(getattr(o, f)).copy() for f in ("force_totals", "Pthrust", "Pdrag", "EffPDef", "EffPDefBnd")} for o in s.obstacles]

            run_ranks(rank, NRANKS)
            assert [tuple(s.checksum(f) for f in ("vel", "pres")) for s in sims] == before
            del sims, views
            gc.collect()
    finally:
        check(lib().cup3d_debug_set_option(b"forces_chunk", 0))
    # the one-rank run on the whole mesh: CreateObstacles leaves the same chi field there (chi does not depend on the partition)
    one = cu.SimulationData(**c.sim_kwargs)
    one.upload("vel", FC.vel_of(name))
    one.upload("pres", FC.pres_of(name))
    one.nu = FC.NU
    one.shapes, one.obstacles = [cu.ObstacleShape(o["ids"], o["sdf"], o["udef"], o["transvel_correction"]) for o in obstacles], []
    cu.CreateObstacles(one)(0.0)
    partial = [[None, None] for _ in range(NRANKS)]
    for r in range(NRANKS):
        mine = np.where(owner == r)[0]
        one.surfaces = [cu.ObstacleSurface(mine[s.slots], s.first, s.ijk, s.dchi, s.udef, s.cm, s.vel, s.omega) for s in surfaces[r]]
        for call in range(2):
            want = cu.ComputeForces(one)(0.0)
            for k, ((gp, gq), (wp, wq)) in enumerate(zip(got[r][call], want)):
                assert gp.shape == wp.shape and gq.shape == wq.shape
                assert np.array_equal(gp, wp), f"rank {r}, call {call}, obstacle {k}: points differ, max |d| = {np.abs(gp - wp).max():.3g}"
                assert np.array_equal(gq, wq), f"rank {r}, call {call}, obstacle {k}: block sums differ, max |d| = {np.abs(gq - wq).max():.3g}"
            partial[r][call] = [FC.totals(q, s.slots) for (_, q), s in zip(want, surfaces[r])]
    assert got[0][0][1][0].shape == (19, 0) and got[0][0][1][1].shape == (0, 19) and len(got[1][0][1][1]) > 0   # rank 0 holds none of the second obstacle
    assert min(len(got[r][0][0][1]) for r in range(NRANKS)) > 0
    for call in range(2):
        for k in range(2):
            total = partial[0][call][k] + partial[1][call][k]   # the all-reduce of two ranks
            for r in range(NRANKS):
                h = held[r][call][k]
                assert np.array_equal(h["force_totals"], total), (call, k, r)
                vel = K.APPROACH["AB"[k]]["vel"]
                assert (float(h["Pthrust"]), float(h["Pdrag"]), float(h["EffPDef"]), float(h["EffPDefBnd"])) == tuple(float(v) for v in FC.derived(total, vel))
            assert np.abs(total).max() > 0
    assert not np.array_equal(partial[1][1][1], partial[1][0][1])   # the carried sums moved between the calls
    del one
    gc.collect()


def test_nothing_retained_on_one_rank_is_an_error_on_both():
    """rank 0 has dropped its blocks: it still makes its tile rounds, asking for nothing, returns CUP3D_ESTATE and rank 1 CUP3D_ECOMM
    at the first obstacle's all-reduce; nothing of the caller's is written on either, and neither is left waiting for the other"""
    name = "uniform8"
    c, owner, make_sims = ranks_of(name)
    mesh = mesh_of(c)
    obstacles = two_obstacles(c, owner)
    status, untouched = {}, {}
    check(lib().cup3d_debug_set_option(b"forces_chunk", two_rounds(owner)))
    try:
        with VirtualComm(NRANKS):
            sims, _ = make_sims()
            prepare(sims, name, owner, obstacles)
            run_ranks(lambda r: cu.CreateObstacles(sims[r])(0.0), NRANKS)
            assert lib().cup3d_create_obstacles(sims[0].handle, -1, None) == -1   # a refused call drops what rank 0 held
            before = [tuple(s.checksum(f) for f in ("vel", "chi", "pres")) for s in sims]

            def rank(r):
                arr = (ObstacleForces * 2)()
                pts, rows = np.full((2, 19 * 4096), 5.0), np.full((2, 64 * 19), 6.0)
                for k in range(2):
                    for d in range(3):
                        arr[k].cm[d], arr[k].vel[d], arr[k].omega[d] = sims[r].shapes[k].cm[d], 0.25, 0.125
                    for q in range(19):
                        arr[k].totals[q] = 7.0
                    arr[k].Pthrust = arr[k].EffPDef = 7.0
                    arr[k].points, arr[k].qoi = pts[k].ctypes.data, rows[k].ctypes.data
                image = bytes(arr)
                status[r] = lib().cup3d_compute_forces_resident_over_ranks(sims[r].handle, mesh.handle, owner.ctypes.data_as(C.c_void_p), FC.NU, 2, arr)
                untouched[r] = bytes(arr) == image and bool((pts == 5.0).all()) and bool((rows == 6.0).all())

            run_ranks(rank, NRANKS)
            check(lib().cup3d_device_synchronize())
            assert [tuple(s.checksum(f) for f in ("vel", "chi", "pres")) for s in sims] == before
            del sims
            gc.collect()
    finally:
        check(lib().cup3d_debug_set_option(b"forces_chunk", 0))
    assert status == {0: ESTATE, 1: ECOMM}, status
    assert all(untouched.values()), untouched


def test_two_allreduces_per_obstacle():
    """19 sums and the flag cross the ranks in pieces of at most 16 values: 2 all-reduces per obstacle and rank, none for the tiles, and
    the count does not depend on the rank's share (rank 0 takes part in the second obstacle's with zeros).  cup3d_stats_read counts
    them process-wide, i.e. for both ranks (tests/test_gpu_obstacle_allreduce_counts.py)."""
    name = "uniform8"
    c, owner, make_sims = ranks_of(name)
    mesh = mesh_of(c)
    obstacles = two_obstacles(c, owner)
    with VirtualComm(NRANKS):
        sims, views = make_sims()
        prepare(sims, name, owner, obstacles)
        run_ranks(lambda r: cu.CreateObstacles(sims[r])(0.0), NRANKS)
        for s in sims:
            rigid(s)
            s.resident_obstacles = True
        counts = []
        for call in range(2):   # the first call builds the plans, the second does not: the same count
            st = RunStats()
            check(lib().cup3d_stats_reset())
            run_ranks(lambda r: cu.ComputeForces(sims[r])(0, mesh=mesh, owner=owner), NRANKS)
            check(lib().cup3d_stats_read(C.byref(st)))
            counts.append(int(st.allreduces))
            assert st.field_bytes_uploaded == 0
        del sims, views
        gc.collect()
    assert counts == [NRANKS * 2 * len(obstacles)] * 2, counts
