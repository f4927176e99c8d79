"""cup3d_compute_forces_over_ranks: the surface forces of obstacles on a mesh spread over ranks, on ONE GPU -- the ranks are host threads of
this process and the in-process communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_labs_over_ranks.py, whose
run_ranks / VirtualComm are used here.  MI355X only (-m gpu).

Neither a tile nor a block's points and sums depend on how the mesh is partitioned: each rank's points / qoi must equal, bit for bit, the
restatement on the GLOBAL mesh (tests/surface_forces_cases.py) restricted to the rank's blocks.  The module runs with `poison_ghosts`:
every cell of the ghost pool that did not travel is NaN."""
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import labs_ranks_cases as LC
import surface_forces_cases as SC
from cup3d_amd.capi import check, lib
from test_gpu_labs_over_ranks import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


@pytest.fixture(scope="module", autouse=True)
def _poison_the_cells_that_are_not_shipped():
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 1))
    yield
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 0))


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def share(e, owner, r, results):
    """rank r's part of every obstacle of e -- the blocks it owns, in the obstacle's order, with LOCAL slots -- and the part of
    `results` (the restatement on the global mesh) that belongs to them"""
    mine = np.where(owner == r)[0]
    local = {int(g): i for i, g in enumerate(mine)}
    surfaces, want = [], []
    for o, (points, qoi) in zip(e.obstacles, results):
        keep = [i for i, g in enumerate(o["slots"]) if owner[g] == r]
        cols = np.concatenate([np.arange(o["first"][i], o["first"][i + 1]) for i in keep]).astype(int) if keep else np.zeros(0, dtype=int)
        counts = [o["first"][i + 1] - o["first"][i] for i in keep]
        surfaces.append(cu.ObstacleSurface([local[int(o["slots"][i])] for i in keep], np.concatenate([[0], np.cumsum(counts)]), o["ijk"][cols], o["dchi"][cols],
                                           o["udef"][keep], o["cm"], o["vel"], o["omega"], o["qoi"][keep]))
        want.append((points[:, cols], qoi[keep]))
    return surfaces, want


def run(e, mesh, owner, sims, nranks):
    """two collective calls in a row on every rank; asserts each rank's results"""
    got = [[None, None] for _ in range(nranks)]
    parts = [share(e, owner, r, e.first_call) for r in range(nranks)]
    for r in range(nranks):
        sims[r].surfaces = parts[r][0]

    def rank(r):
        for call in range(2):
            got[r][call] = cu.ComputeForces(sims[r])(0, mesh=mesh, owner=owner)

    run_ranks(rank, nranks)
    for r in range(nranks):
        for call, results in enumerate((e.first_call, e.second_call)):
            want = share(e, owner, r, results)[1]
            for k, ((gp, gq), (wp, wq)) in enumerate(zip(got[r][call], want)):
                assert gp.shape == wp.shape and gq.shape == wq.shape
                assert np.array_equal(gp, wp), f"rank {r}, call {call}, obstacle {k}: points differ, max |d| = {np.abs(gp - wp).max():.3g}"
                assert np.array_equal(gq, wq), f"rank {r}, call {call}, obstacle {k}: block sums differ, max |d| = {np.abs(gq - wq).max():.3g}"


def view_sims(e, mesh, owner, nranks):
    views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
    sims = [cu.SimulationData(view=views[r], levelStart=0, **e.sim_kwargs()) for r in range(nranks)]
    for r, s in enumerate(sims):
        mine = views[r].global_slot[:views[r].nlocal]
        assert np.array_equal(mine, np.where(owner == r)[0])
        for f in ("vel", "chi", "pres"):
            s.upload(f, getattr(e, f)[mine])
    return views, sims


@pytest.mark.parametrize("kind,nranks,seed", [("ranges", 2, 0), ("scattered", 3, 11)])
def test_multi_level_mesh_over_ranks(kind, nranks, seed):
    e = SC.expected("amr_mixed_l12")
    mesh = cu.operators.Grid(e.bpd, e.lmax, 0, e.ext, e.bc, leaves=e.leaves)
    assert np.array_equal(mesh.tables, e.m.tables)
    owner = LC.owners(e.nb, kind, nranks, seed)
    a, b = e.obstacles
    if kind == "ranges":
        assert set(owner[a["slots"]].tolist()) == {0, 1}   # obstacle A lies on both sides of the rank boundary ...
        assert set(owner[b["slots"]].tolist()) == {1}      # ... and rank 0 holds none of B's blocks
    with VirtualComm(nranks):
        views, sims = view_sims(e, mesh, owner, nranks)
        assert sum(v.nghost for v in views) > 0
        before = [tuple(s.checksum(f) for f in ("vel", "chi", "pres")) for s in sims]
        run(e, mesh, owner, sims, nranks)
        assert [tuple(s.checksum(f) for f in ("vel", "chi", "pres")) for s in sims] == before
        del sims, views
        gc.collect()


def test_uniform_share_in_chunks():
    """one rank's share of a uniform grid on 2 ranks, with a tile scratch of 2 blocks: every rank makes the same number of tile rounds
    whatever its share of an obstacle is"""
    e = SC.expected("uniform64")
    nranks = 2
    mesh, owner = cu.operators.uniform_share_mesh(e.bpd, e.lmax, e.level, e.ext, e.bc, nranks)
    assert np.array_equal(mesh.tables, e.m.tables)
    a, b = e.obstacles
    assert set(owner[a["slots"]].tolist()) == {0, 1} and len(set(owner[b["slots"]].tolist())) == 1
    assert max(int((owner[a["slots"]] == r).sum()) for r in range(nranks)) > 2   # more blocks on a rank than one chunk holds
    check(lib().cup3d_debug_set_option(b"forces_chunk", 2))
    try:
        with VirtualComm(nranks):
            sims = [cu.SimulationData(rank=r, nranks=nranks, levelStart=e.level, **e.sim_kwargs()) for r in range(nranks)]
            for r, s in enumerate(sims):
                for f in ("vel", "chi", "pres"):
                    s.upload(f, getattr(e, f)[owner == r])
            run(e, mesh, owner, sims, nranks)
            del sims
            gc.collect()
    finally:
        check(lib().cup3d_debug_set_option(b"forces_chunk", 0))


def test_a_rank_with_refused_arguments_does_not_hold_up_the_others():
    """one rank's surface list is bad (an ijk of 8): that rank still makes its tile calls, asking for nothing, and returns CUP3D_EINVAL with
    nothing written; the other rank's results are the restatement's"""
    import ctypes as C
    from cup3d_amd.capi import ObstacleSurface
    e = SC.expected("amr_mixed_l12")
    mesh = cu.operators.Grid(e.bpd, e.lmax, 0, e.ext, e.bc, leaves=e.leaves)
    nranks, bad_rank = 2, 1
    owner = LC.owners(e.nb, "ranges", nranks, 0)
    got, status = [None] * nranks, [None] * nranks
    with VirtualComm(nranks):
        views, sims = view_sims(e, mesh, owner, nranks)
        parts = [share(e, owner, r, e.first_call) for r in range(nranks)]
        sims[0].surfaces = parts[0][0]
        surf = parts[bad_rank][0]
        assert len(surf[0].ijk) > 0
        surf[0].ijk[-1, 1] = 8
        pts = [np.full((19, len(o.ijk)), 5.0) for o in surf]
        qoi = [np.full((len(o.slots), 19), 6.0) for o in surf]
        arr = (ObstacleSurface * len(surf))()
        for a, o, p, q in zip(arr, surf, pts, qoi):
            a.nblocks = len(o.slots)
            a.slots, a.first, a.ijk, a.dchi, a.udef = (v.ctypes.data for v in (o.slots, o.first, o.ijk, o.dchi, o.udef))
            a.points, a.qoi = p.ctypes.data, q.ctypes.data
            for d in range(3):
                a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]

        def rank(r):
            if r == bad_rank:
                status[r] = lib().cup3d_compute_forces_over_ranks(sims[r].handle, mesh.handle, owner.ctypes.data_as(C.c_void_p), SC.NU, len(surf), arr)
            else:
                got[r] = cu.ComputeForces(sims[r])(0, mesh=mesh, owner=owner)
                status[r] = 0

        run_ranks(rank, nranks)
        check(lib().cup3d_device_synchronize())
        del sims, views
        gc.collect()
    assert status[bad_rank] == -1   # CUP3D_EINVAL
    assert all((p == 5.0).all() for p in pts) and all((q == 6.0).all() for q in qoi)
    for (gp, gq), (wp, wq) in zip(got[0], parts[0][1]):
        assert np.array_equal(gp, wp) and np.array_equal(gq, wq)
