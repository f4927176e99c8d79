"""Device resources of the C-ABI objects: what cup3d_sim_create / the solvers / the mesh adaptation allocate, cup3d_sim_destroy gives
back (a long run of the reference adapts its mesh every 20 steps and rebuilds its device mirror each time, SURVEY 8b "Ownership")."""
import gc
import threading

import numpy as np
import pytest

import cup3d_amd as cu
from cup3d_amd.capi import check, lib

pytestmark = pytest.mark.gpu


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _one_life(block_solver, adapt):
    sim = cu.SimulationData(bpdx=1, bpdy=1, bpdz=1, levelMax=5 if adapt else 4, levelStart=3, extent=2 * np.pi, nu=0.01, BC_x="wall", BC_y="periodic",
                            BC_z="freespace", blockSolver=block_solver)
    g = sim.grid
    rng = np.random.default_rng(7)
    sim.upload("vel", rng.uniform(-1, 1, (g.nblocks, 8, 8, 8, 3)))
    S = cu.Simulation(sim)
    if adapt:
        cu.ComputeVorticity(S.sim)(0)
        w = S.sim.download("tmpV")
        linf = np.sqrt((w ** 2).sum(axis=-1)).reshape(S.sim.nblocks, -1).max(axis=1)
        S.adaptMesh(float(np.quantile(linf, 0.8)), -1.0)   # a second device mirror replaces the first
        assert S.sim.nblocks > g.nblocks
    S.sim.step = 5
    S.advance(0.01)
    assert S.sim.last_poisson.iterations > 0


def _run_ranks(fn, nranks):
    errs = [None] * nranks

    def work(r):
        try:
            fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    ts = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in errs:
        if e is not None:
            raise e


def _two_ranks(life):
    """life(nranks) under the in-process communicator of two thread ranks (cup3d_debug_virtual_comm)"""
    check(lib().cup3d_debug_virtual_comm(2))
    try:
        life(2)
        gc.collect()
    finally:
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)


def _life_ranks_multigrid(n):
    """(a) a uniform level-2 grid over two ranks, one step with the multigrid preconditioner: the comm-only sims of its coarse levels, the
    halo buffers"""
    kw = dict(bpdx=1, bpdy=1, bpdz=1, levelMax=3, levelStart=2, extent=2 * np.pi, nu=0.01, BC_x="wall", BC_y="periodic", BC_z="freespace", blockSolver=5)
    sims = [cu.SimulationData(rank=r, nranks=n, **kw) for r in range(n)]
    for r, s in enumerate(sims):
        s.upload("vel", np.random.default_rng(7 + r).uniform(-1, 1, (s.nblocks, 8, 8, 8, 3)))
        s.step = 5

    def rank(r):
        cu.AdvectionDiffusion(sims[r])(0.01)
        cu.PressureProjection(sims[r])(0.01)
        assert sims[r].last_poisson.iterations > 0

    _run_ranks(rank, n)


def _life_views_labs(n):
    """(b) the two-level mesh as two rank views, one step and one cup3d_sim_labs_over_ranks: the views' box tables, the ghost pool, LabsView"""
    import labs_ranks_cases as LC
    bpd, lmax, bc, ext, lv, zs = LC.mesh_recipe("amr_periodic_l01")
    mesh = cu.operators.Grid(bpd, lmax, 0, ext, bc, leaves=(lv, zs))
    owner = LC.owners(mesh.nblocks, "ranges", n, 0)
    views = [mesh.rank_view(owner, r, n) for r in range(n)]
    sims = [cu.SimulationData(view=views[r], levelStart=0, bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, extent=ext, nu=0.01, BC_x=bc[0], BC_y=bc[1],
                              BC_z=bc[2]) for r in range(n)]
    for r, s in enumerate(sims):
        s.upload("vel", np.random.default_rng(7 + r).uniform(-1, 1, (s.nblocks, 8, 8, 8, 3)))
        s.step = 5

    def rank(r):
        cu.AdvectionDiffusion(sims[r])(0.01)
        cu.PressureProjection(sims[r])(0.01)
        assert sims[r].last_poisson.iterations > 0
        assert sims[r].labs_over_ranks("vel", 4, mesh, owner, tensorial=True).shape[0] == sims[r].nblocks

    _run_ranks(rank, n)


def _life_obstacles():
    """(c) one rank with the spheres A, B of tests/collision_cases.py: the retained set, the resident plan, the forces scratch, LabTables"""
    import collision_cases as K
    c, obs = K.CC.case("uniform8"), K.obstacles("uniform8")
    sim = cu.SimulationData(**c.sim_kwargs)
    sim.upload("vel", np.random.default_rng(3).uniform(-1, 1, (c.nb, 8, 8, 8, 3)))
    sim.lambda_penal, sim.bImplicitPenalization, sim.resident_obstacles = 1e4, False, True
    sim.shapes, sim.obstacles = [cu.ObstacleShape(obs[k]["ids"], obs[k]["sdf"], obs[k]["udef"], obs[k]["transvel_correction"]) for k in "AB"], []
    cu.CreateObstacles(sim)(0.0)
    sim.obstacles = [s.data(K.APPROACH[k]["vel"], K.APPROACH[k]["omega"]) for s, k in zip(sim.shapes, "AB")]
    before = sim.device_bytes()
    cu.UpdateObstacles(sim)(K.DT)
    cu.Penalization(sim)(K.DT)
    check(lib().cup3d_update_tmpv_resident(sim.handle, 2))
    assert sim.device_bytes() > before   # the plan
    sim.surfaces = [s.surface(K.APPROACH[k]["vel"], K.APPROACH[k]["omega"]) for s, k in zip(sim.shapes, "AB")]
    assert all(len(q) for _, q in cu.ComputeForces(sim)(0))
    assert sim.labs("vel", 2).shape[0] == c.nb


_LIVES = {"ranks_multigrid": lambda: _two_ranks(_life_ranks_multigrid), "views_labs": lambda: _two_ranks(_life_views_labs), "obstacles": _life_obstacles}


@pytest.mark.parametrize("block_solver,adapt", [(0, False), (1, False), (5, False), (0, True), ("ranks_multigrid", None), ("views_labs", None),
                                                ("obstacles", None)])
def test_create_step_destroy_returns_the_device_memory(block_solver, adapt):
    """20 lives of a simulation (create, upload, [adapt], one full step, destroy): the free device memory afterwards is what it was
    after the first life (pinned staging buffers and the profiler's event pool are allocated once per process).  The named lives (_LIVES)
    cover what a one-rank step never allocates.  The 8 MiB bound cannot see a leaked index table of a few kilobytes: for those,
    tests/test_device_memory_owner.py (nothing is released by hand any more) and tests/test_gpu_device_bytes_ledger.py are the guard."""
    life = _LIVES[block_solver] if block_solver in _LIVES else (lambda: _one_life(block_solver, adapt))
    life()
    gc.collect()
    before = _free_bytes()
    for _ in range(20):
        life()
        gc.collect()
    after = _free_bytes()
    assert before - after < (8 << 20), f"{(before - after) / 2 ** 20:.1f} MiB of device memory lost over 20 create / destroy cycles"


def test_error_codes_instead_of_crashes():
    """No exception and no abort crosses the C boundary (SURVEY 8b "Errors"): misuse comes back as an error code with a message."""
    L = lib()
    assert L.cup3d_sim_upload(None, 0, np.zeros(1)) != 0
    sim = cu.SimulationData(bpdx=1, bpdy=1, bpdz=1, levelMax=2, levelStart=1, extent=1.0, BC_x="periodic", BC_y="periodic", BC_z="periodic")
    buf = np.zeros((sim.nblocks, 8, 8, 8))
    assert L.cup3d_sim_upload(sim.handle, 99, buf) != 0          # unknown field
    assert b"field" in L.cup3d_last_error()
    with pytest.raises(cu.capi.Cup3dError):
        check(L.cup3d_sim_upload(sim.handle, 99, buf))
    sim.blockSolver = 7                                                                              # unknown block solver code
    sim.upload("lhs", np.random.default_rng(0).uniform(-1, 1, buf.shape))
    with pytest.raises(cu.capi.Cup3dError):
        cu.makePoissonSolver(sim).solve()
