"""The multi-rank control flow of the hot path executed on ONE GPU: the ranks of a run are host threads of this process, each
driving its own device mirror through the ordinary C-ABI entry points, and an in-process communicator (cup3d_debug_virtual_comm)
stands in for RCCL -- device copies between the ranks' pack buffers, a rank-ordered sum for the all-reduces, host barriers for
the ordering.  Everything else is the code that runs under `torch.distributed.run`: the Hilbert-range partition, the halo plans,
the pack kernels, the inner/boundary split, the ghost-block and face-flux exchanges of multi-level meshes
(SynchronizerMPI_AMR::fetch 2423-2544, FluxCorrectionMPI 2848-2945), which rank owns the corner cell of the mean constraint, and
the order of the collectives inside PoissonSolverAMR::solve (14363-14616).  MI355X only (-m gpu).

Stated bounds
  * stencil operators (advect-diffuse RK3, LHS without the mean row, pressure RHS with chi / udef, divP, gradP, vorticity):
    BIT-EXACT against the one-rank oracle, on uniform grids and on multi-level meshes spread over 2 / 3 / 5 ranks;
  * findMaxU: exact (max is order independent);
  * projection: the dot products are summed per rank and then over ranks, another rounding than on one rank, so the comparison is
    at tight Poisson tolerance (1e-12 / 1e-10 on both sides): max|dp| <= 1e-6 max|p|, max|du| <= 1e-6 max|correction|, identical
    iteration / restart counts on all ranks of a run; at the default tolerance the returned iterate satisfies the reference's
    stopping rule.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import cup3d_amd as cu
import helmholtz_cases as H
import implicit_step_restatement as ST
import multigrid_cases as K
import oracle_lib as O
from cup3d_amd.capi import check, lib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
EXT = 2 * np.pi


@pytest.fixture(scope="module", autouse=True)
def _poison_the_cells_that_are_not_shipped():
    """Every test of this file runs with `poison_ghosts`: after each sub-box ghost exchange of a rank view the ghost blocks hold NaN in every
    cell that did not travel.  The tests compare with the one-rank oracle bit for bit, so a consumer that read a cell outside the box the
    exchange plan gives its block (Grid::ghost_box) would turn them red."""
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 1))
    yield
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 0))


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def run_ranks(fn, nranks):
    """fn(rank) on one host thread per rank; the first exception of any rank is re-raised."""
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


class VirtualComm:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        check(lib().cup3d_debug_virtual_comm(self.n))
        return self

    def __exit__(self, *a):
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)


# ------------------------------------------------------------------ uniform grids: face-slab halos + the solver's all-reduces
@pytest.mark.parametrize("nranks", [2, 3, 8])
@pytest.mark.parametrize("bc", [("periodic", "periodic", "periodic"), ("wall", "periodic", "freespace")])
def test_uniform_grid_full_step_over_ranks(nranks, bc):
    bpd, lmax, level = (2, 2, 2), 2, 1
    o = O.OracleGrid(bpd, lmax, level, EXT, bc)
    rng = np.random.default_rng(9)
    NX, NY, NZ = o.ncell
    velg, presg = rng.uniform(-1, 1, (NZ, NY, NX, 3)), rng.uniform(-1, 1, (NZ, NY, NX))
    dt, nu, uinf = 0.02, 0.01, np.array([0.1, 0.2, -0.3])
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=nu, uinf=uinf)
    # one-rank device run of the same thing (tight tolerance) for the solver comparison
    one = cu.SimulationData(poissonTol=1e-12, poissonTolRel=1e-10, **kw)
    one.upload("vel", one.grid.to_blocks(velg))
    cu.AdvectionDiffusion(one)(dt)
    one.step = 5
    cu.PressureProjection(one)(dt)
    vel_one, pres_one = np.zeros_like(velg), np.zeros_like(presg)
    one.grid.scatter_to_global(one.download("vel"), vel_one)
    one.grid.scatter_to_global(one.download("pres"), pres_one)
    ref, tmp = o.to_blocks(velg), np.zeros((o.nb, 8, 8, 8, 3))
    o.advect_diffuse(ref, tmp, dt, nu, uinf)
    adv_ref = o.to_global(ref)
    out = {}
    with VirtualComm(nranks):
        sims = [cu.SimulationData(rank=r, nranks=nranks, poissonTol=1e-12, poissonTolRel=1e-10, **kw) for r in range(nranks)]
        assert sum(s.nblocks for s in sims) == o.nb

        def rank(r):
            s = sims[r]
            s.upload("vel", s.grid.to_blocks(velg))
            umax = cu.findMaxU(s)
            cu.AdvectionDiffusion(s)(dt)
            adv = s.download("vel")
            s.step = 5
            res = cu.PressureProjection(s)(dt)
            out[r] = (umax, adv, s.download("vel"), s.download("pres"), res.iterations, res.restarts)

        run_ranks(rank, nranks)
        got_adv, got_vel, got_pres = np.zeros_like(velg), np.zeros_like(velg), np.zeros_like(presg)
        for r, s in enumerate(sims):
            s.grid.scatter_to_global(out[r][1], got_adv)
            s.grid.scatter_to_global(out[r][2], got_vel)
            s.grid.scatter_to_global(out[r][3], got_pres)
        del sims
    assert all(out[r][0] == np.abs(velg + uinf).max() for r in range(nranks))
    assert np.array_equal(got_adv, adv_ref)                              # halo slabs + inner/boundary split: bit-exact
    assert len({(out[r][4], out[r][5]) for r in range(nranks)}) == 1     # every rank took the same path through solve()
    # (not compared with the one-rank run: this deep into the residual -- 1e-12 / 1e-10 -- whether a "serious breakdown" restart
    #  fires, 14566, depends on the rounding of the dot products: 1 restart on 8 ranks vs 0 on one rank was observed)
    corr = np.abs(vel_one - adv_ref).max()
    assert np.abs(got_pres - pres_one).max() <= 1e-6 * np.abs(pres_one).max()
    assert np.abs(got_vel - vel_one).max() <= 1e-6 * corr


def test_uniform_grid_default_tolerance_over_ranks():
    """Default Poisson tolerances on 3 ranks: the iterate the sharded solver returns satisfies the reference's stopping rule, with
    the residual evaluated by the ORACLE's operator on the gathered field."""
    bpd, lmax, level, bc, nranks = (2, 2, 2), 3, 2, ("wall", "wall", "wall"), 3
    o = O.OracleGrid(bpd, lmax, level, EXT, bc)
    vel = o.taylor_green([EXT] * 3, 1.0)
    velg = o.to_global(vel)
    dt = 0.3 * o.h
    b = o.pressure_rhs(vel, np.zeros_like(vel), np.zeros((o.nb, 8, 8, 8)), dt)
    bg = o.to_global(b)
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    out = {}
    with VirtualComm(nranks):
        sims = [cu.SimulationData(rank=r, nranks=nranks, **kw) for r in range(nranks)]

        def rank(r):
            s = sims[r]
            s.upload("vel", s.grid.to_blocks(velg))
            check(lib().cup3d_pressure_rhs(s.handle, dt))
            rhs = s.download("lhs")
            s.fill("pres", 0.0)
            res = cu.makePoissonSolver(s).solve()
            out[r] = (rhs, s.download("pres"), res.iterations, res.norm0)

        run_ranks(rank, nranks)
        got_b, got_x = np.zeros_like(bg), np.zeros_like(bg)
        for r, s in enumerate(sims):
            s.grid.scatter_to_global(out[r][0], got_b)
            s.grid.scatter_to_global(out[r][1], got_x)
        del sims
    assert np.array_equal(got_b, bg)
    x = o.to_blocks(got_x)
    b0 = b.copy()
    b0[int(np.where((o.index == 0).all(axis=1))[0][0]), 0, 0, 0] = 0.0
    res = np.linalg.norm((b0 - o.lhs(x, 1)).ravel())
    res0 = np.linalg.norm(b0.ravel())
    assert abs(out[0][3] - res0) <= 1e-10 * res0
    assert res <= max(1e-6, 1e-4 * res0) * (1 + 1e-6), (res, res0, out[0][2])
    xo = np.zeros_like(b)
    info = o.solve(b.copy(), xo)
    assert out[0][2] <= 1.3 * info.iters + 5, (out[0][2], info.iters)


# ------------------------------------------------------------------ multi-level meshes spread over ranks (rank views)
_mesh_case = K.mesh_case   # the three three-level meshes (shared with the V-cycle tests: tests/multigrid_cases.py)


def _owners(nb, nranks, kind, seed=0):
    if kind == "ranges":  # contiguous runs of the m_vInfo order, the shape GridMPI / LoadBalancer leave behind
        return (np.arange(nb) * nranks // nb).astype(np.int32)
    rng = np.random.default_rng(seed)  # scattered ownership: every neighbour relation crosses ranks somewhere
    ow = rng.integers(0, nranks, nb).astype(np.int32)
    ow[:nranks] = np.arange(nranks)
    return ow


@pytest.mark.parametrize("nranks,kind", [(2, "ranges"), (3, "ranges"), (5, "ranges"), (3, "scattered")])
@pytest.mark.parametrize("name", ["l012_wall", "l012_periodic", "l012_box322"])
def test_multilevel_mesh_over_ranks_stencils_bitexact(name, nranks, kind):
    bpd, lmax, bc, lv, zs = _mesh_case(name)
    m = O.OracleMesh(bpd, lmax, EXT, bc, lv, zs)
    mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
    assert np.array_equal(mesh.tables, m.tables)
    nb = m.nb
    owner = _owners(nb, nranks, kind, seed=len(name))
    rng = np.random.default_rng(5)
    f = dict(vel=rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), pres=rng.uniform(-1, 1, (nb, 8, 8, 8)), udef=rng.uniform(-1, 1, (nb, 8, 8, 8, 3)),
             chi=(rng.uniform(0, 1, (nb, 8, 8, 8)) > 0.7) * rng.uniform(0, 1, (nb, 8, 8, 8)))
    dt, nu, uinf = 0.01, 0.02, (0.1, -0.2, 0.3)
    ref = dict(adv=m.advect_diffuse(f["vel"], dt, nu, uinf)[0], lhs=m.lhs(f["pres"], 0), rhs=m.pressure_rhs(f["vel"], f["udef"], f["chi"], dt),
               rhs0=m.pressure_rhs(f["vel"], np.zeros_like(f["vel"]), np.zeros_like(f["pres"]), dt), divp=m.div_pressure(f["pres"])[..., 0],
               gradp=m.grad_p(f["pres"], dt), vort=m.vorticity(f["vel"]), maxu=m.max_u(f["vel"], uinf))
    got = {k: np.zeros_like(v) for k, v in ref.items() if k != "maxu"}
    maxu = [None] * nranks
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=nu, uinf=uinf)
    with VirtualComm(nranks):
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]
        assert sum(v.nghost for v in views) > 0

        def rank(r):
            s, v = sims[r], views[r]
            mine = v.global_slot[:v.nlocal]
            s.upload("vel", f["vel"][mine])
            maxu[r] = cu.findMaxU(s)
            cu.AdvectionDiffusion(s)(dt)
            got["adv"][mine] = s.download("vel")
            s.upload("pres", f["pres"][mine])
            s.bMeanConstraint = 0
            cu.ComputeLHS(s)(0)
            got["lhs"][mine] = s.download("lhs")
            s.upload("vel", f["vel"][mine]); s.upload("tmpV", f["udef"][mine]); s.upload("chi", f["chi"][mine])
            check(lib().cup3d_pressure_rhs(s.handle, dt))
            got["rhs"][mine] = s.download("lhs")
            s.fill("chi", 0.0); s.fill("tmpV", 0.0)
            check(lib().cup3d_pressure_rhs(s.handle, dt))
            got["rhs0"][mine] = s.download("lhs")
            check(lib().cup3d_div_pressure(s.handle))
            got["divp"][mine] = s.download("tmpV")[..., 0]
            check(lib().cup3d_grad_p(s.handle, dt))
            got["gradp"][mine] = s.download("tmpV")
            cu.ComputeVorticity(s)(0)
            got["vort"][mine] = s.download("tmpV")

        run_ranks(rank, nranks)
        del sims, views
    assert all(u == ref["maxu"] for u in maxu)
    for k in got:
        assert np.array_equal(got[k], ref[k]), (name, nranks, kind, k, np.abs(got[k] - ref[k]).max())


@pytest.mark.parametrize("nranks,kind", [(2, "ranges"), (3, "scattered")])
@pytest.mark.parametrize("name", ["l012_wall", "l012_box322"])
def test_multilevel_mesh_over_ranks_projection(name, nranks, kind):
    """PressureProjection (second-order pressure path, mean constraint 1) on a three-level mesh spread over ranks, tight tolerance on
    both sides, against the one-rank oracle; two steps of advect-diffuse + projection stay together."""
    bpd, lmax, bc, lv, zs = _mesh_case(name)
    m = O.OracleMesh(bpd, lmax, EXT, bc, lv, zs)
    mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
    nb = m.nb
    owner = _owners(nb, nranks, kind, seed=7)
    rng = np.random.default_rng(11)
    vel0, pres0 = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    dt, nu = 0.01, 0.02
    v, p = vel0.copy(), pres0.copy()
    info, _, _ = m.project(v, p, dt, 5, tol=1e-12, tol_rel=1e-10)
    corr = np.abs(v - vel0).max()
    v2, _ = m.advect_diffuse(v, dt, nu, (0, 0, 0))
    p2 = p.copy()
    m.project(v2, p2, dt, 6, tol=1e-12, tol_rel=1e-10)
    got_v, got_p, got_v2 = np.zeros_like(v), np.zeros_like(p), np.zeros_like(v)
    its = [None] * nranks
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=nu,
              poissonTol=1e-12, poissonTolRel=1e-10)
    with VirtualComm(nranks):
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]

        def rank(r):
            s, vw = sims[r], views[r]
            mine = vw.global_slot[:vw.nlocal]
            s.upload("vel", vel0[mine]); s.upload("pres", pres0[mine])
            s.step = 5
            res = cu.PressureProjection(s)(dt)
            its[r] = (res.iterations, res.restarts)
            got_v[mine], got_p[mine] = s.download("vel"), s.download("pres")
            cu.AdvectionDiffusion(s)(dt)
            s.step = 6
            cu.PressureProjection(s)(dt)
            got_v2[mine] = s.download("vel")

        run_ranks(rank, nranks)
        del sims, views
    assert len(set(its)) == 1
    assert its[0][0] <= 1.3 * info.iters + 5, (its, info.iters)
    assert np.abs(got_p - p).max() <= 1e-6 * np.abs(p).max()
    assert np.abs(got_v - v).max() <= 1e-6 * corr
    assert np.abs(got_v2 - v2).max() <= 1e-6 * max(corr, np.abs(v2 - v).max())


@pytest.mark.parametrize("nranks,kind", [(2, "ranges"), (3, "ranges"), (3, "scattered"), (5, "scattered")])
@pytest.mark.parametrize("name", ["l012_wall", "l012_periodic", "l012_box322"])
def test_multigrid_on_a_multilevel_mesh_over_ranks(name, nranks, kind):
    """block_solver 5 on a multi-level mesh SPREAD OVER RANKS: one V-cycle over all ranks on the octree's levels.  Every rank holds its
    owned nodes of every level (leaves + ancestors; an ancestor lives with its first child) plus ghost nodes; the iterate's ghost nodes are
    refreshed before every launch that reads them, restricted octants travel to remote parents, prolongation and coarse/fine ghosts read
    the remote parent's final iterate (Grid::mg_hierarchy, multigrid.hip).  Below the level-0 mean (one all-reduce instead of one
    workgroup's sum) the distributed cycle computes what the one-rank cycle computes:
      * ONE application M^-1 r (cup3d_preconditioner) equals the one-rank application to rounding of that mean (1e-13 of the result);
      * the projection with it: the same pressure as the one-rank multigrid run to 5e-6 (both stopped by the same rule), the same iteration
        count (+-1), every rank on the same path."""
    bpd, lmax, bc, lv, zs = _mesh_case(name)
    mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
    nb = mesh.nblocks
    owner = _owners(nb, nranks, kind, seed=3 + len(name))
    rng = np.random.default_rng(21)
    r0 = rng.uniform(-1, 1, (nb, 8, 8, 8))
    vel0, pres0 = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    dt = 0.01
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=0.02,
              poissonTol=1e-11, poissonTolRel=1e-10, blockSolver=5)
    one = cu.SimulationData(leaves=(lv, zs), **kw)
    one.upload("pres", r0)
    check(lib().cup3d_preconditioner(one.handle, 5))
    z_one = one.download("pres")
    one.upload("vel", vel0); one.upload("pres", pres0)
    one.step = 5
    res_one = cu.PressureProjection(one)(dt)
    v_one, p_one = one.download("vel"), one.download("pres")
    z, v, p = np.zeros_like(z_one), np.zeros_like(v_one), np.zeros_like(p_one)
    its = [None] * nranks
    with VirtualComm(nranks):
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]

        def rank(r):
            s, vw = sims[r], views[r]
            mine = vw.global_slot[:vw.nlocal]
            s.upload("pres", r0[mine])
            check(lib().cup3d_preconditioner(s.handle, 5))
            z[mine] = s.download("pres")
            s.upload("vel", vel0[mine]); s.upload("pres", pres0[mine])
            s.step = 5
            res = cu.PressureProjection(s)(dt)
            its[r] = (res.iterations, res.restarts)
            v[mine], p[mine] = s.download("vel"), s.download("pres")

        run_ranks(rank, nranks)
        del sims, views
    assert np.abs(z - z_one).max() <= 1e-12 * np.abs(z_one).max(), np.abs(z - z_one).max() / np.abs(z_one).max()
    assert len(set(its)) == 1, its
    print(f"{name} on {nranks} ranks ({kind}): {its[0][0]} iterations, one rank {res_one.iterations}")
    assert abs(its[0][0] - res_one.iterations) <= 1, (its, res_one.iterations)
    assert np.abs(p - p_one).max() <= 5e-6 * np.abs(p_one).max()      # (two solves stopped by the same rule: cond(A) x the residual tolerance; 6e-7 seen)
    assert np.abs(v - v_one).max() <= 5e-6 * np.abs(v_one - vel0).max()    # (13 against 14 iterations on l012_wall: 1.2e-6 seen)


@pytest.mark.parametrize("name,nranks,kind", [("l012_wall", 3, "ranges"), ("l012_box322", 5, "scattered"), ("l012_periodic", 2, "ranges")])
def test_sub_box_ghost_exchange_same_bits_fewer_bytes(name, nranks, kind):
    """The ghost-block exchange of rank views in its sub-box form (only the box of cells the star-stencil consumers read: the w layers
    behind a shared face, the 2w layers a restriction averages, the coarse shadow patch of an interpolation -- comm.hip, Grid::ghost_box)
    against whole 8^3 ghost blocks (`whole_ghost_blocks`): advect-diffuse (width 3, vector), LHS, pressure RHS with chi / udef, gradP,
    vorticity (width 1) give the SAME BITS -- with every cell that is not shipped poisoned with NaN (the module-wide `poison_ghosts`), so a
    consumer reading outside its box could not go unnoticed -- and fewer bytes cross ranks."""
    bpd, lmax, bc, lv, zs = _mesh_case(name)
    mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
    nb = mesh.nblocks
    owner = _owners(nb, nranks, kind, seed=11)
    rng = np.random.default_rng(8)
    f = dict(vel=rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), pres=rng.uniform(-1, 1, (nb, 8, 8, 8)), udef=rng.uniform(-1, 1, (nb, 8, 8, 8, 3)),
             chi=(rng.uniform(0, 1, (nb, 8, 8, 8)) > 0.7) * rng.uniform(0, 1, (nb, 8, 8, 8)))
    dt, nu, uinf = 0.01, 0.02, (0.1, -0.2, 0.3)
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=nu, uinf=uinf)
    res, sent = {}, {}
    for whole in (0, 1):
        check(lib().cup3d_debug_set_option(b"whole_ghost_blocks", whole))
        try:
            got = {k: np.zeros((nb, 8, 8, 8, 3)) for k in ("adv", "gradp", "vort")}
            got.update({k: np.zeros((nb, 8, 8, 8)) for k in ("lhs", "rhs")})
            with VirtualComm(nranks):
                views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
                sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]
                lib().cup3d_stats_reset()

                def rank(r):
                    s, v = sims[r], views[r]
                    mine = v.global_slot[:v.nlocal]
                    s.upload("vel", f["vel"][mine])
                    cu.AdvectionDiffusion(s)(dt)
                    got["adv"][mine] = s.download("vel")
                    s.upload("pres", f["pres"][mine])
                    s.bMeanConstraint = 0
                    cu.ComputeLHS(s)(0)
                    got["lhs"][mine] = s.download("lhs")
                    s.upload("vel", f["vel"][mine]); s.upload("tmpV", f["udef"][mine]); s.upload("chi", f["chi"][mine])
                    check(lib().cup3d_pressure_rhs(s.handle, dt))
                    got["rhs"][mine] = s.download("lhs")
                    check(lib().cup3d_grad_p(s.handle, dt))
                    got["gradp"][mine] = s.download("tmpV")
                    cu.ComputeVorticity(s)(0)
                    got["vort"][mine] = s.download("tmpV")

                run_ranks(rank, nranks)
                st = cu.capi.RunStats()
                lib().cup3d_stats_read(C.byref(st))
                sent[whole] = st.halo_bytes_sent
                del sims, views
            res[whole] = got
        finally:
            check(lib().cup3d_debug_set_option(b"whole_ghost_blocks", 0))
    for k in res[0]:
        assert not np.isnan(res[0][k]).any(), k
        assert np.array_equal(res[0][k], res[1][k]), (name, nranks, kind, k)
    print(f"{name} on {nranks} ranks ({kind}): {sent[0] / 1e6:.2f} MB in sub-boxes, {sent[1] / 1e6:.2f} MB as whole blocks (x{sent[1] / sent[0]:.2f})")
    assert sent[0] < sent[1]


# ------------------------------------------------------------------ mesh adaptation over ranks: the LoadBalancer's block traffic
def _states_from_tables(old, new):
    """valid states of the old leaves that turn the old block list into the new one"""
    have = {(int(l), int(i), int(j), int(k)) for l, _, i, j, k, _ in new}
    st = np.zeros(len(old), dtype=np.int8)
    for b, (l, _, i, j, k, _) in enumerate(old):
        if (int(l), int(i), int(j), int(k)) in have:
            continue
        st[b] = 1 if (int(l) + 1, 2 * int(i), 2 * int(j), 2 * int(k)) in have else -1
    return st


@pytest.mark.parametrize("case", [0, 1, 2, 3, 5])
def test_block_migration_equals_one_rank_adaptation(golden_dir, case):
    """tests/golden/adapt_mpi.npz holds transitions of the reference's adaptMesh under a REAL MPI: block list and owner rank of every
    block before and after (children with the refined parent, octets gathered on the base block's rank, Balance_Diffusion /
    Balance_Global).  cup3d_adapt_migrate carries vel and pres from the old ownership to the new one; every rank ends up with the
    reference's block list for that rank, filled with exactly the bits the one-rank adaptation (itself pinned against the
    reference) produces."""
    z = np.load(os.path.join(golden_dir, "adapt_mpi.npz"))
    bx, by, bz, lmax, b0, b1, b2, nranks = (int(v) for v in z[f"t{case}_meta"])
    old, new, ow_old, ow_new = z[f"t{case}_old"], z[f"t{case}_new"], z[f"t{case}_old_owner"].astype(np.int32), z[f"t{case}_new_owner"].astype(np.int32)
    st = _states_from_tables(old, new)
    bpd, bc = (bx, by, bz), (b0, b1, b2)
    g_old = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(old[:, 0].astype(np.int32), old[:, 1].copy()))
    assert np.array_equal(g_old.tables[:, :2], old[:, :2])
    rng = np.random.default_rng(case)
    nb = len(old)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    bcn = {0: "freespace", 1: "periodic", 2: "wall"}
    kw = dict(bpdx=bx, bpdy=by, bpdz=bz, levelMax=lmax, levelStart=0, extent=EXT, BC_x=bcn[b0], BC_y=bcn[b1], BC_z=bcn[b2])
    one = cu.SimulationData(leaves=(old[:, 0].astype(np.int32), old[:, 1].copy()), **kw)
    one.upload("vel", vel); one.upload("pres", pres)
    ref = one.adapted(st)
    assert np.array_equal(ref.grid.tables[:, :2], new[:, :2])
    vel_ref, pres_ref = ref.download("vel"), ref.download("pres")
    got_v, got_p = np.zeros_like(vel_ref), np.zeros_like(pres_ref)
    tabs = [None] * nranks
    with VirtualComm(nranks):
        views = [g_old.rank_view(ow_old, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]
        news = [None] * nranks

        def rank(r):
            s, v = sims[r], views[r]
            mine = v.global_slot[:v.nlocal]
            s.upload("vel", vel[mine]); s.upload("pres", pres[mine])
            n, new_mesh, new_owner = s.adapted_over_ranks(g_old, ow_old, st, r, nranks)
            assert np.array_equal(new_owner, ow_new)      # the LoadBalancer's ownership rule, pinned against the MPI reference
            sel = np.where(new_owner == r)[0]
            tabs[r] = n.grid.tables
            got_v[sel], got_p[sel] = n.download("vel"), n.download("pres")
            news[r] = n

        run_ranks(rank, nranks)
        del sims, views, news
    for r in range(nranks):
        assert np.array_equal(tabs[r][:, :2], new[ow_new == r][:, :2]), r   # the reference's block list of that rank
    assert np.array_equal(got_v, vel_ref) and np.array_equal(got_p, pres_ref)


@pytest.mark.parametrize("bad_rank", [0, 2])
def test_a_bad_call_on_one_rank_fails_on_every_rank_at_once(golden_dir, bad_rank):
    """Collective status agreement (comm.hip, agree): cup3d_adapt_migrate is a collective; when ONE rank's call is invalid -- here an
    unknown field id, found by that rank's local checks -- every rank must get an error back before anything is exchanged, within
    seconds, instead of the valid ranks blocking in the exchange for ever (the reference ends such runs with MPI_Abort on all ranks,
    main.cpp:15265, 15289).  The communicator stays usable: the same ranks then complete a correct migration."""
    import time
    z = np.load(os.path.join(golden_dir, "adapt_mpi.npz"))
    case = 1
    bx, by, bz, lmax, b0, b1, b2, nranks = (int(v) for v in z[f"t{case}_meta"])
    old, new, ow_old = z[f"t{case}_old"], z[f"t{case}_new"], z[f"t{case}_old_owner"].astype(np.int32)
    assert bad_rank < nranks
    st = _states_from_tables(old, new)
    g_old = cu.operators.Grid((bx, by, bz), lmax, 0, EXT, (b0, b1, b2), leaves=(old[:, 0].astype(np.int32), old[:, 1].copy()))
    bcn = {0: "freespace", 1: "periodic", 2: "wall"}
    kw = dict(bpdx=bx, bpdy=by, bpdz=bz, levelMax=lmax, levelStart=0, extent=EXT, BC_x=bcn[b0], BC_y=bcn[b1], BC_z=bcn[b2])
    lv, zs = g_old.adapted_leaves(st)
    new_mesh = cu.operators.Grid((bx, by, bz), lmax, 0, EXT, (b0, b1, b2), leaves=(lv, zs))
    new_owner = g_old.adapted_owners(ow_old, st, nranks, new_mesh)
    codes, texts, took = [None] * nranks, [None] * nranks, [None] * nranks
    with VirtualComm(nranks):
        views = [g_old.rank_view(ow_old, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]
        dsts = [sims[r]._like(view=new_mesh.rank_view(new_owner, r, nranks)) for r in range(nranks)]

        def migrate(r, field):
            return lib().cup3d_adapt_migrate(g_old.handle, ow_old.ctypes.data_as(C.c_void_p), sims[r].handle, new_mesh.handle,
                                             new_owner.ctypes.data_as(C.c_void_p), dsts[r].handle, field)

        def rank(r):
            t0 = time.time()
            codes[r] = migrate(r, 99 if r == bad_rank else cu.operators.FIELDS["vel"])
            texts[r] = lib().cup3d_last_error().decode()
            took[r] = time.time() - t0

        run_ranks(rank, nranks)
        assert all(c == -1 for c in codes), codes                       # CUP3D_EINVAL everywhere: the worst code any rank arrived with
        assert max(took) < 5.0, took
        assert "unknown field id" in texts[bad_rank]
        assert all("another rank could not take part" in texts[r] for r in range(nranks) if r != bad_rank), texts
        # ... and the communicator is not left half-way through an exchange: a correct collective call works right after
        ok = [None] * nranks

        def again(r):
            ok[r] = migrate(r, cu.operators.FIELDS["vel"])

        run_ranks(again, nranks)
        assert ok == [0] * nranks, ok
        del sims, views, dsts


def test_adaptive_loop_on_three_ranks_equals_one_rank():
    """adaptMesh every step (vorticity tags -> gathered -> ValidStates -> Adapt + LoadBalancer + block migration) alternating with the
    advection-diffusion step, on 3 ranks and on one: block lists identical at every step, velocity bit-identical (every operator
    involved is order independent), and the owners follow the LoadBalancer's rule."""
    bpd, lmax, bc, nu, nranks = (2, 2, 2), 3, ("periodic", "wall", "freespace"), 0.05, 3
    g0 = cu.operators.Grid(bpd, lmax, 0, EXT, bc)
    lv, zs = g0.tables[:, 0].astype(np.int32), g0.tables[:, 1].copy()
    geom, nb = g0.geom, g0.nblocks
    ax = np.arange(8) + 0.5
    vel = np.zeros((nb, 8, 8, 8, 3))
    for b in range(nb):   # a compact vortex: refinement stays local
        h = geom[b, 0]
        Z, Y, X = np.meshgrid(geom[b, 3] + ax * h, geom[b, 2] + ax * h, geom[b, 1] + ax * h, indexing="ij")
        gss = np.exp(-((X - 2.5) ** 2 + (Y - 3.0) ** 2 + (Z - 3.2) ** 2) / 0.8)
        vel[b, ..., 0], vel[b, ..., 1], vel[b, ..., 2] = -(Y - 3.0) * gss, (X - 2.5) * gss, 0.2 * gss
    kw = dict(bpdx=2, bpdy=2, bpdz=2, levelMax=lmax, levelStart=0, extent=EXT, nu=nu, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    one = cu.SimulationData(leaves=(lv, zs), **kw)
    one.upload("vel", vel)
    S1 = cu.Simulation(one)
    cu.ComputeVorticity(one)(0)
    w = one.download("tmpV")
    linf = np.sqrt((w ** 2).sum(axis=-1)).reshape(nb, -1).max(axis=1)
    rt, ct = float(np.quantile(linf, 0.6)), float(np.quantile(linf, 0.4))
    dt, nsteps = 0.02, 5
    ref = []
    for n in range(nsteps):
        S1.adaptMesh(rt, ct)
        cu.AdvectionDiffusion(S1.sim)(dt)
        ref.append((S1.sim.grid.tables.copy(), S1.sim.download("vel")))
    assert len({len(t) for t, _ in ref}) >= 3
    # three ranks
    mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
    owner = (np.arange(nb) * nranks // nb).astype(np.int32)
    gathered, bar = [None] * nranks, threading.Barrier(nranks)
    state = [None] * nranks
    got = [[None] * nranks for _ in range(nsteps)]
    with VirtualComm(nranks):
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]

        def rank(r):
            def allgather(a):
                gathered[r] = a.copy()
                bar.wait(timeout=60)
                out = [g.copy() for g in gathered]
                bar.wait(timeout=60)
                return out
            s = sims[r]
            s.upload("vel", vel[views[r].global_slot[:views[r].nlocal]])
            S, m, ow = cu.Simulation(s), mesh, owner
            for n in range(nsteps):
                _, m, ow = S.adaptMeshOverRanks(m, ow, r, nranks, rt, ct, allgather)
                cu.AdvectionDiffusion(S.sim)(dt)
                got[n][r] = (m.tables.copy(), np.asarray(ow).copy(), S.sim.grid.tables.copy(), S.sim.download("vel"))
            state[r] = S

        run_ranks(rank, nranks)
        del sims, views, state
    for n in range(nsteps):
        tab, vref = ref[n]
        gt, ow = got[n][0][0], got[n][0][1]
        assert np.array_equal(gt, tab), n                                   # the global block list, bit-exactly
        cnt = np.bincount(ow, minlength=nranks)
        assert cnt.min() > 0
        v = np.zeros_like(vref)
        for r in range(nranks):
            assert np.array_equal(got[n][r][1], ow)
            assert np.array_equal(got[n][r][2], tab[ow == r]), (n, r)       # each rank holds its share, in the global order
            v[ow == r] = got[n][r][3]
        assert np.array_equal(v, vref), n


@pytest.mark.parametrize("nranks", [4, 8])
def test_adapted_mesh_of_thousands_of_blocks_over_ranks(nranks):
    """A three-level mesh of a few thousand blocks built by the device's own adaptMesh around a compact vortex (the shape of
    `bench.py --amr`, one size down), then spread over 4 / 8 ranks in contiguous runs of the m_vInfo order: one full step -- advect-diffuse
    bit-exact against the one-rank device run, projection at tight tolerance to 1e-6 -- with send lists of hundreds of ghost blocks and
    face-flux arrays per rank."""
    ext, lmax, base = 2 * np.pi, 6, 3
    kw = dict(bpdx=1, bpdy=1, bpdz=1, levelMax=lmax, levelStart=base, extent=ext, nu=0.002, BC_x="wall", BC_y="periodic", BC_z="freespace",
              poissonTol=1e-12, poissonTolRel=1e-10)
    sim = cu.SimulationData(**kw)
    g = sim.grid
    ax = np.arange(8) + 0.5
    X = (g.index[:, 0, None] * 8 + ax[None, :])[:, None, None, :] * g.h
    Y = (g.index[:, 1, None] * 8 + ax[None, :])[:, None, :, None] * g.h
    Z = (g.index[:, 2, None] * 8 + ax[None, :])[:, :, None, None] * g.h
    gss = np.exp(-((X - 2.6) ** 2 + (Y - 3.1) ** 2 + (Z - 3.4) ** 2) / 0.6)
    sim.upload("vel", np.ascontiguousarray(np.stack([-(Y - 3.1) * gss, (X - 2.6) * gss, 0.3 * gss + 0 * X], axis=-1)))
    S = cu.Simulation(sim)
    for _ in range(2):
        cu.ComputeVorticity(S.sim)(0)
        w = S.sim.download("tmpV")
        linf = np.sqrt((w ** 2).sum(axis=-1)).reshape(S.sim.nblocks, -1).max(axis=1)
        S.adaptMesh(float(np.quantile(linf, 0.7)), -1.0)
    one = S.sim
    t = one.grid.tables
    nb = one.nblocks
    assert nb > 2000 and len(set(t[:, 0].tolist())) == 3
    vel0, dt = one.download("vel"), 0.01
    cu.AdvectionDiffusion(one)(dt)
    adv_ref = one.download("vel")
    one.step = 5
    cu.PressureProjection(one)(dt)
    vel_ref, pres_ref = one.download("vel"), one.download("pres")
    corr = np.abs(vel_ref - adv_ref).max()
    mesh = cu.operators.Grid((1, 1, 1), lmax, 0, ext, ("wall", "periodic", "freespace"), leaves=(t[:, 0].astype(np.int32), t[:, 1].copy()))
    owner = (np.arange(nb) * nranks // nb).astype(np.int32)
    got_adv, got_vel, got_pres = np.zeros_like(vel0), np.zeros_like(vel0), np.zeros_like(pres_ref)
    its = [None] * nranks
    kw.pop("levelStart")
    with VirtualComm(nranks):
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(levelStart=0, view=views[r], **kw) for r in range(nranks)]
        assert min(v.nghost for v in views) > 100
        assert all(0 < v.ninner < v.nlocal for v in views)   # both passes of every stencil launch run: inner blocks, then the ones that wait

        def rank(r):
            s, mine = sims[r], views[r].global_slot[:views[r].nlocal]
            s.upload("vel", vel0[mine])
            cu.AdvectionDiffusion(s)(dt)
            got_adv[mine] = s.download("vel")
            s.step = 5
            res = cu.PressureProjection(s)(dt)
            its[r] = res.iterations
            got_vel[mine], got_pres[mine] = s.download("vel"), s.download("pres")

        run_ranks(rank, nranks)
        del sims, views
    assert np.array_equal(got_adv, adv_ref)
    assert len(set(its)) == 1
    assert np.abs(got_pres - pres_ref).max() <= 1e-6 * np.abs(pres_ref).max()
    assert np.abs(got_vel - vel_ref).max() <= 1e-6 * corr


@pytest.mark.parametrize("nranks,level", [(2, 3), (8, 3), (4, 4)])
def test_multigrid_preconditioner_coupled_over_ranks(nranks, level):
    """block_solver 5 over ranks: ONE V-cycle over all ranks -- every level partitioned like the solver's grid, its iterate exchanged as
    face slabs before every launch that reads ghosts (multigrid.hip mg_setup).  Same operator, same stopping rule: the converged
    pressure equals the one-rank block-CG run's to solver tolerance, every rank takes the same path, and the iteration count stays
    within 2 of the ONE-RANK multigrid run (the levels below the one where the partition stops nesting are replaced by sweeps)."""
    bpd, lmax, bc = (1, 1, 1), level + 1, ("wall", "wall", "wall")
    kw = dict(bpdx=1, bpdy=1, bpdz=1, levelMax=lmax, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=0.01,
              poissonTol=1e-11, poissonTolRel=1e-9)
    one = cu.SimulationData(**kw)
    g = one.grid
    n = 8 << level
    from bench import taylor_green_blocks
    vel = taylor_green_blocks(g, [EXT] * 3, 1.0)
    one.upload("vel", vel)
    dt = 0.3 * g.h
    one.step = 5
    r1 = cu.PressureProjection(one)(dt)
    mg1 = cu.SimulationData(blockSolver=5, **kw)           # the one-rank multigrid run: the iteration count to match
    mg1.upload("vel", vel)
    mg1.step = 5
    rmg = cu.PressureProjection(mg1)(dt)
    del mg1
    pres_one, vel_one = np.zeros((n, n, n)), np.zeros((n, n, n, 3))
    g.scatter_to_global(one.download("pres"), pres_one)
    g.scatter_to_global(one.download("vel"), vel_one)
    velg = np.zeros((n, n, n, 3))
    g.scatter_to_global(vel, velg)
    out = {}
    with VirtualComm(nranks):
        sims = [cu.SimulationData(rank=r, nranks=nranks, blockSolver=5, **kw) for r in range(nranks)]

        def rank(r):
            s = sims[r]
            s.upload("vel", s.grid.to_blocks(velg))
            s.step = 5
            res = cu.PressureProjection(s)(dt)
            out[r] = (s.download("vel"), s.download("pres"), res.iterations)

        run_ranks(rank, nranks)
        got_vel, got_pres = np.zeros_like(velg), np.zeros_like(pres_one)
        for r, s in enumerate(sims):
            s.grid.scatter_to_global(out[r][0], got_vel)
            s.grid.scatter_to_global(out[r][1], got_pres)
        del sims
    its = {out[r][2] for r in range(nranks)}
    assert len(its) == 1
    it = its.pop()
    print(f"multigrid over {nranks} ranks, {n}^3: {it} BiCGSTAB iterations (multigrid on one rank: {rmg.iterations}, block CG on one rank: {r1.iterations})")
    assert it <= rmg.iterations + 2 and it < r1.iterations // 2
    corr = np.abs(vel_one - velg).max()
    assert np.abs(got_pres - pres_one).max() <= 1e-6 * np.abs(pres_one).max()
    assert np.abs(got_vel - vel_one).max() <= 1e-6 * corr


@pytest.mark.parametrize("nranks", [2, 4])
def test_multigrid_cycle_over_ranks_equals_the_restatement(nranks):
    """ONE application of the uniform V-cycle coupled over ranks (cup3d_preconditioner(sim, 5) on every rank, in place) against the dense
    NumPy restatement in longdouble -- the first check of this cycle over ranks against anything but itself.  (1,1,1) level 2, walls: the
    partition of 2 or 4 ranks nests down to level 1 and no further, so the restatement's hierarchy has depth 2, its coarsest level (8
    blocks) takes 16 x 4 and loses its mean over ALL cells (one all-reduce on the device).  Tolerance as in tests/test_gpu_multigrid_cycle.py:
    32 x max(|z_f64 - z_ld|, 4 eps max|z_ld|); observed ratio 1.11 on 2 and on 4 ranks."""
    bpd, level, bc = K.RANKS_CASE
    r, (z64, zld) = K.restated_uniform("ranks", "random", depth=2, coarsest=(16, 4))
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=level + 1, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], blockSolver=5)
    out = {}
    with VirtualComm(nranks):
        sims = [cu.SimulationData(rank=q, nranks=nranks, **kw) for q in range(nranks)]

        def rank(q):
            s = sims[q]
            s.upload("pres", s.grid.to_blocks(r))
            check(lib().cup3d_preconditioner(s.handle, 5))
            out[q] = s.download("pres")

        run_ranks(rank, nranks)
        z = np.full_like(r, np.nan)
        for q, s in enumerate(sims):
            s.grid.scatter_to_global(out[q], z)
        del sims
    assert np.isfinite(z).all()
    unit = K.tolerance(z64, zld) / K.MARGIN
    err = float(np.abs(z - zld).max())
    print(f"V-cycle over {nranks} ranks: max|z_dev - z_ld| = {err:.3e} = {err / unit:.2f} x max(|z_f64 - z_ld|, 4 eps |z_ld|) (bound {K.MARGIN})")
    assert err <= K.MARGIN * unit


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("name", ["amr_periodic_l01", "amr_mixed_l12"])
def test_grad_chi_on_tmp_over_ranks_equals_the_reference(golden_dir, name, nranks):
    """compute<ScalarLab>(GradChiOnTmp(sim), sim.chi) on a multi-level mesh spread over ranks: chi of the edge / corner / finer neighbours
    other ranks own arrives by the plan of the rank's tensorial view; the gathered tmpV equals the REFERENCE's output bit for bit
    (tests/golden/grad_chi.npz, the one-rank pin of tests/test_gpu_amr.py), with and without the levelMaxVorticity cap."""
    BCN = {0: "periodic", 1: "wall", 2: "freespace"}
    z, vz = np.load(os.path.join(golden_dir, "grad_chi.npz")), np.load(os.path.join(golden_dir, "vorticity.npz"))
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    t = g["tables"]
    bpd, lmax, bc = tuple(int(b) for b in g["bpd"]), int(g["level_max"]), tuple(BCN[int(b)] for b in g["bc"])
    ext = float(g["extent"])
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    mesh = cu.operators.Grid(bpd, lmax, 0, ext, bc, leaves=(t[:, 0].astype(np.int32), t[:, 1].copy()))
    nb = len(t)
    owner = (np.arange(nb) * nranks // nb).astype(np.int32)
    rt, ct = (float(v) for v in vz[name + "_tol"])
    chi, vort = z[name + "_chi"], vz[name + "_vort"]
    got = {tag: np.zeros_like(vort) for tag in ("", "_capped")}
    with VirtualComm(nranks):
        views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]

        def rank(r):
            s, mine = sims[r], views[r].global_slot[:views[r].nlocal]
            s.Rtol, s.Ctol = rt, ct
            s.upload("chi", chi[mine])
            for tag, lmv in (("", lmax), ("_capped", lmax - 1)):
                s.levelMaxVorticity = lmv
                s.upload("tmpV", vort[mine])
                cu.GradChiOnTmp(s)(0, mesh=mesh, owner=owner)
                got[tag][mine] = s.download("tmpV")

        run_ranks(rank, nranks)
        del sims, views
    for tag in ("", "_capped"):
        assert np.array_equal(got[tag], z[name + "_tmpV" + tag]), (name, tag)


# ------------------------------------------------------------------ implicit diffusion over ranks (AdvectionDiffusionImplicit, main.cpp:10030-10118)
# KernelAdvect, KernelDiffusionRHS and KernelLHSDiffusion with their inner-then-boundary split -- the Helmholtz tiles' per-component
# domain-face rule has to survive into the second ghost-fill pass (halo_finish restores scalar_bc_dir) -- the k_imp_* passes on rank views,
# and DiffusionSolver::solve with all-reduced totals.  Stencils and the step without iterations: BIT-EXACT against the one-rank oracle /
# tests/implicit_step_restatement.py; solves: the solver-tolerance bounds of tests/test_gpu_amr.py::test_implicit_diffusion_solver (the
# ranks sum the dot products in another association).
IMP_DT, IMP_NU, IMP_UINF = 0.05, 2.0, (0.1, -0.2, 0.3)


class _Spread:
    """One mesh on `nranks` thread ranks (inside a VirtualComm): a uniform grid cut by the library, or a multi-level mesh by rank views of
    the ownership `kind`.  take(r, a): rank r's blocks of an array in the one-rank slot order; gather(parts): back into that order."""

    def __init__(self, name, nranks, kind="ranges", seed=0, **sim_kw):
        self.nranks = nranks
        if name == "uniform222":
            bpd, lmax, level, bc = (2, 2, 2), 2, 1, ("wall", "periodic", "freespace")
            lv, zs = H.uniform_leaves(bpd, lmax, level)
            self.og = O.OracleGrid(bpd, lmax, level, EXT, bc)
        else:
            bpd, lmax, bc, lv, zs = _mesh_case(name)
            level, self.og = 0, None
        self.m = m = O.OracleMesh(bpd, lmax, EXT, bc, lv, zs)
        self.h = np.array([m.h(b) for b in range(m.nb)])
        kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2],
                  nu=IMP_NU, uinf=IMP_UINF, **sim_kw)
        if self.og is not None:
            assert np.array_equal(self.og.tables[:, :5], m.tables[:, :5])
            self.views = None
            self.sims = [cu.SimulationData(rank=r, nranks=nranks, **kw) for r in range(nranks)]
        else:
            mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
            assert np.array_equal(mesh.tables, m.tables)
            owner = _owners(m.nb, nranks, kind, seed=seed)
            self.views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
            self.sims = [cu.SimulationData(view=v, **kw) for v in self.views]
            self.mine = [v.global_slot[:v.nlocal] for v in self.views]
            assert sum(v.nghost for v in self.views) > 0
        assert sum(s.nblocks for s in self.sims) == m.nb
        rng = np.random.default_rng(6)
        self.vel, self.pres, self.rhs = 0.5 * rng.uniform(-1, 1, (m.nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (m.nb, 8, 8, 8)), rng.uniform(-1, 1, (m.nb, 8, 8, 8))

    def take(self, r, a):
        return self.sims[r].grid.to_blocks(self.og.to_global(a)) if self.og is not None else a[self.mine[r]]

    def gather(self, parts):
        if self.og is None:
            out = np.zeros((self.m.nb,) + parts[0].shape[1:])
            for r in range(self.nranks):
                out[self.mine[r]] = parts[r]
            return out
        NX, NY, NZ = self.og.ncell
        g = np.zeros((NZ, NY, NX) + parts[0].shape[4:])
        for r, s in enumerate(self.sims):
            s.grid.scatter_to_global(parts[r], g)
        return self.og.to_blocks(g)

    def not_inner(self, r):
        """one-rank slots of rank r's blocks that wait for the ghost exchange (filled in the second pass)"""
        v = self.views[r]
        inner = np.zeros(max(v.ninner, 1), dtype=np.int32)
        check(lib().cup3d_debug_grid_inner_blocks(v.handle, inner.ctypes.data_as(C.c_void_p)))
        return self.mine[r][np.setdiff1d(np.arange(v.nlocal), inner[:v.ninner])]

    def run(self, fn):
        """fn(rank, sim) -> dict of arrays; returns the gathered dict"""
        out = [None] * self.nranks

        def rank(r):
            out[r] = fn(r, self.sims[r])

        run_ranks(rank, self.nranks)
        return {k: (self.gather([o[k] for o in out]) if isinstance(out[0][k], np.ndarray) else [o[k] for o in out]) for k in out[0]}

    def close(self):
        del self.sims, self.views


def _implicit_stencils(S_):
    def fn(r, s):
        got = {}
        s.upload("vel", S_.take(r, S_.vel))
        check(lib().cup3d_advect_implicit(s.handle, IMP_DT, IMP_NU, np.array(IMP_UINF)))
        got["adv_vel"], got["adv_tmpV"] = s.download("vel"), s.download("tmpV")
        s.upload("vel", S_.take(r, S_.vel))
        check(lib().cup3d_diffusion_rhs(s.handle))
        got["rhs"] = s.download("tmpV")
        for d in range(3):
            s.upload("pres", S_.take(r, S_.pres))
            check(lib().cup3d_diffusion_lhs(s.handle, d, IMP_DT, IMP_NU))
            got[f"lhs{d}"] = s.download("lhs")
        return got

    got = S_.run(fn)
    m = S_.m
    v, t = m.advect_implicit(S_.vel, IMP_DT, IMP_NU, IMP_UINF, False)
    ref = dict(adv_vel=v, adv_tmpV=t, rhs=m.diffusion_rhs(S_.vel), **{f"lhs{d}": m.diff_lhs(S_.pres, d, IMP_DT, IMP_NU) for d in range(3)})
    return got, ref


@pytest.mark.parametrize("nranks,kind", [(2, "ranges"), (3, "scattered"), (5, "ranges")])
@pytest.mark.parametrize("name", ["l012_wall", "l012_periodic", "l012_box322"])
def test_implicit_diffusion_stencils_on_a_multilevel_mesh_over_ranks(name, nranks, kind):
    with VirtualComm(nranks):
        S_ = _Spread(name, nranks, kind, seed=len(name))
        got, ref = _implicit_stencils(S_)
        if name == "l012_wall":
            # the face rule of the component must matter on a block of the SECOND pass (the blocks that wait for the ghost exchange: filled
            # after halo_begin has returned and scalar_bc_dir was reset): else a lost hand-over of the direction would go unseen
            differs = np.where((ref["lhs0"] != ref["lhs1"]).reshape(S_.m.nb, -1).any(axis=1))[0]
            waiting = np.concatenate([S_.not_inner(r) for r in range(nranks)])
            assert len(np.intersect1d(differs, waiting)) > 0, (differs, waiting)
        S_.close()
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (name, nranks, kind, k, np.abs(got[k] - ref[k]).max())


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_implicit_diffusion_stencils_on_a_uniform_grid_over_ranks(nranks):
    """(2,2,2) level 1, wall / periodic / freespace: face slabs instead of ghost blocks"""
    with VirtualComm(nranks):
        S_ = _Spread("uniform222", nranks)
        got, ref = _implicit_stencils(S_)
        S_.close()
    assert not np.array_equal(ref["lhs0"], ref["lhs2"])
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (nranks, k, np.abs(got[k] - ref[k]).max())


def _implicit_step(S_, tol, tol_rel, max_iter=None):
    def fn(r, s):
        s.upload("vel", S_.take(r, S_.vel))
        s.upload("pres", S_.take(r, S_.pres))
        p = cu.capi.PoissonParams()
        lib().cup3d_poisson_default_params(C.byref(p))
        p.tol, p.tol_rel = tol, tol_rel
        if max_iter is not None:
            p.max_iter = max_iter
        res = (cu.capi.PoissonResult * 3)()
        check(lib().cup3d_advect_diffuse_implicit(s.handle, IMP_DT, IMP_NU, np.array(IMP_UINF), C.byref(p), res))
        return dict(vel=s.download("vel"), tmpV=s.download("tmpV"), pres=s.download("pres"), counts=tuple((res[i].iterations, res[i].restarts) for i in range(3)))

    return S_.run(fn)


@pytest.mark.parametrize("name,nranks,kind", [("uniform222", 3, "ranges"), ("l012_wall", 3, "scattered")])
def test_implicit_step_without_iterations_over_ranks_is_the_restated_step(name, nranks, kind):
    """max_iter = 0: every solve returns its zero guess, nothing that depends on the partition enters -- vel, tmpV and pres are the bits of
    tests/implicit_step_restatement.py (k_imp_* on rank views: per-block h of the local slots, component planes of the local blocks)"""
    with VirtualComm(nranks):
        S_ = _Spread(name, nranks, kind, seed=7)
        got = _implicit_step(S_, 0.0, 0.0, max_iter=0)
        S_.close()
    m = S_.m
    want = ST.euler(S_.vel, S_.pres, S_.h, IMP_DT, IMP_NU, lambda v: m.advect_implicit(v, IMP_DT, IMP_NU, IMP_UINF, False), m.diffusion_rhs,
                    lambda rhs, x0, direction: x0.copy())
    assert all(c == ((0, 0),) * 3 for c in got["counts"])
    for k in ("tmpV", "vel", "pres"):
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), (name, k, np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize("name,nranks,kind", [("uniform222", 2, "ranges"), ("uniform222", 3, "ranges"), ("l012_wall", 2, "ranges")])
def test_implicit_step_at_tight_tolerance_over_ranks(name, nranks, kind):
    with VirtualComm(nranks):
        S_ = _Spread(name, nranks, kind, seed=7)
        got = _implicit_step(S_, 1e-12, 1e-11)
        S_.close()
    v, its = S_.m.advdiff_implicit(S_.vel, S_.pres, IMP_DT, IMP_NU, IMP_UINF, False, 1e-12, 1e-11)
    assert len(set(got["counts"])) == 1, got["counts"]          # every rank took the same path through the three solves
    assert all(c[0] > 3 for c in got["counts"][0])
    assert np.array_equal(got["pres"], S_.pres)
    change = np.abs(v - S_.vel).max()
    assert change > 1e-3
    assert np.abs(got["vel"] - v).max() <= 1e-6 * change


def test_diffusion_solve_at_default_tolerance_over_three_ranks():
    """the iterate the sharded Helmholtz solve returns satisfies the reference's stopping rule under the ORACLE's operator on the gathered field"""
    nranks, d = 3, 1
    with VirtualComm(nranks):
        S_ = _Spread("uniform222", nranks)

        def fn(r, s):
            s.upload("lhs", S_.take(r, S_.rhs))
            s.upload("pres", S_.take(r, S_.pres))
            p, res = cu.capi.PoissonParams(), cu.capi.PoissonResult()
            lib().cup3d_poisson_default_params(C.byref(p))
            check(lib().cup3d_diffusion_solve(s.handle, d, IMP_DT, IMP_NU, C.byref(p), C.byref(res)))
            return dict(x=s.download("pres"), its=res.iterations)

        got = S_.run(fn)
        S_.close()
    m = S_.m
    res = np.linalg.norm((S_.rhs - m.diff_lhs(got["x"], d, IMP_DT, IMP_NU)).ravel())
    res0 = np.linalg.norm((S_.rhs - m.diff_lhs(S_.pres, d, IMP_DT, IMP_NU)).ravel())
    assert len(set(got["its"])) == 1 and got["its"][0] >= 2
    assert res <= 1.05 * max(1e-6, 1e-4 * res0), (res, res0)
