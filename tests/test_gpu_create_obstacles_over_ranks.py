"""cup3d_create_obstacles on a grid spread over 2 ranks, on ONE GPU -- the ranks are host threads of this process and the in-process
communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_update_obstacles_over_ranks.py.  MI355X only (-m gpu).

What a block's chi, mass / CoM row and surface points are does not depend on how the mesh is partitioned: each rank's rows must equal, bit
for bit, the rows of the restatement on the GLOBAL mesh (tests/characteristic_cases.py) that belong to its blocks.  The totals are sums of
two rank partials, so they differ from the one-rank totals by the reassociation of the block sum and nothing else: per entry at most
nblocks eps sum_b |block row_b|.  With two ranks the all-reduce is ONE addition, which commutes, so the totals are also known exactly: the
restatement's own pieces, recombined as the ranks combine them, give the centre of mass, the blocks' momenta, the corrections and the
corrected udef bit for bit."""
import gc

import numpy as np
import pytest

import characteristic_cases as CC
import characteristic_restatement as R
import cup3d_amd as cu
import labs_ranks_cases as LC
from cup3d_amd.capi import ObstacleShape, check, lib
from test_gpu_labs_over_ranks import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
NRANKS = 2


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def ranks_of(name):
    """(case, owner [nb], make_sims) -- call make_sims() inside VirtualComm"""
    c = CC.case(name)
    if c.leaves is None:
        mesh, owner = cu.operators.uniform_share_mesh(c.bpd, c.lmax, c.sim_kwargs["levelStart"], CC.EXT, c.bc, NRANKS)

        def make_sims():
            return [cu.SimulationData(rank=r, nranks=NRANKS, **c.sim_kwargs) for r in range(NRANKS)], None
    else:
        mesh = cu.operators.Grid(c.bpd, c.lmax, 0, CC.EXT, c.bc, leaves=c.leaves)
        assert np.array_equal(mesh.tables, c.tables)
        owner = LC.owners(c.nb, "ranges", NRANKS, 0)

        def make_sims():
            views = [mesh.rank_view(owner, r, NRANKS) for r in range(NRANKS)]
            kw = {k: v for k, v in c.sim_kwargs.items() if k != "leaves"}
            return [cu.SimulationData(view=views[r], **kw) for r in range(NRANKS)], views
    assert np.array_equal(mesh.geom, c.geom)
    return c, owner, make_sims


def share(o, owner, r):
    """rank r's part of obstacle o: the blocks it owns, in the obstacle's order, with LOCAL slots; `keep` = their positions in o"""
    local = {int(g): i for i, g in enumerate(np.where(owner == r)[0])}
    keep = [i for i, g in enumerate(o["ids"]) if owner[g] == r]
    return cu.ObstacleShape([local[int(o["ids"][i])] for i in keep], o["sdf"][keep].reshape(len(keep), 10, 10, 10),
                            o["udef"][keep].reshape(len(keep), 8, 8, 8, 3), o["transvel_correction"]), keep


def recombined(c, o, r, keeps):
    """the restatement's pieces for obstacle o (r: its Result on the global mesh) combined as two ranks combine them"""
    ids = [int(b) for b in o["ids"]]
    com = np.zeros(4)
    for keep in keeps:   # each rank: its rows in slot order; then one addition
        com = com + np.array(R.grid_com([r.block_com[i].tolist() for i in keep], [ids[i] for i in keep]))
    CM = [com[1] / com[0], com[2] / com[0], com[3] / com[0]]
    old = [float(v) for v in o["transvel_correction"]]
    rows = [R.udef_momenta(r.chi[i].tolist(), o["udef"][i], c.geom[b, 0], c.geom[b, 1:4], CM, old) for i, b in enumerate(ids)]
    M = np.zeros(13)
    for keep in keeps:
        M = M + np.array(R.momenta_totals([rows[i] for i in keep], [ids[i] for i in keep]))
    mass, tv, J, av = R.accumulate(M.tolist())
    udef = np.array([R.remove(o["udef"][i], c.geom[b, 0], c.geom[b, 1:4], CM, tv, av) for i, b in enumerate(ids)])
    return dict(com_totals=com, cm=np.array(CM), block_momenta=np.array(rows), udef_totals=M, mass=mass, transvel_correction=np.array(tv), J=np.array(J),
                angvel_correction=np.array(av), udef=udef)


@pytest.mark.parametrize("name", ["uniform8", "amr_periodic_l01"])
def test_rows_per_rank_and_totals_over_ranks(name):
    c, owner, make_sims = ranks_of(name)
    a, b = c.obstacles
    assert set(owner[a["ids"]].tolist()) == {0, 1}          # both obstacles lie on both sides of the rank boundary
    only1 = [i for i, g in enumerate(a["ids"]) if owner[g] == 1]
    third = dict(a, ids=a["ids"][only1], sdf=a["sdf"][only1], udef=a["udef"][only1])   # ... and rank 0 holds none of this one's blocks
    obstacles = [a, b, third]
    _, (want_third,) = R.create(c.geom, c.nb, [third])
    want_field, want_all = R.create(c.geom, c.nb, obstacles)
    got = [None] * NRANKS
    fields = [None] * NRANKS
    with VirtualComm(NRANKS):
        sims, views = make_sims()
        rng = np.random.default_rng(3)
        vel = rng.uniform(-1, 1, (c.nb, 8, 8, 8, 3))
        for r, s in enumerate(sims):
            s.upload("vel", vel[owner == r])
            s.fill("chi", 0.7)
            s.shapes = [share(o, owner, r)[0] for o in obstacles]
        assert len(sims[0].shapes[2].slots) == 0 and len(sims[1].shapes[2].slots) > 0
        before = [s.checksum("vel") for s in sims]

        def rank(r):
            cu.CreateObstacles(sims[r])(0.0)
            got[r] = sims[r].shapes
            fields[r] = sims[r].download("chi")

        run_ranks(rank, NRANKS)
        assert [s.checksum("vel") for s in sims] == before
        del sims, views
        gc.collect()
    for r in range(NRANKS):
        assert np.array_equal(fields[r], want_field[owner == r]), f"rank {r}: the resident chi differs from the global restatement's"
    for k, (o, w) in enumerate(zip(obstacles, want_all)):
        keeps = [share(o, owner, r)[1] for r in range(NRANKS)]
        x = recombined(c, o, w, keeps)
        for r, keep in enumerate(keeps):
            g = got[r][k]
            what = f"obstacle {k}, rank {r}"
            assert np.array_equal(g.chi, w.chi[keep]) and np.array_equal(g.block_com, w.block_com[keep]), what
            assert np.array_equal(np.diff(g.first), np.diff(w.first)[keep]), what
            pts = np.concatenate([np.arange(w.first[i], w.first[i + 1]) for i in keep]).astype(int) if keep else np.zeros(0, dtype=int)
            assert np.array_equal(g.ijk, w.ijk[pts]) and np.array_equal(g.dchi, w.dchi[pts]) and np.array_equal(g.delta, w.delta[pts]), what
            assert np.array_equal(g.block_momenta, x["block_momenta"][keep]), what
            assert np.array_equal(g.udef_corrected, x["udef"][keep]), what
            for f in ("com_totals", "cm", "udef_totals", "mass", "J", "transvel_correction", "angvel_correction"):
                assert np.array_equal(getattr(g, f), x[f]), (what, f)   # the same bits on both ranks
        # against the one-rank restatement: the reassociation of the block sum and nothing else
        n, eps = len(o["ids"]), np.finfo(float).eps
        d = np.abs(got[0][k].com_totals - w.com_totals)
        assert (d <= n * eps * np.abs(w.block_com).sum(axis=0)).all(), f"obstacle {k}: com totals off by {d.max():.3g}"
        # the momenta see the centre of mass move by that much as well: rows are bounded by M[0] max|udef| (1 + |p|^2), a loose scale
        scale = w.mass * (1 + np.abs(o["udef"]).max()) * (1 + (2 * CC.EXT) ** 2)
        d = np.abs(got[0][k].udef_totals - w.udef_totals)
        assert (d <= 8 * n * eps * scale).all(), f"obstacle {k}: momenta totals off by {d.max():.3g}"
    assert np.array_equal(got[1][2].chi, want_third.chi)


def test_a_bad_slot_on_one_rank_is_an_error_on_both():
    """rank 1 lists a slot it does not have: it returns CUP3D_EINVAL, rank 0 an error at the first all-reduce, nothing of the caller's is
    written on either, and neither is left waiting for the other"""
    c, owner, make_sims = ranks_of("uniform8")
    a = c.obstacles[0]
    status, untouched = [None] * NRANKS, [None] * NRANKS
    with VirtualComm(NRANKS):
        sims, _ = make_sims()
        parts = [share(a, owner, r)[0] for r in range(NRANKS)]
        parts[1].slots[-1] = sims[1].nblocks

        def rank(r):
            p = parts[r]
            n = len(p.slots)
            arr = (ObstacleShape * 1)()
            w = dict(udef=p.udef.copy(), chi=np.full((n, 8, 8, 8), 7.0), first=np.full(n + 1, 7, dtype=np.int32), ijk=np.full((512 * n, 3), 7, dtype=np.int32),
                     dchi=np.full((512 * n, 3), 7.0), delta=np.full(512 * n, 7.0), block_com=np.full((n, 4), 7.0), block_momenta=np.full((n, 13), 7.0))
            arr[0].nblocks, arr[0].slots, arr[0].sdf = n, p.slots.ctypes.data, p.sdf.ctypes.data
            for k, v in w.items():
                setattr(arr[0], k, v.ctypes.data)
            for q in range(4):
                arr[0].com_totals[q] = 5.0
            status[r] = lib().cup3d_create_obstacles(sims[r].handle, 1, arr)
            untouched[r] = all((w[k] == 7).all() for k in w if k != "udef") and np.array_equal(w["udef"], p.udef) and list(arr[0].com_totals) == [5.0] * 4

        run_ranks(rank, NRANKS)
        check(lib().cup3d_device_synchronize())
        del sims
        gc.collect()
    assert status[1] == -1 and status[0] == -4   # CUP3D_EINVAL where the slot is bad, CUP3D_ECOMM on the partner
    assert all(untouched)
