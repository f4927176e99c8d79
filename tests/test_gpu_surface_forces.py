"""cup3d_compute_forces: KernelComputeForces::visit (main.cpp:12273-12493) on the device (k_surface_forces, csrc/obstacles_forces.hip) against its
plain-Python restatement (tests/surface_forces_restatement.py) evaluated on the CPU oracle's [-4,5) tiles.  The inputs are those of
tests/surface_forces_cases.py, which tests/test_surface_forces_cases.py shows to take every path of the functor.  MI355X only (-m gpu).

Everything is bit-exact (np.array_equal): the per-point arrays, and the block sums, which the kernel adds in the reference's point order."""
import ctypes as C
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import oracle_lib as O
import surface_forces_cases as SC
from cup3d_amd.capi import ObstacleSurface, RunStats, check, lib

pytestmark = pytest.mark.gpu
EINVAL = -1
_sims = {}


def surfaces_of(e):
    return [cu.ObstacleSurface(o["slots"], o["first"], o["ijk"], o["dchi"], o["udef"], o["cm"], o["vel"], o["omega"], o["qoi"]) for o in e.obstacles]


def case(name):
    """(expected, sim with the seeded vel / chi / pres uploaded), built once per mesh; the fields are never modified"""
    if name not in _sims:
        e = SC.expected(name)
        kw = dict(levelStart=e.level) if e.level is not None else dict(levelStart=0, leaves=e.leaves)
        sim = cu.SimulationData(**e.sim_kwargs(), **kw)
        assert np.array_equal(sim.grid.tables, e.m.tables)   # same blocks in the same order on both sides
        for f in ("vel", "chi", "pres"):
            sim.upload(f, getattr(e, f))
        _sims[name] = (e, sim)
    return _sims[name]


def same(got, want, what):
    for k, ((gp, gq), (wp, wq)) in enumerate(zip(got, want)):
        bad = gp != wp
        assert not bad.any(), f"{what}, obstacle {k}: points differ in arrays {sorted(set(np.where(bad)[0].tolist()))}, max |d| = {np.abs(gp - wp).max():.3g}"
        bad = gq != wq
        assert not bad.any(), f"{what}, obstacle {k}: block sums differ in {sorted(set(np.where(bad)[1].tolist()))}, max |d| = {np.abs(gq - wq).max():.3g}"
        assert np.array_equal(gp, wp) and np.array_equal(gq, wq)


@pytest.mark.parametrize("name", SC.SINGLE_RANK)
def test_points_and_sums_equal_the_restatement(name):
    e, sim = case(name)
    if name in SC.GOLDEN:
        assert len(set(e.hs.tolist())) >= 2
    before = tuple(sim.checksum(f) for f in ("vel", "chi", "pres"))
    sim.surfaces = surfaces_of(e)
    st = RunStats()
    check(lib().cup3d_stats_reset())
    first = cu.ComputeForces(sim)(0)
    check(lib().cup3d_stats_read(C.byref(st)))
    same(first, e.first_call, (name, "first call"))
    assert st.field_bytes_downloaded == sum((len(o["ijk"]) + len(o["slots"])) * 19 * 8 for o in e.obstacles)   # points and sums, nothing else
    # the second call starts from the sums the first returned: eight accumulate, eleven restart (12283-12293)
    second = cu.ComputeForces(sim)(0)
    same(second, e.second_call, (name, "second call"))
    assert not np.array_equal(second[0][1], first[0][1])
    assert tuple(sim.checksum(f) for f in ("vel", "chi", "pres")) == before   # the fields are only read


def test_two_obstacles_sharing_a_block_get_their_own_results():
    e, sim = case("box222_wall")
    a, b = surfaces_of(e)
    shared = set(a.slots.tolist()) & set(b.slots.tolist())
    assert shared
    sim.surfaces = [b]
    alone = cu.ComputeForces(sim)(0)
    same(alone, e.first_call[1:], "obstacle B alone")
    sim.surfaces = [surfaces_of(e)[1], surfaces_of(e)[0]]   # the other order
    swapped = cu.ComputeForces(sim)(0)
    same(swapped, e.first_call[::-1], "B before A")
    ia, ib = a.slots.tolist().index(min(shared)), b.slots.tolist().index(min(shared))
    assert not np.array_equal(e.first_call[0][1][ia], e.first_call[1][1][ib])


def test_slot_lists_longer_than_one_scratch_chunk():
    """the tile scratch holds a bounded number of blocks; `forces_chunk` (testing library) makes that bound 2, so that the 5 blocks of
    obstacle A go through it in three rounds -- and the scratch is part of cup3d_sim_device_bytes"""
    e = SC.expected("amr_mixed_l12")
    sim = cu.SimulationData(**e.sim_kwargs(), levelStart=0, leaves=e.leaves)
    for f in ("vel", "chi", "pres"):
        sim.upload(f, getattr(e, f))
    check(lib().cup3d_debug_set_option(b"forces_chunk", 2))
    try:
        bytes0 = sim.device_bytes()
        sim.surfaces = surfaces_of(e)
        same(cu.ComputeForces(sim)(0), e.first_call, "chunks of 2 blocks")
        grown = sim.device_bytes() - bytes0
        assert grown >= 2 * 131072                 # two blocks' vel and chi tiles ...
        assert grown < 5 * 131072 + (4 << 20)      # ... and not five (the staged arrays and the tables of cup3d_sim_labs are small)
        same(cu.ComputeForces(sim)(0), e.second_call, "chunks of 2 blocks, second call")
        assert sim.device_bytes() - bytes0 == grown   # grow-only, and nothing grew
    finally:
        check(lib().cup3d_debug_set_option(b"forces_chunk", 0))
    del sim
    gc.collect()


def _struct(o, points, qoi, **override):
    a = ObstacleSurface()
    arrs = dict(slots=o.slots, first=o.first, ijk=o.ijk, dchi=o.dchi, udef=o.udef)
    arrs.update(override)
    a.nblocks = override.get("nblocks", len(o.slots))
    for k in ("slots", "first", "ijk", "dchi", "udef"):
        setattr(a, k, None if arrs[k] is None else arrs[k].ctypes.data)
    a.points = None if override.get("null_points") else points.ctypes.data
    a.qoi = None if override.get("null_qoi") else qoi.ctypes.data
    for d in range(3):
        a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]
    return a, arrs   # arrs keeps the overridden arrays alive


def test_refused_calls_touch_nothing():
    e, sim = case("box222_wall")
    good, other = surfaces_of(e)
    n, npts = len(good.slots), len(good.ijk)
    bad_slot_hi, bad_slot_lo = good.slots.copy(), good.slots.copy()
    bad_slot_hi[2], bad_slot_lo[0] = e.nb, -1
    first_from_1, first_down = good.first.copy(), good.first.copy()
    first_from_1[0] = 1
    first_down[2] = first_down[1] - 1
    ijk_hi, ijk_lo = good.ijk.copy(), good.ijk.copy()
    ijk_hi[npts - 1, 2], ijk_lo[0, 0] = 8, -1
    cases = [dict(slots=None), dict(first=None), dict(ijk=None), dict(dchi=None), dict(udef=None), dict(slots=bad_slot_hi), dict(slots=bad_slot_lo),
             dict(first=first_from_1), dict(first=first_down), dict(ijk=ijk_hi), dict(ijk=ijk_lo), dict(nblocks=-1),
             dict(null_points=True), dict(null_qoi=True)]
    for ov in cases:
        # a good obstacle first: nothing of it may be written either when the second one is refused
        pts = [np.full((19, npts), 5.0), np.full((19, len(other.ijk)), 5.0)]
        qoi = [np.full((n, 19), 6.0), np.full((len(other.slots), 19), 6.0)]
        arr = (ObstacleSurface * 2)()
        arr[0], _ = _struct(other, pts[1], qoi[1])
        arr[1], keep = _struct(good, pts[0], qoi[0], **ov)
        check(lib().cup3d_sim_fill(sim.handle, cu.operators.FIELDS["lhs"], 0.0))   # a successful call in between: the error text is this call's own
        assert lib().cup3d_compute_forces(sim.handle, SC.NU, 2, arr) == EINVAL, ov.keys()
        assert len(lib().cup3d_last_error()) > 0
        check(lib().cup3d_device_synchronize())
        assert all((p == 5.0).all() for p in pts) and all((q == 6.0).all() for q in qoi), ov.keys()
    arr = (ObstacleSurface * 1)()
    arr[0], _ = _struct(good, np.zeros((19, npts)), np.zeros((n, 19)))
    assert lib().cup3d_compute_forces(None, SC.NU, 1, arr) == EINVAL
    assert lib().cup3d_compute_forces(sim.handle, SC.NU, 1, None) == EINVAL
    assert lib().cup3d_compute_forces(sim.handle, SC.NU, -1, arr) == EINVAL


def test_nothing_to_do_is_not_an_error():
    e, sim = case("box222_wall")
    assert lib().cup3d_compute_forces(sim.handle, SC.NU, 0, None) == 0
    sim.surfaces = []
    assert cu.ComputeForces(sim)(0) == []
    empty = cu.ObstacleSurface([], [0], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 8, 8, 8, 3)), (0, 0, 0), (0, 0, 0), (0, 0, 0))
    sim.surfaces = [empty, surfaces_of(e)[0]]
    out = cu.ComputeForces(sim)(0)
    assert out[0][0].shape == (19, 0) and out[0][1].shape == (0, 19)
    same(out[1:], e.first_call[:1], "after an obstacle without blocks")
    # a block whose point list is empty between two that have points: its sums are the eleven zeroes and the eight it came with
    o = e.obstacles[1]
    first = np.array([0, o["first"][1], o["first"][1], o["first"][2]], dtype=np.int32)
    slots = np.array([o["slots"][0], o["slots"][1], o["slots"][1]], dtype=np.int32)
    udef = o["udef"][[0, 1, 1]]
    qoi = np.concatenate([o["qoi"][:1], np.full((1, 19), 3.0), o["qoi"][1:]])
    sim.surfaces = [cu.ObstacleSurface(slots, first, o["ijk"], o["dchi"], udef, o["cm"], o["vel"], o["omega"], qoi)]
    (points, got), = cu.ComputeForces(sim)(0)
    assert np.array_equal(points, e.first_call[1][0]) and np.array_equal(got[[0, 2]], e.first_call[1][1])
    import surface_forces_restatement as R
    carried = [R.QOI_NAMES.index(k) for k in R.CARRIED]
    assert (got[1, carried] == 3.0).all() and (np.delete(got[1], carried) == 0.0).all()


def test_rank_view_is_refused():
    """the single-rank entry on a sim whose neighbours live on another rank says so instead of returning wrong numbers"""
    bpd, lmax, bc = (2, 2, 2), 3, ("wall", "freespace", "wall")
    lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 0, 0, 0), (1, 0, 0, 0)])
    mesh = cu.operators.Grid(bpd, lmax, 0, SC.EXT, bc, leaves=(lv, zs))
    owner = (np.arange(mesh.nblocks) * 2 // mesh.nblocks).astype(np.int32)
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=SC.EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    o = SC.make_obstacles(4, 1)[1]
    check(lib().cup3d_debug_virtual_comm(2))   # the in-process communicator of test_gpu_multirank.py: two ranks on one device
    try:
        views = [mesh.rank_view(owner, r, 2) for r in range(2)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(2)]
        assert min(v.nlocal for v in views) >= 4
        points, qoi = np.full((19, len(o["ijk"])), 5.0), np.full((2, 19), 6.0)
        s = cu.ObstacleSurface(o["slots"], o["first"], o["ijk"], o["dchi"], o["udef"], o["cm"], o["vel"], o["omega"])
        arr = (ObstacleSurface * 1)()
        arr[0], _ = _struct(s, points, qoi)
        assert lib().cup3d_compute_forces(sims[0].handle, SC.NU, 1, arr) == EINVAL
        assert b"rank" in lib().cup3d_last_error()
        assert (points == 5.0).all() and (qoi == 6.0).all()
        del sims
        gc.collect()
    finally:
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)


def test_one_ranks_share_of_a_uniform_grid_is_refused():
    """... and so is the single-rank entry on one rank's share of a uniform grid: EINVAL before anything is staged, nothing written"""
    e = SC.expected("uniform64")
    o = e.obstacles[1]
    check(lib().cup3d_debug_virtual_comm(2))
    try:
        sims = [cu.SimulationData(rank=r, nranks=2, levelStart=e.level, **e.sim_kwargs()) for r in range(2)]
        assert all(s.nblocks == 32 for s in sims)
        for sim in sims:
            bytes0 = sim.device_bytes()
            points, qoi = np.full((19, len(o["ijk"])), 5.0), np.full((len(o["slots"]), 19), 6.0)
            s = cu.ObstacleSurface(o["slots"] % 32, o["first"], o["ijk"], o["dchi"], o["udef"], o["cm"], o["vel"], o["omega"])
            arr = (ObstacleSurface * 1)()
            arr[0], _ = _struct(s, points, qoi)
            assert lib().cup3d_compute_forces(sim.handle, SC.NU, 1, arr) == EINVAL
            assert b"rank" in lib().cup3d_last_error()
            check(lib().cup3d_device_synchronize())
            assert (points == 5.0).all() and (qoi == 6.0).all()
            assert sim.device_bytes() == bytes0   # refused before the scratch or the staged arrays were allocated
        del sims
        gc.collect()
    finally:
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)


def test_a_normal_that_is_not_a_number_stays_inside_the_tile():
    """A zero dchi makes the unit normal NaN.  The reference's round() of it is undefined (and the restatement has no answer for it); the
    kernel clamps the rounded step, so the march of such a point takes no step at all and every read stays inside the tile.  Its
    neighbours in the block are evaluated as if it were not there, its own copies (position, P, v, vDef) are exact, the six forces per
    unit area, which use the unit normal, are NaN, and the vorticity and the block's sums, which do not, are finite."""
    e, sim = case("box222_wall")
    o = e.obstacles[1]
    mid = int(o["first"][0]) + 7
    dchi = o["dchi"].copy()
    dchi[mid] = 0.0
    sim.surfaces = [cu.ObstacleSurface(o["slots"], o["first"], o["ijk"], dchi, o["udef"], o["cm"], o["vel"], o["omega"], o["qoi"])]
    (points, qoi), = cu.ComputeForces(sim)(0)
    want_p, want_q = e.first_call[1]
    others = np.arange(points.shape[1]) != mid
    assert np.array_equal(points[:, others], want_p[:, others])
    copies = [0, 1, 2, 3, 13, 14, 15, 16, 17, 18]   # pX pY pZ P vxDef vX vyDef vY vzDef vZ
    assert np.array_equal(points[copies, mid], want_p[copies, mid])
    assert np.isnan(points[4:10, mid]).all()         # fX fY fZ fxV fyV fzV
    assert np.isfinite(points[10:13, mid]).all()     # omegaX omegaY omegaZ
    assert np.array_equal(qoi[1], want_q[1])         # the other block of the obstacle
    assert np.isfinite(qoi[0]).all() and not np.array_equal(qoi[0], want_q[0])
