"""cup3d_compute_forces_resident -- ComputeForces with Obstacle::computeForces on the blocks cup3d_create_obstacles keeps on the
device (k_retained_surface, csrc/obstacles_create.hip; k_surface_forces_set, csrc/obstacles_forces.hip) -- against the staged
cup3d_compute_forces on the surface list and corrected udef that cup3d_create_obstacles returned to the host.  MI355X only (-m gpu).

Two sims per mesh: both run CreateObstacles, the twin then runs the staged call on shape.surface(vel, omega).  Everything is bit-exact
(np.array_equal): the kernels share their body, the rebuilt ijk / dchi come from the statements that made the staged ones (the 19 point
arrays pin them: positions, normals and everything derived), and the totals are the rows added in ascending slot order
(tests/resident_forces_cases.py)."""
import ctypes as C
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import resident_forces_cases as FC
from cup3d_amd.capi import ObstacleForces, RunStats, check, lib

pytestmark = pytest.mark.gpu
K, RC = FC.K, FC.RC
EINVAL, ESTATE = -1, -5
TILE_BYTES = (16 ** 3) * 4 * 8   # one block's vel and chi tiles in the scratch
FIELDS = ("vel", "chi", "pres")
_sims = {}


def sims_of(name):
    """(staged, resident): two sims of the mesh"""
    if name not in _sims:
        c = K.CC.case(name)
        _sims[name] = tuple(cu.SimulationData(**c.sim_kwargs) for _ in range(2))
    return _sims[name]


def shape_of(o, reverse=False):
    s = slice(None, None, -1) if reverse else slice(None)
    return cu.ObstacleShape(o["ids"][s], o["sdf"][s], o["udef"][s], o["transvel_correction"])


def create(sim, name, keys, reverse_first=False):
    """vel and pres uploaded, CreateObstacles for the set, sim.obstacles in the set's rigid state, the staged surfaces with zero sums"""
    obs = K.obstacles(name)
    sim.upload("vel", FC.vel_of(name))
    sim.upload("pres", FC.pres_of(name))
    sim.nu = FC.NU
    sim.shapes, sim.obstacles = [shape_of(obs[k], reverse_first and n == 0) for n, k in enumerate(keys)], []
    cu.CreateObstacles(sim)(0.0)
    sim.obstacles = [s.data(K.APPROACH[k]["vel"], K.APPROACH[k]["omega"]) for s, k in zip(sim.shapes, keys)]
    sim.surfaces = [s.surface(o.vel, o.omega) for s, o in zip(sim.shapes, sim.obstacles)]


def warm_tiles(sim):
    """the tables of cup3d_sim_labs_device are built by the first tile a sim is asked for and counted from then on: ask for one (a
    [-1,2) chi tile of block 0, written over the start of lhs, which nothing here reads) so that the byte counts below are the call's own"""
    ptr = C.c_void_p()
    check(lib().cup3d_sim_device_ptr(sim.handle, cu.operators.FIELDS["lhs"], C.byref(ptr)))
    sim.labs_into(ptr.value, "chi", 1, tensorial=True, slots=np.zeros(1, dtype=np.int32))


def counted(op):
    """(what op returns, field bytes it brought down); it takes none up"""
    st = RunStats()
    check(lib().cup3d_stats_reset())
    out = op()
    check(lib().cup3d_stats_read(C.byref(st)))
    assert st.field_bytes_uploaded == 0
    return out, int(st.field_bytes_downloaded)


def staged_call(sim):
    sim.resident_obstacles = False
    return cu.ComputeForces(sim)(0.0)


def resident_call(sim):
    sim.resident_obstacles = True
    try:
        return cu.ComputeForces(sim)(0.0)
    finally:
        sim.resident_obstacles = False


def same(got, want, what):
    assert len(got) == len(want)
    for k, ((gp, gq), (wp, wq)) in enumerate(zip(got, want)):
        assert gp.shape == wp.shape and gq.shape == wq.shape, (what, k, gp.shape, wp.shape, gq.shape, wq.shape)
        bad = gp != wp
        assert not bad.any(), f"{what}, obstacle {k}: points differ in arrays {sorted(set(np.where(bad)[0].tolist()))}, max |d| = {np.abs(gp - wp).max():.3g}"
        bad = gq != wq
        assert not bad.any(), f"{what}, obstacle {k}: block sums differ in {sorted(set(np.where(bad)[1].tolist()))}, max |d| = {np.abs(gq - wq).max():.3g}"
        assert np.array_equal(gp, wp) and np.array_equal(gq, wq)


def totals_follow(sim, rows, what):
    """every ObstacleData holds the sums of `rows` [(points, qoi)] in ascending slot order and what 13089-13114 make of them"""
    for k, (o, surf, (_, qoi)) in enumerate(zip(sim.obstacles, sim.surfaces, rows)):
        t = FC.totals(qoi, surf.slots)
        assert np.array_equal(o.force_totals, t), (what, k, np.abs(o.force_totals - t).max())
        assert np.abs(t).max() > 0
        assert np.array_equal(np.concatenate([o.surf_force, o.pres_force, o.visc_force, o.surf_torque]), t[:12])
        assert (o.drag, o.thrust, o.Pout, o.PoutBnd, o.defPower, o.defPowerBnd, o.pLocom) == tuple(t[12:])
        assert (o.Pthrust, o.Pdrag, o.EffPDef, o.EffPDefBnd) == tuple(float(v) for v in FC.derived(t, o.vel)), (what, k)


def lists(sim):
    return [s.first for s in sim.shapes], [s.slots for s in sim.shapes]


@pytest.mark.parametrize("name", FC.NAMES)
@pytest.mark.parametrize("keys", list(FC.SETS))
def test_the_resident_call_equals_the_staged_one_twice(name, keys):
    staged, _ = sims_of(name)
    resident = cu.SimulationData(**K.CC.case(name).sim_kwargs)   # a sim of its own: the scratch only grows, and its bytes are counted below
    create(staged, name, keys)
    create(resident, name, keys)
    warm_tiles(resident)
    want1 = staged_call(staged)
    want2 = staged_call(staged)   # from the sums the first call left in the surfaces
    assert not np.array_equal(want2[0][1], want1[0][1])   # the eight carried sums moved ...
    carried = np.array([1, 2, 4, 5, 7, 8, 15, 17])
    assert np.array_equal(np.delete(want2[0][1], carried, axis=1), np.delete(want1[0][1], carried, axis=1))   # ... the eleven restarted
    plan = FC.surface_plan(*lists(resident))
    rows, tiles, points = len(plan["row_obst"]), len(plan["tile_slots"]), int(plan["row_first"][-1])
    assert tiles < rows and [len(q) for _, q in want1] == np.diff(plan["row_base"]).tolist()
    before = tuple(resident.checksum(f) for f in FIELDS)
    bytes0 = resident.device_bytes()
    got1, down = counted(lambda: resident_call(resident))
    same(got1, want1, (name, keys, "first call"))
    totals_follow(resident, want1, (name, keys, "first call"))
    assert down == (rows + points) * 19 * 8   # the rows once, the points once
    # the surface plan, the plan of the resident operators (none of them has run), the tiles of every distinct slot and the points
    grown = resident.device_bytes() - bytes0
    assert grown == FC.surface_plan_bytes(*lists(resident)) + RC.plan_bytes(lists(resident)[1]) + tiles * TILE_BYTES + points * 19 * 8, grown
    got2, down = counted(lambda: resident_call(resident))
    same(got2, want2, (name, keys, "second call"))
    totals_follow(resident, want2, (name, keys, "second call"))
    assert down == (rows + points) * 19 * 8 and resident.device_bytes() - bytes0 == grown   # nothing grows
    assert tuple(resident.checksum(f) for f in FIELDS) == before   # the fields are only read
    del resident
    gc.collect()


@pytest.mark.parametrize("name", FC.NAMES)
def test_rows_follow_the_listed_order_and_totals_do_not(name):
    """with A's list reversed its rows and points come back in that order, as the staged call returns them for the reversed list, and
    the totals are those of the list as it was: rows are added in ascending slot order"""
    staged, resident = sims_of(name)
    create(staged, name, "ABC")
    straight = staged_call(staged)
    create(staged, name, "ABC", reverse_first=True)
    create(resident, name, "ABC", reverse_first=True)
    assert list(resident.shapes[0].slots) == sorted(resident.shapes[0].slots, reverse=True)
    want = staged_call(staged)
    got = resident_call(resident)
    same(got, want, (name, "A reversed"))
    assert np.array_equal(want[0][1], straight[0][1][::-1]) and len(want[0][1]) > 1
    totals_follow(resident, want, (name, "A reversed"))
    for k, (o, (_, qoi)) in enumerate(zip(resident.obstacles, straight)):
        slots = np.sort(resident.surfaces[k].slots) if k == 0 else resident.surfaces[k].slots
        assert np.array_equal(o.force_totals, FC.totals(qoi, slots)), k


def test_a_new_set_restarts_the_sums_and_replaces_the_plan():
    staged, resident = sims_of("uniform8")
    create(resident, "uniform8", "ABC")
    resident_call(resident)   # the grow-only scratch is as large as it gets here
    create(resident, "uniform8", "AB")
    resident_call(resident)
    resident_call(resident)   # the carried sums of A, B have moved twice
    base = resident.device_bytes() - FC.surface_plan_bytes(*lists(resident)) - RC.plan_bytes(lists(resident)[1])
    create(staged, "uniform8", "ABC")
    want1, want2 = staged_call(staged), staged_call(staged)
    create(resident, "uniform8", "ABC")
    nb = resident.nblocks
    assert resident.device_bytes() == base + 24420 * nb   # the old set went with both plans; C's blocks came; no new plan yet
    same(resident_call(resident), want1, "AB twice, then ABC: the sums restart from zero")
    assert resident.device_bytes() == base + 24420 * nb + FC.surface_plan_bytes(*lists(resident)) + RC.plan_bytes(lists(resident)[1])
    same(resident_call(resident), want2, "ABC, second call")
    # a resident operator first: the forces call then adds the surface plan alone
    create(resident, "uniform8", "ABC")
    resident.lambda_penal, resident.bImplicitPenalization, resident.resident_obstacles = RC.LAMBDA, False, True
    cu.UpdateObstacles(resident)(RC.DT)
    resident.resident_obstacles = False
    for o, k in zip(resident.obstacles, "ABC"):
        o.vel, o.omega = np.array(K.APPROACH[k]["vel"]), np.array(K.APPROACH[k]["omega"])
    bytes0 = resident.device_bytes()
    same(resident_call(resident), want1, "after UpdateObstacles built the other plan")
    assert resident.device_bytes() - bytes0 == FC.surface_plan_bytes(*lists(resident))
    # a refused cup3d_create_obstacles drops the set and both plans
    assert lib().cup3d_create_obstacles(resident.handle, -1, None) == EINVAL
    assert resident.device_bytes() == base - 2 * 24420 * nb
    arr = (ObstacleForces * 3)()
    assert lib().cup3d_compute_forces_resident(resident.handle, FC.NU, 3, arr) == ESTATE


def test_chunks_of_two_tiles_give_the_same_bits():
    """`forces_chunk` (testing library) makes the scratch hold 2 tiles, so that the 8 distinct slots go through it in four chunks, each
    one launch over a contiguous range of the slot-major schedule -- and a fresh sim's scratch is those 2 tiles"""
    name = "amr_periodic_l01"
    staged, _ = sims_of(name)
    create(staged, name, "ABC")
    want1, want2 = staged_call(staged), staged_call(staged)
    sim = cu.SimulationData(**K.CC.case(name).sim_kwargs)
    create(sim, name, "ABC")
    warm_tiles(sim)
    plan = FC.surface_plan(*lists(sim))
    assert len(plan["tile_slots"]) == 8 and len(plan["row_obst"]) == 16
    check(lib().cup3d_debug_set_option(b"forces_chunk", 2))
    try:
        bytes0 = sim.device_bytes()
        same(resident_call(sim), want1, "chunks of 2 tiles")
        points = int(plan["row_first"][-1])
        assert sim.device_bytes() - bytes0 == FC.surface_plan_bytes(*lists(sim)) + RC.plan_bytes(lists(sim)[1]) + 2 * TILE_BYTES + points * 19 * 8
        same(resident_call(sim), want2, "chunks of 2 tiles, second call")
    finally:
        check(lib().cup3d_debug_set_option(b"forces_chunk", 0))
    del sim
    gc.collect()


def raw(sim, n, *, handle=True, null_array=False, nobst=None, points=True, qoi=True):
    """the entry point on pre-filled structs; returns (rc, nothing of the caller's written?)"""
    arr = (ObstacleForces * max(1, n))()
    pts, rows = np.full((max(1, n), 19 * 4096), 5.0), np.full((max(1, n), 64 * 19), 6.0)   # room for any sphere of the cases
    for k in range(max(1, n)):
        for d in range(3):
            arr[k].cm[d], arr[k].vel[d], arr[k].omega[d] = 3.0 + 0.1 * d, 0.25, 0.125
        for q in range(19):
            arr[k].totals[q] = 7.0
        arr[k].Pthrust = arr[k].Pdrag = arr[k].EffPDef = arr[k].EffPDefBnd = 7.0
        arr[k].points = pts[k].ctypes.data if points else None
        arr[k].qoi = rows[k].ctypes.data if qoi else None
    image = bytes(arr)
    rc = lib().cup3d_compute_forces_resident(sim.handle if handle else None, FC.NU, n if nobst is None else nobst, None if null_array else arr)
    check(lib().cup3d_device_synchronize())
    return rc, bytes(arr) == image and bool((pts == 5.0).all()) and bool((rows == 6.0).all())


def test_refused_calls_touch_nothing():
    c = K.CC.case("uniform8")
    fresh = cu.SimulationData(**c.sim_kwargs)
    assert raw(fresh, 2) == (ESTATE, True)   # no cup3d_create_obstacles yet
    assert b"cup3d_create_obstacles" in lib().cup3d_last_error()
    _, sim = sims_of("uniform8")
    create(sim, "uniform8", "AB")
    before = tuple(sim.checksum(f) for f in FIELDS) + (sim.device_bytes(),)
    assert raw(sim, 3) == (ESTATE, True) and raw(sim, 1) == (ESTATE, True)   # two obstacles are retained
    assert b"cup3d_create_obstacles" in lib().cup3d_last_error()
    for kw in (dict(handle=False), dict(nobst=-1), dict(null_array=True)):
        assert raw(sim, 2, **kw) == (EINVAL, True), kw
    assert raw(sim, 2, nobst=0) == (0, True) and raw(sim, 2, nobst=0, null_array=True) == (0, True)   # nothing to do
    assert tuple(sim.checksum(f) for f in FIELDS) + (sim.device_bytes(),) == before   # no plan was built, nothing was launched
    rc, untouched = raw(sim, 2)   # and the same call without a fault goes through
    assert rc == 0 and not untouched
    assert tuple(sim.checksum(f) for f in FIELDS) == before[:3] and sim.device_bytes() > before[3]


def test_without_points_only_the_rows_come_down():
    """points = NULL for every obstacle: exactly Rs * 19 * 8 bytes are downloaded, no points buffer is allocated, and rows and totals are
    the same bits"""
    name = "uniform8"
    staged, _ = sims_of(name)
    create(staged, name, "ABC")
    want = staged_call(staged)
    sim = cu.SimulationData(**K.CC.case(name).sim_kwargs)
    create(sim, name, "ABC")
    warm_tiles(sim)
    plan = FC.surface_plan(*lists(sim))
    rows, tiles = len(plan["row_obst"]), len(plan["tile_slots"])
    arr = (ObstacleForces * 3)()
    out = [np.zeros((len(q), 19)) for _, q in want]
    for a, o, q in zip(arr, sim.obstacles, out):
        a.points, a.qoi = None, q.ctypes.data
        for d in range(3):
            a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]
    bytes0 = sim.device_bytes()
    _, down = counted(lambda: check(lib().cup3d_compute_forces_resident(sim.handle, FC.NU, 3, arr)))
    assert down == rows * 19 * 8
    assert sim.device_bytes() - bytes0 == FC.surface_plan_bytes(*lists(sim)) + RC.plan_bytes(lists(sim)[1]) + tiles * TILE_BYTES
    for k, (q, (_, wq), surf) in enumerate(zip(out, want, sim.surfaces)):
        assert np.array_equal(q, wq), k
        assert np.array_equal(np.array(arr[k].totals[:]), FC.totals(wq, surf.slots)), k
    # qoi = NULL as well: the totals alone
    arr2 = (ObstacleForces * 3)()
    for a, b in zip(arr2, arr):
        for d in range(3):
            a.cm[d], a.vel[d], a.omega[d] = b.cm[d], b.vel[d], b.omega[d]
    staged_again = staged_call(staged)
    check(lib().cup3d_compute_forces_resident(sim.handle, FC.NU, 3, arr2))
    for k, ((_, wq), surf) in enumerate(zip(staged_again, sim.surfaces)):
        assert np.array_equal(np.array(arr2[k].totals[:]), FC.totals(wq, surf.slots)), k
    del sim
    gc.collect()


@pytest.mark.parametrize("name", ["uniform8", "amr_periodic_l01"])
def test_a_rank_of_a_spread_grid_is_refused(name):
    """the one-rank entry point on one rank's share of a uniform grid, or on a rank view of a two-level mesh, says so instead of
    returning wrong numbers: EINVAL, nothing built"""
    from test_gpu_create_obstacles_over_ranks import ranks_of
    _, _, make_sims = ranks_of(name)
    check(lib().cup3d_debug_virtual_comm(2))
    try:
        sims, views = make_sims()
        for sim in sims:
            bytes0 = sim.device_bytes()
            assert raw(sim, 2) == (EINVAL, True)
            assert b"rank" in lib().cup3d_last_error()
            assert sim.device_bytes() == bytes0
        del sims, views
        gc.collect()
    finally:
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)
