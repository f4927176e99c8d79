"""cup3d_update_obstacles: UpdateObstacles::operator() (main.cpp:13812-13837) -- k_fluid_momenta on the device, the block sum, the two
penal* branches and Obstacle::computeVelocities on the host (csrc/obstacles_update.hip) -- against its plain-Python restatement
(tests/fluid_momenta_restatement.py, pinned by tests/test_fluid_momenta_restatement.py) on the inputs of tests/fluid_momenta_cases.py.
MI355X only (-m gpu).

The blocks' 29 sums and their totals are bit-exact (np.array_equal): the kernel adds the cells in the reference's order.  The velocities
come out of a 6 x 6 LU solve on both sides and may differ by 64 eps cond(A) max|x|."""
import ctypes as C

import numpy as np
import pytest

import cup3d_amd as cu
import fluid_momenta_cases as FC
from cup3d_amd.capi import Obstacle, ObstacleMotion, RunStats, check, lib

pytestmark = pytest.mark.gpu
EINVAL = -1
_sims = {}
CASES = [(n, i) for n in FC.NAMES for i in (0, 1)]


def case(name):
    """(case, sim with vel and chi uploaded), built once per mesh; the tests put the fields back if they change them"""
    if name not in _sims:
        c = FC.case(name)
        sim = cu.SimulationData(**c.sim_kwargs)
        assert sim.nblocks == c.nb
        if c.leaves is not None:
            assert np.array_equal(sim.grid.tables, c.tables)   # same blocks in the same order on both sides
        sim.upload("vel", c.vel)
        sim.upload("chi", c.chi_field)
        sim.lambda_penal = FC.LAMBDA
        _sims[name] = (c, sim)
    return _sims[name]


def data(o, **kw):
    return cu.ObstacleData(o["ids"], o["chi"], o["udef"], o["cm"], o["vel"], o["omega"], **kw)


def run(sim, implicit, obstacles):
    sim.obstacles, sim.bImplicitPenalization = obstacles, bool(implicit)
    cu.UpdateObstacles(sim)(FC.DT)
    return obstacles


def same_sums(o, r, implicit, what):
    n = 29 if implicit else 13
    bad = o.block_sums[:, :n] != r.rows[:, :n]
    assert not bad.any(), f"{what}: block sums differ in columns {sorted(set(np.where(bad)[1].tolist()))}, max |d| = {np.abs(o.block_sums[:, :n] - r.rows[:, :n]).max():.3g}"
    assert np.array_equal(o.totals, r.M), f"{what}: totals differ in {np.where(o.totals != r.M)[0].tolist()}, max |d| = {np.abs(o.totals - r.M).max():.3g}"


def same_motion(o, r, what):
    tol = FC.velocity_bound(r)
    dv, dw = np.abs(o.vel_computed - r.vel_computed).max(), np.abs(o.omega_computed - r.omega_computed).max()
    print(f"{what}: |dv| = {dv:.3g}, |dw| = {dw:.3g}, bound {tol:.3g}, cond(A) = {np.linalg.cond(r.A):.3g}")
    assert dv <= tol and dw <= tol, what


@pytest.mark.parametrize("name,implicit", CASES)
def test_sums_totals_and_velocities_equal_the_restatement(name, implicit):
    c, sim = case(name)
    r = FC.expected(name, implicit, sim.grid.geom)
    before = sim.checksum("vel")
    st = RunStats()
    check(lib().cup3d_stats_reset())
    o, = run(sim, implicit, [data(c.obstacles[0])])
    check(lib().cup3d_stats_read(C.byref(st)))
    same_sums(o, r, implicit, (name, implicit))
    same_motion(o, r, (name, implicit))
    assert st.field_bytes_downloaded == len(o.slots) * 29 * 8   # the blocks' sums and nothing else
    if not implicit:
        assert (o.totals[13:] == 0).all()
    # nothing forced, nothing blocked: the obstacle moves as computed
    assert np.array_equal(o.vel, o.vel_computed) and np.array_equal(o.omega, o.omega_computed)
    assert sim.checksum("vel") == before   # vel is only read
    again, = run(sim, implicit, [data(c.obstacles[0])])
    for k in ("block_sums", "totals", "vel", "omega", "vel_computed", "omega_computed"):
        assert np.array_equal(getattr(again, k), getattr(o, k)), k


@pytest.mark.parametrize("name,implicit", CASES)
def test_explicit_case_leaves_the_implicit_columns_alone(name, implicit):
    """block_sums handed in pre-filled: without implicit penalisation columns 13..28 are not written"""
    c, sim = case(name)
    a = data(c.obstacles[0])
    arr = cu.operators._obstacle_array([a])
    mot = (ObstacleMotion * 1)()
    sums = np.full((len(a.slots), 29), 7.0)
    mot[0].block_sums = sums.ctypes.data
    check(lib().cup3d_update_obstacles(sim.handle, FC.DT, FC.LAMBDA, implicit, 1, arr, mot))
    r = FC.expected(name, implicit, sim.grid.geom)
    n = 29 if implicit else 13
    assert np.array_equal(sums[:, :n], r.rows[:, :n]) and (sums[:, n:] == 7.0).all()
    assert np.array_equal(np.array(mot[0].totals[:]), r.M)


@pytest.mark.parametrize("name,implicit", CASES)
def test_forced_and_blocked_components(name, implicit):
    c, sim = case(name)
    kw = dict(forced=(1, 0, 0), block_rotation=(0, 0, 1), vel_imposed=(0.7, 0.0, 0.0))
    r = FC.expected(name, implicit, sim.grid.geom, 0, kw["forced"], kw["block_rotation"], kw["vel_imposed"])
    o, = run(sim, implicit, [data(c.obstacles[0], **kw)])
    same_sums(o, r, implicit, (name, implicit, "forced"))
    same_motion(o, r, (name, implicit, "forced"))
    assert o.vel[0] == 0.7 and o.omega[2] == 0.0
    assert np.array_equal(o.vel[1:], o.vel_computed[1:]) and np.array_equal(o.omega[:2], o.omega_computed[:2])
    free = FC.expected(name, implicit, sim.grid.geom)
    # the edits changed the other unknowns (the free rotations always; the free translations only where penalCM couples them)
    assert not np.allclose(o.omega_computed[:2], free.omega_computed[:2], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,implicit", CASES)
def test_slot_order_of_the_list_does_not_matter(name, implicit):
    c, sim = case(name)
    a = c.obstacles[0]
    r = FC.expected(name, implicit, sim.grid.geom)
    perm = np.random.default_rng(5).permutation(len(a["ids"]))
    assert not np.array_equal(perm, np.arange(len(perm)))
    o, = run(sim, implicit, [data(dict(a, ids=a["ids"][perm], chi=a["chi"][perm], udef=a["udef"][perm]))])
    n = 29 if implicit else 13
    assert np.array_equal(o.totals, r.M) and np.array_equal(o.block_sums[:, :n], r.rows[perm][:, :n])


@pytest.mark.parametrize("name,implicit", CASES)
def test_two_obstacles_in_one_call_equal_two_calls(name, implicit):
    c, sim = case(name)
    both = run(sim, implicit, [data(c.obstacles[0]), data(c.obstacles[1])])
    assert set(both[0].slots.tolist()) & set(both[1].slots.tolist())   # they share blocks
    for k in (0, 1):
        alone, = run(sim, implicit, [data(c.obstacles[k])])
        r = FC.expected(name, implicit, sim.grid.geom, k)
        same_sums(alone, r, implicit, (name, implicit, "obstacle", k))
        same_motion(alone, r, (name, implicit, "obstacle", k))
        for f in ("block_sums", "totals", "vel", "omega", "vel_computed", "omega_computed"):
            assert np.array_equal(getattr(both[k], f), getattr(alone, f)), (k, f)
    assert not np.array_equal(both[0].totals, both[1].totals)


@pytest.mark.parametrize("name,implicit", CASES)
def test_nan_under_skipped_cells_reaches_no_output(name, implicit):
    """NaN in vel wherever the obstacle's chi <= 0 -- and in every block the obstacle does not list: no bit of any output changes"""
    c, sim = case(name)
    a = c.obstacles[0]
    r = FC.expected(name, implicit, sim.grid.geom)
    bad = np.full_like(c.vel, np.nan)
    sub = c.vel[a["ids"]].copy()
    sub[a["chi"] <= 0] = np.nan
    bad[a["ids"]] = sub
    assert np.isnan(sub).any() and not np.isnan(sub).all()
    sim.upload("vel", bad)
    try:
        o, = run(sim, implicit, [data(a)])
    finally:
        sim.upload("vel", c.vel)
    same_sums(o, r, implicit, (name, implicit, "NaN"))
    same_motion(o, r, (name, implicit, "NaN"))
    assert np.isfinite(o.vel).all() and np.isfinite(o.omega).all()


def _call(sim, implicit, obstacles, dt=FC.DT, handle=True, null_motion=False, null_obstacles=False, **override):
    """the raw entry point on pre-filled outputs; `override` replaces fields of the LAST obstacle's struct.  Returns (rc, untouched?)"""
    arr = cu.operators._obstacle_array(obstacles)
    for k, v in override.items():
        setattr(arr[len(obstacles) - 1], k, v)
    mot = (ObstacleMotion * len(obstacles))()
    sums = [np.full((len(o.slots), 29), 7.0) for o in obstacles]
    for m, b in zip(mot, sums):
        m.block_sums = b.ctypes.data
        for q in range(29):
            m.totals[q] = 5.0
        for d in range(3):
            m.vel_computed[d] = m.omega_computed[d] = 6.0
    rc = lib().cup3d_update_obstacles(sim.handle if handle else None, dt, FC.LAMBDA, implicit, len(obstacles), None if null_obstacles else arr,
                                      None if null_motion else mot)
    check(lib().cup3d_device_synchronize())
    untouched = all((b == 7.0).all() for b in sums) and all(list(m.totals) == [5.0] * 29 and list(m.vel_computed) + list(m.omega_computed) == [6.0] * 6 for m in mot)
    untouched = untouched and all(list(a.vel) == list(o.vel) and list(a.omega) == list(o.omega) for a, o in zip(arr, obstacles))
    return rc, untouched


@pytest.mark.parametrize("implicit", [0, 1])
def test_refused_calls_touch_nothing(implicit):
    c, sim = case("uniform8")
    good, other = data(c.obstacles[0]), data(c.obstacles[1])
    hi, lo = good.slots.copy(), good.slots.copy()
    hi[1], lo[0] = c.nb, -1
    empty = cu.ObstacleData(good.slots, np.zeros_like(good.chi), good.udef, good.cm, good.vel, good.omega)
    below = cu.ObstacleData(good.slots, -np.abs(good.chi), good.udef, good.cm, good.vel, good.omega)
    before = sim.checksum("vel")
    refused = [dict(dt=0.0), dict(dt=-0.01), dict(handle=False), dict(null_motion=True), dict(null_obstacles=True), dict(slots=None), dict(chi=None),
               dict(udef=None), dict(slots=hi.ctypes.data), dict(slots=lo.ctypes.data), dict(nblocks=-1)]
    for kw in refused:
        # a good obstacle first: nothing of it may be written either when the one after it is refused
        rc, untouched = _call(sim, implicit, [other, good], **kw)
        assert rc == EINVAL and untouched, kw
    for bad in (empty, below):   # chi all zero / nowhere positive: the reference's assert(M[0] > EPS)
        rc, untouched = _call(sim, implicit, [other, bad])
        assert rc == EINVAL and untouched
        assert b"volume" in lib().cup3d_last_error()
    assert lib().cup3d_update_obstacles(sim.handle, FC.DT, FC.LAMBDA, implicit, -1, None, None) == EINVAL
    rc, untouched = _call(sim, implicit, [other, good])   # and the same call without the fault goes through
    assert rc == 0 and not untouched
    assert sim.checksum("vel") == before


def test_nothing_to_do_is_not_an_error():
    c, sim = case("uniform8")
    assert lib().cup3d_update_obstacles(sim.handle, FC.DT, FC.LAMBDA, 1, 0, None, None) == 0
    sim.obstacles = []
    assert cu.UpdateObstacles(sim)(FC.DT) is None
