"""cup3d_update_obstacles_resident, cup3d_penalization_resident and cup3d_update_tmpv_resident -- UpdateObstacles, Penalization and
kernelUpdateTmpV on the blocks cup3d_create_obstacles keeps on the device, one launch per operator (csrc/obstacles_update.hip, csrc/obstacles_penalization.hip) -- against the
staged entry points cup3d_update_obstacles, cup3d_penalization and cup3d_update_tmpv, which take the same chi and udef from the host,
obstacle after obstacle.  MI355X only (-m gpu).

Everything is bit-exact (np.array_equal): the kernels share their bodies, the slot-major kernels walk a slot's obstacles in the staged
calls' order (tests/test_resident_obstacles_cases.py counts the cells where another order shows), and the host halves are the same code."""
import ctypes as C
import gc

import numpy as np
import pytest

import cup3d_amd as cu
import resident_obstacles_cases as RC
from cup3d_amd.capi import ObstacleBody, ObstacleMotion, RunStats, check, lib

pytestmark = pytest.mark.gpu
K = RC.K
EINVAL, ESTATE = -1, -5
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


def create(sim, name, keys, implicit, reverse_first=False):
    """vel uploaded, CreateObstacles for the set, sim.obstacles in the set's rigid state"""
    obs = K.obstacles(name)
    sim.upload("vel", RC.vel_of(name))
    sim.lambda_penal, sim.bImplicitPenalization = RC.LAMBDA, bool(implicit)
    sim.shapes, sim.obstacles = [shape_of(obs[k], reverse_first and n == 0) for n, k in enumerate(keys)], []
    cu.CreateObstacles(sim)(0.0)
    rigid(sim, keys)


def rigid(sim, keys):
    sim.obstacles = [s.data(K.APPROACH[k]["vel"], K.APPROACH[k]["omega"], forced=(k == "B", 0, 0), vel_imposed=(0.125, 0, 0)) for s, k in zip(sim.shapes, keys)]


def downloaded(op, *a):
    """field bytes the call brought down; it takes none up"""
    st = RunStats()
    check(lib().cup3d_stats_reset())
    op(*a)
    check(lib().cup3d_stats_read(C.byref(st)))
    assert st.field_bytes_uploaded == 0
    return int(st.field_bytes_downloaded)


def sequence(sim, resident):
    """UpdateObstacles -> Penalization -> tmpV = 0, kernelUpdateTmpV; returns what they leave and the bytes each downloaded"""
    sim.resident_obstacles = resident
    n = len(sim.obstacles)
    down = [downloaded(cu.UpdateObstacles(sim), RC.DT), downloaded(cu.Penalization(sim), RC.DT)]
    sim.fill("tmpV", 0.0)
    if resident:
        down.append(downloaded(lambda: check(lib().cup3d_update_tmpv_resident(sim.handle, n))))
    else:
        down.append(downloaded(lambda: check(lib().cup3d_update_tmpv(sim.handle, n, cu.operators._obstacle_array(sim.obstacles)))))
    out = dict(obstacles=[{f: np.array(getattr(o, f)).copy() for f in ("block_sums", "totals", "vel_computed", "omega_computed", "vel", "omega", "force", "torque")}
                          for o in sim.obstacles])
    for f in ("vel", "tmpV", "chi"):
        out[f] = sim.download(f)
    return out, down


def same(got, want, what, skip=()):
    for k, (g, w) in enumerate(zip(got["obstacles"], want["obstacles"])):
        for f in w:
            if (k, f) not in skip:
                assert np.array_equal(g[f], w[f]), (what, k, f)
    for f in ("vel", "tmpV", "chi"):
        assert np.array_equal(got[f], want[f]), (what, f)


@pytest.mark.parametrize("name", RC.NAMES)
@pytest.mark.parametrize("keys", list(RC.SETS))
@pytest.mark.parametrize("implicit", [0, 1])
def test_the_resident_calls_equal_the_staged_ones(name, keys, implicit):
    staged, resident = sims_of(name)
    create(staged, name, keys, implicit)
    create(resident, name, keys, implicit)
    want, staged_down = sequence(staged, False)
    lists = [s.slots for s in resident.shapes]
    rows = sum(len(s) for s in lists)
    bytes0 = resident.device_bytes()
    got, down = sequence(resident, True)
    same(got, want, (name, keys, implicit))
    assert np.abs(want["vel"] - RC.vel_of(name)).max() > 0 and np.abs(want["tmpV"]).max() > 0
    # one download per operator, whatever the number of obstacles; the staged calls download the same rows obstacle by obstacle
    assert down == [rows * 29 * 8, rows * 6 * 8, 0] and staged_down[0] == down[0]
    # the plan is built by the first resident call, counted, and kept
    assert resident.device_bytes() - bytes0 == RC.plan_bytes(lists) > 0
    # a second call from the same state: the same bits, and nothing grows
    resident.upload("vel", RC.vel_of(name))
    rigid(resident, keys)
    again, down = sequence(resident, True)
    same(again, want, (name, keys, implicit, "second call"))
    assert resident.device_bytes() - bytes0 == RC.plan_bytes(lists) and down == [rows * 29 * 8, rows * 6 * 8, 0]


@pytest.mark.parametrize("name", RC.NAMES)
def test_block_sums_follow_the_listed_order(name):
    """with A's list reversed its block_sums come back reversed, and nothing else changes: rows are added in ascending slot order"""
    staged, resident = sims_of(name)
    create(staged, name, "ABC", 1)
    want, _ = sequence(staged, False)
    create(resident, name, "ABC", 1, reverse_first=True)
    assert list(resident.shapes[0].slots) == sorted(resident.shapes[0].slots, reverse=True)
    got, _ = sequence(resident, True)
    same(got, want, (name, "A reversed"), skip={(0, "block_sums")})
    assert np.array_equal(got["obstacles"][0]["block_sums"], want["obstacles"][0]["block_sums"][::-1])


def test_a_new_set_replaces_the_plan():
    staged, resident = sims_of("uniform8")
    create(resident, "uniform8", "AB", 0)
    sequence(resident, True)   # the plan of A, B exists
    base = resident.device_bytes() - RC.plan_bytes([s.slots for s in resident.shapes])
    create(staged, "uniform8", "ABC", 0)
    want, _ = sequence(staged, False)
    create(resident, "uniform8", "ABC", 0)
    nb = resident.nblocks
    assert resident.device_bytes() == base + 24420 * nb   # the old set went with its plan; C's blocks came, the new plan is not built yet
    got, _ = sequence(resident, True)
    same(got, want, "AB, then ABC")
    assert resident.device_bytes() == base + 24420 * nb + RC.plan_bytes([s.slots for s in resident.shapes])
    # a refused cup3d_create_obstacles drops the set and its plan
    assert lib().cup3d_create_obstacles(resident.handle, -1, None) == EINVAL
    assert resident.device_bytes() == base - 2 * 24420 * nb
    assert lib().cup3d_update_tmpv_resident(resident.handle, 3) == ESTATE


def test_a_one_block_obstacle_counts_by_the_formulas():
    """one listed block: its slot list and the plan's three row tables are ONE int32 each, and are counted as 4 bytes -- the 8 bytes an
    empty table gets are for an empty table only.  Over ranks an obstacle with a single local block is ordinary."""
    c, o = K.CC.case("uniform8"), K.obstacles("uniform8")["A"]
    i = int(np.argmax(o["chi"].reshape(len(o["ids"]), -1).sum(axis=1)))   # the block that holds most of the sphere
    sim = cu.SimulationData(**c.sim_kwargs)
    sim.upload("vel", RC.vel_of("uniform8"))
    sim.lambda_penal, sim.bImplicitPenalization, sim.resident_obstacles = RC.LAMBDA, False, True
    sim.shapes, sim.obstacles = [cu.ObstacleShape(o["ids"][i:i + 1], o["sdf"][i:i + 1], o["udef"][i:i + 1], o["transvel_correction"])], []
    bytes0 = sim.device_bytes()
    cu.CreateObstacles(sim)(0.0)
    assert sim.device_bytes() - bytes0 == 24420   # slots 4 + geom 32 + sdf 8000 + chi 4096 + udef 12288, as per block in the tests above
    sim.obstacles = [sim.shapes[0].data(K.APPROACH["A"]["vel"], K.APPROACH["A"]["omega"])]
    bytes1 = sim.device_bytes()
    cu.UpdateObstacles(sim)(RC.DT)
    assert sim.device_bytes() - bytes1 == RC.plan_bytes([sim.shapes[0].slots]) == (32 + 72) + (3 * 4 + 29 * 8) + 2 * 4
    del sim
    gc.collect()


def test_a_sim_with_a_plan_is_destroyed():
    c = K.CC.case("uniform8")
    sim = cu.SimulationData(**c.sim_kwargs)
    create(sim, "uniform8", "AB", 0)
    bytes0 = sim.device_bytes()
    sequence(sim, True)
    assert sim.device_bytes() > bytes0
    del sim   # cup3d_sim_destroy frees the retained set and the plan with it
    gc.collect()
    check(lib().cup3d_device_synchronize())


def raw(sim, which, n, *, handle=True, dt=RC.DT, null=(), nobst=None):
    """an entry point on pre-filled structs; returns (rc, nothing of the caller's written?)"""
    body = (ObstacleBody * max(1, n))()
    mot = (ObstacleMotion * max(1, n))()
    sums = np.full((max(1, n), 64, 29), 7.0)
    for k in range(max(1, n)):
        for d in range(3):
            body[k].cm[d], body[k].vel[d], body[k].omega[d], body[k].force[d], body[k].torque[d] = 3.0 + 0.1 * d, 0.25, 0.125, 7.0, 7.0
            mot[k].vel_computed[d] = mot[k].omega_computed[d] = 7.0
        for q in range(29):
            mot[k].totals[q] = 7.0
        mot[k].block_sums = sums[k].ctypes.data
    image = bytes(body), bytes(mot)
    h = sim.handle if handle else None
    count = n if nobst is None else nobst
    if which == "update":
        rc = lib().cup3d_update_obstacles_resident(h, dt, RC.LAMBDA, 1, count, None if "body" in null else body, None if "motion" in null else mot)
    elif which == "penalization":
        rc = lib().cup3d_penalization_resident(h, dt, RC.LAMBDA, 1, count, None if "body" in null else body)
    else:
        rc = lib().cup3d_update_tmpv_resident(h, count)
    check(lib().cup3d_device_synchronize())
    return rc, (bytes(body), bytes(mot)) == image and bool((sums == 7.0).all())


def test_refused_calls_touch_nothing():
    c = K.CC.case("uniform8")
    fresh = cu.SimulationData(**c.sim_kwargs)
    for which in ("update", "penalization", "tmpv"):
        assert raw(fresh, which, 2) == (ESTATE, True), which   # no cup3d_create_obstacles yet
        assert b"cup3d_create_obstacles" in lib().cup3d_last_error()
    _, sim = sims_of("uniform8")
    create(sim, "uniform8", "AB", 1)
    sim.fill("tmpV", 0.5)
    before = sim.checksum("vel"), sim.checksum("tmpV"), sim.checksum("chi"), sim.device_bytes()
    for which in ("update", "penalization", "tmpv"):
        assert raw(sim, which, 3) == (ESTATE, True) and raw(sim, which, 1) == (ESTATE, True), which   # two obstacles are retained
        assert b"cup3d_create_obstacles" in lib().cup3d_last_error()
        for kw in (dict(handle=False), dict(nobst=-1)):
            assert raw(sim, which, 2, **kw) == (EINVAL, True), (which, kw)
        assert raw(sim, which, 2, nobst=0) == (0, True), which   # nothing to do
    for which in ("update", "penalization"):
        for kw in (dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(null=("body",))):
            assert raw(sim, which, 2, **kw) == (EINVAL, True), (which, kw)
    assert raw(sim, "update", 2, null=("motion",)) == (EINVAL, True)
    assert (sim.checksum("vel"), sim.checksum("tmpV"), sim.checksum("chi"), sim.device_bytes()) == before   # no plan was built either
    # and the same calls without a fault go through
    rc, untouched = raw(sim, "update", 2)
    assert rc == 0 and not untouched and sim.checksum("vel") == before[0]
    rc, untouched = raw(sim, "penalization", 2)
    assert rc == 0 and not untouched and sim.checksum("vel") != before[0]
    assert raw(sim, "tmpv", 2) == (0, True) and sim.checksum("tmpV") != before[1]
    assert sim.device_bytes() == before[3] + RC.plan_bytes([s.slots for s in sim.shapes])


def test_the_order_of_the_obstacles_shows_on_the_device():
    """the staged calls with the obstacles listed C, B, A leave other bits in vel and tmpV than with A, B, C: the comparison above would
    catch a kernel that walks a slot's obstacles in another order"""
    staged, _ = sims_of("amr_periodic_l01")
    create(staged, "amr_periodic_l01", "ABC", 0)
    want, _ = sequence(staged, False)
    staged.upload("vel", RC.vel_of("amr_periodic_l01"))
    rigid(staged, "ABC")
    staged.obstacles = staged.obstacles[::-1]
    # UpdateObstacles does not depend on the order; its velocities go into Penalization as above
    got, _ = sequence(staged, False)
    for g, w in zip(got["obstacles"][::-1], want["obstacles"]):
        assert np.array_equal(g["vel"], w["vel"]) and np.array_equal(g["omega"], w["omega"])
    assert int((got["tmpV"] != want["tmpV"]).any(axis=-1).sum()) == 211   # tests/test_resident_obstacles_cases.py
    assert not np.array_equal(got["vel"], want["vel"])
