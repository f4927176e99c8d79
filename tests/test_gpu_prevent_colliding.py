"""cup3d_prevent_colliding_obstacles: Penalization::preventCollidingObstacles (main.cpp:14009-14324) -- k_collision_sums on the blocks
cup3d_create_obstacles keeps on the device, the all-reduces and the pair loop on the host (csrc/obstacles_collisions.hip) -- against its plain-Python
restatement (tests/collision_restatement.py, pinned by tests/test_collision_restatement.py) on the scenarios of tests/collision_cases.py.
MI355X only (-m gpu).

Everything is bit-exact (np.array_equal): the kernel adds in the reference's order, and the host arithmetic has the same association on
both sides."""
import ctypes as C

import numpy as np
import pytest

import collision_cases as K
import cup3d_amd as cu
from cup3d_amd.capi import ObstacleCollision, RunStats, check, lib

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
RETAINED_PER_BLOCK = 4 + 4 * 8 + 1000 * 8 + 512 * 8 + 1536 * 8   # slot, geom, sdfLab, chi, udef
_sims = {}


def sim_of(name):
    if name not in _sims:
        c = K.CC.case(name)
        sim = cu.SimulationData(**c.sim_kwargs)
        assert np.array_equal(sim.grid.geom, c.geom)
        sim.upload("vel", np.random.default_rng(3).uniform(-1, 1, (c.nb, 8, 8, 8, 3)))
        _sims[name] = sim
    return _sims[name]


def shape_of(o, reverse=False):
    s = slice(None, None, -1) if reverse else slice(None)
    return cu.ObstacleShape(o["ids"][s], o["sdf"][s], o["udef"][s], o["transvel_correction"])


def create_shapes(sim, shapes):
    """CreateObstacles; the blocks of THIS call stay on the device and are counted, those of the call before are gone"""
    bytes0 = sim.device_bytes() - getattr(sim, "_retained", 0)
    sim.shapes, sim.obstacles = shapes, []
    cu.CreateObstacles(sim)(0.0)
    sim._retained = RETAINED_PER_BLOCK * sum(len(s.slots) for s in shapes)
    assert sim.device_bytes() - bytes0 == sim._retained


def create(sim, name, which, reverse_first=False):
    """CreateObstacles for the scenario's obstacles, then sim.obstacles in the scenario's rigid state.  Returns the bodies before."""
    keys, _, bodies = K.scenario(name, which)
    obs = K.obstacles(name)
    create_shapes(sim, [shape_of(obs[k], reverse_first and n == 0) for n, k in enumerate(keys)])
    sim.obstacles = [s.data(b["vel"], b["omega"], forced=b["forced"]) for s, b in zip(sim.shapes, bodies)]
    for o, b in zip(sim.obstacles, bodies):   # what the device made of the shapes is what the restatement started from
        assert np.array_equal(o.cm, b["cm"]) and o.mass == b["mass"] and np.array_equal(o.J, b["J"])
    return bodies


def same(sim, r, what):
    for k, (o, b) in enumerate(zip(sim.obstacles, r.bodies)):
        assert np.array_equal(o.collision_sums, np.array(r.sums[k])), (what, k, "sums", o.collision_sums, r.sums[k])
        for f in ("vel", "omega", "collision_vel", "collision_omega"):
            assert np.array_equal(getattr(o, f), np.array(b[f])), (what, k, f, getattr(o, f), b[f])
        assert o.collision_counter == b["collision_counter"], (what, k)
    assert sim.bCollisionID == r.collided and sim.bCollision == r.any, (what, sim.bCollisionID, r.collided)


@pytest.mark.parametrize("name", K.NAMES)
@pytest.mark.parametrize("which", list(K.SCENARIOS))
def test_everything_equals_the_restatement(name, which):
    sim = sim_of(name)
    r, _ = K.expected(name, which)
    create(sim, name, which)
    before = sim.checksum("vel"), sim.checksum("chi"), sim.device_bytes()
    st = RunStats()
    check(lib().cup3d_stats_reset())
    sim.bCollision = False
    cu.PreventCollidingObstacles(sim)(K.DT)
    check(lib().cup3d_stats_read(C.byref(st)))
    same(sim, r, (name, which))
    assert st.field_bytes_downloaded == 20 * 8 * len(sim.obstacles) and st.field_bytes_uploaded == 0
    assert (sim.checksum("vel"), sim.checksum("chi"), sim.device_bytes()) == before
    # a second call from the same state: the same bits, and nothing grows
    bodies = K.scenario(name, which)[2]
    sim.obstacles = [s.data(b["vel"], b["omega"], forced=b["forced"]) for s, b in zip(sim.shapes, bodies)]
    sim.bCollision = False
    cu.PreventCollidingObstacles(sim)(K.DT)
    same(sim, r, (name, which, "second call"))
    assert sim.device_bytes() == before[2]


@pytest.mark.parametrize("name", K.NAMES)
def test_the_order_of_the_retained_lists_does_not_matter(name):
    """B's list descends already; with A's reversed as well the blocks are still visited in ascending slot order"""
    sim = sim_of(name)
    r, _ = K.expected(name, "approach")
    create(sim, name, "approach", reverse_first=True)
    assert list(sim.shapes[0].slots) == sorted(sim.shapes[0].slots, reverse=True)
    sim.bCollision = False
    cu.PreventCollidingObstacles(sim)(K.DT)
    same(sim, r, (name, "A reversed"))


def raw(sim, n, *, handle=True, dt=K.DT, null=(), nobst=None):
    """the entry point on pre-filled structs; returns (rc, nothing of the caller's written?)"""
    arr = (ObstacleCollision * max(1, n))()
    for k, a in enumerate(arr):
        a.mass = 1.0 + k
        for q in range(6):
            a.J[q] = 0.5 if q < 3 else 0.0
        for d in range(3):
            a.cm[d], a.vel[d], a.omega[d], a.collision_vel[d], a.collision_omega[d] = 1.0 + d, 0.25, 0.125, 7.0, 7.0
        a.collision_counter = 7.0
        for q in range(20):
            a.sums[q] = 7.0
    ids = np.full(max(2, n * (n - 1)), 7, dtype=np.int32)
    nids, hit = C.c_int(7), C.c_int(7)
    image = bytes(arr)
    rc = lib().cup3d_prevent_colliding_obstacles(sim.handle if handle else None, dt, n if nobst is None else nobst, None if "obstacles" in null else arr,
                                                 ids.ctypes.data_as(C.c_void_p), None if "ncollided" in null else C.byref(nids),
                                                 None if "any" in null else C.byref(hit))
    check(lib().cup3d_device_synchronize())
    return rc, bytes(arr) == image and (ids == 7).all() and nids.value == 7 and hit.value == 7


def test_refused_calls_touch_nothing():
    c = K.CC.case("uniform8")
    fresh = cu.SimulationData(**c.sim_kwargs)
    assert raw(fresh, 2) == (ESTATE, True)   # no cup3d_create_obstacles yet
    assert b"cup3d_create_obstacles" in lib().cup3d_last_error()
    sim = sim_of("uniform8")
    create(sim, "uniform8", "approach")
    before = sim.checksum("vel"), sim.checksum("chi"), sim.device_bytes()
    assert raw(sim, 3) == (ESTATE, True) and raw(sim, 1) == (ESTATE, True)   # two obstacles are retained
    for kw in (dict(handle=False), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(nobst=-1), dict(null=("obstacles",)), dict(null=("ncollided",)),
               dict(null=("any",))):
        assert raw(sim, 2, **kw) == (EINVAL, True), kw
    assert raw(sim, 2, nobst=0) == (0, True)   # nothing to do
    assert (sim.checksum("vel"), sim.checksum("chi"), sim.device_bytes()) == before
    rc, untouched = raw(sim, 2)   # and the same call without a fault goes through
    assert rc == 0 and not untouched
    # a refused cup3d_create_obstacles drops what was retained
    assert lib().cup3d_create_obstacles(sim.handle, -1, None) == EINVAL
    assert sim.device_bytes() == before[2] - sim._retained
    sim._retained = 0
    assert raw(sim, 2) == (ESTATE, True)


def test_one_obstacle_finds_nothing():
    sim = sim_of("uniform8")
    create_shapes(sim, [shape_of(K.obstacles("uniform8")["A"])])   # the next successful call replaces what the last one left
    sim.obstacles = [sim.shapes[0].data((0.1, 0.2, 0.3), (0.0, 0.1, 0.0))]
    sim.bCollision = False
    cu.PreventCollidingObstacles(sim)(K.DT)
    o = sim.obstacles[0]
    assert (o.collision_sums == 0).all() and sim.bCollisionID == [] and not sim.bCollision
    assert np.array_equal(o.vel, [0.1, 0.2, 0.3]) and o.collision_counter == 0.0
    sim.obstacles = []
    assert cu.PreventCollidingObstacles(sim)(K.DT) is None and sim.bCollisionID == []
