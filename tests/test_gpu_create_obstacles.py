"""cup3d_create_obstacles: the grid half of CreateObstacles::operator() (main.cpp:13596-13619) -- k_characteristic, k_udef_momenta and
k_remove_udef_momenta on the device, kernelComputeGridCoM and kernelAccumulateUdefMomenta on the host (csrc/obstacles_create.hip) -- against its
plain-Python restatement (tests/characteristic_restatement.py, pinned by tests/test_characteristic_restatement.py) on the inputs of
tests/characteristic_cases.py.  MI355X only (-m gpu).

Everything is bit-exact (np.array_equal): the kernels add in the reference's order and write the surface points in its push_back
order, and the host half is the same scalar arithmetic on both sides."""
import ctypes as C

import numpy as np
import pytest

import characteristic_cases as CC
import cup3d_amd as cu
from cup3d_amd.capi import ObstacleShape, RunStats, check, lib

pytestmark = pytest.mark.gpu
EINVAL = -1
_sims = {}
FIELDS = ("chi", "first", "ijk", "dchi", "delta", "block_com", "com_totals", "cm", "block_momenta", "udef_totals", "mass", "J",
          "transvel_correction", "angvel_correction")


def case(name):
    """(case, sim with vel and pres uploaded), built once per mesh"""
    if name not in _sims:
        c = CC.case(name)
        sim = cu.SimulationData(**c.sim_kwargs)
        assert sim.nblocks == c.nb
        if c.leaves is not None:
            assert np.array_equal(sim.grid.tables, c.tables)   # same blocks in the same order on both sides
        assert np.array_equal(sim.grid.geom, c.geom)
        rng = np.random.default_rng(3)
        sim.upload("vel", rng.uniform(-1, 1, (c.nb, 8, 8, 8, 3)))
        sim.upload("pres", rng.uniform(-1, 1, (c.nb, 8, 8, 8)))
        _sims[name] = (c, sim)
    return _sims[name]


def shapes_of(obstacles, corrections=None):
    return [cu.ObstacleShape(o["ids"], o["sdf"], o["udef"], o["transvel_correction"] if corrections is None else corrections[k])
            for k, o in enumerate(obstacles)]


def same(shape, r, what):
    for f in FIELDS:
        got, want = np.asarray(getattr(shape, f)), np.asarray(getattr(r, f))
        assert got.shape == want.shape, (what, f, got.shape, want.shape)
        assert np.array_equal(got, want), f"{what}: {f} differs in {int((got != want).sum())} of {got.size} entries, max |d| = {np.abs(got - want).max():.3g}"
    bad = shape.udef_corrected != r.udef
    assert not bad.any(), f"{what}: corrected udef differs in {int(bad.sum())} entries, max |d| = {np.abs(shape.udef_corrected - r.udef).max():.3g}"


def promised_bytes(shapes):
    """the header's DOWNLOADS paragraph"""
    return sum(len(s.slots) * (4 * 8 + 4 + 13 * 8 + 2048 * 8) + len(s.delta) * (3 * 4 + 4 * 8) for s in shapes)


@pytest.mark.parametrize("name", CC.NAMES)
def test_everything_equals_the_restatement(name):
    c, sim = case(name)
    field, first, second, _ = CC.expected(name, sim.grid.geom)
    sim.fill("chi", 0.7)   # what the call has to clear, blocks no obstacle lists included
    before = sim.checksum("vel"), sim.checksum("pres")
    sim.shapes = shapes_of(c.obstacles)
    st = RunStats()
    check(lib().cup3d_stats_reset())
    cu.CreateObstacles(sim)(0.0)
    check(lib().cup3d_stats_read(C.byref(st)))
    for k, (s, r) in enumerate(zip(sim.shapes, first)):
        same(s, r, (name, "obstacle", k))
    assert st.field_bytes_downloaded == promised_bytes(sim.shapes)
    got = sim.download("chi")
    assert np.array_equal(got, field), f"{name}: the resident chi differs in {int((got != field).sum())} cells"
    assert (sim.checksum("vel"), sim.checksum("pres")) == before
    # the udef the geometry wrote is the caller's, and stays
    for s, o in zip(sim.shapes, c.obstacles):
        assert np.array_equal(s.udef, o["udef"]) and not np.array_equal(s.udef_corrected, o["udef"])
    # the next step: the same geometry, oldCorrVel = what this call returned
    again = shapes_of(c.obstacles, [s.transvel_correction for s in sim.shapes])
    sim.shapes = again
    cu.CreateObstacles(sim)(0.0)
    for k, (s, r) in enumerate(zip(again, second)):
        same(s, r, (name, "second call, obstacle", k))
    assert np.array_equal(sim.download("chi"), field)
    assert not np.array_equal(again[0].angvel_correction, first[0].angvel_correction)


@pytest.mark.parametrize("name", CC.NAMES)
def test_one_obstacle_alone_and_the_order_of_the_list(name):
    """obstacle B alone (its slots descend) and with its blocks shuffled: rows follow the list, totals do not change"""
    c, sim = case(name)
    _, first, _, _ = CC.expected(name, sim.grid.geom)
    b, r = c.obstacles[1], first[1]
    sim.shapes = shapes_of([b])
    cu.CreateObstacles(sim)(0.0)
    same(sim.shapes[0], r, (name, "B alone"))
    assert np.array_equal(sim.download("chi")[b["ids"]], r.chi)   # alone, the field holds this obstacle's chi
    perm = np.random.default_rng(5).permutation(len(b["ids"]))
    sim.shapes = shapes_of([dict(b, ids=b["ids"][perm], sdf=b["sdf"][perm], udef=b["udef"][perm])])
    cu.CreateObstacles(sim)(0.0)
    s = sim.shapes[0]
    for f in ("com_totals", "cm", "udef_totals", "mass", "J", "transvel_correction", "angvel_correction"):
        assert np.array_equal(getattr(s, f), getattr(r, f)), f
    assert np.array_equal(s.chi, r.chi[perm]) and np.array_equal(s.udef_corrected, r.udef[perm]) and np.array_equal(s.block_momenta, r.block_momenta[perm])
    assert np.array_equal(np.diff(s.first), np.diff(r.first)[perm])
    for i, j in enumerate(perm):
        assert np.array_equal(s.dchi[s.first[i]:s.first[i + 1]], r.dchi[r.first[j]:r.first[j + 1]])
        assert np.array_equal(s.ijk[s.first[i]:s.first[i + 1]], r.ijk[r.first[j]:r.first[j + 1]])


def _call(sim, obstacles, handle=True, null_shapes=False, nobst=None, **override):
    """the raw entry point on pre-filled outputs; `override` replaces fields of the LAST obstacle's struct.  Returns (rc, untouched?)"""
    arr = (ObstacleShape * len(obstacles))()
    keep = []
    for o, a in zip(obstacles, arr):
        n = len(o["ids"])
        w = dict(slots=np.ascontiguousarray(o["ids"], dtype=np.int32), sdf=np.ascontiguousarray(o["sdf"]), udef=o["udef"].copy(), chi=np.full((n, 8, 8, 8), 7.0),
                 block_com=np.full((n, 4), 7.0), block_momenta=np.full((n, 13), 7.0), first=np.full(n + 1, 7, dtype=np.int32),
                 ijk=np.full((512 * n, 3), 7, dtype=np.int32), dchi=np.full((512 * n, 3), 7.0), delta=np.full(512 * n, 7.0))
        a.nblocks = n
        for k, v in w.items():
            setattr(a, k, v.ctypes.data)
        for d in range(3):
            a.transvel_correction[d], a.angvel_correction[d], a.cm[d] = 0.25, 5.0, 5.0
        a.mass = 5.0
        for q in range(6):
            a.J[q] = 5.0
        for q in range(4):
            a.com_totals[q] = 5.0
        for q in range(13):
            a.udef_totals[q] = 5.0
        keep.append(w)
    for k, v in override.items():
        setattr(arr[len(obstacles) - 1], k, v)
    rc = lib().cup3d_create_obstacles(sim.handle if handle else None, len(obstacles) if nobst is None else nobst, None if null_shapes else arr)
    check(lib().cup3d_device_synchronize())
    untouched = True
    for o, a, w in zip(obstacles, arr, keep):
        untouched &= all((w[k] == 7).all() for k in ("chi", "block_com", "block_momenta", "first", "ijk", "dchi", "delta"))
        untouched &= np.array_equal(w["udef"], o["udef"])
        untouched &= list(a.transvel_correction) == [0.25] * 3 and list(a.angvel_correction) + list(a.cm) == [5.0] * 6 and a.mass == 5.0
        untouched &= list(a.J) == [5.0] * 6 and list(a.com_totals) == [5.0] * 4 and list(a.udef_totals) == [5.0] * 13
    return rc, bool(untouched)


def test_refused_calls_touch_nothing():
    c, sim = case("uniform8")
    a, b = c.obstacles
    hi, lo = np.ascontiguousarray(b["ids"], dtype=np.int32), np.ascontiguousarray(b["ids"], dtype=np.int32)
    hi[1], lo[0] = c.nb, -1
    sim.fill("chi", 0.3)
    before = sim.checksum("chi"), sim.checksum("vel"), sim.checksum("pres")
    refused = [dict(handle=False), dict(null_shapes=True), dict(nobst=-1), dict(nblocks=-1), dict(slots=hi.ctypes.data), dict(slots=lo.ctypes.data)]
    refused += [{k: None} for k in ("slots", "sdf", "udef", "chi", "first", "ijk", "dchi", "delta")]
    for kw in refused:
        # a good obstacle first: nothing of it may be written either when the one after it is refused
        rc, untouched = _call(sim, [a, b], **kw)
        assert rc == EINVAL and untouched, kw
        assert (sim.checksum("chi"), sim.checksum("vel"), sim.checksum("pres")) == before, kw   # not even the clear
    # a body without volume as the second of two: the reference's assert(com[0] > epsilon); the resident chi is unspecified afterwards
    rc, untouched = _call(sim, [a, c.nothing])
    assert rc == EINVAL and untouched
    assert b"volume" in lib().cup3d_last_error()
    assert (sim.checksum("vel"), sim.checksum("pres")) == before[1:]
    rc, untouched = _call(sim, [a, b])   # and the same call without a fault goes through
    assert rc == 0 and not untouched


def test_nothing_to_do_is_not_an_error_and_clears_nothing():
    c, sim = case("uniform8")
    sim.fill("chi", 0.3)
    before = sim.checksum("chi")
    assert lib().cup3d_create_obstacles(sim.handle, 0, None) == 0
    sim.shapes = []
    assert cu.CreateObstacles(sim)(0.0) is None
    assert sim.checksum("chi") == before   # CreateObstacles::operator() returns at 13590, before CHI.clear()
    del sim.shapes
