"""cup3d_sim_labs / cup3d_sim_labs_device: ghosted block tiles of any stencil box, built on the device (k_labs, csrc/labs.hip), against the
CPU oracle's restatement of BlockLab::load + post_load (orc_mesh_labs, pinned to the compiled reference for these boxes by
test_oracle_amr.py and test_oracle_wide_labs.py) and against the reference's own tiles.

Everything is bit-exact: np.array_equal on the cells the reference defines (oracle_lib.lab_mask), NaN on the others (the edge and
corner ghosts of a star tile with width <= 2)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

import cup3d_amd as cu
import oracle_lib as O
from cup3d_amd.capi import RunStats, check, lib
from cup3d_amd.operators import FIELDS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EXT = 2 * np.pi
EINVAL = -1

# name -> bpd, levelMax, bc, leaves (None: the uniform grid at level 0)
UNIFORM = {
    "one_block_periodic": ((1, 1, 1), 1, ("periodic", "periodic", "periodic")),   # one block that is its own 26 neighbours
    "box321_every_bc": ((3, 2, 1), 1, ("periodic", "wall", "freespace")),         # non-cubic; blocks both first and last along z
    "box222_wall": ((2, 2, 2), 1, ("wall", "wall", "wall")),
}
GOLDEN = ("amr_periodic_l01", "amr_mixed_l12")   # the smallest shapes with coarser and finer neighbours at faces, edges and corners

_cases = {}


def case(name):
    """(sim with seeded vel / pres uploaded, oracle mesh, vel, pres), built once per mesh and shared, never modified."""
    if name not in _cases:
        if name in UNIFORM:
            bpd, lmax, bc = UNIFORM[name]
            sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
            m = O.OracleMesh(bpd, lmax, EXT, bc, sim.grid.tables[:, 0], sim.grid.tables[:, 1])
        else:
            g = np.load(os.path.join(GOLD, name + ".npz"))
            bpd, lmax, t = tuple(int(b) for b in g["bpd"]), int(g["level_max"]), g["tables"]
            bc = tuple(O.BC_NAMES[int(b)] for b in g["bc"])
            m = O.OracleMesh(bpd, lmax, float(g["extent"]), bc, t[:, 0], t[:, 1])
            sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=float(g["extent"]), BC_x=bc[0], BC_y=bc[1],
                                    BC_z=bc[2], leaves=(t[:, 0], t[:, 1]))
        assert np.array_equal(sim.grid.tables, m.tables)   # same blocks in the same order on both sides
        rng = np.random.default_rng(len(name))
        vel, pres = rng.uniform(-1, 1, (m.nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (m.nb, 8, 8, 8))
        sim.upload("vel", vel)
        sim.upload("pres", pres)
        _cases[name] = (sim, m, vel, pres)
    return _cases[name]


def same_tiles(got, ref, w, tens, what):
    """got [n, L, L, L(, nc)] equals ref [n, L, L, L, nc] bit for bit on lab_mask and is NaN off it"""
    got = got.reshape(ref.shape)
    mask = O.lab_mask(-w, w + 1, tens)
    bad = got[:, mask] != ref[:, mask]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} defined cells differ, max |d| = {np.abs(got[:, mask] - ref[:, mask]).max():.3g}"
    assert np.isnan(got[:, ~mask]).all(), f"{what}: a cell the reference leaves undefined is not NaN"
    assert not np.isnan(got[:, mask]).any(), what


# ---- 1 and 2: every box on uniform grids and on the committed multi-level meshes
@pytest.mark.parametrize("w", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(UNIFORM) + list(GOLDEN))
def test_tiles_equal_the_oracle(name, w):
    sim, m, vel, pres = case(name)
    if name in GOLDEN:
        assert len(set(m.tables[:, 0].tolist())) >= 2
    for tens in (False, True):
        for fname, field in (("vel", vel), ("pres", pres)):
            got = sim.labs(fname, w, tensorial=tens)
            L = 8 + 2 * w
            assert got.shape == ((m.nb, L, L, L, 3) if fname == "vel" else (m.nb, L, L, L))
            same_tiles(got, m.labs(field, -w, w + 1, tens), w, tens, (name, fname, w, tens))


# ---- 3: against the reference's own tiles
needs_ref = pytest.mark.skipif(not O.have_ref_tool(), reason="oracle/_ref/ref_tool not built (no reference tree here)")
LIVE = [
    ((2, 2, 2), 3, ("periodic",) * 3, 2, 2.0),
    ((2, 2, 2), 3, ("wall", "wall", "wall"), 2, 2.0),
    ((3, 2, 2), 3, ("periodic", "freespace", "wall"), 2, 2.0),
    ((2, 2, 2), 4, ("wall", "periodic", "freespace"), 3, 1.0),  # three levels
]   # the mesh recipes of test_oracle_amr.py::LIVE


@needs_ref
@pytest.mark.parametrize("bpd,lmax,bc,passes,rtol", LIVE)
def test_tiles_equal_the_reference(bpd, lmax, bc, passes, rtol):
    sys.path.insert(0, GOLD)
    import make_golden as M
    wd = O.tempfile.mkdtemp(prefix="labs_")
    pre = M.amr_mesh_script(wd, bpd, passes, rtol)
    args = O.ref_args(bpd, lmax, 0, EXT, bc)
    _, wd = O.run_ref(pre + ["tables t1.bin"], args, threads=1, workdir=wd)
    t1, _ = O.read_tables(os.path.join(wd, "t1.bin"))
    nb = len(t1)
    assert len(set(t1[:, 0].tolist())) >= (3 if lmax == 4 else 2)
    rng = np.random.default_rng(7)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    vel.tofile(os.path.join(wd, "velb.bin"))
    pres.tofile(os.path.join(wd, "presb.bin"))
    boxes = [("vel", -4, 5, 1), ("pres", -4, 5, 1), ("vel", -2, 3, 1), ("vel", -3, 4, 0), ("pres", -1, 2, 0)]
    script = pre + ["loadb vel velb.bin", "loadb pres presb.bin"] + [f"lab {f} {s} {e} {t} lab{i}.bin" for i, (f, s, e, t) in enumerate(boxes)]
    _, wd = O.run_ref(script, args, threads=1, workdir=wd)
    sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2],
                            leaves=(t1[:, 0], t1[:, 1]))
    assert np.array_equal(sim.grid.tables, t1)
    sim.upload("vel", vel)
    sim.upload("pres", pres)
    for i, (f, s, e, t) in enumerate(boxes):
        L, nc = 8 + e - s - 1, 3 if f == "vel" else 1
        ref = np.fromfile(os.path.join(wd, f"lab{i}.bin")).reshape(nb, L, L, L, nc)
        got = sim.labs(f, -s, tensorial=bool(t)).reshape(ref.shape)
        mask = O.lab_mask(s, e, bool(t))
        assert np.array_equal(got[:, mask], ref[:, mask]), (f, s, e, t)
        assert np.isnan(got[:, ~mask]).all(), (f, s, e, t)


# ---- 4: slot lists
@pytest.mark.parametrize("name", ["box321_every_bc", "amr_mixed_l12"])
def test_slot_lists(name):
    sim, m, vel, pres = case(name)
    rng = np.random.default_rng(3)
    for fname, w, tens in (("vel", 4, True), ("pres", 1, False), ("vel", 2, False)):
        every = sim.labs(fname, w, tensorial=tens)
        assert np.array_equal(sim.labs(fname, w, tensorial=tens, slots=np.arange(m.nb)), every, equal_nan=True)
        sl = rng.permutation(m.nb)[:max(3, m.nb // 2)]
        sl = np.concatenate([sl, sl[1:2]])   # shuffled, one repeat
        assert np.array_equal(sim.labs(fname, w, tensorial=tens, slots=sl), every[sl], equal_nan=True)


# ---- 5: the device variant
def test_device_variant_equals_the_host_variant():
    import torch
    sim, m, vel, pres = case("amr_mixed_l12")
    for fname, w, tens in (("vel", 4, True), ("pres", 1, False)):
        host = sim.labs(fname, w, tensorial=tens)
        dev = torch.full(host.shape, 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert sim.labs_into(dev.data_ptr(), fname, w, tensorial=tens) == host.shape
        check(lib().cup3d_device_synchronize())   # the device variant is stream-ordered on the library's stream and does not wait
        assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True)
        sl = np.array([m.nb - 1, 0, 5, 0], dtype=np.int32)
        part = torch.zeros((len(sl),) + host.shape[1:], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sim.labs_into(part.data_ptr(), fname, w, tensorial=tens, slots=sl)
        check(lib().cup3d_device_synchronize())
        assert np.array_equal(part.cpu().numpy(), host[sl], equal_nan=True)


# ---- 6: a scalar as BlockLabBC<.., direction k>
@pytest.mark.parametrize("name", ["box321_every_bc", "amr_mixed_l12"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_scalar_dir(name, k):
    sim, m, vel, pres = case(name)
    ref = np.zeros((m.nb, 10, 10, 10, 1))
    O.lib().orc_mesh_labs(m.m, np.ascontiguousarray(pres), 1, 2 + k, -1, 2, 0, ref)
    same_tiles(sim.labs("pres", 1, scalar_dir=k), ref, 1, False, (name, "scalar_dir", k))
    mask = O.lab_mask(-1, 2, False)
    assert not np.array_equal(ref[:, mask], m.labs(pres, -1, 2, False)[:, mask])   # ... and it is another tile than the ScalarLab's


# ---- 7: errors and purity
def _refused(sim, field, n, slots, w, tens, sdir, out):
    """Both variants refuse the call with CUP3D_EINVAL and a text of their own and write nothing: the host variant not into `out`,
    the device variant not into a real device buffer of the same size that holds a sentinel."""
    import torch
    L = lib()
    sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.int32).ctypes.data_as(C.c_void_p)
    dev = None if out is None else torch.full((out.size,), 5.0, dtype=torch.float64, device="cuda")
    for fn, dst in ((L.cup3d_sim_labs, None if out is None else out.ctypes.data_as(C.c_void_p)),
                    (L.cup3d_sim_labs_device, None if out is None else C.c_void_p(dev.data_ptr()))):
        check(L.cup3d_sim_fill(sim.handle, FIELDS["lhs"], 0.0))   # a successful call in between: the error text is this call's own
        before = None if out is None else out.copy()
        assert fn(sim.handle, field, n, sl, w, tens, sdir, dst) == EINVAL, (fn.__name__, field, n, w, sdir)
        assert len(L.cup3d_last_error()) > 0
        if out is not None:
            assert np.array_equal(out, before)
    if dev is not None:
        check(L.cup3d_device_synchronize())
        assert bool((dev == 5.0).all())
    return L.cup3d_last_error().decode()


def test_refused_calls():
    sim, m, vel, pres = case("box222_wall")
    nb = m.nb
    out = np.full((nb, 16, 16, 16, 3), 5.0)
    V, P = FIELDS["vel"], FIELDS["pres"]
    for w in (0, 5, -1):
        assert "width" in _refused(sim, V, nb, None, w, 1, -1, out)
    assert "field" in _refused(sim, 99, nb, None, 1, 0, -1, out)
    _refused(sim, V, nb, None, 1, 0, -1, None)                      # null output
    assert "slot" in _refused(sim, V, 2, [0, nb], 1, 0, -1, out)
    assert "slot" in _refused(sim, V, 2, [-1, 0], 1, 0, -1, out)
    assert "vector" in _refused(sim, V, nb, None, 1, 0, 1, out)     # scalar_dir on a vector field
    _refused(sim, P, nb, None, 1, 0, 3, out)                        # no such direction
    _refused(sim, V, nb - 1, None, 1, 0, -1, out)                   # slots = NULL means all blocks
    assert lib().cup3d_sim_labs(None, V, nb, None, 1, 0, -1, out.ctypes.data_as(C.c_void_p)) == EINVAL


def test_rank_view_is_refused():
    """Tiles whose neighbours live on another rank are out of scope: the call says so instead of returning wrong tiles."""
    bpd, lmax, bc = (2, 2, 2), 3, ("wall", "freespace", "wall")
    lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 0, 0, 0), (1, 0, 0, 0)])
    mesh = cu.operators.Grid(bpd, lmax, 0, EXT, bc, leaves=(lv, zs))
    owner = (np.arange(mesh.nblocks) * 2 // mesh.nblocks).astype(np.int32)
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    check(lib().cup3d_debug_virtual_comm(2))   # the in-process communicator of test_gpu_multirank.py: two ranks on one device
    try:
        views = [mesh.rank_view(owner, r, 2) for r in range(2)]
        sims = [cu.SimulationData(view=views[r], **kw) for r in range(2)]
        assert sum(v.nghost for v in views) > 0
        out = np.full((views[0].nlocal, 10, 10, 10, 3), 5.0)
        assert "rank" in _refused(sims[0], FIELDS["vel"], views[0].nlocal, None, 1, 0, -1, out)
        with pytest.raises(cu.capi.Cup3dError):
            sims[1].labs("pres", 1)
        del sims
        gc.collect()
    finally:
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)


def test_labs_read_only_and_leave_the_operators_alone():
    """The tiles are built from the blocks alone: the fields' checksums do not move, the byte count of the host variant is the
    tiles' own, and an operator that builds its ghost slabs behind the same mesh gives the bits it gives without the calls."""
    sim, m, vel, pres = case("amr_mixed_l12")
    before = (sim.checksum("vel"), sim.checksum("pres"))
    st = RunStats()
    check(lib().cup3d_stats_reset())
    sim.labs("vel", 4, tensorial=True)
    sim.labs("pres", 2, slots=[3, 1, 3])
    check(lib().cup3d_stats_read(C.byref(st)))
    assert st.field_bytes_downloaded == m.nb * 16 ** 3 * 3 * 8 + 3 * 12 ** 3 * 8 and st.field_bytes_uploaded == 0
    sim.labs("vel", 1)
    sim.labs("pres", 1, scalar_dir=1)
    assert (sim.checksum("vel"), sim.checksum("pres")) == before
    g = np.load(os.path.join(GOLD, "amr_mixed_l12.npz"))
    bpd, bc, t = tuple(int(b) for b in g["bpd"]), tuple(O.BC_NAMES[int(b)] for b in g["bc"]), g["tables"]
    res = []
    for with_labs in (False, True):
        s = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=int(g["level_max"]), levelStart=0, extent=float(g["extent"]), nu=0.02,
                              BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], uinf=(0.1, -0.2, 0.3), leaves=(t[:, 0], t[:, 1]))
        s.upload("vel", vel)
        if with_labs:
            s.labs("vel", 3)
            s.labs("tmpV", 4, tensorial=True, slots=[0, 2])
        cu.AdvectionDiffusion(s)(0.01)
        res.append(s.download("vel"))
    assert np.array_equal(res[0], res[1])
    assert np.array_equal(res[0], m.advect_diffuse(vel, 0.01, 0.02, (0.1, -0.2, 0.3))[0])


# ---- 8: memory
def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _one_life():
    sim = cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=2, levelStart=1, extent=EXT, BC_x="wall", BC_y="periodic", BC_z="freespace")
    sim.upload("vel", np.random.default_rng(1).uniform(-1, 1, (sim.nblocks, 8, 8, 8, 3)))
    assert sim.labs("vel", 4, tensorial=True).shape == (64, 16, 16, 16, 3)
    assert sim.labs("pres", 1, slots=[5, 5]).shape == (2, 10, 10, 10)
    del sim


def test_destroy_returns_what_labs_allocated():
    """The tables and the 64 MiB staging buffer the first cup3d_sim_labs of a sim allocates go back in cup3d_sim_destroy: after a
    first life (pinned buffers and the event pool are allocated once per process) the free device memory is where it was."""
    _one_life()
    gc.collect()
    before = _free_bytes()
    for _ in range(3):
        _one_life()
        gc.collect()
    after = _free_bytes()
    assert before - after < (8 << 20), f"{(before - after) / 2 ** 20:.1f} MiB of device memory lost over 3 create / labs / destroy cycles"
