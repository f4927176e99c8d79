"""cup3d_sim_labs_over_ranks / cup3d_sim_labs_over_ranks_device: ghosted block tiles on a mesh spread over ranks (k_labs_view and the
request / data exchange of csrc/labs.hip, the request plan of Grid::lab_boxes), on ONE GPU: the ranks are host threads of this process
and the in-process communicator (cup3d_debug_virtual_comm) stands in for RCCL, as in test_gpu_multirank.py.  MI355X only (-m gpu).

A tile does not depend on how the mesh is partitioned: the expected tiles are the CPU oracle's (OracleMesh.labs, pinned to the compiled
reference by test_oracle_amr.py and test_oracle_wide_labs.py) of the GLOBAL mesh with the global field, restricted to the rank's
blocks.  Everything is bit-exact: equal on the cells the reference defines (oracle_lib.lab_mask), NaN on the others.  The whole module
runs with `poison_ghosts`: every cell of the ghost pool that did not travel is NaN, so a tile that reads outside the box its rank asked
for turns a test red.  tests/test_labs_over_ranks_cases.py (no GPU) shows that the owner maps used here cross every class of neighbour."""
import ctypes as C
import gc
import threading
import time

import numpy as np
import pytest

import cup3d_amd as cu
import labs_ranks_cases as LC
import oracle_lib as O
from cup3d_amd.capi import RunStats, check, lib
from cup3d_amd.operators import FIELDS

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _poison_the_cells_that_are_not_shipped():
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


def same_tiles(got, ref, w, tens, what):
    """got [n, L, L, L(, nc)] equals ref [n, L, L, L, nc] bit for bit on lab_mask and is NaN off it"""
    got = got.reshape(ref.shape)
    mask = O.lab_mask(-w, w + 1, tens)
    bad = got[:, mask] != ref[:, mask]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} defined cells differ, max |d| = {np.abs(got[:, mask] - ref[:, mask]).max():.3g}"
    assert np.isnan(got[:, ~mask]).all(), f"{what}: a cell the reference leaves undefined is not NaN"
    assert not np.isnan(got[:, mask]).any(), what


class Case:
    """A global mesh with seeded global vel / pres and the oracle's tiles of them, computed once per (field, box) and never modified."""

    def __init__(self, name, bpd, lmax, bc, ext, lv, zs):
        self.name, self.bpd, self.lmax, self.bc, self.ext = name, bpd, lmax, bc, ext
        self.mesh = cu.operators.Grid(bpd, lmax, 0, ext, bc, leaves=(lv, zs))
        t = self.mesh.tables
        self.m = O.OracleMesh(bpd, lmax, ext, bc, t[:, 0], t[:, 1])
        assert np.array_equal(self.m.tables, t)   # same blocks in the same order on both sides
        self.nb = self.mesh.nblocks
        rng = np.random.default_rng(len(name))
        self.f = dict(vel=rng.uniform(-1, 1, (self.nb, 8, 8, 8, 3)), pres=rng.uniform(-1, 1, (self.nb, 8, 8, 8)))
        self.kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
        self._ref = {}

    def ref(self, fname, w, tens):
        if (fname, w, tens) not in self._ref:
            self._ref[(fname, w, tens)] = self.m.labs(self.f[fname], -w, w + 1, tens)
        return self._ref[(fname, w, tens)]

    def view_sims(self, owner, nranks, **more):
        """this mesh spread over ranks: (views, sims with vel / pres of their blocks uploaded, the global slots of each rank's blocks)"""
        views = [self.mesh.rank_view(owner, r, nranks) for r in range(nranks)]
        sims = [cu.SimulationData(view=views[r], levelStart=0, **self.kw, **more) for r in range(nranks)]
        mine = [v.global_slot[:v.nlocal] for v in views]
        for r, s in enumerate(sims):
            assert np.array_equal(mine[r], np.where(owner == r)[0])
            s.upload("vel", self.f["vel"][mine[r]])
            s.upload("pres", self.f["pres"][mine[r]])
        return views, sims, mine


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name, *LC.mesh_recipe(name))
    return _cases[name]


def gather(c, sims, mine, owner, combos):
    """every rank asks for all its blocks, for every (field, w, tensorial) of combos in turn; the tiles, gathered in global order"""
    got = [dict() for _ in sims]

    def rank(r):
        for fname, w, tens in combos:
            got[r][(fname, w, tens)] = sims[r].labs_over_ranks(fname, w, c.mesh, owner, tensorial=tens)

    run_ranks(rank, len(sims))
    out = {}
    for k in combos:
        ref = c.ref(*k)
        full = np.zeros_like(ref)
        for r in range(len(sims)):
            full[mine[r]] = got[r][k].reshape((len(mine[r]),) + ref.shape[1:])
        out[k] = full
    return out


# ---- 1: multi-level meshes, every owner map
@pytest.mark.parametrize("kind,nranks,seed", LC.MAPS)
@pytest.mark.parametrize("name", LC.MESHES)
def test_tiles_equal_the_oracle_on_every_owner_map(name, kind, nranks, seed):
    c = case(name)
    assert len(set(c.mesh.tables[:, 0].tolist())) >= 2
    owner = LC.owners(c.nb, kind, nranks, seed)
    widths = (1, 2, 3, 4) if (kind, nranks, seed) == LC.ALL_WIDTHS_MAP else (1, 4)
    combos = [(fname, w, tens) for w in widths for tens in (False, True) for fname in ("vel", "pres")]
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)
        assert sum(v.nghost for v in views) > 0
        got = gather(c, sims, mine, owner, combos)
        del sims, views
        gc.collect()
    for k in combos:
        same_tiles(got[k], c.ref(*k), k[1], k[2], (name, kind, nranks) + k)


# ---- 2: one rank's share of a uniform grid
_uniform = {}


def uniform_case():
    if not _uniform:
        bpd, lmax, level, bc = (2, 2, 2), 2, 1, ("periodic", "wall", "freespace")
        whole = cu.operators.Grid(bpd, lmax, level, LC.EXT, bc)
        c = Case("uniform64", bpd, lmax, bc, LC.EXT, whole.tables[:, 0].astype(np.int32), whole.tables[:, 1].copy())
        assert c.nb == 64
        _uniform["c"] = (c, level)
    return _uniform["c"]


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_uniform_share(nranks):
    c, level = uniform_case()
    mesh, owner = cu.operators.uniform_share_mesh(c.bpd, c.lmax, level, c.ext, c.bc, nranks)
    assert np.array_equal(mesh.tables, c.mesh.tables)
    combos = [(fname, w, tens) for w in (1, 3, 4) for fname, tens in (("vel", True), ("pres", False))]
    got = [dict() for _ in range(nranks)]
    with VirtualComm(nranks):
        sims = [cu.SimulationData(rank=r, nranks=nranks, levelStart=level, **c.kw) for r in range(nranks)]
        mine = [np.where(owner == r)[0] for r in range(nranks)]
        for r, s in enumerate(sims):
            s.upload("vel", c.f["vel"][mine[r]])
            s.upload("pres", c.f["pres"][mine[r]])

        def rank(r):
            for fname, w, tens in combos:
                got[r][(fname, w, tens)] = sims[r].labs_over_ranks(fname, w, mesh, owner, tensorial=tens)

        run_ranks(rank, nranks)
        del sims
        gc.collect()
    for k in combos:
        ref = c.ref(*k)
        full = np.zeros_like(ref)
        for r in range(nranks):
            full[mine[r]] = got[r][k].reshape((len(mine[r]),) + ref.shape[1:])
        same_tiles(full, ref, k[1], k[2], ("uniform share", nranks) + k)


# ---- 3: slot lists and uneven requests
def test_slot_lists_and_uneven_requests():
    c = case("amr_mixed_l12")
    kind, nranks, seed = LC.MAPS[2]
    owner = LC.owners(c.nb, kind, nranks, seed)
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)
        n0 = views[0].nlocal
        short = np.array([n0 - 1, 0, n0 // 2, 0, n0 - 1], dtype=np.int32)   # short, unordered, repeated
        asks = [short, np.zeros(0, dtype=np.int32), None]   # rank 1 needs nothing, rank 2 everything
        for fname, w, tens in (("vel", 4, True), ("pres", 1, False), ("vel", 2, False)):
            got = [None] * nranks

            def rank(r):
                got[r] = sims[r].labs_over_ranks(fname, w, c.mesh, owner, tensorial=tens, slots=asks[r])

            run_ranks(rank, nranks)
            ref = c.ref(fname, w, tens)
            same_tiles(got[0], ref[mine[0]][short], w, tens, ("short list", fname, w, tens))
            assert got[1].shape[0] == 0
            same_tiles(got[2], ref[mine[2]], w, tens, ("everything", fname, w, tens))
            # ... and nobody needs anything: the call still returns on every rank
            none = [None] * nranks

            def rank0(r):
                none[r] = sims[r].labs_over_ranks(fname, w, c.mesh, owner, tensorial=tens, slots=[])

            run_ranks(rank0, nranks)
            assert all(a.shape[0] == 0 for a in none)
        del sims, views
        gc.collect()


# ---- 4: a scalar as BlockLabBC<.., direction k>
@pytest.mark.parametrize("k", [0, 1, 2])
def test_scalar_dir(k):
    c = case("amr_mixed_l12")
    kind, nranks, seed = LC.MAPS[2]
    owner = LC.owners(c.nb, kind, nranks, seed)
    pres = c.f["pres"]
    ref = np.zeros((c.nb, 10, 10, 10, 1))
    O.lib().orc_mesh_labs(c.m.m, np.ascontiguousarray(pres), 1, 2 + k, -1, 2, 0, ref)
    got = [None] * nranks
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)

        def rank(r):
            got[r] = sims[r].labs_over_ranks("pres", 1, c.mesh, owner, scalar_dir=k)

        run_ranks(rank, nranks)
        del sims, views
        gc.collect()
    full = np.zeros_like(ref)
    for r in range(nranks):
        full[mine[r]] = got[r].reshape((len(mine[r]),) + ref.shape[1:])
    same_tiles(full, ref, 1, False, ("scalar_dir", k))
    mask = O.lab_mask(-1, 2, False)
    assert not np.array_equal(ref[:, mask], c.ref("pres", 1, False)[:, mask])   # ... and it is another tile than the ScalarLab's


# ---- 5: the device variant
def test_device_variant_equals_the_host_variant():
    import torch
    c = case("amr_mixed_l12")
    kind, nranks, seed = LC.MAPS[2]
    owner = LC.owners(c.nb, kind, nranks, seed)
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)
        for fname, w, tens in (("vel", 4, True), ("pres", 1, False)):
            sl = [np.array([len(mine[r]) - 1, 0, 0], dtype=np.int32) for r in range(nranks)]
            host, part_host = [None] * nranks, [None] * nranks

            def rank_host(r):
                host[r] = sims[r].labs_over_ranks(fname, w, c.mesh, owner, tensorial=tens)
                part_host[r] = sims[r].labs_over_ranks(fname, w, c.mesh, owner, tensorial=tens, slots=sl[r])

            run_ranks(rank_host, nranks)
            dev = [torch.full(host[r].shape, 7.0, dtype=torch.float64, device="cuda") for r in range(nranks)]
            part = [torch.full(part_host[r].shape, 7.0, dtype=torch.float64, device="cuda") for r in range(nranks)]
            torch.cuda.synchronize()

            def rank_dev(r):
                assert sims[r].labs_over_ranks_into(dev[r].data_ptr(), fname, w, c.mesh, owner, tensorial=tens) == host[r].shape
                sims[r].labs_over_ranks_into(part[r].data_ptr(), fname, w, c.mesh, owner, tensorial=tens, slots=sl[r])

            run_ranks(rank_dev, nranks)
            check(lib().cup3d_device_synchronize())   # the device variant's tiles are stream-ordered on the library's stream
            for r in range(nranks):
                assert np.array_equal(dev[r].cpu().numpy(), host[r], equal_nan=True)
                assert np.array_equal(part[r].cpu().numpy(), part_host[r], equal_nan=True)
                assert np.array_equal(part_host[r], host[r][sl[r]], equal_nan=True)
        del sims, views
        gc.collect()


# ---- 6: only what the tiles read travels
def test_bytes_sent():
    c = case("l012_box322")
    kind, nranks, seed = LC.MAPS[2]
    owner = LC.owners(c.nb, kind, nranks, seed)
    reads = LC.neighbour_reads(c.mesh.tables, c.mesh.interface()[2], c.bpd)
    pairs = {(int(owner[b]), n) for b, _, _, n in reads if owner[b] != owner[n]}   # (rank, remote block) the tiles read
    lonely = next(b for b, _, _, n in reads if owner[b] == 0 and owner[n] != 0)    # a block of rank 0 with a remote neighbour
    st = RunStats()

    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)

        def sent(asks, w):
            check(lib().cup3d_stats_reset())
            run_ranks(lambda r: sims[r].labs_over_ranks("vel", w, c.mesh, owner, tensorial=True, slots=asks[r]), nranks)
            check(lib().cup3d_stats_read(C.byref(st)))
            return st.halo_bytes_sent

        nothing = sent([[]] * nranks, 4)
        one = sent([[int(np.where(mine[0] == lonely)[0][0])]] + [[]] * (nranks - 1), 4)
        all1 = sent([None] * nranks, 1)
        all4 = sent([None] * nranks, 4)
        del sims, views
        gc.collect()
    whole = 512 * 3 * 8 * len(pairs)
    print(f"halo_bytes_sent: nobody asks {nothing:.0f}, one block {one:.0f}, all tiles w=1 {all1:.0f}, all tiles w=4 {all4:.0f}; "
          f"whole blocks for the {len(pairs)} (rank, remote block) pairs {whole}")
    assert nothing < one < all1 < all4 < whole


# ---- 7: one bad rank fails everyone
@pytest.mark.parametrize("what", ["width", "slot"])
def test_a_bad_call_on_one_rank_fails_on_every_rank_at_once(what):
    c = case("l012_wall")
    nranks, bad_rank = 3, 1
    owner = LC.owners(c.nb, "ranges", nranks, 0)
    codes, texts, took = [None] * nranks, [None] * nranks, [None] * nranks
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)
        before = [(s.checksum("vel"), s.checksum("pres")) for s in sims]
        outs = [np.full((len(mine[r]), 10, 10, 10, 3), 5.0) for r in range(nranks)]

        def call(r, bad):
            n, sl, w = len(mine[r]), None, 1
            if bad and what == "width":
                w = 5
            if bad and what == "slot":
                n, sl = 2, np.array([0, len(mine[r])], dtype=np.int32)
            return lib().cup3d_sim_labs_over_ranks(sims[r].handle, c.mesh.handle, owner.ctypes.data_as(C.c_void_p), FIELDS["vel"], n,
                                                   None if sl is None else sl.ctypes.data_as(C.c_void_p), w, 0, -1, outs[r].ctypes.data_as(C.c_void_p))

        def rank(r):
            t0 = time.time()
            codes[r] = call(r, r == bad_rank)
            texts[r] = lib().cup3d_last_error().decode()
            took[r] = time.time() - t0

        run_ranks(rank, nranks)
        assert all(code == EINVAL for code in codes), codes
        assert max(took) < 5.0, took
        assert what in texts[bad_rank]
        assert all("another rank could not take part" in texts[r] for r in range(nranks) if r != bad_rank), texts
        assert all((o == 5.0).all() for o in outs)                                         # nothing has been touched
        assert [(s.checksum("vel"), s.checksum("pres")) for s in sims] == before
        ok = [None] * nranks

        def again(r):
            ok[r] = call(r, False)

        run_ranks(again, nranks)   # the communicator is not left half-way through an exchange
        assert ok == [0] * nranks, ok
        ref = c.ref("vel", 1, False)
        for r in range(nranks):
            same_tiles(outs[r], ref[mine[r]], 1, False, ("after the refused call", r))
        del sims, views
        gc.collect()


def test_bad_arguments_every_rank_can_find():
    """NULL mesh / owner, a rank view in the mesh's place, an owner out of range, a sim that holds other blocks than the rank's leaves:
    refused on every rank (all ranks make the same mistake here), and a correct call works afterwards."""
    c = case("l012_wall")
    nranks = 2
    owner = LC.owners(c.nb, "ranges", nranks, 0)
    wrong = owner.copy()
    wrong[[int(np.where(owner == 0)[0][0]), int(np.where(owner == 1)[0][0])]] = [1, 0]   # same counts, other blocks
    far = owner.copy()
    far[0] = nranks
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)
        assert sorted((wrong == r).sum() for r in range(nranks)) == sorted(len(m) for m in mine)

        def attempt(mesh_handle, ow):
            codes, texts = [None] * nranks, [None] * nranks
            outs = [np.full((len(mine[r]), 10, 10, 10), 5.0) for r in range(nranks)]

            def rank(r):
                codes[r] = lib().cup3d_sim_labs_over_ranks(sims[r].handle, mesh_handle, None if ow is None else ow.ctypes.data_as(C.c_void_p), FIELDS["pres"],
                                                           len(mine[r]), None, 1, 0, -1, outs[r].ctypes.data_as(C.c_void_p))
                texts[r] = lib().cup3d_last_error().decode()

            run_ranks(rank, nranks)
            return codes, texts, outs

        for mh, ow, word in ((None, owner, "null"), (c.mesh.handle, None, "null"), (views[0].handle, owner, "GLOBAL"), (c.mesh.handle, far, "owner"),
                             (c.mesh.handle, wrong, "leaves")):
            codes, texts, outs = attempt(mh, ow)
            assert codes == [EINVAL] * nranks, (word, codes)
            assert any(word in t for t in texts), (word, texts)
            assert all((o == 5.0).all() for o in outs)
        codes, texts, outs = attempt(c.mesh.handle, owner)
        assert codes == [0] * nranks, texts
        for r in range(nranks):
            same_tiles(outs[r], c.ref("pres", 1, False)[mine[r]], 1, False, ("after the refused calls", r))
        del sims, views
        gc.collect()


# ---- 8: one rank
def test_one_rank_equals_cup3d_sim_labs():
    c = case("amr_mixed_l12")
    sim = cu.SimulationData(leaves=(c.mesh.tables[:, 0].astype(np.int32), c.mesh.tables[:, 1].copy()), levelStart=0, **c.kw)
    sim.upload("vel", c.f["vel"])
    sim.upload("pres", c.f["pres"])
    owner = np.zeros(c.nb, dtype=np.int32)
    for fname, w, tens, sl in (("vel", 4, True, None), ("pres", 1, False, None), ("vel", 2, False, [5, 0, 5]), ("pres", 3, True, [c.nb - 1])):
        assert np.array_equal(sim.labs_over_ranks(fname, w, c.mesh, owner, tensorial=tens, slots=sl), sim.labs(fname, w, tensorial=tens, slots=sl), equal_nan=True)
    u, level = uniform_case()
    mesh, ow = cu.operators.uniform_share_mesh(u.bpd, u.lmax, level, u.ext, u.bc, 1)
    one = cu.SimulationData(levelStart=level, **u.kw)
    one.upload("vel", u.f["vel"])
    assert np.array_equal(one.labs_over_ranks("vel", 4, mesh, ow, tensorial=True), one.labs("vel", 4, tensorial=True), equal_nan=True)


# ---- 9: read-only, and what destroy gives back
def test_read_only_and_leaves_the_operators_alone():
    c = case("l012_box322")
    kind, nranks, seed = LC.MAPS[2]
    owner = LC.owners(c.nb, kind, nranks, seed)
    dt, nu, uinf = 0.01, 0.02, (0.1, -0.2, 0.3)
    res = []
    for with_labs in (False, True):
        out = np.zeros_like(c.f["vel"])
        with VirtualComm(nranks):
            views, sims, mine = c.view_sims(owner, nranks, nu=nu, uinf=uinf)
            before = [(s.checksum("vel"), s.checksum("pres")) for s in sims]

            def tiles(r):
                sims[r].labs_over_ranks("vel", 3, c.mesh, owner)
                sims[r].labs_over_ranks("pres", 4, c.mesh, owner, tensorial=True, slots=[0, len(mine[r]) - 1, 0])
                sims[r].labs_over_ranks("vel", 1, c.mesh, owner, slots=[])

            def step(r):
                cu.AdvectionDiffusion(sims[r])(dt)
                out[mine[r]] = sims[r].download("vel")

            if with_labs:
                run_ranks(tiles, nranks)
                assert [(s.checksum("vel"), s.checksum("pres")) for s in sims] == before
            run_ranks(step, nranks)
            del sims, views
            gc.collect()
        res.append(out)
    assert np.array_equal(res[0], res[1])
    assert np.array_equal(res[0], c.m.advect_diffuse(c.f["vel"], dt, nu, uinf)[0])


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _one_life():
    c = case("amr_mixed_l12")
    nranks = 2
    owner = LC.owners(c.nb, "ranges", nranks, 0)
    with VirtualComm(nranks):
        views, sims, mine = c.view_sims(owner, nranks)

        def rank(r):
            assert sims[r].labs_over_ranks("vel", 4, c.mesh, owner, tensorial=True).shape == (len(mine[r]), 16, 16, 16, 3)
            assert sims[r].labs_over_ranks("pres", 1, c.mesh, owner, slots=[1, 1]).shape == (2, 10, 10, 10)

        run_ranks(rank, nranks)
        del sims, views
        gc.collect()


def test_destroy_returns_what_the_calls_allocated():
    """The cached view's tables, the exchange buffers, the ghost pool and the staging buffer go back in cup3d_sim_destroy: after a first
    life (pinned buffers and the event pool are allocated once per process) the free device memory is where it was."""
    _one_life()
    gc.collect()
    before = _free_bytes()
    for _ in range(3):
        _one_life()
        gc.collect()
    after = _free_bytes()
    assert before - after < (8 << 20), f"{(before - after) / 2 ** 20:.1f} MiB of device memory lost over 3 create / labs_over_ranks / destroy cycles"
