"""cup3d_sim_device_bytes at fixed checkpoints of three small sims, against constants.  The ledger is kept by the owners of
csrc/devmem.hpp: an allocation is counted if and only if its call site names the Sim, so a buffer that starts or stops being counted, or
is counted by another amount or at another moment, moves one of these numbers.  MI355X only (-m gpu).

The retained obstacle set and the resident plan are not repeated here: tests/test_gpu_resident_obstacles.py and
tests/test_gpu_prevent_colliding.py hold their formulas.

EXPECTED holds what this file's MEASURE functions return with the library of the commit BEFORE the owners existed (hand-kept
`s->bytes +=` lines) on an MI355X; it does not come from the code under test."""
import gc
import threading

import numpy as np
import pytest

import cup3d_amd as cu
import labs_ranks_cases as LC
from cup3d_amd.capi import check, lib

pytestmark = pytest.mark.gpu
EXT = 2 * np.pi
BC = ("periodic", "wall", "freespace")
UNIFORM = dict(bpdx=1, bpdy=1, bpdz=1, levelMax=3, extent=EXT, BC_x=BC[0], BC_y=BC[1], BC_z=BC[2])   # level 2: 64 blocks
AMR = "amr_periodic_l01"   # the smallest two-level mesh of the AMR tests (tests/golden)
SOLVERS = (0, 1, 5)


def run_ranks(fn, nranks):
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


def _fields(nb, seed):
    rng = np.random.default_rng(seed)
    rhs = rng.uniform(-1, 1, (nb, 8, 8, 8))
    return rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rhs - rhs.mean()


def _surface(nb):
    """two blocks with one and two surface points: enough for the tile scratch and every staged array of cup3d_compute_forces"""
    slots = [0, nb - 1]
    return cu.ObstacleSurface(slots, [0, 1, 3], [[3, 3, 3], [4, 4, 4], [1, 6, 2]], np.full((3, 3), 0.25), np.zeros((2, 8, 8, 8, 3)), (1.0, 1.0, 1.0), (0.1, 0.0, 0.0),
                              (0.0, 0.0, 0.1))


def _one_rank(make, mesh, owner):
    """the checkpoints of a sim on one rank; make() -> a fresh sim"""
    import torch
    out = {}
    sim = make()
    nb = sim.nblocks
    vel, rhs = _fields(nb, 5)
    out["create"] = sim.device_bytes()
    sim.upload("vel", vel)
    out["upload"] = sim.device_bytes()
    sim.upload("pres", rhs)
    assert sim.device_bytes() == out["upload"]   # the staging area is made once
    for k in SOLVERS:
        s = make()
        s.blockSolver = k
        s.upload("lhs", rhs)
        cu.makePoissonSolver(s).solve()
        out[f"solve_{k}"] = s.device_bytes()
    s = make()
    s.upload("vel", vel)
    s.labs("vel", 1)
    out["labs_host"] = s.device_bytes()
    s = make()
    s.upload("vel", vel)
    dst = torch.zeros((nb, 10, 10, 10, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.labs_into(dst.data_ptr(), "vel", 1)
    check(lib().cup3d_device_synchronize())
    out["labs_device"] = s.device_bytes()
    s = make()
    s.upload("vel", vel)
    s.labs_over_ranks("vel", 1, mesh, owner)
    out["labs_over_ranks"] = s.device_bytes()
    s = make()
    s.upload("vel", vel)
    s.surfaces = [_surface(nb)]
    cu.ComputeForces(s)(0)
    out["compute_forces"] = s.device_bytes()
    del sim, s, dst
    gc.collect()
    return out


def measure_uniform():
    mesh, owner = cu.operators.uniform_share_mesh((1, 1, 1), 3, 2, EXT, BC, 1)
    return _one_rank(lambda: cu.SimulationData(levelStart=2, **UNIFORM), mesh, owner)


def measure_amr():
    bpd, lmax, bc, ext, lv, zs = LC.mesh_recipe(AMR)
    assert len(set(lv.tolist())) == 2
    mesh = cu.operators.Grid(bpd, lmax, 0, ext, bc, leaves=(lv, zs))
    kw = dict(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=0, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    return _one_rank(lambda: cu.SimulationData(leaves=(lv, zs), **kw), mesh, np.zeros(mesh.nblocks, dtype=np.int32))


def measure_two_ranks():
    """the uniform grid as a share of two thread ranks: [rank 0, rank 1] per checkpoint.  No labs_host / labs_device here: cup3d_sim_labs
    refuses a sim that holds one rank's share (labs_check, csrc/labs.hip); its tiles come from cup3d_sim_labs_over_ranks."""
    n = 2
    mesh, owner = cu.operators.uniform_share_mesh((1, 1, 1), 3, 2, EXT, BC, n)
    out = {}

    def make():
        return [cu.SimulationData(rank=r, nranks=n, levelStart=2, **UNIFORM) for r in range(n)]

    def note(key, sims):
        out[key] = [s.device_bytes() for s in sims]

    check(lib().cup3d_debug_virtual_comm(n))
    try:
        sims = make()
        f = [_fields(s.nblocks, 5 + r) for r, s in enumerate(sims)]
        note("create", sims)
        for r, s in enumerate(sims):
            s.upload("vel", f[r][0])
        note("upload", sims)
        for k in SOLVERS:
            ss = make()
            for r, s in enumerate(ss):
                s.blockSolver = k
                s.upload("lhs", f[r][1])
            run_ranks(lambda r: cu.makePoissonSolver(ss[r]).solve(), n)
            note(f"solve_{k}", ss)
        run_ranks(lambda r: sims[r].labs_over_ranks("vel", 1, mesh, owner), n)
        note("labs_over_ranks", sims)
        ss = make()
        for r, s in enumerate(ss):
            s.upload("vel", f[r][0])
            s.surfaces = [_surface(s.nblocks)]
        run_ranks(lambda r: cu.ComputeForces(ss[r])(0, mesh, owner), n)
        note("compute_forces", ss)
        del sims, ss, s
        gc.collect()
    finally:
        lib().cup3d_device_synchronize()
        lib().cup3d_debug_virtual_comm(0)
    return out


MEASURE = dict(uniform=measure_uniform, amr=measure_amr, two_ranks=measure_two_ranks)

# bytes; the parent commit's library (see the module docstring)
EXPECTED = {
    "uniform": {
        "create": 3670656, "upload": 5243776, "solve_0": 9966144, "solve_1": 9966144, "solve_5": 10338880, "labs_host": 72394464,
        "labs_device": 5285600, "labs_over_ranks": 6801178, "compute_forces": 5573272
    },
    "amr": {
        "create": 1245552, "upload": 1614252, "solve_0": 2721204, "solve_1": 2721204, "solve_5": 2930612, "labs_host": 68763852,
        "labs_device": 1654988, "labs_over_ranks": 1994566, "compute_forces": 1942660
    },
    "two_ranks": {
        "create": [2261376, 2261376], "upload": [3047936, 3047936], "solve_0": [5409216, 5409216], "solve_1": [5409216, 5409216],
        "solve_5": [5589440, 5589440], "labs_over_ranks": [4326880, 4326880], "compute_forces": [3541728, 3541728]
    },
}


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


@pytest.mark.parametrize("kind", sorted(MEASURE))
def test_device_bytes_at_the_checkpoints(kind):
    got = MEASURE[kind]()
    print(kind, got)
    assert got == EXPECTED[kind]
