"""k_loop2_cg_w5: the second fused BiCGSTAB loop kernel of uniform grids held to 5 wavefronts per SIMD (poisson_loops.hpp).  Launches of
>= kLoop2FiveWavesFrom blocks take it instead of k_loop2_cg_w4.  It is a body of its own (loop2_cg5_body), written so that the plane loop
fits 96 registers, but per cell it is the same arithmetic in the same order with the same stores and the same per-block sums: every vector,
hence every iterate, the iteration count and the returned pressure, are the same BITS.  No test grid reaches the production threshold,
hence the testing build's `loop2_five_waves`: 1 = always, 2 = never.  MI355X only (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import cup3d_amd as cu
import oracle_lib as O
from cup3d_amd.capi import check, lib
from test_gpu_multirank import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
EXT = 2 * np.pi
WALL = ("wall", "wall", "wall")


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


class five_waves:
    """`loop2_five_waves` = opt for the body of the with-statement; back to the production choice behind it"""

    def __init__(self, opt):
        self.opt = opt

    def __enter__(self):
        check(lib().cup3d_debug_set_option(b"loop2_five_waves", self.opt))

    def __exit__(self, *a):
        check(lib().cup3d_debug_set_option(b"loop2_five_waves", 0))


def fused_iteration_sums(sim):
    sums = (C.c_ulonglong * 18)()
    check(lib().cup3d_poisson_path_checksum(sim.handle, 0, 1, sums))
    return [int(v) for v in sums]


@pytest.mark.parametrize("bpd,lmax,level,bc", [
    ((1, 1, 1), 2, 1, WALL),                            # 16^3: 8 blocks, every one with three domain faces
    ((1, 1, 1), 3, 2, WALL),                            # 32^3: 64 blocks -- interior, face, edge and corner blocks
    ((2, 1, 1), 2, 1, ("periodic", "wall", "periodic")),   # 32 x 16 x 16: the periodic neighbour slots of tile_issue_faces
])
def test_one_fused_iteration_is_bit_identical(bpd, lmax, level, bc):
    """the 18 solver vectors after ONE iteration's kernels as the solver launches them (mean-constraint row 1, hand-set scalars)"""
    sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=level, extent=EXT, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    res = {}
    for opt in (1, 2):
        with five_waves(opt):
            res[opt] = fused_iteration_sums(sim)
    assert len(set(res[1])) > 1
    assert res[1] == res[2], [(i, a, b) for i, (a, b) in enumerate(zip(res[1], res[2])) if a != b]


@pytest.fixture(scope="module")
def taylor_green_32():
    o = O.OracleGrid((1, 1, 1), 3, 2, EXT, WALL)
    return o.to_global(o.taylor_green([EXT] * 3, 1.0))


@pytest.mark.parametrize("mc", [0, 1, 2, 3])
def test_one_whole_solve_is_bit_identical(mc, taylor_green_32):
    """32^3 all-wall Taylor-Green, the projection of step 21 (second-order pressure path): the corner-row selects of tile_lhs<0> (modes 1
    and 3) and the add_mean path (mode 2) over a whole solve -- iteration count, restart count and every bit of pressure and velocity"""
    res = {}
    for opt in (1, 2):
        with five_waves(opt):
            sim = cu.SimulationData(bpdx=1, bpdy=1, bpdz=1, levelMax=3, levelStart=2, extent=EXT, nu=0.01, BC_x="wall", BC_y="wall", BC_z="wall",
                                    bMeanConstraint=mc)
            sim.upload("vel", sim.grid.to_blocks(taylor_green_32))
            sim.fill("pres", 0.0)
            sim.step = 21
            r = cu.PressureProjection(sim)(0.3 * sim.grid.h)
            res[opt] = (r.iterations, r.restarts, sim.download("pres"), sim.download("vel"))
    print("iterations", res[1][0], "restarts", res[1][1])
    assert res[1][0] > 3 and res[1][:2] == res[2][:2], (res[1][:2], res[2][:2])
    assert np.array_equal(res[1][2], res[2][2]) and np.array_equal(res[1][3], res[2][3])


def test_one_fused_iteration_over_two_ranks_is_bit_identical():
    """32^3 over two thread ranks (the in-process communicator): the faces towards the other rank come from the halo slabs (n >= kNbrHalo in
    tile_issue_faces) and the launch is split into inner and boundary blocks; every rank's 18 sums"""
    nranks = 2
    res = {}
    for opt in (1, 2):
        with five_waves(opt), VirtualComm(nranks):
            sims = [cu.SimulationData(rank=r, nranks=nranks, bpdx=1, bpdy=1, bpdz=1, levelMax=3, levelStart=2, extent=EXT,
                                      BC_x="wall", BC_y="wall", BC_z="wall") for r in range(nranks)]
            assert sum(s.nblocks for s in sims) == 64 and all(s.nblocks for s in sims)
            out = [None] * nranks

            def rank(r):
                out[r] = fused_iteration_sums(sims[r])

            run_ranks(rank, nranks)
            res[opt] = out
            del sims
    assert res[1][0] != res[1][1]
    assert res[1] == res[2]
