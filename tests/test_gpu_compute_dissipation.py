"""cup3d_compute_dissipation (cup3d_amd/csrc/diagnostics.hip) against tests/dissipation_restatement.py fed with the oracle's tiles.
MI355X only (-m gpu).

Stated bounds
  * block_sums[:, 0:19]: BIT FOR BIT the restatement's, signs of zeros included; qoi[0:19]: bit for bit the slot-order totals of the
    device's own rows and of the restatement's.
  * Column 19 holds std::sqrt.  A correctly rounded square root would make it bitwise too; the bound does not assume one.  Per
    block |d| <= (2u + 2 gamma_512) sum|t_i|: each summand hCube * sqrt(s) may differ by a relative 2u between two implementations whose
    square roots are each within one ulp (u = 2^-53), and two orderly sums of 512 terms that are each within gamma_512 sum|t_i| of the
    exact sum of their own summands differ by at most twice that.  For the total the same with gamma_N, N = 512 nb.
    ON THE MI355X COLUMN 19 WAS IN FACT BITWISE in every case, rows and totals (the test prints it per case).
  * Device memory: the first call allocates the geometry table [nb][4] and the rows [nb + 1][20] (the last row holds the rank's
    totals, which the level table does not need: std::pow(h, 3) per level travels as a kernel argument) = nb * (4 + 20) * 8 + 160 bytes;
    a second call allocates nothing and returns identical bits.

Measured on the MI355X, release library, all-periodic random fields, median of 20 calls after warm-up (scripts/dissipation_probe.py):
  256^3 (32 768 blocks): k_dissipation 1.00 ms + k_rows_total 0.53 ms, 1.56 ms the whole call on the host's clock; the algorithmic traffic
  (40 B per cell) over 8 TB/s is 0.084 ms; downloading vel, pres and chi, the path this replaces, takes 65-68 ms.
  512^3 (262 144 blocks): 7.95 ms + 4.1-4.3 ms, 12.1-12.2 ms the call; traffic 0.67 ms; the download 339-387 ms.
The ordered sums dominate by far more than the traffic time; that is accepted."""
import ctypes as C

import numpy as np
import pytest

import cup3d_amd as cu
import dissipation_cases as D
import dissipation_restatement as R
from cup3d_amd.capi import check, lib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
CUP3D_EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def loaded(name):
    c = D.case(name)
    sim = cu.SimulationData(**c.sim_kwargs)
    assert sim.nblocks == c.nb and np.array_equal(sim.grid.tables, c.tables)
    sim.upload("vel", c.vel)
    sim.upload("pres", c.pres)
    if c.chi is not None:
        sim.upload("chi", c.chi)
    return c, sim


@pytest.mark.parametrize("name", list(D.CASES))
def test_rows_and_totals_against_the_restatement(name):
    c, sim = loaded(name)
    before = sim.device_bytes()
    sums = {f: sim.checksum(f) for f in ("vel", "pres", "chi", "tmpV")}
    op = cu.ComputeDissipation(sim)
    qoi = op.compute(block_sums=True).copy()
    rows = sim.diagnostics["block_sums"].copy()
    grown = sim.device_bytes() - before
    assert grown == c.nb * (4 + 20) * 8 + 20 * 8, grown
    want_rows, want_tot, abs_rows = D.expected(name)
    # columns 0..18: every bit
    assert np.array_equal(bits(rows[:, :19]), bits(want_rows[:, :19])), np.argwhere(bits(rows[:, :19]) != bits(want_rows[:, :19]))[:5]
    own = np.array(R.totals(rows))
    assert np.array_equal(bits(qoi[:19]), bits(own[:19]))
    assert np.array_equal(bits(qoi[:19]), bits(want_tot[:19]))
    # column 19: the derived bound; whether it was in fact bitwise is printed
    d_rows = np.abs(rows[:, 19] - want_rows[:, 19])
    bound_rows = (2 * D.U + 2 * D.gamma(512)) * abs_rows[:, 19]
    print(f"{name}: column 19 bitwise rows={np.array_equal(bits(rows[:, 19]), bits(want_rows[:, 19]))} total={bits(qoi[19:]) == bits(want_tot[19:])} "
          f"max |d|/bound = {float((d_rows / bound_rows).max()):.3g}")
    assert (d_rows <= bound_rows).all()
    assert bits(qoi[19:]) == bits(own[19:])   # the total of the device's own column is an orderly sum of doubles: bitwise whatever sqrt does
    assert abs(qoi[19] - want_tot[19]) <= (2 * D.U + 2 * D.gamma(512 * c.nb)) * abs_rows[:, 19].sum()
    # a second call: identical bits, no growth, nothing else touched
    qoi2 = op.compute(block_sums=True)
    assert np.array_equal(bits(qoi2), bits(qoi)) and np.array_equal(bits(sim.diagnostics["block_sums"]), bits(rows))
    assert sim.device_bytes() == before + grown
    assert {f: sim.checksum(f) for f in sums} == sums


def test_one_block_is_the_reference_with_one_thread():
    """one running sum per quantity over all cells, the reference's one-thread association, in float64: the device's totals bit for bit"""
    c, sim = loaded("one_block")
    qoi = cu.ComputeDissipation(sim).compute()
    q, _, n = R.one_thread(c.vel_labs, c.pres_labs, D.chi_of(c), c.geom, c.extents, D.NU, dtype=np.float64)
    assert n == 512 and np.array_equal(bits(qoi[:19]), bits(np.array(q[:19], dtype=np.float64)))


def test_without_block_sums_and_null_arguments():
    c, sim = loaded("three_blocks")
    want = D.expected("three_blocks")[1]
    qoi = cu.ComputeDissipation(sim).compute()
    assert "block_sums" not in sim.diagnostics and np.array_equal(bits(qoi[:19]), bits(want[:19]))
    ext = np.array(c.extents)
    out = np.full(20, 7.0)
    before, sums = sim.device_bytes(), {f: sim.checksum(f) for f in ("vel", "pres", "chi", "tmpV")}
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib().cup3d_compute_dissipation(sim.handle, D.NU, p(ext), None, None) == CUP3D_EINVAL
    assert lib().cup3d_compute_dissipation(sim.handle, D.NU, None, p(out), None) == CUP3D_EINVAL
    assert lib().cup3d_compute_dissipation(None, D.NU, p(ext), p(out), None) == CUP3D_EINVAL
    assert (out == 7.0).all() and sim.device_bytes() == before and {f: sim.checksum(f) for f in sums} == sums
    fresh = cu.SimulationData(**c.sim_kwargs)   # ... and on a sim that never made the call, nothing is allocated either
    b0 = fresh.device_bytes()
    assert lib().cup3d_compute_dissipation(fresh.handle, D.NU, p(ext), None, None) == CUP3D_EINVAL and fresh.device_bytes() == b0
    check(lib().cup3d_compute_dissipation(fresh.handle, D.NU, p(ext), p(out), None))
    assert fresh.device_bytes() == b0 + c.nb * 24 * 8 + 160
