"""cup3d_fix_mass_flux (cup3d_amd/csrc/diagnostics.hip) against the restatement of FixMassFlux::operator() (main.cpp:12199-12248) in
tests/dissipation_restatement.py: the five numbers the reference prints and every bit of vel.  MI355X only (-m gpu).

Everything here is exact: the mean is an orderly sum (cells in z, y, x order per block, blocks in slot order), a division, and the update
is one expression per cell in the reference's association -- so the bound is zero, with uinf != 0."""
import ctypes as C

import numpy as np
import pytest

import cup3d_amd as cu
import dissipation_cases as D
from cup3d_amd.capi import check, lib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def loaded(name):
    c = D.case(name)
    sim = cu.SimulationData(uinf=D.UINF, uMax_forced=D.UMAX_FORCED, bFixMassFlux=True, **c.sim_kwargs)
    sim.upload("vel", c.vel)
    return c, sim


@pytest.mark.parametrize("name", D.MASS_FLUX_CASES)
def test_five_numbers_and_every_bit_of_vel(name):
    c, sim = loaded(name)
    want, want_vel = D.expected_mass_flux(name)
    before = sim.device_bytes()
    got = cu.FixMassFlux(sim)(D.DT)
    assert got is sim.mass_flux and set(got) == set(want)
    for k in want:
        assert bits(got[k]) == bits(want[k]), (k, got[k], want[k])
    vel = sim.download("vel")
    assert np.array_equal(bits(vel), bits(want_vel))
    assert np.array_equal(bits(vel[..., 1:]), bits(c.vel[..., 1:]))        # components 1 and 2 untouched
    assert not np.array_equal(vel[..., 0], c.vel[..., 0])                   # ... and component 0 was moved
    assert sim.device_bytes() == before + c.nb * 24 * 8 + 160              # the buffers cup3d_compute_dissipation shares
    cu.FixMassFlux(sim)(D.DT)
    assert sim.device_bytes() == before + c.nb * 24 * 8 + 160


def test_null_out_is_accepted_and_null_arrays_are_not():
    c, sim = loaded("sixteen_mixed")
    _, want_vel = D.expected_mass_flux("sixteen_mixed")
    ext, uinf = np.array(c.extents), np.array(D.UINF)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib().cup3d_fix_mass_flux(sim.handle, D.UMAX_FORCED, D.NU, D.DT, None, p(uinf), None) == -1
    assert lib().cup3d_fix_mass_flux(sim.handle, D.UMAX_FORCED, D.NU, D.DT, p(ext), None, None) == -1
    assert np.array_equal(bits(sim.download("vel")), bits(c.vel))
    check(lib().cup3d_fix_mass_flux(sim.handle, D.UMAX_FORCED, D.NU, D.DT, p(ext), p(uinf), None))
    assert np.array_equal(bits(sim.download("vel")), bits(want_vel))
