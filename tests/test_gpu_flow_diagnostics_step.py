"""ComputeDissipation and FixMassFlux as entries of the Python pipeline (cup3d_amd/operators.py; setupOperators, main.cpp:15229-15246).
MI355X only (-m gpu)."""
import numpy as np
import pytest

import cup3d_amd as cu
import oracle_lib as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
EXT = 2 * np.pi


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


def taylor_green_16(**kw):
    bc = ("periodic", "periodic", "periodic")
    sim = cu.SimulationData(bpdx=1, bpdy=1, bpdz=1, levelMax=2, levelStart=1, extent=EXT, nu=0.01, CFL=0.3, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], **kw)
    g = O.OracleGrid((1, 1, 1), 2, 1, EXT, bc)
    sim.upload("vel", g.taylor_green([EXT] * 3, 1.0))
    return sim


def names(S):
    return [type(op).__name__ for op in S.pipeline]


def test_diagnostics_every_second_step():
    sim = taylor_green_16(freqDiagnostics=2)
    S = cu.Simulation(sim, diagnostics=True)
    assert names(S) == ["AdvectionDiffusion", "PressureProjection", "ComputeDissipation"]
    seen = []
    for step in range(5):
        S.advance(S.calcMaxTimestep())       # ComputeDissipation runs last, before sim.step moves on
        d = getattr(sim, "diagnostics", None)
        assert d is not None and d["qoi"].shape == (20,)
        if step % 2:
            assert d["step"] == step - 1     # an odd step leaves the previous entry alone
            continue
        assert d["step"] == step
        seen.append(step)
        alone = cu.ComputeDissipation(sim).compute().copy()      # a stand-alone call on the same state
        assert np.array_equal(alone.view(np.int64), d["qoi"].view(np.int64))
        sim.diagnostics = d
    assert seen == [0, 2, 4]
    assert len(cu.ComputeDissipation.NAMES) == 20 and cu.operators.NAMES is cu.ComputeDissipation.NAMES
    ke = sim.diagnostics["qoi"][cu.ComputeDissipation.NAMES.index("kinetic_energy")]
    assert 0 < ke < 0.125 * EXT ** 3 * 1.0001        # Taylor-Green with umax 1 starts at (1/8) L^3 and decays
    off = taylor_green_16(freqDiagnostics=0)
    Soff = cu.Simulation(off, diagnostics=True)
    Soff.advance(Soff.calcMaxTimestep())
    assert not hasattr(off, "diagnostics")


def test_mass_flux_takes_the_forcing_s_place():
    sim = taylor_green_16(bFixMassFlux=True, uMax_forced=1.0)
    S = cu.Simulation(sim)
    assert names(S) == ["AdvectionDiffusion", "FixMassFlux", "PressureProjection"]
    S.advance(S.calcMaxTimestep())
    assert sim.mass_flux["u_avg"] == 2 / 3
    assert names(cu.Simulation(taylor_green_16(uMax_forced=1.0))) == ["AdvectionDiffusion", "ExternalForcing", "PressureProjection"]
    assert names(cu.Simulation(taylor_green_16(bFixMassFlux=True))) == ["AdvectionDiffusion", "PressureProjection"]   # no forcing without uMax_forced (15235)


def test_default_pipeline_is_what_it_was():
    sim = taylor_green_16()
    assert (sim.bFixMassFlux, sim.freqDiagnostics) == (False, 100)
    assert names(cu.Simulation(sim)) == ["AdvectionDiffusion", "PressureProjection"]
    assert names(cu.Simulation(taylor_green_16(implicitDiffusion=True))) == ["AdvectionDiffusionImplicit", "PressureProjection"]


def test_flags_survive_mesh_adaptation():
    bc = ("periodic", "periodic", "periodic")
    sim = cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=2, levelStart=0, extent=EXT, nu=0.01, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2],
                            bFixMassFlux=True, uMax_forced=1.0, freqDiagnostics=7, leaves=O.build_balanced_mesh((2, 2, 2), 2, bc, []))
    sim.upload("vel", np.random.default_rng(3).uniform(-1, 1, (sim.nblocks, 8, 8, 8, 3)))
    S = cu.Simulation(sim, diagnostics=True)
    before = names(S)
    st = S.adaptMesh(Rtol=1e-3, Ctol=1e-9)
    assert (st != 0).any() and S.sim is not sim
    assert (S.sim.bFixMassFlux, S.sim.freqDiagnostics) == (True, 7) and names(S) == before and before[-1] == "ComputeDissipation" and "FixMassFlux" in before
