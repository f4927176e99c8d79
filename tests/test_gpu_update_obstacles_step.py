"""The resident obstacle step: Simulation(sim, obstacle_operators=True).advance(dt) -- AdvectionDiffusion -> ExternalForcing ->
UpdateObstacles -> Penalization -> PressureProjection, every operator on the device -- against `op midstep` of the compiled reference
(oracle/_ref/ref_tool) with the same synthetic obstacle, at the configuration and with the bounds of
tests/test_gpu_dropin.py::test_resident_mode_with_an_obstacle.  Only chi and the initial fields go up; during the step nothing but the
obstacle's block sums comes down.  MI355X only (-m gpu)."""
import ctypes as C
import os

import numpy as np
import pytest

import cup3d_amd as cu
import oracle_lib as O
from cup3d_amd.capi import RunStats, check, lib

REF_HIP = os.path.join(O.ORACLE_DIR, "_ref", "ref_tool_hip")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (O.have_ref_tool() and os.path.exists(REF_HIP)), reason="oracle/_ref binaries not built")]
EXT = 2 * np.pi


@pytest.mark.parametrize("implicit", [0, 1])
def test_resident_obstacle_step_reproduces_the_reference(tmp_path, implicit):
    bpd, lmax, bc = (2, 2, 2), 2, ("periodic", "wall", "freespace")
    nu, umax_forced, lam, dt, step, nb = 0.01, 1.0, 1e4, 0.01, 4, 64
    args = O.ref_args(bpd, lmax, 1, EXT, bc, nu=nu, umax_forced=umax_forced, extra=["-poissonTol", "1e-12", "-poissonTolRel", "1e-10"])
    rng = np.random.default_rng(8)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    obst, chif = O.synthetic_obstacle(None, nb, 9)
    d = tmp_path
    O.write_obstacle_file(str(d / "ob.bin"), obst)
    vel.tofile(str(d / "velb.bin")); pres.tofile(str(d / "presb.bin")); chif.tofile(str(d / "chib.bin"))
    O.run_ref(["tables t.bin", "obstacle ob.bin", "loadb vel velb.bin", "loadb pres presb.bin", "loadb chi chib.bin", f"set lambda {lam!r}",
               f"set implicit {implicit}", f"set step {step}", f"op midstep {dt!r}", "dump vel pv.bin", "dump pres pp.bin", "forces f.bin"],
              args, workdir=str(d))
    rv, rp, rf = O.read_blocks(str(d / "pv.bin"), nb, 3), O.read_blocks(str(d / "pp.bin"), nb, 1), np.fromfile(str(d / "f.bin"))
    t, _ = O.read_tables(str(d / "t.bin"))

    sim = cu.SimulationData(bpdx=bpd[0], bpdy=bpd[1], bpdz=bpd[2], levelMax=lmax, levelStart=1, extent=EXT, nu=nu, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2],
                            uMax_forced=umax_forced, poissonTol=1e-12, poissonTolRel=1e-10)
    assert np.array_equal(sim.grid.tables, t)   # same blocks in the same order on both sides
    rigid = obst["rigid"]
    ob = cu.ObstacleData(obst["ids"], obst["chi"], obst["udef"], rigid[0:3], rigid[3:6], rigid[6:9])
    sim.obstacles, sim.lambda_penal, sim.bImplicitPenalization, sim.step = [ob], lam, bool(implicit), step
    sim.upload("vel", vel); sim.upload("pres", pres); sim.upload("chi", chif)
    S = cu.Simulation(sim, obstacle_operators=True)
    assert [type(op).__name__ for op in S.pipeline] == ["AdvectionDiffusion", "ExternalForcing", "UpdateObstacles", "Penalization", "PressureProjection"]
    st = RunStats()
    check(lib().cup3d_stats_reset())
    S.advance(dt)
    check(lib().cup3d_stats_read(C.byref(st)))
    assert st.field_bytes_downloaded == len(obst["ids"]) * 29 * 8 and st.field_bytes_uploaded == 0   # the obstacle's sums, and no field
    v, p = sim.download("vel"), sim.download("pres")
    change = np.abs(rv - vel).max()
    assert change > 0.5 and len(obst["ids"]) < nb        # the obstacle acted, and on a subset of the blocks
    f6 = np.concatenate([ob.force, ob.torque])
    ev, ep, ef = np.abs(rv - v).max() / change, np.abs(rp - p).max() / np.abs(rp).max(), np.abs(rf - f6).max() / np.abs(rf).max()
    print(f"implicit {implicit}: velocity {ev:.3g} x change, pressure {ep:.3g}, force {ef:.3g}")
    assert ev <= 1e-6
    assert ep <= 1e-6
    assert ef <= 1e-12
    assert not np.array_equal(ob.vel, rigid[3:6]) and not np.array_equal(ob.omega, rigid[6:9])   # the obstacle's motion was updated
    # the default pipeline is unchanged
    assert [type(op).__name__ for op in cu.Simulation(sim).pipeline] == ["AdvectionDiffusion", "ExternalForcing", "PressureProjection"]
