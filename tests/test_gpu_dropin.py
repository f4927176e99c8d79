"""End-to-end drop-in: the UNMODIFIED reference translation unit with its AdvectionDiffusion /
PressureProjection pipeline entries swapped for the HIP-backed operators of
cup3d_amd/host/cup3d_hip_operators.h (oracle/_ref/ref_tool_hip), against the
same reference binary running its own CPU operators (oracle/_ref/ref_tool).  Same command line,
same script, same initial condition; only the two hot-path operators differ."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

REF_HIP = os.path.join(O.ORACLE_DIR, "_ref", "ref_tool_hip")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (O.have_ref_tool() and os.path.exists(REF_HIP)), reason="oracle/_ref binaries not built")]


def run(tool, script, args, wd, extra_env=None):
    with open(os.path.join(wd, "script.txt"), "w") as f:
        f.write("\n".join(script) + "\n")
    env = dict(os.environ, OMP_NUM_THREADS="1", **(extra_env or {}))
    out = subprocess.run([tool, "script.txt", "--"] + list(args), cwd=wd, env=env, check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600).stdout.decode()
    return [dict([("op", l.split()[1])] + [(kv.split("=")[0], float(kv.split("=")[1])) for kv in l.split()[2:]])
            for l in out.splitlines() if l.startswith("REF ")]


@pytest.mark.parametrize("mode", ["hip on", "hip resident3"])
def test_cpp_host_leaves_cleanly_under_a_checked_heap(tmp_path, mode):
    """SURVEY 8b "Errors": a drop-in for a C++ main() must not abort its host at exit.  The unmodified reference TU + the shim, three
    steps, under glibc's checked heap (MALLOC_CHECK_=3: every free verified, abort on corruption): exit code 0 (`run` raises otherwise).
    (Round 5's exit-time "double free or corruption" was a PYTHON host's: two copies of librccl, comm.hip load_rccl; scripts/exit_repro.py
    is its reproducer and tests/test_gpu_release_flavour.py its regression test.)"""
    args = O.ref_args((1, 1, 1), 3, 2, 2 * np.pi, ("wall", "periodic", "freespace"), nu=0.01, cfl=0.3, extra=["-rampup", "3"])
    d = tmp_path / "hip"
    d.mkdir()
    r = run(REF_HIP, [mode, "zero chi", "op steps 3", "dump vel v.bin"], args, str(d), extra_env={"MALLOC_CHECK_": "3"})
    assert r and r[-1]["op"] == "steps" and np.isfinite(O.read_blocks(os.path.join(str(d), "v.bin"), 64, 3)).all()


@pytest.mark.parametrize("mode", ["hip on", "hip resident", "hip resident2"])
@pytest.mark.parametrize("bc", [("periodic", "periodic", "periodic"), ("wall", "wall", "wall"), ("freespace", "periodic", "wall")])
def test_reference_time_loop_with_hip_operators(tmp_path, bc, mode):
    bpd, lmax, lstart, nsteps = (1, 1, 1), 3, 2, 5
    args = O.ref_args(bpd, lmax, lstart, 2 * np.pi, bc, nu=0.01, cfl=0.3, extra=["-rampup", "3"])
    tail = ["zero chi"] + sum([["op steps 1", f"dump vel v{n}.bin", f"dump pres p{n}.bin"] for n in range(nsteps)], [])
    cpu_dir, hip_dir = tmp_path / "cpu", tmp_path / "hip"
    cpu_dir.mkdir()
    hip_dir.mkdir()
    rc = run(O.REF_TOOL, tail, args, str(cpu_dir))
    rh = run(REF_HIP, [mode] + tail, args, str(hip_dir))  # "hip resident": vel stays in HBM between the two operators; ExternalForcing on device
    nb = 64
    for n in range(nsteps):
        assert abs(rc[n]["value"] - rh[n]["value"]) <= 1e-3 * rc[n]["value"]          # dt from findMaxU
        vc, vh = (O.read_blocks(os.path.join(str(d), f"v{n}.bin"), nb, 3) for d in (cpu_dir, hip_dir))
        pc, ph = (O.read_blocks(os.path.join(str(d), f"p{n}.bin"), nb, 1) for d in (cpu_dir, hip_dir))
        assert np.abs(vc - vh).max() <= 5e-3 * max(1.0, np.abs(vc).max())   # default solver tolerance; see tests/test_gpu_parity.py
        assert np.abs(pc - ph).max() <= 0.05 * max(1e-3, np.abs(pc).max())


def test_single_operators_through_the_shim(tmp_path):
    """AdvectionDiffusionHIP bit-exact, PressureProjectionHIP within solver tolerance, on seeded input."""
    bpd, lmax, lstart, bc = (2, 2, 2), 1, 0, ("periodic", "wall", "freespace")
    rng = np.random.default_rng(3)
    velg = rng.uniform(-1, 1, (16, 16, 16, 3))
    args = O.ref_args(bpd, lmax, lstart, 2 * np.pi, bc)
    script = ["zero chi", "loadg vel vel_in.bin", "set nu 0.02", "set uinfx 0.1", "op advdiff 0.01", "dump vel ad.bin", "dump tmpV adt.bin",
              "set step 4", "op project 0.01", "dump vel pr.bin", "dump pres prp.bin"]
    res = {}
    for tag, tool, pre in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, ["hip on"])):
        d = tmp_path / tag
        d.mkdir()
        velg.tofile(str(d / "vel_in.bin"))
        run(tool, pre + script, args, str(d))
        res[tag] = {k: O.read_blocks(str(d / f), 8, nc) for k, f, nc in (("ad", "ad.bin", 3), ("adt", "adt.bin", 3), ("pr", "pr.bin", 3), ("prp", "prp.bin", 1))}
    assert np.array_equal(res["cpu"]["ad"], res["hip"]["ad"])
    assert np.array_equal(res["cpu"]["adt"], res["hip"]["adt"])
    assert np.abs(res["cpu"]["pr"] - res["hip"]["pr"]).max() <= 0.05 * np.abs(res["cpu"]["pr"] - res["cpu"]["ad"]).max()
    assert np.abs(res["cpu"]["prp"] - res["hip"]["prp"]).max() <= 0.05 * np.abs(res["cpu"]["prp"]).max()


FISH_ARGS = ["-bMeanConstraint", "2", "-bpdx", "2", "-bpdy", "2", "-bpdz", "2", "-CFL", "0.4", "-Ctol", "0.1", "-extentx", "1", "-factory-content",
             "StefanFish L=0.4 T=1.0 xpos=0.5 ypos=0.5 zpos=0.5 heightProfile=danio widthProfile=stefan bFixFrameOfRef=1", "-levelMax", "3",
             "-levelStart", "1", "-nu", "0.001", "-poissonSolver", "iterative", "-Rtol", "5", "-tdump", "0", "-tend", "0", "-factory", "",
             "-poissonTol", "1e-9", "-poissonTolRel", "1e-8"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["hip on", "hip resident", "hip resident2"])
def test_fish_plumbing_run(tmp_path, mode):
    """BASELINE configs[0]: a single carling-fish swimmer (StefanFish, the parameters of the reference's run.sh / fish.ipynb, one fish),
    coarse 2-level AMR (levels 1 and 2 of a 2^3-block box, 148 blocks), one rank, 30 steps of the reference's own time loop --
    CreateObstacles, adaptMesh (steps < 10 and every 20th, 15314), AdvectionDiffusion, UpdateObstacles, Penalization,
    PressureProjection with chi / udef, ComputeForces -- once with the reference's CPU operators and once with the two hot-path
    operators swapped for the HIP ones (default round-trip mode, resident mode, and resident across steps: vel / pres go up only
    when the mirror is rebuilt after an adaptation).  Same binary otherwise, including the stand-ins
    for the two GSL entry points (oracle/refbuild/gsl: nothing is claimed about GSL itself).  Block lists identical at both
    check points; velocity, pressure and chi to solver round-off (Poisson tolerance 1e-9 / 1e-8 on both sides)."""
    res = {}
    script = ["op steps 12", "tables t12.bin", "op steps 18", "tables t30.bin", "dump vel v.bin", "dump pres p.bin", "dump chi c.bin"]
    for tag, tool, pre in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, [mode])):
        d = tmp_path / tag
        d.mkdir()
        with open(str(d / "script.txt"), "w") as f:
            f.write("\n".join(pre + script) + "\n")
        out = subprocess.run([tool, "script.txt", "--"] + FISH_ARGS, cwd=str(d), env=dict(os.environ, OMP_NUM_THREADS="8"), check=True,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800).stdout.decode()
        its = [float(l.split()[3].split("=")[1]) for l in out.splitlines() if l.startswith("REF steps")]
        t12, t30 = O.read_tables(str(d / "t12.bin"))[0], O.read_tables(str(d / "t30.bin"))[0]
        nb = len(t30)
        res[tag] = (t12, t30, O.read_blocks(str(d / "v.bin"), nb, 3), O.read_blocks(str(d / "p.bin"), nb, 1), O.read_blocks(str(d / "c.bin"), nb, 1), its)
    c, h = res["cpu"], res["hip"]
    assert np.array_equal(c[0], h[0]) and np.array_equal(c[1], h[1])            # the adapted block lists, bit-exactly
    assert len(set(c[1][:, 0].tolist())) == 2 and len(c[1]) > 100               # two levels, the fish refined
    assert (c[4] > 0).sum() > 100 and np.abs(c[2]).max() > 1e-3                 # there IS a fish, and it moves the fluid
    assert np.abs(c[2] - h[2]).max() <= 1e-6 * np.abs(c[2]).max()
    assert np.abs(c[3] - h[3]).max() <= 1e-4 * np.abs(c[3]).max()
    assert np.abs(c[4] - h[4]).max() <= 1e-6
    assert sum(h[5]) <= 1.3 * sum(c[5]) + 10, (h[5], c[5])


@pytest.mark.timeout(300)
@pytest.mark.skipif(not (O.ref_tool_knows_obst() and O.ref_tool_knows_obst(REF_HIP)), reason="oracle/_ref binaries built from a harness without the `obst` commands")
def test_fish_create_and_forces_through_the_shim(tmp_path):
    """CreateObstaclesHIP and ComputeForcesHIP (CUP3D_HIP_CREATE=1, CUP3D_HIP_FORCES=1) executed: the reference binary and the reference +
    shim binary, one OpenMP thread each, get the fish_one command line (tests/fish_cases.py: the mesh after init is the fixture's), the
    fixture's vel and pres (`loadb`) and the fixture's obstacle state and clock (`obst loadstate`), and each runs the CreateObstacles entry
    and the ComputeForces entry of its pipeline once (`obst run`).  No solver sits in between, so everything the two operators leave in
    the reference's own objects must be bit-equal: the chi field, every ObstacleBlock's chi and udef, the surface lists, the 19 per-point
    arrays and the 19 sums, and the obstacle's state.  One launch of each binary: 0.46 s for the whole test on MI355X; the limit of 120 s per launch is to
    test_fish_plumbing_run's 800 s (30 steps, hundreds of solver iterations each) what two operator calls are to that."""
    import fish_cases as F
    d = F.load("fish_one")
    nb = len(d["tables"])
    script = ["tables t.bin", "loadb vel v.bin", "loadb pres p.bin", "obst loadstate s.bin", "obst run create", "obst run forces", "obst blocks b.bin",
              "dump chi c.bin"]
    res = {}
    for tag, tool, pre, env in (("cpu", O.REF_TOOL, [], {}), ("hip", REF_HIP, ["hip on"], {"CUP3D_HIP_CREATE": "1", "CUP3D_HIP_FORCES": "1"})):
        wd = tmp_path / tag
        wd.mkdir()
        np.ascontiguousarray(d["vel"]).tofile(str(wd / "v.bin"))
        np.ascontiguousarray(d["pres"]).tofile(str(wd / "p.bin"))
        O.write_records(str(wd / "s.bin"), [("sim", d["c.in.sim"]), ("o0.state", d["c.in.o0.state"])])
        with open(str(wd / "script.txt"), "w") as f:
            f.write("\n".join(pre + script) + "\n")
        out = subprocess.run([tool, "script.txt", "--"] + F.ref_args("fish_one"), cwd=str(wd), env=dict(os.environ, OMP_NUM_THREADS="1", **env), check=True,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).stdout.decode()
        ran = [l.split("entry=")[1] for l in out.splitlines() if l.startswith("REF obstrun")]   # the operators `obst run` found in the pipeline
        assert ran == (["cup3d_hip::CreateObstaclesHIP", "cup3d_hip::ComputeForcesHIP"] if tag == "hip" else ["CreateObstacles", "ComputeForces"]), ran
        assert np.array_equal(O.read_tables(str(wd / "t.bin"))[0], d["tables"])
        res[tag] = dict(O.read_records(str(wd / "b.bin")), chi_field=O.read_blocks(str(wd / "c.bin"), nb, 1))
    c, h = res["cpu"], res["hip"]
    assert sorted(c) == sorted(h)
    assert c["o0.first"][-1] > 500 and np.abs(c["o0.points"]).max() > 0 and np.abs(c["o0.qoi"]).max() > 0 and (c["chi_field"] > 0).sum() > 100
    for k in sorted(c):
        assert c[k].shape == h[k].shape and np.array_equal(c[k], h[k]), f"{k}: {int((c[k] != h[k]).sum())} of {c[k].size} entries differ"


def test_poisson_solver_through_the_factory_key(tmp_path):
    """-poissonSolver cuda_iterative: the slot makePoissonSolver (main.cpp:14747-14758) reserves for a GPU solver, filled by
    cup3d_hip::makePoissonSolver; PoissonSolverBase::solve() contract: right-hand side in sim.lhs, initial guess and result in
    sim.pres.  Both iterates satisfy the stopping rule; the key "iterative" still yields the reference's own solver (bit-equal
    result), an unknown key the reference's own error."""
    bpd, lmax, lstart, bc = (2, 2, 2), 2, 1, ("wall", "periodic", "freespace")
    rng = np.random.default_rng(17)
    n = 32
    rhs, x0 = rng.uniform(-1, 1, (n, n, n)), rng.uniform(-1, 1, (n, n, n))
    args = O.ref_args(bpd, lmax, lstart, 2 * np.pi, bc)
    res = {}
    for tag, tool, pre in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, ["hipsolver cuda_iterative"]), ("same", REF_HIP, ["hipsolver iterative"])):
        d = tmp_path / tag
        d.mkdir()
        rhs.tofile(str(d / "rhs.bin")); x0.tofile(str(d / "x0.bin"))
        rec = run(tool, pre + ["zero chi", "loadg lhs rhs.bin", "loadg pres x0.bin", "op solve", "dump pres x.bin"], args, str(d))
        res[tag] = (O.read_blocks(str(d / "x.bin"), 64, 1), rec[-1]["iters"])
    assert np.array_equal(res["cpu"][0], res["same"][0]) and res["cpu"][1] == res["same"][1]
    o = O.OracleGrid(bpd, lmax, lstart, 2 * np.pi, bc)
    b = o.to_blocks(rhs)
    b[int(np.where((o.index == 0).all(axis=1))[0][0]), 0, 0, 0] = 0.0
    res0 = np.linalg.norm((b - o.lhs(o.to_blocks(x0), 1)).ravel())
    tau = max(1e-6, 1e-4 * res0)
    for tag in ("cpu", "hip"):
        assert np.linalg.norm((b - o.lhs(res[tag][0], 1)).ravel()) <= tau * (1 + 1e-6), tag
    d = tmp_path / "bad"
    d.mkdir()
    with pytest.raises(subprocess.CalledProcessError):
        run(REF_HIP, ["hipsolver no_such_solver"], args, str(d))


def test_multilevel_mesh_through_the_shim(tmp_path):
    """The reference adapts its mesh (its own adaptMesh on a localised vortex: levels 1 and 2), then runs its pipeline on
    that multi-level mesh with the HIP operators: DeviceMirror rebuilds the device topology from m_vInfo's leaves
    (cup3d_grid_create_mesh); coarse/fine ghosts and flux correction run on the device."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_golden as M
    bpd, lmax, bc = (2, 2, 2), 3, ("freespace", "wall", "periodic")
    args = O.ref_args(bpd, lmax, 0, 2 * np.pi, bc, nu=0.02, cfl=0.3, extra=["-rampup", "3", "-poissonTol", "1e-12", "-poissonTolRel", "1e-10"])
    res = {}
    for tag, tool, pre_hip in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, ["hip on"])):
        d = tmp_path / tag
        d.mkdir()
        pre = M.amr_mesh_script(str(d), bpd, 2)
        # freeze the mesh afterwards: adaptMesh inside advance() then neither refines nor compresses
        script = pre + ["tables t.bin", "amrtol 1e9 -1"] + pre_hip + ["set uinfx 0.1", "op advdiff 0.01", "dump vel ad.bin", "set step 4", "op project 0.01",
                                                                    "dump vel pr.bin", "dump pres prp.bin", "op steps 3", "dump vel st.bin", "dump pres stp.bin",
                                                                    "tables t2.bin"]
        run(tool, script, args, str(d))
        t, _ = O.read_tables(str(d / "t.bin"))
        t2, _ = O.read_tables(str(d / "t2.bin"))
        assert np.array_equal(t, t2) and len(set(t[:, 0].tolist())) == 2
        nb = len(t)
        res[tag] = {k: O.read_blocks(str(d / f), nb, nc) for k, f, nc in (("ad", "ad.bin", 3), ("pr", "pr.bin", 3), ("prp", "prp.bin", 1),
                                                                           ("st", "st.bin", 3), ("stp", "stp.bin", 1))}
        res[tag]["t"] = t
    c, h = res["cpu"], res["hip"]
    assert np.array_equal(c["t"], h["t"])
    assert np.array_equal(c["ad"], h["ad"])                                   # advect-diffuse on the AMR mesh: bit-exact
    corr = np.abs(c["pr"] - c["ad"]).max()
    assert np.abs(c["pr"] - h["pr"]).max() <= 1e-6 * corr                     # projection, both sides at 1e-12 / 1e-10
    assert np.abs(c["prp"] - h["prp"]).max() <= 1e-6 * np.abs(c["prp"]).max()
    assert np.abs(c["st"] - h["st"]).max() <= 1e-6 * np.abs(c["st"]).max()    # three steps of the reference's own loop
    assert np.abs(c["stp"] - h["stp"]).max() <= 1e-5 * np.abs(c["stp"]).max()


def test_projection_with_an_obstacle_through_the_shim(tmp_path):
    """PressureProjectionHIP with obstacles: the shim runs the reference's own kernelUpdateTmpV on the host, uploads chi and tmpV
    (= udef) and the device right-hand side reads both.  Synthetic obstacle; both sides at 1e-12 / 1e-10."""
    bpd, lmax, bc = (2, 2, 2), 2, ("periodic", "wall", "freespace")
    args = O.ref_args(bpd, lmax, 1, 2 * np.pi, bc, extra=["-poissonTol", "1e-12", "-poissonTolRel", "1e-10"])
    nb = 64
    rng = np.random.default_rng(8)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    obst, chif = O.synthetic_obstacle(None, nb, 9)
    res = {}
    for tag, tool, pre in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, ["hip on"])):
        d = tmp_path / tag
        d.mkdir()
        O.write_obstacle_file(str(d / "ob.bin"), obst)
        vel.tofile(str(d / "velb.bin")); pres.tofile(str(d / "presb.bin")); chif.tofile(str(d / "chib.bin"))
        run(tool, pre + ["obstacle ob.bin", "loadb vel velb.bin", "loadb pres presb.bin", "loadb chi chib.bin", "set step 4", "op project 0.01",
                         "dump vel pv.bin", "dump pres pp.bin"], args, str(d))
        res[tag] = (O.read_blocks(str(d / "pv.bin"), nb, 3), O.read_blocks(str(d / "pp.bin"), nb, 1))
    corr = np.abs(res["cpu"][0] - vel).max()
    assert np.abs(res["cpu"][0] - res["hip"][0]).max() <= 1e-6 * corr
    assert np.abs(res["cpu"][1] - res["hip"][1]).max() <= 1e-6 * np.abs(res["cpu"][1]).max()


def test_implicit_diffusion_through_the_shim(tmp_path):
    """-implicitDiffusion 1: install() swaps AdvectionDiffusionImplicit for AdvectionDiffusionImplicitHIP (KernelAdvect +
    KernelDiffusionRHS + three DiffusionSolver solves on the device).
    (a) One periodic block: the reference's in-place KernelAdvect is invisible to every tile, so reference and device compute
        the same thing: agreement to solver round-off at tight tolerances.
    (b) 64 blocks, Taylor-Green: the reference (one thread) lets later blocks see the already advected velocity of earlier
        ones -- its own result depends on block order and thread timing -- while the device reads the velocity on entry; the
        two differ by O(dt) of the advective increment (1 % here, measured with the oracle's two modes), which bounds what can
        be asserted: 5 % of the step's change.  pres must come back untouched on both sides."""
    rng = np.random.default_rng(8)
    for tag, bpd, lmax, lstart, nb, dt, nu, tol in (("one", (1, 1, 1), 1, 0, 1, 0.05, 2.0, 1e-7), ("tgv", (1, 1, 1), 3, 2, 64, 0.003, 0.01, 0.05)):
        args = O.ref_args(bpd, lmax, lstart, 2 * np.pi, ("periodic",) * 3, extra=["-implicitDiffusion", "1"])
        pres = rng.uniform(-1, 1, (nb, 8, 8, 8))
        script = ["zero chi", "loadb pres p_in.bin", f"set nu {nu}", "set difftol 1e-12", "set difftolrel 1e-11", "dump vel v0.bin"]
        if tag == "one":
            script.insert(1, "loadb vel v_in.bin")
        script += [f"op advdiff_implicit {dt}", "dump vel v1.bin", "dump pres p1.bin"]
        out = {}
        for side, tool, pre in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, ["hip on"])):
            d = tmp_path / (tag + side)
            d.mkdir()
            pres.tofile(str(d / "p_in.bin"))
            (0.5 * np.random.default_rng(9).uniform(-1, 1, (1, 8, 8, 8, 3))).tofile(str(d / "v_in.bin"))
            run(tool, pre + script, args, str(d))
            out[side] = [O.read_blocks(str(d / f), nb, nc) for f, nc in (("v0.bin", 3), ("v1.bin", 3), ("p1.bin", 1))]
            assert np.array_equal(out[side][2], pres)
        change = np.abs(out["cpu"][1] - out["cpu"][0]).max()
        assert change > 1e-3
        assert np.abs(out["cpu"][1] - out["hip"][1]).max() <= tol * change, tag


@pytest.mark.parametrize("implicit", [0, 1])
def test_resident_mode_with_an_obstacle(tmp_path, implicit):
    """AdvectionDiffusion -> ExternalForcing -> UpdateObstacles -> Penalization -> PressureProjection of the reference's pipeline
    (`op midstep`) with a synthetic obstacle.  `hip on`: every operator round-trips its fields.  `hip resident`: the velocity stays in
    HBM from AdvectionDiffusionHIP to PressureProjectionHIP (ExternalForcing on the device) and only the blocks the obstacle covers
    travel: UpdateObstaclesHIP fetches them for the reference's own UpdateObstacles / Penalization, PressureProjectionHIP sends them
    back.  Both must reproduce the CPU run: a stale host block would change the obstacle's computed velocity and the penalised cells."""
    bpd, lmax, bc = (2, 2, 2), 2, ("periodic", "wall", "freespace")
    args = O.ref_args(bpd, lmax, 1, 2 * np.pi, bc, extra=["-poissonTol", "1e-12", "-poissonTolRel", "1e-10"])
    nb = 64
    rng = np.random.default_rng(8)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    obst, chif = O.synthetic_obstacle(None, nb, 9)
    res = {}
    for tag, tool, pre in (("cpu", O.REF_TOOL, []), ("hip", REF_HIP, ["hip on"]), ("res", REF_HIP, ["hip resident"])):
        d = tmp_path / tag
        d.mkdir()
        O.write_obstacle_file(str(d / "ob.bin"), obst)
        vel.tofile(str(d / "velb.bin")); pres.tofile(str(d / "presb.bin")); chif.tofile(str(d / "chib.bin"))
        run(tool, pre + ["obstacle ob.bin", "loadb vel velb.bin", "loadb pres presb.bin", "loadb chi chib.bin", "set lambda 1e4", f"set implicit {implicit}",
                         "set step 4", "op midstep 0.01", "dump vel pv.bin", "dump pres pp.bin", "forces f.bin"], args, str(d))
        res[tag] = (O.read_blocks(str(d / "pv.bin"), nb, 3), O.read_blocks(str(d / "pp.bin"), nb, 1), np.fromfile(str(d / "f.bin")))
    change = np.abs(res["cpu"][0] - vel).max()
    assert change > 0.5 and len(obst["ids"]) < nb        # the obstacle acted, and on a subset of the blocks
    for tag in ("hip", "res"):
        assert np.abs(res["cpu"][0] - res[tag][0]).max() <= 1e-6 * change, tag
        assert np.abs(res["cpu"][1] - res[tag][1]).max() <= 1e-6 * np.abs(res["cpu"][1]).max(), tag
        assert np.array_equal(res["cpu"][2], res[tag][2]), tag    # penalisation force / torque: host operator on identical inputs


@pytest.mark.parametrize("bc", [("wall", "wall", "wall"), ("freespace", "periodic", "wall")])
def test_device_led_time_loop_without_findmaxu_on_the_host(tmp_path, bc):
    """`hip resident3` (DeviceMirror::device_led): vel and pres never come down between steps; the time loop calls
    cup3d_hip::calcMaxTimestep -- Simulation::calcMaxTimestep (main.cpp:15254-15305) with findMaxU (15259) taken on the device -- and
    cup3d_hip::advance, which refreshes the host copy only before adaptMesh / a dump.  Same device operators, same dt expressions, an
    exact maximum: the 24-step trajectory (across the adaptMesh calls of steps 0-9 and 20, frozen mesh) is BIT-IDENTICAL to
    `hip resident2`, dt for dt and field for field, and the reference's CPU run stays as close as in the other modes."""
    bpd, lmax, lstart, nsteps = (1, 1, 1), 3, 2, 24
    args = O.ref_args(bpd, lmax, lstart, 2 * np.pi, bc, nu=0.01, cfl=0.3, extra=["-rampup", "3"])
    tail = ["zero chi", f"rep {nsteps}", "op steps 1", "rep 1", "dump vel v.bin", "dump pres p.bin"]
    res = {}
    for tag, tool, pre in (("cpu", O.REF_TOOL, []), ("r2", REF_HIP, ["hip resident2"]), ("r3", REF_HIP, ["hip resident3"])):
        d = tmp_path / tag
        d.mkdir()
        rec = run(tool, pre + tail, args, str(d))
        res[tag] = ([r["value"] for r in rec if r["op"] == "steps"], O.read_blocks(str(d / "v.bin"), 64, 3), O.read_blocks(str(d / "p.bin"), 64, 1))
    assert len(res["r3"][0]) == nsteps and res["r3"][0] == res["r2"][0]                       # every dt, bit for bit
    assert np.array_equal(res["r3"][1], res["r2"][1]) and np.array_equal(res["r3"][2], res["r2"][2])
    assert np.abs(res["cpu"][1] - res["r3"][1]).max() <= 5e-3 * max(1.0, np.abs(res["cpu"][1]).max())
    assert max(abs(a - b) / a for a, b in zip(res["cpu"][0], res["r3"][0])) <= 1e-3
