#!/usr/bin/env python3
"""Generate the golden vectors in tests/golden/*.npz from the compiled, unmodified
reference (oracle/_ref/ref_tool, built by `make -C oracle ref` from /root/reference).

Run in the build container only (the GPU box has no /root/reference and uses the
committed .npz files).  The reference runs with OMP_NUM_THREADS=1 so that its
OpenMP reductions are sequential and the bits are reproducible.

    python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

EXT = 2 * np.pi

FIELD_CASES = [
    # name, bpd, levelMax, levelStart, bc, seed
    ("f16_periodic", (2, 2, 2), 1, 0, ("periodic", "periodic", "periodic"), 11),
    ("f16_wall", (1, 1, 1), 2, 1, ("wall", "wall", "wall"), 12),
    ("f16_mixed", (2, 2, 2), 1, 0, ("freespace", "wall", "periodic"), 13),
    ("f24x16x8_mixed", (3, 2, 1), 1, 0, ("periodic", "freespace", "wall"), 14),
]
SFC_CASES = [((1, 1, 1), 4), ((2, 2, 2), 3), ((2, 1, 1), 3), ((3, 2, 1), 2), ((4, 4, 4), 1),
             ((1, 1, 2), 3), ((1, 2, 2), 3), ((1, 3, 1), 2), ((2, 1, 3), 2)]  # 1x1x2 and 1x2x2 are curve prefixes: 'regular' without being cubes


def field_case(name, bpd, lmax, lstart, bc, seed):
    rng = np.random.default_rng(seed)
    NX, NY, NZ = [(b << lstart) * 8 for b in bpd]
    velg = rng.uniform(-1, 1, (NZ, NY, NX, 3))
    presg = rng.uniform(-1, 1, (NZ, NY, NX))
    rhsg = rng.uniform(-1, 1, (NZ, NY, NX))
    chig = (rng.uniform(0, 1, (NZ, NY, NX)) > 0.7) * rng.uniform(0, 1, (NZ, NY, NX))
    udefg = rng.uniform(-1, 1, (NZ, NY, NX, 3))
    wd = O.tempfile.mkdtemp(prefix="golden_")
    for n, a in (("vel", velg), ("pres", presg), ("rhs", rhsg), ("chi", chig), ("udef", udefg)):
        a.tofile(os.path.join(wd, n + "_in.bin"))
    dt, nu, uinf, step = 0.01, 0.02, (0.1, -0.2, 0.3), 5
    script = [
        "tables tables.bin", "zero chi",
        "loadg vel vel_in.bin", f"set nu {nu}", f"set uinfx {uinf[0]}", f"set uinfy {uinf[1]}", f"set uinfz {uinf[2]}",
        "op maxu",
        f"op advdiff {dt}", "dump vel ad_vel.bin", "dump tmpV ad_tmpV.bin",
        "loadg pres pres_in.bin", "op lhs", "dump lhs lhs.bin",
        "set mean 2", "loadg pres pres_in.bin", "op lhs", "dump lhs lhs_mean2.bin",
        "set mean 0", "loadg pres pres_in.bin", "op lhs", "dump lhs lhs_mean0.bin", "set mean 1",
        "loadg pres pres_in.bin", "op precond", "dump pres precond.bin",
        "loadg lhs rhs_in.bin", "loadg pres pres_in.bin", "op solve", "dump pres solve.bin",
        # pressure RHS with a non-trivial chi / udef (tmpV holds udef, main.cpp:15081-15085)
        f"set dt {dt}", "loadg vel vel_in.bin", "loadg tmpV udef_in.bin", "loadg chi chi_in.bin", "op rhs", "dump lhs rhs.bin",
        "zero chi", "loadg pres pres_in.bin", "op divp", "dump tmpV divp.bin", "op gradp", "dump tmpV gradp.bin",
        "loadg vel vel_in.bin", "loadg pres pres_in.bin", f"set step {step}", f"op project {dt}",
        "dump vel pr_vel.bin", "dump pres pr_pres.bin",
        "loadg vel vel_in.bin", "loadg pres pres_in.bin", "set step 1", f"op project {dt}",
        "dump vel pr1_vel.bin", "dump pres pr1_pres.bin",
    ]
    recs, wd = O.run_ref(script, O.ref_args(bpd, lmax, lstart, EXT, bc), threads=1, workdir=wd)
    t, geom = O.read_tables(os.path.join(wd, "tables.bin"))
    nb = t.shape[0]
    rb = lambda f, nc: O.read_blocks(os.path.join(wd, f), nb, nc)  # noqa: E731
    iters = {r["op"] + str(i): int(r["iters"]) for i, r in enumerate(recs)}
    solve_iters = [int(r["iters"]) for r in recs if r["op"] == "solve"]
    proj_iters = [int(r["iters"]) for r in recs if r["op"] == "project"]
    out = dict(
        bpd=np.array(bpd), level_max=lmax, level=lstart, bc=np.array([O.BC[b] for b in bc]), extent=EXT,
        dt=dt, nu=nu, uinf=np.array(uinf), step=step,
        tables=t, geom=geom, vel_in=velg, pres_in=presg, rhs_in=rhsg, chi_in=chig, udef_in=udefg,
        maxu=[r for r in recs if r["op"] == "maxu"][0]["value"],
        ad_vel=rb("ad_vel.bin", 3), ad_tmpV=rb("ad_tmpV.bin", 3),
        lhs=rb("lhs.bin", 1), lhs_mean2=rb("lhs_mean2.bin", 1), lhs_mean0=rb("lhs_mean0.bin", 1),
        precond=rb("precond.bin", 1), solve=rb("solve.bin", 1), solve_iters=solve_iters[0],
        rhs=rb("rhs.bin", 1), divp=rb("divp.bin", 3)[..., 0].copy(), gradp=rb("gradp.bin", 3),
        pr_vel=rb("pr_vel.bin", 3), pr_pres=rb("pr_pres.bin", 1), pr_iters=proj_iters[0],
        pr1_vel=rb("pr1_vel.bin", 3), pr1_pres=rb("pr1_pres.bin", 1), pr1_iters=proj_iters[1],
    )
    del iters
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "blocks", nb, "solve iters", solve_iters, "project iters", proj_iters)


def mean3_case():
    """-bMeanConstraint 3 (any value > 2): ComputeLHS pins the corner cell, LHS(0,0,0) = p(0,0,0) (main.cpp:9316-9325), and
    solve() zeroes the right-hand side there (14404-14407).  One LHS application, one solve and one projection of the reference."""
    name, bpd, lmax, lstart, bc, seed = "mean3_mixed", (2, 2, 2), 1, 0, ("freespace", "wall", "periodic"), 17
    rng = np.random.default_rng(seed)
    NX, NY, NZ = [(b << lstart) * 8 for b in bpd]
    velg, presg, rhsg = rng.uniform(-1, 1, (NZ, NY, NX, 3)), rng.uniform(-1, 1, (NZ, NY, NX)), rng.uniform(-1, 1, (NZ, NY, NX))
    wd = O.tempfile.mkdtemp(prefix="golden_")
    for n, a in (("vel", velg), ("pres", presg), ("rhs", rhsg)):
        a.tofile(os.path.join(wd, n + "_in.bin"))
    dt, step = 0.01, 5
    script = ["tables tables.bin", "zero chi", "set mean 3", "set nu 0.02",
              "loadg pres pres_in.bin", "op lhs", "dump lhs lhs.bin",
              "loadg lhs rhs_in.bin", "loadg pres pres_in.bin", "op solve", "dump pres solve.bin",
              "loadg vel vel_in.bin", "loadg pres pres_in.bin", f"set step {step}", f"op project {dt}", "dump vel pr_vel.bin", "dump pres pr_pres.bin"]
    recs, wd = O.run_ref(script, O.ref_args(bpd, lmax, lstart, EXT, bc), threads=1, workdir=wd)
    t, geom = O.read_tables(os.path.join(wd, "tables.bin"))
    nb = t.shape[0]
    rb = lambda f, nc: O.read_blocks(os.path.join(wd, f), nb, nc)  # noqa: E731
    out = dict(bpd=np.array(bpd), level_max=lmax, level=lstart, bc=np.array([O.BC[b] for b in bc]), extent=EXT, dt=dt, step=step, tables=t,
               vel_in=velg, pres_in=presg, rhs_in=rhsg, lhs=rb("lhs.bin", 1), solve=rb("solve.bin", 1),
               solve_iters=[int(r["iters"]) for r in recs if r["op"] == "solve"][0],
               pr_vel=rb("pr_vel.bin", 3), pr_pres=rb("pr_pres.bin", 1), pr_iters=[int(r["iters"]) for r in recs if r["op"] == "project"][0])
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "solve iters", out["solve_iters"], "project iters", out["pr_iters"])


def traj_case():
    """Full reference time stepping (calcMaxTimestep + advance) from the Taylor-Green IC."""
    bpd, lmax, lstart, bc = (2, 2, 2), 1, 0, ("periodic", "periodic", "periodic")
    nsteps = 6
    script = ["tables tables.bin", "zero chi", "dump vel v0.bin"]
    for n in range(nsteps):
        script += ["op steps 1", f"dump vel v{n + 1}.bin", f"dump pres p{n + 1}.bin"]
    recs, wd = O.run_ref(script, O.ref_args(bpd, lmax, lstart, EXT, bc, nu=0.01, cfl=0.3, extra=["-rampup", "4"]), threads=1)
    t, geom = O.read_tables(os.path.join(wd, "tables.bin"))
    nb = t.shape[0]
    out = dict(bpd=np.array(bpd), level_max=lmax, level=lstart, bc=np.array([O.BC[b] for b in bc]), extent=EXT,
               nu=0.01, cfl=0.3, rampup=4, umax_forced=1.0, tables=t,
               dts=np.array([r["value"] for r in recs]), iters=np.array([int(r["iters"]) for r in recs]),
               vel=np.stack([O.read_blocks(os.path.join(wd, f"v{n}.bin"), nb, 3) for n in range(nsteps + 1)]),
               pres=np.stack([O.read_blocks(os.path.join(wd, f"p{n + 1}.bin"), nb, 1) for n in range(nsteps)]))
    np.savez_compressed(os.path.join(HERE, "traj16_tgv.npz"), **out)
    print("traj16_tgv dts", out["dts"], "iters", out["iters"])


def adapt_cases():
    """Whole-mesh refine then compress through the reference's own adaptMesh (main.cpp:15179-15194): every
    block tagged Refine (tolerance -1), then every block tagged Compress (tolerance 1e300)."""
    bpd, lmax = (2, 2, 2), 3
    for name, bc, seed in (("adapt16_periodic", ("periodic",) * 3, 31), ("adapt16_mixed", ("wall", "freespace", "periodic"), 32),
                           ("adapt16_wall", ("wall",) * 3, 33)):
        rng = np.random.default_rng(seed)
        velg, presg = rng.uniform(-1, 1, (16, 16, 16, 3)), rng.uniform(-1, 1, (16, 16, 16))
        velg *= (0.35 + 0.65 * (np.arange(16) // 8))[None, None, :, None] * (0.6 + 0.4 * (np.arange(16) // 8))[:, None, None, None]  # per-block amplitudes
        wd = O.tempfile.mkdtemp(prefix="golden_")
        velg.tofile(os.path.join(wd, "vel_in.bin"))
        presg.tofile(os.path.join(wd, "pres_in.bin"))
        script = ["loadg vel vel_in.bin", "loadg pres pres_in.bin", "tagvel 1.0 0.5 tags.bin", "amrtol -1 -2", "adapt", "tables t1.bin",
                  "dump vel v1.bin", "dump pres p1.bin", "amrtol 1e300 1e299", "adapt", "tables t2.bin", "dump vel v2.bin", "dump pres p2.bin"]
        recs, wd = O.run_ref(script, O.ref_args(bpd, lmax, 0, EXT, bc), threads=1, workdir=wd)
        t1, _ = O.read_tables(os.path.join(wd, "t1.bin"))
        t2, _ = O.read_tables(os.path.join(wd, "t2.bin"))
        out = dict(bpd=np.array(bpd), level_max=lmax, bc=np.array([O.BC[b] for b in bc]), extent=EXT, vel_in=velg, pres_in=presg,
                   tag_rtol=1.0, tag_ctol=0.5, tags=np.fromfile(os.path.join(wd, "tags.bin"), dtype=np.int8), tables_fine=t1, tables_coarse=t2,
                   vel_fine=O.read_blocks(os.path.join(wd, "v1.bin"), len(t1), 3), pres_fine=O.read_blocks(os.path.join(wd, "p1.bin"), len(t1), 1),
                   vel_coarse=O.read_blocks(os.path.join(wd, "v2.bin"), len(t2), 3), pres_coarse=O.read_blocks(os.path.join(wd, "p2.bin"), len(t2), 1))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, "blocks", len(t2), "->", len(t1), "->", len(t2), "tags", out["tags"])


def vortex_field(bpd):
    """Localised Gaussian vortex on the level-0 cells: makes TagLoadedBlock refine a compact region."""
    N = [b * 8 for b in bpd]
    x = [(np.arange(n) + 0.5) * EXT / max(N) for n in N]
    Z, Y, X = np.meshgrid(x[2], x[1], x[0], indexing="ij")
    g = np.exp(-((X - 2.0) ** 2 + (Y - 2.0) ** 2 + (Z - 2.3) ** 2) / 0.5)
    return np.stack([-(Y - 2.0) * g, (X - 2.0) * g, 0.3 * g], axis=-1) * 3


def amr_mesh_script(wd, bpd, passes, rtol=2.0):
    vortex_field(bpd).tofile(os.path.join(wd, "vel_in.bin"))
    # chi is adapted without data transfer (new blocks hold uninitialised memory, which GradChiOnTmp would read at the
    # next adaptMesh, main.cpp:8541-8600): clear it after every pass
    return ["zero chi", "loadg vel vel_in.bin", f"amrtol {rtol} 0.01"] + ["adapt", "zero chi"] * passes


AMR_CASES = [
    # name, bpd, levelMax, bc, adapt passes, seed, full
    ("amr_periodic_l01", (2, 2, 2), 3, ("periodic", "periodic", "periodic"), 1, 41, True),
    ("amr_mixed_l12", (2, 2, 2), 3, ("freespace", "wall", "periodic"), 2, 42, False),
]


def amr_case(name, bpd, lmax, bc, passes, seed, full):
    """Operators on a multi-level mesh produced by the reference's own adaptMesh; block-ordered random fields
    are loaded into the adapted mesh (`loadb`)."""
    wd = O.tempfile.mkdtemp(prefix="golden_")
    pre = amr_mesh_script(wd, bpd, passes)
    args = O.ref_args(bpd, lmax, 0, EXT, bc)
    recs, wd = O.run_ref(pre + ["tables t1.bin"], args, threads=1, workdir=wd)
    t1, _ = O.read_tables(os.path.join(wd, "t1.bin"))
    nb = len(t1)
    rng = np.random.default_rng(seed)
    vel, pres, rhs = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    udef = rng.uniform(-1, 1, (nb, 8, 8, 8, 3))
    chi = (rng.uniform(0, 1, (nb, 8, 8, 8)) > 0.7) * rng.uniform(0, 1, (nb, 8, 8, 8))
    for n, a in (("velb", vel), ("presb", pres), ("rhsb", rhs), ("udefb", udef), ("chib", chi)):
        a.tofile(os.path.join(wd, n + ".bin"))
    dt, nu, uinf, step = 0.01, 0.02, (0.1, -0.2, 0.3), 5
    script = pre + [
        "loadb vel velb.bin", "loadb pres presb.bin", f"set nu {nu}", f"set uinfx {uinf[0]}", f"set uinfy {uinf[1]}", f"set uinfz {uinf[2]}",
        "lab vel -3 4 0 lab_vel34.bin", "lab pres -1 2 0 lab_p12.bin", "lab vel -1 2 1 lab_v12t.bin",
        f"op advdiff {dt}", "dump vel ad_vel.bin", "loadb pres presb.bin", "op lhs", "dump lhs lhs.bin",
        "loadb pres presb.bin", "op precond", "dump pres precond.bin",
        "loadb lhs rhsb.bin", "loadb pres presb.bin", "op solve", "dump pres solve.bin",
        f"set dt {dt}", "loadb vel velb.bin", "loadb tmpV udefb.bin", "loadb chi chib.bin", "op rhs", "dump lhs rhs.bin",
        "zero chi", "loadb pres presb.bin", "op divp", "dump tmpV divp.bin", "op gradp", "dump tmpV gradp.bin",
        "loadb vel velb.bin", "loadb pres presb.bin", f"set step {step}", f"op project {dt}", "dump vel pr_vel.bin", "dump pres pr_pres.bin",
    ]
    recs, wd = O.run_ref(script, args, threads=1, workdir=wd)
    rb = lambda f, nc: O.read_blocks(os.path.join(wd, f), nb, nc)  # noqa: E731
    out = dict(bpd=np.array(bpd), level_max=lmax, bc=np.array([O.BC[b] for b in bc]), extent=EXT, tables=t1, dt=dt, nu=nu,
               uinf=np.array(uinf), step=step, vel_in=vel, pres_in=pres, rhs_in=rhs, udef_in=udef, chi_in=chi,
               ad_vel=rb("ad_vel.bin", 3), lhs=rb("lhs.bin", 1), rhs=rb("rhs.bin", 1), pr_vel=rb("pr_vel.bin", 3), pr_pres=rb("pr_pres.bin", 1),
               solve_iters=[int(r["iters"]) for r in recs if r["op"] == "solve"][0],
               pr_iters=[int(r["iters"]) for r in recs if r["op"] == "project"][0])
    if full:
        def lab(f, L, nc, s, e, tens):   # cells the reference never defines (stale memory) are cleared: reproducible files
            a = np.fromfile(os.path.join(wd, f)).reshape(nb, L, L, L, nc)
            a[:, ~O.lab_mask(s, e, tens)] = 0.0
            return a
        out.update(lab_vel34=lab("lab_vel34.bin", 14, 3, -3, 4, False), lab_p12=lab("lab_p12.bin", 10, 1, -1, 2, False),
                   lab_v12t=lab("lab_v12t.bin", 10, 3, -1, 2, True),
                   precond=rb("precond.bin", 1), solve=rb("solve.bin", 1), divp=rb("divp.bin", 3)[..., 0].copy(), gradp=rb("gradp.bin", 3))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "blocks", nb, "levels", sorted(set(t1[:, 0].tolist())), "solve iters", out["solve_iters"], "project iters", out["pr_iters"])


def vorticity_cases():
    """ComputeVorticity + the per-block tags of tmpV_amr->Tag() (the decision input of adaptMesh) on the velocity inputs of
    existing cases: one uniform grid and the two multi-level meshes.  Stores only the outputs."""
    out = {}
    for name in ("f16_mixed", "amr_periodic_l01", "amr_mixed_l12"):
        g = np.load(os.path.join(HERE, name + ".npz"))
        bpd, lmax = tuple(int(b) for b in g["bpd"]), int(g["level_max"])
        bc = tuple(O.BC_NAMES[int(b)] for b in g["bc"])
        wd = O.tempfile.mkdtemp(prefix="golden_")
        if name.startswith("amr"):
            passes = [c for c in AMR_CASES if c[0] == name][0][4]
            pre, lstart = amr_mesh_script(wd, bpd, passes), 0
            g["vel_in"].tofile(os.path.join(wd, "v.bin"))
            pre += ["loadb vel v.bin"]
        else:
            lstart = int(g["level"])
            g["vel_in"].tofile(os.path.join(wd, "v.bin"))
            pre = ["zero chi", "loadg vel v.bin"]
        args = O.ref_args(bpd, lmax, lstart, EXT, bc)
        recs, wd = O.run_ref(pre + ["tables t.bin", "op vorticity", "dump tmpV w.bin"], args, threads=1, workdir=wd)
        t, _ = O.read_tables(os.path.join(wd, "t.bin"))
        assert np.array_equal(t, g["tables"]), name
        w = O.read_blocks(os.path.join(wd, "w.bin"), len(t), 3)
        linf = np.sqrt((w ** 2).sum(axis=-1)).reshape(len(t), -1).max(axis=1)
        rt, ct = float(np.quantile(linf, 0.6)), float(np.quantile(linf, 0.3))  # a mix of Refine / Leave / Compress
        recs, wd = O.run_ref(pre + ["op vorticity", f"tagtmp {rt!r} {ct!r} tags.bin"], args, threads=1, workdir=wd)
        out[name + "_vort"] = w
        out[name + "_tags"] = np.fromfile(os.path.join(wd, "tags.bin"), dtype=np.int8)
        out[name + "_tol"] = np.array([rt, ct])
        print(name, "vorticity max", np.abs(out[name + "_vort"]).max(), "tags", {int(k): int((out[name + "_tags"] == k).sum()) for k in (-1, 0, 1)})
    np.savez_compressed(os.path.join(HERE, "vorticity.npz"), **out)


def blob_chi(t, geom, seed):
    """A smooth body indicator on block-ordered cells: chi = 1 deep inside a few balls, 0 far away, a ramp of a few cells in between --
    surfaces cross blocks, sit next to coarse/fine faces and leave most blocks untouched (the shape GradChiOnTmp exists for)."""
    rng = np.random.default_rng(seed)
    ax = np.arange(8) + 0.5
    ext = (geom[:, 1:] + 8 * geom[:, :1]).max(axis=0)
    centres = rng.uniform(0.2, 0.8, (3, 3)) * ext
    radii = rng.uniform(0.12, 0.25, 3) * ext.min()
    chi = np.zeros((len(t), 8, 8, 8))
    for b in range(len(t)):
        h = geom[b, 0]
        Z, Y, X = np.meshgrid(geom[b, 3] + ax * h, geom[b, 2] + ax * h, geom[b, 1] + ax * h, indexing="ij")
        d = np.full(X.shape, np.inf)
        for c, r in zip(centres, radii):
            d = np.minimum(d, np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r)
        chi[b] = np.clip(0.5 - d / (4 * geom[:, 0].min()), -0.2, 1.3)   # values outside [0,1] exercise the clamp
    return chi


def grad_chi_cases():
    """compute<ScalarLab>(GradChiOnTmp(sim), sim.chi) (main.cpp:8540-8600, the chi-driven half of adaptMesh's tagging input) on the
    vorticity of existing cases, with a synthetic body indicator: tmpV after the operator, for levelMaxVorticity = levelMax and for
    levelMaxVorticity = levelMax - 1 (the capping branch).  Stores the chi input and the outputs."""
    out = {}
    vz = np.load(os.path.join(HERE, "vorticity.npz"))
    for name in ("f16_mixed", "amr_periodic_l01", "amr_mixed_l12"):
        g = np.load(os.path.join(HERE, name + ".npz"))
        bpd, lmax = tuple(int(b) for b in g["bpd"]), int(g["level_max"])
        bc = tuple(O.BC_NAMES[int(b)] for b in g["bc"])
        wd = O.tempfile.mkdtemp(prefix="golden_")
        if name.startswith("amr"):
            passes = [c for c in AMR_CASES if c[0] == name][0][4]
            pre, lstart = amr_mesh_script(wd, bpd, passes), 0
        else:
            pre, lstart = ["zero chi"], int(g["level"])
        args = O.ref_args(bpd, lmax, lstart, EXT, bc)
        recs, wd = O.run_ref(pre + ["tables t.bin"], args, threads=1, workdir=wd)
        t, geom = O.read_tables(os.path.join(wd, "t.bin"))
        assert np.array_equal(t, g["tables"]), name
        chi = blob_chi(t, geom, 77)
        w = vz[name + "_vort"]
        rt, ct = (float(v) for v in vz[name + "_tol"])
        chi.tofile(os.path.join(wd, "chib.bin")); w.tofile(os.path.join(wd, "wb.bin"))
        out[name + "_chi"] = chi
        for tag, lmv in (("", lmax), ("_capped", lmax - 1)):
            recs, wd = O.run_ref(pre + ["loadb chi chib.bin", "loadb tmpV wb.bin", f"set rtol {rt!r}", f"set ctol {ct!r}", f"set lmaxvort {lmv}", "op gradchi",
                                        "dump tmpV out.bin"], args, threads=1, workdir=wd)
            out[name + "_tmpV" + tag] = O.read_blocks(os.path.join(wd, "out.bin"), len(t), 3)
        changed = (out[name + "_tmpV"] != w).any(axis=(1, 2, 3, 4))
        print(name, "blocks", len(t), "changed by GradChiOnTmp", int(changed.sum()), "flagged 1e10", int((out[name + "_tmpV"][..., 0] == 1e10).any(axis=(1, 2, 3)).sum()),
              "capped variant differs in", int((out[name + "_tmpV_capped"] != out[name + "_tmpV"]).any(axis=(1, 2, 3, 4)).sum()))
    np.savez_compressed(os.path.join(HERE, "grad_chi.npz"), **out)


def octet_fields(t, seed):
    """Block-ordered random fields whose amplitude is shared by the eight siblings of an octet (and scaled with the block
    size), so that whole octets get the same vorticity tag and compression survives ValidStates."""
    rng = np.random.default_rng(seed)
    amp = {}
    a = np.array([amp.setdefault((int(l), int(i) // 2, int(j) // 2, int(k) // 2), rng.choice([0.02, 0.3, 1.0])) for l, _, i, j, k, _ in t])
    nb = len(t)
    vel = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)) * (a / 2.0 ** t[:, 0])[:, None, None, None, None]
    return vel, rng.uniform(-1, 1, (nb, 8, 8, 8))


def amr_adapt_case(name, bpd, lmax, bc, passes, seed, qr=0.75, qc=0.4):
    """One full Simulation::adaptMesh (main.cpp:15179-15194) of the reference on a multi-level mesh: vorticity tags,
    ValidStates, refine / compress of vel and pres."""
    wd = O.tempfile.mkdtemp(prefix="golden_")
    pre = amr_mesh_script(wd, bpd, passes)
    args = O.ref_args(bpd, lmax, 0, EXT, bc)
    _, wd = O.run_ref(pre + ["tables t.bin"], args, threads=1, workdir=wd)
    t, _ = O.read_tables(os.path.join(wd, "t.bin"))
    vel, pres = octet_fields(t, seed)
    vel.tofile(os.path.join(wd, "velb.bin"))
    pres.tofile(os.path.join(wd, "presb.bin"))
    _, wd = O.run_ref(pre + ["loadb vel velb.bin", "op vorticity", "dump tmpV w.bin"], args, threads=1, workdir=wd)
    w = O.read_blocks(os.path.join(wd, "w.bin"), len(t), 3)
    linf = np.sqrt((w ** 2).sum(axis=-1)).reshape(len(t), -1).max(axis=1)
    rt, ct = float(np.quantile(linf, qr)), float(np.quantile(linf, qc))
    _, wd = O.run_ref(pre + ["loadb vel velb.bin", "loadb pres presb.bin", "op vorticity", f"tagtmp {rt!r} {ct!r} tags.bin", f"amrtol {rt!r} {ct!r}",
                             "adapt", "tables t2.bin", "dump vel v2.bin", "dump pres p2.bin"], args, threads=1, workdir=wd)
    t2, _ = O.read_tables(os.path.join(wd, "t2.bin"))
    tags = np.fromfile(os.path.join(wd, "tags.bin"), dtype=np.int8)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), bpd=np.array(bpd), level_max=lmax, bc=np.array([O.BC[b] for b in bc]), extent=EXT,
                        tables=t, vel_in=vel, pres_in=pres, tol=np.array([rt, ct]), tags=tags, tables_new=t2,
                        vel_new=O.read_blocks(os.path.join(wd, "v2.bin"), len(t2), 3), pres_new=O.read_blocks(os.path.join(wd, "p2.bin"), len(t2), 1))
    print(name, "blocks", len(t), "->", len(t2), "tags", {int(k): int((tags == k).sum()) for k in (-1, 0, 1)},
          "levels", sorted(set(t[:, 0].tolist())), "->", sorted(set(t2[:, 0].tolist())))


def obstacle_cases():
    """KernelPenalization (+ force / torque), kernelUpdateTmpV inside PressureProjection and the chi-weighted right-hand side of
    the reference, driven by a synthetic obstacle (oracle_lib.synthetic_obstacle: chi and udef of the test's choosing on any mesh; the
    reference's own fish run here too, on the GSL stand-ins of oracle/refbuild/gsl: fish_cases below).  One uniform grid and one multi-level mesh; stores the obstacle, the inputs and the outputs."""
    out = {}
    for name, implicit, lam in (("f16_mixed", 1, 1e6), ("amr_periodic_l01", 0, 1e4)):
        g = np.load(os.path.join(HERE, name + ".npz"))
        bpd, lmax = tuple(int(b) for b in g["bpd"]), int(g["level_max"])
        bc = tuple(O.BC_NAMES[int(b)] for b in g["bc"])
        t = g["tables"]
        nb = len(t)
        wd = O.tempfile.mkdtemp(prefix="golden_")
        if name.startswith("amr"):
            passes = [c for c in AMR_CASES if c[0] == name][0][4]
            pre, lstart = amr_mesh_script(wd, bpd, passes), 0
        else:
            pre, lstart = ["zero chi"], int(g["level"])
        rng = np.random.default_rng(77)
        vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
        obst, chif = O.synthetic_obstacle(None, nb, 78)
        O.write_obstacle_file(os.path.join(wd, "ob.bin"), obst)
        for n, a in (("velb", vel), ("presb", pres), ("chib", chif)):
            a.tofile(os.path.join(wd, n + ".bin"))
        dt, step = 0.01, 5
        script = pre + ["tables t.bin", "obstacle ob.bin", "loadb vel velb.bin", "loadb pres presb.bin", "loadb chi chib.bin", f"set lambda {lam}",
                        f"set implicit {implicit}", f"op penalize {dt}", "dump vel pen.bin", "forces f.bin", "loadb vel velb.bin", f"set step {step}",
                        f"op project {dt}", "dump vel pv.bin", "dump pres pp.bin"]
        recs, wd = O.run_ref(script, O.ref_args(bpd, lmax, lstart, EXT, bc), threads=1, workdir=wd)
        t2, _ = O.read_tables(os.path.join(wd, "t.bin"))
        assert np.array_equal(t2, t), name
        out.update({name + "_vel_in": vel, name + "_pres_in": pres, name + "_chi_field": chif, name + "_ids": obst["ids"], name + "_ochi": obst["chi"],
                    name + "_oudef": obst["udef"], name + "_rigid": obst["rigid"], name + "_par": np.array([dt, lam, implicit, step]),
                    name + "_pen_vel": O.read_blocks(os.path.join(wd, "pen.bin"), nb, 3), name + "_force6": np.fromfile(os.path.join(wd, "f.bin")),
                    name + "_pr_vel": O.read_blocks(os.path.join(wd, "pv.bin"), nb, 3), name + "_pr_pres": O.read_blocks(os.path.join(wd, "pp.bin"), nb, 1),
                    name + "_pr_iters": [int(r["iters"]) for r in recs if r["op"] == "project"][0]})
        print(name, "obstacle blocks", len(obst["ids"]), "force", out[name + "_force6"][:3], "project iters", out[name + "_pr_iters"])
    np.savez_compressed(os.path.join(HERE, "obstacle_ops.npz"), **out)


def fish_cases():
    """The reference's own obstacles: StefanFish through CreateObstacles (statement by statement), UpdateObstacles, the collision model and
    ComputeForces, by the harness's `obst` commands.  Recipes, array names and the split into fish_*_<part>.npz: tests/fish_cases.py."""
    import fish_cases as F
    for name in F.CASES:
        d = F.run(name)
        cov = F.parse_coverage(str(d["coverage"]))
        assert all(int(cov[f"o{k}.blocks_with_points"]) >= 8 for k in range(F.nobstacles(name))), cov   # the fish still has a surface worth the name
        if name == "fish_two_hit":
            assert d["k.collided"].tolist() == [0, 1] and int(d["k.bCollision"][0]) == 1, "the reference reports no collision"
            assert d["k2.collided"].tolist() == [0, 1] and cov["resolved_when_closing"] == "1,1,1,1,1"   # ... and resolves it once the two close in
        if name == "fish_two_miss":
            assert int(cov["shared_blocks"]) > 0 and d["k.collided"].size == 0 and int(d["k.bCollision"][0]) == 0
        F.save(name, d)
        print(str(d["coverage"]))


def implicit_cases():
    """AdvectionDiffusionImplicit (main.cpp:10030-10118) and its parts -- KernelAdvect, KernelDiffusionRHS, DiffusionSolver::_lhs for
    the three directions, diffusion_kernels::getZImplParallel, DiffusionSolver::solve -- on a uniform mixed-BC grid and on a
    multi-level mesh, ONE thread (KernelAdvect updates vel in place while later blocks still read it: the reference's result is
    only defined for a fixed block order)."""
    out = {}
    for name in ("f16_mixed", "amr_mixed_l12"):
        g = np.load(os.path.join(HERE, name + ".npz"))
        bpd, lmax = tuple(int(b) for b in g["bpd"]), int(g["level_max"])
        bc = tuple(O.BC_NAMES[int(b)] for b in g["bc"])
        t = g["tables"]
        nb = len(t)
        wd = O.tempfile.mkdtemp(prefix="golden_")
        if name.startswith("amr"):
            passes = [c for c in AMR_CASES if c[0] == name][0][4]
            pre, lstart = amr_mesh_script(wd, bpd, passes), 0
        else:
            pre, lstart = ["zero chi"], int(g["level"])
        rng = np.random.default_rng(91)
        vel, pres, rhs = 0.5 * rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8)), rng.uniform(-1, 1, (nb, 8, 8, 8))
        for n, a in (("velb", vel), ("presb", pres), ("rhsb", rhs)):
            a.tofile(os.path.join(wd, n + ".bin"))
        dt, nu, uinf = 0.05, 2.0, (0.1, -0.2, 0.3)  # nu*dt/h^2 = O(1): the Helmholtz solves need O(10) iterations
        script = pre + ["tables t.bin", f"set nu {nu}", f"set dt {dt}", f"set uinfx {uinf[0]}", f"set uinfy {uinf[1]}", f"set uinfz {uinf[2]}",
                        "loadb vel velb.bin", "op advect", "dump vel adv_vel.bin", "dump tmpV adv_tmp.bin",
                        "loadb vel velb.bin", "op diffrhs", "dump tmpV drhs.bin"]
        for d in range(3):
            script += ["loadb pres presb.bin", f"op difflhs {d}", f"dump lhs dlhs{d}.bin"]
        script += ["loadb pres presb.bin", "op diffprecond", "dump pres dpre.bin",
                   "set difftol 1e-9", "set difftolrel 1e-9", "loadb lhs rhsb.bin", "loadb pres presb.bin", "op diffsolve 1", "dump pres dsol.bin",
                   "set difftol 1e-6", "set difftolrel 1e-4",
                   "loadb vel velb.bin", "loadb pres presb.bin", f"op advdiff_implicit {dt}", "dump vel imp_vel.bin", "dump pres imp_pres.bin"]
        recs, wd = O.run_ref(script, O.ref_args(bpd, lmax, lstart, EXT, bc), threads=1, workdir=wd)
        t2, _ = O.read_tables(os.path.join(wd, "t.bin"))
        assert np.array_equal(t2, t), name
        rb = lambda f, nc: O.read_blocks(os.path.join(wd, f), nb, nc)  # noqa: E731
        assert np.array_equal(rb("imp_pres.bin", 1), pres)
        out.update({name + "_vel_in": vel, name + "_pres_in": pres, name + "_rhs_in": rhs, name + "_par": np.array([dt, nu, *uinf]),
                    name + "_adv_vel": rb("adv_vel.bin", 3), name + "_adv_tmp": rb("adv_tmp.bin", 3), name + "_drhs": rb("drhs.bin", 3),
                    name + "_dlhs": np.stack([rb(f"dlhs{d}.bin", 1) for d in range(3)]), name + "_dpre": rb("dpre.bin", 1),
                    name + "_dsol": rb("dsol.bin", 1), name + "_imp_vel": rb("imp_vel.bin", 3),
                    name + "_dsol_iters": [int(float(r["value"])) for r in recs if r["op"] == "diffsolve"][0]})
        print(name, "blocks", nb, "diffsolve iters", out[name + "_dsol_iters"])
    np.savez_compressed(os.path.join(HERE, "implicit_diffusion.npz"), **out)


PARTITION_CASES = [((2, 2, 2), 3, 2, 3), ((1, 2, 3), 2, 1, 2), ((2, 2, 2), 3, 2, 7), ((3, 1, 2), 3, 2, 5), ((1, 1, 1), 3, 2, 8)]


def partition_cases():
    """Block ownership on several ranks (GridMPI 2970-2986: contiguous ranges of the Hilbert order, the first ranks one block
    longer) from the reference run under a REAL MPI (oracle/_ref/ref_tool_mpi, conda MPICH of the build container): per case and
    rank the block table (level, Z, index, blockID_2) of that rank."""
    out = {}
    for k, (bpd, lmax, lstart, nranks) in enumerate(PARTITION_CASES):
        wd = O.run_ref_mpi(["tables t.bin"], O.ref_args(bpd, lmax, lstart, EXT, ("periodic",) * 3), nranks)
        out[f"case{k}"] = np.array(list(bpd) + [lmax, lstart, nranks])
        for r in range(nranks):
            t, _ = O.read_tables(os.path.join(wd, f"t.bin.r{r}"))
            out[f"case{k}_r{r}"] = t
        print("partition", bpd, lmax, lstart, nranks, [len(out[f"case{k}_r{r}"]) for r in range(nranks)])
    np.savez_compressed(os.path.join(HERE, "partition_mpi.npz"), **out)


def _mpi_tables(wd, name, n):
    return [O.read_tables(os.path.join(wd, f"{name}.r{r}"))[0] for r in range(n)]


def _octet_threshold(t, linf, k):
    mx = {}
    for row, v in zip(t, linf):
        key = (int(row[0]), int(row[2]) // 2, int(row[3]) // 2, int(row[4]) // 2)
        mx[key] = max(mx.get(key, 0.0), float(v))
    s = sorted(mx.values())
    return float(np.sqrt(s[k - 1] * s[k]))


def adapt_mpi_cases():
    """Block ownership after Simulation::adaptMesh on several ranks of a REAL MPI (oracle/_ref/ref_tool_mpi): per transition the
    global block table before and after with the owner rank of every block.  Covers refinement (children stay), compression of
    octets that straddle ranks (PrepareCompression), Balance_Global and the Balance_Diffusion path (max/min <= 1.01)."""
    out, k = {}, 0

    def store(bpd, lmax, bc, n, T0, T1, what):
        nonlocal k
        old, new = np.concatenate(T0), np.concatenate(T1)
        assert np.all(np.diff(old[:, 5]) > 0) and np.all(np.diff(new[:, 5]) > 0)      # ranks own contiguous runs of the global order
        out[f"t{k}_meta"] = np.array(list(bpd) + [lmax] + [O.BC[b] for b in bc] + [n])
        out[f"t{k}_old"], out[f"t{k}_new"] = old, new
        out[f"t{k}_old_owner"] = np.concatenate([np.full(len(t), r, dtype=np.int32) for r, t in enumerate(T0)])
        out[f"t{k}_new_owner"] = np.concatenate([np.full(len(t), r, dtype=np.int32) for r, t in enumerate(T1)])
        print("adapt_mpi", k, what, bpd, lmax, n, [len(t) for t in T0], "->", [len(t) for t in T1], "levels", np.bincount(old[:, 0]), "->", np.bincount(new[:, 0]))
        k += 1

    # refinement only, from the Gaussian vortex
    for bpd, lmax, bc, n, passes, rtol in (((2, 2, 2), 3, ("periodic", "wall", "freespace"), 3, 2, 2.0), ((3, 2, 2), 4, ("periodic", "freespace", "wall"), 5, 3, 1.0)):
        wd = O.tempfile.mkdtemp(prefix="golden_")
        script = amr_mesh_script(wd, bpd, 0, rtol) + ["tables t0.bin"]
        for p in range(passes):
            script += ["adapt", "zero chi", f"tables t{p + 1}.bin"]
        O.run_ref_mpi(script, O.ref_args(bpd, lmax, 0, EXT, bc), n, workdir=wd)
        T = [_mpi_tables(wd, f"t{p}.bin", n) for p in range(passes + 1)]
        for p in range(passes):
            store(bpd, lmax, bc, n, T[p], T[p + 1], "refine")
    # refinement + compression / compression only, from block-ordered fields loaded into the mesh of a first run
    for bpd, lmax, bc, n, pre_passes, lstart, seed, mode in (((2, 2, 2), 3, ("freespace", "wall", "periodic"), 3, 2, 0, 12, "octets"),
                                                             ((2, 2, 2), 4, ("periodic",) * 3, 5, 0, 3, 9, "dip1"),
                                                             ((2, 2, 2), 4, ("periodic", "wall", "freespace"), 4, 0, 3, 7, "dip1"),
                                                             ((2, 2, 2), 4, ("periodic",) * 3, 3, 0, 3, 11, "dip40"),
                                                             ((1, 2, 2), 4, ("wall", "periodic", "periodic"), 7, 0, 3, 13, "dip150")):
        wd = O.tempfile.mkdtemp(prefix="golden_")
        pre = amr_mesh_script(wd, bpd, pre_passes) if lstart == 0 else ["zero chi"]
        args = O.ref_args(bpd, lmax, lstart, EXT, bc)
        O.run_ref_mpi(pre + ["tables t.bin"], args, n, workdir=wd)
        T0 = _mpi_tables(wd, "t.bin", n)
        t = np.concatenate(T0)
        rng = np.random.default_rng(seed)
        if mode == "octets":
            vel, _ = octet_fields(t, seed)
        else:  # a smooth amplitude dip around one block: the vorticity of a random field scales with the local amplitude
            h = EXT / (8 * max(bpd) * 2 ** t[:, 0].astype(float))
            ctr = (t[:, 2:5] + 0.5) * 8 * h[:, None]
            d = np.abs(ctr - ctr[rng.integers(len(t))])
            d = np.minimum(d, EXT - d)
            amp = 1.0 - 0.999 * np.exp(-(d ** 2).sum(axis=1) / ((3 if mode == "dip1" else 8) * 8 * h) ** 2)
            vel = rng.uniform(-1, 1, (len(t), 8, 8, 8, 3)) * amp[:, None, None, None, None]
        vel.tofile(os.path.join(wd, "velb.bin"))
        O.run_ref_mpi(pre + ["loadb vel velb.bin", "op vorticity", "dump tmpV w.bin"], args, n, workdir=wd)
        w = np.concatenate([O.read_blocks(os.path.join(wd, f"w.bin.r{r}"), len(T0[r]), 3) for r in range(n)])
        linf = np.sqrt((w ** 2).sum(axis=-1)).reshape(len(t), -1).max(axis=1)
        rt, ct = (float(np.quantile(linf, 0.75)), float(np.quantile(linf, 0.4))) if mode == "octets" else (1e9, _octet_threshold(t, linf, int(mode[3:])))
        O.run_ref_mpi(pre + ["loadb vel velb.bin", f"amrtol {rt!r} {ct!r}", "adapt", "tables t2.bin"], args, n, workdir=wd)
        store(bpd, lmax, bc, n, T0, _mpi_tables(wd, "t2.bin", n), mode)
    np.savez_compressed(os.path.join(HERE, "adapt_mpi.npz"), **out)


def sfc_cases():
    out = {}
    for bpd, lmax in SFC_CASES:
        recs, wd = O.run_ref(["sfc sfc.bin"], O.ref_args(bpd, lmax, lmax - 1, EXT, ("periodic",) * 3), threads=1)
        a = np.fromfile(os.path.join(wd, "sfc.bin"), dtype=np.int64).reshape(-1, 38)
        out["sfc_%d_%d_%d_L%d" % (bpd + (lmax,))] = a
    np.savez_compressed(os.path.join(HERE, "sfc_tables.npz"), **out)
    print("sfc tables:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if not O.have_ref_tool():
        sys.exit("oracle/_ref/ref_tool missing: run `make -C oracle ref` where /root/reference exists")
    if sys.argv[1:] == ["mean3"]:   # one case only (added in round 3; the others regenerate identically)
        mean3_case()
        sys.exit(0)
    if sys.argv[1:] == ["fish"]:   # the obstacle operators' fixtures only (the others regenerate identically)
        fish_cases()
        sys.exit(0)
    sfc_cases()
    adapt_cases()
    for c in AMR_CASES:
        amr_case(*c)
    amr_adapt_case("amr_adapt_mixed", (2, 2, 2), 3, ("freespace", "wall", "periodic"), 2, 12)
    for c in FIELD_CASES:
        field_case(*c)
    mean3_case()
    traj_case()
    vorticity_cases()
    grad_chi_cases()
    obstacle_cases()
    fish_cases()
    implicit_cases()
    if O.have_ref_tool_mpi():
        partition_cases()
        adapt_mpi_cases()
