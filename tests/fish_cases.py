"""The compiled reference's own fish as fixtures of the obstacle operators.  TEST INFRASTRUCTURE; a helper module, not a test file.

oracle/_ref/ref_tool (the unmodified reference with the GSL stand-ins of oracle/refbuild/gsl, one OpenMP thread) runs StefanFish through its
own time loop for a few steps and then through the harness's `obst` commands (oracle/ref_harness.cpp): CreateObstacles::operator() replayed
statement by statement with a dump between the statements, UpdateObstacles with both bImplicitPenalization values from the same state,
Penalization::preventCollidingObstacles, and ComputeForces twice in a row.  Everything is taken after the geometry has run, so what the
stand-ins make of the midline does not matter: the operators under test see the same sdfLab and udef on both sides.

  CASES      the recipes: command line and script per case
  run        one case through ref_tool -> {name: array} (where oracle/_ref/ref_tool exists: tests/golden/make_golden.py and the live test)
  save/load  the committed fixtures tests/golden/<case>_<part>.npz; a case is split over several files to keep each one small
  coverage   the paths a case takes, as one line (stored in the fixture, asserted by tests/test_fish_fixtures.py)

Array names: tables, geom, vel, pres (the whole mesh, block order); c.* = `obst create`, u0.* / u1.* = `obst update` without / with implicit
penalisation, k.* = `obst collide` as the run left the pair, k2.* .. k6.* with the two sent towards each other (CLOSING), f1.* / f2.* = `obst forces`, first and second call, pe0.* / pe1.* = `obst penalize` without / with implicit penalisation (pe.vel: the obstacle's
blocks of sim.vel afterwards).  o<k>.<what> belongs to obstacle k; `state` rows
follow get_state() of the harness (STATE below)."""
import glob
import os

import numpy as np

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BC = ("freespace", "freespace", "freespace")
EXTENT = 1.0
# slices of an obstacle's state vector (oracle/ref_harness.cpp, get_state) and of the clock (get_sim_state)
STATE = dict(position=slice(0, 3), absPos=slice(3, 6), quaternion=slice(6, 10), vel=slice(10, 13), omega=slice(13, 16), mass=16, length=17, J=slice(18, 24),
             cm=slice(24, 27), transvel_correction=slice(27, 30), angvel_correction=slice(30, 33), collision_counter=43, collision_vel=slice(44, 47),
             collision_omega=slice(47, 50), forced=slice(50, 53), block_rotation=slice(53, 56), vel_imposed=slice(59, 62), penalM=62, penalCM=slice(63, 66),
             penalJ=slice(66, 72), penalLmom=slice(72, 75), penalAmom=slice(75, 78), vel_computed=slice(78, 81), omega_computed=slice(81, 84))
SIM = dict(time=0, step=1, dt=2, dt_old=3, uinf=slice(4, 7), coefU=slice(7, 10), lambda_=10, nu=11, implicit=12)


def _fish(L, x, y, z):
    return f"StefanFish L={L} T=1.0 xpos={x} ypos={y} zpos={z} heightProfile=danio widthProfile=stefan bFixFrameOfRef=1"


# bpd, levelMax, levelStart, steps of the reference's own loop before the operators are taken, fish (L, xpos, ypos, zpos)
CASES = {
    # test_fish_plumbing_run's fish and resolution (tests/test_gpu_dropin.py) in half the box: 2 x 1 x 1 blocks at level 0, levels 1 and 2
    "fish_one": dict(bpd=(2, 1, 1), lmax=3, lstart=1, steps=4, fish=[(0.4, 0.5, 0.25, 0.25)]),
    # two fish side by side whose bodies share cells: the collision model resolves the pair
    "fish_two_hit": dict(bpd=(2, 1, 1), lmax=3, lstart=1, steps=4, fish=[(0.4, 0.5, 0.25, 0.25), (0.4, 0.52, 0.262, 0.25)],),
    # ... and far enough apart to share blocks but no cell
    "fish_two_miss": dict(bpd=(2, 1, 1), lmax=3, lstart=1, steps=4, fish=[(0.4, 0.5, 0.22, 0.25), (0.4, 0.5, 0.30, 0.25)],),
}
# transVel and angVel of fish 0 and fish 1 (which lies at the larger y) for the calls after the first: towards each other in y, at
# several speeds and spins, so that the pair loop and ElasticCollision (13967-14007) see more than one set of numbers
CLOSING = [((0.02, 0.1, 0.01, 0.05, -0.02, 0.03), (-0.01, -0.1, 0.0, -0.04, 0.01, 0.02)),
           ((0.3, 0.25, -0.2, 0.0, 0.0, 0.0), (-0.2, -0.35, 0.15, 0.0, 0.0, 0.0)),
           ((0.0, 0.05, 0.0, 0.7, -0.9, 1.1), (0.0, -0.07, 0.0, -1.3, 0.4, 0.6)),
           ((-0.11, 0.013, 0.17, 0.21, 0.34, -0.55), (0.19, -0.23, -0.029, -0.31, 0.37, 0.41)),
           ((0.5, 0.6, 0.7, -0.8, 0.9, 1.0), (0.45, -0.1, 0.65, 1.1, -1.2, 1.3))]
COLLIDE_TAGS = ("k",) + tuple(f"k{n}" for n in range(2, 2 + len(CLOSING)))   # k: the pair as the run left it
PARTS = ("vel", "pres", "create", "ops")   # the files of one case: <case>_<part>.npz


def ref_args(case):
    c = CASES[case]
    return ["-bMeanConstraint", "2", "-bpdx", str(c["bpd"][0]), "-bpdy", str(c["bpd"][1]), "-bpdz", str(c["bpd"][2]), "-CFL", "0.4", "-Ctol", "0.1",
            "-extentx", repr(EXTENT), "-factory-content", "\n".join(_fish(*f) for f in c["fish"]), "-levelMax", str(c["lmax"]), "-levelStart", str(c["lstart"]),
            "-nu", "0.001", "-poissonSolver", "iterative", "-Rtol", "5", "-tdump", "0", "-tend", "0", "-factory", "", "-poissonTol", "1e-9",
            "-poissonTolRel", "1e-8", "-BC_x", BC[0], "-BC_y", BC[1], "-BC_z", BC[2]]


def script(case):
    c = CASES[case]
    s = [f"op steps {c['steps']}", "tables t.bin", "dump vel v.bin", "dump pres p.bin", "obst create c.bin", "obst state s.bin"]
    if len(c["fish"]) == 1:
        # UpdateObstacles twice from the one state; explicit first: the sixteen G* sums are then still the constructor's zeros
        s += ["set implicit 0", "obst update u0.bin", "obst loadstate s.bin", "set implicit 1", "obst update u1.bin", "obst forces f1.bin", "obst forces f2.bin"]
        # the rest of Penalization::operator() with either flag, each from the velocity the steps left (it writes sim.vel)
        s += ["set implicit 0", "obst penalize pe0.bin", "dump vel pv0.bin", "loadb vel v.bin", "set implicit 1", "obst penalize pe1.bin", "dump vel pv1.bin"]
    else:
        # the collision model on the pair as the run left it, then with the two sent towards each other (fish 1 lies at the larger y)
        s += ["obst collide k.bin"]
        for tag, (a, b) in zip(COLLIDE_TAGS[1:], CLOSING):
            s += ["obst motion 0 " + " ".join(repr(v) for v in a), "obst motion 1 " + " ".join(repr(v) for v in b), f"obst collide {tag}.bin"]
    return s


def run(case, workdir=None):
    """the case through oracle/_ref/ref_tool, one thread -> {name: array}"""
    _, wd = O.run_ref(script(case), ref_args(case), threads=1, workdir=workdir)
    t, geom = O.read_tables(os.path.join(wd, "t.bin"))
    out = {"tables": t, "geom": geom}
    files = [("c", "c.bin")]
    if len(CASES[case]["fish"]) == 1:
        out["vel"], out["pres"] = O.read_blocks(os.path.join(wd, "v.bin"), len(t), 3), O.read_blocks(os.path.join(wd, "p.bin"), len(t), 1)
        files += [("u0", "u0.bin"), ("u1", "u1.bin"), ("f1", "f1.bin"), ("f2", "f2.bin"), ("pe0", "pe0.bin"), ("pe1", "pe1.bin")]
        ids = O.read_records(os.path.join(wd, "c.bin"))["o0.ids"]
        for tag in ("pe0", "pe1"):   # KernelPenalization writes the obstacle's blocks and no other: only those are kept
            pv = O.read_blocks(os.path.join(wd, f"pv{tag[-1]}.bin"), len(t), 3)
            rest = np.setdiff1d(np.arange(len(t)), ids)
            assert np.array_equal(pv[rest], out["vel"][rest]) and not np.array_equal(pv[ids], out["vel"][ids])
            out[f"{tag}.vel"] = pv[ids]
    else:
        files += [(tag, tag + ".bin") for tag in COLLIDE_TAGS]
    for tag, f in files:
        for k, v in O.read_records(os.path.join(wd, f)).items():
            out[f"{tag}.{k}"] = v
    out["coverage"] = np.array(coverage(case, out))
    return out


def part_of(key):
    if key in ("vel",):
        return "vel"
    if key in ("pres", "tables", "geom", "c.chi_field", "coverage"):
        return "pres"
    return "create" if key.startswith("c.") else "ops"


def save(case, arrays):
    for part in PARTS:
        sub = {k: v for k, v in arrays.items() if part_of(k) == part}
        if sub:
            np.savez_compressed(os.path.join(GOLDEN, f"{case}_{part}.npz"), **sub)


_loaded = {}


def load(case):
    """the committed fixture of the case, all its files merged; read once, never modified"""
    if case not in _loaded:
        d = {}
        for f in sorted(glob.glob(os.path.join(GOLDEN, case + "_*.npz"))):
            with np.load(f) as z:
                for k in z.files:
                    d[k] = z[k]
                    d[k].setflags(write=False)
        _loaded[case] = d
    return _loaded[case]


def nobstacles(case):
    return len(CASES[case]["fish"])


def obstacle(d, tag, k):
    """obstacle k's arrays of one command, reshaped: tag 'c' -> ids, sdf, udef, chi, block_com, first, ijk, dchi, delta, cm, block_momenta, mass,
    J, transvel_correction, angvel_correction, udef_corrected (and oldcorr, the transVel_correction going in)"""
    pre = f"{tag}.o{k}."
    o = {key[len(pre):]: v for key, v in d.items() if key.startswith(pre)}
    n = len(d[f"c.o{k}.ids"])
    shapes = dict(sdf=(n, 10, 10, 10), udef=(n, 8, 8, 8, 3), chi=(n, 8, 8, 8), block_com=(n, 4), ijk=(-1, 3), dchi=(-1, 3), block_momenta=(n, 13),
                  udef_corrected=(n, 8, 8, 8, 3), block_sums=(n, 29), qoi=(-1, 19), qoi_before=(-1, 19), points=(19, -1))
    for key, shp in shapes.items():
        if key in o:
            o[key] = o[key].reshape(shp)
    if tag == "c":
        o["mass"] = float(o["mass"][0])
        o["oldcorr"] = d[f"c.created.o{k}.state"][STATE["transvel_correction"]]
    return o


def mesh(d, case):
    c = CASES[case]
    t = d["tables"]
    return O.OracleMesh(c["bpd"], c["lmax"], EXTENT, BC, t[:, 0].astype(np.int32), t[:, 1].copy())


def sim_kwargs(d, case, **kw):
    """cup3d_amd.SimulationData arguments for the mesh of the fixture"""
    c = CASES[case]
    t = d["tables"]
    return dict(bpdx=c["bpd"][0], bpdy=c["bpd"][1], bpdz=c["bpd"][2], levelMax=c["lmax"], levelStart=0, extent=EXTENT, BC_x=BC[0], BC_y=BC[1], BC_z=BC[2],
                leaves=(t[:, 0].astype(np.int32), t[:, 1].copy()), **kw)


def straddling(d, case, ids):
    """how many of the listed blocks have a face neighbour on another level"""
    c = CASES[case]
    t = d["tables"]
    leaves = {tuple(int(v) for v in (r[0], r[2], r[3], r[4])) for r in t}
    count = 0
    for b in ids:
        l, i, j, k = (int(v) for v in (t[b, 0], t[b, 2], t[b, 3], t[b, 4]))
        hit = False
        for a, s in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)):
            q = [i, j, k]
            q[a] += s
            if q[a] < 0 or q[a] >= (c["bpd"][a] << l):
                continue   # the domain's face (no periodic direction in these cases)
            hit |= (l, q[0], q[1], q[2]) not in leaves
        count += hit
    return count


def forces_inputs(d, case):
    """the [-4,5) tensorial tiles of vel and of the chi field CreateObstacles left, the blocks' h and origins"""
    m = mesh(d, case)
    assert np.array_equal(m.tables, d["tables"])
    nb = len(d["tables"])
    return m.labs(np.ascontiguousarray(d["vel"]), -4, 5, True), m.labs(np.ascontiguousarray(d["c.chi_field"]).reshape(nb, 8, 8, 8), -4, 5, True), d["geom"][:, 0], d["geom"][:, 1:4]


def surface_of(d, k, tag="f1"):
    """obstacle k as surface_forces_restatement.compute_forces takes it: the blocks with points, in blockID order"""
    c, f = obstacle(d, "c", k), obstacle(d, tag, k)
    keep = np.where(np.diff(c["first"]) > 0)[0]
    assert np.array_equal(c["ids"][keep], f["slots"]) and np.array_equal(np.diff(c["first"])[keep], np.diff(f["first"]))
    s = d[f"{tag}.in.o{k}.state"]
    return dict(slots=f["slots"], first=f["first"], ijk=c["ijk"], dchi=c["dchi"], udef=c["udef_corrected"][keep], cm=s[STATE["cm"]], vel=s[STATE["vel"]],
                omega=s[STATE["omega"]], qoi=f["qoi_before"])


def coverage(case, d):
    """one line of key=value words: what the case exercises"""
    import surface_forces_restatement as SF
    n = nobstacles(case)
    t = d["tables"]
    words = [f"{case}:", f"mesh_blocks={len(t)}", "levels=" + ",".join(str(v) for v in sorted(set(t[:, 0].tolist())))]
    for k in range(n):
        ids, first = d[f"c.o{k}.ids"], d[f"c.o{k}.first"]
        words += [f"o{k}.blocks={len(ids)}", f"o{k}.blocks_with_points={int((np.diff(first) > 0).sum())}", f"o{k}.surface_points={int(first[-1])}",
                  f"o{k}.blocks_at_a_coarse_fine_face={straddling(d, case, ids)}"]
    if n == 1:
        vt, ct, hs, org = forces_inputs(d, case)
        o = surface_of(d, 0)
        counts = {}
        for i, b in enumerate(o["slots"]):
            for p in range(int(o["first"][i]), int(o["first"][i + 1])):
                tr = set()
                SF.visit(vt[b], ct[b], d["pres"][b], hs[b], org[b], o["udef"][i], o["ijk"][p:p + 1], o["dchi"][p:p + 1], o["cm"], o["vel"], o["omega"],
                         float(d["f1.in.sim"][SIM["nu"]]), np.zeros(19), tr)
                for order in (6, 3, 2):
                    if any(f"dveld{a}_{order}" in tr for a in "xyz"):
                        tr.add(f"points_with_a_{order}_point_first_derivative")
                if tr & {"break_at_1", "break_at_2", "break_at_3", "break_at_4", "no_break"}:
                    tr.add("points_marching_1_cell_or_more")
                if any(name.endswith("_fallback") for name in tr):
                    tr.add("points_with_a_mixed_derivative_fallback")
                for name in tr:
                    counts[name] = counts.get(name, 0) + 1
        for name in ("points_with_a_6_point_first_derivative", "points_with_a_3_point_first_derivative", "points_with_a_2_point_first_derivative",
                     "points_with_a_mixed_derivative_fallback", "points_marching_1_cell_or_more", "no_break", "continue_x", "continue_y", "continue_z"):
            words.append(f"{name}={counts.get(name, 0)}")
    else:
        a, b = obstacle(d, "c", 0), obstacle(d, "c", 1)
        shared = sorted(set(a["ids"].tolist()) & set(b["ids"].tolist()))
        cells = sum(int(((a["chi"][a["ids"].tolist().index(s)] > 0) & (b["chi"][b["ids"].tolist().index(s)] > 0)).sum()) for s in shared)
        words += [f"shared_blocks={len(shared)}", f"shared_cells={cells}"]
        words += ["collided=" + ",".join(str(v) for v in d["k.collided"].tolist()), f"bCollision={int(d['k.bCollision'][0])}",
                  "collided_when_closing=" + ",".join(str(v) for v in d["k2.collided"].tolist()),
                  "resolved_when_closing=" + ",".join(str(int(not np.array_equal(d[f'{t}.in.o0.state'], d[f'{t}.out.o0.state']))) for t in COLLIDE_TAGS[1:])]
    return " ".join(words)


def parse_coverage(line):
    """{key: value string} of a coverage line"""
    return dict(w.split("=", 1) for w in line.split()[1:])
