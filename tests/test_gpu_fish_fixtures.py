"""The device's obstacle operators against the compiled reference's own fish, bit for bit.  MI355X only (-m gpu); fixtures only.

tests/golden/fish_*.npz (tests/fish_cases.py) hold what the unmodified reference, on one OpenMP thread, left after each statement of
CreateObstacles::operator() and after UpdateObstacles, Penalization and ComputeForces for StefanFish on two-level meshes of 72 - 100 blocks.
The entry points take the fixture's inputs -- sdfLab and udef as the reference's geometry wrote them, the whole mesh's vel and pres, the
obstacles' rigid state -- and must return the fixture's outputs (np.array_equal):

  cup3d_create_obstacles                 one fish and both pairs; then cup3d_compute_forces on its surface list, first and second call
  cup3d_update_obstacles(_resident)      without and with implicit penalisation
  cup3d_penalization(_resident)          likewise: the velocity; force and torque within the reassociation of their sums (see the test)
  cup3d_prevent_colliding_obstacles      both placements, as the run left the pair and sent towards each other in five ways
  over 2 thread ranks, poison_ghosts on  create and forces: see test_one_fish_over_two_ranks for what can be bitwise there and what cannot

The velocities of UpdateObstacles come out of a 6 x 6 LU solve; the reference's goes through the LU of oracle/refbuild/gsl (a stand-in with
the same pivoting, not GSL's code), and it is that binary's bits the device reproduces here.  tests/test_gpu_update_obstacles.py keeps its
bound of 64 eps cond(A) max|x| for what another correct LU may give."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest

import collision_restatement as KR
import cup3d_amd as cu
import fish_cases as F
import labs_ranks_cases as LC
import surface_forces_restatement as SF
from cup3d_amd.capi import check, lib

pytestmark = pytest.mark.gpu
S, SIM = F.STATE, F.SIM
TWO = ("fish_two_hit", "fish_two_miss")
CREATED = ("chi", "block_com", "first", "ijk", "dchi", "delta", "cm", "block_momenta", "mass", "J", "transvel_correction", "angvel_correction")
_sims = {}


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} entries differ, max |d| = {np.abs(got.astype(float) - want).max():.3g}"


def sim_of(case):
    """(fixture, sim on its mesh with vel and pres uploaded where the fixture has them), once per case"""
    if case not in _sims:
        d = F.load(case)
        sim = cu.SimulationData(**F.sim_kwargs(d, case, nu=0.001))
        assert np.array_equal(sim.grid.tables, d["tables"]) and np.array_equal(sim.grid.geom, d["geom"])   # the reference's blocks in its order
        if "vel" in d:
            assert float(d["f1.in.sim"][SIM["nu"]]) == sim.nu
            sim.upload("vel", d["vel"])
            sim.upload("pres", d["pres"])
        _sims[case] = (d, sim)
    return _sims[case]


def create(case):
    """CreateObstacles on the fixture's sdfLab / udef / oldCorrVel; returns (fixture, sim) with sim.shapes filled"""
    d, sim = sim_of(case)
    sim.fill("chi", 0.7)   # what the call has to clear
    sim.shapes, sim.obstacles = [], []
    for k in range(F.nobstacles(case)):
        o = F.obstacle(d, "c", k)
        sim.shapes.append(cu.ObstacleShape(o["ids"], o["sdf"], o["udef"], o["oldcorr"]))
    cu.CreateObstacles(sim)(0.0)
    return d, sim


def body(shape, state):
    """the ObstacleData of a shape in the rigid state of a fixture row"""
    o = shape.data(state[S["vel"]], state[S["omega"]], forced=state[S["forced"]], block_rotation=state[S["block_rotation"]], vel_imposed=state[S["vel_imposed"]])
    o.collision_vel, o.collision_omega = state[S["collision_vel"]].copy(), state[S["collision_omega"]].copy()
    o.collision_counter = float(state[S["collision_counter"]])
    return o


@pytest.mark.parametrize("case", list(F.CASES))
def test_create_obstacles_statement_by_statement(case):
    d, sim = create(case)
    for k, s in enumerate(sim.shapes):
        o = F.obstacle(d, "c", k)
        for f in CREATED:
            same(getattr(s, f), o[f], (case, k, f))
        same(s.udef_corrected, o["udef_corrected"], (case, k, "udef after kernelRemoveUdefMomenta"))
        same(s.udef, o["udef"], (case, k, "the caller's udef stays"))
    same(sim.download("chi").ravel(), d["c.chi_field"], "the resident chi field")
    if "vel" in d:
        same(sim.download("vel"), d["vel"], "vel is not touched")


def test_compute_forces_on_the_created_surface_first_and_second_call():
    d, sim = create("fish_one")
    s = d["f1.in.o0.state"]
    sim.surfaces = [sim.shapes[0].surface(s[S["vel"]], s[S["omega"]])]
    same(sim.surfaces[0].slots, d["f1.o0.slots"], "the blocks with points")
    for call in ("f1", "f2"):
        f = F.obstacle(d, call, 0)
        same(sim.surfaces[0].qoi, f["qoi_before"], (call, "the sums going in"))
        (points, qoi), = cu.ComputeForces(sim)(0.0)
        for a, name in enumerate(SF.POINT_NAMES):
            same(points[a], f["points"][a], (call, name))
        for a, name in enumerate(SF.QOI_NAMES):
            same(qoi[:, a], f["qoi"][:, a], (call, name))
    carried = [SF.QOI_NAMES.index(n) for n in SF.CARRIED]
    assert not np.array_equal(F.obstacle(d, "f2", 0)["qoi"][:, carried], F.obstacle(d, "f1", 0)["qoi"][:, carried])


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("implicit", [0, 1])
def test_update_obstacles(implicit, resident):
    d, sim = create("fish_one")
    tag = f"u{implicit}"
    sin, sout, clock, u = d[f"{tag}.in.o0.state"], d[f"{tag}.out.o0.state"], d[f"{tag}.in.sim"], F.obstacle(d, tag, 0)
    sim.obstacles = [body(sim.shapes[0], sin)]
    sim.lambda_penal, sim.bImplicitPenalization, sim.resident_obstacles = float(clock[SIM["lambda_"]]), bool(implicit), resident
    try:
        cu.UpdateObstacles(sim)(float(clock[SIM["dt"]]))
    finally:
        sim.resident_obstacles = False
    o = sim.obstacles[0]
    n = 29 if implicit else 13
    same(o.block_sums[:, :n], u["block_sums"][:, :n], "the blocks' sums")
    print(f"implicit {implicit}, resident {resident}: |dv| = {np.abs(o.vel_computed - sout[S['vel_computed']]).max():.3g}, "
          f"|dw| = {np.abs(o.omega_computed - sout[S['omega_computed']]).max():.3g}")
    same(o.vel_computed, sout[S["vel_computed"]], "transVel_computed")
    same(o.omega_computed, sout[S["omega_computed"]], "angVel_computed")
    same(o.vel, sout[S["vel"]], "transVel")
    same(o.omega, sout[S["omega"]], "angVel")
    same(sim.download("vel"), d["vel"], "vel is only read")


def penalization_terms(d, tag):
    """(number of terms, sum |term| [6]) of the six sums of KernelPenalization (13904-13909) over the fish's cells; float64 numpy, for a bound only"""
    c, s, clock = F.obstacle(d, "c", 0), d[f"{tag}.in.o0.state"], d[f"{tag}.in.sim"]
    dt, lam, implicit = float(clock[SIM["dt"]]), float(clock[SIM["lambda_"]]), int(clock[SIM["implicit"]])
    h, org = d["geom"][c["ids"], 0], d["geom"][c["ids"], 1:4]
    i = np.arange(8) + 0.5
    p = np.stack(np.broadcast_arrays(*[(org[:, a][:, None, None, None] + h[:, None, None, None] * i.reshape([-1 if q == 2 - a else 1 for q in range(3)])[None])
                                       for a in range(3)]), axis=-1) - s[S["cm"]]
    utot = s[S["vel"]] + np.cross(s[S["omega"]], p) + c["udef_corrected"]
    X = (c["chi"] > 0.5).astype(float) if implicit else c["chi"]
    fac = X * lam / (1 + X * lam * dt) if implicit else X / dt
    fp = fac[..., None] * (utot - d["vel"][c["ids"]]) * (c["chi"] > 0)[..., None]
    dv = (h ** 3)[:, None, None, None, None]
    # every product of the torque's differences counts on its own
    tq = np.stack([np.abs(p[..., 1] * fp[..., 2]) + np.abs(p[..., 2] * fp[..., 1]), np.abs(p[..., 2] * fp[..., 0]) + np.abs(p[..., 0] * fp[..., 2]),
                   np.abs(p[..., 0] * fp[..., 1]) + np.abs(p[..., 1] * fp[..., 0])], axis=-1)
    return int((c["chi"] > 0).sum()), np.concatenate([(dv * np.abs(fp)).sum(axis=(0, 1, 2, 3)), (dv * tq).sum(axis=(0, 1, 2, 3))])


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("implicit", [0, 1])
def test_penalization(implicit, resident):
    d, sim = create("fish_one")
    tag = f"pe{implicit}"
    sin, clock, ids = d[f"{tag}.in.o0.state"], d[f"{tag}.in.sim"], d["c.o0.ids"]
    sim.obstacles = [body(sim.shapes[0], sin)]
    sim.lambda_penal, sim.bImplicitPenalization, sim.resident_obstacles = float(clock[SIM["lambda_"]]), bool(implicit), resident
    try:
        cu.Penalization(sim)(float(clock[SIM["dt"]]))
        got = sim.download("vel")
    finally:
        sim.resident_obstacles = False
        sim.upload("vel", d["vel"])   # the other tests' input
    same(got[ids], d[f"{tag}.vel"], "the obstacle's blocks of vel")
    rest = np.setdiff1d(np.arange(len(got)), ids)
    same(got[rest], d["vel"][rest], "every other block")
    # force and torque are sums over all cells of the obstacle.  Not reproducible bitwise BY CONTRACT (csrc/obstacles.hpp, header): the device
    # adds a block's cells in tree order, the reference in iz, iy, ix order (13876-13909).  Two orders of one sum of N terms differ by at most
    # (N - 1) eps sum|term| each way.  Measured on MI355X (explicit, staged): max |d| = 1.4e-20 on force z = -3.65e-14, the sum of 348 terms
    # whose absolute values add up to 5.5e-6 (bound 8.4e-19); force x and y, which do not cancel, come out bit-equal.
    got6, want6 = np.concatenate([sim.obstacles[0].force, sim.obstacles[0].torque]), d[f"{tag}.o0.force6"]
    nterms, absum = penalization_terms(d, tag)
    bound = 2 * (nterms - 1) * np.finfo(float).eps * absum
    print(f"implicit {implicit}, resident {resident}: force / torque |d| = {np.abs(got6 - want6)}, bound {bound}, |sum| = {np.abs(want6)}")
    assert (np.abs(got6 - want6) <= bound).all()


@pytest.mark.parametrize("tag", F.COLLIDE_TAGS)
@pytest.mark.parametrize("case", TWO)
def test_prevent_colliding_obstacles(case, tag):
    d, sim = create(case)
    sin = [d[f"{tag}.in.o{k}.state"] for k in range(2)]
    sout = [d[f"{tag}.out.o{k}.state"] for k in range(2)]
    sim.obstacles = [body(s, st) for s, st in zip(sim.shapes, sin)]
    for o, st in zip(sim.obstacles, sin):   # what the device made of the shapes is the state the reference's call started from
        same(o.cm, st[S["cm"]], "cm")
        same(o.mass, st[S["mass"]], "mass")
        same(o.J, st[S["J"]], "J")
    sim.bCollision = False
    cu.PreventCollidingObstacles(sim)(float(d[f"{tag}.in.sim"][SIM["dt"]]))
    for k, (o, st) in enumerate(zip(sim.obstacles, sout)):
        for f in ("vel", "omega", "collision_vel", "collision_omega"):
            same(getattr(o, f), st[S[f]], (case, tag, k, f))
        assert o.collision_counter == st[S["collision_counter"]]
    assert sim.bCollisionID == d[f"{tag}.collided"].tolist()
    # the reference keeps its CollisionInfo sums in a local: the fixture cannot hold them.  The restatement -- equal to the reference in
    # everything the function leaves (tests/test_fish_fixtures.py) -- stands in for them
    obstacles = [dict(ids=o["ids"], sdf=o["sdf"], chi=o["chi"], udef=o["udef_corrected"]) for o in (F.obstacle(d, "c", k) for k in range(2))]
    bodies = [dict(cm=st[S["cm"]], mass=st[S["mass"]], J=st[S["J"]], forced=st[S["forced"]].astype(int), vel=st[S["vel"]], omega=st[S["omega"]],
                   collision_vel=st[S["collision_vel"]], collision_omega=st[S["collision_omega"]], collision_counter=st[S["collision_counter"]]) for st in sin]
    r = KR.prevent(d["geom"], obstacles, bodies, float(d[f"{tag}.in.sim"][SIM["dt"]]))
    for k, o in enumerate(sim.obstacles):
        same(o.collision_sums, np.array(r.sums[k]), (case, tag, k, "the 20 CollisionInfo sums"))
    assert sim.bCollision == (case == "fish_two_hit")
    resolved = case == "fish_two_hit" and tag != "k"
    assert np.array_equal(sim.obstacles[0].vel, sin[0][S["vel"]]) != resolved


# what does not depend on the obstacle's centre of mass: positions, pressure, tractions, vorticity, the fluid's velocity; and their sums
POINTS_FREE_OF_CM = ("pX", "pY", "pZ", "P", "fX", "fY", "fZ", "fxV", "fyV", "fzV", "omegaX", "omegaY", "omegaZ", "vX", "vY", "vZ")
QOI_FREE_OF_CM = ("forcex", "forcey", "forcez", "forcex_P", "forcey_P", "forcez_P", "forcex_V", "forcey_V", "forcez_V", "drag", "thrust", "Pout", "PoutBnd")


@pytest.mark.timeout(600)
def test_one_fish_over_two_ranks():
    """CreateObstacles, then ComputeForces twice, on the fixture mesh spread over 2 thread ranks (the in-process communicator of
    test_gpu_labs_over_ranks.py), every ghost cell that did not travel poisoned with NaN.

    Bit for bit against the fixture: chi, the mass / CoM rows, the surface lists, the resident chi field, and of ComputeForces everything
    that does not read the centre of mass (POINTS_FREE_OF_CM, QOI_FREE_OF_CM).

    NOT reproducible bitwise against the one-thread reference, by the reference's own order dependence: the centre of mass and the 13
    momenta are sums over blocks, and two ranks add their partial sums, ((rows of rank 0) + (rows of rank 1)), where one thread adds the
    rows one after the other.  Everything downstream of the centre of mass -- block momenta, corrections, corrected udef, vxDef .. vzDef,
    torque, defPower, pLocom -- inherits that.  Those are held, bit for bit, to the restatements evaluated in the ranks' association
    (the restatements themselves equal the reference bit for bit: tests/test_fish_fixtures.py); the distance to the fixture is printed
    (measured on MI355X: |cm - fixture| = 2.2e-16, max |udef_corrected - fixture| = 1.4e-17, on both ranks)."""
    from test_gpu_create_obstacles_over_ranks import recombined, share
    from test_gpu_labs_over_ranks import VirtualComm, run_ranks
    case, nranks = "fish_one", 2
    d = F.load(case)
    c = F.CASES[case]
    o = F.obstacle(d, "c", 0)
    nb = len(d["tables"])
    t = d["tables"]
    mesh = cu.operators.Grid(c["bpd"], c["lmax"], 0, F.EXTENT, F.BC, leaves=(t[:, 0].astype(np.int32), t[:, 1].copy()))
    assert np.array_equal(mesh.tables, t)
    owner = LC.owners(nb, "ranges", nranks, 0)
    assert set(owner[o["ids"]].tolist()) == {0, 1}   # the fish lies on both sides of the rank boundary
    ob = dict(ids=o["ids"], sdf=o["sdf"], udef=o["udef"], transvel_correction=o["oldcorr"])
    keeps = [share(ob, owner, r)[1] for r in range(nranks)]
    x = recombined(SimpleNamespace(geom=d["geom"]), ob, SimpleNamespace(block_com=o["block_com"], chi=o["chi"]), keeps)
    state = d["f1.in.o0.state"]
    shapes, fields, forces = [None] * nranks, [None] * nranks, [[None, None] for _ in range(nranks)]
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 1))
    try:
        with VirtualComm(nranks):
            views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
            kw = {k: v for k, v in F.sim_kwargs(d, case, nu=0.001).items() if k != "leaves"}
            sims = [cu.SimulationData(view=views[r], **kw) for r in range(nranks)]
            for r, s in enumerate(sims):
                s.upload("vel", d["vel"][owner == r])
                s.upload("pres", d["pres"][owner == r])
                s.shapes = [share(ob, owner, r)[0]]

            def rank(r):
                cu.CreateObstacles(sims[r])(0.0)
                shapes[r] = sims[r].shapes[0]
                fields[r] = sims[r].download("chi")
                sims[r].surfaces = [shapes[r].surface(state[S["vel"]], state[S["omega"]])]
                for call in range(2):
                    forces[r][call] = cu.ComputeForces(sims[r])(0, mesh=mesh, owner=owner)[0]

            run_ranks(rank, nranks)
            del sims, views
            gc.collect()
    finally:
        check(lib().cup3d_debug_set_option(b"poison_ghosts", 0))
    # the restatement of ComputeForces with the ranks' centre of mass and corrected udef
    vt, ct, hs, org = F.forces_inputs(d, case)
    surf = F.surface_of(d, 0, "f1")
    keep_pts = np.where(np.diff(o["first"]) > 0)[0]
    surf = dict(surf, cm=x["cm"], udef=x["udef"][keep_pts], qoi=np.zeros_like(surf["qoi"]))
    want1 = SF.compute_forces(vt, ct, d["pres"], hs, org, 0.001, surf)
    want2 = SF.compute_forces(vt, ct, d["pres"], hs, org, 0.001, surf, qoi_in=want1[1])
    fix = [F.obstacle(d, "f1", 0), F.obstacle(d, "f2", 0)]
    for r, keep in enumerate(keeps):
        g = shapes[r]
        same(fields[r].ravel(), d["c.chi_field"].reshape(nb, -1)[owner == r].ravel(), f"rank {r}: the resident chi field")
        same(g.chi, o["chi"][keep], f"rank {r}: chi")
        same(g.block_com, o["block_com"][keep], f"rank {r}: mass / CoM rows")
        same(np.diff(g.first), np.diff(o["first"])[keep], f"rank {r}: points per block")
        pts = np.concatenate([np.arange(o["first"][i], o["first"][i + 1]) for i in keep]).astype(int)
        same(g.ijk, o["ijk"][pts], f"rank {r}: ijk")
        same(g.dchi, o["dchi"][pts], f"rank {r}: dchi")
        same(g.delta, o["delta"][pts], f"rank {r}: delta")
        for f in ("cm", "mass", "J", "transvel_correction", "angvel_correction"):
            same(getattr(g, f), x[f], f"rank {r}: {f} in the ranks' association")
        same(g.block_momenta, x["block_momenta"][keep], f"rank {r}: block momenta")
        same(g.udef_corrected, x["udef"][keep], f"rank {r}: corrected udef")
        print(f"rank {r}: |cm - fixture| = {np.abs(g.cm - o['cm']).max():.3g}, |udef_corrected - fixture| = {np.abs(g.udef_corrected - o['udef_corrected'][keep]).max():.3g}")
        # forces: this rank's blocks with points, in the order of the fixture's list
        mine = [i for i, b in enumerate(surf["slots"]) if owner[b] == r]
        cols = np.concatenate([np.arange(surf["first"][i], surf["first"][i + 1]) for i in mine]).astype(int)
        for call, want in enumerate((want1, want2)):
            gp, gq = forces[r][call]
            same(gp, want[0][:, cols], f"rank {r}, call {call}: points against the restatement in the ranks' association")
            same(gq, want[1][mine], f"rank {r}, call {call}: sums against the restatement in the ranks' association")
            for name in POINTS_FREE_OF_CM:
                a = SF.POINT_NAMES.index(name)
                same(gp[a], fix[call]["points"][a][cols], f"rank {r}, call {call}: {name} against the fixture")
            for name in QOI_FREE_OF_CM:
                a = SF.QOI_NAMES.index(name)
                same(gq[:, a], fix[call]["qoi"][mine, a], f"rank {r}, call {call}: {name} against the fixture")
