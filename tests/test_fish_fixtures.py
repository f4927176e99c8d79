"""The four obstacle restatements against the compiled reference's own fish, bit for bit.  No GPU.

tests/golden/fish_*.npz (tests/fish_cases.py, tests/golden/make_golden.py) hold what oracle/_ref/ref_tool -- the unmodified reference, one
OpenMP thread -- left after each statement of CreateObstacles::operator() and after UpdateObstacles, Penalization::preventCollidingObstacles
and ComputeForces, for StefanFish on two-level meshes.  The restatements were written from the reference's text; here they meet its bits:

  characteristic_restatement   chi, the chi field, mass / CoM rows, the surface lists in push_back order, the centre of mass, the 13 sums,
                               mass, J, both corrections, the corrected udef
  fluid_momenta_restatement    the 29 (13 without implicit penalisation) sums per block, penalM .. penalAmom, the computed and the new velocities
  collision_restatement        the pair as the run left it (reported, not resolved: projVel <= 0), sent towards each other (resolved), and a
                               pair that shares blocks but no cell
  surface_forces_restatement   on the oracle's [-4,5) tensorial tiles of the fixture mesh: the 19 per-point arrays and the 19 sums, first
                               call and second call (the eight carried sums go on from the first call's)

Where oracle/_ref/ref_tool exists the generator's scripts are run again and must reproduce every committed array.

What the fish do NOT reach (NOT_REACHED below, by the names the restatements' traces use) stays with the synthetic cases:
tests/test_surface_forces_cases.py, tests/test_characteristic_cases.py and tests/test_collision_cases.py assert that those take them."""
import numpy as np
import pytest

import characteristic_restatement as CR
import collision_restatement as KR
import fish_cases as F
import fluid_momenta_restatement as MR
import oracle_lib as O
import surface_forces_restatement as SF

S, SIM = F.STATE, F.SIM
TWO = ("fish_two_hit", "fish_two_miss")
RESOLVED = F.COLLIDE_TAGS[1:]   # the calls of fish_two_hit in which the two approach along the contact normal (projVel > 0); in k they do not

# paths of the functors no fish of the fixtures takes; the synthetic inputs named in the docstring cover them
NOT_REACHED = {
    "surface_forces": {"dveldx_2", "dveldy_2", "dveldz_2", "dveldxdy_fallback", "dveldydz_fallback", "dveldxdz_fallback", "no_break", "break_at_3",
                       "break_at_4", "continue_x", "continue_y", "continue_z", "vel_norm<=1e-9"},
    "characteristic": {"sdf==+h", "sdf==-h", "far_inside"},   # at h = 1/64 no cell of an L = 0.4 fish lies deeper than h inside it
    "collision": {"forced_mass_1e10", "imagmax_restarts_per_j", "totals_run_on_across_j", "iMom_persists_across_an_empty_j"},
}


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} entries differ, max |d| = {np.abs(got.astype(float) - want).max():.3g}"


@pytest.mark.skipif(not O.ref_tool_knows_obst(), reason="oracle/_ref/ref_tool not built, or built from a harness without the `obst` commands (make -C oracle ref)")
@pytest.mark.parametrize("case", list(F.CASES))
def test_rerunning_the_generator_reproduces_the_committed_arrays(case):
    d, live = F.load(case), F.run(case)
    assert sorted(d) == sorted(live)
    for k in sorted(d):
        if k == "coverage":
            assert str(d[k]) == str(live[k])
        else:
            assert d[k].dtype == live[k].dtype and d[k].shape == live[k].shape and d[k].tobytes() == live[k].tobytes(), k


_created = {}


def created(case):
    """characteristic_restatement.create on the fixture's sdfLab and udef: (chi field, [Result], trace), once per case"""
    if case not in _created:
        d = F.load(case)
        obstacles = []
        for k in range(F.nobstacles(case)):
            o = F.obstacle(d, "c", k)
            obstacles.append(dict(ids=o["ids"], sdf=o["sdf"], udef=o["udef"], transvel_correction=o["oldcorr"]))
        trace = set()
        field, res = CR.create(d["geom"], len(d["tables"]), obstacles, trace)
        _created[case] = (field, res, trace)
    return _created[case]


@pytest.mark.parametrize("case", list(F.CASES))
def test_characteristic_restatement_equals_create_obstacles_statement_by_statement(case):
    d = F.load(case)
    field, res, trace = created(case)
    same(field.ravel(), d["c.chi_field"], "chi field")
    assert (d["c.chi_field"] > 0).sum() > 100
    for k, r in enumerate(res):
        o = F.obstacle(d, "c", k)
        same(r.chi, o["chi"], "chi")                                     # after KernelCharacteristicFunction
        same(r.block_com, o["block_com"], "mass, CoM_x, CoM_y, CoM_z")
        same(r.first, o["first"], "first")
        same(r.ijk, o["ijk"], "ix, iy, iz")
        same(r.dchi, o["dchi"], "dchidx, dchidy, dchidz")
        same(r.delta, o["delta"], "delta")
        same(r.cm, o["cm"], "centerOfMass")                              # after kernelComputeGridCoM
        same(r.block_momenta, o["block_momenta"], "the 13 sums")         # after kernelIntegrateUdefMomenta
        same(r.mass, o["mass"], "mass")                                  # after kernelAccumulateUdefMomenta
        same(r.J, o["J"], "J")
        same(r.transvel_correction, o["transvel_correction"], "transVel_correction")
        same(r.angvel_correction, o["angvel_correction"], "angVel_correction")
        same(r.udef, o["udef_corrected"], "udef after kernelRemoveUdefMomenta")
        assert np.abs(o["udef_corrected"] - o["udef"]).max() > 0 and len(o["delta"]) > 500
        # what goes out is what went in plus the statements' results (finalize() changes none of it)
        out = d[f"c.out.o{k}.state"]
        same(out[S["cm"]], o["cm"], "state cm")
        same(out[S["J"]], o["J"], "state J")
    assert not (trace & NOT_REACHED["characteristic"])
    assert {"band", "far_outside", "gradH<1e-12", "Delta<=EPS", "gradUSq!=1"} <= trace


@pytest.mark.parametrize("implicit", [0, 1])
def test_fluid_momenta_restatement_equals_update_obstacles(implicit):
    d = F.load("fish_one")
    tag = f"u{implicit}"
    c, u = F.obstacle(d, "c", 0), F.obstacle(d, tag, 0)
    sin, sout, sim = d[f"{tag}.in.o0.state"], d[f"{tag}.out.o0.state"], d[f"{tag}.in.sim"]
    assert int(sim[SIM["implicit"]]) == implicit and sin[S["collision_counter"]] <= 0
    same(sin[S["cm"]], c["cm"], "the centre of mass CreateObstacles left")
    r = MR.update(d["vel"], d["geom"], c["ids"], c["chi"], c["udef_corrected"], sin[S["cm"]], sim[SIM["lambda_"]], sim[SIM["dt"]], implicit,
                  forced=sin[S["forced"]], block_rotation=sin[S["block_rotation"]], vel_imposed=sin[S["vel_imposed"]])
    n = 29 if implicit else 13
    same(r.rows[:, :n], u["block_sums"][:, :n], "block sums")
    if not implicit:
        assert np.isnan(r.rows[:, 13:]).all() and (u["block_sums"][:, 13:] == 0).all()   # untouched on both sides
    penalM, penalCM, penalJ, penalLmom, penalAmom = MR.penal(r.M, implicit)
    for name, v in (("penalM", penalM), ("penalCM", penalCM), ("penalJ", penalJ), ("penalLmom", penalLmom), ("penalAmom", penalAmom)):
        same(v, sout[S[name]], name)
    same(r.vel_computed, sout[S["vel_computed"]], "transVel_computed")
    same(r.omega_computed, sout[S["omega_computed"]], "angVel_computed")
    same(r.vel, sout[S["vel"]], "transVel")
    same(r.omega, sout[S["omega"]], "angVel")
    assert np.abs(sout[S["vel"]]).max() > 0 and not np.array_equal(sin[S["vel"]], sout[S["vel"]])


def bodies_of(d, tag, n):
    out = []
    for k in range(n):
        s = d[f"{tag}.o{k}.state"]
        out.append(dict(cm=s[S["cm"]], mass=s[S["mass"]], J=s[S["J"]], forced=s[S["forced"]].astype(int), vel=s[S["vel"]], omega=s[S["omega"]],
                        collision_vel=s[S["collision_vel"]], collision_omega=s[S["collision_omega"]], collision_counter=s[S["collision_counter"]]))
    return out


@pytest.mark.parametrize("tag", F.COLLIDE_TAGS)
@pytest.mark.parametrize("case", TWO)
def test_collision_restatement_equals_prevent_colliding_obstacles(case, tag):
    d = F.load(case)
    obstacles = []
    for k in range(2):
        o = F.obstacle(d, "c", k)
        obstacles.append(dict(ids=o["ids"], sdf=o["sdf"], chi=o["chi"], udef=o["udef_corrected"]))
    trace = set()
    r = KR.prevent(d["geom"], obstacles, bodies_of(d, tag + ".in", 2), float(d[f"{tag}.in.sim"][SIM["dt"]]), trace)
    want = bodies_of(d, tag + ".out", 2)
    assert r.collided == d[f"{tag}.collided"].tolist()
    for k in range(2):
        for f in ("vel", "omega", "collision_vel", "collision_omega", "collision_counter"):
            same(r.bodies[k][f], want[k][f], (k, f))
    resolved = case == "fish_two_hit" and tag in RESOLVED
    assert ("resolved" in trace) == resolved and ("projVel<=0" in trace) == (case == "fish_two_hit" and not resolved)
    assert np.array_equal(want[0]["vel"], bodies_of(d, tag + ".in", 2)[0]["vel"]) != resolved
    if tag == "k":
        assert bool(r.any) == bool(d["k.bCollision"][0])   # bCollision is set and never cleared: k2 inherits k's
    assert not (trace & NOT_REACHED["collision"])


@pytest.mark.parametrize("implicit", [0, 1])
def test_the_oracles_penalization_equals_the_references_on_the_fish(implicit):
    """not one of the four restatements: the C oracle's KernelPenalization + kernelFinalizePenalizationForce, the yardstick of cup3d_penalization"""
    d = F.load("fish_one")
    c, tag = F.obstacle(d, "c", 0), f"pe{implicit}"
    s, sim, nb = d[f"{tag}.in.o0.state"], d[f"{tag}.in.sim"], len(d["tables"])
    assert int(sim[SIM["implicit"]]) == implicit
    obst = dict(ids=c["ids"], chi=c["chi"], udef=c["udef_corrected"], rigid=np.concatenate([s[S["cm"]], s[S["vel"]], s[S["omega"]]]))
    v, f6 = F.mesh(d, "fish_one").penalize(d["vel"], d["c.chi_field"].reshape(nb, 8, 8, 8), obst, float(sim[SIM["dt"]]), float(sim[SIM["lambda_"]]), implicit)
    same(v[c["ids"]], d[f"{tag}.vel"], "the penalised velocity")
    same(f6, d[f"{tag}.o0.force6"], "force, torque")
    assert np.abs(f6).max() > 0


_forces = {}


def forces(call):
    """surface_forces_restatement.compute_forces on the oracle's tiles of the fixture mesh: (points, qoi, trace), once per call"""
    if call not in _forces:
        d = F.load("fish_one")
        if "tiles" not in _forces:
            _forces["tiles"] = F.forces_inputs(d, "fish_one")
        vt, ct, hs, org = _forces["tiles"]
        trace = set()
        o = F.surface_of(d, 0, call)
        _forces[call] = SF.compute_forces(vt, ct, d["pres"], hs, org, float(d[f"{call}.in.sim"][SIM["nu"]]), o, trace=trace) + (trace,)
    return _forces[call]


@pytest.mark.parametrize("call", ["f1", "f2"])
def test_surface_forces_restatement_equals_compute_forces(call):
    d = F.load("fish_one")
    f = F.obstacle(d, call, 0)
    points, qoi, trace = forces(call)
    for a, name in enumerate(SF.POINT_NAMES):
        same(points[a], f["points"][a], name)
    for a, name in enumerate(SF.QOI_NAMES):
        same(qoi[:, a], f["qoi"][:, a], name)
    carried = [SF.QOI_NAMES.index(n) for n in SF.CARRIED]
    if call == "f1":
        assert (f["qoi_before"] == 0).all()                # fresh ObstacleBlocks
    else:
        same(f["qoi_before"], F.obstacle(d, "f1", 0)["qoi"], "the sums the first call left")
        assert np.abs(f["qoi_before"][:, carried]).max() > 0
        first = F.obstacle(d, "f1", 0)["qoi"]
        zeroed = [a for a in range(19) if a not in carried]
        same(f["qoi"][:, zeroed], first[:, zeroed], "the eleven sums that restart")          # same inputs: same sums
        assert not np.array_equal(f["qoi"][:, carried], first[:, carried])                    # the eight go on
    # Obstacle::computeForces: the blocks' sums added in blockID order (13082-13086) -- over ALL ObstacleBlocks; those without points add 0
    tot = np.zeros(19)
    for row in f["qoi"]:
        tot = tot + row
    same(tot, f["totals"], "surfForce .. pLocom")
    assert not (trace & NOT_REACHED["surface_forces"])
    assert {"dveldx_6", "dveldy_6", "dveldz_6", "dveldxdy_full", "dveldydz_full", "dveldxdz_full", "break_at_0", "break_at_1", "vel_norm>1e-9"} <= trace
    assert trace & {"dveldx_3", "dveldy_3", "dveldz_3"}   # the march carries some points to within five cells of the tile's edge


@pytest.mark.parametrize("case", list(F.CASES))
def test_stored_coverage_lines(case):
    """what the generator printed: a case without surface points, without a marching point or without its collision no longer tests
    what it is there for"""
    d = F.load(case)
    line = str(d["coverage"])
    assert line.startswith(case + ":")
    cov = F.parse_coverage(line)
    assert cov["levels"] == "1,2" and int(cov["mesh_blocks"]) == len(d["tables"])
    for k in range(F.nobstacles(case)):
        assert int(cov[f"o{k}.surface_points"]) > 0 and int(cov[f"o{k}.blocks_with_points"]) >= 8
        assert int(cov[f"o{k}.blocks_at_a_coarse_fine_face"]) > 0
    if case == "fish_one":
        assert int(cov["points_marching_1_cell_or_more"]) > 0
        assert int(cov["points_with_a_6_point_first_derivative"]) > 0 and int(cov["points_with_a_3_point_first_derivative"]) > 0
        # listed in NOT_REACHED: the synthetic cases cover them
        assert int(cov["points_with_a_2_point_first_derivative"]) == 0 and int(cov["points_with_a_mixed_derivative_fallback"]) == 0
    elif case == "fish_two_hit":
        assert cov["collided"] == "0,1" and cov["collided_when_closing"] == "0,1" and cov["resolved_when_closing"] == "1,1,1,1,1" and int(cov["shared_cells"]) > 0
    else:
        assert int(cov["shared_blocks"]) > 0 and int(cov["shared_cells"]) == 0 and cov["collided"] == "" and cov["collided_when_closing"] == ""


def test_the_synthetic_cases_still_cover_what_the_fish_do_not_reach():
    import characteristic_cases as CC
    import collision_cases as KC
    import surface_forces_cases as SC
    assert NOT_REACHED["surface_forces"] <= SC.ALL_PATHS
    seen = set()
    for name in SC.SINGLE_RANK:
        seen |= SC.expected(name).trace
    assert NOT_REACHED["surface_forces"] <= seen
    seen = set()
    for name in CC.NAMES:
        seen |= CC.expected(name)[3]
    assert NOT_REACHED["characteristic"] <= seen
    seen = set()
    for which in KC.SCENARIOS:
        seen |= KC.expected("uniform8", which)[1]
    assert NOT_REACHED["collision"] <= seen
