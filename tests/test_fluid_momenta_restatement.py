"""Pins tests/fluid_momenta_restatement.py, the plain-Python yardstick of cup3d_update_obstacles (no GPU).

Against the compiled reference: `op midstep` of oracle/_ref/ref_tool runs AdvectionDiffusion -> ExternalForcing -> UpdateObstacles ->
Penalization -> PressureProjection (setupOperators, main.cpp:15229-15246) with a synthetic obstacle.  The CPU oracle has every member of
that chain except UpdateObstacles, so the chain oracle -> restatement -> oracle reproduces the reference's step only if the restatement
computes the obstacle's new motion -- with the OLD motion the same chain misses by a quarter of the step's change, which is asserted too.
Bounds: the project's own for this pipeline (tests/test_gpu_dropin.py::test_resident_mode_with_an_obstacle).

By its own properties: a rigid velocity field gives its own translation and rotation back; the forced / blocked row edits."""
import numpy as np
import pytest

import cup3d_amd as cu
import fluid_momenta_restatement as R
import oracle_lib as O

EXT = 2 * np.pi
_midstep = {}


def midstep(tmp_path_factory, implicit):
    """the reference's `op midstep` and the two oracle chains (new motion from the restatement / old motion), once per `implicit`"""
    if implicit in _midstep:
        return _midstep[implicit]
    bpd, lmax, bc = (2, 2, 2), 2, ("periodic", "wall", "freespace")
    nu, umax_forced, lam, dt, step, nb = 0.01, 1.0, 1e4, 0.01, 4, 64
    args = O.ref_args(bpd, lmax, 1, EXT, bc, nu=nu, umax_forced=umax_forced, extra=["-poissonTol", "1e-12", "-poissonTolRel", "1e-10"])
    rng = np.random.default_rng(8)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    obst, chif = O.synthetic_obstacle(None, nb, 9)
    d = tmp_path_factory.mktemp(f"midstep{implicit}")
    O.write_obstacle_file(str(d / "ob.bin"), obst)
    vel.tofile(str(d / "velb.bin")); pres.tofile(str(d / "presb.bin")); chif.tofile(str(d / "chib.bin"))
    O.run_ref(["tables t.bin", "obstacle ob.bin", "loadb vel velb.bin", "loadb pres presb.bin", "loadb chi chib.bin", f"set lambda {lam!r}",
               f"set implicit {implicit}", f"set step {step}", f"op midstep {dt!r}", "dump vel pv.bin", "dump pres pp.bin", "forces f.bin"],
              args, workdir=str(d))
    ref = (O.read_blocks(str(d / "pv.bin"), nb, 3), O.read_blocks(str(d / "pp.bin"), nb, 1), np.fromfile(str(d / "f.bin")))
    t, geom = O.read_tables(str(d / "t.bin"))
    assert len(t) == nb
    m = O.OracleMesh(bpd, lmax, EXT, bc, t[:, 0], t[:, 1])
    assert np.array_equal(m.tables, t)
    v1, _ = m.advect_diffuse(vel, dt, nu, (0.0, 0.0, 0.0))
    H = EXT   # sim.extents[1]: the three extents are equal here
    v1[..., 0] += 8 * umax_forced * nu / H / H * dt   # ExternalForcing, 10581-10596
    r = R.update(v1, geom, obst["ids"], obst["chi"], obst["udef"], obst["rigid"][0:3], lam, dt, implicit)
    chains = {}
    for tag, rigid in (("new", np.concatenate([obst["rigid"][0:3], r.vel, r.omega])), ("old", obst["rigid"])):
        ob = dict(obst, rigid=rigid)
        v2, f6 = m.penalize(v1, chif, ob, dt, lam, implicit)
        p2 = pres.copy()
        m.project_obst(v2, p2, dt, step, chif, ob, tol=1e-12, tol_rel=1e-10)
        chains[tag] = (v2, p2, f6)
    _midstep[implicit] = (vel, ref, chains, r, obst)
    return _midstep[implicit]


@pytest.mark.skipif(not O.have_ref_tool(), reason="oracle/_ref/ref_tool not built")
@pytest.mark.parametrize("implicit", [0, 1])
def test_restatement_reproduces_the_references_obstacle_step(tmp_path_factory, implicit):
    vel, ref, chains, r, obst = midstep(tmp_path_factory, implicit)
    change = np.abs(ref[0] - vel).max()
    assert change > 0.5 and len(obst["ids"]) < 64
    v, p, f6 = chains["new"]
    ev, ep, ef = np.abs(ref[0] - v).max() / change, np.abs(ref[1] - p).max() / np.abs(ref[1]).max(), np.abs(ref[2] - f6).max() / np.abs(ref[2]).max()
    miss = np.abs(ref[0] - chains["old"][0]).max() / change
    print(f"implicit {implicit}: velocity {ev:.3g} x change, pressure {ep:.3g}, force {ef:.3g}; old motion misses by {miss:.3g} x change")
    assert ev <= 1e-6
    assert ep <= 1e-6
    assert ef <= 1e-12
    assert miss > 0.1   # the test sees the operator
    assert np.isfinite(r.M).all() and r.M[0] > 0
    if not implicit:
        assert (r.M[13:] == 0).all() and np.isnan(r.rows[:, 13:]).all()


def rigid_case(implicit):
    """8 blocks (bpd 1,1,1 at level 1), a synthetic obstacle, vel = v0 + w0 x (x - cm)"""
    g = cu.Grid((1, 1, 1), 2, 1, EXT, ("periodic", "wall", "freespace"))
    assert g.nblocks == 8
    obst, _ = O.synthetic_obstacle(None, 8, 9)
    ids, chi = obst["ids"], obst["chi"]
    ax = np.arange(8) + 0.5
    pos = np.zeros((8, 8, 8, 8, 3))
    for s in range(8):
        h, o = g.geom[s, 0], g.geom[s, 1:4]
        pos[s, ..., 0] = (o[0] + h * ax)[None, None, :]
        pos[s, ..., 1] = (o[1] + h * ax)[None, :, None]
        pos[s, ..., 2] = (o[2] + h * ax)[:, None, None]
    if implicit:
        cm, udef = np.array([1.3, 2.9, 3.7]), np.zeros_like(obst["udef"])
    else:   # penalCM is 0 in this branch: the obstacle's own centroid
        w = np.where(chi > 0, chi, 0.0)
        cm, udef = (w[..., None] * pos[ids]).sum(axis=(0, 1, 2, 3)) / w.sum(), obst["udef"]
    v0, w0 = np.array([0.3, -0.2, 0.5]), np.array([0.11, 0.07, -0.13])
    vel = v0 + np.cross(np.broadcast_to(w0, pos.shape), pos - cm)
    return g, ids, chi, udef, cm, vel, v0, w0


@pytest.mark.parametrize("implicit", [0, 1])
def test_rigid_motion_in_rigid_motion_out(implicit):
    g, ids, chi, udef, cm, vel, v0, w0 = rigid_case(implicit)
    r = R.update(vel, g.geom, ids, chi, udef, cm, 1e4, 0.01, implicit)
    print(f"implicit {implicit}: |v - v0| = {np.abs(r.vel - v0).max():.3g}, |w - w0| = {np.abs(r.omega - w0).max():.3g}, cond(A) = {np.linalg.cond(r.A):.3g}")
    assert np.abs(r.vel - v0).max() <= 1e-12 and np.abs(r.omega - w0).max() <= 1e-12
    assert np.array_equal(r.vel, r.vel_computed) and np.array_equal(r.omega, r.omega_computed)


@pytest.mark.parametrize("implicit", [0, 1])
def test_forced_and_blocked_components(implicit):
    g, ids, chi, udef, cm, vel, v0, w0 = rigid_case(implicit)
    free = R.update(vel, g.geom, ids, chi, udef, cm, 1e4, 0.01, implicit)
    r = R.update(vel, g.geom, ids, chi, udef, cm, 1e4, 0.01, implicit, forced=(1, 0, 0), block_rotation=(0, 0, 1), vel_imposed=(0.7, 0.0, 0.0))
    assert r.vel[0] == 0.7 and r.omega[2] == 0.0
    assert abs(r.vel_computed[0] - 0.7) <= 4 * np.finfo(float).eps and r.omega_computed[2] == 0.0
    assert np.array_equal(r.M, free.M) and np.array_equal(r.rows, free.rows, equal_nan=True)   # the edits touch the solve only
    # rows 0 and 5 keep their diagonal; the other four equations are those of the free system, with the new unknowns
    assert np.array_equal(r.A[[1, 2, 3, 4]], free.A[[1, 2, 3, 4]]) and np.count_nonzero(r.A[0]) == 1 and np.count_nonzero(r.A[5]) == 1
    x = np.concatenate([r.vel_computed, r.omega_computed])
    assert np.abs(r.A @ x - r.b).max() <= 1e-12 * np.abs(r.b).max()
    assert not np.allclose(x[[1, 2, 3, 4]], np.concatenate([free.vel_computed, free.omega_computed])[[1, 2, 3, 4]], rtol=1e-6, atol=0)


def test_lu_solve_pivots():
    """a matrix whose leading entry is zero, and one that needs a swap in a later column"""
    rng = np.random.default_rng(1)
    for n in (2, 6):
        A = rng.uniform(-1, 1, (n, n))
        A[0, 0] = 0.0
        A[n - 1, n - 2] = 50.0
        b = rng.uniform(-1, 1, n)
        x = np.array(R.lu_solve(A.ravel().tolist(), b.tolist()))
        assert np.abs(x - np.linalg.solve(A, b)).max() <= 64 * np.finfo(float).eps * np.linalg.cond(A) * np.abs(x).max()


def test_skipped_cells_do_not_reach_a_sum():
    g, ids, chi, udef, cm, vel, v0, w0 = rigid_case(1)
    r = R.update(vel, g.geom, ids, chi, udef, cm, 1e4, 0.01, 1)
    bad = vel.copy()
    assert (chi <= 0).any()
    sub = bad[ids]
    sub[chi <= 0] = np.nan
    bad[ids] = sub
    q = R.update(bad, g.geom, ids, chi, udef, cm, 1e4, 0.01, 1)
    assert np.array_equal(q.rows, r.rows) and np.array_equal(q.M, r.M)
    # slot order, not list order
    perm = np.arange(len(ids))[::-1]
    q = R.update(vel, g.geom, ids[perm], chi[perm], udef[perm], cm, 1e4, 0.01, 1)
    assert np.array_equal(q.M, r.M) and np.array_equal(q.rows, r.rows[perm])
