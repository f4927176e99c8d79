"""tests/collision_restatement.py pinned by closed forms, conservation laws and the symmetry of a pair (no GPU)."""
import numpy as np
import pytest

import collision_cases as K
import collision_restatement as R

EPS = np.finfo(float).eps


def tensor(J):
    return np.array([[J[0], J[3], J[4]], [J[3], J[1], J[5]], [J[4], J[5], J[2]]])


def test_compute_j_is_the_inverse_inertia_times_the_arm_cross_the_normal():
    rng = np.random.default_rng(2)
    A = rng.uniform(-1, 1, (3, 3))
    T = A @ A.T + 3 * np.eye(3)
    J = [T[0, 0], T[1, 1], T[2, 2], T[0, 1], T[0, 2], T[1, 2]]
    Rc, Rr, N = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    want = np.linalg.solve(T, np.cross(Rc - Rr, N))
    assert np.abs(np.array(R.ComputeJ(Rc, Rr, N, J)) - want).max() <= 64 * EPS * np.linalg.cond(T) * np.abs(want).max()


def test_two_equal_spheres_head_on_exchange_their_velocities():
    """contact point on the line of centres, normal along it: no torque, and e = 1 swaps the normal velocities"""
    I = [0.4, 0.4, 0.4, 0.0, 0.0, 0.0]
    v1, v2 = [0.5, 0.1, 0.0], [-0.25, -0.2, 0.0]
    hv1, hv2, ho1, ho2 = R.ElasticCollision(2.0, 2.0, I, I, v1, v2, [0, 0, 0.3], [0, 0, 0], [0, 0, 0], [2, 0, 0], 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, v1, v2)
    assert np.allclose(hv1, [-0.25, 0.1, 0.0], rtol=0, atol=8 * EPS) and np.allclose(hv2, [0.5, -0.2, 0.0], rtol=0, atol=8 * EPS)
    assert ho1 == [0, 0, 0.3] and ho2 == [0, 0, 0]


def conservation_bound(before, after):
    """Linear: hv = v + (N / m) impulse, so m hv - m v = N impulse up to the three roundings of hv and of the product, each relative
    to a term no larger than m (|v| + |hv|): 8 eps sum_bodies m (|v| + |hv|).
    Angular about the origin: J ho - J o = J (J^-1 ((C - c) x N)) impulse, and ComputeJ forms J^-1 explicitly from cofactors, so the
    product returns (C - c) x N to 64 eps cond(J) -- the bound fluid_momenta_cases.velocity_bound allows two solves of one system -- of
    its own size; the m c x v terms add the linear error times |c|.  The scale is the sum of |J| |o|, |J| |ho|, m |c| |v| and
    m |c| |hv| over both bodies."""
    lin = sum(b["mass"] * (np.abs(b["vel"]).max() + np.abs(a["vel"]).max()) for b, a in zip(before, after))
    cond = max(np.linalg.cond(tensor(b["J"])) for b in before)
    ang = sum(np.abs(tensor(b["J"])).max() * 3 * (np.abs(b["omega"]).max() + np.abs(a["omega"]).max()) +
              b["mass"] * 2 * np.abs(b["cm"]).max() * (np.abs(b["vel"]).max() + np.abs(a["vel"]).max()) for b, a in zip(before, after))
    return 8 * EPS * lin, 64 * EPS * cond * ang


@pytest.mark.parametrize("name", K.NAMES)
def test_a_resolved_pair_of_free_bodies_conserves_momentum_and_angular_momentum(name):
    r, trace = K.expected(name, "approach")
    assert "resolved" in trace
    before = K.scenario(name, "approach")[2]

    def momenta(bodies):
        P = sum(b["mass"] * np.array(b["vel"]) for b in bodies)
        L = sum(tensor(b["J"]) @ np.array(b["omega"]) + b["mass"] * np.cross(np.array(b["cm"]), np.array(b["vel"])) for b in bodies)
        return P, L

    (P0, L0), (P1, L1) = momenta(before), momenta(r.bodies)
    lin, ang = conservation_bound(before, r.bodies)
    assert np.abs(P1 - P0).max() <= lin, (np.abs(P1 - P0).max(), lin)
    assert np.abs(L1 - L0).max() <= ang, (np.abs(L1 - L0).max(), ang)
    assert np.abs(P1 - P0).max() < 1e-3 * np.abs(np.array(r.bodies[0]["vel"]) - before[0]["vel"]).max() * before[0]["mass"]   # something did change


@pytest.mark.parametrize("name", K.NAMES)
@pytest.mark.parametrize("which", ["approach", "apart", "A_forced"])
def test_swapping_the_two_obstacles_swaps_the_roles(name, which):
    """The sums swap halves bit for bit (the same cells in the same order), the normal changes sign exactly and projVel is the same
    number; ElasticCollision's denominator adds its two torque terms in the other order, so the impulse agrees to 4 eps and the velocities to
    8 eps (|v| + |hv|)."""
    r, _ = K.expected(name, which)
    _, obst, bodies = K.scenario(name, which)
    s = R.prevent(K.CC.case(name).geom, obst[::-1], bodies[::-1], K.DT)
    a, b = np.array(r.sums), np.array(s.sums)
    assert np.array_equal(b[0, :10], a[0, 10:]) and np.array_equal(b[0, 10:], a[0, :10]) and np.array_equal(b[1, :10], a[1, 10:])
    assert (s.collided, s.any) == (r.collided, r.any)
    for x, y, z in zip(r.bodies, s.bodies[::-1], bodies):
        assert x["collision_counter"] == y["collision_counter"]
        for f in ("vel", "omega"):
            tol = 8 * EPS * (np.abs(z[f]).max() + np.abs(x[f]).max())
            assert np.abs(np.array(x[f]) - np.array(y[f])).max() <= tol, (f, x[f], y[f])


def test_over_ranks_keeps_the_momentum_of_the_rank_that_holds_the_maximum():
    one = [0.0] * 20
    lo, hi = list(one), list(one)
    lo[0], lo[4:7], lo[14:17] = 2.0, [0.1, 0.0, 0.0], [0.0, 0.3, 0.0]
    hi[0], hi[4:7], hi[14:17] = 3.0, [0.0, 0.2, 0.0], [0.0, 0.0, 0.1]
    (t,) = R.over_ranks([[lo], [hi]])
    assert t[0] == 5.0 and t[4:7] == [0.0, 0.2, 0.0] and t[14:17] == [0.0, 0.3, 0.0]
    # within 1e-10 of each other both survive and ADD, as written (14160-14161)
    near = list(hi)
    near[4:7] = [0.0, 0.2 + 1e-12, 0.0]
    (t,) = R.over_ranks([[hi], [near]])
    assert t[5] == 0.2 + (0.2 + 1e-12)
