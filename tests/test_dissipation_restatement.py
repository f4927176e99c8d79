"""tests/dissipation_restatement.py by its own properties, and the MUTATION CATALOGUE of the cases the GPU tests use (no GPU).

The restatement is the yardstick of cup3d_compute_dissipation and cup3d_fix_mass_flux; the oracle has no such function, so what pins the
yardstick is: closed forms it must reproduce (a rigid rotation, Taylor-Green at the second-order rate), identities (chi = 1), its distance
from a long-double running sum within the textbook bound, and the catalogue: every line of KernelDissipation that is easy to get wrong,
broken on purpose, must move a total by more than 1e6 u sum|t_i| on every case -- otherwise the bit-for-bit comparison on the device
would not be telling these apart from rounding."""
import math

import numpy as np
import pytest

import dissipation_cases as D
import dissipation_restatement as R
import oracle_lib as O

EXT = D.EXT


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------- the vectorised form is the scalar form
@pytest.mark.parametrize("name", D.SMALL)
def test_fast_form_is_the_scalar_form_bit_for_bit(name):
    c = D.case(name)
    blocks = list(range(c.nb)) if c.nb <= 24 else list(range(0, c.nb, max(1, c.nb // 12)))
    assert np.array_equal(bits(D.rows(c, fast=True, blocks=blocks)), bits(D.rows(c, fast=False, blocks=blocks)))
    for m in R.MUTATIONS:
        assert np.array_equal(bits(D.rows(c, True, m, blocks=blocks[:2])), bits(D.rows(c, False, m, blocks=blocks[:2]))), m


def test_fast_form_on_a_sample_of_the_large_case():
    c = D.case("blocks_1280")
    blocks = [0, 1, 319, 640, 1279]
    assert np.array_equal(bits(D.rows(c, fast=True, blocks=blocks)), bits(D.rows(c, fast=False, blocks=blocks)))
    assert np.array_equal(bits(D.expected("blocks_1280")[0][blocks]), bits(D.rows(c, fast=False, blocks=blocks)))


# ---------------------------------------------------------------- closed forms
def test_rigid_rotation_on_interior_blocks():
    """u = Omega x (x - c) is linear: central differences are exact up to rounding.  Interior blocks of the all-periodic (2,2,2) level-1
    grid... have no interior at 4 blocks a side unless the tiles come from the analytic field itself: the [-1,2) tiles are filled with
    the linear field, ghosts included, so that no ghost rule enters."""
    Om, cen = np.array([0.3, -0.7, 1.1]), np.array([EXT / 2] * 3)
    h = EXT / 32
    ext = [EXT] * 3
    for idx in ((1, 1, 1), (2, 1, 2), (1, 2, 1)):
        origin = np.array(idx) * 8 * h
        i = np.arange(-1, 9)
        z, y, x = np.meshgrid(origin[2] + h * (i + 0.5), origin[1] + h * (i + 0.5), origin[0] + h * (i + 0.5), indexing="ij")
        r = np.stack([x, y, z], -1) - cen
        U = np.cross(np.broadcast_to(Om, r.shape), r)
        P = np.zeros((10, 10, 10))
        q = np.array(R.block_sums(U, P, np.zeros((8, 8, 8)), [h, *origin], ext, 0.02))
        V = 512 * h ** 3
        assert np.allclose(q[0:3], 2 * Om * V, rtol=1e-12)                        # curl = 2 Omega
        assert abs(q[16]) < 1e-12                                                 # rigid motion: no strain, zero Laplacian
        assert math.isclose(q[17], 2 * Om @ U[1:9, 1:9, 1:9].reshape(-1, 3).sum(0) * h ** 3, rel_tol=1e-12, abs_tol=1e-12)
        assert math.isclose(q[19], 2 * np.linalg.norm(Om) * V, rel_tol=1e-12)
        rr = r[1:9, 1:9, 1:9].reshape(-1, 3)
        L = (np.cross(rr, np.cross(np.broadcast_to(Om, rr.shape), rr))).sum(0) * h ** 3   # angular momentum about c, closed form per cell
        assert np.allclose(q[12:15], L, rtol=1e-12, atol=1e-12)
        assert np.allclose(q[6:9], U[1:9, 1:9, 1:9].reshape(-1, 3).sum(0) * h ** 3, rtol=1e-12, atol=1e-13)


def _taylor_green_totals(level):
    bc = ("periodic", "periodic", "periodic")
    g = O.OracleGrid((1, 1, 1), level + 1, level, EXT, bc)
    vel = g.taylor_green([EXT] * 3, 1.0)
    m = O.OracleMesh((1, 1, 1), level + 1, EXT, bc, g.tables[:, 0].astype(np.int32), g.tables[:, 1].copy())
    assert np.array_equal(m.tables, g.tables)
    labs, plabs = m.labs(vel, -1, 2), np.zeros((g.nb, 10, 10, 10))
    rows = [R.block_sums_fast(labs[b], plabs[b], np.zeros((8, 8, 8)), g.geom[b], [EXT] * 3, 1.0) for b in range(g.nb)]
    return np.array(R.totals(rows))


def test_taylor_green_second_order():
    """u = (cos x sin y sin z, -sin x cos y sin z, 0) from orc_ic_taylor_green, all periodic, 16^3 and 32^3.
    Kinetic energy: L^3/8, and the midpoint sum of a trigonometric polynomial is exact, so it agrees to rounding at both sizes.
    Enstrophy E = integral |omega|^2 = 3 L^3/4 enters QOI[16] twice: with nu = 1 and chi = 0 it is sum(u . lap_h u) + sum(2 D_h : D_h)
    = -(2 sin(h/2) / h)^2 E + (sin(h) / h)^2 E, the two discrete enstrophies, whose analytic values cancel (the viscous power of a
    periodic flow integrates to zero): each agrees with E at second order, so their sum tends to 0 = its analytic value at that rate.
    integral |omega| (QOI[19]) against a 256^3 midpoint quadrature of the analytic |omega|, the same rate."""
    exact_ke, exact_ens = EXT ** 3 / 8, 3 * EXT ** 3 / 4
    t16, t32 = _taylor_green_totals(1), _taylor_green_totals(2)
    assert math.isclose(t16[18], exact_ke, rel_tol=1e-13) and math.isclose(t32[18], exact_ke, rel_tol=1e-13)
    for t, h in ((t16, EXT / 16), (t32, EXT / 32)):   # ... and it is that difference of the two discrete enstrophies, to rounding
        assert math.isclose(t[16], exact_ens * ((math.sin(h) / h) ** 2 - (2 * math.sin(h / 2) / h) ** 2), rel_tol=1e-10)
    order = math.log2(abs(t16[16]) / abs(t32[16]))
    x = (np.arange(256) + 0.5) * (EXT / 256)
    cx, sx = np.cos(x), np.sin(x)
    w2 = ((sx[None, None, :] * cx[None, :, None] * cx[:, None, None]) ** 2 + (cx[None, None, :] * sx[None, :, None] * cx[:, None, None]) ** 2
          + (2 * cx[None, None, :] * cx[None, :, None] * sx[:, None, None]) ** 2)
    exact_abs = float(np.sqrt(w2).sum()) * (EXT / 256) ** 3
    e16, e32 = abs(t16[19] - exact_abs), abs(t32[19] - exact_abs)
    order_abs = math.log2(e16 / e32)
    print(f"viscous power (two discrete enstrophies) 16^3 {t16[16]:.3e}, 32^3 {t32[16]:.3e}: observed order {order:.3f}; "
          f"integral |omega| error 16^3 {e16:.3e}, 32^3 {e32:.3e}: observed order {order_abs:.3f}")
    assert order > 1.8 and order_abs > 1.8
    assert abs(t32[17]) < 1e-12 * exact_ens and np.abs(t32[0:3]).max() < 1e-12 * exact_ens      # no helicity, no net vorticity


def test_chi_one_zeroes_both_powers_exactly():
    c = D.case("sixteen_mixed")
    for b in (0, 7, 15):
        q = R.block_sums(c.vel_labs[b], c.pres_labs[b], np.ones((8, 8, 8)), c.geom[b], c.extents, D.NU)
        assert q[15] == 0.0 and q[16] == 0.0
        assert all(v != 0.0 for k, v in enumerate(q) if k not in (15, 16))


@pytest.mark.parametrize("name", ["one_block", "sixteen_mixed", "l012_wall"])
def test_float64_against_the_long_double_running_sum(name):
    """|float64 totals - one long-double running sum| <= gamma_N sum|t_i| per quantity, N = number of cells (Higham, Thm 4.? recursive summation:
    any order of N - 1 additions); the long double sum's own error is 2^-11 of that"""
    c = D.case(name)
    q, A, n = R.one_thread(c.vel_labs, c.pres_labs, D.chi_of(c), c.geom, c.extents, D.NU, dtype=np.longdouble)
    assert n == 512 * c.nb
    tot = D.expected(name)[1]
    for k in range(20):
        assert abs(np.longdouble(tot[k]) - q[k]) <= D.gamma(n) * A[k], k
    if c.nb == 1:   # one block: the library's association IS the one-thread association
        q64, _, _ = R.one_thread(c.vel_labs, c.pres_labs, D.chi_of(c), c.geom, c.extents, D.NU, dtype=np.float64)
        assert np.array_equal(bits(np.array(q64, dtype=np.float64)), bits(tot))


# ---------------------------------------------------------------- the mutation catalogue
# mutation -> the cases where it cannot show, with the reason
NOT_APPLICABLE = {
    "pres_ghost_negated_at_wall": {"l012_periodic": "no wall"},
    "chi_ignored": {n: "chi is untouched (zero) in this case: ignoring it is the identity" for n, v in D.CASES.items() if not v[4]},
}


@pytest.mark.parametrize("name", list(D.CASES))
def test_mutation_catalogue(name):
    c = D.case(name)
    rows, tot, abs_rows = D.expected(name)
    floor = 1e6 * D.U * abs_rows.sum(axis=0)
    for m in R.MUTATIONS + ("pres_ghost_negated_at_wall",):
        if m == "pres_ghost_negated_at_wall":
            if name in NOT_APPLICABLE[m]:
                assert not D.wall_faces(c)
                continue
            assert D.wall_faces(c)
            mr = D.rows(c, pres_labs=D.pres_labs_with_negated_wall_ghosts(c))
        else:
            mr = D.rows(c, mutation=m)
        mt = np.array(R.totals(mr))
        moved = np.abs(mt - tot)
        if m == "hhh_for_pow":
            # shows only bitwise where it shows at all: far below the floor.  For every spacing of these cases (2 pi / (8 n)) the correctly
            # rounded pow(h, 3) and the twice-rounded h*h*h turn out to be the SAME double, so here it does not show: not applicable, for
            # that reason, which is asserted.  test_pow_and_hhh_differ_elsewhere shows the restatement telling them apart at h = 0.3.
            assert (moved <= floor).all()
            same = all(math.pow(float(h), 3) == float(h) * float(h) * float(h) for h in set(c.geom[:, 0].tolist()))
            assert np.array_equal(bits(mr), bits(rows)) == same
            continue
        if name in NOT_APPLICABLE.get(m, {}):
            assert np.array_equal(bits(mr), bits(rows)), (m, NOT_APPLICABLE[m][name])
            continue
        assert (moved > floor).any(), (m, float((moved / floor).max()))


def test_pow_and_hhh_differ_elsewhere():
    h = 0.3
    assert math.pow(h, 3) != h * h * h
    c = D.case("one_block")
    geom = [h, 0.0, 0.0, 0.0]
    a = R.block_sums(c.vel_labs[0], c.pres_labs[0], D.chi_of(c)[0], geom, [2.4] * 3, D.NU)
    b = R.block_sums(c.vel_labs[0], c.pres_labs[0], D.chi_of(c)[0], geom, [2.4] * 3, D.NU, "hhh_for_pow")
    assert not np.array_equal(bits(a), bits(b)) and np.allclose(a, b, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- FixMassFlux
def test_fix_mass_flux_restatement_properties():
    c = D.case("sixteen_mixed")
    out, vel = D.expected_mass_flux("sixteen_mixed")
    assert out["u_avg"] == 2.0 / 3.0 * D.UMAX_FORCED and out["scale"] == 6 * out["delta_u"] and out["delta_u"] == out["u_avg"] - out["u_avg_msr"]
    mean = ((c.vel[..., 0] + D.UINF[0]) * c.geom[:, 0, None, None, None] ** 3).sum() / np.prod(c.extents)
    assert math.isclose(out["u_avg_msr"], mean, rel_tol=1e-12)
    assert np.array_equal(vel[..., 1:], c.vel[..., 1:])
    # the correction is the parabola 6 * scale * y/H (1 - y/H): its volume mean is scale = 6 delta_u (the reference's second factor 6, kept)
    added = ((vel[..., 0] - c.vel[..., 0]) * c.geom[:, 0, None, None, None] ** 3).sum() / np.prod(c.extents)
    assert math.isclose(added, out["scale"], rel_tol=2e-3)     # midpoint rule on 16 cells across the channel: 1 - 1/(2 * 16^2)
    assert math.isclose(out["re_tau"], math.sqrt(abs(out["delta_u"] / D.DT)) / D.NU, rel_tol=1e-15)
