"""The restatement of KernelComputeForces::visit (tests/surface_forces_restatement.py) against analysis.  No GPU.

A 3 x 3 x 3-block level-0 grid, the centre block: its [-4,5) tile reads same-level neighbours only -- no boundary condition, no wrap.
The velocity is a quadratic, u_c = a_c + b_c . x + x^T C_c x with seeded coefficients in [-1, 1] on the 2 pi box; chi = 0 everywhere, so
the march along the normal stops at kk = 0 and the stencils sit on the surface cell; one surface point in every cell of the block;
seeded normals with every sign pattern.  The 6-point and 3-point first derivatives, the second and mixed differences and the Taylor
shift are exact for quadratics, so fxV, fyV, fzV must equal nu (grad u . d) and omegaX/Y/Z the analytic curl, within 1e-11 absolute: a
bound, not a measurement -- fewer than a hundred operations on O(10) values, divided by h ~ 0.26.

With chi = 0 the stencils never leave the surface cell, so the second and mixed differences and the Taylor shift are multiplied by zero.
A second run with chi = 1 (`shifted`) marches four cells out and back and pins those against the same analysis, under a bound of its own."""
import numpy as np
import pytest

import oracle_lib as O
import surface_forces_restatement as R

EXT = 2 * np.pi
NU = 0.013
TOL = 1e-11


def _build(chi_value, cells):
    bpd, bc = (3, 3, 3), ("periodic", "wall", "freespace")
    t = O.OracleGrid(bpd, 1, 0, EXT, bc).tables
    m = O.OracleMesh(bpd, 1, EXT, bc, t[:, 0].astype(np.int32), t[:, 1].copy())
    centre = [s for s in range(m.nb) if tuple(m.tables[s, 2:5]) == (1, 1, 1)][0]
    h = m.h(centre)
    assert abs(h - EXT / 24) < 1e-15
    rng = np.random.default_rng(5)
    a, b, Cm = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, (3, 3)), rng.uniform(-1, 1, (3, 3, 3))
    vel = np.zeros((m.nb, 8, 8, 8, 3))
    for s in range(m.nb):
        idx = m.tables[s, 2:5]
        ax = [(idx[d] * 8 + np.arange(8) + 0.5) * h for d in range(3)]
        Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        pos = np.stack([X, Y, Z], axis=-1)
        for c in range(3):
            vel[s, ..., c] = a[c] + pos @ b[c] + np.einsum("...i,ij,...j->...", pos, Cm[c], pos)
    chi = np.full((m.nb, 8, 8, 8), float(chi_value))
    pres = rng.uniform(-1, 1, (m.nb, 8, 8, 8))
    udef = rng.uniform(-1, 1, (8, 8, 8, 3))
    ijk = np.array([(x, y, z) for z in cells for y in cells for x in cells], dtype=np.int32)
    dchi = rng.uniform(0.1, 1, (len(ijk), 3))
    signs = np.array([[1 if (k >> d) & 1 else -1 for d in range(3)] for k in range(8)])
    dchi *= signs[np.arange(len(ijk)) % 8]   # every sign pattern, equally often
    assert {tuple(np.sign(v).astype(int)) for v in dchi} == {tuple(s) for s in signs}
    cm, utrans, omega = rng.uniform(0, EXT, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    qoi0 = rng.uniform(-1, 1, 19)
    origin = m.tables[centre, 2:5] * 8 * h
    trace = set()
    vt, ct = m.labs(vel, -4, 5, True)[centre], m.labs(chi, -4, 5, True)[centre]
    points, qoi = R.visit(vt, ct, pres[centre], h, origin, udef, ijk, dchi, cm, utrans, omega,
                          NU, qoi0, trace)
    return dict(vt=vt, ct=ct, h=h, origin=origin, b=b, C=Cm, vel=vel[centre], pres=pres[centre], udef=udef, ijk=ijk, dchi=dchi, cm=cm, utrans=utrans, omega=omega,
                qoi0=qoi0, points=dict(zip(R.POINT_NAMES, points)), qoi=dict(zip(R.QOI_NAMES, qoi)), trace=trace)


@pytest.fixture(scope="module")
def setup():
    return _build(0.0, range(8))   # one surface point in every cell of the block


@pytest.fixture(scope="module")
def shifted():
    """chi = 1 everywhere: the march never breaks and ends up to four cells away from the surface cell, so the second and mixed differences
    and the Taylor shift back (12375-12437) carry weight.  Surface cells 2..5 only: from there the march stays within [-2, 9], where the
    first derivatives take the 6- or 3-point branch and the mixed ones the full branch, all exact for quadratics (the 2-point and
    fallback branches, reached from the outer cells, are first-order and are not)."""
    return _build(1.0, range(2, 6))


def _grad(s):
    """analytic du_c/dx_j at every surface point: [n][3][3]"""
    pos = s["origin"] + s["h"] * (s["ijk"] + 0.5)
    return s["b"][None] + np.einsum("cij,nj->nci", s["C"] + s["C"].transpose(0, 2, 1), pos)


def test_the_march_stops_at_once_and_no_two_point_branch_is_used(setup):
    t = setup["trace"]
    assert "break_at_0" in t and not any(k.startswith("break_at_") and k != "break_at_0" for k in t) and "no_break" not in t
    assert not any(k.endswith("_2") or k.endswith("_fallback") for k in t)
    assert {"dveldx_6", "dveldx_3", "dveldy_6", "dveldy_3", "dveldz_6", "dveldz_3"} <= t


def test_viscous_force_is_nu_grad_u_dot_d(setup):
    s, G = setup, _grad(setup)
    d = s["dchi"] / np.sqrt((s["dchi"] ** 2).sum(axis=1))[:, None]
    want = NU * np.einsum("nci,ni->nc", G, d)
    for c, name in enumerate(("fxV", "fyV", "fzV")):
        err = np.abs(s["points"][name] - want[:, c]).max()
        print(name, "max abs error", err)
        assert err <= TOL, (name, err)


def test_vorticity_is_the_analytic_curl(setup):
    s, G = setup, _grad(setup)
    want = {"omegaX": G[:, 2, 1] - G[:, 1, 2], "omegaY": G[:, 0, 2] - G[:, 2, 0], "omegaZ": G[:, 1, 0] - G[:, 0, 1]}
    for name, w in want.items():
        err = np.abs(s["points"][name] - w).max()
        print(name, "max abs error", err)
        assert err <= TOL, (name, err)


def test_copies_are_exact(setup):
    s, p = setup, setup["points"]
    i, j, k = s["ijk"].T
    assert np.array_equal(p["P"], s["pres"][k, j, i])
    for c, (v, vd) in enumerate((("vX", "vxDef"), ("vY", "vyDef"), ("vZ", "vzDef"))):
        assert np.array_equal(p[v], s["vel"][k, j, i, c])
        assert np.array_equal(p[vd], s["udef"][k, j, i, c])
    for c, name in enumerate(("pX", "pY", "pZ")):
        assert np.array_equal(p[name], s["origin"][c] + s["h"] * (s["ijk"][:, c] + 0.5))
    d = s["dchi"] / np.sqrt((s["dchi"] ** 2).sum(axis=1))[:, None]
    for c, (f, fv) in enumerate((("fX", "fxV"), ("fY", "fyV"), ("fZ", "fzV"))):   # total = pressure + viscous part
        assert np.abs(p[f] - (-p["P"] * d[:, c] + p[fv])).max() <= 1e-14


def test_block_sums_are_left_to_right_sums_and_eight_carry_on(setup):
    """Every block sum is the left-to-right Python sum of the per-point terms, started from +0.0 for the eleven the functor zeroes and
    from the value given for the other eight.  The term of point i is what the functor adds for a block that holds that point alone,
    started from zero: 0 + t = t exactly (and for drag 0 - t = -t, so adding it is subtracting t)."""
    s, q = setup, setup["qoi"]
    zero = np.zeros(19)
    terms = np.zeros((512, 19))
    for i in range(512):
        _, terms[i] = R.visit(s["vt"], s["ct"], s["pres"], s["h"], s["origin"], s["udef"], s["ijk"][i:i + 1], s["dchi"][i:i + 1], s["cm"], s["utrans"],
                              s["omega"], NU, zero)
    for k, name in enumerate(R.QOI_NAMES):
        acc = float(s["qoi0"][k]) if name in R.CARRIED else 0.0
        for v in terms[:, k]:
            acc = acc + float(v)
        assert acc == q[name], name
        assert np.isfinite(acc) and (name not in R.CARRIED or acc != float(np.sum(terms[:, k])))   # the start value is in the sum
    assert set(R.CARRIED) == {"forcey", "forcez", "forcey_P", "forcez_P", "forcey_V", "forcez_V", "PoutBnd", "defPowerBnd"}
    assert len(R.ZEROED) == 11


# Bound for the shifted run, from the arithmetic and not from its outcome: |u| <= 1 + 3 * 5.3 + 9 * 5.3^2 < 270 on the tile, a difference
# quotient of up to nine terms errs by at most ~20 eps |u| = 6e-13 (eps = 1.1e-16), a gradient entry adds the first derivative and three
# second / mixed ones times shifts of up to 4 cells: 13 * 6e-13 = 8e-12, divided by h = 0.26: 3e-11; the curl subtracts two: 6e-11.
TOL_SHIFTED = 1e-10


def test_shifted_march_uses_the_taylor_terms_and_exact_branches_only(shifted):
    t = shifted["trace"]
    assert "no_break" in t and not any(k.startswith("break_at_") for k in t)
    assert not any(k.endswith("_2") or k.endswith("_fallback") for k in t), sorted(t)
    assert {"dveldxdy_full", "dveldydz_full", "dveldxdz_full"} <= t


def test_shifted_viscous_force_and_vorticity_are_analytic(shifted):
    s, G = shifted, _grad(shifted)
    d = s["dchi"] / np.sqrt((s["dchi"] ** 2).sum(axis=1))[:, None]
    want = NU * np.einsum("nci,ni->nc", G, d)
    for c, name in enumerate(("fxV", "fyV", "fzV")):
        err = np.abs(s["points"][name] - want[:, c]).max()
        print(name, "max abs error", err)
        assert err <= TOL_SHIFTED * NU, (name, err)
    curl = {"omegaX": G[:, 2, 1] - G[:, 1, 2], "omegaY": G[:, 0, 2] - G[:, 2, 0], "omegaZ": G[:, 1, 0] - G[:, 0, 1]}
    for name, w in curl.items():
        err = np.abs(s["points"][name] - w).max()
        print(name, "max abs error", err)
        assert err <= TOL_SHIFTED, (name, err)
