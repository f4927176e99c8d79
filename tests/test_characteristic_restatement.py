"""Pins tests/characteristic_restatement.py, the plain-Python yardstick of cup3d_create_obstacles (no GPU).

No reference binary can run the operator (the harness's synthetic obstacle has no sdfLab), so the restatement is pinned by closed forms:

  a sphere   sdf = R - |x - c|, R = 1.3, c = (3.3, 3.0, 3.2) on uniform grids of extent 2 pi: the mass against 4/3 pi R^3 and the centre
             of mass against c.  Measured with the restatement (relative mass error / largest centre component error):
                 16^3   -2.594e-3 / 1.692e-3
                 32^3   +1.994e-5 / 2.912e-4
                 64^3   -1.982e-5 / 1.562e-5
             and each bound is twice the measured value.  The surface area sum(delta) is NOT pinned by convergence: it is -1.28 %, +2.07 %
             and +2.91 % off 4 pi R^2 at the three sizes and does not converge, because gradH is one-sided (and first-order wrong
             across the kink of chi) at block faces, which a finer grid has more of per surface area; only a loose 5 % is asserted.
  planes     sdf = a - x (and along y, z) with the band inside the block: per column sum(Delta) telescopes to h^2 (chi_in - chi_out)
             = h^2 to a few ulp, and band chi = -gradI / (1 + EPS); planes whose band touches index 0 and index 7 pin the
             one-sided branches against values worked out by hand.
  momenta    after kernelRemoveUdefMomenta the 13 sums of the corrected udef have M[1..6] at round-off."""
import numpy as np
import pytest

import characteristic_cases as CC
import characteristic_restatement as R
import cup3d_amd as cu

EPS = R.EPS
EXT = 2 * np.pi
SPHERE_R, SPHERE_C = 1.3, (3.3, 3.0, 3.2)
# level -> (cells per side, bound on |relative mass error|, bound on the centre-of-mass error): twice what the docstring records
SPHERE = {1: (16, 2 * 2.594e-3, 2 * 1.692e-3), 2: (32, 2 * 1.994e-5, 2 * 2.912e-4), 3: (64, 2 * 1.982e-5, 2 * 1.562e-5)}


def zeros():
    return [[[0.0] * 8 for _ in range(8)] for _ in range(8)]


@pytest.mark.parametrize("level", sorted(SPHERE))
def test_sphere_mass_and_centre_of_mass(level):
    n, mass_bound, com_bound = SPHERE[level]
    g = cu.operators.Grid((1, 1, 1), 4, level, EXT, ("periodic",) * 3)
    assert g.ncell == (n, n, n)
    ids = np.arange(g.nblocks)
    sdf = CC.sdf_tiles(g.geom, ids, CC.sphere(SPHERE_C, SPHERE_R))
    rows, area = [], 0.0
    for b in ids:
        _, row, pts = R.characteristic(sdf[b], g.geom[b, 0], g.geom[b, 1:4], zeros())
        rows.append(row)
        area += sum(p[6] for p in pts)
    com = R.grid_com(rows, ids)
    V = 4.0 / 3.0 * np.pi * SPHERE_R ** 3
    dm, dc, da = (com[0] - V) / V, np.abs(np.array(com[1:]) / com[0] - SPHERE_C).max(), area / (4 * np.pi * SPHERE_R ** 2) - 1
    print(f"{n}^3: relative mass error {dm:.4g}, centre of mass error {dc:.4g}, relative area error {da:.4g}")
    assert abs(dm) <= mass_bound
    assert dc <= com_bound
    assert abs(da) <= 0.05   # consistency only, see the docstring


def plane_sdf(axis, h, a, sign):
    """sdfLab of the block at the origin for sdf = sign * (a - coordinate along `axis`), axis 0 = x"""
    i = h * (np.arange(-1, 9) + 0.5)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    return sign * (a - (x, y, z)[axis])


def along(axis, a):
    """array [8][8][8] (z, y, x) -> the same with `axis` (0 = x) moved last, so that columns along the plane's normal are rows"""
    return np.moveaxis(np.asarray(a), 2 - axis, -1)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plane_inside_a_block(axis):
    h = EXT / 16
    a = 4.2 * h   # band cells 3 and 4; gradH is non-zero in cells 2..5, all with the central difference
    sdf = plane_sdf(axis, h, a, +1.0)
    field = zeros()
    chi, row, pts = R.characteristic(sdf, h, (0.0, 0.0, 0.0), field)
    assert np.array_equal(np.array(field), np.array(chi))   # max(chi, 0) into a cleared field
    chi = along(axis, chi)
    assert (chi[..., :3] == 1).all() and (chi[..., 5:] == 0).all()
    d = a - h * (np.arange(-1, 9) + 0.5)
    inv2h = .5 / h
    for i in (3, 4):
        gradI = inv2h * (max(0.0, d[i + 2]) - max(0.0, d[i]))   # d[i + 1] is cell i
        want = -gradI / (1 + EPS)
        assert np.abs(chi[..., i] - want).max() <= 4 * EPS * want, i
        assert 0 < want < 1
    assert len(pts) == 64 * 4
    cells = sorted({p[axis] for p in pts})
    assert cells == [2, 3, 4, 5]
    delta = np.zeros((8, 8, 8))
    for p in pts:
        delta[p[2], p[1], p[0]] = p[6]
        n = [-p[6] * (-1.0 if k == axis else 0.0) for k in range(3)]   # dchi = -delta * gradU, gradU = -e_axis
        assert np.abs(np.array(p[3:6]) - n).max() <= 4 * EPS * p[6]
    col = along(axis, delta).sum(axis=-1)
    assert np.abs(col - h * h).max() <= 8 * EPS * h * h   # h^2 (chi_in - chi_out)
    # the block's mass: the columns' chi
    assert abs(row[0] - 64 * h ** 3 * chi[0, 0].sum()) <= 512 * EPS * row[0]


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("low", [True, False])
def test_plane_at_a_block_face_takes_the_one_sided_branches(axis, low):
    """h = 1, block at the origin, the plane one cell from the face: band cells 0 and 1 (low) or 7 and 6 (high), inside towards the
    face.  By hand, with e = 1 + EPS: chi = 0.75 / e and 0.25 / e; gradH at the face cell 2 (2 * 0.25 - 1.5 * 0.75) / e = -1.25 / e (its
    sign follows the side), at the next two the central differences -0.75 / e and -0.25 / e; Delta = 0.5 |gradH| / e."""
    sdf = plane_sdf(axis, 1.0, 1.0, +1.0) if low else plane_sdf(axis, 1.0, 7.0, -1.0)
    chi, row, pts = R.characteristic(sdf, 1.0, (0.0, 0.0, 0.0), zeros())
    chi = along(axis, chi)
    e = 1 + EPS
    face, step = (0, 1) if low else (7, -1)
    assert np.allclose(chi[..., face], 0.75 / e, rtol=4 * EPS, atol=0) and np.allclose(chi[..., face + step], 0.25 / e, rtol=4 * EPS, atol=0)
    rest = [i for i in range(8) if i not in (face, face + step)]
    assert (chi[..., rest] == 0).all()
    want = {face: 0.625 / e / e, face + step: 0.375 / e / e, face + 2 * step: 0.125 / e / e}
    assert len(pts) == 64 * 3
    for p in pts:
        assert p[axis] in want
        assert abs(p[6] - want[p[axis]]) <= 4 * EPS * want[p[axis]], p
        n = [0.0, 0.0, 0.0]
        n[axis] = p[6] if low else -p[6]   # dchi = -delta * gradU, gradU = -/+ e_axis: it points out of the body
        assert np.abs(np.array(p[3:6]) - n).max() <= 4 * EPS * p[6]
    # push_back order: z, then y, then x
    order = [(p[2], p[1], p[0]) for p in pts]
    assert order == sorted(order)


@pytest.mark.parametrize("name", CC.NAMES)
def test_removed_momenta_are_gone(name):
    """The 13 sums re-evaluated on the corrected udef, with oldCorrVel = 0 and with the new correction: M[1..6] at round-off.  Bound, from
    the arithmetic: each of the N = 512 nblocks additions of a sum errs by at most eps times a partial sum <= M[0] max|udef| max(1, |p|),
    and the same holds for the sums the corrections were computed from; 4 N eps M[0] max|udef| max(1, |p|) covers both and the 3 x 3
    solve (cond(J) < 10 for these bodies).  Measured: below 1e-3 of that bound."""
    c = CC.case(name)
    _, first, _, _ = CC.expected(name)
    for o, r in zip(c.obstacles, first):
        ids = [int(b) for b in o["ids"]]
        N = 512 * len(ids)
        pmax = max(1.0, float(np.abs(c.geom[:, 1:4]).max() + 8 * c.geom[:, 0].max()))
        scale = r.mass * np.abs(o["udef"]).max() * pmax
        bound = 4 * N * EPS * scale
        for old in ((0.0, 0.0, 0.0), r.transvel_correction.tolist()):
            rows = [R.udef_momenta(r.chi[i].tolist(), r.udef[i], c.geom[b, 0], c.geom[b, 1:4], r.cm.tolist(), old) for i, b in enumerate(ids)]
            M = R.momenta_totals(rows, ids)
            print(name, "oldCorrVel", old, "max |M[1..6]| =", np.abs(M[1:7]).max(), "bound", bound)
            assert M[0] == r.udef_totals[0]
            assert np.abs(M[1:7]).max() <= bound
        assert np.abs(r.udef_totals[1:7]).max() > 1e6 * bound   # before the removal they were not small


def test_volume_asserts_and_invert_sym():
    c = CC.case("uniform8")
    with pytest.raises(R.VolumeError):
        R.create(c.geom, c.nb, [c.obstacles[0], c.nothing])
    with pytest.raises(R.VolumeError):
        R.accumulate([EPS] + [1.0] * 12)
    assert R.invertSym([1.0, 1.0, 0.0, 0.0, 0.0, 0.0]) == [0.0] * 6   # the detJ guard
    J = [2.0, 3.0, 4.0, 0.5, -0.25, 0.125]
    A = np.array([[J[0], J[3], J[4]], [J[3], J[1], J[5]], [J[4], J[5], J[2]]])
    inv = R.invertSym(J)
    B = np.array([[inv[0], inv[3], inv[4]], [inv[3], inv[1], inv[5]], [inv[4], inv[5], inv[2]]])
    assert np.abs(A @ B - np.eye(3)).max() <= 16 * EPS
