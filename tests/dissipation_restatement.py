"""ComputeDissipation::operator() (main.cpp:10436-10447, KernelDissipation 10347-10434) and FixMassFlux::operator() (12199-12248) restated
in plain Python, line by line.  TEST INFRASTRUCTURE.

The yardstick of cup3d_compute_dissipation and cup3d_fix_mass_flux (cup3d_amd/csrc/diagnostics.hip), written from the reference's text and
not from the kernels: scalar float64 arithmetic (Python floats: IEEE doubles, no contraction) in the reference's association, on the
ghosted [-1,2) tiles the oracle builds (oracle_lib.OracleMesh.labs(field, -1, 2); a uniform grid is the one-level mesh of its blocks).

  cell_terms       the 20 summands of one cell, QOI order (the term of QOI[15] is the one the reference SUBTRACTS)
  block_sums       one block: 20 sums from 0.0 over its 512 cells in iz, iy, ix order (QOI[15] by -=)
  totals           the block rows added from 0.0 in ascending slot order -- the association the library defines
  one_thread       the reference with one OpenMP thread: ONE running sum per quantity over all cells of all blocks, in long double
                   (np.longdouble: 64-bit mantissa on x86) and in float64; on a one-block grid the float64 form equals totals(block_sums)
  block_sums_fast  block_sums with NumPy doing each IEEE operation on all 512 cells at once (every ufunc is one correctly rounded
                   operation per element, np.add.accumulate adds strictly in index order): the same bits, ~100 times faster;
                   tests/test_dissipation_restatement.py holds it to block_sums bit for bit
  fix_mass_flux    the five numbers of the printf at 12229-12234 and the new vel

`mutation` (block_sums, block_sums_fast, cell_terms) deliberately breaks one line, for the catalogue of tests/test_dissipation_restatement.py."""
import math

import numpy as np

NQOI = 20
MUTATIONS = ("hhh_for_pow", "d12_without_half", "plus_for_minus_15", "center_left_out", "chi_ignored", "half_for_third")


def cell_terms(U, P, X, h, origin, center, nu, ix, iy, iz, mutation=None):
    """U [10][10][10][3], P [10][10][10] nested lists of the block's tiles (index [z+1][y+1][x+1]), X the cell's chi"""
    hCube, inv2h, invHh = math.pow(h, 3), .5 / h, 1 / (h * h)   # 10362
    if mutation == "hhh_for_pow":
        hCube = h * h * h
    L = U[iz + 1][iy + 1][ix + 1]
    LW, LE = U[iz + 1][iy + 1][ix], U[iz + 1][iy + 1][ix + 2]
    LS, LN = U[iz + 1][iy][ix + 1], U[iz + 1][iy + 2][ix + 1]
    LF, LB = U[iz][iy + 1][ix + 1], U[iz + 2][iy + 1][ix + 1]
    p = [origin[0] + h * (ix + 0.5), origin[1] + h * (iy + 0.5), origin[2] + h * (iz + 0.5)]   # Info::pos, 369-373
    c = (0.0, 0.0, 0.0) if mutation == "center_left_out" else center
    PX, PY, PZ = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    if mutation == "chi_ignored":
        X = 0.0
    WX = inv2h * ((LN[2] - LS[2]) - (LB[1] - LF[1]))
    WY = inv2h * ((LB[0] - LF[0]) - (LE[2] - LW[2]))
    WZ = inv2h * ((LE[1] - LW[1]) - (LN[0] - LS[0]))
    dPdx = inv2h * (P[iz + 1][iy + 1][ix + 2] - P[iz + 1][iy + 1][ix])
    dPdy = inv2h * (P[iz + 1][iy + 2][ix + 1] - P[iz + 1][iy][ix + 1])
    dPdz = inv2h * (P[iz + 2][iy + 1][ix + 1] - P[iz][iy + 1][ix + 1])
    lapU = invHh * (LE[0] + LW[0] + LN[0] + LS[0] + LB[0] + LF[0] - 6 * L[0])
    lapV = invHh * (LE[1] + LW[1] + LN[1] + LS[1] + LB[1] + LF[1] - 6 * L[1])
    lapW = invHh * (LE[2] + LW[2] + LN[2] + LS[2] + LB[2] + LF[2] - 6 * L[2])
    V1 = lapU * L[0] + lapV * L[1] + lapW * L[2]
    D11 = inv2h * (LE[0] - LW[0])
    D22 = inv2h * (LN[1] - LS[1])
    D33 = inv2h * (LB[2] - LF[2])
    D12 = inv2h * (LN[0] - LS[0] + LE[1] - LW[1]) / 2
    if mutation == "d12_without_half":
        D12 = inv2h * (LN[0] - LS[0] + LE[1] - LW[1])
    D13 = inv2h * (LB[0] - LF[0] + LE[2] - LW[2]) / 2
    D23 = inv2h * (LN[2] - LS[2] + LB[1] - LF[1]) / 2
    V2 = D11 * D11 + D22 * D22 + D33 * D33 + 2 * (D12 * D12 + D13 * D13 + D23 * D23)
    third = 2 if mutation == "half_for_third" else 3
    return [hCube * WX,
            hCube * WY,
            hCube * WZ,
            hCube / 2 * (PY * WZ - PZ * WY),
            hCube / 2 * (PZ * WX - PX * WZ),
            hCube / 2 * (PX * WY - PY * WX),
            hCube * L[0],
            hCube * L[1],
            hCube * L[2],
            hCube / third * (PX * (PY * WY + PZ * WZ) - WX * (PY * PY + PZ * PZ)),
            hCube / third * (PY * (PX * WX + PZ * WZ) - WY * (PX * PX + PZ * PZ)),
            hCube / third * (PZ * (PX * WX + PY * WY) - WZ * (PX * PX + PY * PY)),
            hCube * (PY * L[2] - PZ * L[1]),
            hCube * (PZ * L[0] - PX * L[2]),
            hCube * (PX * L[1] - PY * L[0]),
            (1 - X) * hCube * (dPdx * L[0] + dPdy * L[1] + dPdz * L[2]),
            (1 - X) * hCube * nu * (V1 + 2 * V2),
            hCube * (WX * L[0] + WY * L[1] + WZ * L[2]),
            hCube * (L[0] * L[0] + L[1] * L[1] + L[2] * L[2]) / 2,
            hCube * math.sqrt(WX * WX + WY * WY + WZ * WZ)]


def _lists(vel_lab, pres_lab, chi):
    return (np.asarray(vel_lab, dtype=np.float64).reshape(10, 10, 10, 3).tolist(), np.asarray(pres_lab, dtype=np.float64).reshape(10, 10, 10).tolist(),
            np.asarray(chi, dtype=np.float64).reshape(8, 8, 8).tolist())


def block_sums(vel_lab, pres_lab, chi, geom4, extents, nu, mutation=None):
    """One block: vel_lab [10][10][10][3], pres_lab [10][10][10] (the [-1,2) tiles, z, y, x order), chi [8][8][8], geom4 = h, origin."""
    U, P, CHI = _lists(vel_lab, pres_lab, chi)
    h, origin = float(geom4[0]), [float(v) for v in geom4[1:4]]
    center = (float(extents[0]) / 2, float(extents[1]) / 2, float(extents[2]) / 2)   # 10357
    nu = float(nu)
    Q = [0.0] * NQOI
    for iz in range(8):
        for iy in range(8):
            for ix in range(8):
                t = cell_terms(U, P, CHI[iz][iy][ix], h, origin, center, nu, ix, iy, iz, mutation)
                for k in range(NQOI):
                    if k == 15 and mutation != "plus_for_minus_15":
                        Q[k] -= t[k]
                    else:
                        Q[k] += t[k]
    return Q


def totals(rows):
    """the blocks' rows [nb][20] (slot order) added from 0.0 in ascending slot order"""
    T = [0.0] * NQOI
    for row in rows:
        for k in range(NQOI):
            T[k] += float(row[k])
    return T


def one_thread(vel_labs, pres_labs, chi, geom, extents, nu, dtype=np.longdouble):
    """The reference under one OpenMP thread: one running sum per quantity over all cells of all blocks (block order, then iz, iy, ix), the
    float64 summands accumulated in `dtype`.  Returns (sums [20] in dtype, sum of |summand| [20] as float64, number of cells)."""
    center = (float(extents[0]) / 2, float(extents[1]) / 2, float(extents[2]) / 2)
    Q = [dtype(0.0)] * NQOI
    A = [0.0] * NQOI
    n = 0
    for b in range(len(geom)):
        U, P, CHI = _lists(vel_labs[b], pres_labs[b], chi[b])
        h, origin = float(geom[b][0]), [float(v) for v in geom[b][1:4]]
        for iz in range(8):
            for iy in range(8):
                for ix in range(8):
                    t = cell_terms(U, P, CHI[iz][iy][ix], h, origin, center, float(nu), ix, iy, iz)
                    for k in range(NQOI):
                        Q[k] = Q[k] - dtype(t[k]) if k == 15 else Q[k] + dtype(t[k])
                        A[k] += abs(t[k])
                    n += 1
    return Q, A, n


def block_terms_fast(vel_lab, pres_lab, chi, geom4, extents, nu, mutation=None):
    """cell_terms on all 512 cells of a block at once: [20][8][8][8] (z, y, x)"""
    U = np.asarray(vel_lab, dtype=np.float64).reshape(10, 10, 10, 3)
    P = np.asarray(pres_lab, dtype=np.float64).reshape(10, 10, 10)
    X = np.asarray(chi, dtype=np.float64).reshape(8, 8, 8)
    h = float(geom4[0])
    hCube, inv2h, invHh = math.pow(h, 3), .5 / h, 1 / (h * h)
    if mutation == "hhh_for_pow":
        hCube = h * h * h
    c = slice(1, 9)
    L = [U[c, c, c, k] for k in range(3)]
    LW, LE = [U[c, c, 0:8, k] for k in range(3)], [U[c, c, 2:10, k] for k in range(3)]
    LS, LN = [U[c, 0:8, c, k] for k in range(3)], [U[c, 2:10, c, k] for k in range(3)]
    LF, LB = [U[0:8, c, c, k] for k in range(3)], [U[2:10, c, c, k] for k in range(3)]
    i = np.arange(8)
    cen = (0.0, 0.0, 0.0) if mutation == "center_left_out" else (float(extents[0]) / 2, float(extents[1]) / 2, float(extents[2]) / 2)
    ones = np.ones((8, 8, 8))
    PX = ((float(geom4[1]) + h * (i + 0.5)) - cen[0])[None, None, :] * ones
    PY = ((float(geom4[2]) + h * (i + 0.5)) - cen[1])[None, :, None] * ones
    PZ = ((float(geom4[3]) + h * (i + 0.5)) - cen[2])[:, None, None] * ones
    if mutation == "chi_ignored":
        X = np.zeros((8, 8, 8))
    WX = inv2h * ((LN[2] - LS[2]) - (LB[1] - LF[1]))
    WY = inv2h * ((LB[0] - LF[0]) - (LE[2] - LW[2]))
    WZ = inv2h * ((LE[1] - LW[1]) - (LN[0] - LS[0]))
    dPdx = inv2h * (P[c, c, 2:10] - P[c, c, 0:8])
    dPdy = inv2h * (P[c, 2:10, c] - P[c, 0:8, c])
    dPdz = inv2h * (P[2:10, c, c] - P[0:8, c, c])
    lapU = invHh * (LE[0] + LW[0] + LN[0] + LS[0] + LB[0] + LF[0] - 6 * L[0])
    lapV = invHh * (LE[1] + LW[1] + LN[1] + LS[1] + LB[1] + LF[1] - 6 * L[1])
    lapW = invHh * (LE[2] + LW[2] + LN[2] + LS[2] + LB[2] + LF[2] - 6 * L[2])
    V1 = lapU * L[0] + lapV * L[1] + lapW * L[2]
    D11 = inv2h * (LE[0] - LW[0])
    D22 = inv2h * (LN[1] - LS[1])
    D33 = inv2h * (LB[2] - LF[2])
    D12 = inv2h * (LN[0] - LS[0] + LE[1] - LW[1]) / 2
    if mutation == "d12_without_half":
        D12 = inv2h * (LN[0] - LS[0] + LE[1] - LW[1])
    D13 = inv2h * (LB[0] - LF[0] + LE[2] - LW[2]) / 2
    D23 = inv2h * (LN[2] - LS[2] + LB[1] - LF[1]) / 2
    V2 = D11 * D11 + D22 * D22 + D33 * D33 + 2 * (D12 * D12 + D13 * D13 + D23 * D23)
    third = 2 if mutation == "half_for_third" else 3
    nu = float(nu)
    return np.array([hCube * WX,
                     hCube * WY,
                     hCube * WZ,
                     hCube / 2 * (PY * WZ - PZ * WY),
                     hCube / 2 * (PZ * WX - PX * WZ),
                     hCube / 2 * (PX * WY - PY * WX),
                     hCube * L[0],
                     hCube * L[1],
                     hCube * L[2],
                     hCube / third * (PX * (PY * WY + PZ * WZ) - WX * (PY * PY + PZ * PZ)),
                     hCube / third * (PY * (PX * WX + PZ * WZ) - WY * (PX * PX + PZ * PZ)),
                     hCube / third * (PZ * (PX * WX + PY * WY) - WZ * (PX * PX + PY * PY)),
                     hCube * (PY * L[2] - PZ * L[1]),
                     hCube * (PZ * L[0] - PX * L[2]),
                     hCube * (PX * L[1] - PY * L[0]),
                     (1 - X) * hCube * (dPdx * L[0] + dPdy * L[1] + dPdz * L[2]),
                     (1 - X) * hCube * nu * (V1 + 2 * V2),
                     hCube * (WX * L[0] + WY * L[1] + WZ * L[2]),
                     hCube * (L[0] * L[0] + L[1] * L[1] + L[2] * L[2]) / 2,
                     hCube * np.sqrt(WX * WX + WY * WY + WZ * WZ)])


def block_sums_fast(vel_lab, pres_lab, chi, geom4, extents, nu, mutation=None):
    """block_sums by block_terms_fast: the summands behind a leading 0.0, accumulated in index order (a - x is a + (-x) exactly)"""
    t = block_terms_fast(vel_lab, pres_lab, chi, geom4, extents, nu, mutation).reshape(NQOI, 512)
    if mutation != "plus_for_minus_15":
        t[15] = -t[15]
    return np.add.accumulate(np.concatenate([np.zeros((NQOI, 1)), t], axis=1), axis=1)[:, -1].tolist()


def abs_sums(vel_lab, pres_lab, chi, geom4, extents, nu):
    """sum of |summand| of one block, per quantity: what the rounding bounds are stated in"""
    return np.abs(block_terms_fast(vel_lab, pres_lab, chi, geom4, extents, nu)).reshape(NQOI, 512).sum(axis=1)


def fix_mass_flux(vel, geom, uMax_forced, nu, dt, extents, uinf, allreduce=None):
    """vel [nb][8][8][8][3] (slot order), geom [nb][4].  avgUx_nonUniform (12199-12216): every block's 512 terms (u + uinf[0]) * h3 added
    from 0.0 in z, y, x order, the block sums from 0.0 in slot order (the library's association), / volume; allreduce: what turns this
    rank's value into the sum over ranks (12224), None on one rank.  Returns ({u_avg_msr, u_avg, delta_u, scale, re_tau}, new vel)."""
    vel = np.array(vel, dtype=np.float64)
    volume = float(extents[0]) * float(extents[1]) * float(extents[2])
    y_max = float(extents[1])
    u_avg = 2.0 / 3.0 * float(uMax_forced)
    avgUx = 0.
    for b in range(len(geom)):
        h = float(geom[b][0])
        h3 = h * h * h
        s = 0.0
        for u in vel[b, :, :, :, 0].reshape(512).tolist():
            s += (u + float(uinf[0])) * h3
        avgUx += s
    avgUx = avgUx / volume
    u_avg_msr = avgUx if allreduce is None else allreduce(avgUx)
    delta_u = u_avg - u_avg_msr
    reTau = math.sqrt(math.fabs(delta_u / float(dt))) / float(nu)
    scale = 6 * delta_u
    for b in range(len(geom)):
        h, oy = float(geom[b][0]), float(geom[b][2])
        for y in range(8):
            p1 = oy + h * (y + 0.5)
            aux = 6 * scale * p1 / y_max * (1.0 - p1 / y_max)
            vel[b, :, y, :, 0] += aux
    return dict(u_avg_msr=u_avg_msr, u_avg=u_avg, delta_u=delta_u, scale=scale, re_tau=reTau), vel
