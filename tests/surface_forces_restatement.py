"""KernelComputeForces::visit (main.cpp:12273-12493) restated in plain Python, line by line.  TEST INFRASTRUCTURE.

The yardstick of k_surface_forces (cup3d_amd/csrc/obstacles_forces.hip) on inputs of the tests' choosing (every path of the functor:
tests/surface_forces_cases.py), written out once more from the reference's text and not from the kernel; the compiled reference runs the
functor on its own fish, and this restatement equals it there bit for bit (tests/test_fish_fixtures.py, tests/golden/fish_one_*.npz):
scalar float64 arithmetic (Python floats: IEEE doubles, no contraction) in the reference's association, `round` half away from zero,
sums added point by point in order i = 0..nPoints-1.  It is evaluated on [-4,5) tensorial tiles -- the CPU oracle's
(OracleMesh.labs(field, -4, 5, True), pinned bit for bit to the compiled reference) in the tests.

Kept as written in the reference: the `sx` (not `sy`) in the 2-point branch of dveldy (12364), and the precedence of the mixed
derivatives' fallback, sx*sy*(a - b) - (c - d) (12394-12395, 12406-12407, 12418-12419).

visit() zeroes eleven of the nineteen block sums at entry (12283-12293); the other eight -- forcey, forcez, forcey_P, forcez_P,
forcey_V, forcez_V, PoutBnd, defPowerBnd -- go on from the values they had: `qoi_in` is where they start.

`trace`, when given, is a set that collects the name of every path a point took (tests/test_surface_forces_cases.py).
"""
import math

import numpy as np

# the 19 per-point arrays the functor writes (12444-12462), in the order of cup3d_obstacle_surface::points
POINT_NAMES = ("pX", "pY", "pZ", "P", "fX", "fY", "fZ", "fxV", "fyV", "fzV", "omegaX", "omegaY", "omegaZ",
               "vxDef", "vX", "vyDef", "vY", "vzDef", "vZ")
# ObstacleBlock::sumQoI (7289-7307)
QOI_NAMES = ("forcex", "forcey", "forcez", "forcex_P", "forcey_P", "forcez_P", "forcex_V", "forcey_V", "forcez_V",
             "torquex", "torquey", "torquez", "drag", "thrust", "Pout", "PoutBnd", "defPower", "defPowerBnd", "pLocom")
ZEROED = ("forcex", "forcex_V", "forcex_P", "torquex", "torquey", "torquez", "thrust", "drag", "Pout", "defPower", "pLocom")  # 12283-12293
CARRIED = tuple(n for n in QOI_NAMES if n not in ZEROED)

BIG, SMALL, SIZE = 5, -4, 8
BIGG = SIZE + BIG - 1   # 12253
C0, C1, C2, C3, C4, C5 = -137. / 60., 5., -5., 10. / 3., -5. / 4., 1. / 5.   # 12256-12261


def inrange(i):   # 12262
    return i >= SMALL and i < BIGG


def c_round(v):
    """C's round(): to the nearest integer, halves away from zero"""
    a = abs(v)
    r = math.floor(a)
    if a - r >= 0.5:   # exact: a and r are less than one apart
        r += 1
    return int(r) if v >= 0 else -int(r)


def visit(vel_tile, chi_tile, pres_block, h, origin, udef, ijk, dchi, cm, utrans, omega, nu, qoi_in, trace=None):
    """One ObstacleBlock with nPoints = len(ijk) > 0.  vel_tile [16][16][16][3], chi_tile [16][16][16] (z, y, x; cell (x, y, z) of the
    block at [z+4][y+4][x+4]), pres_block [8][8][8], udef [8][8][8][3], ijk [n][3] = surface ix, iy, iz, dchi [n][3] = dchidx, dchidy,
    dchidz.  Returns (points [19][n], qoi [19])."""
    V = np.asarray(vel_tile, dtype=np.float64).reshape(16, 16, 16, 3).tolist()
    X = np.asarray(chi_tile, dtype=np.float64).reshape(16, 16, 16).tolist()
    PB = np.asarray(pres_block, dtype=np.float64).reshape(8, 8, 8).tolist()
    UD = np.asarray(udef, dtype=np.float64).reshape(8, 8, 8, 3).tolist()
    h = float(h)
    origin = [float(v) for v in origin]
    CM = [float(v) for v in cm]
    uTrans = [float(v) for v in utrans]
    omega = [float(v) for v in omega]
    nu = float(nu)
    n = len(ijk)
    assert n > 0   # 12280
    mark = (lambda s: None) if trace is None else trace.add

    def l(x, y, z, c):
        return V[z + 4][y + 4][x + 4][c]

    q = dict(zip(QOI_NAMES, (float(v) for v in qoi_in)))
    for name in ZEROED:   # 12283-12293
        q[name] = 0.0
    velUnit = [0., 0., 0.]
    vel_norm = math.sqrt(uTrans[0] * uTrans[0] + uTrans[1] * uTrans[1] + uTrans[2] * uTrans[2])
    if vel_norm > 1e-9:
        mark("vel_norm>1e-9")
        velUnit = [uTrans[0] / vel_norm, uTrans[1] / vel_norm, uTrans[2] / vel_norm]
    else:
        mark("vel_norm<=1e-9")
    _1oH = nu / h
    out = {name: [0.0] * n for name in POINT_NAMES}
    for i in range(n):
        ix, iy, iz = (int(v) for v in ijk[i])
        p = [origin[0] + h * (ix + 0.5), origin[1] + h * (iy + 0.5), origin[2] + h * (iz + 0.5)]   # Info::pos, 369-373
        normX, normY, normZ = (float(v) for v in dchi[i])
        norm = 1.0 / math.sqrt(normX * normX + normY * normY + normZ * normZ)
        dx = normX * norm
        dy = normY * norm
        dz = normZ * norm
        x, y, z = ix, iy, iz
        broke = False
        for kk in range(5):   # 12323-12341
            dxi = c_round(kk * dx)
            dyi = c_round(kk * dy)
            dzi = c_round(kk * dz)
            if ix + dxi + 1 >= SIZE + BIG - 1 or ix + dxi - 1 < SMALL:
                mark("continue_x")
                continue
            if iy + dyi + 1 >= SIZE + BIG - 1 or iy + dyi - 1 < SMALL:
                mark("continue_y")
                continue
            if iz + dzi + 1 >= SIZE + BIG - 1 or iz + dzi - 1 < SMALL:
                mark("continue_z")
                continue
            x = ix + dxi
            y = iy + dyi
            z = iz + dzi
            if X[z + 4][y + 4][x + 4] < 0.01:
                mark("break_at_%d" % kk)
                broke = True
                break
        if not broke:
            mark("no_break")
        sx = +1 if normX > 0 else -1
        sy = +1 if normY > 0 else -1
        sz = +1 if normZ > 0 else -1
        fsx, fsy, fsz = float(sx), float(sy), float(sz)
        dveldx, dveldy, dveldz = [0.] * 3, [0.] * 3, [0.] * 3
        dveldx2, dveldy2, dveldz2 = [0.] * 3, [0.] * 3, [0.] * 3
        dveldxdy, dveldxdz, dveldydz = [0.] * 3, [0.] * 3, [0.] * 3
        for c in range(3):   # VectorElement arithmetic is componentwise (5787-5836)
            if inrange(x + 5 * sx):
                mark("dveldx_6")
                dveldx[c] = fsx * (C0 * l(x, y, z, c) + C1 * l(x + sx, y, z, c) + C2 * l(x + 2 * sx, y, z, c) + C3 * l(x + 3 * sx, y, z, c) +
                                   C4 * l(x + 4 * sx, y, z, c) + C5 * l(x + 5 * sx, y, z, c))
            elif inrange(x + 2 * sx):
                mark("dveldx_3")
                dveldx[c] = fsx * (-1.5 * l(x, y, z, c) + 2.0 * l(x + sx, y, z, c) - 0.5 * l(x + 2 * sx, y, z, c))
            else:
                mark("dveldx_2")
                dveldx[c] = fsx * (l(x + sx, y, z, c) - l(x, y, z, c))
            if inrange(y + 5 * sy):
                mark("dveldy_6")
                dveldy[c] = fsy * (C0 * l(x, y, z, c) + C1 * l(x, y + sy, z, c) + C2 * l(x, y + 2 * sy, z, c) + C3 * l(x, y + 3 * sy, z, c) +
                                   C4 * l(x, y + 4 * sy, z, c) + C5 * l(x, y + 5 * sy, z, c))
            elif inrange(y + 2 * sy):
                mark("dveldy_3")
                dveldy[c] = fsy * (-1.5 * l(x, y, z, c) + 2.0 * l(x, y + sy, z, c) - 0.5 * l(x, y + 2 * sy, z, c))
            else:
                mark("dveldy_2")
                dveldy[c] = fsx * (l(x, y + sy, z, c) - l(x, y, z, c))   # sx, as written at 12364
            if inrange(z + 5 * sz):
                mark("dveldz_6")
                dveldz[c] = fsz * (C0 * l(x, y, z, c) + C1 * l(x, y, z + sz, c) + C2 * l(x, y, z + 2 * sz, c) + C3 * l(x, y, z + 3 * sz, c) +
                                   C4 * l(x, y, z + 4 * sz, c) + C5 * l(x, y, z + 5 * sz, c))
            elif inrange(z + 2 * sz):
                mark("dveldz_3")
                dveldz[c] = fsz * (-1.5 * l(x, y, z, c) + 2.0 * l(x, y, z + sz, c) - 0.5 * l(x, y, z + 2 * sz, c))
            else:
                mark("dveldz_2")
                dveldz[c] = fsz * (l(x, y, z + sz, c) - l(x, y, z, c))
            dveldx2[c] = l(x - 1, y, z, c) - 2.0 * l(x, y, z, c) + l(x + 1, y, z, c)
            dveldy2[c] = l(x, y - 1, z, c) - 2.0 * l(x, y, z, c) + l(x, y + 1, z, c)
            dveldz2[c] = l(x, y, z - 1, c) - 2.0 * l(x, y, z, c) + l(x, y, z + 1, c)
            if inrange(x + 2 * sx) and inrange(y + 2 * sy):
                mark("dveldxdy_full")
                dveldxdy[c] = float(sx * sy) * (
                    -0.5 * (-1.5 * l(x + 2 * sx, y, z, c) + 2.0 * l(x + 2 * sx, y + sy, z, c) - 0.5 * l(x + 2 * sx, y + 2 * sy, z, c)) +
                    2.0 * (-1.5 * l(x + sx, y, z, c) + 2.0 * l(x + sx, y + sy, z, c) - 0.5 * l(x + sx, y + 2 * sy, z, c)) -
                    1.5 * (-1.5 * l(x, y, z, c) + 2.0 * l(x, y + sy, z, c) - 0.5 * l(x, y + 2 * sy, z, c)))
            else:
                mark("dveldxdy_fallback")
                dveldxdy[c] = float(sx * sy) * (l(x + sx, y + sy, z, c) - l(x + sx, y, z, c)) - (l(x, y + sy, z, c) - l(x, y, z, c))
            if inrange(y + 2 * sy) and inrange(z + 2 * sz):
                mark("dveldydz_full")
                dveldydz[c] = float(sy * sz) * (
                    -0.5 * (-1.5 * l(x, y + 2 * sy, z, c) + 2.0 * l(x, y + 2 * sy, z + sz, c) - 0.5 * l(x, y + 2 * sy, z + 2 * sz, c)) +
                    2.0 * (-1.5 * l(x, y + sy, z, c) + 2.0 * l(x, y + sy, z + sz, c) - 0.5 * l(x, y + sy, z + 2 * sz, c)) -
                    1.5 * (-1.5 * l(x, y, z, c) + 2.0 * l(x, y, z + sz, c) - 0.5 * l(x, y, z + 2 * sz, c)))
            else:
                mark("dveldydz_fallback")
                dveldydz[c] = float(sy * sz) * (l(x, y + sy, z + sz, c) - l(x, y + sy, z, c)) - (l(x, y, z + sz, c) - l(x, y, z, c))
            if inrange(x + 2 * sx) and inrange(z + 2 * sz):
                mark("dveldxdz_full")
                dveldxdz[c] = float(sx * sz) * (
                    -0.5 * (-1.5 * l(x, y, z + 2 * sz, c) + 2.0 * l(x + sx, y, z + 2 * sz, c) - 0.5 * l(x + 2 * sx, y, z + 2 * sz, c)) +
                    2.0 * (-1.5 * l(x, y, z + sz, c) + 2.0 * l(x + sx, y, z + sz, c) - 0.5 * l(x + 2 * sx, y, z + sz, c)) -
                    1.5 * (-1.5 * l(x, y, z, c) + 2.0 * l(x + sx, y, z, c) - 0.5 * l(x + 2 * sx, y, z, c)))
            else:
                mark("dveldxdz_fallback")
                dveldxdz[c] = float(sx * sz) * (l(x + sx, y, z + sz, c) - l(x, y, z + sz, c)) - (l(x + sx, y, z, c) - l(x, y, z, c))
        ex, ey, ez = float(ix - x), float(iy - y), float(iz - z)
        dudx = dveldx[0] + dveldx2[0] * ex + dveldxdy[0] * ey + dveldxdz[0] * ez   # 12420-12437
        dvdx = dveldx[1] + dveldx2[1] * ex + dveldxdy[1] * ey + dveldxdz[1] * ez
        dwdx = dveldx[2] + dveldx2[2] * ex + dveldxdy[2] * ey + dveldxdz[2] * ez
        dudy = dveldy[0] + dveldy2[0] * ey + dveldydz[0] * ez + dveldxdy[0] * ex
        dvdy = dveldy[1] + dveldy2[1] * ey + dveldydz[1] * ez + dveldxdy[1] * ex
        dwdy = dveldy[2] + dveldy2[2] * ey + dveldydz[2] * ez + dveldxdy[2] * ex
        dudz = dveldz[0] + dveldz2[0] * ez + dveldxdz[0] * ex + dveldydz[0] * ey
        dvdz = dveldz[1] + dveldz2[1] * ez + dveldxdz[1] * ex + dveldydz[1] * ey
        dwdz = dveldz[2] + dveldz2[2] * ez + dveldxdz[2] * ex + dveldydz[2] * ey
        P = PB[iz][iy][ix]
        fXV = _1oH * (dudx * normX + dudy * normY + dudz * normZ)
        fYV = _1oH * (dvdx * normX + dvdy * normY + dvdz * normZ)
        fZV = _1oH * (dwdx * normX + dwdy * normY + dwdz * normZ)
        fXP, fYP, fZP = -P * normX, -P * normY, -P * normZ
        fXT, fYT, fZT = fXV + fXP, fYV + fYP, fZV + fZP
        out["pX"][i] = p[0]
        out["pY"][i] = p[1]
        out["pZ"][i] = p[2]
        out["P"][i] = P
        out["fX"][i] = -P * dx + _1oH * (dudx * dx + dudy * dy + dudz * dz)
        out["fY"][i] = -P * dy + _1oH * (dvdx * dx + dvdy * dy + dvdz * dz)
        out["fZ"][i] = -P * dz + _1oH * (dwdx * dx + dwdy * dy + dwdz * dz)
        out["fxV"][i] = _1oH * (dudx * dx + dudy * dy + dudz * dz)
        out["fyV"][i] = _1oH * (dvdx * dx + dvdy * dy + dvdz * dz)
        out["fzV"][i] = _1oH * (dwdx * dx + dwdy * dy + dwdz * dz)
        out["omegaX"][i] = (dwdy - dvdz) / h
        out["omegaY"][i] = (dudz - dwdx) / h
        out["omegaZ"][i] = (dvdx - dudy) / h
        vxDef = out["vxDef"][i] = UD[iz][iy][ix][0]
        vX = out["vX"][i] = l(ix, iy, iz, 0)
        vyDef = out["vyDef"][i] = UD[iz][iy][ix][1]
        vY = out["vY"][i] = l(ix, iy, iz, 1)
        vzDef = out["vzDef"][i] = UD[iz][iy][ix][2]
        vZ = out["vZ"][i] = l(ix, iy, iz, 2)
        q["forcex"] += fXT
        q["forcey"] += fYT
        q["forcez"] += fZT
        q["forcex_V"] += fXV
        q["forcey_V"] += fYV
        q["forcez_V"] += fZV
        q["forcex_P"] += fXP
        q["forcey_P"] += fYP
        q["forcez_P"] += fZP
        q["torquex"] += (p[1] - CM[1]) * fZT - (p[2] - CM[2]) * fYT
        q["torquey"] += (p[2] - CM[2]) * fXT - (p[0] - CM[0]) * fZT
        q["torquez"] += (p[0] - CM[0]) * fYT - (p[1] - CM[1]) * fXT
        forcePar = fXT * velUnit[0] + fYT * velUnit[1] + fZT * velUnit[2]
        mark("forcePar>0" if forcePar > 0 else ("forcePar<0" if forcePar < 0 else "forcePar=0"))
        q["thrust"] += .5 * (forcePar + abs(forcePar))
        q["drag"] -= .5 * (forcePar - abs(forcePar))
        powOut = fXT * vX + fYT * vY + fZT * vZ
        powDef = fXT * vxDef + fYT * vyDef + fZT * vzDef
        mark("powOut<0" if powOut < 0 else "powOut>=0")
        mark("powDef<0" if powDef < 0 else "powDef>=0")
        q["Pout"] += powOut
        q["PoutBnd"] += powOut if powOut < 0.0 else 0.0       # std::min((Real)0, powOut)
        q["defPower"] += powDef
        q["defPowerBnd"] += powDef if powDef < 0.0 else 0.0
        rVec = [p[0] - CM[0], p[1] - CM[1], p[2] - CM[2]]
        uSolid = [uTrans[0] + omega[1] * rVec[2] - rVec[1] * omega[2],
                  uTrans[1] + omega[2] * rVec[0] - rVec[2] * omega[0],
                  uTrans[2] + omega[0] * rVec[1] - rVec[0] * omega[1]]
        q["pLocom"] += fXT * uSolid[0] + fYT * uSolid[1] + fZT * uSolid[2]
    return np.array([out[name] for name in POINT_NAMES], dtype=np.float64).reshape(19, n), np.array([q[name] for name in QOI_NAMES], dtype=np.float64)


def compute_forces(vel_tiles, chi_tiles, pres, hs, origins, nu, obstacle, qoi_in=None, trace=None):
    """KernelComputeForces for one obstacle over a mesh: vel_tiles [nb][16][16][16][3], chi_tiles [nb][16][16][16](,1), pres [nb][8][8][8]
    for every block of the mesh, hs [nb], origins [nb][3]; `obstacle` holds slots [n], first [n+1], ijk, dchi, udef [n][8][8][8][3], cm,
    vel, omega (only blocks with points are listed, 12280) and qoi [n][19], the block sums before the call, unless qoi_in is given.
    Returns (points [19][npoints], qoi [n][19])."""
    slots, first = obstacle["slots"], obstacle["first"]
    qin = obstacle["qoi"] if qoi_in is None else qoi_in
    npts = int(first[-1])
    points, qoi = np.zeros((19, npts)), np.zeros((len(slots), 19))
    for i, b in enumerate(slots):
        a, e = int(first[i]), int(first[i + 1])
        pts, qoi[i] = visit(vel_tiles[b], chi_tiles[b], pres[b], hs[b], origins[b], obstacle["udef"][i], obstacle["ijk"][a:e], obstacle["dchi"][a:e],
                            obstacle["cm"], obstacle["vel"], obstacle["omega"], nu, qin[i], trace)
        points[:, a:e] = pts
    return points, qoi
