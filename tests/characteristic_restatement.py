"""The grid half of CreateObstacles::operator() (main.cpp:13596-13619) restated in plain Python, line by line.  TEST INFRASTRUCTURE.

The yardstick of cup3d_create_obstacles (k_characteristic, k_udef_momenta, k_remove_udef_momenta and the host half,
cup3d_amd/csrc/obstacles_create.hip), written from the reference's text and not from the kernels: scalar float64 arithmetic (Python floats: IEEE
doubles, no contraction) in the reference's association.

  characteristic   KernelCharacteristicFunction::operate (13298-13403) for one ObstacleBlock: chi, the max into the block of the chi
                   field, mass / CoM_x / CoM_y / CoM_z over all 512 cells, the surface points in push_back order
  grid_com         kernelComputeGridCoM (13406-13425), one thread: block rows in ascending slot order
  udef_momenta     _kernelIntegrateUdefMomenta (13426-13488) for one ObstacleBlock: V, FX FY FZ, TX TY TZ, J0..J5
  accumulate       kernelAccumulateUdefMomenta (13495-13550, justDebug = false), one thread, with invertSym (9092-9105)
  remove           kernelRemoveUdefMomenta (13551-13588) for one ObstacleBlock
  create           all of it for the obstacles of one call, in the reference's loop order: blocks outside, obstacles inside (13301)

tests/test_characteristic_restatement.py pins it by closed forms: a sphere's mass and centre, planes, and the removed momenta."""
import sys

import numpy as np

EPS = float(np.finfo(np.float64).eps)   # 13290
NAMES = ("V", "FX", "FY", "FZ", "TX", "TY", "TZ", "J0", "J1", "J2", "J3", "J4", "J5")


class VolumeError(ValueError):
    """one of the reference's two asserts on the obstacle's volume (13420, 13520) fails"""


def characteristic(sdf, h, origin, field, trace=None):
    """One ObstacleBlock.  sdf: [10][10][10] (sdfLab, index [z+1][y+1][x+1]); field: the block of the chi field as nested lists
    [8][8][8], updated in place (13349).  Returns (CHI nested list, [mass, CoM_x, CoM_y, CoM_z], points) with points the surface in
    push_back order: tuples (ix, iy, iz, dchidx, dchidy, dchidz, delta).  trace: a set that collects the names of the paths taken."""
    SDFLAB = np.asarray(sdf, dtype=np.float64).reshape(10, 10, 10).tolist()
    h = float(h)
    origin = [float(v) for v in origin]
    inv2h, fac1, vol = .5 / h, .5 * h * h, h * h * h   # 13299
    gp = 1
    Nx = Ny = Nz = 8
    CHI = [[[0.0] * 8 for _ in range(8)] for _ in range(8)]
    CoM_x = CoM_y = CoM_z = mass = 0.0
    note = trace.add if trace is not None else (lambda s: None)
    for z in range(Nz):
        for y in range(Ny):
            for x in range(Nx):
                if SDFLAB[z + 1][y + 1][x + 1] > +gp * h or SDFLAB[z + 1][y + 1][x + 1] < -gp * h:
                    CHI[z][y][x] = 1.0 if SDFLAB[z + 1][y + 1][x + 1] > 0 else 0.0
                    note("far_inside" if CHI[z][y][x] else "far_outside")
                else:
                    distPx = SDFLAB[z + 1][y + 1][x + 1 + 1]
                    distMx = SDFLAB[z + 1][y + 1][x + 1 - 1]
                    distPy = SDFLAB[z + 1][y + 1 + 1][x + 1]
                    distMy = SDFLAB[z + 1][y + 1 - 1][x + 1]
                    distPz = SDFLAB[z + 1 + 1][y + 1][x + 1]
                    distMz = SDFLAB[z + 1 - 1][y + 1][x + 1]
                    gradUX = inv2h * (distPx - distMx)
                    gradUY = inv2h * (distPy - distMy)
                    gradUZ = inv2h * (distPz - distMz)
                    gradUSq = gradUX * gradUX + gradUY * gradUY + gradUZ * gradUZ + EPS
                    IplusX = max(0.0, distPx)
                    IminuX = max(0.0, distMx)
                    IplusY = max(0.0, distPy)
                    IminuY = max(0.0, distMy)
                    IplusZ = max(0.0, distPz)
                    IminuZ = max(0.0, distMz)
                    gradIX = inv2h * (IplusX - IminuX)
                    gradIY = inv2h * (IplusY - IminuY)
                    gradIZ = inv2h * (IplusZ - IminuZ)
                    numH = gradIX * gradUX + gradIY * gradUY + gradIZ * gradUZ
                    CHI[z][y][x] = numH / gradUSq
                    note("band")
                    if SDFLAB[z + 1][y + 1][x + 1] == h:
                        note("sdf==+h")
                    if SDFLAB[z + 1][y + 1][x + 1] == -h:
                        note("sdf==-h")
                    if abs(gradUSq - EPS - 1.0) > 1e-3:
                        note("gradUSq!=1")
                p = [origin[0] + h * (x + 0.5), origin[1] + h * (y + 0.5), origin[2] + h * (z + 0.5)]   # Info::pos, 369-373
                field[z][y][x] = max(CHI[z][y][x], field[z][y][x])   # std::max(a, b): a unless a < b, and so is Python's
                CoM_x += CHI[z][y][x] * vol * p[0]
                CoM_y += CHI[z][y][x] * vol * p[1]
                CoM_z += CHI[z][y][x] * vol * p[2]
                mass += CHI[z][y][x] * vol
    points = []
    for z in range(Nz):
        for y in range(Ny):
            for x in range(Nx):
                distPx = SDFLAB[z + 1][y + 1][x + 1 + 1]
                distMx = SDFLAB[z + 1][y + 1][x + 1 - 1]
                distPy = SDFLAB[z + 1][y + 1 + 1][x + 1]
                distMy = SDFLAB[z + 1][y + 1 - 1][x + 1]
                distPz = SDFLAB[z + 1 + 1][y + 1][x + 1]
                distMz = SDFLAB[z + 1 - 1][y + 1][x + 1]
                gradUX = inv2h * (distPx - distMx)
                gradUY = inv2h * (distPy - distMy)
                gradUZ = inv2h * (distPz - distMz)
                gradUSq = gradUX * gradUX + gradUY * gradUY + gradUZ * gradUZ + EPS
                if x == 0:
                    gradHX = 2.0 * (-0.5 * CHI[z][y][x + 2] + 2.0 * CHI[z][y][x + 1] - 1.5 * CHI[z][y][x])
                elif x == Nx - 1:
                    gradHX = 2.0 * (1.5 * CHI[z][y][x] - 2.0 * CHI[z][y][x - 1] + 0.5 * CHI[z][y][x - 2])
                else:
                    gradHX = CHI[z][y][x + 1] - CHI[z][y][x - 1]
                if y == 0:
                    gradHY = 2.0 * (-0.5 * CHI[z][y + 2][x] + 2.0 * CHI[z][y + 1][x] - 1.5 * CHI[z][y][x])
                elif y == Ny - 1:
                    gradHY = 2.0 * (1.5 * CHI[z][y][x] - 2.0 * CHI[z][y - 1][x] + 0.5 * CHI[z][y - 2][x])
                else:
                    gradHY = CHI[z][y + 1][x] - CHI[z][y - 1][x]
                if z == 0:
                    gradHZ = 2.0 * (-0.5 * CHI[z + 2][y][x] + 2.0 * CHI[z + 1][y][x] - 1.5 * CHI[z][y][x])
                elif z == Nz - 1:
                    gradHZ = 2.0 * (1.5 * CHI[z][y][x] - 2.0 * CHI[z - 1][y][x] + 0.5 * CHI[z - 2][y][x])
                else:
                    gradHZ = CHI[z + 1][y][x] - CHI[z - 1][y][x]
                if gradHX * gradHX + gradHY * gradHY + gradHZ * gradHZ < 1e-12:
                    note("gradH<1e-12")
                    continue
                numD = gradHX * gradUX + gradHY * gradUY + gradHZ * gradUZ
                Delta = fac1 * numD / gradUSq
                if Delta > EPS:
                    # ObstacleBlock::write (7422-7431)
                    points.append((x, y, z, -Delta * gradUX, -Delta * gradUY, -Delta * gradUZ, Delta))
                    for a, i in zip("xyz", (x, y, z)):
                        if i == 0 or i == 7:
                            note(f"point_{a}{i}")
                else:
                    note("Delta<=EPS")
    return CHI, [mass, CoM_x, CoM_y, CoM_z], points


def grid_com(rows, slots):
    """com[4] of kernelComputeGridCoM before the all-reduce (13408-13418): rows [mass, CoM_x, CoM_y, CoM_z] in ascending slot order"""
    com = [0.0, 0.0, 0.0, 0.0]
    for i in sorted(range(len(slots)), key=lambda i: int(slots[i])):
        for k in range(4):
            com[k] += rows[i][k]
    return com


def udef_momenta(CHI, udef, h, origin, CM, oldCorrVel):
    """One ObstacleBlock (13446-13486): [V, FX, FY, FZ, TX, TY, TZ, J0, J1, J2, J3, J4, J5]"""
    UDEF = np.asarray(udef, dtype=np.float64).reshape(8, 8, 8, 3).tolist()
    h = float(h)
    origin = [float(v) for v in origin]
    VV = FX = FY = FZ = TX = TY = TZ = J0 = J1 = J2 = J3 = J4 = J5 = 0.0
    for z in range(8):
        for y in range(8):
            for x in range(8):
                if CHI[z][y][x] <= 0:
                    continue
                p = [origin[0] + h * (x + 0.5), origin[1] + h * (y + 0.5), origin[2] + h * (z + 0.5)]
                dv, X = h * h * h, CHI[z][y][x]
                p[0] -= CM[0]
                p[1] -= CM[1]
                p[2] -= CM[2]
                dUs = UDEF[z][y][x][0] - oldCorrVel[0]
                dVs = UDEF[z][y][x][1] - oldCorrVel[1]
                dWs = UDEF[z][y][x][2] - oldCorrVel[2]
                VV += X * dv
                FX += X * UDEF[z][y][x][0] * dv
                FY += X * UDEF[z][y][x][1] * dv
                FZ += X * UDEF[z][y][x][2] * dv
                TX += X * (p[1] * dWs - p[2] * dVs) * dv
                TY += X * (p[2] * dUs - p[0] * dWs) * dv
                TZ += X * (p[0] * dVs - p[1] * dUs) * dv
                J0 += X * (p[1] * p[1] + p[2] * p[2]) * dv
                J3 -= X * p[0] * p[1] * dv
                J1 += X * (p[0] * p[0] + p[2] * p[2]) * dv
                J4 -= X * p[0] * p[2] * dv
                J2 += X * (p[0] * p[0] + p[1] * p[1]) * dv
                J5 -= X * p[1] * p[2] * dv
    return [VV, FX, FY, FZ, TX, TY, TZ, J0, J1, J2, J3, J4, J5]


def invertSym(J):
    """9092-9105"""
    detJ = J[0] * (J[1] * J[2] - J[5] * J[5]) + J[3] * (J[4] * J[5] - J[2] * J[3]) + J[4] * (J[3] * J[5] - J[1] * J[4])
    if abs(detJ) <= sys.float_info.min:
        return [0.0] * 6
    return [(J[1] * J[2] - J[5] * J[5]) / detJ, (J[0] * J[2] - J[4] * J[4]) / detJ, (J[0] * J[1] - J[3] * J[3]) / detJ,
            (J[4] * J[5] - J[2] * J[3]) / detJ, (J[3] * J[5] - J[1] * J[4]) / detJ, (J[3] * J[4] - J[0] * J[5]) / detJ]


def momenta_totals(rows, slots):
    """M[13] of kernelAccumulateUdefMomenta before the all-reduce (13498-13517)"""
    M = [0.0] * 13
    for i in sorted(range(len(slots)), key=lambda i: int(slots[i])):
        for k in range(13):
            M[k] += rows[i][k]
    return M


def accumulate(M):
    """13520-13547 with justDebug = false: (mass, transVel_correction, J, angVel_correction)"""
    if not M[0] > EPS:
        raise VolumeError(f"M[0] = {M[0]}")
    AM = [M[4], M[5], M[6]]
    J = [M[7], M[8], M[9], M[10], M[11], M[12]]
    invJ = invertSym(J)
    transVel = [M[1] / M[0], M[2] / M[0], M[3] / M[0]]
    angVel = [invJ[0] * AM[0] + invJ[3] * AM[1] + invJ[4] * AM[2],
              invJ[3] * AM[0] + invJ[1] * AM[1] + invJ[5] * AM[2],
              invJ[4] * AM[0] + invJ[5] * AM[1] + invJ[2] * AM[2]]
    return M[0], transVel, J, angVel


def remove(udef, h, origin, CM, transVel_correction, angVel_correction):
    """One ObstacleBlock (13570-13585): the corrected udef as an array [8][8][8][3]"""
    UDEF = np.asarray(udef, dtype=np.float64).reshape(8, 8, 8, 3).tolist()
    h = float(h)
    origin = [float(v) for v in origin]
    for z in range(8):
        for y in range(8):
            for x in range(8):
                p = [origin[0] + h * (x + 0.5), origin[1] + h * (y + 0.5), origin[2] + h * (z + 0.5)]
                p[0] -= CM[0]
                p[1] -= CM[1]
                p[2] -= CM[2]
                rotVel_correction = [angVel_correction[1] * p[2] - angVel_correction[2] * p[1],
                                     angVel_correction[2] * p[0] - angVel_correction[0] * p[2],
                                     angVel_correction[0] * p[1] - angVel_correction[1] * p[0]]
                UDEF[z][y][x][0] -= transVel_correction[0] + rotVel_correction[0]
                UDEF[z][y][x][1] -= transVel_correction[1] + rotVel_correction[1]
                UDEF[z][y][x][2] -= transVel_correction[2] + rotVel_correction[2]
    return np.array(UDEF)


class Result:
    """one obstacle of a create() call: chi [n][8][8][8], block_com [n][4], first [n+1], ijk [np][3], dchi [np][3], delta [np],
    com_totals [4], cm [3], block_momenta [n][13], udef_totals [13], mass, transvel_correction [3], J [6], angvel_correction [3],
    udef [n][8][8][8][3] (corrected)"""


def create(geom, nb, obstacles, trace=None):
    """geom [nb][4]: h, origin of every block of the mesh; obstacles: dicts with ids [n], sdf [n][10][10][10], udef [n][8][8][8][3] and
    transvel_correction [3] (oldCorrVel).  Returns (the chi field [nb][8][8][8], [Result per obstacle]); raises VolumeError where the
    reference's asserts fail.  One rank, one thread."""
    geom = np.asarray(geom, dtype=np.float64)
    field = [None] * nb
    chis = [[None] * len(o["ids"]) for o in obstacles]
    coms = [[None] * len(o["ids"]) for o in obstacles]
    pts = [[None] * len(o["ids"]) for o in obstacles]
    where = [{int(b): i for i, b in enumerate(o["ids"])} for o in obstacles]
    for b in range(nb):   # 13596-13600, then K.operate block by block, the obstacles inside (13301)
        field[b] = [[[0.0] * 8 for _ in range(8)] for _ in range(8)]
        for k, o in enumerate(obstacles):
            i = where[k].get(b)
            if i is None:
                continue
            chis[k][i], coms[k][i], pts[k][i] = characteristic(o["sdf"][i], geom[b, 0], geom[b, 1:4], field[b], trace)
    out = []
    for k, o in enumerate(obstacles):
        ids = [int(b) for b in o["ids"]]
        r = Result()
        n = len(ids)
        r.chi = np.array(chis[k], dtype=np.float64).reshape(n, 8, 8, 8)
        r.block_com = np.array(coms[k], dtype=np.float64).reshape(n, 4)
        r.first = np.concatenate([[0], np.cumsum([len(p) for p in pts[k]])]).astype(np.int32)
        flat = [p for block in pts[k] for p in block]
        r.ijk = np.array([p[0:3] for p in flat], dtype=np.int32).reshape(-1, 3)
        r.dchi = np.array([p[3:6] for p in flat], dtype=np.float64).reshape(-1, 3)
        r.delta = np.array([p[6] for p in flat], dtype=np.float64)
        com = grid_com(coms[k], ids)
        if not com[0] > EPS:   # 13420
            raise VolumeError(f"obstacle {k}: com[0] = {com[0]}")
        r.com_totals = np.array(com)
        CM = [com[1] / com[0], com[2] / com[0], com[3] / com[0]]
        r.cm = np.array(CM)
        old = [float(v) for v in o.get("transvel_correction", (0.0, 0.0, 0.0))]
        rows = [udef_momenta(chis[k][i], o["udef"][i], geom[b, 0], geom[b, 1:4], CM, old) for i, b in enumerate(ids)]
        r.block_momenta = np.array(rows, dtype=np.float64).reshape(n, 13)
        M = momenta_totals(rows, ids)
        r.udef_totals = np.array(M)
        mass, tv, J, av = accumulate(M)
        r.mass, r.transvel_correction, r.J, r.angvel_correction = mass, np.array(tv), np.array(J), np.array(av)
        r.udef = np.array([remove(o["udef"][i], geom[b, 0], geom[b, 1:4], CM, tv, av) for i, b in enumerate(ids)]).reshape(n, 8, 8, 8, 3)
        out.append(r)
    return np.array(field, dtype=np.float64).reshape(nb, 8, 8, 8), out
