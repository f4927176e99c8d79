"""UpdateObstacles::operator() (main.cpp:13812-13837) restated in plain Python, line by line.  TEST INFRASTRUCTURE.

The yardstick of cup3d_update_obstacles (k_fluid_momenta and the host half, cup3d_amd/csrc/obstacles_update.hip), written from the reference's
text and not from the kernel: scalar float64 arithmetic (Python floats: IEEE doubles, no contraction) in the reference's association.

  block_sums   KernelIntegrateFluidMomenta<0/1>::visit (13637-13734): the 29 sums of one ObstacleBlock, cells in iz, iy, ix order,
               those with chi <= 0 skipped, in the order kernelFinalizeObstacleVel packs M (13748-13777)
  totals       kernelFinalizeObstacleVel's loop with one thread (13741-13781): block rows added in ascending slot order
  penal        the two branches of 13796-13808
  system       the 6 x 6 matrix and right-hand side of Obstacle::computeVelocities with the bForcedInSimFrame / bBlockRotation edits
               (12922-13014)
  lu_solve     a dense LU with partial pivoting (what 13015-13021 ask of GSL; same mathematics as oracle/refbuild/gsl)
  update       all of it for one obstacle -> the new transVel / angVel by 13039-13068 (no collision override)

tests/test_fluid_momenta_restatement.py pins it: against the compiled reference's `op midstep`, and by its own properties."""
import numpy as np

NAMES = ("V", "FX", "FY", "FZ", "TX", "TY", "TZ", "J0", "J1", "J2", "J3", "J4", "J5",
         "GfX", "GpX", "GpY", "GpZ", "Gj0", "Gj1", "Gj2", "Gj3", "Gj4", "Gj5", "GuX", "GuY", "GuZ", "GaX", "GaY", "GaZ")
NQOI, NEXPLICIT = 29, 13


def block_sums(vel_block, chi, udef, h, origin, cm, lambda_, dt, implicit):
    """One ObstacleBlock: vel_block [8][8][8][3] (the block of sim.vel), chi [8][8][8], udef [8][8][8][3] (z, y, x order).  Returns
    the 29 sums as a list; entries 13..28 are None without implicit penalisation (the reference does not touch them)."""
    B = np.asarray(vel_block, dtype=np.float64).reshape(8, 8, 8, 3).tolist()
    CHI = np.asarray(chi, dtype=np.float64).reshape(8, 8, 8).tolist()
    UDEF = np.asarray(udef, dtype=np.float64).reshape(8, 8, 8, 3).tolist()
    h = float(h)
    origin = [float(v) for v in origin]
    CM = [float(v) for v in cm]
    VV = FX = FY = FZ = TX = TY = TZ = 0.0
    J0 = J1 = J2 = J3 = J4 = J5 = 0.0
    GfX = GpX = GpY = GpZ = Gj0 = Gj1 = Gj2 = Gj3 = Gj4 = Gj5 = GuX = GuY = GuZ = GaX = GaY = GaZ = 0.0
    lambdt = float(lambda_) * float(dt)   # 13664
    for iz in range(8):
        for iy in range(8):
            for ix in range(8):
                if CHI[iz][iy][ix] <= 0:
                    continue
                p = [origin[0] + h * (ix + 0.5), origin[1] + h * (iy + 0.5), origin[2] + h * (iz + 0.5)]   # Info::pos, 369-373
                dv, X = h * h * h, CHI[iz][iy][ix]   # dvol, 13629
                p[0] -= CM[0]
                p[1] -= CM[1]
                p[2] -= CM[2]
                u = B[iz][iy][ix]
                VV += X * dv
                J0 += X * dv * (p[1] * p[1] + p[2] * p[2])
                J1 += X * dv * (p[0] * p[0] + p[2] * p[2])
                J2 += X * dv * (p[0] * p[0] + p[1] * p[1])
                J3 -= X * dv * p[0] * p[1]
                J4 -= X * dv * p[0] * p[2]
                J5 -= X * dv * p[1] * p[2]
                FX += X * dv * u[0]
                FY += X * dv * u[1]
                FZ += X * dv * u[2]
                TX += X * dv * (p[1] * u[2] - p[2] * u[1])
                TY += X * dv * (p[2] * u[0] - p[0] * u[2])
                TZ += X * dv * (p[0] * u[1] - p[1] * u[0])
                if implicit:
                    X1 = 1.0 if CHI[iz][iy][ix] > 0.5 else 0.0
                    penalFac = dv * lambdt * X1 / (1 + X1 * lambdt)
                    GfX += penalFac
                    GpX += penalFac * p[0]
                    GpY += penalFac * p[1]
                    GpZ += penalFac * p[2]
                    Gj0 += penalFac * (p[1] * p[1] + p[2] * p[2])
                    Gj1 += penalFac * (p[0] * p[0] + p[2] * p[2])
                    Gj2 += penalFac * (p[0] * p[0] + p[1] * p[1])
                    Gj3 -= penalFac * p[0] * p[1]
                    Gj4 -= penalFac * p[0] * p[2]
                    Gj5 -= penalFac * p[1] * p[2]
                    DiffU = [u[0] - UDEF[iz][iy][ix][0], u[1] - UDEF[iz][iy][ix][1], u[2] - UDEF[iz][iy][ix][2]]
                    GuX += penalFac * DiffU[0]
                    GuY += penalFac * DiffU[1]
                    GuZ += penalFac * DiffU[2]
                    GaX += penalFac * (p[1] * DiffU[2] - p[2] * DiffU[1])
                    GaY += penalFac * (p[2] * DiffU[0] - p[0] * DiffU[2])
                    GaZ += penalFac * (p[0] * DiffU[1] - p[1] * DiffU[0])
    out = [VV, FX, FY, FZ, TX, TY, TZ, J0, J1, J2, J3, J4, J5]
    if implicit:
        return out + [GfX, GpX, GpY, GpZ, Gj0, Gj1, Gj2, Gj3, Gj4, Gj5, GuX, GuY, GuZ, GaX, GaY, GaZ]
    return out + [None] * (NQOI - NEXPLICIT)


def totals(rows, slots, implicit):
    """M of kernelFinalizeObstacleVel before the all-reduce: the blocks' rows added in ascending slot order, one thread"""
    M = [0.0] * NQOI
    n = NQOI if implicit else NEXPLICIT
    for i in sorted(range(len(slots)), key=lambda i: int(slots[i])):
        for k in range(n):
            M[k] += rows[i][k]
    return M


def penal(M, implicit):
    """(penalM, penalCM, penalJ, penalLmom, penalAmom), 13796-13808"""
    if implicit:
        return M[13], [M[14], M[15], M[16]], [M[17], M[18], M[19], M[20], M[21], M[22]], [M[23], M[24], M[25]], [M[26], M[27], M[28]]
    return M[0], [0.0, 0.0, 0.0], [M[7], M[8], M[9], M[10], M[11], M[12]], [M[1], M[2], M[3]], [M[4], M[5], M[6]]


def system(penalM, penalCM, penalJ, penalLmom, penalAmom, forced=(0, 0, 0), block_rotation=(0, 0, 0), vel_imposed=(0.0, 0.0, 0.0)):
    """A (36 values, row-major) and b of Obstacle::computeVelocities, 12922-13014"""
    A = [0.0] * 36
    A[0 * 6 + 0] = penalM
    A[0 * 6 + 4] = +penalCM[2]
    A[0 * 6 + 5] = -penalCM[1]
    A[1 * 6 + 1] = penalM
    A[1 * 6 + 3] = -penalCM[2]
    A[1 * 6 + 5] = +penalCM[0]
    A[2 * 6 + 2] = penalM
    A[2 * 6 + 3] = +penalCM[1]
    A[2 * 6 + 4] = -penalCM[0]
    A[3 * 6 + 1] = -penalCM[2]
    A[3 * 6 + 2] = +penalCM[1]
    A[3 * 6 + 3] = penalJ[0]
    A[3 * 6 + 4] = penalJ[3]
    A[3 * 6 + 5] = penalJ[4]
    A[4 * 6 + 0] = +penalCM[2]
    A[4 * 6 + 2] = -penalCM[0]
    A[4 * 6 + 3] = penalJ[3]
    A[4 * 6 + 4] = penalJ[1]
    A[4 * 6 + 5] = penalJ[5]
    A[5 * 6 + 0] = -penalCM[1]
    A[5 * 6 + 1] = +penalCM[0]
    A[5 * 6 + 3] = penalJ[4]
    A[5 * 6 + 4] = penalJ[5]
    A[5 * 6 + 5] = penalJ[2]
    b = [penalLmom[0], penalLmom[1], penalLmom[2], penalAmom[0], penalAmom[1], penalAmom[2]]
    for d in range(3):
        if forced[d]:   # 12967-12990
            for k in range(6):
                if k != d:
                    A[d * 6 + k] = 0.0
            b[d] = penalM * float(vel_imposed[d])
    for d in range(3):
        if block_rotation[d]:   # 12991-13014
            for k in range(6):
                if k != 3 + d:
                    A[(3 + d) * 6 + k] = 0.0
            b[3 + d] = 0.0
    return A, b


def lu_solve(A, b):
    """x with A x = b: LU with partial pivoting (rows swapped so that the largest |entry| of the column, the first of equals, is the
    pivot), forward and back substitution"""
    n = len(b)
    a = [[float(A[i * n + k]) for k in range(n)] for i in range(n)]
    y = [float(v) for v in b]
    for j in range(n - 1):
        piv = j
        for i in range(j + 1, n):
            if abs(a[i][j]) > abs(a[piv][j]):
                piv = i
        if piv != j:
            a[j], a[piv] = a[piv], a[j]
            y[j], y[piv] = y[piv], y[j]
        if a[j][j] == 0.0:
            continue
        for i in range(j + 1, n):
            l = a[i][j] / a[j][j]
            a[i][j] = l
            for k in range(j + 1, n):
                a[i][k] -= l * a[j][k]
            y[i] -= l * y[j]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        x[i] = y[i]
        for k in range(i + 1, n):
            x[i] -= a[i][k] * x[k]
        x[i] /= a[i][i]
    return x


class Result:
    """rows [n][29] (NaN where the reference computes nothing), M [29], A [6][6], b [6], vel_computed, omega_computed, vel, omega"""


def update(vel, geom, slots, chi, udef, cm, lambda_, dt, implicit, forced=(0, 0, 0), block_rotation=(0, 0, 0), vel_imposed=(0.0, 0.0, 0.0)):
    """One obstacle on one rank.  vel [nb][8][8][8][3]: the velocity field; geom [nb][4]: h and origin of every block (the grid tables);
    slots [n], chi [n][8][8][8], udef [n][8][8][8][3]: the ObstacleBlocks."""
    r = Result()
    rows = [block_sums(vel[int(s)], chi[i], udef[i], geom[int(s)][0], geom[int(s)][1:4], cm, lambda_, dt, implicit) for i, s in enumerate(slots)]
    r.M = totals(rows, slots, implicit)
    r.rows = np.array([[np.nan if v is None else v for v in row] for row in rows], dtype=np.float64).reshape(len(slots), NQOI)
    finish(r, implicit, forced, block_rotation, vel_imposed)
    return r


def finish(r, implicit, forced=(0, 0, 0), block_rotation=(0, 0, 0), vel_imposed=(0.0, 0.0, 0.0)):
    """from r.M (after the sum over ranks) to the velocities"""
    A, b = system(*penal(r.M, implicit), forced, block_rotation, vel_imposed)
    r.A, r.b = np.array(A).reshape(6, 6), np.array(b)
    x = lu_solve(A, b)
    r.vel_computed, r.omega_computed = np.array(x[:3]), np.array(x[3:])
    r.vel = np.array([float(vel_imposed[d]) if forced[d] else x[d] for d in range(3)])          # 13039-13053
    r.omega = np.array([0.0 if block_rotation[d] else x[3 + d] for d in range(3)])               # 13054-13068
    r.M = np.array(r.M)
    return r
