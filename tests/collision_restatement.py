"""Penalization::preventCollidingObstacles (main.cpp:14009-14323) with ComputeJ and ElasticCollision (13939-14007) restated in plain
Python, line by line.  TEST INFRASTRUCTURE.

The yardstick of cup3d_prevent_colliding_obstacles (k_collision_sums and the host half, cup3d_amd/csrc/obstacles_collisions.hip), written from the
reference's text and not from the kernel: scalar float64 arithmetic (Python floats: IEEE doubles, no contraction, math.sqrt correctly
rounded) in the reference's association.

  collision_info   the loop of 14037-14142 with one thread, for the ObstacleBlocks one rank holds: collisions[i] as 20 numbers in the
                   member order of 14015-14034
  over_ranks       14143-14207: buffermax, the MPI_MAX, the iok / jok test, the MPI_SUM -- ranks combined in rank order
  resolve          14208-14323 with one thread: pairs i < j in order, later pairs see the velocities earlier pairs wrote
  prevent          all of it on one rank

An obstacle is a dict with ids [n], sdf [n][10][10][10], chi [n][8][8][8], udef [n][8][8][8][3]; a body (its rigid state) a dict with cm,
mass, J [6], forced [3], vel, omega, collision_vel, collision_omega, collision_counter.  `trace` is a set that collects the names of the
paths taken.  tests/test_collision_restatement.py pins it by closed forms and conservation laws."""
import math

import numpy as np

MEMBERS = ("iM", "iPosX", "iPosY", "iPosZ", "iMomX", "iMomY", "iMomZ", "ivecX", "ivecY", "ivecZ",
           "jM", "jPosX", "jPosY", "jPosZ", "jMomX", "jMomY", "jMomZ", "jvecX", "jvecY", "jvecZ")


def ComputeJ(Rc, R, N, I):
    """13939-13966"""
    m00 = I[0]
    m01 = I[3]
    m02 = I[4]
    m11 = I[1]
    m12 = I[5]
    m22 = I[2]
    a00 = m22 * m11 - m12 * m12
    a01 = m02 * m12 - m22 * m01
    a02 = m01 * m12 - m02 * m11
    a11 = m22 * m00 - m02 * m02
    a12 = m01 * m02 - m00 * m12
    a22 = m00 * m11 - m01 * m01
    determinant = 1.0 / ((m00 * a00) + (m01 * a01) + (m02 * a02))
    a00 *= determinant
    a01 *= determinant
    a02 *= determinant
    a11 *= determinant
    a12 *= determinant
    a22 *= determinant
    aux_0 = (Rc[1] - R[1]) * N[2] - (Rc[2] - R[2]) * N[1]
    aux_1 = (Rc[2] - R[2]) * N[0] - (Rc[0] - R[0]) * N[2]
    aux_2 = (Rc[0] - R[0]) * N[1] - (Rc[1] - R[1]) * N[0]
    return [a00 * aux_0 + a01 * aux_1 + a02 * aux_2,
            a01 * aux_0 + a11 * aux_1 + a12 * aux_2,
            a02 * aux_0 + a12 * aux_1 + a22 * aux_2]


def ElasticCollision(m1, m2, I1, I2, v1, v2, o1, o2, C1, C2, NX, NY, NZ, CX, CY, CZ, vc1, vc2):
    """13967-14007: (hv1, hv2, ho1, ho2)"""
    e = 1.0
    N = [NX, NY, NZ]
    C = [CX, CY, CZ]
    k1 = [N[0] / m1, N[1] / m1, N[2] / m1]
    k2 = [-N[0] / m2, -N[1] / m2, -N[2] / m2]
    J1 = ComputeJ(C, C1, N, I1)
    J2 = ComputeJ(C, C2, N, I2)
    nom = (e + 1) * ((vc1[0] - vc2[0]) * N[0] + (vc1[1] - vc2[1]) * N[1] + (vc1[2] - vc2[2]) * N[2])
    denom = (-(1.0 / m1 + 1.0 / m2) +
             -((J1[1] * (C[2] - C1[2]) - J1[2] * (C[1] - C1[1])) * N[0] +
               (J1[2] * (C[0] - C1[0]) - J1[0] * (C[2] - C1[2])) * N[1] +
               (J1[0] * (C[1] - C1[1]) - J1[1] * (C[0] - C1[0])) * N[2]) -
             ((J2[1] * (C[2] - C2[2]) - J2[2] * (C[1] - C2[1])) * N[0] +
              (J2[2] * (C[0] - C2[0]) - J2[0] * (C[2] - C2[2])) * N[1] +
              (J2[0] * (C[1] - C2[1]) - J2[1] * (C[0] - C2[0])) * N[2]))
    impulse = nom / (denom + 1e-21)
    hv1 = [v1[0] + k1[0] * impulse, v1[1] + k1[1] * impulse, v1[2] + k1[2] * impulse]
    hv2 = [v2[0] + k2[0] * impulse, v2[1] + k2[1] * impulse, v2[2] + k2[2] * impulse]
    ho1 = [o1[0] + J1[0] * impulse, o1[1] + J1[1] * impulse, o1[2] + J1[2] * impulse]
    ho2 = [o2[0] - J2[0] * impulse, o2[1] - J2[1] * impulse, o2[2] - J2[2] * impulse]
    return hv1, hv2, ho1, ho2


def _lists(o):
    """the arrays of one obstacle as nested lists of Python floats, by block id"""
    ids = [int(b) for b in o["ids"]]
    n = len(ids)
    sdf = np.asarray(o["sdf"], dtype=np.float64).reshape(n, 10, 10, 10).tolist()
    chi = np.asarray(o["chi"], dtype=np.float64).reshape(n, 8, 8, 8).tolist()
    udef = np.asarray(o["udef"], dtype=np.float64).reshape(n, 8, 8, 8, 3).tolist()
    return {b: (sdf[i], chi[i], udef[i]) for i, b in enumerate(ids)}


def collision_info(geom, obstacles, bodies, trace=None):
    """14037-14142 for the blocks listed (one rank's): [N][20].  obstacleBlocks is indexed by block, so the blocks two obstacles share
    are visited in ascending block id whatever order the lists have."""
    geom = np.asarray(geom, dtype=np.float64)
    note = trace.add if trace is not None else (lambda s: None)
    N = len(obstacles)
    blocks = [_lists(o) for o in obstacles]
    collisions = []
    for i in range(N):
        coll = dict.fromkeys(MEMBERS, 0.0)
        iBlocks = blocks[i]
        iU0, iU1, iU2 = (float(v) for v in bodies[i]["vel"])
        iomega0, iomega1, iomega2 = (float(v) for v in bodies[i]["omega"])
        iCx, iCy, iCz = (float(v) for v in bodies[i]["cm"])
        contributing = 0
        before = 0.0   # imagmax at the end of the previous j that had cells
        for j in range(N):
            if i == j:
                continue
            jBlocks = blocks[j]
            jU0, jU1, jU2 = (float(v) for v in bodies[j]["vel"])
            jomega0, jomega1, jomega2 = (float(v) for v in bodies[j]["omega"])
            jCx, jCy, jCz = (float(v) for v in bodies[j]["cm"])
            imagmax = 0.0
            jmagmax = 0.0
            cells = 0
            for k in sorted(set(iBlocks) & set(jBlocks)):
                iSDF, iChi, iUDEF = iBlocks[k]
                jSDF, jChi, jUDEF = jBlocks[k]
                h = float(geom[k, 0])
                origin = [float(v) for v in geom[k, 1:4]]
                for z in range(8):
                    for y in range(8):
                        for x in range(8):
                            if iChi[z][y][x] <= 0.0 or jChi[z][y][x] <= 0.0:
                                continue
                            cells += 1
                            p = [origin[0] + h * (x + 0.5), origin[1] + h * (y + 0.5), origin[2] + h * (z + 0.5)]   # Info::pos, 369-373
                            iMomX = iU0 + iomega1 * (p[2] - iCz) - iomega2 * (p[1] - iCy) + iUDEF[z][y][x][0]
                            iMomY = iU1 + iomega2 * (p[0] - iCx) - iomega0 * (p[2] - iCz) + iUDEF[z][y][x][1]
                            iMomZ = iU2 + iomega0 * (p[1] - iCy) - iomega1 * (p[0] - iCx) + iUDEF[z][y][x][2]
                            jMomX = jU0 + jomega1 * (p[2] - jCz) - jomega2 * (p[1] - jCy) + jUDEF[z][y][x][0]
                            jMomY = jU1 + jomega2 * (p[0] - jCx) - jomega0 * (p[2] - jCz) + jUDEF[z][y][x][1]
                            jMomZ = jU2 + jomega0 * (p[1] - jCy) - jomega1 * (p[0] - jCx) + jUDEF[z][y][x][2]
                            imag = iMomX * iMomX + iMomY * iMomY + iMomZ * iMomZ
                            jmag = jMomX * jMomX + jMomY * jMomY + jMomZ * jMomZ
                            ivecX = iSDF[z + 1][y + 1][x + 2] - iSDF[z + 1][y + 1][x]
                            ivecY = iSDF[z + 1][y + 2][x + 1] - iSDF[z + 1][y][x + 1]
                            ivecZ = iSDF[z + 2][y + 1][x + 1] - iSDF[z][y + 1][x + 1]
                            jvecX = jSDF[z + 1][y + 1][x + 2] - jSDF[z + 1][y + 1][x]
                            jvecY = jSDF[z + 1][y + 2][x + 1] - jSDF[z + 1][y][x + 1]
                            jvecZ = jSDF[z + 2][y + 1][x + 1] - jSDF[z][y + 1][x + 1]
                            normi = 1.0 / (math.sqrt(ivecX * ivecX + ivecY * ivecY + ivecZ * ivecZ) + 1e-21)
                            normj = 1.0 / (math.sqrt(jvecX * jvecX + jvecY * jvecY + jvecZ * jvecZ) + 1e-21)
                            coll["iM"] += 1
                            coll["iPosX"] += p[0]
                            coll["iPosY"] += p[1]
                            coll["iPosZ"] += p[2]
                            coll["ivecX"] += ivecX * normi
                            coll["ivecY"] += ivecY * normi
                            coll["ivecZ"] += ivecZ * normi
                            if imag > imagmax:
                                if imag <= before:
                                    note("imagmax_restarts_per_j")   # a cell the previous j's maximum would have kept out
                                imagmax = imag
                                coll["iMomX"] = iMomX
                                coll["iMomY"] = iMomY
                                coll["iMomZ"] = iMomZ
                            coll["jM"] += 1
                            coll["jPosX"] += p[0]
                            coll["jPosY"] += p[1]
                            coll["jPosZ"] += p[2]
                            coll["jvecX"] += jvecX * normj
                            coll["jvecY"] += jvecY * normj
                            coll["jvecZ"] += jvecZ * normj
                            if jmag > jmagmax:
                                jmagmax = jmag
                                coll["jMomX"] = jMomX
                                coll["jMomY"] = jMomY
                                coll["jMomZ"] = jMomZ
            if cells:
                contributing += 1
                before = imagmax
                if contributing > 1:
                    note("totals_run_on_across_j")
            elif contributing:
                note("iMom_persists_across_an_empty_j")
        collisions.append([coll[m] for m in MEMBERS])
    return collisions


def over_ranks(partials):
    """14143-14207: partials[r] = collisions of rank r ([N][20]).  Returns [N][20] as every rank holds them afterwards; MPI_MAX and
    MPI_SUM combine the ranks in rank order (with two ranks: one max, one addition)."""
    N = len(partials[0])
    own = []
    for coll in partials:
        own.append([[c[4] * c[4] + c[5] * c[5] + c[6] * c[6], c[14] * c[14] + c[15] * c[15] + c[16] * c[16]] for c in coll])
    buffermax = [[own[0][i][0], own[0][i][1]] for i in range(N)]
    for r in range(1, len(partials)):
        for i in range(N):
            for q in range(2):
                buffermax[i][q] = max(buffermax[i][q], own[r][i][q])
    total = [[0.0] * 20 for _ in range(N)]
    for r, coll in enumerate(partials):
        for i in range(N):
            iok = abs(own[r][i][0] - buffermax[i][0]) < 1e-10
            jok = abs(own[r][i][1] - buffermax[i][1]) < 1e-10
            buf = list(coll[i])
            for q in (4, 5, 6):
                buf[q] = buf[q] if iok else 0
            for q in (14, 15, 16):
                buf[q] = buf[q] if jok else 0
            total[i] = buf if r == 0 else [a + b for a, b in zip(total[i], buf)]
    return total


def resolve(collisions, bodies, dt, trace=None):
    """14208-14323 with one thread.  Returns (bodies after, bCollisionID, bCollision set?); `bodies` is not modified."""
    note = trace.add if trace is not None else (lambda s: None)
    out = [dict(b, cm=[float(v) for v in b["cm"]], J=[float(v) for v in b["J"]], vel=[float(v) for v in b["vel"]],
                omega=[float(v) for v in b["omega"]], collision_vel=[float(v) for v in b.get("collision_vel", (0, 0, 0))],
                collision_omega=[float(v) for v in b.get("collision_omega", (0, 0, 0))], collision_counter=float(b.get("collision_counter", 0.0)),
                mass=float(b["mass"]), forced=[int(v) for v in b.get("forced", (0, 0, 0))]) for b in bodies]
    N = len(out)
    ids, hit = [], False
    for i in range(N):
        for j in range(i + 1, N):
            m1 = out[i]["mass"]
            m2 = out[j]["mass"]
            v1 = list(out[i]["vel"])
            o1 = list(out[i]["omega"])
            v2 = list(out[j]["vel"])
            o2 = list(out[j]["omega"])
            I1 = out[i]["J"]
            I2 = out[j]["J"]
            C1 = out[i]["cm"]
            C2 = out[j]["cm"]
            coll = dict(zip(MEMBERS, collisions[i]))
            coll_other = dict(zip(MEMBERS, collisions[j]))
            tolerance = 0.001
            if coll["iM"] < tolerance or coll["jM"] < tolerance:
                note("iM<tolerance")
                continue
            if coll_other["iM"] < tolerance or coll_other["jM"] < tolerance:
                note("other_iM<tolerance")
                continue
            if (abs(coll["iPosX"] / coll["iM"] - coll_other["iPosX"] / coll_other["iM"]) > 0.2 or
                    abs(coll["iPosY"] / coll["iM"] - coll_other["iPosY"] / coll_other["iM"]) > 0.2 or
                    abs(coll["iPosZ"] / coll["iM"] - coll_other["iPosZ"] / coll_other["iM"]) > 0.2):
                note("positions_differ_by_more_than_0.2")
                continue
            hit = True
            ids.append(i)
            ids.append(j)
            norm_i = math.sqrt(coll["ivecX"] * coll["ivecX"] + coll["ivecY"] * coll["ivecY"] + coll["ivecZ"] * coll["ivecZ"])
            norm_j = math.sqrt(coll["jvecX"] * coll["jvecX"] + coll["jvecY"] * coll["jvecY"] + coll["jvecZ"] * coll["jvecZ"])
            mX = coll["ivecX"] / norm_i - coll["jvecX"] / norm_j
            mY = coll["ivecY"] / norm_i - coll["jvecY"] / norm_j
            mZ = coll["ivecZ"] / norm_i - coll["jvecZ"] / norm_j
            inorm = 1.0 / math.sqrt(mX * mX + mY * mY + mZ * mZ)
            NX = mX * inorm
            NY = mY * inorm
            NZ = mZ * inorm
            projVel = (coll["jMomX"] - coll["iMomX"]) * NX + (coll["jMomY"] - coll["iMomY"]) * NY + (coll["jMomZ"] - coll["iMomZ"]) * NZ
            if projVel <= 0:
                note("projVel<=0")
                continue
            inv_iM = 1.0 / coll["iM"]
            inv_jM = 1.0 / coll["jM"]
            iPX = coll["iPosX"] * inv_iM
            iPY = coll["iPosY"] * inv_iM
            iPZ = coll["iPosZ"] * inv_iM
            jPX = coll["jPosX"] * inv_jM
            jPY = coll["jPosY"] * inv_jM
            jPZ = coll["jPosZ"] * inv_jM
            CX = 0.5 * (iPX + jPX)
            CY = 0.5 * (iPY + jPY)
            CZ = 0.5 * (iPZ + jPZ)
            vc1 = [coll["iMomX"], coll["iMomY"], coll["iMomZ"]]
            vc2 = [coll["jMomX"], coll["jMomY"], coll["jMomZ"]]
            iforced = bool(out[i]["forced"][0] or out[i]["forced"][1] or out[i]["forced"][2])
            jforced = bool(out[j]["forced"][0] or out[j]["forced"][1] or out[j]["forced"][2])
            m1_i = 1e10 * m1 if iforced else m1
            m2_j = 1e10 * m2 if jforced else m2
            if iforced or jforced:
                note("forced_mass_1e10")
            hv1, hv2, ho1, ho2 = ElasticCollision(m1_i, m2_j, I1, I2, v1, v2, o1, o2, C1, C2, NX, NY, NZ, CX, CY, CZ, vc1, vc2)
            note("resolved")
            out[i]["vel"], out[j]["vel"], out[i]["omega"], out[j]["omega"] = list(hv1), list(hv2), list(ho1), list(ho2)
            out[i]["collision_vel"], out[i]["collision_omega"] = list(hv1), list(ho1)
            out[j]["collision_vel"], out[j]["collision_omega"] = list(hv2), list(ho2)
            out[i]["collision_counter"] = 0.01 * dt
            out[j]["collision_counter"] = 0.01 * dt
    return out, ids, hit


class Result:
    """sums [N][20], bodies (after), collided (bCollisionID), any (bCollision set)"""


def prevent(geom, obstacles, bodies, dt, trace=None, partials=None):
    """The whole function.  partials: the ranks' collision_info results where the mesh is spread over ranks (default: one rank)."""
    r = Result()
    if partials is None:
        partials = [collision_info(geom, obstacles, bodies, trace)]
    r.partials = partials
    r.sums = over_ranks(partials)
    r.bodies, r.collided, r.any = resolve(r.sums, bodies, dt, trace)
    return r
