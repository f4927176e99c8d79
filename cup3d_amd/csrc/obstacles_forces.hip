// cup3d_compute_forces / cup3d_compute_forces_over_ranks.  KernelComputeForces::visit (main.cpp:12273-12493) for the ObstacleBlocks of
// one obstacle that have surface points: per point the one-sided finite differences of the velocity along the surface normal on the
// block's [-4,5) tensorial tile, the 19 per-point arrays and the 19 block sums.  The tiles are the ones cup3d_sim_labs_device writes
// (Matrix3D layout, [16][16][16][nc]) into a scratch buffer of the sim, a bounded number of blocks at a time.
// One wavefront per block.  The reference adds the points of a block in order i = 0..nPoints-1, and so does the kernel: per chunk of 64
// points every lane evaluates one point and leaves its 19 summands in LDS, then lanes 0..18 each add one quantity over the chunk in point
// order onto a running total they keep in a register.  No tree, no atomic: the sums are the reference's bit for bit.
// Of the nineteen sums the functor zeroes eleven at entry (12283-12293); forcey, forcez, forcey_P, forcez_P, forcey_V, forcez_V, PoutBnd
// and defPowerBnd go on from what the block held, so qoi is in/out.
// cup3d_compute_forces_resident / cup3d_compute_forces_resident_over_ranks: the same on the blocks cup3d_create_obstacles retained
// (k_surface_forces_set: one wavefront per surface row of the SurfacePlan, all obstacles of a chunk of tiles in one launch; the tiles are
// built once per distinct slot), followed by Obstacle::computeForces (13079-13115): rows in blockID order, the ranks, 13108-13114.
// Kept as written: the `sx` in the 2-point branch of dveldy (12364) and the precedence of the mixed derivatives' fallback,
// sx*sy*(a - b) - (c - d) (12394-12395, 12406-12407, 12418-12419).
#include "obstacles.hpp"

namespace cup3d {

struct SurfItems {
  const int32_t *slots;  // [m] block slot of each listed ObstacleBlock (pres is read from the resident field)
  const double *geom;    // [m][4]: h, origin[3]
  const int32_t *first;  // [m+1] first point of each block in ijk / dchi / points
  const int32_t *ijk;    // [npoints][3] surface_data::ix, iy, iz
  const double *dchi;    // [npoints][3] surface_data::dchidx, dchidy, dchidz
  const double *udef;    // [m][8][8][8][3]
  const double *vel;     // [m][16][16][16][3] tiles
  const double *chi;     // [m][16][16][16]
  double *points;        // [19][npoints]
  double *qoi;           // [m][19] in/out
  long npoints;
};

constexpr int kQoI = 19;
// sumQoI order (7289-7307): forcex,y,z, forcex,y,z_P, forcex,y,z_V, torquex,y,z, drag, thrust, Pout, PoutBnd, defPower, defPowerBnd, pLocom;
// the ones visit() does NOT zero at entry
constexpr unsigned kQoICarried = (1u << 1) | (1u << 2) | (1u << 4) | (1u << 5) | (1u << 7) | (1u << 8) | (1u << 15) | (1u << 17);

// one velocity component of the nine difference quotients at (x, y, z) of the tile T ([16][16][16][3], component c already added to
// the pointer), shifted back to the surface cell: row c of the velocity gradient (12345-12437)
__device__ __forceinline__ void surface_gradient_row(const double *__restrict__ T, int x, int y, int z, int sx, int sy, int sz, double ex, double ey,
                                                     double ez, double *__restrict__ ddx, double *__restrict__ ddy, double *__restrict__ ddz) {
  const double c0 = -137. / 60., c1 = 5., c2 = -5., c3 = 10. / 3., c4 = -5. / 4., c5 = 1. / 5.;
  auto l = [&](int i, int j, int k) { return T[(((k + 4) * 16 + (j + 4)) * 16 + (i + 4)) * 3]; };
  auto inrange = [](int i) { return i >= -4 && i < 12; };
  const double fsx = sx, fsy = sy, fsz = sz;
  double dx1, dy1, dz1;
  if (inrange(x + 5 * sx))
    dx1 = fsx * (c0 * l(x, y, z) + c1 * l(x + sx, y, z) + c2 * l(x + 2 * sx, y, z) + c3 * l(x + 3 * sx, y, z) + c4 * l(x + 4 * sx, y, z) + c5 * l(x + 5 * sx, y, z));
  else if (inrange(x + 2 * sx))
    dx1 = fsx * (-1.5 * l(x, y, z) + 2.0 * l(x + sx, y, z) - 0.5 * l(x + 2 * sx, y, z));
  else
    dx1 = fsx * (l(x + sx, y, z) - l(x, y, z));
  if (inrange(y + 5 * sy))
    dy1 = fsy * (c0 * l(x, y, z) + c1 * l(x, y + sy, z) + c2 * l(x, y + 2 * sy, z) + c3 * l(x, y + 3 * sy, z) + c4 * l(x, y + 4 * sy, z) + c5 * l(x, y + 5 * sy, z));
  else if (inrange(y + 2 * sy))
    dy1 = fsy * (-1.5 * l(x, y, z) + 2.0 * l(x, y + sy, z) - 0.5 * l(x, y + 2 * sy, z));
  else
    dy1 = fsx * (l(x, y + sy, z) - l(x, y, z));  // sx: as the reference has it (12364)
  if (inrange(z + 5 * sz))
    dz1 = fsz * (c0 * l(x, y, z) + c1 * l(x, y, z + sz) + c2 * l(x, y, z + 2 * sz) + c3 * l(x, y, z + 3 * sz) + c4 * l(x, y, z + 4 * sz) + c5 * l(x, y, z + 5 * sz));
  else if (inrange(z + 2 * sz))
    dz1 = fsz * (-1.5 * l(x, y, z) + 2.0 * l(x, y, z + sz) - 0.5 * l(x, y, z + 2 * sz));
  else
    dz1 = fsz * (l(x, y, z + sz) - l(x, y, z));
  const double dx2 = l(x - 1, y, z) - 2.0 * l(x, y, z) + l(x + 1, y, z);
  const double dy2 = l(x, y - 1, z) - 2.0 * l(x, y, z) + l(x, y + 1, z);
  const double dz2 = l(x, y, z - 1) - 2.0 * l(x, y, z) + l(x, y, z + 1);
  double dxy, dxz, dyz;
  const double sxy = sx * sy, syz = sy * sz, sxz = sx * sz;
  if (inrange(x + 2 * sx) && inrange(y + 2 * sy))
    dxy = sxy * (-0.5 * (-1.5 * l(x + 2 * sx, y, z) + 2.0 * l(x + 2 * sx, y + sy, z) - 0.5 * l(x + 2 * sx, y + 2 * sy, z)) +
                 2.0 * (-1.5 * l(x + sx, y, z) + 2.0 * l(x + sx, y + sy, z) - 0.5 * l(x + sx, y + 2 * sy, z)) -
                 1.5 * (-1.5 * l(x, y, z) + 2.0 * l(x, y + sy, z) - 0.5 * l(x, y + 2 * sy, z)));
  else
    dxy = sxy * (l(x + sx, y + sy, z) - l(x + sx, y, z)) - (l(x, y + sy, z) - l(x, y, z));
  if (inrange(y + 2 * sy) && inrange(z + 2 * sz))
    dyz = syz * (-0.5 * (-1.5 * l(x, y + 2 * sy, z) + 2.0 * l(x, y + 2 * sy, z + sz) - 0.5 * l(x, y + 2 * sy, z + 2 * sz)) +
                 2.0 * (-1.5 * l(x, y + sy, z) + 2.0 * l(x, y + sy, z + sz) - 0.5 * l(x, y + sy, z + 2 * sz)) -
                 1.5 * (-1.5 * l(x, y, z) + 2.0 * l(x, y, z + sz) - 0.5 * l(x, y, z + 2 * sz)));
  else
    dyz = syz * (l(x, y + sy, z + sz) - l(x, y + sy, z)) - (l(x, y, z + sz) - l(x, y, z));
  if (inrange(x + 2 * sx) && inrange(z + 2 * sz))
    dxz = sxz * (-0.5 * (-1.5 * l(x, y, z + 2 * sz) + 2.0 * l(x + sx, y, z + 2 * sz) - 0.5 * l(x + 2 * sx, y, z + 2 * sz)) +
                 2.0 * (-1.5 * l(x, y, z + sz) + 2.0 * l(x + sx, y, z + sz) - 0.5 * l(x + 2 * sx, y, z + sz)) -
                 1.5 * (-1.5 * l(x, y, z) + 2.0 * l(x + sx, y, z) - 0.5 * l(x + 2 * sx, y, z)));
  else
    dxz = sxz * (l(x + sx, y, z + sz) - l(x, y, z + sz)) - (l(x + sx, y, z) - l(x, y, z));
  *ddx = dx1 + dx2 * ex + dxy * ey + dxz * ez;  // 12420-12437
  *ddy = dy1 + dy2 * ey + dyz * ez + dxy * ex;
  *ddz = dz1 + dz2 * ez + dxz * ex + dyz * ey;
}

// What one wavefront reads and writes of the ObstacleBlock it evaluates
struct SurfBlock {
  const double *geom;    // [4] of the block: h, origin[3]
  const int32_t *ijk;    // [..][3] the list that holds the block's points [p0, p1)
  const double *dchi;    // [..][3]
  int p0, p1;
  const double *udef;    // [8][8][8][3] of the block
  const double *pres;    // [8][8][8] of the block's slot in the resident field
  const double *vel;     // [16][16][16][3] tile
  const double *chi;     // [16][16][16] tile
  double *points;        // [19][np]; may be null where kPointsOptional
  size_t np;
  double *qoi;           // [19] of the block, in/out
};

// KernelComputeForces::visit on one ObstacleBlock by one wavefront.  The body of both k_surface_forces and k_surface_forces_set;
// kPointsOptional: the per-point arrays are stored only if B.points is not null (the same in every lane).
template <bool kPointsOptional>
__device__ __forceinline__ void surface_forces_block(const SurfBlock &B, double nu, double cm0, double cm1, double cm2, double u0, double u1, double u2, double o0,
                                                     double o1, double o2, double (*sm)[64] /* LDS [19][64] */) {
  const int lane = threadIdx.x;
  const double h = B.geom[0];
  const double *__restrict__ VT = B.vel;
  const double *__restrict__ XT = B.chi;
  const int p0 = B.p0, p1 = B.p1;
  double total = 0.0;  // lanes 0..18: the running sum of quantity `lane`
  if (lane < kQoI && ((kQoICarried >> lane) & 1u)) total = B.qoi[lane];
  double velUnit0 = 0., velUnit1 = 0., velUnit2 = 0.;
  const double vel_norm = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
  if (vel_norm > 1e-9) {
    velUnit0 = u0 / vel_norm;
    velUnit1 = u1 / vel_norm;
    velUnit2 = u2 / vel_norm;
  }
  const double _1oH = nu / h;
  for (int base = p0; base < p1; base += 64) {
    const int i = base + lane;
    if (i < p1) {
      const int ix = B.ijk[3 * (size_t)i], iy = B.ijk[3 * (size_t)i + 1], iz = B.ijk[3 * (size_t)i + 2];
      const double px = B.geom[1] + h * (ix + 0.5), py = B.geom[2] + h * (iy + 0.5), pz = B.geom[3] + h * (iz + 0.5);
      const double normX = B.dchi[3 * (size_t)i], normY = B.dchi[3 * (size_t)i + 1], normZ = B.dchi[3 * (size_t)i + 2];
      const double norm = 1.0 / sqrt(normX * normX + normY * normY + normZ * normZ);
      const double dx = normX * norm, dy = normY * norm, dz = normZ * norm;
      int x = ix, y = iy, z = iz;
      for (int kk = 0; kk < 5; kk++) {  // 12323-12341
        // |kk * d| <= 4 for a unit normal; the clamp keeps a normal that is not a number from steering the march out of the tile
        const int dxi = (int)fmin(fmax(round(kk * dx), -16.0), 16.0);
        const int dyi = (int)fmin(fmax(round(kk * dy), -16.0), 16.0);
        const int dzi = (int)fmin(fmax(round(kk * dz), -16.0), 16.0);
        if (ix + dxi + 1 >= 12 || ix + dxi - 1 < -4) continue;
        if (iy + dyi + 1 >= 12 || iy + dyi - 1 < -4) continue;
        if (iz + dzi + 1 >= 12 || iz + dzi - 1 < -4) continue;
        x = ix + dxi;
        y = iy + dyi;
        z = iz + dzi;
        if (XT[((z + 4) * 16 + (y + 4)) * 16 + (x + 4)] < 0.01) break;
      }
      const int sx = normX > 0 ? +1 : -1, sy = normY > 0 ? +1 : -1, sz = normZ > 0 ? +1 : -1;
      const double ex = ix - x, ey = iy - y, ez = iz - z;
      double dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz;
      surface_gradient_row(VT + 0, x, y, z, sx, sy, sz, ex, ey, ez, &dudx, &dudy, &dudz);
      surface_gradient_row(VT + 1, x, y, z, sx, sy, sz, ex, ey, ez, &dvdx, &dvdy, &dvdz);
      surface_gradient_row(VT + 2, x, y, z, sx, sy, sz, ex, ey, ez, &dwdx, &dwdy, &dwdz);
      const int cell = (iz * 8 + iy) * 8 + ix;
      const double P = B.pres[cell];
      const double fXV = _1oH * (dudx * normX + dudy * normY + dudz * normZ);
      const double fYV = _1oH * (dvdx * normX + dvdy * normY + dvdz * normZ);
      const double fZV = _1oH * (dwdx * normX + dwdy * normY + dwdz * normZ);
      const double fXP = -P * normX, fYP = -P * normY, fZP = -P * normZ;
      const double fXT = fXV + fXP, fYT = fYV + fYP, fZT = fZV + fZP;
      const double *__restrict__ U = B.udef + (size_t)cell * 3;
      const double vxDef = U[0], vyDef = U[1], vzDef = U[2];
      const double *__restrict__ VC = VT + (((iz + 4) * 16 + (iy + 4)) * 16 + (ix + 4)) * 3;
      const double vX = VC[0], vY = VC[1], vZ = VC[2];
      if (!kPointsOptional || B.points) {
        double *__restrict__ o = B.points + i;
        const size_t np = B.np;
        o[0 * np] = px;
        o[1 * np] = py;
        o[2 * np] = pz;
        o[3 * np] = P;
        o[4 * np] = -P * dx + _1oH * (dudx * dx + dudy * dy + dudz * dz);
        o[5 * np] = -P * dy + _1oH * (dvdx * dx + dvdy * dy + dvdz * dz);
        o[6 * np] = -P * dz + _1oH * (dwdx * dx + dwdy * dy + dwdz * dz);
        o[7 * np] = _1oH * (dudx * dx + dudy * dy + dudz * dz);
        o[8 * np] = _1oH * (dvdx * dx + dvdy * dy + dvdz * dz);
        o[9 * np] = _1oH * (dwdx * dx + dwdy * dy + dwdz * dz);
        o[10 * np] = (dwdy - dvdz) / h;
        o[11 * np] = (dudz - dwdx) / h;
        o[12 * np] = (dvdx - dudy) / h;
        o[13 * np] = vxDef;
        o[14 * np] = vX;
        o[15 * np] = vyDef;
        o[16 * np] = vY;
        o[17 * np] = vzDef;
        o[18 * np] = vZ;
      }
      // the summands of 12463-12491, in sumQoI order
      sm[0][lane] = fXT;
      sm[1][lane] = fYT;
      sm[2][lane] = fZT;
      sm[3][lane] = fXP;
      sm[4][lane] = fYP;
      sm[5][lane] = fZP;
      sm[6][lane] = fXV;
      sm[7][lane] = fYV;
      sm[8][lane] = fZV;
      const double rx = px - cm0, ry = py - cm1, rz = pz - cm2;
      sm[9][lane] = ry * fZT - rz * fYT;
      sm[10][lane] = rz * fXT - rx * fZT;
      sm[11][lane] = rx * fYT - ry * fXT;
      const double forcePar = fXT * velUnit0 + fYT * velUnit1 + fZT * velUnit2;
      sm[12][lane] = .5 * (forcePar - fabs(forcePar));  // drag: SUBTRACTED below (12478)
      sm[13][lane] = .5 * (forcePar + fabs(forcePar));
      const double powOut = fXT * vX + fYT * vY + fZT * vZ;
      const double powDef = fXT * vxDef + fYT * vyDef + fZT * vzDef;
      sm[14][lane] = powOut;
      sm[15][lane] = powOut < 0.0 ? powOut : 0.0;  // std::min((Real)0, powOut)
      sm[16][lane] = powDef;
      sm[17][lane] = powDef < 0.0 ? powDef : 0.0;
      const double uS0 = u0 + o1 * rz - ry * o2, uS1 = u1 + o2 * rx - rz * o0, uS2 = u2 + o0 * ry - rx * o1;
      sm[18][lane] = fXT * uS0 + fYT * uS1 + fZT * uS2;
    }
    __syncthreads();
    if (lane < kQoI) {
      const int cnt = min(64, p1 - base);
      if (lane == 12)
        for (int j = 0; j < cnt; ++j) total -= sm[12][j];
      else
        for (int j = 0; j < cnt; ++j) total += sm[lane][j];
    }
    __syncthreads();
  }
  if (lane < kQoI) B.qoi[lane] = total;
}

__global__ void __launch_bounds__(64) k_surface_forces(SurfItems it, const double *__restrict__ pres, double nu, double cm0, double cm1, double cm2, double u0,
                                                        double u1, double u2, double o0, double o1, double o2) {
  __shared__ double sm[kQoI][64];
  const int b = blockIdx.x;
  const SurfBlock B{it.geom + 4 * (size_t)b, it.ijk, it.dchi, it.first[b], it.first[b + 1], it.udef + (size_t)b * 1536, pres + (size_t)it.slots[b] * 512,
                    it.vel + (size_t)b * 12288, it.chi + (size_t)b * 4096, it.points, (size_t)it.npoints, it.qoi + (size_t)b * kQoI};
  surface_forces_block<false>(B, nu, cm0, cm1, cm2, u0, u1, u2, o0, o1, o2, sm);
}

// The same for the surface rows of the retained set (SurfacePlan, obstacles.hpp), all obstacles of a chunk of tiles in one launch:
// workgroup j evaluates scheduled row e0 + j.  The row's obstacle, block, tile and point range come from the plan's tables, udef is read
// where cup3d_create_obstacles left it, cm / vel / omega from the plan's body table, the tile is number row_tile - tile0 of the scratch,
// and the nineteen sums are the plan's row, read and written in place.
__global__ void __launch_bounds__(64) k_surface_forces_set(PlanItems pl, SurfacePlanItems sp, int e0, int tile0, const double *__restrict__ vel_tiles,
                                                            const double *__restrict__ chi_tiles, const double *__restrict__ pres, double nu,
                                                            double *__restrict__ points /* [19][P] or null */) {
  __shared__ double sm[kQoI][64];
  const int r = constant(sp.sched_rows)[e0 + blockIdx.x];
  const int k = constant(sp.row_obst)[r], b = constant(sp.row_block)[r], t = constant(sp.row_tile)[r] - tile0;
  const ObstItems it = plan_obstacle(pl, k);
  Constant<double> *body = constant(pl.body) + 9 * (size_t)k;
  const SurfBlock B{it.geom + 4 * (size_t)b, sp.ijk, sp.dchi, constant(sp.row_first)[r], constant(sp.row_first)[r + 1], it.udef + (size_t)b * 1536,
                    pres + (size_t)it.slots[b] * 512, vel_tiles + (size_t)t * 12288, chi_tiles + (size_t)t * 4096, points, (size_t)sp.npoints,
                    sp.qoi + (size_t)r * kQoI};
  surface_forces_block<true>(B, nu, body[0], body[1], body[2], body[3], body[4], body[5], body[6], body[7], body[8], sm);
}

// device buffers of cup3d_compute_forces, kept in the sim and only ever grown: the tile scratch of one chunk of blocks and the staged
// arrays of one obstacle
struct ForcesScratch {
  DevGrow vel, chi, slots, geom, first, ijk, dchi, udef, points, qoi;
};

void forces_destroy(Sim *s) {
  ForcesScratch *F = s->forces;
  if (!F) return;
  delete F;  // the buffers take their bytes off the ledger
  s->forces = nullptr;
}

namespace {
constexpr long kForcesChunk = 512;  // blocks whose tiles the scratch holds at a time: 512 x (98 304 + 32 768) B = 64 MiB
// Over ranks every chunk is a round of collective tile calls that all ranks make, needed or not (cup3d_compute_forces_over_ranks), so
// the bound is eight times as large there -- 512 MiB at most, and only as much as the rank's share of the obstacle asks for
constexpr long kForcesChunkOverRanks = 4096;
long forces_chunk(bool over_ranks = false) {
  const int dbg = debug_option("forces_chunk");  // tests: a small chunk, so that a short slot list spans several
  return dbg > 0 ? dbg : (over_ranks ? kForcesChunkOverRanks : kForcesChunk);
}

// what one rank can get wrong in one obstacle; nothing is allocated, launched or written before every obstacle of a call has passed
int surface_check(const Sim *s, const cup3d_obstacle_surface &o, int k) {
  if (o.nblocks < 0) { set_error("cup3d_compute_forces: obstacle %d has nblocks = %ld", k, o.nblocks); return CUP3D_EINVAL; }
  if (o.nblocks == 0) return CUP3D_OK;
  if (!o.slots || !o.first || !o.ijk || !o.dchi || !o.udef || !o.points || !o.qoi) {
    set_error("cup3d_compute_forces: obstacle %d has blocks but a null array", k);
    return CUP3D_EINVAL;
  }
  for (long i = 0; i < o.nblocks; ++i)
    if (o.slots[i] < 0 || o.slots[i] >= s->nb) { set_error("cup3d_compute_forces: obstacle %d: block slot %d out of range", k, (int)o.slots[i]); return CUP3D_EINVAL; }
  if (o.first[0] != 0) { set_error("cup3d_compute_forces: obstacle %d: first[0] = %d, expected 0", k, (int)o.first[0]); return CUP3D_EINVAL; }
  for (long i = 0; i < o.nblocks; ++i)
    if (o.first[i + 1] < o.first[i]) { set_error("cup3d_compute_forces: obstacle %d: first decreases at block %ld", k, i); return CUP3D_EINVAL; }
  const long np = o.first[o.nblocks];
  for (long i = 0; i < 3 * np; ++i)
    if (o.ijk[i] < 0 || o.ijk[i] >= kBS) { set_error("cup3d_compute_forces: obstacle %d: surface point %ld has index %d outside [0, 8)", k, i / 3, (int)o.ijk[i]); return CUP3D_EINVAL; }
  return CUP3D_OK;
}

// the arrays of one obstacle -> device; *it describes the whole obstacle (surface_launch cuts a chunk of blocks out of it)
int surface_stage(Sim *s, const cup3d_obstacle_surface &o, SurfItems *it) {
  ForcesScratch *F = s->forces;
  const size_t nb = (size_t)o.nblocks, np = (size_t)o.first[o.nblocks];
  std::vector<double> gm;
  int rc;
  if ((rc = block_geometry(s, o.slots, o.nblocks, gm)) || (rc = F->slots.upload(o.slots, nb * sizeof(int32_t), 8, stream(), s)) ||
      (rc = F->geom.upload(gm.data(), gm.size() * sizeof(double), 8, stream(), s)) ||
      (rc = F->first.upload(o.first, (nb + 1) * sizeof(int32_t), 8, stream(), s)) || (rc = F->ijk.upload(o.ijk, np * 3 * sizeof(int32_t), 8, stream(), s)) ||
      (rc = F->dchi.upload(o.dchi, np * 3 * sizeof(double), 8, stream(), s)) || (rc = F->udef.upload(o.udef, nb * 1536 * sizeof(double), 8, stream(), s)) ||
      (rc = F->qoi.upload(o.qoi, nb * kQoI * sizeof(double), 8, stream(), s)) || (rc = F->points.need(std::max<size_t>(np, 1) * kQoI * sizeof(double), s)))
    return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));  // gm is a local
  *it = SurfItems{F->slots.as<const int32_t>(), F->geom.as<const double>(), F->first.as<const int32_t>(), F->ijk.as<const int32_t>(), F->dchi.as<const double>(),
                  F->udef.as<const double>(), F->vel.as<const double>(), F->chi.as<const double>(), F->points.as<double>(), F->qoi.as<double>(), (long)np};
  return CUP3D_OK;
}

int surface_launch(Sim *s, const cup3d_obstacle_surface &o, const SurfItems &whole, long t0, long m, double nu) {
  SurfItems it = whole;  // blocks [t0, t0 + m): their tiles are the scratch's first m
  it.slots += t0;
  it.geom += 4 * t0;
  it.first += t0;
  it.udef += (size_t)t0 * 1536;
  it.qoi += (size_t)t0 * kQoI;
  ProfileScope ps("surface_forces");
  hipLaunchKernelGGL(k_surface_forces, dim3((unsigned)m), dim3(64), 0, stream(), it, (const double *)s->pres, nu, o.cm[0], o.cm[1], o.cm[2], o.vel[0], o.vel[1],
                     o.vel[2], o.omega[0], o.omega[1], o.omega[2]);
  CUP3D_HIP(hipGetLastError());
  return CUP3D_OK;
}

int surface_download(Sim *s, const cup3d_obstacle_surface &o) {
  ForcesScratch *F = s->forces;
  const size_t nb = (size_t)o.nblocks, np = (size_t)o.first[o.nblocks];
  {
    ProfileScope ps("surface_forces_download");
    if (np) CUP3D_HIP(hipMemcpyAsync(o.points, F->points.get(), np * kQoI * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipMemcpyAsync(o.qoi, F->qoi.get(), nb * kQoI * sizeof(double), hipMemcpyDeviceToHost, stream()));
  }
  CUP3D_HIP(hipStreamSynchronize(stream()));
  stats_field_download((np + nb) * kQoI * sizeof(double));
  return CUP3D_OK;
}

int scratch_for(Sim *s, long m) {
  if (!s->forces) s->forces = new ForcesScratch();
  int rc;
  if ((rc = s->forces->vel.need((size_t)m * 12288 * sizeof(double), s)) || (rc = s->forces->chi.need((size_t)m * 4096 * sizeof(double), s))) return rc;
  return CUP3D_OK;
}

// the largest block count of a rank, read off `owner`, in chunks: the rounds of collective tile calls every rank makes
long rounds_over_ranks(const Sim *s, const Grid *gm, const int32_t *owner, long chunk) {
  long most = 0;
  std::vector<long> count(std::max(s->grid->nranks, 1), 0);
  for (int64_t b = 0; b < gm->nblocks(); ++b)
    if (owner[b] >= 0 && owner[b] < (int32_t)count.size()) most = std::max(most, ++count[owner[b]]);
  return (most + chunk - 1) / chunk;
}

// Obstacle::computeForces from 13108 on, with the EPS in scope there (12811)
void derived_powers(cup3d_obstacle_forces &o) {
  const double EPS = DBL_EPSILON;
  const double thrust = o.totals[13], drag = o.totals[12], defPower = o.totals[16], defPowerBnd = o.totals[17];
  const double vel_norm = std::sqrt(o.vel[0] * o.vel[0] + o.vel[1] * o.vel[1] + o.vel[2] * o.vel[2]);
  o.Pthrust = thrust * vel_norm;
  o.Pdrag = drag * vel_norm;
  o.EffPDef = o.Pthrust / (o.Pthrust - std::min(defPower, (double)0) + EPS);
  o.EffPDefBnd = o.Pthrust / (o.Pthrust - defPowerBnd + EPS);
}

// cup3d_compute_forces_resident (mesh == nullptr) and cup3d_compute_forces_resident_over_ranks
int forces_resident(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, double nu, int nobst, cup3d_obstacle_forces *out) {
  const bool over_ranks = mesh != nullptr;
  const char *who = over_ranks ? "cup3d_compute_forces_resident_over_ranks" : "cup3d_compute_forces_resident";
  Sim *s = reinterpret_cast<Sim *>(h);
  const long chunk = forces_chunk(over_ranks);
  const long rounds = over_ranks ? rounds_over_ranks(s, reinterpret_cast<const Grid *>(mesh), owner, chunk) : 0;
  bool want_points = false;
  for (int k = 0; k < nobst; ++k) want_points = want_points || out[k].points;
  RetainedObstacles *R = nullptr;
  ResidentPlan *P = nullptr;
  SurfacePlan *Q = nullptr;
  std::vector<double> table, rows;
  // what this rank can get wrong: nothing of the call is launched before it has passed.  Over ranks a rank that fails here still takes
  // part in the tile calls, asking for nothing, and in the all-reduces, where its flag ends the call on every rank.
  auto prepare = [&]() -> int {
    int rc;
    if ((rc = retained_for(s, who, nobst, &R)) || (rc = surface_plan(s, R, &Q)) || (rc = resident_plan(s, R, &P))) return rc;
    if (Q->rows == 0) return CUP3D_OK;
    if ((rc = scratch_for(s, std::min(chunk, Q->ntiles)))) return rc;
    if (want_points && (rc = s->forces->points.need((size_t)Q->npoints * kQoI * sizeof(double), s))) return rc;
    table.resize(9 * (size_t)nobst);
    for (int k = 0; k < nobst; ++k)
      for (int d = 0; d < 3; ++d) {
        table[9 * (size_t)k + d] = out[k].cm[d];
        table[9 * (size_t)k + 3 + d] = out[k].vel[d];
        table[9 * (size_t)k + 6 + d] = out[k].omega[d];
      }
    CUP3D_HIP(hipMemcpyAsync(P->body.get(), table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
    return CUP3D_OK;
  };
  const int local = prepare();
  if (local && !over_ranks) return local;
  const std::string local_text = local ? cup3d_last_error() : "";
  const long nrows = local ? 0 : Q->rows, ntiles = local ? 0 : Q->ntiles;
  const long nchunks = over_ranks ? rounds : (ntiles + chunk - 1) / chunk;
  int rc;
  for (long c = 0; c < nchunks; ++c) {  // the tiles of `chunk` distinct slots at a time: each slot's tiles are built once, whoever holds it
    const long t0 = c * chunk, m = std::max(0L, std::min(chunk, ntiles - t0));
    const int32_t *slots = m ? Q->tile_slots.data() + t0 : nullptr;
    void *vel = m ? s->forces->vel.get() : nullptr, *chi = m ? s->forces->chi.get() : nullptr;
    if (over_ranks) {
      if ((rc = cup3d_sim_labs_over_ranks_device(h, mesh, owner, CUP3D_FIELD_VEL, m, slots, 4, 1, -1, vel)) ||
          (rc = cup3d_sim_labs_over_ranks_device(h, mesh, owner, CUP3D_FIELD_CHI, m, slots, 4, 1, -1, chi)))
        return rc;
    } else if ((rc = cup3d_sim_labs_device(h, CUP3D_FIELD_VEL, m, slots, 4, 1, -1, vel)) || (rc = cup3d_sim_labs_device(h, CUP3D_FIELD_CHI, m, slots, 4, 1, -1, chi))) {
      return rc;
    }
    if (m == 0) continue;
    const int e0 = Q->sched_first[t0], e1 = Q->sched_first[t0 + m];  // the slot-major schedule: a chunk of tiles is a range of scheduled rows
    ProfileScope ps("surface_forces_set");
    hipLaunchKernelGGL(k_surface_forces_set, dim3((unsigned)(e1 - e0)), dim3(64), 0, stream(), plan_items(P), surface_plan_items(Q), e0, (int)t0,
                       s->forces->vel.as<const double>(), s->forces->chi.as<const double>(), (const double *)s->pres, nu,
                       want_points ? s->forces->points.as<double>() : (double *)nullptr);
    CUP3D_HIP(hipGetLastError());
  }
  if (nrows > 0) {
    rows.resize((size_t)nrows * kQoI);
    {
      ProfileScope ps("surface_forces_download");
      CUP3D_HIP(hipMemcpyAsync(rows.data(), Q->qoi.get(), rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    CUP3D_HIP(hipStreamSynchronize(stream()));
    stats_field_download(rows.size() * sizeof(double));
  }
  // Obstacle::computeForces (13079-13107): the blocks' rows in blockID order, then the ranks
  std::vector<double> totals((size_t)nobst * kQoI, 0.0);
  Dev<void> red;  // the all-reduce operand of this call (sums_over_ranks)
  if (scalars_cross_ranks(s) && (rc = red.alloc((kQoI + 1) * sizeof(double), IfEmpty::eight_bytes))) return rc;
  for (int k = 0; k < nobst; ++k) {
    double *T = &totals[(size_t)k * kQoI];
    if (!local) {
      const long r0 = Q->row_base[k], n = Q->row_base[k + 1] - r0;
      // rows of blocks without points are all zero and missing here: the sum starts at +0 and never becomes -0, so that changes no bit
      add_rows_in_slot_order(Q->row_slot.data() + r0, n, rows.data() + (size_t)r0 * kQoI, kQoI, kQoI, T);
    }
    if ((rc = sums_over_ranks(s, red.as<double>(), T, kQoI, false, local, who, k))) {  // MPI_Allreduce(sum, 19), 13087
      if (local) set_error("%s", local_text.c_str());
      return rc;
    }
  }
  // every obstacle has passed: the caller's structs.  An obstacle's points are columns [p0, p0 + np) of the device's [19][P]: they come
  // down last, straight into the arrays of the obstacles that asked, one strided copy each
  size_t points_down = 0;
  for (int k = 0; k < nobst; ++k) {
    cup3d_obstacle_forces &o = out[k];
    const long r0 = Q->row_base[k], n = Q->row_base[k + 1] - r0;
    const size_t p0 = (size_t)Q->first_h[r0], np = (size_t)Q->first_h[r0 + n] - p0;
    if (o.points && np) {
      ProfileScope ps("surface_forces_download");
      CUP3D_HIP(hipMemcpy2DAsync(o.points, np * sizeof(double), s->forces->points.as<const double>() + p0, (size_t)Q->npoints * sizeof(double), np * sizeof(double), kQoI,
                                 hipMemcpyDeviceToHost, stream()));
      points_down += np * kQoI * sizeof(double);
    }
    if (o.qoi)
      for (size_t i = 0; i < (size_t)n * kQoI; ++i) o.qoi[i] = rows[(size_t)r0 * kQoI + i];
    for (int q = 0; q < kQoI; ++q) o.totals[q] = totals[(size_t)k * kQoI + q];
    derived_powers(o);
  }
  if (points_down) {
    CUP3D_HIP(hipStreamSynchronize(stream()));
    stats_field_download(points_down);
  }
  return CUP3D_OK;
}
}  // namespace

}  // namespace cup3d

using namespace cup3d;

extern "C" int cup3d_compute_forces(cup3d_sim_t *h, double nu, int nobst, cup3d_obstacle_surface *obst) {
  if (!h || nobst < 0 || (nobst > 0 && !obst)) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (s->grid->n_local >= 0 || s->grid->nranks > 1) {
    set_error("cup3d_compute_forces: this sim holds one rank's share of a grid spread over %d ranks; the tiles need cup3d_compute_forces_over_ranks", s->grid->nranks);
    return CUP3D_EINVAL;
  }
  int rc;
  for (int k = 0; k < nobst; ++k)
    if ((rc = surface_check(s, obst[k], k))) return rc;
  const long chunk = forces_chunk();
  for (int k = 0; k < nobst; ++k) {  // obstacles one after the other, as KernelComputeForces::operator() visits them (12270-12271)
    const cup3d_obstacle_surface &o = obst[k];
    if (o.nblocks == 0) continue;
    SurfItems it;
    if ((rc = scratch_for(s, std::min(chunk, o.nblocks))) || (rc = surface_stage(s, o, &it))) return rc;
    for (long t0 = 0; t0 < o.nblocks; t0 += chunk) {
      const long m = std::min(chunk, o.nblocks - t0);
      if ((rc = cup3d_sim_labs_device(h, CUP3D_FIELD_VEL, m, o.slots + t0, 4, 1, -1, s->forces->vel.get())) ||
          (rc = cup3d_sim_labs_device(h, CUP3D_FIELD_CHI, m, o.slots + t0, 4, 1, -1, s->forces->chi.get())) || (rc = surface_launch(s, o, it, t0, m, nu)))
        return rc;
    }
    if ((rc = surface_download(s, o))) return rc;
  }
  return CUP3D_OK;
}

extern "C" int cup3d_compute_forces_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, double nu, int nobst, cup3d_obstacle_surface *obst) {
  if (!h || nobst < 0 || (nobst > 0 && !obst)) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (!mesh || !owner) { set_error("cup3d_compute_forces_over_ranks: null mesh / owner"); return CUP3D_EINVAL; }
  const Grid *gm = reinterpret_cast<const Grid *>(mesh);
  // The tile calls are collectives, so every rank has to make the same number of them per obstacle whatever its own share of the obstacle
  // is.  No rank holds more ObstacleBlocks of one obstacle than it holds blocks, and the largest block count of a rank is something every
  // rank reads off `owner`: that many blocks, chunk by chunk, is the number of rounds -- with no collective of this entry point's own.
  const long chunk = forces_chunk(/*over_ranks=*/true);
  const long rounds = rounds_over_ranks(s, gm, owner, chunk);
  // a rank whose own arguments are bad still takes part, asking for no tile, and reports the error afterwards: the others finish
  int bad = CUP3D_OK;
  for (int k = 0; k < nobst && !bad; ++k) {
    bad = surface_check(s, obst[k], k);
    if (!bad && obst[k].nblocks > s->nb) {
      set_error("cup3d_compute_forces_over_ranks: obstacle %d lists %ld blocks, the rank holds %ld", k, obst[k].nblocks, (long)s->nb);
      bad = CUP3D_EINVAL;
    }
  }
  std::string bad_text = bad ? cup3d_last_error() : "";
  int rc;
  for (int k = 0; k < nobst; ++k) {
    const cup3d_obstacle_surface &o = obst[k];
    const long nblocks = bad ? 0 : o.nblocks;
    SurfItems it;
    if (nblocks && ((rc = scratch_for(s, std::min(chunk, nblocks))) || (rc = surface_stage(s, o, &it)))) return rc;
    for (long r = 0; r < rounds; ++r) {
      const long t0 = r * chunk, m = std::max(0L, std::min(chunk, nblocks - t0));
      if ((rc = cup3d_sim_labs_over_ranks_device(h, mesh, owner, CUP3D_FIELD_VEL, m, m ? o.slots + t0 : nullptr, 4, 1, -1, m ? s->forces->vel.get() : nullptr)) ||
          (rc = cup3d_sim_labs_over_ranks_device(h, mesh, owner, CUP3D_FIELD_CHI, m, m ? o.slots + t0 : nullptr, 4, 1, -1, m ? s->forces->chi.get() : nullptr)))
        return rc;
      if (m && (rc = surface_launch(s, o, it, t0, m, nu))) return rc;
    }
    if (nblocks && (rc = surface_download(s, o))) return rc;
  }
  if (bad) { set_error("%s", bad_text.c_str()); return bad; }
  return CUP3D_OK;
}

extern "C" int cup3d_compute_forces_resident(cup3d_sim_t *h, double nu, int nobst, cup3d_obstacle_forces *obst) {
  if (!h || nobst < 0 || (nobst > 0 && !obst)) return CUP3D_EINVAL;
  if (nobst == 0) return CUP3D_OK;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (s->grid->n_local >= 0 || s->grid->nranks > 1) {
    set_error("cup3d_compute_forces_resident: this sim holds one rank's share of a grid spread over %d ranks; the tiles need cup3d_compute_forces_resident_over_ranks",
              s->grid->nranks);
    return CUP3D_EINVAL;
  }
  return forces_resident(h, nullptr, nullptr, nu, nobst, obst);
}

extern "C" int cup3d_compute_forces_resident_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, double nu, int nobst,
                                                        cup3d_obstacle_forces *obst) {
  if (!h || nobst < 0 || (nobst > 0 && !obst)) return CUP3D_EINVAL;
  if (!mesh || !owner) { set_error("cup3d_compute_forces_resident_over_ranks: null mesh / owner"); return CUP3D_EINVAL; }
  if (nobst == 0) return CUP3D_OK;
  return forces_resident(h, mesh, owner, nu, nobst, obst);
}
