// cup3d_create_obstacles; the retained set, its plan and its surface plan.  The grid half of CreateObstacles::operator() (main.cpp:13596-13619): the chi field cleared,
// KernelCharacteristicFunction::operate (13298-13403), kernelComputeGridCoM (13406-13425), _kernelIntegrateUdefMomenta (13426-13488),
// kernelAccumulateUdefMomenta (13495-13550) and kernelRemoveUdefMomenta (13551-13588) from the signed distance the obstacle's geometry
// left in ObstacleBlock::sdfLab.  The staging is per call, as in cup3d_penalization.
// One wavefront per ObstacleBlock in the two kernels that sum.  k_characteristic keeps sdfLab (8 000 B) and the block's chi (4 096 B) in
// LDS; per z-plane every lane evaluates one cell, leaves its four summands in LDS and lanes 0..3 add them in cell order (ALL cells: the
// reference skips none here).  The second loop then takes each plane again: a ballot of the accepted cells and a running count give
// every surface point the place push_back gives it -- z, y, x order -- in the block's own stretch of a staging array, and k_pack_surface
// moves the stretches to their CSR places once the host has turned the counts into `first`.  k_udef_momenta is k_fluid_momenta's pattern
// with the thirteen terms of 13473-13485 in THEIR association (X * UDEF * dv, X * (..) * dv, X * p0 * p1 * dv), which is not
// k_fluid_momenta's (X * dv * ..).
#include "obstacles.hpp"

namespace cup3d {

constexpr int kUdefMomenta = 13;  // V, FX FY FZ, TX TY TZ, J0..J5 (kernelAccumulateUdefMomenta's M, 13504-13516)
constexpr unsigned kUdefMomentaSubtracted = (1u << 10) | (1u << 11) | (1u << 12);  // J3 J4 J5 are accumulated with -= (13481-13485)

struct ShapeItems {
  const int32_t *slots;  // [n]
  const double *geom;    // [n][4]: h, origin[3]
  const double *sdf;     // [n][10][10][10]
  double *udef;          // [n][512][3]
  double *chi;           // [n][512]
  double *com;           // [n][4]: mass, CoM_x, CoM_y, CoM_z
  double *momenta;       // [n][13]
  int32_t *count;        // [n] nPoints
  int32_t *ijk;          // [n][512][3]  each block's points from the start of its own stretch
  double *dchi;          // [n][512][3]
  double *delta;         // [n][512]
};

// One cell of the surface loop of KernelCharacteristicFunction::operate (13355-13400) from sdfLab [10][10][10] and the block's chi
// [8][8][8], both in LDS: whether (x, y, z) is a surface point, and its Delta and grad U.  The body of both k_characteristic and
// k_retained_surface.
__device__ __forceinline__ bool surface_cell(const double *sdf, const double *chi, int x, int y, int z, double inv2h, double fac1, double *Delta,
                                             double *gUX, double *gUY, double *gUZ) {
  const double EPS = DBL_EPSILON;
  auto S = [&](int k, int j, int i) { return sdf[((k + 1) * 10 + (j + 1)) * 10 + (i + 1)]; };
  auto X = [&](int k, int j, int i) { return chi[(k * 8 + j) * 8 + i]; };
  const double gradUX = inv2h * (S(z, y, x + 1) - S(z, y, x - 1));
  const double gradUY = inv2h * (S(z, y + 1, x) - S(z, y - 1, x));
  const double gradUZ = inv2h * (S(z + 1, y, x) - S(z - 1, y, x));
  const double gradUSq = gradUX * gradUX + gradUY * gradUY + gradUZ * gradUZ + EPS;
  const double gradHX = (x == 0) ? 2.0 * (-0.5 * X(z, y, x + 2) + 2.0 * X(z, y, x + 1) - 1.5 * X(z, y, x))
                                 : ((x == 7) ? 2.0 * (1.5 * X(z, y, x) - 2.0 * X(z, y, x - 1) + 0.5 * X(z, y, x - 2)) : (X(z, y, x + 1) - X(z, y, x - 1)));
  const double gradHY = (y == 0) ? 2.0 * (-0.5 * X(z, y + 2, x) + 2.0 * X(z, y + 1, x) - 1.5 * X(z, y, x))
                                 : ((y == 7) ? 2.0 * (1.5 * X(z, y, x) - 2.0 * X(z, y - 1, x) + 0.5 * X(z, y - 2, x)) : (X(z, y + 1, x) - X(z, y - 1, x)));
  const double gradHZ = (z == 0) ? 2.0 * (-0.5 * X(z + 2, y, x) + 2.0 * X(z + 1, y, x) - 1.5 * X(z, y, x))
                                 : ((z == 7) ? 2.0 * (1.5 * X(z, y, x) - 2.0 * X(z - 1, y, x) + 0.5 * X(z - 2, y, x)) : (X(z + 1, y, x) - X(z - 1, y, x)));
  bool accepted = false;
  *Delta = 0.0;
  if (!(gradHX * gradHX + gradHY * gradHY + gradHZ * gradHZ < 1e-12)) {
    const double numD = gradHX * gradUX + gradHY * gradUY + gradHZ * gradUZ;
    *Delta = fac1 * numD / gradUSq;
    accepted = *Delta > EPS;
  }
  *gUX = gradUX;
  *gUY = gradUY;
  *gUZ = gradUZ;
  return accepted;
}

__global__ void __launch_bounds__(64) k_characteristic(ShapeItems it, double *__restrict__ chi_field) {
  __shared__ double sdf[1000];
  __shared__ double chi[512];
  __shared__ double sm[4][65];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int slot = it.slots[b];
  for (int i = lane; i < 1000; i += 64) sdf[i] = it.sdf[(size_t)b * 1000 + i];
  __syncthreads();
  const double EPS = DBL_EPSILON;
  const double h = it.geom[4 * b], inv2h = .5 / h, fac1 = .5 * h * h, vol = h * h * h;  // 13299
  const int gp = 1;
  const int x = lane & 7, y = lane >> 3;
  auto S = [&](int k, int j, int i) { return sdf[((k + 1) * 10 + (j + 1)) * 10 + (i + 1)]; };
  double total = 0.0;  // lanes 0..3: mass, CoM_x, CoM_y, CoM_z
  for (int z = 0; z < 8; ++z) {
    const double d = S(z, y, x);
    double CHI;
    if (d > +gp * h || d < -gp * h) {
      CHI = d > 0 ? 1 : 0;
    } else {
      const double distPx = S(z, y, x + 1), distMx = S(z, y, x - 1);
      const double distPy = S(z, y + 1, x), distMy = S(z, y - 1, x);
      const double distPz = S(z + 1, y, x), distMz = S(z - 1, y, x);
      const double gradUX = inv2h * (distPx - distMx);
      const double gradUY = inv2h * (distPy - distMy);
      const double gradUZ = inv2h * (distPz - distMz);
      const double gradUSq = gradUX * gradUX + gradUY * gradUY + gradUZ * gradUZ + EPS;
      // std::max((Real)0.0, dist): the first operand unless it is smaller
      const double IplusX = 0.0 < distPx ? distPx : 0.0, IminuX = 0.0 < distMx ? distMx : 0.0;
      const double IplusY = 0.0 < distPy ? distPy : 0.0, IminuY = 0.0 < distMy ? distMy : 0.0;
      const double IplusZ = 0.0 < distPz ? distPz : 0.0, IminuZ = 0.0 < distMz ? distMz : 0.0;
      const double gradIX = inv2h * (IplusX - IminuX);
      const double gradIY = inv2h * (IplusY - IminuY);
      const double gradIZ = inv2h * (IplusZ - IminuZ);
      const double numH = gradIX * gradUX + gradIY * gradUY + gradIZ * gradUZ;
      CHI = numH / gradUSq;
    }
    const int c = z * 64 + lane;
    chi[c] = CHI;
    it.chi[(size_t)b * 512 + c] = CHI;
    const double p0 = it.geom[4 * b + 1] + h * (x + 0.5), p1 = it.geom[4 * b + 2] + h * (y + 0.5), p2 = it.geom[4 * b + 3] + h * (z + 0.5);
    const double r = chi_field[(size_t)slot * 512 + c];
    chi_field[(size_t)slot * 512 + c] = CHI < r ? r : CHI;  // std::max(CHI, b.s), 13349
    sm[0][lane] = CHI * vol;
    sm[1][lane] = CHI * vol * p0;
    sm[2][lane] = CHI * vol * p1;
    sm[3][lane] = CHI * vol * p2;
    __syncthreads();
    if (lane < 4)
      for (int j = 0; j < 64; ++j) total += sm[lane][j];
    __syncthreads();
  }
  if (lane < 4) it.com[(size_t)b * 4 + lane] = total;
  int npoints = 0;  // the same in every lane
  for (int z = 0; z < 8; ++z) {  // 13355-13400
    double Delta, gradUX, gradUY, gradUZ;
    const bool accepted = surface_cell(sdf, chi, x, y, z, inv2h, fac1, &Delta, &gradUX, &gradUY, &gradUZ);
    const unsigned long long mask = __ballot(accepted);
    if (accepted) {  // ObstacleBlock::write (7422-7431)
      const size_t at = (size_t)b * 512 + npoints + __popcll(mask & ((1ull << lane) - 1ull));  // < 512: one place per cell at most
      it.ijk[3 * at] = x;
      it.ijk[3 * at + 1] = y;
      it.ijk[3 * at + 2] = z;
      it.dchi[3 * at] = -Delta * gradUX;
      it.dchi[3 * at + 1] = -Delta * gradUY;
      it.dchi[3 * at + 2] = -Delta * gradUZ;
      it.delta[at] = Delta;
    }
    npoints += __popcll(mask);
  }
  if (lane == 0) it.count[b] = npoints;
}

// block b's points: from its stretch of the staging arrays to [first[b], first[b+1]) of the CSR arrays
__global__ void __launch_bounds__(64) k_pack_surface(ShapeItems it, const int32_t *__restrict__ first, int32_t *__restrict__ ijk, double *__restrict__ dchi,
                                                      double *__restrict__ delta) {
  const int b = blockIdx.x;
  const int p0 = first[b], n = first[b + 1] - p0;
  for (int i = threadIdx.x; i < n; i += 64) {
    const size_t from = (size_t)b * 512 + i, to = (size_t)p0 + i;
    for (int d = 0; d < 3; ++d) {
      ijk[3 * to + d] = it.ijk[3 * from + d];
      dchi[3 * to + d] = it.dchi[3 * from + d];
    }
    delta[to] = it.delta[from];
  }
}

// The surface loop again, for one surface row of the retained set by one wavefront (SurfacePlan, obstacles.hpp): sdfLab and chi are read
// where cup3d_create_obstacles left them, and every point goes straight to its CSR place, which the host knows from the counts that
// call brought down.  The same statements, ballot and running count as in k_characteristic, so the same points in the same order.
__global__ void __launch_bounds__(64) k_retained_surface(PlanItems pl, const double *const *__restrict__ sdf_of, const int32_t *__restrict__ row_obst,
                                                          const int32_t *__restrict__ row_block, const int32_t *__restrict__ row_first,
                                                          int32_t *__restrict__ ijk, double *__restrict__ dchi) {
  __shared__ double sdf[1000];
  __shared__ double chi[512];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int k = constant(row_obst)[r], b = constant(row_block)[r];
  const int p0 = constant(row_first)[r], p1 = constant(row_first)[r + 1];
  const ObstItems it = plan_obstacle(pl, k);
  const double *__restrict__ from = constant(sdf_of)[k] + (size_t)b * 1000;
  for (int i = lane; i < 1000; i += 64) sdf[i] = from[i];
  for (int i = lane; i < 512; i += 64) chi[i] = it.chi[(size_t)b * 512 + i];
  __syncthreads();
  const double h = it.geom[4 * b], inv2h = .5 / h, fac1 = .5 * h * h;  // 13299
  const int x = lane & 7, y = lane >> 3;
  int npoints = 0;  // the same in every lane
  for (int z = 0; z < 8; ++z) {
    double Delta, gradUX, gradUY, gradUZ;
    const bool accepted = surface_cell(sdf, chi, x, y, z, inv2h, fac1, &Delta, &gradUX, &gradUY, &gradUZ);
    const unsigned long long mask = __ballot(accepted);
    const int at = p0 + npoints + __popcll(mask & ((1ull << lane) - 1ull));
    if (accepted && at < p1) {  // at < p1 whenever the count is the one the host was given: the row's stretch bounds the writes regardless
      ijk[3 * (size_t)at] = x;
      ijk[3 * (size_t)at + 1] = y;
      ijk[3 * (size_t)at + 2] = z;
      dchi[3 * (size_t)at] = -Delta * gradUX;
      dchi[3 * (size_t)at + 1] = -Delta * gradUY;
      dchi[3 * (size_t)at + 2] = -Delta * gradUZ;
    }
    npoints += __popcll(mask);
  }
}

__global__ void __launch_bounds__(64) k_udef_momenta(ShapeItems it, double cm0, double cm1, double cm2, double oc0, double oc1, double oc2) {
  __shared__ double sm[kUdefMomenta][65];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double h = it.geom[4 * b], dv = h * h * h;  // 13466
  const int ix = lane & 7, iy = lane >> 3;
  const bool subtracted = (kUdefMomentaSubtracted >> lane) & 1u;
  double total = 0.0;  // lanes 0..12: the running sum of quantity `lane`
  for (int iz = 0; iz < 8; ++iz) {
    const int c = iz * 64 + lane;
    const double X = it.chi[(size_t)b * 512 + c];
    const bool visited = !(X <= 0);  // `if (CHI[z][y][x] <= 0) continue;`
    const unsigned long long mask = __ballot(visited);
    if (visited) {
      double p[3] = {it.geom[4 * b + 1] + h * (ix + 0.5), it.geom[4 * b + 2] + h * (iy + 0.5), it.geom[4 * b + 3] + h * (iz + 0.5)};
      p[0] -= cm0; p[1] -= cm1; p[2] -= cm2;
      const double *U = it.udef + ((size_t)b * 512 + c) * 3;
      const double U0 = U[0], U1 = U[1], U2 = U[2];
      const double dUs = U0 - oc0, dVs = U1 - oc1, dWs = U2 - oc2;
      sm[0][lane] = X * dv;
      sm[1][lane] = X * U0 * dv;
      sm[2][lane] = X * U1 * dv;
      sm[3][lane] = X * U2 * dv;
      sm[4][lane] = X * (p[1] * dWs - p[2] * dVs) * dv;
      sm[5][lane] = X * (p[2] * dUs - p[0] * dWs) * dv;
      sm[6][lane] = X * (p[0] * dVs - p[1] * dUs) * dv;
      sm[7][lane] = X * (p[1] * p[1] + p[2] * p[2]) * dv;
      sm[8][lane] = X * (p[0] * p[0] + p[2] * p[2]) * dv;
      sm[9][lane] = X * (p[0] * p[0] + p[1] * p[1]) * dv;
      sm[10][lane] = X * p[0] * p[1] * dv;
      sm[11][lane] = X * p[0] * p[2] * dv;
      sm[12][lane] = X * p[1] * p[2] * dv;
    }
    __syncthreads();
    if (lane < kUdefMomenta) {
      for (int j = 0; j < 64; ++j)
        if ((mask >> j) & 1ull) {
          const double x = sm[lane][j];
          total = subtracted ? total - x : total + x;
        }
    }
    __syncthreads();
  }
  if (lane < kUdefMomenta) it.momenta[(size_t)b * kUdefMomenta + lane] = total;
}

__global__ void __launch_bounds__(256) k_remove_udef_momenta(ShapeItems it, double cm0, double cm1, double cm2, double t0, double t1, double t2, double a0,
                                                              double a1, double a2) {
  const int b = blockIdx.x, t = threadIdx.x;
  const double h = it.geom[4 * b];
  for (int k = 0; k < 2; ++k) {
    const int c = k * 256 + t, ix = c & 7, iy = (c >> 3) & 7, iz = c >> 6;
    double p[3] = {it.geom[4 * b + 1] + h * (ix + 0.5), it.geom[4 * b + 2] + h * (iy + 0.5), it.geom[4 * b + 3] + h * (iz + 0.5)};
    p[0] -= cm0; p[1] -= cm1; p[2] -= cm2;
    const double rot0 = a1 * p[2] - a2 * p[1], rot1 = a2 * p[0] - a0 * p[2], rot2 = a0 * p[1] - a1 * p[0];  // 13578-13581
    double *U = it.udef + ((size_t)b * 512 + c) * 3;
    U[0] = U[0] - (t0 + rot0);
    U[1] = U[1] - (t1 + rot1);
    U[2] = U[2] - (t2 + rot2);
  }
}

namespace {
// invertSym (9092-9105)
void invert_sym(const double *J, double *inv) {
  const double detJ = J[0] * (J[1] * J[2] - J[5] * J[5]) + J[3] * (J[4] * J[5] - J[2] * J[3]) + J[4] * (J[3] * J[5] - J[1] * J[4]);
  if (std::fabs(detJ) <= DBL_MIN) {
    for (int q = 0; q < 6; ++q) inv[q] = 0.0;
    return;
  }
  inv[0] = (J[1] * J[2] - J[5] * J[5]) / detJ;
  inv[1] = (J[0] * J[2] - J[4] * J[4]) / detJ;
  inv[2] = (J[0] * J[1] - J[3] * J[3]) / detJ;
  inv[3] = (J[4] * J[5] - J[2] * J[3]) / detJ;
  inv[4] = (J[3] * J[5] - J[1] * J[4]) / detJ;
  inv[5] = (J[3] * J[4] - J[0] * J[5]) / detJ;
}

int shape_check(const Sim *s, const cup3d_obstacle_shape &o, int k) {
  if (o.nblocks < 0) { set_error("cup3d_create_obstacles: obstacle %d has nblocks = %ld", k, o.nblocks); return CUP3D_EINVAL; }
  if (o.nblocks == 0) return CUP3D_OK;
  if (!o.slots || !o.sdf || !o.udef || !o.chi || !o.first || !o.ijk || !o.dchi || !o.delta) {
    set_error("cup3d_create_obstacles: obstacle %d has blocks but a null array", k);
    return CUP3D_EINVAL;
  }
  for (long i = 0; i < o.nblocks; ++i)
    if (o.slots[i] < 0 || o.slots[i] >= s->nb) { set_error("cup3d_create_obstacles: obstacle %d: block slot %d out of range", k, (int)o.slots[i]); return CUP3D_EINVAL; }
  return CUP3D_OK;
}

// what one obstacle of a call leaves on the device and on the host until every obstacle of the call has passed
struct ShapeWork {
  Dev<void> slots, geom, sdf, udef, chi, com, momenta, count, st_ijk, st_dchi, st_delta, first, ijk, dchi, delta;
  ShapeItems it;
  std::vector<double> com_rows, momenta_rows;
  std::vector<int32_t> first_h;
  double com_totals[4], M[kUdefMomenta], cm[3], transvel[3], angvel[3];
};

// This rank's n blocks of obstacle k up, KernelCharacteristicFunction on them -- chi into W and the resident field, the surface points
// packed -- and kernelComputeGridCoM's block rows added in slot order onto W.com_totals (13411-13418)
int characteristic_pass(Sim *s, const cup3d_obstacle_shape &o, long n, int k, ShapeWork &W) {
  if (n == 0) return CUP3D_OK;
  const size_t nb = (size_t)n;
  std::vector<double> gm;
  int rc;
  if ((rc = block_geometry(s, o.slots, n, gm)) || (rc = W.slots.upload(o.slots, nb * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
      (rc = W.geom.upload(gm.data(), gm.size() * sizeof(double), stream(), IfEmpty::eight_bytes)) || (rc = W.sdf.upload(o.sdf, nb * 1000 * sizeof(double), stream(), IfEmpty::eight_bytes)) ||
      (rc = W.udef.upload(o.udef, nb * 1536 * sizeof(double), stream(), IfEmpty::eight_bytes)) || (rc = W.chi.alloc(nb * 512 * sizeof(double), IfEmpty::eight_bytes)) ||
      (rc = W.com.alloc(nb * 4 * sizeof(double), IfEmpty::eight_bytes)) || (rc = W.momenta.alloc(nb * kUdefMomenta * sizeof(double), IfEmpty::eight_bytes)) ||
      (rc = W.count.alloc(nb * sizeof(int32_t), IfEmpty::eight_bytes)) || (rc = W.st_ijk.alloc(nb * 1536 * sizeof(int32_t), IfEmpty::eight_bytes)) ||
      (rc = W.st_dchi.alloc(nb * 1536 * sizeof(double), IfEmpty::eight_bytes)) || (rc = W.st_delta.alloc(nb * 512 * sizeof(double), IfEmpty::eight_bytes)))
    return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));  // gm is a local
  W.it = ShapeItems{W.slots.as<const int32_t>(), W.geom.as<const double>(), W.sdf.as<const double>(), W.udef.as<double>(), W.chi.as<double>(), W.com.as<double>(),
                    W.momenta.as<double>(), W.count.as<int32_t>(), W.st_ijk.as<int32_t>(), W.st_dchi.as<double>(), W.st_delta.as<double>()};
  {
    ProfileScope ps("characteristic");
    hipLaunchKernelGGL(k_characteristic, dim3((unsigned)n), dim3(64), 0, stream(), W.it, s->chi);
  }
  CUP3D_HIP(hipGetLastError());
  W.com_rows.resize(nb * 4);
  std::vector<int32_t> count(nb);
  CUP3D_HIP(hipMemcpyAsync(W.com_rows.data(), W.com.get(), nb * 4 * sizeof(double), hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipMemcpyAsync(count.data(), W.count.get(), nb * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipStreamSynchronize(stream()));
  stats_field_download(nb * (4 * sizeof(double) + sizeof(int32_t)));
  for (size_t i = 0; i < nb; ++i) {
    if (count[i] < 0 || count[i] > 512) { set_error("cup3d_create_obstacles: obstacle %d: block %ld reports %d surface points", k, (long)i, (int)count[i]); return CUP3D_ESTATE; }
    W.first_h[i + 1] = W.first_h[i] + count[i];
  }
  const size_t np = (size_t)W.first_h[nb];
  if ((rc = W.first.upload(W.first_h.data(), (nb + 1) * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) || (rc = W.ijk.alloc(np * 3 * sizeof(int32_t), IfEmpty::eight_bytes)) ||
      (rc = W.dchi.alloc(np * 3 * sizeof(double), IfEmpty::eight_bytes)) || (rc = W.delta.alloc(np * sizeof(double), IfEmpty::eight_bytes)))
    return rc;
  {
    ProfileScope ps("pack_surface");
    hipLaunchKernelGGL(k_pack_surface, dim3((unsigned)n), dim3(64), 0, stream(), W.it, W.first.as<const int32_t>(), W.ijk.as<int32_t>(), W.dchi.as<double>(),
                       W.delta.as<double>());
  }
  CUP3D_HIP(hipGetLastError());
  add_rows_in_slot_order(o.slots, n, W.com_rows.data(), 4, 4, W.com_totals);
  return CUP3D_OK;
}

// _kernelIntegrateUdefMomenta about W.cm on this rank's n blocks; kernelAccumulateUdefMomenta's block rows added in slot order onto W.M
// (13501-13517)
int momenta_pass(Sim *s, const cup3d_obstacle_shape &o, long n, ShapeWork &W) {
  if (n == 0) return CUP3D_OK;
  {
    ProfileScope ps("udef_momenta");
    hipLaunchKernelGGL(k_udef_momenta, dim3((unsigned)n), dim3(64), 0, stream(), W.it, W.cm[0], W.cm[1], W.cm[2], W.transvel[0], W.transvel[1], W.transvel[2]);
  }
  CUP3D_HIP(hipGetLastError());
  W.momenta_rows.resize((size_t)n * kUdefMomenta);
  CUP3D_HIP(hipMemcpyAsync(W.momenta_rows.data(), W.momenta.get(), W.momenta_rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipStreamSynchronize(stream()));
  stats_field_download(W.momenta_rows.size() * sizeof(double));
  add_rows_in_slot_order(o.slots, n, W.momenta_rows.data(), kUdefMomenta, kUdefMomenta, W.M);
  return CUP3D_OK;
}

// every obstacle of the call has passed: the caller's arrays of one of them
int shape_copy_out(cup3d_obstacle_shape &o, const ShapeWork &W) {
  const size_t nb = (size_t)o.nblocks, np = (size_t)W.first_h[nb];
  if (nb) {
    CUP3D_HIP(hipMemcpyAsync(o.chi, W.chi.get(), nb * 512 * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipMemcpyAsync(o.udef, W.udef.get(), nb * 1536 * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (np) {
      CUP3D_HIP(hipMemcpyAsync(o.ijk, W.ijk.get(), np * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipMemcpyAsync(o.dchi, W.dchi.get(), np * 3 * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipMemcpyAsync(o.delta, W.delta.get(), np * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    CUP3D_HIP(hipStreamSynchronize(stream()));
    stats_field_download(nb * 2048 * sizeof(double) + np * (3 * sizeof(int32_t) + 4 * sizeof(double)));
    for (size_t i = 0; i <= nb; ++i) o.first[i] = W.first_h[i];
    if (o.block_com)
      for (size_t i = 0; i < nb * 4; ++i) o.block_com[i] = W.com_rows[i];
    if (o.block_momenta)
      for (size_t i = 0; i < nb * kUdefMomenta; ++i) o.block_momenta[i] = W.momenta_rows[i];
  } else if (o.first) {
    o.first[0] = 0;
  }
  for (int q = 0; q < 4; ++q) o.com_totals[q] = W.com_totals[q];
  for (int q = 0; q < kUdefMomenta; ++q) o.udef_totals[q] = W.M[q];
  o.mass = W.M[0];  // 13532
  for (int q = 0; q < 6; ++q) o.J[q] = W.M[7 + q];  // 13536-13541
  for (int d = 0; d < 3; ++d) {
    o.cm[d] = W.cm[d];
    o.transvel_correction[d] = W.transvel[d];
    o.angvel_correction[d] = W.angvel[d];
  }
  return CUP3D_OK;
}

// the call itself; `work` holds every obstacle's device buffers when it returns, whatever it returns
int create_obstacles(Sim *s, int nobst, cup3d_obstacle_shape *shapes, std::vector<ShapeWork> &work) {
  const char *who = "cup3d_create_obstacles";
  const bool cross = scalars_cross_ranks(s);
  // nothing is written, on the device or the host, before every obstacle of the call has passed.  Over ranks a rank whose own arguments
  // are refused still takes part in the first all-reduce, where its flag ends the call on every rank.
  int bad = CUP3D_OK;
  for (int k = 0; k < nobst && !bad; ++k) bad = shape_check(s, shapes[k], k);
  if (bad && !cross) return bad;
  const std::string bad_text = bad ? cup3d_last_error() : "";
  Dev<void> red;  // the all-reduce operand of this call (sums_over_ranks): up to 13 totals and the error flag
  int rc;
  if (cross && (rc = red.alloc((kUdefMomenta + 1) * sizeof(double), IfEmpty::eight_bytes))) return rc;
  if (!bad) {  // CHI.clear() of every block (13596-13600)
    CUP3D_HIP(hipMemsetAsync(s->chi, 0, (size_t)s->nb * 512 * sizeof(double), stream()));
    s->chi_nonzero = true;
  }
  for (int k = 0; k < nobst; ++k) {  // obstacles one after the other: the max into the chi field in the order 13301 visits them
    const cup3d_obstacle_shape &o = shapes[k];
    ShapeWork &W = work[k];
    const long n = bad ? 0 : o.nblocks;
    for (int q = 0; q < 4; ++q) W.com_totals[q] = 0.0;
    for (int q = 0; q < kUdefMomenta; ++q) W.M[q] = 0.0;
    W.first_h.assign((size_t)n + 1, 0);
    rc = sums_over_ranks(s, red.as<double>(), W.com_totals, 4, false, bad ? bad : characteristic_pass(s, o, n, k, W), who, k);  // MPI_Allreduce(com, 4), 13419
    if (rc) {
      if (bad) set_error("%s", bad_text.c_str());
      return rc;
    }
    if (!(W.com_totals[0] > DBL_EPSILON)) {  // assert(com[0] > epsilon), 13420: the same total on every rank
      set_error("cup3d_create_obstacles: obstacle %d has volume %g", k, W.com_totals[0]);
      return CUP3D_EINVAL;
    }
    for (int d = 0; d < 3; ++d) {
      W.cm[d] = W.com_totals[1 + d] / W.com_totals[0];
      W.transvel[d] = o.transvel_correction[d];  // oldCorrVel, 13436
    }
    if ((rc = sums_over_ranks(s, red.as<double>(), W.M, kUdefMomenta, false, momenta_pass(s, o, n, W), who, k))) return rc;  // MPI_Allreduce(M, 13), 13519
    if (!(W.M[0] > DBL_EPSILON)) {  // assert(M[0] > EPS), 13520
      set_error("cup3d_create_obstacles: obstacle %d has volume %g under chi > 0", k, W.M[0]);
      return CUP3D_EINVAL;
    }
    double invJ[6];
    invert_sym(W.M + 7, invJ);
    const double *AM = W.M + 4;
    for (int d = 0; d < 3; ++d) W.transvel[d] = W.M[1 + d] / W.M[0];  // 13533-13535
    W.angvel[0] = invJ[0] * AM[0] + invJ[3] * AM[1] + invJ[4] * AM[2];  // 13542-13547
    W.angvel[1] = invJ[3] * AM[0] + invJ[1] * AM[1] + invJ[5] * AM[2];
    W.angvel[2] = invJ[4] * AM[0] + invJ[5] * AM[1] + invJ[2] * AM[2];
    if (n > 0) {
      ProfileScope ps("remove_udef_momenta");
      hipLaunchKernelGGL(k_remove_udef_momenta, dim3((unsigned)n), dim3(256), 0, stream(), W.it, W.cm[0], W.cm[1], W.cm[2], W.transvel[0], W.transvel[1],
                         W.transvel[2], W.angvel[0], W.angvel[1], W.angvel[2]);
      CUP3D_HIP(hipGetLastError());
    }
  }
  // every obstacle has passed: the caller's arrays
  for (int k = 0; k < nobst; ++k)
    if ((rc = shape_copy_out(shapes[k], work[k]))) return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return CUP3D_OK;
}
}  // namespace

void retained_destroy(Sim *s) {
  if (!s->retained) return;
  s->bytes -= s->retained->bytes;
  delete s->retained;  // Dev<void> frees
  s->retained = nullptr;
}

int retained_for(Sim *s, const char *who, int nobst, RetainedObstacles **out) {
  RetainedObstacles *R = s->retained;
  if (!R) { set_error("%s: no cup3d_create_obstacles has left its blocks on the device", who); return CUP3D_ESTATE; }
  if ((int)R->obst.size() != nobst) {
    set_error("%s: %d obstacles, but cup3d_create_obstacles left %d", who, nobst, (int)R->obst.size());
    return CUP3D_ESTATE;
  }
  *out = R;
  return CUP3D_OK;
}

int resident_plan(Sim *s, RetainedObstacles *R, ResidentPlan **out) {
  if (R->plan) { *out = R->plan; return CUP3D_OK; }
  const size_t N = R->obst.size();
  ResidentPlan *P = new ResidentPlan;
  struct Drop { ResidentPlan *p; ~Drop() { delete p; } } drop{P};  // until it is handed over
  P->row_base.assign(N + 1, 0);
  for (size_t k = 0; k < N; ++k) P->row_base[k + 1] = P->row_base[k] + R->obst[k].nblocks;
  P->rows = P->row_base[N];
  if (P->rows > 0) {
    const size_t nr = (size_t)P->rows;
    std::vector<ObstItems> items(N);
    std::vector<int32_t> row_obst(nr), row_block(nr), row_slot(nr), sched_rows(nr), sched_first;
    for (size_t k = 0; k < N; ++k) {
      const RetainedObstacles::One &o = R->obst[k];
      items[k] = ObstItems{o.slots.as<const int32_t>(), o.geom.as<const double>(), o.chi.as<const double>(), o.udef.as<const double>()};
      for (long i = 0; i < o.nblocks; ++i) {
        const size_t r = (size_t)(P->row_base[k] + i);
        row_obst[r] = (int32_t)k;
        row_block[r] = (int32_t)i;
        row_slot[r] = o.slots_h[i];
      }
    }
    for (size_t r = 0; r < nr; ++r) sched_rows[r] = (int32_t)r;
    // rows ascend with k, so a stable sort by slot leaves every slot's rows in ascending obstacle order
    std::stable_sort(sched_rows.begin(), sched_rows.end(), [&](int32_t a, int32_t b) { return row_slot[a] < row_slot[b]; });
    for (size_t e = 0; e < nr; ++e)
      if (e == 0 || row_slot[sched_rows[e]] != row_slot[sched_rows[e - 1]]) sched_first.push_back((int32_t)e);
    P->nslots = (long)sched_first.size();
    sched_first.push_back((int32_t)nr);
    int rc;
    if ((rc = P->obst.upload(items.data(), N * sizeof(ObstItems), stream(), IfEmpty::eight_bytes)) || (rc = P->row_obst.upload(row_obst.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = P->row_block.upload(row_block.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) || (rc = P->sched_first.upload(sched_first.data(), sched_first.size() * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = P->sched_rows.upload(sched_rows.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) || (rc = P->body.alloc(N * 9 * sizeof(double), IfEmpty::eight_bytes)) ||
        (rc = P->out.alloc(nr * kMomenta * sizeof(double), IfEmpty::eight_bytes)))
      return rc;
    CUP3D_HIP(hipStreamSynchronize(stream()));  // the tables are locals
    P->bytes = P->obst.bytes() + P->row_obst.bytes() + P->row_block.bytes() + P->sched_first.bytes() + P->sched_rows.bytes() + P->body.bytes() + P->out.bytes();
  }
  drop.p = nullptr;
  R->plan = P;
  R->bytes += P->bytes;
  s->bytes += P->bytes;
  *out = P;
  return CUP3D_OK;
}

PlanItems plan_items(const ResidentPlan *P) {
  return PlanItems{P->obst.as<const ObstItems>(), P->row_obst.as<const int32_t>(), P->row_block.as<const int32_t>(), P->sched_first.as<const int32_t>(),
                   P->sched_rows.as<const int32_t>(), P->body.as<const double>()};
}

int surface_plan(Sim *s, RetainedObstacles *R, SurfacePlan **out) {
  if (R->surface) { *out = R->surface; return CUP3D_OK; }
  int rc;
  ResidentPlan *P;
  if ((rc = resident_plan(s, R, &P))) return rc;  // the obstacles' array pointers and rigid state are its tables
  const size_t N = R->obst.size();
  SurfacePlan *Q = new SurfacePlan;
  struct Drop { SurfacePlan *p; ~Drop() { delete p; } } drop{Q};  // until it is handed over
  std::vector<int32_t> row_obst, row_block;
  Q->row_base.assign(N + 1, 0);
  Q->first_h.assign(1, 0);
  long npoints = 0;
  for (size_t k = 0; k < N; ++k) {
    const RetainedObstacles::One &o = R->obst[k];
    if ((long)o.first_h.size() != o.nblocks + 1) { set_error("the retained obstacle %d has no surface list", (int)k); return CUP3D_ESTATE; }
    for (long i = 0; i < o.nblocks; ++i) {
      const long n = (long)o.first_h[i + 1] - o.first_h[i];
      if (n <= 0) continue;
      npoints += n;
      if (n > 512 || npoints > INT32_MAX) { set_error("the retained obstacle %d: block %ld lists %ld surface points, %ld so far", (int)k, i, n, npoints); return CUP3D_ESTATE; }
      row_obst.push_back((int32_t)k);
      row_block.push_back((int32_t)i);
      Q->row_slot.push_back(o.slots_h[i]);
      Q->first_h.push_back((int32_t)npoints);
    }
    Q->row_base[k + 1] = (long)row_obst.size();
  }
  Q->rows = (long)row_obst.size();
  Q->npoints = npoints;
  if (Q->rows > 0) {
    const size_t nr = (size_t)Q->rows, np = (size_t)npoints;
    std::vector<int32_t> sched_rows(nr), row_tile(nr);
    std::vector<const double *> sdf(N);
    for (size_t k = 0; k < N; ++k) sdf[k] = R->obst[k].sdf.as<const double>();
    for (size_t r = 0; r < nr; ++r) sched_rows[r] = (int32_t)r;
    // rows ascend with k, so a stable sort by slot leaves every slot's rows in ascending obstacle order
    std::stable_sort(sched_rows.begin(), sched_rows.end(), [&](int32_t a, int32_t b) { return Q->row_slot[a] < Q->row_slot[b]; });
    for (size_t e = 0; e < nr; ++e) {
      const int32_t slot = Q->row_slot[sched_rows[e]];
      if (e == 0 || slot != Q->tile_slots.back()) {
        Q->tile_slots.push_back(slot);
        Q->sched_first.push_back((int32_t)e);
      }
      row_tile[sched_rows[e]] = (int32_t)Q->tile_slots.size() - 1;
    }
    Q->ntiles = (long)Q->tile_slots.size();
    Q->sched_first.push_back((int32_t)nr);
    // what the kernels index with, against its bound, before any of it is on the device
    for (size_t r = 0; r < nr; ++r) {
      const bool ok = row_obst[r] >= 0 && (size_t)row_obst[r] < N && row_block[r] >= 0 && row_block[r] < R->obst[row_obst[r]].nblocks && row_tile[r] >= 0 &&
                      row_tile[r] < Q->ntiles && Q->first_h[r] >= 0 && Q->first_h[r] < Q->first_h[r + 1] && Q->first_h[r + 1] <= npoints && Q->row_slot[r] >= 0 &&
                      Q->row_slot[r] < s->nb && sched_rows[r] >= 0 && (size_t)sched_rows[r] < nr;
      if (!ok) { set_error("the surface plan's row %ld is out of bounds", (long)r); return CUP3D_ESTATE; }
    }
    if ((rc = Q->sdf.upload(sdf.data(), N * sizeof(const double *), stream(), IfEmpty::eight_bytes)) ||
        (rc = Q->row_obst.upload(row_obst.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = Q->row_block.upload(row_block.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = Q->row_tile.upload(row_tile.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = Q->sched_rows.upload(sched_rows.data(), nr * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = Q->row_first.upload(Q->first_h.data(), (nr + 1) * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = Q->ijk.alloc(np * 3 * sizeof(int32_t), IfEmpty::eight_bytes)) || (rc = Q->dchi.alloc(np * 3 * sizeof(double), IfEmpty::eight_bytes)) ||
        (rc = Q->qoi.alloc_zeroed(nr * 19 * sizeof(double), stream())))
      return rc;
    {
      ProfileScope ps("retained_surface");
      hipLaunchKernelGGL(k_retained_surface, dim3((unsigned)nr), dim3(64), 0, stream(), plan_items(P), Q->sdf.as<const double *const>(), Q->row_obst.as<const int32_t>(),
                         Q->row_block.as<const int32_t>(), Q->row_first.as<const int32_t>(), Q->ijk.as<int32_t>(), Q->dchi.as<double>());
    }
    CUP3D_HIP(hipGetLastError());
    CUP3D_HIP(hipStreamSynchronize(stream()));  // the tables are locals
    Q->bytes = Q->sdf.bytes() + Q->row_obst.bytes() + Q->row_block.bytes() + Q->row_tile.bytes() + Q->sched_rows.bytes() + Q->row_first.bytes() + Q->ijk.bytes() +
               Q->dchi.bytes() + Q->qoi.bytes();
  }
  drop.p = nullptr;
  R->surface = Q;
  R->bytes += Q->bytes;
  s->bytes += Q->bytes;
  *out = Q;
  return CUP3D_OK;
}

SurfacePlanItems surface_plan_items(const SurfacePlan *Q) {
  return SurfacePlanItems{Q->row_obst.as<const int32_t>(), Q->row_block.as<const int32_t>(), Q->row_tile.as<const int32_t>(), Q->row_first.as<const int32_t>(),
                          Q->sched_rows.as<const int32_t>(), Q->ijk.as<const int32_t>(), Q->dchi.as<const double>(), Q->qoi.as<double>(), Q->npoints};
}

}  // namespace cup3d

using namespace cup3d;

extern "C" int cup3d_create_obstacles(cup3d_sim_t *h, int nobst, cup3d_obstacle_shape *shapes) {
  if (!h || nobst < 0 || (nobst > 0 && !shapes)) {
    if (h) retained_destroy(reinterpret_cast<Sim *>(h));  // a refused call drops what an earlier one left
    return CUP3D_EINVAL;
  }
  if (nobst == 0) return CUP3D_OK;  // 13590: nothing is cleared either
  Sim *s = reinterpret_cast<Sim *>(h);
  retained_destroy(s);
  std::vector<ShapeWork> work((size_t)nobst);
  const int rc = create_obstacles(s, nobst, shapes, work);
  if (rc) return rc;  // the resident chi is unspecified: nothing is kept, `work` frees its buffers
  // slots, geom, sdfLab, chi and the corrected udef of every obstacle stay for cup3d_prevent_colliding_obstacles
  RetainedObstacles *R = new RetainedObstacles;
  R->obst.resize((size_t)nobst);
  for (int k = 0; k < nobst; ++k) {
    ShapeWork &W = work[k];
    RetainedObstacles::One &o = R->obst[k];
    o.nblocks = shapes[k].nblocks;
    o.slots_h.assign(shapes[k].slots, shapes[k].slots + o.nblocks);
    o.first_h = std::move(W.first_h);  // the points per block, for the surface plan of cup3d_compute_forces_resident: no device byte
    o.slots = std::move(W.slots);
    o.geom = std::move(W.geom);
    o.sdf = std::move(W.sdf);
    o.chi = std::move(W.chi);
    o.udef = std::move(W.udef);
    R->bytes += o.slots.bytes() + o.geom.bytes() + o.sdf.bytes() + o.chi.bytes() + o.udef.bytes();
  }
  s->retained = R;
  s->bytes += R->bytes;
  return CUP3D_OK;
}
