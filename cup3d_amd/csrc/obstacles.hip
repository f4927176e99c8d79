// Obstacle operators that sit between / inside the two hot-path operators: KernelPenalization
// (main.cpp:13841-13912) + kernelFinalizePenalizationForce (13913-13938), kernelUpdateTmpV (14948-14979), UpdateObstacles (13812-13837),
// ComputeForces (12273-12503) and the grid half of CreateObstacles (13596-13619).
// The obstacles themselves (geometry -- the signed distance and the deformation velocity -- and rigid-body integration) stay on the host;
// cup3d_create_obstacles turns the signed distance into chi, surface points and momentum-free udef, and the other kernels take the
// ObstacleBlocks of one obstacle at a time -- chi[8][8][8] and udef[8][8][8][3] in the reference's own (AoS) layout -- so the
// velocity does not have to leave HBM between AdvectionDiffusion and PressureProjection when obstacles are present.  The *_resident
// entry points run UpdateObstacles, Penalization and kernelUpdateTmpV on the blocks cup3d_create_obstacles keeps, all obstacles at once.
// Velocities and tmpV are bit-exact with the reference; the penalisation force / torque sums are reductions (block totals summed in block
// order on the host, cells within a block in tree order on the device); the momenta of UpdateObstacles and the surface sums of
// ComputeForces are added in the reference's own order and are bit-exact per block.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "sim.hpp"
#include "tile.hpp"

namespace cup3d {

struct ObstItems {
  const int32_t *slots;  // [n] block slot of each ObstacleBlock
  const double *geom;    // [n][4]: h, origin[3] of that block (Info::h, Info::origin)
  const double *chi;     // [n][512]
  const double *udef;    // [n][512][3]
};

// KernelPenalization on ObstacleBlock i of `it` by one 256-thread workgroup; the block's six sums go to forces[0..5].  The body of both
// k_penalize and k_penalize_set: a thread owns cells t and 256 + t of the slot.
__device__ __forceinline__ void penalize_block(const ObstItems &it, const int i, double *__restrict__ vel, const double *__restrict__ chi_field, double dt,
                                               double lambdaFac, int implicit, double cm0, double cm1, double cm2, double v0, double v1, double v2,
                                               double o0, double o1, double o2, double *__restrict__ forces /* [6] */, double *red /* LDS [4] */) {
  const int t = threadIdx.x;
  const int slot = it.slots[i];
  const double h = it.geom[4 * i], dv = pow(h, 3.0);
  double F[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 2; ++k) {
    const int c = k * 256 + t, ix = c & 7, iy = (c >> 3) & 7, iz = c >> 6;
    const double CHI = it.chi[(size_t)i * 512 + c];
    if (chi_field[(size_t)slot * 512 + c] > CHI) continue;
    if (CHI <= 0) continue;
    double p[3] = {it.geom[4 * i + 1] + h * (ix + 0.5), it.geom[4 * i + 2] + h * (iy + 0.5), it.geom[4 * i + 3] + h * (iz + 0.5)};
    p[0] -= cm0; p[1] -= cm1; p[2] -= cm2;
    const double *U = it.udef + ((size_t)i * 512 + c) * 3;
    const double UT0 = v0 + o1 * p[2] - o2 * p[1] + U[0];
    const double UT1 = v1 + o2 * p[0] - o0 * p[2] + U[1];
    const double UT2 = v2 + o0 * p[1] - o1 * p[0] + U[2];
    const double X = implicit ? (CHI > 0.5 ? 1.0 : 0.0) : CHI;
    const double penalFac = implicit ? X * lambdaFac / (1 + X * lambdaFac * dt) : X * lambdaFac;
    double *b = vel + (size_t)slot * 1536 + c;
    const double FPX = penalFac * (UT0 - b[0]), FPY = penalFac * (UT1 - b[512]), FPZ = penalFac * (UT2 - b[1024]);
    b[0] = b[0] + dt * FPX;
    b[512] = b[512] + dt * FPY;
    b[1024] = b[1024] + dt * FPZ;
    F[0] += dv * FPX; F[1] += dv * FPY; F[2] += dv * FPZ;
    F[3] += dv * (p[1] * FPZ - p[2] * FPY);
    F[4] += dv * (p[2] * FPX - p[0] * FPZ);
    F[5] += dv * (p[0] * FPY - p[1] * FPX);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double s = group_sum<4>(F[q], red);
    if (t == 0) forces[q] = s;
  }
}

__global__ void __launch_bounds__(256) k_penalize(ObstItems it, double *__restrict__ vel, const double *__restrict__ chi_field, double dt,
                                                   double lambdaFac, int implicit, double cm0, double cm1, double cm2, double v0, double v1, double v2,
                                                   double o0, double o1, double o2, double *__restrict__ forces /* [n][6] */) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  penalize_block(it, i, vel, chi_field, dt, lambdaFac, implicit, cm0, cm1, cm2, v0, v1, v2, o0, o1, o2, forces + (size_t)i * 6, red);
}

// kernelUpdateTmpV on ObstacleBlock i of `it`; the body of both k_update_tmpv and k_update_tmpv_set
__device__ __forceinline__ void update_tmpv_block(const ObstItems &it, const int i, double *__restrict__ tmpV, const double *__restrict__ chi_field) {
  const int t = threadIdx.x;
  const int slot = it.slots[i];
  for (int k = 0; k < 2; ++k) {
    const int c = k * 256 + t;
    if (chi_field[(size_t)slot * 512 + c] > it.chi[(size_t)i * 512 + c]) continue;
    const double *U = it.udef + ((size_t)i * 512 + c) * 3;
    double *b = tmpV + (size_t)slot * 1536 + c;
    b[0] += U[0]; b[512] += U[1]; b[1024] += U[2];
  }
}

__global__ void __launch_bounds__(256) k_update_tmpv(ObstItems it, double *__restrict__ tmpV, const double *__restrict__ chi_field) {
  update_tmpv_block(it, blockIdx.x, tmpV, chi_field);
}

namespace {
struct DevBuf {
  void *p = nullptr;
  size_t size = 0;  // bytes allocated
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), size(o.size) { o.p = nullptr; o.size = 0; }  // a retained buffer changes hands (RetainedObstacles)
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(size, o.size); return *this; }
  int alloc(size_t bytes) { CUP3D_HIP(hipMalloc(&p, bytes ? bytes : 8)); size = bytes ? bytes : 8; return CUP3D_OK; }
  int upload(const void *src, size_t bytes) {
    int rc = alloc(bytes);
    if (rc) return rc;
    if (bytes) CUP3D_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream()));
    return CUP3D_OK;
  }
  ~DevBuf() { if (p) hipFree(p); }
};

int stage(const Sim *s, const cup3d_obstacle &o, DevBuf &slots, DevBuf &geom, DevBuf &chi, DevBuf &udef, ObstItems *it) {
  const Grid *g = s->grid;
  std::vector<double> gm(4 * (size_t)o.nblocks);
  for (long i = 0; i < o.nblocks; ++i) {
    const int32_t b = o.slots[i];
    if (b < 0 || b >= s->nb) { set_error("obstacle block slot %d out of range", (int)b); return CUP3D_EINVAL; }
    const double h = g->multilevel ? g->hb[b] : g->h;
    gm[4 * i] = h;
    for (int d = 0; d < 3; ++d) gm[4 * i + 1 + d] = g->index[3 * (size_t)b + d] * kBS * h;  // Info::origin, main.cpp:1066-1068
  }
  int rc;
  if ((rc = slots.upload(o.slots, o.nblocks * sizeof(int32_t))) || (rc = geom.upload(gm.data(), gm.size() * sizeof(double))) ||
      (rc = chi.upload(o.chi, (size_t)o.nblocks * 512 * sizeof(double))) || (rc = udef.upload(o.udef, (size_t)o.nblocks * 1536 * sizeof(double))))
    return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));  // gm is a local
  it->slots = (const int32_t *)slots.p;
  it->geom = (const double *)geom.p;
  it->chi = (const double *)chi.p;
  it->udef = (const double *)udef.p;
  return CUP3D_OK;
}

// the first `width` columns of rows [n][stride] added in ascending slot order onto total[width]: the reference's loops over
// obstacleBlocks with one thread
void add_rows_in_slot_order(const int32_t *slots, long n, const double *rows, int stride, int width, double *total) {
  std::vector<long> order(n);
  for (long i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](long a, long b) { return slots[a] < slots[b]; });
  for (long i : order)
    for (int q = 0; q < width; ++q) total[q] += rows[(size_t)i * stride + q];
}

// The host half of kernelFinalizePenalizationForce (13913-13938) that cup3d_penalization and cup3d_penalization_resident share: obstacle
// k's six sums M[0..5] cross the ranks, MPI_Allreduce(M, 6) at 13931, on the stream every RCCL call of the library uses.
// M[6] rides along: 0, or 1 from a rank whose local part failed (rc != 0) -- the ranks agree on the outcome in the collective they hold
// anyway, so that one rank's bad obstacle returns an error everywhere instead of leaving the others inside the all-reduce
int penalization_force_over_ranks(Sim *s, const char *who, int k, int rc, double *M /* [7] */) {
  if (scalars_cross_ranks(s)) {
    M[6] = rc ? 1.0 : 0.0;
    double *d = s->d_red;
    hipStream_t cs = scalar_stream(s);
    int rc2;
    CUP3D_HIP(hipStreamSynchronize(stream()));
    CUP3D_HIP(hipMemcpyAsync(d, M, 7 * sizeof(double), hipMemcpyHostToDevice, cs));
    if ((rc2 = allreduce(s, d, 7, false, cs))) return rc ? rc : rc2;
    CUP3D_HIP(hipMemcpyAsync(M, d, 7 * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
    if (!rc && M[6] != 0.0) {
      set_error("%s: obstacle %d failed on %d other rank(s)", who, k, (int)M[6]);
      rc = CUP3D_ECOMM;
    }
  }
  return rc;
}

// Obstacle::force / torque (13932-13937)
void force_from_sums(const double *M, double *force, double *torque) {
  for (int d = 0; d < 3; ++d) { force[d] = M[d]; torque[d] = M[3 + d]; }
}
}  // namespace

}  // namespace cup3d

using namespace cup3d;

extern "C" int cup3d_penalization(cup3d_sim_t *h, double dt, double lambda, int implicit, int nobst, cup3d_obstacle *obst) {
  if (!h || (nobst > 0 && !obst) || dt <= 0) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const double lambdaFac = implicit ? lambda : 1.0 / dt;  // 13867
  for (int k = 0; k < nobst; ++k) {  // obstacles one after the other, as KernelPenalization::operator() visits them (13849-13852)
    cup3d_obstacle &o = obst[k];
    for (int d = 0; d < 3; ++d) o.force[d] = o.torque[d] = 0.0;
    // A rank whose share of the grid this obstacle does not touch still takes part in the all-reduce below with M = 0: the
    // reference issues MPI_Allreduce(M, 6) for every obstacle on every rank (13931), and skipping it here would pair this rank's
    // NEXT collective with the other ranks' 6-double sum.  M[6] is penalization_force_over_ranks' flag.
    double M[7] = {0, 0, 0, 0, 0, 0, 0};
    auto local_part = [&]() -> int {
      if (o.nblocks <= 0) return CUP3D_OK;
      int rc;
      if (!o.slots || !o.chi || !o.udef) { set_error("cup3d_penalization: obstacle %d has blocks but no slots / chi / udef", k); return CUP3D_EINVAL; }
      DevBuf slots, geom, chi, udef, forces;
      ObstItems it;
      if ((rc = stage(s, o, slots, geom, chi, udef, &it))) return rc;
      if ((rc = forces.alloc((size_t)o.nblocks * 6 * sizeof(double)))) return rc;
      {
        ProfileScope ps("penalization");
        hipLaunchKernelGGL(k_penalize, dim3((unsigned)o.nblocks), dim3(256), 0, stream(), it, s->vel, s->chi, dt, lambdaFac, implicit ? 1 : 0, o.cm[0], o.cm[1],
                           o.cm[2], o.vel[0], o.vel[1], o.vel[2], o.omega[0], o.omega[1], o.omega[2], (double *)forces.p);
      }
      CUP3D_HIP(hipGetLastError());
      std::vector<double> F((size_t)o.nblocks * 6);
      CUP3D_HIP(hipMemcpyAsync(F.data(), forces.p, F.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
      // kernelFinalizePenalizationForce (13913-13938): block totals in block (slot) order
      add_rows_in_slot_order(o.slots, o.nblocks, F.data(), 6, 6, M);
      return CUP3D_OK;
    };
    int rc = penalization_force_over_ranks(s, "cup3d_penalization", k, local_part(), M);
    if (rc) return rc;
    force_from_sums(M, o.force, o.torque);
  }
  return CUP3D_OK;
}

extern "C" int cup3d_update_tmpv(cup3d_sim_t *h, int nobst, const cup3d_obstacle *obst) {
  if (!h || (nobst > 0 && !obst)) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  for (int k = 0; k < nobst; ++k) {
    const cup3d_obstacle &o = obst[k];
    if (o.nblocks <= 0) continue;
    if (!o.slots || !o.chi || !o.udef) return CUP3D_EINVAL;
    DevBuf slots, geom, chi, udef;
    ObstItems it;
    int rc = stage(s, o, slots, geom, chi, udef, &it);
    if (rc) return rc;
    ProfileScope ps("update_tmpv");
    hipLaunchKernelGGL(k_update_tmpv, dim3((unsigned)o.nblocks), dim3(256), 0, stream(), it, s->tmpV, s->chi);
    CUP3D_HIP(hipGetLastError());
    CUP3D_HIP(hipStreamSynchronize(stream()));  // the staged arrays are freed on scope exit
  }
  if (nobst > 0) s->udef_nonzero = true;
  return CUP3D_OK;
}

// ==== cup3d_update_obstacles.  UpdateObstacles::operator() (main.cpp:13812-13837): KernelIntegrateFluidMomenta<0/1>::visit (13637-13734)
// on the device, kernelFinalizeObstacleVel (13737-13811) and Obstacle::computeVelocities (12921-13068) on the host.
// One wavefront per ObstacleBlock.  The reference adds the cells of a block in iz, iy, ix order and skips those with chi <= 0, and so does
// the kernel: per z-plane (64 cells) every lane evaluates one cell and leaves its summands in LDS, then lanes 0..28 each add one quantity
// over the plane in cell order onto a running total they keep in a register -- only the cells the reference visits (a ballot of the
// wavefront says which), so that a skipped cell is neither read from LDS nor multiplied by zero.  No tree, no atomic: the sums are the
// reference's bit for bit.  The rows of sm are padded by one double: lane q reads sm[q][j], and a row length of 64 doubles would put all
// 29 readers on one LDS bank.
namespace cup3d {

constexpr int kMomenta = 29;          // M of kernelFinalizeObstacleVel (13748-13777): V, FX FY FZ, TX TY TZ, J0..J5, then with implicit
constexpr int kMomentaExplicit = 13;  // penalisation GfX, GpX GpY GpZ, Gj0..Gj5, GuX GuY GuZ, GaX GaY GaZ
// J3..J5 and Gj3..Gj5 are accumulated with -= (13698-13700, 13720-13722)
constexpr unsigned kMomentaSubtracted = (1u << 10) | (1u << 11) | (1u << 12) | (1u << 20) | (1u << 21) | (1u << 22);

// KernelIntegrateFluidMomenta on ObstacleBlock b of `it` by one wavefront; the block's 29 sums go to sums[0..28].  The body of both
// k_fluid_momenta and k_fluid_momenta_set.
__device__ __forceinline__ void fluid_momenta_block(const ObstItems &it, const int b, const double *__restrict__ vel, double lambdt, int implicit, double cm0,
                                                    double cm1, double cm2, double *__restrict__ sums /* [29] */, double (*sm)[65] /* LDS [29][65] */) {
  const int lane = threadIdx.x;
  const int slot = it.slots[b];
  const double h = it.geom[4 * b], dv = h * h * h;  // dvol, 13629
  const int nq = implicit ? kMomenta : kMomentaExplicit;
  const int ix = lane & 7, iy = lane >> 3;
  const bool subtracted = (kMomentaSubtracted >> lane) & 1u;
  double total = 0.0;  // lanes 0..nq-1: the running sum of quantity `lane`
  for (int iz = 0; iz < 8; ++iz) {
    const int c = iz * 64 + lane;
    const double X = it.chi[(size_t)b * 512 + c];
    const bool visited = !(X <= 0);  // `if (CHI[iz][iy][ix] <= 0) continue;`
    const unsigned long long mask = __ballot(visited);
    if (visited) {
      double p[3] = {it.geom[4 * b + 1] + h * (ix + 0.5), it.geom[4 * b + 2] + h * (iy + 0.5), it.geom[4 * b + 3] + h * (iz + 0.5)};
      p[0] -= cm0; p[1] -= cm1; p[2] -= cm2;
      const double *u = vel + (size_t)slot * 1536 + c;
      const double u0 = u[0], u1 = u[512], u2 = u[1024];
      sm[0][lane] = X * dv;
      sm[1][lane] = X * dv * u0;
      sm[2][lane] = X * dv * u1;
      sm[3][lane] = X * dv * u2;
      sm[4][lane] = X * dv * (p[1] * u2 - p[2] * u1);
      sm[5][lane] = X * dv * (p[2] * u0 - p[0] * u2);
      sm[6][lane] = X * dv * (p[0] * u1 - p[1] * u0);
      sm[7][lane] = X * dv * (p[1] * p[1] + p[2] * p[2]);
      sm[8][lane] = X * dv * (p[0] * p[0] + p[2] * p[2]);
      sm[9][lane] = X * dv * (p[0] * p[0] + p[1] * p[1]);
      sm[10][lane] = X * dv * p[0] * p[1];
      sm[11][lane] = X * dv * p[0] * p[2];
      sm[12][lane] = X * dv * p[1] * p[2];
      if (implicit) {
        const double X1 = X > 0.5 ? 1.0 : 0.0;
        const double penalFac = dv * lambdt * X1 / (1 + X1 * lambdt);
        const double *U = it.udef + ((size_t)b * 512 + c) * 3;
        const double DiffU[3] = {u0 - U[0], u1 - U[1], u2 - U[2]};
        sm[13][lane] = penalFac;
        sm[14][lane] = penalFac * p[0];
        sm[15][lane] = penalFac * p[1];
        sm[16][lane] = penalFac * p[2];
        sm[17][lane] = penalFac * (p[1] * p[1] + p[2] * p[2]);
        sm[18][lane] = penalFac * (p[0] * p[0] + p[2] * p[2]);
        sm[19][lane] = penalFac * (p[0] * p[0] + p[1] * p[1]);
        sm[20][lane] = penalFac * p[0] * p[1];
        sm[21][lane] = penalFac * p[0] * p[2];
        sm[22][lane] = penalFac * p[1] * p[2];
        sm[23][lane] = penalFac * DiffU[0];
        sm[24][lane] = penalFac * DiffU[1];
        sm[25][lane] = penalFac * DiffU[2];
        sm[26][lane] = penalFac * (p[1] * DiffU[2] - p[2] * DiffU[1]);
        sm[27][lane] = penalFac * (p[2] * DiffU[0] - p[0] * DiffU[2]);
        sm[28][lane] = penalFac * (p[0] * DiffU[1] - p[1] * DiffU[0]);
      }
    }
    __syncthreads();
    if (lane < nq) {
      for (int j = 0; j < 64; ++j)
        if ((mask >> j) & 1ull) {
          const double x = sm[lane][j];
          total = subtracted ? total - x : total + x;
        }
    }
    __syncthreads();
  }
  if (lane < kMomenta) sums[lane] = lane < nq ? total : 0.0;
}

__global__ void __launch_bounds__(64) k_fluid_momenta(ObstItems it, const double *__restrict__ vel, double lambdt, int implicit, double cm0, double cm1,
                                                       double cm2, double *__restrict__ sums /* [n][29] */) {
  __shared__ double sm[kMomenta][65];
  const int b = blockIdx.x;
  fluid_momenta_block(it, b, vel, lambdt, implicit, cm0, cm1, cm2, sums + (size_t)b * kMomenta, sm);
}

namespace {
// Dense LU with partial pivoting for the 6 x 6 system of Obstacle::computeVelocities (what the reference asks of gsl_linalg_LU_decomp /
// gsl_linalg_LU_solve, 13015-13021): row-major A and b are overwritten, the first largest |entry| of a column is the pivot, the right-hand
// side is eliminated along with the rows.  A zero pivot is divided by all the same, so that a singular system gives non-finite velocities
// as it does in the reference, not a silent answer.
void lu_solve6(double *A, double *b, double *x) {
  constexpr int n = 6;
  for (int j = 0; j + 1 < n; ++j) {
    int piv = j;
    for (int i = j + 1; i < n; ++i)
      if (std::fabs(A[i * n + j]) > std::fabs(A[piv * n + j])) piv = i;
    if (piv != j) {
      for (int k = 0; k < n; ++k) std::swap(A[j * n + k], A[piv * n + k]);
      std::swap(b[j], b[piv]);
    }
    if (A[j * n + j] == 0.0) continue;  // nothing below the diagonal of this column either
    for (int i = j + 1; i < n; ++i) {
      const double l = A[i * n + j] / A[j * n + j];
      A[i * n + j] = l;
      for (int k = j + 1; k < n; ++k) A[i * n + k] -= l * A[j * n + k];
      b[i] -= l * b[j];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    x[i] = b[i];
    for (int k = i + 1; k < n; ++k) x[i] -= A[i * n + k] * x[k];
    x[i] /= A[i * n + i];
  }
}

// kernelFinalizeObstacleVel's two branches (13796-13808) and Obstacle::computeVelocities up to transVel_computed / angVel_computed
// (12921-13027); x = transVel_computed, angVel_computed
void rigid_motion_from_momenta(const double *M, int implicit, const cup3d_obstacle_motion &mo, double *x) {
  double penalM, penalCM[3], penalJ[6], penalLmom[3], penalAmom[3];
  if (implicit) {
    penalM = M[13];
    for (int d = 0; d < 3; ++d) { penalCM[d] = M[14 + d]; penalLmom[d] = M[23 + d]; penalAmom[d] = M[26 + d]; }
    for (int q = 0; q < 6; ++q) penalJ[q] = M[17 + q];
  } else {
    penalM = M[0];
    for (int d = 0; d < 3; ++d) { penalCM[d] = 0; penalLmom[d] = M[1 + d]; penalAmom[d] = M[4 + d]; }
    for (int q = 0; q < 6; ++q) penalJ[q] = M[7 + q];
  }
  double A[36] = {penalM,      0.0,         0.0,         0.0,         +penalCM[2], -penalCM[1],   // 12923-12958
                  0.0,         penalM,      0.0,         -penalCM[2], 0.0,         +penalCM[0],
                  0.0,         0.0,         penalM,      +penalCM[1], -penalCM[0], 0.0,
                  0.0,         -penalCM[2], +penalCM[1], penalJ[0],   penalJ[3],   penalJ[4],
                  +penalCM[2], 0.0,         -penalCM[0], penalJ[3],   penalJ[1],   penalJ[5],
                  -penalCM[1], +penalCM[0], 0.0,         penalJ[4],   penalJ[5],   penalJ[2]};
  double b[6] = {penalLmom[0], penalLmom[1], penalLmom[2], penalAmom[0], penalAmom[1], penalAmom[2]};
  for (int d = 0; d < 3; ++d) {
    if (mo.forced[d]) {  // 12967-12990: the row keeps its diagonal only
      for (int k = 0; k < 6; ++k)
        if (k != d) A[d * 6 + k] = 0;
      b[d] = penalM * mo.vel_imposed[d];
    }
    if (mo.block_rotation[d]) {  // 12991-13014
      for (int k = 0; k < 6; ++k)
        if (k != 3 + d) A[(3 + d) * 6 + k] = 0;
      b[3 + d] = 0;
    }
  }
  lu_solve6(A, b, x);
}

// What cup3d_update_obstacles and cup3d_update_obstacles_resident keep of one obstacle until every obstacle of the call has passed
struct MomentaResult {
  const double *rows = nullptr;  // [nblocks][29] in the order listed, or nullptr
  long nblocks = 0;
  double M[kMomenta];
  double x[6];
};

// The host half of UpdateObstacles for obstacle k once this rank's block rows are added into R.M (rc: what that local part returned):
// the all-reduce over ranks (13783), the assert on the volume (13795) and Obstacle::computeVelocities.  red: the call's device buffer
// of 32 doubles where scalars cross ranks.
int obstacle_motion_from_sums(Sim *s, const char *who, int k, int rc, double *red, int implicit, const cup3d_obstacle_motion &mo, MomentaResult &R) {
  double *M = R.M;
  if (scalars_cross_ranks(s)) {
    // the in-process communicator of the tests carries 16 values per all-reduce: two of them, the second with the flag -- 0, or 1 from a
    // rank whose local part failed, so that one rank's bad obstacle returns an error everywhere (as in cup3d_penalization)
    double buf[32] = {0};
    for (int q = 0; q < kMomenta; ++q) buf[q] = rc ? 0.0 : M[q];
    buf[kMomenta] = rc ? 1.0 : 0.0;
    double *d = red;
    hipStream_t cs = scalar_stream(s);
    int rc2;
    CUP3D_HIP(hipStreamSynchronize(stream()));
    CUP3D_HIP(hipMemcpyAsync(d, buf, 32 * sizeof(double), hipMemcpyHostToDevice, cs));
    if ((rc2 = allreduce(s, d, 16, false, cs)) || (rc2 = allreduce(s, d + 16, kMomenta + 1 - 16, false, cs))) return rc ? rc : rc2;
    CUP3D_HIP(hipMemcpyAsync(buf, d, 32 * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
    for (int q = 0; q < kMomenta; ++q) M[q] = buf[q];
    if (!rc && buf[kMomenta] != 0.0) {
      set_error("%s: obstacle %d failed on %d other rank(s)", who, k, (int)buf[kMomenta]);
      rc = CUP3D_ECOMM;
    }
  }
  if (rc) return rc;
  if (!(M[0] > DBL_EPSILON)) {  // assert(M[0] > EPS), 13795: the same total on every rank
    set_error("%s: obstacle %d has volume %g", who, k, M[0]);
    return CUP3D_EINVAL;
  }
  rigid_motion_from_momenta(M, implicit, mo, R.x);
  return CUP3D_OK;
}

// every obstacle of the call has passed: the caller's arrays of one of them; vel / omega are the obstacle's transVel / angVel
void write_obstacle_motion(const MomentaResult &R, int nq, cup3d_obstacle_motion &mo, double *vel, double *omega) {
  if (mo.block_sums)
    for (long i = 0; i < R.nblocks; ++i)
      for (int q = 0; q < nq; ++q) mo.block_sums[(size_t)i * kMomenta + q] = R.rows[(size_t)i * kMomenta + q];
  for (int q = 0; q < kMomenta; ++q) mo.totals[q] = R.M[q];
  for (int d = 0; d < 3; ++d) {
    mo.vel_computed[d] = R.x[d];
    mo.omega_computed[d] = R.x[3 + d];
    vel[d] = mo.forced[d] ? mo.vel_imposed[d] : R.x[d];      // 13039-13053
    omega[d] = mo.block_rotation[d] ? 0.0 : R.x[3 + d];      // 13054-13068
  }
}
}  // namespace

}  // namespace cup3d

extern "C" int cup3d_update_obstacles(cup3d_sim_t *h, double dt, double lambda, int implicit, int nobst, cup3d_obstacle *obst, cup3d_obstacle_motion *motion) {
  if (!h || nobst < 0 || !(dt > 0) || (nobst > 0 && (!obst || !motion))) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const int nq = implicit ? kMomenta : kMomentaExplicit;
  const double lambdt = lambda * dt;  // 13664
  // nothing of the caller's is written before every obstacle of the call has passed: the results wait here
  std::vector<MomentaResult> res((size_t)nobst);
  std::vector<std::vector<double>> rows((size_t)nobst);
  const bool cross = scalars_cross_ranks(s);
  DevBuf red;  // the all-reduce operand of this call: M[0..15] | M[16..28], error flag
  if (cross && nobst > 0) {
    int rc = red.alloc(32 * sizeof(double));
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) {  // obstacles one after the other, as kernelFinalizeObstacleVel visits them (13739)
    const cup3d_obstacle &o = obst[k];
    MomentaResult &R = res[k];
    double *M = R.M;
    for (int q = 0; q < kMomenta; ++q) M[q] = 0.0;
    // a rank that holds none of the obstacle's blocks still takes part in the all-reduce with M = 0 (MPI_Allreduce(M, 29), 13783)
    auto local_part = [&]() -> int {
      if (o.nblocks < 0) { set_error("cup3d_update_obstacles: obstacle %d has nblocks = %ld", k, o.nblocks); return CUP3D_EINVAL; }
      if (o.nblocks == 0) return CUP3D_OK;
      int rc;
      if (!o.slots || !o.chi || !o.udef) { set_error("cup3d_update_obstacles: obstacle %d has blocks but no slots / chi / udef", k); return CUP3D_EINVAL; }
      DevBuf slots, geom, chi, udef, sums;
      ObstItems it;
      if ((rc = stage(s, o, slots, geom, chi, udef, &it))) return rc;
      if ((rc = sums.alloc((size_t)o.nblocks * kMomenta * sizeof(double)))) return rc;
      {
        ProfileScope ps("update_obstacles");
        hipLaunchKernelGGL(k_fluid_momenta, dim3((unsigned)o.nblocks), dim3(64), 0, stream(), it, (const double *)s->vel, lambdt, implicit ? 1 : 0, o.cm[0], o.cm[1],
                           o.cm[2], (double *)sums.p);
      }
      CUP3D_HIP(hipGetLastError());
      rows[k].resize((size_t)o.nblocks * kMomenta);
      CUP3D_HIP(hipMemcpyAsync(rows[k].data(), sums.p, rows[k].size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
      stats_field_download(rows[k].size() * sizeof(double));
      R.rows = rows[k].data();
      R.nblocks = o.nblocks;
      // kernelFinalizeObstacleVel's loop with one thread (13744-13781): block rows in block (slot) order
      add_rows_in_slot_order(o.slots, o.nblocks, R.rows, kMomenta, nq, M);
      return CUP3D_OK;
    };
    int rc = obstacle_motion_from_sums(s, "cup3d_update_obstacles", k, local_part(), (double *)red.p, implicit, motion[k], R);
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) write_obstacle_motion(res[k], nq, motion[k], obst[k].vel, obst[k].omega);
  return CUP3D_OK;
}

// ==== cup3d_compute_forces / cup3d_compute_forces_over_ranks.  KernelComputeForces::visit (main.cpp:12273-12493) for the ObstacleBlocks of
// one obstacle that have surface points: per point the one-sided finite differences of the velocity along the surface normal on the
// block's [-4,5) tensorial tile, the 19 per-point arrays and the 19 block sums.  The tiles are the ones cup3d_sim_labs_device writes
// (Matrix3D layout, [16][16][16][nc]) into a scratch buffer of the sim, a bounded number of blocks at a time.
// One wavefront per block.  The reference adds the points of a block in order i = 0..nPoints-1, and so does the kernel: per chunk of 64
// points every lane evaluates one point and leaves its 19 summands in LDS, then lanes 0..18 each add one quantity over the chunk in point
// order onto a running total they keep in a register.  No tree, no atomic: the sums are the reference's bit for bit.
// Of the nineteen sums the functor zeroes eleven at entry (12283-12293); forcey, forcez, forcey_P, forcez_P, forcey_V, forcez_V, PoutBnd
// and defPowerBnd go on from what the block held, so qoi is in/out.
// Kept as written: the `sx` in the 2-point branch of dveldy (12364) and the precedence of the mixed derivatives' fallback,
// sx*sy*(a - b) - (c - d) (12394-12395, 12406-12407, 12418-12419).
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

__global__ void __launch_bounds__(64) k_surface_forces(SurfItems it, const double *__restrict__ pres, double nu, double cm0, double cm1, double cm2, double u0,
                                                        double u1, double u2, double o0, double o1, double o2) {
  __shared__ double sm[kQoI][64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double h = it.geom[4 * b];
  const double *__restrict__ VT = it.vel + (size_t)b * 12288;
  const double *__restrict__ XT = it.chi + (size_t)b * 4096;
  const int p0 = it.first[b], p1 = it.first[b + 1];
  double total = 0.0;  // lanes 0..18: the running sum of quantity `lane`
  if (lane < kQoI && ((kQoICarried >> lane) & 1u)) total = it.qoi[(size_t)b * kQoI + lane];
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
      const int ix = it.ijk[3 * (size_t)i], iy = it.ijk[3 * (size_t)i + 1], iz = it.ijk[3 * (size_t)i + 2];
      const double px = it.geom[4 * b + 1] + h * (ix + 0.5), py = it.geom[4 * b + 2] + h * (iy + 0.5), pz = it.geom[4 * b + 3] + h * (iz + 0.5);
      const double normX = it.dchi[3 * (size_t)i], normY = it.dchi[3 * (size_t)i + 1], normZ = it.dchi[3 * (size_t)i + 2];
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
      const double P = pres[(size_t)it.slots[b] * 512 + cell];
      const double fXV = _1oH * (dudx * normX + dudy * normY + dudz * normZ);
      const double fYV = _1oH * (dvdx * normX + dvdy * normY + dvdz * normZ);
      const double fZV = _1oH * (dwdx * normX + dwdy * normY + dwdz * normZ);
      const double fXP = -P * normX, fYP = -P * normY, fZP = -P * normZ;
      const double fXT = fXV + fXP, fYT = fYV + fYP, fZT = fZV + fZP;
      const double *__restrict__ U = it.udef + ((size_t)b * 512 + cell) * 3;
      const double vxDef = U[0], vyDef = U[1], vzDef = U[2];
      const double *__restrict__ VC = VT + (((iz + 4) * 16 + (iy + 4)) * 16 + (ix + 4)) * 3;
      const double vX = VC[0], vY = VC[1], vZ = VC[2];
      double *__restrict__ o = it.points + i;
      const size_t np = (size_t)it.npoints;
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
  if (lane < kQoI) it.qoi[(size_t)b * kQoI + lane] = total;
}

// device buffers of cup3d_compute_forces, kept in the sim and only ever grown: the tile scratch of one chunk of blocks and the staged
// arrays of one obstacle
struct ForcesScratch {
  struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    int need(size_t bytes, Sim *s) {
      if (bytes <= cap) return CUP3D_OK;
      if (p) { (void)hipFree(p); s->bytes -= cap; p = nullptr; cap = 0; }
      CUP3D_HIP(hipMalloc(&p, bytes));
      cap = bytes;
      s->bytes += bytes;
      return CUP3D_OK;
    }
    int upload(const void *src, size_t bytes, Sim *s) {
      int rc = need(bytes ? bytes : 8, s);
      if (rc) return rc;
      if (bytes) CUP3D_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream()));
      return CUP3D_OK;
    }
  };
  Buf vel, chi, slots, geom, first, ijk, dchi, udef, points, qoi;
};

void forces_destroy(Sim *s) {
  ForcesScratch *F = s->forces;
  if (!F) return;
  ForcesScratch::Buf *all[] = {&F->vel, &F->chi, &F->slots, &F->geom, &F->first, &F->ijk, &F->dchi, &F->udef, &F->points, &F->qoi};
  for (ForcesScratch::Buf *b : all)
    if (b->p) { (void)hipFree(b->p); s->bytes -= b->cap; }
  delete F;
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
  const Grid *g = s->grid;
  const size_t nb = (size_t)o.nblocks, np = (size_t)o.first[o.nblocks];
  std::vector<double> gm(4 * nb);
  for (size_t i = 0; i < nb; ++i) {
    const int32_t b = o.slots[i];
    const double h = g->multilevel ? g->hb[b] : g->h;
    gm[4 * i] = h;
    for (int d = 0; d < 3; ++d) gm[4 * i + 1 + d] = g->index[3 * (size_t)b + d] * kBS * h;  // Info::origin, main.cpp:1066-1068
  }
  int rc;
  if ((rc = F->slots.upload(o.slots, nb * sizeof(int32_t), s)) || (rc = F->geom.upload(gm.data(), gm.size() * sizeof(double), s)) ||
      (rc = F->first.upload(o.first, (nb + 1) * sizeof(int32_t), s)) || (rc = F->ijk.upload(o.ijk, np * 3 * sizeof(int32_t), s)) ||
      (rc = F->dchi.upload(o.dchi, np * 3 * sizeof(double), s)) || (rc = F->udef.upload(o.udef, nb * 1536 * sizeof(double), s)) ||
      (rc = F->qoi.upload(o.qoi, nb * kQoI * sizeof(double), s)) || (rc = F->points.need(std::max<size_t>(np, 1) * kQoI * sizeof(double), s)))
    return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));  // gm is a local
  *it = SurfItems{(const int32_t *)F->slots.p, (const double *)F->geom.p, (const int32_t *)F->first.p, (const int32_t *)F->ijk.p, (const double *)F->dchi.p,
                  (const double *)F->udef.p, (const double *)F->vel.p, (const double *)F->chi.p, (double *)F->points.p, (double *)F->qoi.p, (long)np};
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
    if (np) CUP3D_HIP(hipMemcpyAsync(o.points, F->points.p, np * kQoI * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipMemcpyAsync(o.qoi, F->qoi.p, nb * kQoI * sizeof(double), hipMemcpyDeviceToHost, stream()));
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
}  // namespace

}  // namespace cup3d

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
      if ((rc = cup3d_sim_labs_device(h, CUP3D_FIELD_VEL, m, o.slots + t0, 4, 1, -1, s->forces->vel.p)) ||
          (rc = cup3d_sim_labs_device(h, CUP3D_FIELD_CHI, m, o.slots + t0, 4, 1, -1, s->forces->chi.p)) || (rc = surface_launch(s, o, it, t0, m, nu)))
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
  long most = 0;
  {
    std::vector<long> count(std::max(s->grid->nranks, 1), 0);
    for (int64_t b = 0; b < gm->nblocks(); ++b)
      if (owner[b] >= 0 && owner[b] < (int32_t)count.size()) most = std::max(most, ++count[owner[b]]);
  }
  const long chunk = forces_chunk(/*over_ranks=*/true);
  const long rounds = (most + chunk - 1) / chunk;
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
      if ((rc = cup3d_sim_labs_over_ranks_device(h, mesh, owner, CUP3D_FIELD_VEL, m, m ? o.slots + t0 : nullptr, 4, 1, -1, m ? s->forces->vel.p : nullptr)) ||
          (rc = cup3d_sim_labs_over_ranks_device(h, mesh, owner, CUP3D_FIELD_CHI, m, m ? o.slots + t0 : nullptr, 4, 1, -1, m ? s->forces->chi.p : nullptr)))
        return rc;
      if (m && (rc = surface_launch(s, o, it, t0, m, nu))) return rc;
    }
    if (nblocks && (rc = surface_download(s, o))) return rc;
  }
  if (bad) { set_error("%s", bad_text.c_str()); return bad; }
  return CUP3D_OK;
}

// ==== cup3d_create_obstacles.  The grid half of CreateObstacles::operator() (main.cpp:13596-13619): the chi field cleared,
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
  auto X = [&](int k, int j, int i) { return chi[(k * 8 + j) * 8 + i]; };
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
    double Delta = 0.0;
    if (!(gradHX * gradHX + gradHY * gradHY + gradHZ * gradHZ < 1e-12)) {
      const double numD = gradHX * gradUX + gradHY * gradUY + gradHZ * gradUZ;
      Delta = fac1 * numD / gradUSq;
      accepted = Delta > EPS;
    }
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
  DevBuf slots, geom, sdf, udef, chi, com, momenta, count, st_ijk, st_dchi, st_delta, first, ijk, dchi, delta;
  ShapeItems it;
  std::vector<double> com_rows, momenta_rows;
  std::vector<int32_t> first_h;
  double com_totals[4], M[kUdefMomenta], cm[3], transvel[3], angvel[3];
};

}  // namespace

// How the resident operators (cup3d_update_obstacles_resident, cup3d_penalization_resident, cup3d_update_tmpv_resident) walk the
// retained set; built from the slots_h lists by the first of them to run after a cup3d_create_obstacles.
// Row r = row_base[k] + i stands for block i of obstacle k in the order listed.  The slot-major schedule lists, per distinct slot any
// obstacle holds, in ascending slot order, the rows of that slot in ascending k (an obstacle's slots are distinct: at most one row per
// obstacle): rows sched_rows[sched_first[j] .. sched_first[j + 1]) for the j-th slot.
struct ResidentPlan {
  long rows = 0, nslots = 0;
  std::vector<long> row_base;   // [N + 1]
  DevBuf obst;                  // ObstItems [N]: the retained slots, geom, chi, udef of every obstacle
  DevBuf row_obst, row_block;   // int32 [rows]: k and i of a row
  DevBuf sched_first, sched_rows;  // int32 [nslots + 1], [rows]
  DevBuf body;                  // double [N][9]: the call's cm, vel, omega of every obstacle
  DevBuf out;                   // double [rows][29]: the call's block rows ([rows][6] for the penalisation forces)
  size_t bytes = 0;
};

// The ShapeWork buffers of the last successful cup3d_create_obstacles that the collision model and the resident operators read, moved
// here instead of freed.
struct RetainedObstacles {
  struct One {
    long nblocks = 0;
    std::vector<int32_t> slots_h;       // the caller's slot list, for the intersections and the plan
    DevBuf slots, geom, sdf, chi, udef;  // [n], [n][4], [n][10][10][10], [n][8][8][8], [n][8][8][8][3] (corrected)
  };
  std::vector<One> obst;
  ResidentPlan *plan = nullptr;  // nullptr until a resident operator asks for it
  size_t bytes = 0;  // counted in Sim::bytes, the plan's included once it exists
  ~RetainedObstacles() { delete plan; }
};

void retained_destroy(Sim *s) {
  if (!s->retained) return;
  s->bytes -= s->retained->bytes;
  delete s->retained;  // DevBuf frees
  s->retained = nullptr;
}

}  // namespace cup3d

// the call itself; `work` holds every obstacle's device buffers when it returns, whatever it returns
static int create_obstacles(Sim *s, int nobst, cup3d_obstacle_shape *shapes, std::vector<ShapeWork> &work) {
  const bool cross = scalars_cross_ranks(s);
  // nothing is written, on the device or the host, before every obstacle of the call has passed.  Over ranks a rank whose own arguments
  // are refused still takes part in the first all-reduce, where its flag ends the call on every rank.
  int bad = CUP3D_OK;
  for (int k = 0; k < nobst && !bad; ++k) bad = shape_check(s, shapes[k], k);
  if (bad && !cross) return bad;
  const std::string bad_text = bad ? cup3d_last_error() : "";
  DevBuf red;  // the all-reduce operand of this call: up to 13 totals and the error flag
  int rc;
  if (cross && (rc = red.alloc(16 * sizeof(double)))) return rc;
  // v[n] summed over the ranks along with a flag -- 0, or 1 from a rank whose local part failed -- so that one rank's failure is an error
  // everywhere and leaves no rank inside a collective (as in cup3d_update_obstacles); n <= 15
  auto over_ranks = [&](double *v, int n, int local, int k) -> int {
    if (!cross) return local;
    double buf[16] = {0};
    for (int q = 0; q < n; ++q) buf[q] = local ? 0.0 : v[q];
    buf[n] = local ? 1.0 : 0.0;
    double *d = (double *)red.p;
    hipStream_t cs = scalar_stream(s);
    int rc2;
    CUP3D_HIP(hipStreamSynchronize(stream()));
    CUP3D_HIP(hipMemcpyAsync(d, buf, 16 * sizeof(double), hipMemcpyHostToDevice, cs));
    if ((rc2 = allreduce(s, d, n + 1, false, cs))) return local ? local : rc2;
    CUP3D_HIP(hipMemcpyAsync(buf, d, 16 * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
    for (int q = 0; q < n; ++q) v[q] = buf[q];
    if (local) return local;
    if (buf[n] != 0.0) {
      set_error("cup3d_create_obstacles: obstacle %d failed on %d other rank(s)", k, (int)buf[n]);
      return CUP3D_ECOMM;
    }
    return CUP3D_OK;
  };
  if (!bad) {  // CHI.clear() of every block (13596-13600)
    CUP3D_HIP(hipMemsetAsync(s->chi, 0, (size_t)s->nb * 512 * sizeof(double), stream()));
    s->chi_nonzero = true;
  }
  for (int k = 0; k < nobst; ++k) {  // obstacles one after the other: the max into the chi field in the order 13301 visits them
    const cup3d_obstacle_shape &o = shapes[k];
    ShapeWork &W = work[k];
    const long n = bad ? 0 : o.nblocks;
    const size_t nb = (size_t)n;
    for (int q = 0; q < 4; ++q) W.com_totals[q] = 0.0;
    for (int q = 0; q < kUdefMomenta; ++q) W.M[q] = 0.0;
    W.first_h.assign(nb + 1, 0);
    auto characteristic = [&]() -> int {
      if (bad) return bad;
      if (n == 0) return CUP3D_OK;
      const Grid *g = s->grid;
      std::vector<double> gm(4 * nb);
      for (size_t i = 0; i < nb; ++i) {
        const int32_t b = o.slots[i];
        const double hb = g->multilevel ? g->hb[b] : g->h;
        gm[4 * i] = hb;
        for (int d = 0; d < 3; ++d) gm[4 * i + 1 + d] = g->index[3 * (size_t)b + d] * kBS * hb;  // Info::origin, main.cpp:1066-1068
      }
      int rc;
      if ((rc = W.slots.upload(o.slots, nb * sizeof(int32_t))) || (rc = W.geom.upload(gm.data(), gm.size() * sizeof(double))) ||
          (rc = W.sdf.upload(o.sdf, nb * 1000 * sizeof(double))) || (rc = W.udef.upload(o.udef, nb * 1536 * sizeof(double))) ||
          (rc = W.chi.alloc(nb * 512 * sizeof(double))) || (rc = W.com.alloc(nb * 4 * sizeof(double))) ||
          (rc = W.momenta.alloc(nb * kUdefMomenta * sizeof(double))) || (rc = W.count.alloc(nb * sizeof(int32_t))) ||
          (rc = W.st_ijk.alloc(nb * 1536 * sizeof(int32_t))) || (rc = W.st_dchi.alloc(nb * 1536 * sizeof(double))) ||
          (rc = W.st_delta.alloc(nb * 512 * sizeof(double))))
        return rc;
      CUP3D_HIP(hipStreamSynchronize(stream()));  // gm is a local
      W.it = ShapeItems{(const int32_t *)W.slots.p, (const double *)W.geom.p, (const double *)W.sdf.p, (double *)W.udef.p, (double *)W.chi.p, (double *)W.com.p,
                        (double *)W.momenta.p, (int32_t *)W.count.p, (int32_t *)W.st_ijk.p, (double *)W.st_dchi.p, (double *)W.st_delta.p};
      {
        ProfileScope ps("characteristic");
        hipLaunchKernelGGL(k_characteristic, dim3((unsigned)n), dim3(64), 0, stream(), W.it, s->chi);
      }
      CUP3D_HIP(hipGetLastError());
      W.com_rows.resize(nb * 4);
      std::vector<int32_t> count(nb);
      CUP3D_HIP(hipMemcpyAsync(W.com_rows.data(), W.com.p, nb * 4 * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipMemcpyAsync(count.data(), W.count.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
      stats_field_download(nb * (4 * sizeof(double) + sizeof(int32_t)));
      for (size_t i = 0; i < nb; ++i) {
        if (count[i] < 0 || count[i] > 512) { set_error("cup3d_create_obstacles: obstacle %d: block %ld reports %d surface points", k, (long)i, (int)count[i]); return CUP3D_ESTATE; }
        W.first_h[i + 1] = W.first_h[i] + count[i];
      }
      const size_t np = (size_t)W.first_h[nb];
      if ((rc = W.first.upload(W.first_h.data(), (nb + 1) * sizeof(int32_t))) || (rc = W.ijk.alloc(np * 3 * sizeof(int32_t))) ||
          (rc = W.dchi.alloc(np * 3 * sizeof(double))) || (rc = W.delta.alloc(np * sizeof(double))))
        return rc;
      {
        ProfileScope ps("pack_surface");
        hipLaunchKernelGGL(k_pack_surface, dim3((unsigned)n), dim3(64), 0, stream(), W.it, (const int32_t *)W.first.p, (int32_t *)W.ijk.p, (double *)W.dchi.p,
                           (double *)W.delta.p);
      }
      CUP3D_HIP(hipGetLastError());
      add_rows_in_slot_order(o.slots, n, W.com_rows.data(), 4, 4, W.com_totals);  // kernelComputeGridCoM, 13411-13418
      return CUP3D_OK;
    };
    rc = over_ranks(W.com_totals, 4, characteristic(), k);  // MPI_Allreduce(com, 4), 13419
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
    auto momenta = [&]() -> int {
      if (n == 0) return CUP3D_OK;
      {
        ProfileScope ps("udef_momenta");
        hipLaunchKernelGGL(k_udef_momenta, dim3((unsigned)n), dim3(64), 0, stream(), W.it, W.cm[0], W.cm[1], W.cm[2], W.transvel[0], W.transvel[1], W.transvel[2]);
      }
      CUP3D_HIP(hipGetLastError());
      W.momenta_rows.resize(nb * kUdefMomenta);
      CUP3D_HIP(hipMemcpyAsync(W.momenta_rows.data(), W.momenta.p, W.momenta_rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
      stats_field_download(W.momenta_rows.size() * sizeof(double));
      add_rows_in_slot_order(o.slots, n, W.momenta_rows.data(), kUdefMomenta, kUdefMomenta, W.M);  // 13501-13517
      return CUP3D_OK;
    };
    if ((rc = over_ranks(W.M, kUdefMomenta, momenta(), k))) return rc;  // MPI_Allreduce(M, 13), 13519
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
  for (int k = 0; k < nobst; ++k) {
    cup3d_obstacle_shape &o = shapes[k];
    ShapeWork &W = work[k];
    const size_t nb = (size_t)o.nblocks, np = (size_t)W.first_h[nb];
    if (nb) {
      CUP3D_HIP(hipMemcpyAsync(o.chi, W.chi.p, nb * 512 * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipMemcpyAsync(o.udef, W.udef.p, nb * 1536 * sizeof(double), hipMemcpyDeviceToHost, stream()));
      if (np) {
        CUP3D_HIP(hipMemcpyAsync(o.ijk, W.ijk.p, np * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
        CUP3D_HIP(hipMemcpyAsync(o.dchi, W.dchi.p, np * 3 * sizeof(double), hipMemcpyDeviceToHost, stream()));
        CUP3D_HIP(hipMemcpyAsync(o.delta, W.delta.p, np * sizeof(double), hipMemcpyDeviceToHost, stream()));
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
  }
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return CUP3D_OK;
}

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
    o.slots = std::move(W.slots);
    o.geom = std::move(W.geom);
    o.sdf = std::move(W.sdf);
    o.chi = std::move(W.chi);
    o.udef = std::move(W.udef);
    R->bytes += o.slots.size + o.geom.size + o.sdf.size + o.chi.size + o.udef.size;
  }
  s->retained = R;
  s->bytes += R->bytes;
  return CUP3D_OK;
}

// ==== cup3d_update_obstacles_resident / cup3d_penalization_resident / cup3d_update_tmpv_resident.  UpdateObstacles (13812-13837),
// KernelPenalization + kernelFinalizePenalizationForce (13841-13938) and kernelUpdateTmpV (14948-14979) on the blocks
// cup3d_create_obstacles retained: no chi or udef goes up, one launch per operator whatever the number of obstacles.
// k_fluid_momenta_set: one wavefront per row of the plan; obstacles are independent here (vel is only read).
// k_penalize_set / k_update_tmpv_set: one workgroup per touched slot walks the slot's rows in ascending obstacle order.  A thread owns the
// same two cells of the slot throughout, so obstacle k + 1 sees what obstacle k wrote, and no other workgroup touches the slot: the
// reference's order (obstacles one after the other, 13849-13852 and 15072-15078) without a launch per obstacle.
// The row, its obstacle and the obstacle's arrays are found through the plan's tables: all of them indexed by blockIdx or by values loaded
// through it, i.e. wave-uniform.
namespace cup3d {

struct PlanItems {
  const ObstItems *obst;                  // [N]
  const int32_t *row_obst, *row_block;    // [rows]
  const int32_t *sched_first, *sched_rows;  // [nslots + 1], [rows]
  const double *body;                     // [N][9]: cm, vel, omega
};

// The plan's tables are written before the launch and only read by the kernels.  Read through the constant address space, a load at a
// wave-uniform index is a scalar load whatever the kernel stores in between, and what it returns -- the row, its obstacle, the obstacle's
// array pointers and rigid state -- stays in scalar registers; as plain global loads next to the stores to vel they would be vector
// loads, and every address formed from them a pair of vector registers.
template <class T>
using Constant = const T __attribute__((address_space(4)));
template <class T>
__device__ __forceinline__ Constant<T> *constant(const T *p) {
  return (Constant<T> *)p;
}
static_assert(sizeof(ObstItems) == 4 * sizeof(unsigned long long), "plan_obstacle reads an ObstItems as four 64-bit words");
__device__ __forceinline__ ObstItems plan_obstacle(const PlanItems &pl, int k) {
  Constant<unsigned long long> *w = constant(reinterpret_cast<const unsigned long long *>(pl.obst)) + 4 * (size_t)k;
  return ObstItems{reinterpret_cast<const int32_t *>(w[0]), reinterpret_cast<const double *>(w[1]), reinterpret_cast<const double *>(w[2]),
                   reinterpret_cast<const double *>(w[3])};
}

__global__ void __launch_bounds__(64) k_fluid_momenta_set(PlanItems pl, const double *__restrict__ vel, double lambdt, int implicit,
                                                           double *__restrict__ sums /* [rows][29] */) {
  __shared__ double sm[kMomenta][65];
  const int r = blockIdx.x;
  const int k = constant(pl.row_obst)[r], b = constant(pl.row_block)[r];
  const ObstItems it = plan_obstacle(pl, k);
  Constant<double> *cm = constant(pl.body) + 9 * (size_t)k;
  fluid_momenta_block(it, b, vel, lambdt, implicit, cm[0], cm[1], cm[2], sums + (size_t)r * kMomenta, sm);
}

__global__ void __launch_bounds__(256) k_penalize_set(PlanItems pl, double *__restrict__ vel, const double *__restrict__ chi_field, double dt, double lambdaFac,
                                                       int implicit, double *__restrict__ forces /* [rows][6] */) {
  __shared__ double red[4];
  const int first = constant(pl.sched_first)[blockIdx.x], last = constant(pl.sched_first)[blockIdx.x + 1];
  for (int e = first; e < last; ++e) {  // ascending obstacle index
    const int r = constant(pl.sched_rows)[e];
    const int k = constant(pl.row_obst)[r], i = constant(pl.row_block)[r];
    const ObstItems it = plan_obstacle(pl, k);
    Constant<double> *B = constant(pl.body) + 9 * (size_t)k;
    penalize_block(it, i, vel, chi_field, dt, lambdaFac, implicit, B[0], B[1], B[2], B[3], B[4], B[5], B[6], B[7], B[8], forces + (size_t)r * 6, red);
  }
}

__global__ void __launch_bounds__(256) k_update_tmpv_set(PlanItems pl, double *__restrict__ tmpV, const double *__restrict__ chi_field) {
  const int first = constant(pl.sched_first)[blockIdx.x], last = constant(pl.sched_first)[blockIdx.x + 1];
  for (int e = first; e < last; ++e) {  // ascending obstacle index
    const int r = constant(pl.sched_rows)[e];
    const ObstItems it = plan_obstacle(pl, constant(pl.row_obst)[r]);
    update_tmpv_block(it, constant(pl.row_block)[r], tmpV, chi_field);
  }
}

namespace {

// the retained set of a resident call of `nobst` obstacles, or why there is none
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

// the plan of the retained set, built on first use
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
      items[k] = ObstItems{(const int32_t *)o.slots.p, (const double *)o.geom.p, (const double *)o.chi.p, (const double *)o.udef.p};
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
    if ((rc = P->obst.upload(items.data(), N * sizeof(ObstItems))) || (rc = P->row_obst.upload(row_obst.data(), nr * sizeof(int32_t))) ||
        (rc = P->row_block.upload(row_block.data(), nr * sizeof(int32_t))) || (rc = P->sched_first.upload(sched_first.data(), sched_first.size() * sizeof(int32_t))) ||
        (rc = P->sched_rows.upload(sched_rows.data(), nr * sizeof(int32_t))) || (rc = P->body.alloc(N * 9 * sizeof(double))) ||
        (rc = P->out.alloc(nr * kMomenta * sizeof(double))))
      return rc;
    CUP3D_HIP(hipStreamSynchronize(stream()));  // the tables are locals
    P->bytes = P->obst.size + P->row_obst.size + P->row_block.size + P->sched_first.size + P->sched_rows.size + P->body.size + P->out.size;
  }
  drop.p = nullptr;
  R->plan = P;
  R->bytes += P->bytes;
  s->bytes += P->bytes;
  *out = P;
  return CUP3D_OK;
}

PlanItems plan_items(const ResidentPlan *P) {
  return PlanItems{(const ObstItems *)P->obst.p, (const int32_t *)P->row_obst.p, (const int32_t *)P->row_block.p, (const int32_t *)P->sched_first.p,
                   (const int32_t *)P->sched_rows.p, (const double *)P->body.p};
}

}  // namespace

}  // namespace cup3d

extern "C" int cup3d_update_obstacles_resident(cup3d_sim_t *h, double dt, double lambda, int implicit, int nobst, cup3d_obstacle_body *body,
                                               cup3d_obstacle_motion *motion) {
  if (!h || nobst < 0 || !(dt > 0) || (nobst > 0 && (!body || !motion))) return CUP3D_EINVAL;
  if (nobst == 0) return CUP3D_OK;
  Sim *s = reinterpret_cast<Sim *>(h);
  const int nq = implicit ? kMomenta : kMomentaExplicit;
  const double lambdt = lambda * dt;  // 13664
  // nothing of the caller's is written before every obstacle of the call has passed: the results wait here
  std::vector<MomentaResult> res((size_t)nobst);
  std::vector<double> rows, table;
  DevBuf red;  // the all-reduce operand of this call: M[0..15] | M[16..28], error flag
  if (scalars_cross_ranks(s)) {
    int rc = red.alloc(32 * sizeof(double));
    if (rc) return rc;
  }
  RetainedObstacles *R = nullptr;
  // this rank's rows of every obstacle in one launch; what it gets wrong travels with the first obstacle's all-reduce
  auto local_part = [&]() -> int {
    int rc;
    ResidentPlan *P;
    if ((rc = retained_for(s, "cup3d_update_obstacles_resident", nobst, &R)) || (rc = resident_plan(s, R, &P))) return rc;
    if (P->rows == 0) return CUP3D_OK;
    table.assign(9 * (size_t)nobst, 0.0);
    for (int k = 0; k < nobst; ++k)
      for (int d = 0; d < 3; ++d) table[9 * (size_t)k + d] = body[k].cm[d];
    CUP3D_HIP(hipMemcpyAsync(P->body.p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
    {
      ProfileScope ps("update_obstacles_set");
      hipLaunchKernelGGL(k_fluid_momenta_set, dim3((unsigned)P->rows), dim3(64), 0, stream(), plan_items(P), (const double *)s->vel, lambdt, implicit ? 1 : 0,
                         (double *)P->out.p);
    }
    CUP3D_HIP(hipGetLastError());
    rows.resize((size_t)P->rows * kMomenta);
    CUP3D_HIP(hipMemcpyAsync(rows.data(), P->out.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));
    stats_field_download(rows.size() * sizeof(double));
    return CUP3D_OK;
  };
  const int local = local_part();
  for (int k = 0; k < nobst; ++k) {  // obstacles one after the other, as kernelFinalizeObstacleVel visits them (13739)
    MomentaResult &Q = res[k];
    for (int q = 0; q < kMomenta; ++q) Q.M[q] = 0.0;
    // a rank that holds none of the obstacle's blocks still takes part in the all-reduce with M = 0 (MPI_Allreduce(M, 29), 13783)
    if (!local && R->obst[k].nblocks > 0) {
      Q.rows = rows.data() + (size_t)R->plan->row_base[k] * kMomenta;
      Q.nblocks = R->obst[k].nblocks;
      // kernelFinalizeObstacleVel's loop with one thread (13744-13781): block rows in block (slot) order
      add_rows_in_slot_order(R->obst[k].slots_h.data(), Q.nblocks, Q.rows, kMomenta, nq, Q.M);
    }
    int rc = obstacle_motion_from_sums(s, "cup3d_update_obstacles_resident", k, local, (double *)red.p, implicit, motion[k], Q);
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) write_obstacle_motion(res[k], nq, motion[k], body[k].vel, body[k].omega);
  return CUP3D_OK;
}

extern "C" int cup3d_penalization_resident(cup3d_sim_t *h, double dt, double lambda, int implicit, int nobst, cup3d_obstacle_body *body) {
  if (!h || nobst < 0 || !(dt > 0) || (nobst > 0 && !body)) return CUP3D_EINVAL;
  if (nobst == 0) return CUP3D_OK;
  Sim *s = reinterpret_cast<Sim *>(h);
  const double lambdaFac = implicit ? lambda : 1.0 / dt;  // 13867
  std::vector<double> F, table;
  RetainedObstacles *R = nullptr;
  // every obstacle's blocks in one launch, slot by slot; what this rank gets wrong travels with the first obstacle's all-reduce
  auto local_part = [&]() -> int {
    int rc;
    ResidentPlan *P;
    if ((rc = retained_for(s, "cup3d_penalization_resident", nobst, &R)) || (rc = resident_plan(s, R, &P))) return rc;
    if (P->rows == 0) return CUP3D_OK;
    table.resize(9 * (size_t)nobst);
    for (int k = 0; k < nobst; ++k)
      for (int d = 0; d < 3; ++d) {
        table[9 * (size_t)k + d] = body[k].cm[d];
        table[9 * (size_t)k + 3 + d] = body[k].vel[d];
        table[9 * (size_t)k + 6 + d] = body[k].omega[d];
      }
    CUP3D_HIP(hipMemcpyAsync(P->body.p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
    {
      ProfileScope ps("penalization_set");
      hipLaunchKernelGGL(k_penalize_set, dim3((unsigned)P->nslots), dim3(256), 0, stream(), plan_items(P), s->vel, (const double *)s->chi, dt, lambdaFac,
                         implicit ? 1 : 0, (double *)P->out.p);
    }
    CUP3D_HIP(hipGetLastError());
    F.resize((size_t)P->rows * 6);
    CUP3D_HIP(hipMemcpyAsync(F.data(), P->out.p, F.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));
    stats_field_download(F.size() * sizeof(double));
    return CUP3D_OK;
  };
  const int local = local_part();
  std::vector<double> sums(7 * (size_t)nobst, 0.0);  // the caller's structs are written once every obstacle has passed
  for (int k = 0; k < nobst; ++k) {  // as kernelFinalizePenalizationForce visits them; a rank without blocks of obstacle k adds zeros
    double *M = &sums[7 * (size_t)k];
    if (!local && R->obst[k].nblocks > 0)
      add_rows_in_slot_order(R->obst[k].slots_h.data(), R->obst[k].nblocks, F.data() + (size_t)R->plan->row_base[k] * 6, 6, 6, M);
    int rc = penalization_force_over_ranks(s, "cup3d_penalization_resident", k, local, M);
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) force_from_sums(&sums[7 * (size_t)k], body[k].force, body[k].torque);
  return CUP3D_OK;
}

extern "C" int cup3d_update_tmpv_resident(cup3d_sim_t *h, int nobst) {
  if (!h || nobst < 0) return CUP3D_EINVAL;
  if (nobst == 0) return CUP3D_OK;
  Sim *s = reinterpret_cast<Sim *>(h);
  int rc;
  RetainedObstacles *R;
  ResidentPlan *P;
  if ((rc = retained_for(s, "cup3d_update_tmpv_resident", nobst, &R)) || (rc = resident_plan(s, R, &P))) return rc;
  if (P->rows > 0) {
    ProfileScope ps("update_tmpv_set");
    hipLaunchKernelGGL(k_update_tmpv_set, dim3((unsigned)P->nslots), dim3(256), 0, stream(), plan_items(P), s->tmpV, (const double *)s->chi);
    CUP3D_HIP(hipGetLastError());
  }
  s->udef_nonzero = true;
  return CUP3D_OK;
}

// ==== cup3d_prevent_colliding_obstacles.  Penalization::preventCollidingObstacles (main.cpp:14009-14324): the CollisionInfo sums
// (14037-14142) on the device from the blocks cup3d_create_obstacles retained, the two all-reduces and the pair loop with ComputeJ /
// ElasticCollision (13939-14007, 14143-14323) on the host.
// One wavefront per obstacle i, k_fluid_momenta's pattern.  For j = 0..N-1, j != i, it visits the blocks both obstacles hold in ascending
// slot order (the host intersects the two slot lists and uploads, per ordered pair, the index pairs into the two obstacles' retained
// arrays).  Per z-plane every lane evaluates one cell; a ballot of !(iChi <= 0) && !(jChi <= 0) says which cells the reference visits,
// and a plane without one is skipped.  The selected lanes leave their summands in LDS, then lanes 0..13 each add one of iM, iPos*, ivec*,
// jM, jPos*, jvec* over the plane in cell order onto a running total they keep in a register -- the totals run on across the blocks and
// across j, as `coll` does.  Lanes 14 and 15 scan the plane's imag / jmag in the same order with the reference's strict `>` against
// imagmax / jmagmax, which restart at 0 for every j, and take the momentum of a cell that wins from three further rows; coll.iMom* / jMom*
// persist across j when no later cell beats 0, as written.  No tree, no atomic: the 20 values are the reference's
// one-thread loop bit for bit.  The rows of sm are padded by one double as in k_fluid_momenta.
namespace cup3d {

constexpr int kCollision = 20;  // CollisionInfo, member order of 14015-14034
constexpr int kCollisionRows = 22;  // 14 sums, imag, jmag, iMom[3], jMom[3]

struct CollisionObstacle {
  const double *geom, *sdf, *chi, *udef;  // the retained arrays of this obstacle
  double cm[3], vel[3], omega[3];         // centerOfMass, transVel, angVel
};

struct CollisionItems {
  const CollisionObstacle *obst;  // [N]
  const int32_t *first;           // [N*N+1]: the ordered pair (i, j) owns pairs [first[i*N+j], first[i*N+j+1])
  const int32_t *pairs;           // [.][2]: block index in i's arrays, block index in j's arrays; ascending slot
  int n;
};

// a value every lane of the wavefront holds alike, moved to scalar registers
__device__ __forceinline__ double wave_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
__device__ __forceinline__ const double *wave_uniform(const double *p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const double *)(((unsigned long long)hi << 32) | lo);
}

__global__ void __launch_bounds__(64) k_collision_sums(CollisionItems it, double *__restrict__ sums /* [N][20] */) {
  __shared__ double sm[kCollisionRows][65];
  const int i = blockIdx.x, lane = threadIdx.x;
  const CollisionObstacle *__restrict__ A = it.obst + i;
  const int ix = lane & 7, iy = lane >> 3;
  const double iU0 = wave_uniform(A->vel[0]), iU1 = wave_uniform(A->vel[1]), iU2 = wave_uniform(A->vel[2]);
  const double iomega0 = wave_uniform(A->omega[0]), iomega1 = wave_uniform(A->omega[1]), iomega2 = wave_uniform(A->omega[2]);
  const double iCx = wave_uniform(A->cm[0]), iCy = wave_uniform(A->cm[1]), iCz = wave_uniform(A->cm[2]);
  const double *__restrict__ iGeom = wave_uniform(A->geom), *__restrict__ iSdf = wave_uniform(A->sdf);
  const double *__restrict__ iChi = wave_uniform(A->chi), *__restrict__ iUdef = wave_uniform(A->udef);
  double acc = 0.0;  // lanes 0..13: the running sum of quantity `lane`; lane 14: imagmax, lane 15: jmagmax
  __shared__ double won[2][3];  // coll.iMom*, coll.jMom*: lane 14's and lane 15's own, no other lane touches them
  if (lane == 14 || lane == 15) won[lane - 14][0] = won[lane - 14][1] = won[lane - 14][2] = 0.0;
  const int mrow = 16 + 3 * (lane & 1);  // lane 14 reads the rows of iMom, lane 15 those of jMom
  for (int j = 0; j < it.n; ++j) {
    if (j == i) continue;
    const CollisionObstacle *__restrict__ B = it.obst + j;
    const double jU0 = wave_uniform(B->vel[0]), jU1 = wave_uniform(B->vel[1]), jU2 = wave_uniform(B->vel[2]);
    const double jomega0 = wave_uniform(B->omega[0]), jomega1 = wave_uniform(B->omega[1]), jomega2 = wave_uniform(B->omega[2]);
    const double jCx = wave_uniform(B->cm[0]), jCy = wave_uniform(B->cm[1]), jCz = wave_uniform(B->cm[2]);
    const double *__restrict__ jSdf = wave_uniform(B->sdf), *__restrict__ jChi = wave_uniform(B->chi), *__restrict__ jUdef = wave_uniform(B->udef);
    if (lane >= 14) acc = 0.0;  // imagmax = jmagmax = 0 (14063-14064)
    const int q0 = __builtin_amdgcn_readfirstlane(it.first[i * it.n + j]), q1 = __builtin_amdgcn_readfirstlane(it.first[i * it.n + j + 1]);
    for (int q = q0; q < q1; ++q) {
      const int bi = __builtin_amdgcn_readfirstlane(it.pairs[2 * q]), bj = __builtin_amdgcn_readfirstlane(it.pairs[2 * q + 1]);
      const double h = wave_uniform(iGeom[4 * bi]), ox = wave_uniform(iGeom[4 * bi + 1]), oy = wave_uniform(iGeom[4 * bi + 2]), oz = wave_uniform(iGeom[4 * bi + 3]);
      const double *__restrict__ iSDF = iSdf + (size_t)bi * 1000;
      const double *__restrict__ jSDF = jSdf + (size_t)bj * 1000;
#pragma unroll 1
      for (int iz = 0; iz < 8; ++iz) {
        const int c = iz * 64 + lane;
        const double iX = iChi[(size_t)bi * 512 + c], jX = jChi[(size_t)bj * 512 + c];
        const bool visited = !(iX <= 0.0) && !(jX <= 0.0);  // `if (iChi[z][y][x] <= 0.0 || jChi[z][y][x] <= 0.0) continue;`
        const unsigned long long mask = __ballot(visited);
        if (mask == 0ull) continue;  // the same in every lane
        if (visited) {
          const double p[3] = {ox + h * (ix + 0.5), oy + h * (iy + 0.5), oz + h * (iz + 0.5)};
          sm[0][lane] = 1.0;
          sm[1][lane] = p[0];
          sm[2][lane] = p[1];
          sm[3][lane] = p[2];
          sm[7][lane] = 1.0;
          sm[8][lane] = p[0];
          sm[9][lane] = p[1];
          sm[10][lane] = p[2];
          const double *iU = iUdef + ((size_t)bi * 512 + c) * 3;
          const double iMomX = iU0 + iomega1 * (p[2] - iCz) - iomega2 * (p[1] - iCy) + iU[0];
          const double iMomY = iU1 + iomega2 * (p[0] - iCx) - iomega0 * (p[2] - iCz) + iU[1];
          const double iMomZ = iU2 + iomega0 * (p[1] - iCy) - iomega1 * (p[0] - iCx) + iU[2];
          sm[14][lane] = iMomX * iMomX + iMomY * iMomY + iMomZ * iMomZ;  // imag
          sm[16][lane] = iMomX;
          sm[17][lane] = iMomY;
          sm[18][lane] = iMomZ;
          __builtin_amdgcn_sched_barrier(0);  // one group's loads at a time: 64 registers, eight wavefronts per SIMD
          const double *jU = jUdef + ((size_t)bj * 512 + c) * 3;
          const double jMomX = jU0 + jomega1 * (p[2] - jCz) - jomega2 * (p[1] - jCy) + jU[0];
          const double jMomY = jU1 + jomega2 * (p[0] - jCx) - jomega0 * (p[2] - jCz) + jU[1];
          const double jMomZ = jU2 + jomega0 * (p[1] - jCy) - jomega1 * (p[0] - jCx) + jU[2];
          sm[15][lane] = jMomX * jMomX + jMomY * jMomY + jMomZ * jMomZ;  // jmag
          sm[19][lane] = jMomX;
          sm[20][lane] = jMomY;
          sm[21][lane] = jMomZ;
          __builtin_amdgcn_sched_barrier(0);  // one group's loads at a time: 64 registers, eight wavefronts per SIMD
          const int s0 = ((iz + 1) * 10 + (iy + 1)) * 10 + (ix + 1);  // sdfLab[z+1][y+1][x+1]
          const double ivecX = iSDF[s0 + 1] - iSDF[s0 - 1], ivecY = iSDF[s0 + 10] - iSDF[s0 - 10], ivecZ = iSDF[s0 + 100] - iSDF[s0 - 100];
          const double normi = 1.0 / (sqrt(ivecX * ivecX + ivecY * ivecY + ivecZ * ivecZ) + 1e-21);
          sm[4][lane] = ivecX * normi;
          sm[5][lane] = ivecY * normi;
          sm[6][lane] = ivecZ * normi;
          __builtin_amdgcn_sched_barrier(0);  // one group's loads at a time: 64 registers, eight wavefronts per SIMD
          const double jvecX = jSDF[s0 + 1] - jSDF[s0 - 1], jvecY = jSDF[s0 + 10] - jSDF[s0 - 10], jvecZ = jSDF[s0 + 100] - jSDF[s0 - 100];
          const double normj = 1.0 / (sqrt(jvecX * jvecX + jvecY * jvecY + jvecZ * jvecZ) + 1e-21);
          sm[11][lane] = jvecX * normj;
          sm[12][lane] = jvecY * normj;
          sm[13][lane] = jvecZ * normj;
        }
        __syncthreads();
        if (lane < 16) {
#pragma unroll 1
          for (unsigned long long m = mask; m; m &= m - 1ull) {  // the visited cells in ascending order, i.e. z, y, x
            const int k = __ffsll((long long)m) - 1;
            const double x = sm[lane][k];
            if (lane < 14) {
              acc += x;
            } else if (x > acc) {  // 14120-14125, 14133-14138
              acc = x;
              won[lane - 14][0] = sm[mrow][k];
              won[lane - 14][1] = sm[mrow + 1][k];
              won[lane - 14][2] = sm[mrow + 2][k];
            }
          }
        }
        __syncthreads();
      }
    }
  }
  // lane -> member of CollisionInfo: iM iPos[3] | iMom[3] | ivec[3] jM jPos[3] | jMom[3] | jvec[3]
  double *out = sums + (size_t)i * kCollision;
  if (lane < 4) out[lane] = acc;
  else if (lane < 11) out[lane + 3] = acc;
  else if (lane < 14) out[lane + 6] = acc;
  else if (lane < 16) {
    const int at = lane == 14 ? 4 : 14;
    out[at] = won[lane - 14][0];
    out[at + 1] = won[lane - 14][1];
    out[at + 2] = won[lane - 14][2];
  }
}

namespace {
// ComputeJ (13939-13966)
void compute_j(const double *Rc, const double *R, const double *N, const double *I, double *J) {
  const double m00 = I[0], m01 = I[3], m02 = I[4], m11 = I[1], m12 = I[5], m22 = I[2];
  double a00 = m22 * m11 - m12 * m12;
  double a01 = m02 * m12 - m22 * m01;
  double a02 = m01 * m12 - m02 * m11;
  double a11 = m22 * m00 - m02 * m02;
  double a12 = m01 * m02 - m00 * m12;
  double a22 = m00 * m11 - m01 * m01;
  const double determinant = 1.0 / ((m00 * a00) + (m01 * a01) + (m02 * a02));
  a00 *= determinant;
  a01 *= determinant;
  a02 *= determinant;
  a11 *= determinant;
  a12 *= determinant;
  a22 *= determinant;
  const double aux_0 = (Rc[1] - R[1]) * N[2] - (Rc[2] - R[2]) * N[1];
  const double aux_1 = (Rc[2] - R[2]) * N[0] - (Rc[0] - R[0]) * N[2];
  const double aux_2 = (Rc[0] - R[0]) * N[1] - (Rc[1] - R[1]) * N[0];
  J[0] = a00 * aux_0 + a01 * aux_1 + a02 * aux_2;
  J[1] = a01 * aux_0 + a11 * aux_1 + a12 * aux_2;
  J[2] = a02 * aux_0 + a12 * aux_1 + a22 * aux_2;
}

// ElasticCollision (13967-14007)
void elastic_collision(double m1, double m2, const double *I1, const double *I2, const double *v1, const double *v2, const double *o1, const double *o2,
                       const double *C1, const double *C2, double NX, double NY, double NZ, double CX, double CY, double CZ, const double *vc1,
                       const double *vc2, double *hv1, double *hv2, double *ho1, double *ho2) {
  const double e = 1.0;
  const double N[3] = {NX, NY, NZ};
  const double C[3] = {CX, CY, CZ};
  const double k1[3] = {N[0] / m1, N[1] / m1, N[2] / m1};
  const double k2[3] = {-N[0] / m2, -N[1] / m2, -N[2] / m2};
  double J1[3], J2[3];
  compute_j(C, C1, N, I1, J1);
  compute_j(C, C2, N, I2, J2);
  const double nom = (e + 1) * ((vc1[0] - vc2[0]) * N[0] + (vc1[1] - vc2[1]) * N[1] + (vc1[2] - vc2[2]) * N[2]);
  const double denom = -(1.0 / m1 + 1.0 / m2) +
                       -((J1[1] * (C[2] - C1[2]) - J1[2] * (C[1] - C1[1])) * N[0] + (J1[2] * (C[0] - C1[0]) - J1[0] * (C[2] - C1[2])) * N[1] +
                         (J1[0] * (C[1] - C1[1]) - J1[1] * (C[0] - C1[0])) * N[2]) -
                       ((J2[1] * (C[2] - C2[2]) - J2[2] * (C[1] - C2[1])) * N[0] + (J2[2] * (C[0] - C2[0]) - J2[0] * (C[2] - C2[2])) * N[1] +
                        (J2[0] * (C[1] - C2[1]) - J2[1] * (C[0] - C2[0])) * N[2]);
  const double impulse = nom / (denom + 1e-21);
  for (int d = 0; d < 3; ++d) {
    hv1[d] = v1[d] + k1[d] * impulse;
    hv2[d] = v2[d] + k2[d] * impulse;
    ho1[d] = o1[d] + J1[d] * impulse;
    ho2[d] = o2[d] - J2[d] * impulse;
  }
}
}  // namespace

}  // namespace cup3d

extern "C" int cup3d_prevent_colliding_obstacles(cup3d_sim_t *h, double dt, int nobst, cup3d_obstacle_collision *obst, int32_t *collided, int *ncollided,
                                                 int *any) {
  if (!h || nobst < 0) return CUP3D_EINVAL;
  if (nobst == 0) return dt > 0 ? CUP3D_OK : CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const size_t N = (size_t)nobst;
  const bool cross = scalars_cross_ranks(s);
  std::vector<double> coll(kCollision * N, 0.0);  // collisions[i], then `buffer`
  // what this rank can get wrong travels with the first all-reduce, so that the other ranks are not left inside it
  auto local_part = [&]() -> int {
    if (!(dt > 0) || !obst || !ncollided || !any) { set_error("cup3d_prevent_colliding_obstacles: dt <= 0 or a null argument"); return CUP3D_EINVAL; }
    const RetainedObstacles *R = s->retained;
    if (!R) { set_error("cup3d_prevent_colliding_obstacles: no cup3d_create_obstacles has left its blocks on the device"); return CUP3D_ESTATE; }
    if (R->obst.size() != N) {
      set_error("cup3d_prevent_colliding_obstacles: %d obstacles, but cup3d_create_obstacles left %d", nobst, (int)R->obst.size());
      return CUP3D_ESTATE;
    }
    // per obstacle the positions of its blocks in ascending slot order; per ordered pair (i, j) the blocks both hold
    std::vector<std::vector<int32_t>> order(N);
    for (size_t k = 0; k < N; ++k) {
      const std::vector<int32_t> &sl = R->obst[k].slots_h;
      order[k].resize(sl.size());
      for (size_t b = 0; b < sl.size(); ++b) order[k][b] = (int32_t)b;
      std::stable_sort(order[k].begin(), order[k].end(), [&](int32_t a, int32_t b) { return sl[a] < sl[b]; });
    }
    std::vector<int32_t> first(N * N + 1, 0), pairs;
    for (size_t i = 0; i < N; ++i)
      for (size_t j = 0; j < N; ++j) {
        if (i != j) {
          const std::vector<int32_t> &si = R->obst[i].slots_h, &sj = R->obst[j].slots_h;
          size_t a = 0, b = 0;
          while (a < order[i].size() && b < order[j].size()) {
            const int32_t x = si[order[i][a]], y = sj[order[j][b]];
            if (x < y) ++a;
            else if (y < x) ++b;
            else { pairs.push_back(order[i][a]); pairs.push_back(order[j][b]); ++a; ++b; }
          }
        }
        first[i * N + j + 1] = (int32_t)(pairs.size() / 2);
      }
    std::vector<CollisionObstacle> co(N);
    for (size_t k = 0; k < N; ++k) {
      const RetainedObstacles::One &o = R->obst[k];
      co[k].geom = (const double *)o.geom.p;
      co[k].sdf = (const double *)o.sdf.p;
      co[k].chi = (const double *)o.chi.p;
      co[k].udef = (const double *)o.udef.p;
      for (int d = 0; d < 3; ++d) { co[k].cm[d] = obst[k].cm[d]; co[k].vel[d] = obst[k].vel[d]; co[k].omega[d] = obst[k].omega[d]; }
    }
    DevBuf d_obst, d_first, d_pairs, d_sums;
    int rc;
    if ((rc = d_obst.upload(co.data(), N * sizeof(CollisionObstacle))) || (rc = d_first.upload(first.data(), first.size() * sizeof(int32_t))) ||
        (rc = d_pairs.upload(pairs.data(), pairs.size() * sizeof(int32_t))) || (rc = d_sums.alloc(coll.size() * sizeof(double))))
      return rc;
    const CollisionItems it{(const CollisionObstacle *)d_obst.p, (const int32_t *)d_first.p, (const int32_t *)d_pairs.p, nobst};
    {
      ProfileScope ps("collision_sums");
      hipLaunchKernelGGL(k_collision_sums, dim3((unsigned)N), dim3(64), 0, stream(), it, (double *)d_sums.p);
    }
    CUP3D_HIP(hipGetLastError());
    CUP3D_HIP(hipMemcpyAsync(coll.data(), d_sums.p, coll.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));  // co, first and pairs are locals
    stats_field_download(coll.size() * sizeof(double));
    return CUP3D_OK;
  };
  int rc = local_part();
  if (rc) std::fill(coll.begin(), coll.end(), 0.0);
  // buffermax (14144-14151), MPI_MAX over the ranks (14152); maxi / maxj of 14156-14159 are the same expressions
  std::vector<double> own_max(2 * N), buffermax(2 * N);
  for (size_t i = 0; i < N; ++i) {
    const double *c = &coll[kCollision * i];
    own_max[2 * i] = c[4] * c[4] + c[5] * c[5] + c[6] * c[6];
    own_max[2 * i + 1] = c[14] * c[14] + c[15] * c[15] + c[16] * c[16];
  }
  buffermax = own_max;
  DevBuf red;  // the all-reduce operand of this call
  if (cross) {
    // pieces of at most 16 values, as the in-process communicator of the tests carries them; the flag -- 0, or 1 from a rank whose local
    // part failed -- is the last value of the first piece, so that every rank knows the outcome before the second (as in
    // cup3d_update_obstacles)
    const size_t len = std::max(2 * N + 1, kCollision * N);
    std::vector<double> buf(len, 0.0);
    const size_t head = std::min<size_t>(15, 2 * N);
    for (size_t q = 0; q < head; ++q) buf[q] = buffermax[q];
    buf[head] = rc ? 1.0 : 0.0;
    for (size_t q = head; q < 2 * N; ++q) buf[q + 1] = buffermax[q];
    int rc2;
    if ((rc2 = red.alloc(len * sizeof(double)))) return rc ? rc : rc2;
    double *d = (double *)red.p;
    hipStream_t cs = scalar_stream(s);
    CUP3D_HIP(hipStreamSynchronize(stream()));
    CUP3D_HIP(hipMemcpyAsync(d, buf.data(), (2 * N + 1) * sizeof(double), hipMemcpyHostToDevice, cs));
    if ((rc2 = allreduce(s, d, (int)head + 1, true, cs))) return rc ? rc : rc2;
    CUP3D_HIP(hipMemcpyAsync(buf.data(), d, (head + 1) * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
    if (rc) return rc;
    if (buf[head] != 0.0) {
      set_error("cup3d_prevent_colliding_obstacles: the call failed on another rank");
      return CUP3D_ECOMM;
    }
    for (size_t at = head + 1; at < 2 * N + 1; at += 16)
      if ((rc2 = allreduce(s, d + at, (int)std::min<size_t>(16, 2 * N + 1 - at), true, cs))) return rc2;
    CUP3D_HIP(hipMemcpyAsync(buf.data(), d, (2 * N + 1) * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
    for (size_t q = 0; q < head; ++q) buffermax[q] = buf[q];
    for (size_t q = head; q < 2 * N; ++q) buffermax[q] = buf[q + 1];
  }
  if (rc) return rc;
  for (size_t i = 0; i < N; ++i) {  // 14154-14182
    double *c = &coll[kCollision * i];
    const bool iok = std::fabs(own_max[2 * i] - buffermax[2 * i]) < 1e-10;
    const bool jok = std::fabs(own_max[2 * i + 1] - buffermax[2 * i + 1]) < 1e-10;
    for (int d = 0; d < 3; ++d) {
      c[4 + d] = iok ? c[4 + d] : 0;
      c[14 + d] = jok ? c[14 + d] : 0;
    }
  }
  if (cross) {  // MPI_SUM of 20 N (14183)
    double *d = (double *)red.p;
    hipStream_t cs = scalar_stream(s);
    int rc2;
    CUP3D_HIP(hipMemcpyAsync(d, coll.data(), coll.size() * sizeof(double), hipMemcpyHostToDevice, cs));
    for (size_t at = 0; at < coll.size(); at += 16)
      if ((rc2 = allreduce(s, d + at, (int)std::min<size_t>(16, coll.size() - at), false, cs))) return rc2;
    CUP3D_HIP(hipMemcpyAsync(coll.data(), d, coll.size() * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
  }
  // 14208-14323 with one thread: pairs i < j in order, later pairs see the velocities earlier pairs wrote.  The caller's structs are
  // written only once every pair has passed.
  std::vector<cup3d_obstacle_collision> out(obst, obst + N);
  std::vector<int32_t> ids;
  bool hit = false;
  for (size_t i = 0; i < N; ++i)
    for (size_t j = i + 1; j < N; ++j) {
      cup3d_obstacle_collision &si = out[i], &sj = out[j];
      const double m1 = si.mass, m2 = sj.mass;
      const double v1[3] = {si.vel[0], si.vel[1], si.vel[2]}, o1[3] = {si.omega[0], si.omega[1], si.omega[2]};
      const double v2[3] = {sj.vel[0], sj.vel[1], sj.vel[2]}, o2[3] = {sj.omega[0], sj.omega[1], sj.omega[2]};
      const double *I1 = si.J, *I2 = sj.J, *C1 = si.cm, *C2 = sj.cm;
      const double *c = &coll[kCollision * i], *co = &coll[kCollision * j];
      const double iM = c[0], iPosX = c[1], iPosY = c[2], iPosZ = c[3], iMomX = c[4], iMomY = c[5], iMomZ = c[6], ivecX = c[7], ivecY = c[8], ivecZ = c[9];
      const double jM = c[10], jPosX = c[11], jPosY = c[12], jPosZ = c[13], jMomX = c[14], jMomY = c[15], jMomZ = c[16], jvecX = c[17], jvecY = c[18],
                   jvecZ = c[19];
      const double tolerance = 0.001;
      if (iM < tolerance || jM < tolerance) continue;
      if (co[0] < tolerance || co[10] < tolerance) continue;
      if (std::fabs(iPosX / iM - co[1] / co[0]) > 0.2 || std::fabs(iPosY / iM - co[2] / co[0]) > 0.2 || std::fabs(iPosZ / iM - co[3] / co[0]) > 0.2) continue;
      hit = true;  // sim.bCollision
      ids.push_back((int32_t)i);
      ids.push_back((int32_t)j);
      const double norm_i = std::sqrt(ivecX * ivecX + ivecY * ivecY + ivecZ * ivecZ);
      const double norm_j = std::sqrt(jvecX * jvecX + jvecY * jvecY + jvecZ * jvecZ);
      const double mX = ivecX / norm_i - jvecX / norm_j;
      const double mY = ivecY / norm_i - jvecY / norm_j;
      const double mZ = ivecZ / norm_i - jvecZ / norm_j;
      const double inorm = 1.0 / std::sqrt(mX * mX + mY * mY + mZ * mZ);
      const double NX = mX * inorm, NY = mY * inorm, NZ = mZ * inorm;
      const double projVel = (jMomX - iMomX) * NX + (jMomY - iMomY) * NY + (jMomZ - iMomZ) * NZ;
      if (projVel <= 0) continue;
      const double inv_iM = 1.0 / iM, inv_jM = 1.0 / jM;
      const double iPX = iPosX * inv_iM, iPY = iPosY * inv_iM, iPZ = iPosZ * inv_iM;
      const double jPX = jPosX * inv_jM, jPY = jPosY * inv_jM, jPZ = jPosZ * inv_jM;
      const double CX = 0.5 * (iPX + jPX), CY = 0.5 * (iPY + jPY), CZ = 0.5 * (iPZ + jPZ);
      const double vc1[3] = {iMomX, iMomY, iMomZ}, vc2[3] = {jMomX, jMomY, jMomZ};
      double ho1[3], ho2[3], hv1[3], hv2[3];
      const bool iforced = si.forced[0] || si.forced[1] || si.forced[2];
      const bool jforced = sj.forced[0] || sj.forced[1] || sj.forced[2];
      const double m1_i = iforced ? 1e10 * m1 : m1;
      const double m2_j = jforced ? 1e10 * m2 : m2;
      elastic_collision(m1_i, m2_j, I1, I2, v1, v2, o1, o2, C1, C2, NX, NY, NZ, CX, CY, CZ, vc1, vc2, hv1, hv2, ho1, ho2);
      for (int d = 0; d < 3; ++d) {
        si.vel[d] = si.collision_vel[d] = hv1[d];
        sj.vel[d] = sj.collision_vel[d] = hv2[d];
        si.omega[d] = si.collision_omega[d] = ho1[d];
        sj.omega[d] = sj.collision_omega[d] = ho2[d];
      }
      si.collision_counter = 0.01 * dt;
      sj.collision_counter = 0.01 * dt;
    }
  for (size_t i = 0; i < N; ++i) {
    obst[i] = out[i];
    for (int q = 0; q < kCollision; ++q) obst[i].sums[q] = coll[kCollision * i + q];
  }
  if (collided)
    for (size_t q = 0; q < ids.size(); ++q) collided[q] = ids[q];
  *ncollided = (int)ids.size();
  *any = hit ? 1 : 0;
  return CUP3D_OK;
}
