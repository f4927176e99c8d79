// cup3d_update_obstacles / cup3d_update_obstacles_resident.  UpdateObstacles::operator() (main.cpp:13812-13837):
// KernelIntegrateFluidMomenta<0/1>::visit (13637-13734) on the device, kernelFinalizeObstacleVel (13737-13811) and
// Obstacle::computeVelocities (12921-13068) on the host -- on the ObstacleBlocks the caller stages, one obstacle at a time, or on the blocks
// cup3d_create_obstacles retained, all obstacles in one launch (k_fluid_momenta_set: one wavefront per row of the plan; obstacles are
// independent here, vel is only read).
// One wavefront per ObstacleBlock.  The reference adds the cells of a block in iz, iy, ix order and skips those with chi <= 0, and so does
// the kernel: per z-plane (64 cells) every lane evaluates one cell and leaves its summands in LDS, then lanes 0..28 each add one quantity
// over the plane in cell order onto a running total they keep in a register -- only the cells the reference visits (a ballot of the
// wavefront says which), so that a skipped cell is neither read from LDS nor multiplied by zero.  No tree, no atomic: the sums are the
// reference's bit for bit.  The rows of sm are padded by one double: lane q reads sm[q][j], and a row length of 64 doubles would put all
// 29 readers on one LDS bank.
#include "obstacles.hpp"

namespace cup3d {

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

__global__ void __launch_bounds__(64) k_fluid_momenta_set(PlanItems pl, const double *__restrict__ vel, double lambdt, int implicit,
                                                           double *__restrict__ sums /* [rows][29] */) {
  __shared__ double sm[kMomenta][65];
  const int r = blockIdx.x;
  const int k = constant(pl.row_obst)[r], b = constant(pl.row_block)[r];
  const ObstItems it = plan_obstacle(pl, k);
  Constant<double> *cm = constant(pl.body) + 9 * (size_t)k;
  fluid_momenta_block(it, b, vel, lambdt, implicit, cm[0], cm[1], cm[2], sums + (size_t)r * kMomenta, sm);
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
// of kMomenta + 1 doubles where scalars cross ranks.
int obstacle_motion_from_sums(Sim *s, const char *who, int k, int rc, double *red, int implicit, const cup3d_obstacle_motion &mo, MomentaResult &R) {
  double *M = R.M;
  if ((rc = sums_over_ranks(s, red, M, kMomenta, false, rc, who, k))) return rc;  // MPI_Allreduce(M, 29), 13783
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

using namespace cup3d;

extern "C" int cup3d_update_obstacles(cup3d_sim_t *h, double dt, double lambda, int implicit, int nobst, cup3d_obstacle *obst, cup3d_obstacle_motion *motion) {
  if (!h || nobst < 0 || !(dt > 0) || (nobst > 0 && (!obst || !motion))) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const int nq = implicit ? kMomenta : kMomentaExplicit;
  const double lambdt = lambda * dt;  // 13664
  // nothing of the caller's is written before every obstacle of the call has passed: the results wait here
  std::vector<MomentaResult> res((size_t)nobst);
  std::vector<std::vector<double>> rows((size_t)nobst);
  const bool cross = scalars_cross_ranks(s);
  Dev<void> red;  // the all-reduce operand of this call (sums_over_ranks)
  if (cross && nobst > 0) {
    int rc = red.alloc((kMomenta + 1) * sizeof(double), IfEmpty::eight_bytes);
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
      Dev<void> slots, geom, chi, udef, sums;
      ObstItems it;
      if ((rc = stage(s, o, slots, geom, chi, udef, &it))) return rc;
      if ((rc = sums.alloc((size_t)o.nblocks * kMomenta * sizeof(double), IfEmpty::eight_bytes))) return rc;
      {
        ProfileScope ps("update_obstacles");
        hipLaunchKernelGGL(k_fluid_momenta, dim3((unsigned)o.nblocks), dim3(64), 0, stream(), it, (const double *)s->vel, lambdt, implicit ? 1 : 0, o.cm[0], o.cm[1],
                           o.cm[2], sums.as<double>());
      }
      CUP3D_HIP(hipGetLastError());
      rows[k].resize((size_t)o.nblocks * kMomenta);
      CUP3D_HIP(hipMemcpyAsync(rows[k].data(), sums.get(), rows[k].size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
      stats_field_download(rows[k].size() * sizeof(double));
      R.rows = rows[k].data();
      R.nblocks = o.nblocks;
      // kernelFinalizeObstacleVel's loop with one thread (13744-13781): block rows in block (slot) order
      add_rows_in_slot_order(o.slots, o.nblocks, R.rows, kMomenta, nq, M);
      return CUP3D_OK;
    };
    int rc = obstacle_motion_from_sums(s, "cup3d_update_obstacles", k, local_part(), red.as<double>(), implicit, motion[k], R);
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) write_obstacle_motion(res[k], nq, motion[k], obst[k].vel, obst[k].omega);
  return CUP3D_OK;
}

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
  Dev<void> red;  // the all-reduce operand of this call (sums_over_ranks)
  if (scalars_cross_ranks(s)) {
    int rc = red.alloc((kMomenta + 1) * sizeof(double), IfEmpty::eight_bytes);
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
    CUP3D_HIP(hipMemcpyAsync(P->body.get(), table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
    {
      ProfileScope ps("update_obstacles_set");
      hipLaunchKernelGGL(k_fluid_momenta_set, dim3((unsigned)P->rows), dim3(64), 0, stream(), plan_items(P), (const double *)s->vel, lambdt, implicit ? 1 : 0,
                         P->out.as<double>());
    }
    CUP3D_HIP(hipGetLastError());
    rows.resize((size_t)P->rows * kMomenta);
    CUP3D_HIP(hipMemcpyAsync(rows.data(), P->out.get(), rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
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
    int rc = obstacle_motion_from_sums(s, "cup3d_update_obstacles_resident", k, local, red.as<double>(), implicit, motion[k], Q);
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) write_obstacle_motion(res[k], nq, motion[k], body[k].vel, body[k].omega);
  return CUP3D_OK;
}
