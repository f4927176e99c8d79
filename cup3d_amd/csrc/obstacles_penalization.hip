// cup3d_penalization / cup3d_update_tmpv and cup3d_penalization_resident / cup3d_update_tmpv_resident.  KernelPenalization
// (main.cpp:13841-13912) + kernelFinalizePenalizationForce (13913-13938) and kernelUpdateTmpV (14948-14979), on the ObstacleBlocks of one
// obstacle the caller stages per call, or on the blocks cup3d_create_obstacles retained: no chi or udef goes up, one launch per operator
// whatever the number of obstacles.
// k_penalize_set / k_update_tmpv_set: one workgroup per touched slot walks the slot's rows in ascending obstacle order.  A thread owns the
// same two cells of the slot throughout, so obstacle k + 1 sees what obstacle k wrote, and no other workgroup touches the slot: the
// reference's order (obstacles one after the other, 13849-13852 and 15072-15078) without a launch per obstacle.
// The row, its obstacle and the obstacle's arrays are found through the plan's tables: all of them indexed by blockIdx or by values loaded
// through it, i.e. wave-uniform.
// Also here: the host helpers every obstacle unit uses (obstacles.hpp).
#include "obstacles.hpp"

namespace cup3d {

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

// ---- the host helpers every obstacle unit uses; what each does is said where it is declared (obstacles.hpp)

int block_geometry(const Sim *s, const int32_t *slots, long n, std::vector<double> &rows) {
  const Grid *g = s->grid;
  rows.resize(4 * (size_t)n);
  for (long i = 0; i < n; ++i) {
    const int32_t b = slots[i];
    if (b < 0 || b >= s->nb) { set_error("obstacle block slot %d out of range", (int)b); return CUP3D_EINVAL; }
    const double h = g->multilevel ? g->hb[b] : g->h;
    rows[4 * i] = h;
    for (int d = 0; d < 3; ++d) rows[4 * i + 1 + d] = g->index[3 * (size_t)b + d] * kBS * h;
  }
  return CUP3D_OK;
}

int stage(const Sim *s, const cup3d_obstacle &o, Dev<void> &slots, Dev<void> &geom, Dev<void> &chi, Dev<void> &udef, ObstItems *it) {
  std::vector<double> gm;
  int rc;
  if ((rc = block_geometry(s, o.slots, o.nblocks, gm)) || (rc = slots.upload(o.slots, o.nblocks * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
      (rc = geom.upload(gm.data(), gm.size() * sizeof(double), stream(), IfEmpty::eight_bytes)) || (rc = chi.upload(o.chi, (size_t)o.nblocks * 512 * sizeof(double), stream(), IfEmpty::eight_bytes)) ||
      (rc = udef.upload(o.udef, (size_t)o.nblocks * 1536 * sizeof(double), stream(), IfEmpty::eight_bytes)))
    return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));  // gm is a local
  it->slots = slots.as<const int32_t>();
  it->geom = geom.as<const double>();
  it->chi = chi.as<const double>();
  it->udef = udef.as<const double>();
  return CUP3D_OK;
}

void add_rows_in_slot_order(const int32_t *slots, long n, const double *rows, int stride, int width, double *total) {
  std::vector<long> order(n);
  for (long i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](long a, long b) { return slots[a] < slots[b]; });
  for (long i : order)
    for (int q = 0; q < width; ++q) total[q] += rows[(size_t)i * stride + q];
}

int sums_over_ranks(Sim *s, double *d, double *v, int n, bool is_max, int local_rc, const char *who, int k) {
  if (!scalars_cross_ranks(s)) return local_rc;
  const int head = std::min(n, kAllreducePiece - 1);  // buf: v[0, head), the flag, v[head, n)
  std::vector<double> buf((size_t)n + 1);
  for (int q = 0; q < n; ++q) buf[q < head ? q : q + 1] = local_rc ? 0.0 : v[q];
  buf[head] = local_rc ? 1.0 : 0.0;
  hipStream_t cs = scalar_stream(s);
  int rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));
  CUP3D_HIP(hipMemcpyAsync(d, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice, cs));
  if ((rc = allreduce(s, d, head + 1, is_max, cs))) return local_rc ? local_rc : rc;
  CUP3D_HIP(hipMemcpyAsync(buf.data(), d, (head + 1) * sizeof(double), hipMemcpyDeviceToHost, cs));
  CUP3D_HIP(hipStreamSynchronize(cs));
  if (local_rc) return local_rc;
  if (buf[head] != 0.0) {
    if (k < 0) set_error("%s: the call failed on another rank", who);
    else set_error("%s: obstacle %d failed on %d other rank(s)", who, k, (int)buf[head]);
    return CUP3D_ECOMM;
  }
  if (n > head) {
    for (int at = head + 1; at < n + 1; at += kAllreducePiece)
      if ((rc = allreduce(s, d + at, std::min(kAllreducePiece, n + 1 - at), is_max, cs))) return rc;
    CUP3D_HIP(hipMemcpyAsync(buf.data() + head + 1, d + head + 1, (n - head) * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
  }
  for (int q = 0; q < n; ++q) v[q] = buf[q < head ? q : q + 1];
  return CUP3D_OK;
}

namespace {
// The host half of kernelFinalizePenalizationForce (13913-13938) that cup3d_penalization and cup3d_penalization_resident share: obstacle
// k's six sums cross the ranks, MPI_Allreduce(M, 6) at 13931, in s->d_red[0, 7) (RedSlot); rc: what this rank's local part returned
int penalization_force_over_ranks(Sim *s, const char *who, int k, int rc, double *M /* [6] */) {
  return sums_over_ranks(s, s->d_red, M, 6, false, rc, who, k);
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
    // NEXT collective with the other ranks' 6-double sum.
    double M[6] = {0, 0, 0, 0, 0, 0};
    auto local_part = [&]() -> int {
      if (o.nblocks <= 0) return CUP3D_OK;
      int rc;
      if (!o.slots || !o.chi || !o.udef) { set_error("cup3d_penalization: obstacle %d has blocks but no slots / chi / udef", k); return CUP3D_EINVAL; }
      Dev<void> slots, geom, chi, udef, forces;
      ObstItems it;
      if ((rc = stage(s, o, slots, geom, chi, udef, &it))) return rc;
      if ((rc = forces.alloc((size_t)o.nblocks * 6 * sizeof(double), IfEmpty::eight_bytes))) return rc;
      {
        ProfileScope ps("penalization");
        hipLaunchKernelGGL(k_penalize, dim3((unsigned)o.nblocks), dim3(256), 0, stream(), it, s->vel, s->chi, dt, lambdaFac, implicit ? 1 : 0, o.cm[0], o.cm[1],
                           o.cm[2], o.vel[0], o.vel[1], o.vel[2], o.omega[0], o.omega[1], o.omega[2], forces.as<double>());
      }
      CUP3D_HIP(hipGetLastError());
      std::vector<double> F((size_t)o.nblocks * 6);
      CUP3D_HIP(hipMemcpyAsync(F.data(), forces.get(), F.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
      // kernelFinalizePenalizationForce (13913-13938): block totals in block (slot) order
      add_rows_in_slot_order(o.slots, o.nblocks, F.data(), 6, 6, M);
      return CUP3D_OK;
    };
    int rc = penalization_force_over_ranks(s, "cup3d_penalization", k, local_part(), M);  // MPI_Allreduce(M, 6), 13931
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
    Dev<void> slots, geom, chi, udef;
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
    CUP3D_HIP(hipMemcpyAsync(P->body.get(), table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
    {
      ProfileScope ps("penalization_set");
      hipLaunchKernelGGL(k_penalize_set, dim3((unsigned)P->nslots), dim3(256), 0, stream(), plan_items(P), s->vel, (const double *)s->chi, dt, lambdaFac,
                         implicit ? 1 : 0, P->out.as<double>());
    }
    CUP3D_HIP(hipGetLastError());
    F.resize((size_t)P->rows * 6);
    CUP3D_HIP(hipMemcpyAsync(F.data(), P->out.get(), F.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));
    stats_field_download(F.size() * sizeof(double));
    return CUP3D_OK;
  };
  const int local = local_part();
  std::vector<double> sums(6 * (size_t)nobst, 0.0);  // the caller's structs are written once every obstacle has passed
  for (int k = 0; k < nobst; ++k) {  // as kernelFinalizePenalizationForce visits them; a rank without blocks of obstacle k adds zeros
    double *M = &sums[6 * (size_t)k];
    if (!local && R->obst[k].nblocks > 0)
      add_rows_in_slot_order(R->obst[k].slots_h.data(), R->obst[k].nblocks, F.data() + (size_t)R->plan->row_base[k] * 6, 6, 6, M);
    int rc = penalization_force_over_ranks(s, "cup3d_penalization_resident", k, local, M);
    if (rc) return rc;
  }
  for (int k = 0; k < nobst; ++k) force_from_sums(&sums[6 * (size_t)k], body[k].force, body[k].torque);
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
