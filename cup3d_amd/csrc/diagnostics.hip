// Whole-grid sums over the resident fields: cup3d_compute_dissipation -- ComputeDissipation::operator() (main.cpp:10436-10447) with
// KernelDissipation (10347-10434) -- and cup3d_fix_mass_flux -- FixMassFlux::operator() (12218-12248) with avgUx_nonUniform (12199-12216).
//
// Every summand is the reference's expression in the reference's association (-ffp-contract=off).  The ORDER of the sums is the
// library's own, because the reference's is unspecified with more than one OpenMP thread:
//   * a block's sums start at 0.0 and add its 512 cells in iz, iy, ix order;
//   * a rank's totals start at 0.0 and add the block sums in ascending slot order;
//   * ranks combine by the library's SUM all-reduce.
// On a one-block grid that is the reference's one-thread result bit for bit.  No atomics on floating-point data and no tree: the
// summands of 256 cells (four z-planes) go to LDS, one lane per quantity adds them in cell order onto a running total it keeps in a
// register (the idiom of fluid_momenta_block, obstacles_update.hip); the rows of the staging array are padded by one double, a row of
// 256 doubles would put every reader on one LDS bank.  k_rows_total then adds the block rows serially, staged through LDS in chunks
// with the next chunk's loads in flight.
//
// hCube of KernelDissipation is std::pow(h, 3), one rounding where h*h*h has two, so the two need not be the same double (they are not
// at h = 0.3; for the spacings 2 pi / (8 n) they happen to be): it is computed on the host with the reference's own call, once per level,
// and reaches the kernel as a table passed by value.  avgUx_nonUniform does multiply.
//
// Device memory: the block geometry [nb][4] = {h, origin} (GridDev carries only the spacings) and the rows [nb + 1][20] (the last row:
// the totals) are allocated by the FIRST call of either entry point, charged to the sim's ledger and released with the sim.
#include <cmath>

#include "obstacles.hpp"  // sums_over_ranks
#include "tile.hpp"
#include "tile7.hpp"
#include "tile_vector.hpp"

namespace cup3d {

constexpr int kQoi = 20;          // RDX[20], 10439
constexpr int kStaged = 256;      // cells staged at a time: the z-planes [4k, 4k + 4) of a block, one cell per thread
constexpr int kTotalChunk = 1280; // doubles per chunk of k_rows_total: 64 rows of 20, or 1280 rows of 1
constexpr int kMaxLevels = 16;

// std::pow(h, 3) of every spacing the mesh holds
struct LevelCubes {
  double h[kMaxLevels], cube[kMaxLevels];
};

// KernelDissipation::operator() on one block by one workgroup; rows[slot][20]
__global__ void __launch_bounds__(256) k_dissipation(GridDev g, const double *__restrict__ vel, const double *__restrict__ pres, const double *__restrict__ chi,
                                                     const double *__restrict__ halo_v, const double *__restrict__ halo_p, const double *__restrict__ geom,
                                                     LevelCubes lc, double nu, double cx, double cy, double cz, double *__restrict__ rows) {
  __shared__ double tv[3 * kT];
  __shared__ double tp[kT];
  __shared__ double sm[kQoi][kStaged + 1];
  const int slot = block_slot(g);
  if (slot < 0) return;
  load_vector_tile(g, slot, vel, halo_v, tv);
  double pc[2];
  load_scalar_tile(g, slot, pres, halo_p, tp, pc);
  __syncthreads();
  const int t = threadIdx.x;
  int x, y, z0, cell0;
  thread_cells(t, x, y, z0, cell0);  // cell0 = z0*64 + y*8 + x: this thread's place in the cell order of either half
  const double h = geom[4 * slot];
  double hCube = 0.0;
#pragma unroll
  for (int i = 0; i < kMaxLevels; ++i) hCube = lc.h[i] == h ? lc.cube[i] : hCube;
  const double inv2h = .5 / h, invHh = 1 / (h * h);
  const double *U = tv, *V = tv + kT, *W = tv + 2 * kT;
  // the adders: five lanes of every wavefront, one quantity each
  const int q = (t >> 6) * 5 + (t & 63);
  const bool adds = (t & 63) < 5;
  double total = 0.0;
  for (int k = 0; k < 2; ++k) {
    const int z = z0 + 4 * k, b = tix(x, y, z);
    const double L0 = U[b], L1 = V[b], L2 = W[b];
    const double LW0 = U[b - 1], LW1 = V[b - 1], LW2 = W[b - 1], LE0 = U[b + 1], LE1 = V[b + 1], LE2 = W[b + 1];
    const double LS0 = U[b - 10], LS1 = V[b - 10], LS2 = W[b - 10], LN0 = U[b + 10], LN1 = V[b + 10], LN2 = W[b + 10];
    const double LF0 = U[b - kTP], LF1 = V[b - kTP], LF2 = W[b - kTP], LB0 = U[b + kTP], LB1 = V[b + kTP], LB2 = W[b + kTP];
    const double X = chi[(size_t)slot * 512 + k * 256 + cell0];
    const double p0 = geom[4 * slot + 1] + h * (x + 0.5), p1 = geom[4 * slot + 2] + h * (y + 0.5), p2 = geom[4 * slot + 3] + h * (z + 0.5);  // Info::pos, 369-373
    const double PX = p0 - cx, PY = p1 - cy, PZ = p2 - cz;
    const double WX = inv2h * ((LN2 - LS2) - (LB1 - LF1));
    const double WY = inv2h * ((LB0 - LF0) - (LE2 - LW2));
    const double WZ = inv2h * ((LE1 - LW1) - (LN0 - LS0));
    const double dPdx = inv2h * (tp[b + 1] - tp[b - 1]);
    const double dPdy = inv2h * (tp[b + 10] - tp[b - 10]);
    const double dPdz = inv2h * (tp[b + kTP] - tp[b - kTP]);
    const double lapU = invHh * (LE0 + LW0 + LN0 + LS0 + LB0 + LF0 - 6 * L0);
    const double lapV = invHh * (LE1 + LW1 + LN1 + LS1 + LB1 + LF1 - 6 * L1);
    const double lapW = invHh * (LE2 + LW2 + LN2 + LS2 + LB2 + LF2 - 6 * L2);
    const double V1 = lapU * L0 + lapV * L1 + lapW * L2;
    const double D11 = inv2h * (LE0 - LW0);
    const double D22 = inv2h * (LN1 - LS1);
    const double D33 = inv2h * (LB2 - LF2);
    const double D12 = inv2h * (LN0 - LS0 + LE1 - LW1) / 2;
    const double D13 = inv2h * (LB0 - LF0 + LE2 - LW2) / 2;
    const double D23 = inv2h * (LN2 - LS2 + LB1 - LF1) / 2;
    const double V2 = D11 * D11 + D22 * D22 + D33 * D33 + 2 * (D12 * D12 + D13 * D13 + D23 * D23);
    sm[0][cell0] = hCube * WX;
    sm[1][cell0] = hCube * WY;
    sm[2][cell0] = hCube * WZ;
    sm[3][cell0] = hCube / 2 * (PY * WZ - PZ * WY);
    sm[4][cell0] = hCube / 2 * (PZ * WX - PX * WZ);
    sm[5][cell0] = hCube / 2 * (PX * WY - PY * WX);
    sm[6][cell0] = hCube * L0;
    sm[7][cell0] = hCube * L1;
    sm[8][cell0] = hCube * L2;
    sm[9][cell0] = hCube / 3 * (PX * (PY * WY + PZ * WZ) - WX * (PY * PY + PZ * PZ));
    sm[10][cell0] = hCube / 3 * (PY * (PX * WX + PZ * WZ) - WY * (PX * PX + PZ * PZ));
    sm[11][cell0] = hCube / 3 * (PZ * (PX * WX + PY * WY) - WZ * (PX * PX + PY * PY));
    sm[12][cell0] = hCube * (PY * L2 - PZ * L1);
    sm[13][cell0] = hCube * (PZ * L0 - PX * L2);
    sm[14][cell0] = hCube * (PX * L1 - PY * L0);
    sm[15][cell0] = (1 - X) * hCube * (dPdx * L0 + dPdy * L1 + dPdz * L2);  // subtracted: QOI[15] -= ..., 10423
    sm[16][cell0] = (1 - X) * hCube * nu * (V1 + 2 * V2);
    sm[17][cell0] = hCube * (WX * L0 + WY * L1 + WZ * L2);
    sm[18][cell0] = hCube * (L0 * L0 + L1 * L1 + L2 * L2) / 2;
    sm[19][cell0] = hCube * sqrt(WX * WX + WY * WY + WZ * WZ);
    __syncthreads();
    if (adds) {
      if (q == 15)
        for (int j = 0; j < kStaged; ++j) total -= sm[q][j];
      else
        for (int j = 0; j < kStaged; ++j) total += sm[q][j];
    }
    __syncthreads();
  }
  if (adds) rows[(size_t)slot * kQoi + q] = total;
}

// out[w] = the first n rows of `rows` [n][w] added in row order onto 0.0, column by column; w = 20 or 1; one workgroup.  The chunk being
// added sits in LDS, the next one's loads are in flight meanwhile; rows past the end are not added (0.0 + -0.0 is not -0.0).
__global__ void __launch_bounds__(256) k_rows_total(const double *__restrict__ rows, long n, int w, double *__restrict__ out) {
  __shared__ double buf[kTotalChunk];
  const int t = threadIdx.x;
  const long len = n * w;
  const int chunk_rows = kTotalChunk / w;
  double pre[kTotalChunk / 256];
#pragma unroll
  for (int i = 0; i < kTotalChunk / 256; ++i) {
    const long at = t + 256 * i;
    pre[i] = at < len ? rows[at] : 0.0;
  }
  double total = 0.0;
  for (long row0 = 0; row0 < n; row0 += chunk_rows) {
#pragma unroll
    for (int i = 0; i < kTotalChunk / 256; ++i) buf[t + 256 * i] = pre[i];
    __syncthreads();
    const long next = (row0 + chunk_rows) * w;
#pragma unroll
    for (int i = 0; i < kTotalChunk / 256; ++i) {
      const long at = next + t + 256 * i;
      pre[i] = at < len ? rows[at] : 0.0;
    }
    if (t < w) {
      const int cnt = (int)(n - row0 < chunk_rows ? n - row0 : chunk_rows);
      for (int r = 0; r < cnt; ++r) total += buf[r * w + t];
    }
    __syncthreads();
  }
  if (t < w) out[t] = total;
}

// avgUx_nonUniform's inner loops (12207-12212) on one block by one wavefront: sums[slot] = the block's 512 terms (u + uinf[0]) * h3
// added in z, y, x order onto 0.0
__global__ void __launch_bounds__(64) k_mass_flux_sum(const double *__restrict__ vel, const double *__restrict__ geom, double uinf0, double *__restrict__ sums) {
  __shared__ double sm[64];
  const int slot = blockIdx.x, lane = threadIdx.x;
  const double h = geom[4 * slot], h3 = h * h * h;
  double total = 0.0;
  for (int iz = 0; iz < 8; ++iz) {
    sm[lane] = (vel[(size_t)slot * 1536 + iz * 64 + lane] + uinf0) * h3;
    __syncthreads();
    if (lane == 0)
      for (int j = 0; j < 64; ++j) total += sm[j];
    __syncthreads();
  }
  if (lane == 0) sums[slot] = total;
}

// FixMassFlux's update loop (12236-12247): vel.u[0] += 6 * scale * p1 / y_max * (1.0 - p1 / y_max), p1 = the cell centre's y
__global__ void __launch_bounds__(256) k_mass_flux_add(double *__restrict__ vel, const double *__restrict__ geom, double scale, double y_max) {
  const int slot = blockIdx.x;
  const double h = geom[4 * slot], oy = geom[4 * slot + 2];
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int iy = (c >> 3) & 7;
    const double p1 = oy + h * (iy + 0.5);
    const double aux = 6 * scale * p1 / y_max * (1.0 - p1 / y_max);
    vel[(size_t)slot * 1536 + c] += aux;
  }
}

namespace {

// the buffers of both entry points, made by the first call of either
int diag_buffers(Sim *s) {
  if (s->d_diag_geom && s->d_diag_rows) return CUP3D_OK;
  const Grid *g = s->grid;
  const size_t nb = (size_t)s->nb;
  std::vector<double> geom(4 * std::max<size_t>(nb, 1), 0.0);
  for (size_t b = 0; b < nb; ++b) {  // Info::h and Info::origin (main.cpp:1066-1068), as cup3d_grid_tables reports them
    const double h = g->multilevel ? g->hb[b] : g->h;
    geom[4 * b] = h;
    for (int d = 0; d < 3; ++d) geom[4 * b + 1 + d] = g->index[3 * b + d] * kBS * h;
  }
  int rc;
  if (!s->d_diag_geom) {
    if ((rc = s->d_diag_geom.alloc(geom.size(), s))) return rc;
    CUP3D_HIP(hipMemcpy(s->d_diag_geom, geom.data(), geom.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!s->d_diag_rows && (rc = s->d_diag_rows.alloc_zeroed((nb + 1) * kQoi, stream(), s))) return rc;
  return CUP3D_OK;
}

int level_cubes(const Sim *s, LevelCubes *lc) {
  const Grid *g = s->grid;
  int n = 0;
  for (int i = 0; i < kMaxLevels; ++i) lc->h[i] = lc->cube[i] = 0.0;
  for (int64_t b = 0; b < s->nb; ++b) {
    const double h = g->multilevel ? g->hb[b] : g->h;
    int i = 0;
    while (i < n && lc->h[i] != h) ++i;
    if (i < n) continue;
    if (n == kMaxLevels) { set_error("cup3d_compute_dissipation: more than %d distinct spacings", kMaxLevels); return CUP3D_EINVAL; }
    lc->h[n] = h;
    lc->cube[n] = std::pow(h, 3);  // 10362
    ++n;
    if (!g->multilevel) break;
  }
  return CUP3D_OK;
}

// this rank's part of ComputeDissipation: rows and totals on the device, the totals (and the rows, where asked for) on the host
int dissipation_local(Sim *s, double nu, const double extents[3], double *totals, double *block_sums) {
  int rc;
  LevelCubes lc;
  if ((rc = level_cubes(s, &lc)) || (rc = diag_buffers(s))) return rc;
  if (s->nb == 0) return CUP3D_OK;
  const Grid *grid = s->grid;
  // the ghosts of pres are parked behind those of vel in the slab buffer (each uses <= 3*64 doubles per face of 9*64), the way
  // cup3d_pressure_rhs parks the udef slabs
  double *halo_p = s->halo_recv;
  if (grid->multilevel) {
    halo_p = s->halo_recv + (size_t)grid->n_amr_faces() * 3 * 64;
    if ((rc = view_exchange_blocks(s, s->pres, 1, 1))) return rc;  // rank views: pres of the ghost blocks
    if ((rc = amr_fill_ghosts(s, s->pres, 1, 1, halo_p))) return rc;
  } else if (grid->nranks > 1 && grid->n_recv_faces > 0) {
    if ((rc = halo_exchange(s, s->pres, 1, 1))) return rc;
    halo_p = s->halo_recv + (size_t)grid->n_recv_faces * 3 * 64;
    CUP3D_HIP(hipMemcpyAsync(halo_p, s->halo_recv, (size_t)grid->n_recv_faces * 64 * sizeof(double), hipMemcpyDeviceToDevice, stream()));
  } else if (grid->nranks > 1) {
    if ((rc = halo_exchange(s, s->pres, 1, 1))) return rc;  // a collective all the same
  }
  if ((rc = halo_exchange(s, s->vel, 3, 1))) return rc;
  const GridDev g = s->gdev();
  double *rows = s->d_diag_rows, *tot = rows + (size_t)s->nb * kQoi;
  {
    ProfileScope ps("dissipation");
    hipLaunchKernelGGL(k_dissipation, dim3(launch_groups(g)), dim3(256), 0, stream(), g, (const double *)s->vel, (const double *)s->pres, (const double *)s->chi,
                       (const double *)s->halo_recv, (const double *)halo_p, (const double *)s->d_diag_geom, lc, nu, extents[0] / 2, extents[1] / 2, extents[2] / 2, rows);
  }
  CUP3D_HIP(hipGetLastError());
  {
    ProfileScope ps("dissipation_total");
    hipLaunchKernelGGL(k_rows_total, dim3(1), dim3(256), 0, stream(), (const double *)rows, (long)s->nb, kQoi, tot);
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipMemcpyAsync(totals, tot, kQoi * sizeof(double), hipMemcpyDeviceToHost, stream()));
  if (block_sums) CUP3D_HIP(hipMemcpyAsync(block_sums, rows, (size_t)s->nb * kQoi * sizeof(double), hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipStreamSynchronize(stream()));
  stats_field_download((block_sums ? (size_t)s->nb + 1 : 1) * kQoi * sizeof(double));
  return CUP3D_OK;
}

// this rank's part of avgUx_nonUniform: the sum before the division by the volume
int mass_flux_local(Sim *s, double uinf0, double *sum) {
  int rc;
  if ((rc = diag_buffers(s))) return rc;
  if (s->nb == 0) return CUP3D_OK;
  double *sums = s->d_diag_rows, *tot = sums + (size_t)s->nb * kQoi;
  {
    ProfileScope ps("mass_flux_sum");
    hipLaunchKernelGGL(k_mass_flux_sum, dim3((unsigned)s->nb), dim3(64), 0, stream(), (const double *)s->vel, (const double *)s->d_diag_geom, uinf0, sums);
    hipLaunchKernelGGL(k_rows_total, dim3(1), dim3(256), 0, stream(), (const double *)sums, (long)s->nb, 1, tot);
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipMemcpyAsync(sum, tot, sizeof(double), hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return CUP3D_OK;
}

}  // namespace

}  // namespace cup3d

using namespace cup3d;

extern "C" int cup3d_compute_dissipation(cup3d_sim_t *h, double nu, const double extents[3], double qoi[20], double *block_sums) {
  if (!h || !extents || !qoi) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  double RDX[kQoi] = {0.0};  // 10439
  const int local = dissipation_local(s, nu, extents, RDX, block_sums);
  Dev<void> red;  // the all-reduce operand of this call (sums_over_ranks)
  if (scalars_cross_ranks(s)) {
    const int rc = red.alloc((kQoi + 1) * sizeof(double), IfEmpty::eight_bytes);
    if (rc) return rc;
  }
  const int rc = sums_over_ranks(s, red.as<double>(), RDX, kQoi, false, local, "cup3d_compute_dissipation", -1);  // MPI_Allreduce(RDX, 20), 10443
  if (rc) return rc;
  for (int q = 0; q < kQoi; ++q) qoi[q] = RDX[q];
  return CUP3D_OK;
}

extern "C" int cup3d_fix_mass_flux(cup3d_sim_t *h, double umax_forced, double nu, double dt, const double extents[3], const double uinf[3], cup3d_mass_flux *out) {
  if (!h || !extents || !uinf) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const double volume = extents[0] * extents[1] * extents[2];  // 12220
  const double y_max = extents[1];
  const double u_avg = 2.0 / 3.0 * umax_forced;
  double avgUx = 0.;  // 12201
  const int local = mass_flux_local(s, uinf[0], &avgUx);
  double u_avg_msr = avgUx / volume;  // the reference divides before it reduces (12214, 12224)
  Dev<void> red;
  if (scalars_cross_ranks(s)) {
    const int rc = red.alloc(2 * sizeof(double), IfEmpty::eight_bytes);
    if (rc) return rc;
  }
  const int rc = sums_over_ranks(s, red.as<double>(), &u_avg_msr, 1, false, local, "cup3d_fix_mass_flux", -1);  // 12224
  if (rc) return rc;
  const double delta_u = u_avg - u_avg_msr;
  const double reTau = std::sqrt(std::fabs(delta_u / dt)) / nu;
  const double scale = 6 * delta_u;
  if (s->nb > 0) {
    ProfileScope ps("mass_flux_add");
    hipLaunchKernelGGL(k_mass_flux_add, dim3((unsigned)s->nb), dim3(256), 0, stream(), (double *)s->vel, (const double *)s->d_diag_geom, scale, y_max);
    CUP3D_HIP(hipGetLastError());
  }
  if (out) { out->u_avg_msr = u_avg_msr; out->u_avg = u_avg; out->delta_u = delta_u; out->scale = scale; out->re_tau = reTau; }
  return CUP3D_OK;
}
