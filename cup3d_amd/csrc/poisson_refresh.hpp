// The every-50th iteration, fused.
// Part of poisson.hip's translation unit: included there once, in order; not a stand-alone header.
#pragma once

namespace cup3d {

// ------------------------------------------------------------------ the every-50th iteration, fused (uniform grids, one rank)
// Every 50th iteration the reference recomputes s, z and the true residual through _lhs instead of the recurrences (14465-14481,
// 14516-14538): four block-CG applications, six LHS applications and six pointwise passes -- rounds 1-4 ran them as sixteen launches
// (24 ms at 512^3, 3.4 times per step).  Here the chain is cut where it MUST be cut -- a block's LHS needs its neighbours' values of the
// vector the previous block solve produced -- and nowhere else: four launches of ONE kernel form (k_refresh), each a tile LHS of its input
// (tile_lhs: bit-identical to k_lhs), the pointwise work that consumes the result, and the block CG on it, by the wavefront that owns the
// block; plus the two pointwise updates that precede an LHS of their own output (k_refresh_pointwise), which also leave the block sums
// the mean-constraint row of that LHS needs -- in k_lhs's cell-to-thread mapping and order, so that the totals, and with them every
// vector of the refresh, are BIT-IDENTICAL to the unfused launches ("no_fuse_refresh", tests).  The per-block dot products it also leaves
// behind are NOT what solve() uses: the refresh's sums come from k_dots2 / k_dots7 over the stored vectors (refresh_iteration says why).
//   kRefS:  s = A phat ; shat = M^-1 s                                   (14468-14469)
//   kRefZ:  z = A shat ; q = r - alpha s, qhat = rhat - alpha shat, y = w - alpha z ; q.y, y.y ; zhat = M^-1 z   (14470-14480, 14488)
//   kRefR:  r = b - A x ; rhat = M^-1 r                                   (14519-14523)
//   kRefW:  w = A rhat ; the seven dot products ; what = M^-1 w           (14524-14537, 14548)
enum { kRefS = 0, kRefZ = 1, kRefR = 2, kRefW = 3 };
template <bool FMA, int EV, int KIND>
__global__ void __launch_bounds__(64) k_refresh(GridDev g, Vecs V, double alpha, const double *__restrict__ xnew, double *__restrict__ block_dots, long nb,
                                                double *__restrict__ block_sums, int *__restrict__ iters_out, LhsIn L) {
  __shared__ double P[kTileLds];
  const int slot = block_slot(g);
  if (slot < 0) return;
  const int l = threadIdx.x;
  const double hq = block_h(g, slot), invh = 1 / hq;
  const size_t bo = (size_t)slot * 512;
  const double *const tin = KIND == kRefS ? V.v[PHAT] : (KIND == kRefZ ? V.v[SHAT] : (KIND == kRefR ? xnew : V.v[RHAT]));
  double *const out = KIND == kRefS ? V.v[SHAT] : (KIND == kRefZ ? V.v[ZHAT] : (KIND == kRefR ? V.v[RHAT] : V.v[WHAT]));
  const LhsFix fx = lhs_fix(L, nullptr, slot, l, hq);  // (no flag to wait for: the total of the input was complete before the launch)
  const TileIdx ix = tile_idx(l);
  TileRegs tr;
  tile_issue_own(slot, tin, l, tr);
  tile_issue_faces(g, slot, tin, L.halo, l, tr);
  tile_commit(tr, P, l);
  double r[8], acc[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int zz = 0; zz < 8; ++zz) {
    const size_t j = bo + zz * 64 + l;
    double cc;
    const double lhs = zz == 0 ? tile_lhs<0>(P, ix, cc, hq, fx) : tile_lhs<1>(P + (zz - 1) * kTilePitch, ix, cc, hq, fx);
    if constexpr (KIND == kRefS) {
      NTS(V.v[S_], j, lhs);
      r[zz] = invh * lhs;
    } else if constexpr (KIND == kRefZ) {
      const double sv = NTL(V.v[S_], j), w = NTL(V.v[W_], j);
      const double q = NTL(V.v[R_], j) - alpha * sv;
      const double qhat = NTL(V.v[RHAT], j) - alpha * cc;   // cc = shat of this cell (the tile's centre)
      const double y = w - alpha * lhs;
      NTS(V.v[Z_], j, lhs); NTS(V.v[Q_], j, q); NTS(V.v[QHAT], j, qhat); NTS(V.v[Y_], j, y);
      acc[0] += q * y;
      acc[1] += y * y;
      r[zz] = invh * lhs;
    } else if constexpr (KIND == kRefR) {
      const double rv = NTL(V.v[B_], j) - lhs;
      NTS(V.v[R_], j, rv);
      r[zz] = invh * rv;
    } else {
      const double r0 = NTL(V.v[R0], j), rv = NTL(V.v[R_], j);
      NTS(V.v[W_], j, lhs);
      acc[0] += r0 * rv;
      acc[1] += r0 * lhs;
      acc[2] += r0 * NTL(V.v[S_], j);
      acc[3] += r0 * NTL(V.v[Z_], j);
      acc[4] += rv * rv;   // norm_1
      acc[5] += r0 * r0;   // norm_2
      r[zz] = invh * lhs;
    }
  }
  if constexpr (KIND == kRefZ) {
    const double d0 = wave_sum(acc[0]), d1 = wave_sum(acc[1]);
    if (l == 0) { block_dots[slot] = d0; block_dots[nb + slot] = d1; }
  } else if constexpr (KIND == kRefW) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double t = wave_sum(acc[i]);
      if (l == 0) block_dots[(size_t)i * nb + slot] = t;
      if (i == 4 && l == 0) block_dots[(size_t)6 * nb + slot] = t;  // norm = the same sum as norm_1
    }
  }
  __syncthreads();  // the tile is read no more: the block solve takes over its LDS
  cg_block<FMA, false, EV>(g, slot, r, out, block_sums, 0.0, 0.0, iters_out, P);
}
typedef void (*RefreshKernel)(GridDev, Vecs, double, const double *, double *, long, double *, int *, LhsIn);
template <bool FMA, int EV>
static RefreshKernel refresh_kernel_of(int kind) {
  static const RefreshKernel table[4] = {k_refresh<FMA, EV, kRefS>, k_refresh<FMA, EV, kRefZ>, k_refresh<FMA, EV, kRefR>, k_refresh<FMA, EV, kRefW>};
  return table[kind];
}
// block_solver 0: the production block CG; 2: the reference's association
static RefreshKernel refresh_kernel(int block_solver, int kind) { return block_solver == 0 ? refresh_kernel_of<true, kCgProduction>(kind) : refresh_kernel_of<false, 0>(kind); }
// the two pointwise updates whose OUTPUT the next kernel applies the LHS to -- WHICH 0: phat = rhat + beta (phat - omega shat) (14467),
// WHICH 1: x = x + alpha phat + omega qhat (14518) -- with the block sums of that output for the mean-constraint row: one workgroup per
// block, k_lhs's cell-to-thread mapping and its sum (stencil.hip), so that the total is the one launch_lhs would have formed
template <int WHICH>
__global__ void __launch_bounds__(256) k_refresh_pointwise(GridDev g, Vecs V, double a, double b, double *__restrict__ block_sums) {
  __shared__ double red[4];
  const int slot = block_slot(g);
  if (slot < 0) return;
  int x, y, z0, cell0;
  thread_cells(threadIdx.x, x, y, z0, cell0);
  double c[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const size_t j = (size_t)slot * 512 + k * 256 + cell0;
    if constexpr (WHICH == 0) c[k] = V.v[RHAT][j] + a * (V.v[PHAT][j] - b * V.v[SHAT][j]);
    else c[k] = V.xin[j] + a * V.v[PHAT][j] + b * V.v[QHAT][j];
    (WHICH == 0 ? V.v[PHAT] : V.v[X_])[j] = c[k];
  }
  if (block_sums) {
    const double h = block_h(g, slot), h3 = h * h * h;
    const double sum = group_sum<4>(c[0] * h3 + c[1] * h3, red);
    if (threadIdx.x == 0) block_sums[slot] = sum;
  }
}

}  // namespace cup3d
