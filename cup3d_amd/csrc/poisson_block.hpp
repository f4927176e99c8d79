// The block solves (block CG, two blocks per wavefront, direct solve) and their launchers.
// Part of poisson.hip's translation unit: included there once, in order; not a stand-alone header.
#pragma once

namespace cup3d {

// ------------------------------------------------------------------ block-local CG
// One wavefront per 8^3 block: lane = (x,y) column, the 8 z-values of r, p, x, Ap in
// registers; z-neighbours come from registers, x/y-neighbours from an LDS copy of p with
// zero rows above and below (the zero Dirichlet halo of the reference's PaddedBlock).
// Two wave reductions per CG iteration (p.Ap and r.r).
// FMA = contract a*b+c where the reference has a separate multiply and add: the production
// launch (block_solver 0); block_solver 2 keeps the reference's association (see launch_precond).
template <bool FMA>
__device__ __forceinline__ double mad(double a, double b, double c) {
  if constexpr (FMA) return __builtin_fma(a, b, c);
  else return a * b + c;
}
// p <- beta p + r written so that the result lands in p's own registers: the compiler turns __builtin_fma(beta, p, r) into the
// two-operand v_fmac_f64 (destination tied to the addend r), which costs a copy of r before and a register rotation after --
// 2 extra moves per cell and iteration in an issue-bound loop.  The three-operand v_fma_f64 has no such tie.
template <bool FMA>
__device__ __forceinline__ double p_update(double beta, double p, double r) {
  if constexpr (!FMA) return beta * p + r;
  double o;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(o) : "v"(beta), "v"(p), "v"(r));
  return o;
}
// LDS layout: [z][row = y + 1 (rows 0 and 9 stay zero)][x], pitch 8 doubles and NO x halo.  With the 10x10-pitched tile of the
// first version half of all LDS cycles were bank conflicts (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.50, and the waves
// spent 35 % of their cycles in SQ_WAIT_INST_LDS: profiles/r01/pmc_block_preconditioner_sq.txt): a 64-bit access is served 32
// lanes at a time, and four 8-wide rows at pitch 10 overlap in banks, while at pitch 8 the four rows tile the 32 bank pairs
// exactly.  The x-1 / x+1 reads of the lanes at x = 0 / 7, which would fetch a cell of the neighbouring row, go to the zero row.
// HELM: diffusion_kernels::getZImplParallel (main.cpp:10534-10579) -- the same block CG with centre coefficient
// -6 - h^2/nu/dt (10570) instead of -6, for the Helmholtz solves of the implicit diffusion.
// V2 (production): the same iteration with three changes that only touch HOW it is evaluated.  The r01 kernel (V2 = false, kept
// for A/B timing and as the reference-association variant) issued 181 VALU instructions per CG iteration per wavefront, 86 of them
// the stencil and the updates; the SIMD's FP64 issue slots (4 cycles per wave64 instruction) AND the CU's LDS pipe (ds_read2_b64 is
// serviced at half the ds_read_b64 rate, MI355X_MICROARCH.md LDS table) were both ~90 % busy, so only fewer instructions help:
//  * the two wave-wide sums go to the otherwise idle FP64 MATRIX pipe: v_mfma_f64_16x16x4_f64 with B = ones sums the lanes
//    {i, i+16, i+32, i+48}; every lane then holds four of the sixteen partial sums, adds them (3 v_add_f64) and a second MFMA
//    leaves the wavefront total in every lane: 3 VALU instructions instead of 12 DPP moves + 6 adds + 2 readlanes + hazard nops
//    per reduction (this is a cross-lane reduction on an idle pipe, not a reformulation of the stencil as a GEMM);
//  * the x/y-neighbour reads are volatile so that the compiler keeps them as 32 ds_read_b64 (2 LDS cycles each) with the z-plane
//    offset in the instruction instead of 16 ds_read2_b64 (8 cycles each) + per-plane address arithmetic;
//  * rr / (a2 + 1e-55) and ss / (rr + 1e-55) use v_rcp_f64 + two Newton steps + one residual correction (8 instructions, result
//    within 1 ulp of the IEEE quotient) instead of the 12-instruction IEEE expansion -- FMA variant only.
typedef double double4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double wave_sum_mfma(double v) {
  const double4_t zero = {0.0, 0.0, 0.0, 0.0};
  double4_t d = __builtin_amdgcn_mfma_f64_16x16x4f64(v, 1.0, zero, 0, 0, 0);  // D[i][j] = sum_k A[i][k]: lanes i, i+16, i+32, i+48
  const double t = (d[0] + d[1]) + (d[2] + d[3]);                              // the four rows of D this lane holds
  d = __builtin_amdgcn_mfma_f64_16x16x4f64(t, 1.0, zero, 0, 0, 0);            // the four 16-lane rows hold disjoint quarters of the rows of D
  return d[0];
}
__device__ __forceinline__ double fast_div(double n, double d) {
  double y = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, y, 1.0);
  y = __builtin_fma(y, e, y);
  e = __builtin_fma(-d, y, 1.0);
  y = __builtin_fma(y, e, y);
  const double q = n * y;
  return __builtin_fma(__builtin_fma(-d, q, n), y, q);
}
// LDS of one block CG: the padded copy of p ([z][10 rows][8], see below) + 8 doubles nobody reads or writes (the footprint the kernels
// have been measured with)
constexpr int kCgLds = 8 * 80 + 8;
template <bool MFMA>
__device__ __forceinline__ double cg_sum(double v) {
  if constexpr (MFMA) return wave_sum_mfma(v);
  else return wave_sum(v);
}
template <bool FAST>
__device__ __forceinline__ double cg_div(double n, double d) {
  if constexpr (FAST) return fast_div(n, d);
  else return n / d;
}

// EV = how the iteration is evaluated, a bit set: 1 = wave sums on the matrix pipe, 2 = single-width volatile LDS reads,
// 4 = reciprocal divisions (FMA variants only), 8 = three-operand FMA for the p update (p_update above); 0 ... 15
// cg_block: the iteration itself, entered with r = the block's right-hand side / h already in registers (lane = (x, y), 8 z per lane) --
// shared by the stand-alone preconditioner kernel and the kernels that produce that right-hand side on the fly (k_loop1_cg / k_loop2_cg)
// AG: the block sum is handed to another wavefront of the SAME launch (Arrive, below): agent-scope store instead of an ordinary one
template <bool FMA, bool HELM, int EV, bool AG = false>
__device__ __forceinline__ void cg_block(const GridDev &g, int slot, double (&r)[8], double *out, double *__restrict__ block_sums, double nu, double dt,
                                         int *__restrict__ iters_out, double *P) {
  // (r01 kernel: 86 VGPRs -> 5 waves/SIMD.  Forcing 6 with amdgpu_waves_per_eu spills five values that are reloaded every iteration:
  //  0.476 vs 0.431 ms at 256^3, so the natural allocation stays.)
  static_assert(EV >= 0 && EV < 16, "EV is a set of the four bits above");
  constexpr bool V2 = (EV & 1) != 0, LDSV = (EV & 2) != 0, FDIV = (EV & 4) != 0 && FMA;
  const int l = threadIdx.x;
  const int base = ((l >> 3) + 1) * 8 + (l & 7);
  for (int i = l; i < 640; i += 64) P[i] = 0.0;
  // x-1 / x+1 reads of the edge lanes are redirected to the zero row of the same plane, at the one bank the other lanes of the
  // half-wave leave free (address 7 for x = 0, address 0 for x = 7): still conflict-free, and no masking arithmetic
  const int am = (l & 7) == 0 ? 7 : base - 1, ap = (l & 7) == 7 ? 0 : base + 1;
  // V2: volatile LDS pointers (address space kept, or the loads become flat): one ds_read_b64 per access, plane offset immediate
  typedef const volatile __attribute__((address_space(3))) double lds_cvd;
  lds_cvd *Pam = (lds_cvd *)(P + am), *Pap = (lds_cvd *)(P + ap), *Pym = (lds_cvd *)(P + base - 8), *Pyp = (lds_cvd *)(P + base + 8);
  double centre = -6.0;
  if constexpr (HELM) { const double hq = block_h(g, slot); centre = -6.0 - hq * hq / nu / dt; }
  double p[8], x[8], Ax[8];
  double rr = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    rr = mad<FMA>(r[z], r[z], rr);
    p[z] = r[z];
    x[z] = 0;
  }
  rr = cg_sum<V2>(rr);
  const double kRel = 1e-7 * 1e-7, kAbs = 1e-16 * 1e-16;  // kSqrNorm{Rel,Abs}Criterion, 14619-14624
  const double sqrNorm0 = (double)1 / (512 * 512) * rr;    // 14734
  int kdone = 0;
  if (sqrNorm0 >= 1e-32) {                                  // else: block stays 0 (14735-14736)
    __syncthreads();
    auto iteration = [&](int k) -> bool {                     // one trip of the loop at 14739; false = leave it
      kdone = k + 1;
#pragma unroll
      for (int z = 0; z < 8; ++z) P[z * 80 + base] = p[z];
      __syncthreads();
      double a2 = 0;
#pragma unroll
      for (int z = 0; z < 8; ++z) {                         // kernelPoissonGetZInner, 14662-14682
        double t;
        if constexpr (LDSV) {
          t = mad<FMA>(centre, p[z], Pam[z * 80] + Pap[z * 80]);
          t += Pym[z * 80];
          t += Pyp[z * 80];
        } else {
          t = mad<FMA>(centre, p[z], P[z * 80 + am] + P[z * 80 + ap]);
          t += P[z * 80 + base - 8];
          t += P[z * 80 + base + 8];
        }
        t += z > 0 ? p[z - 1] : 0.0;
        t += z < 7 ? p[z + 1] : 0.0;
        Ax[z] = t;
        a2 = mad<FMA>(p[z], t, a2);
      }
      __syncthreads();
      a2 = cg_sum<V2>(a2);
      const double a = cg_div<FDIV>(rr, a2 + 1e-55);        // 14684
      double ss = 0;
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        x[z] = mad<FMA>(a, p[z], x[z]);                     // 14688
        r[z] = mad<FMA>(-a, Ax[z], r[z]);                   // subAndSumSqr, 14636-14638
        ss = mad<FMA>(r[z], r[z], ss);
      }
      ss = cg_sum<V2>(ss);
      const double beta = cg_div<FDIV>(ss, rr + 1e-55);       // 14690
      const double sqrNorm = (double)1 / (512 * 512) * ss;  // 14691
      if (sqrNorm < kRel * sqrNorm0 || sqrNorm < kAbs) return false;  // 14692-14694 (returns -1)
#pragma unroll
      for (int z = 0; z < 8; ++z) p[z] = (EV & 8) ? p_update<FMA>(beta, p[z], r[z]) : mad<FMA>(beta, p[z], r[z]);   // 14698-14699
      rr = ss;
      if (rr <= 0) return false;                                   // 14741
      return true;
    };
    // (two iterations per trip, to pay the register rotation of p at the back edge -- 8 v_mov_b64 -- every other iteration, costs
    //  101-119 registers instead of 88-94: below 5 wavefronts per SIMD, not kept)
    for (int k = 0; k < 100; ++k)
      if (!iteration(k)) break;
  }
  double sx = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    out[(size_t)slot * 512 + z * 64 + l] = x[z];
    sx += x[z];
  }
  if (iters_out && l == 0) iters_out[slot] = kdone;  // measurement only (cup3d_profile_enable): CG iterations this block took
  if (block_sums) {  // sum(z*h^3) of this block for the mean constraint of the LHS that follows (9283-9294)
    const double hq = block_h(g, slot), h3 = hq * hq * hq;
    sx = cg_sum<V2>(sx * h3);
    if (l == 0) { if constexpr (AG) st_agent(block_sums + slot, sx); else block_sums[slot] = sx; }
  }
}

template <bool FMA, bool HELM = false, int EV = 0>
__global__ void __launch_bounds__(64) k_precond(GridDev g, const double *in, double *out, double *__restrict__ block_sums, double nu, double dt,
                                                int *__restrict__ iters_out) {
  __shared__ double P[kCgLds];
  const int slot = block_slot(g);
  if (slot < 0) return;
  const double invh = 1 / block_h(g, slot);  // main.cpp:14723
  double r[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) r[z] = invh * in[(size_t)slot * 512 + z * 64 + threadIdx.x];
  cg_block<FMA, HELM, EV>(g, slot, r, out, block_sums, nu, dt, iters_out, P);
}

#ifdef CUP3D_TESTING
// ------------------------------------------------------------------ block CG, two blocks per wavefront
// The full-wave kernel above spends more than half of its FP64 issue slots on work that does not scale with the cells: two
// wave-wide sums (12 DPP moves + 6 adds + read-lanes + hazard nops each), two divisions, loop control.  Here a HALF-wave owns a
// block -- lane = (x, y pair), 16 cells per lane -- so one instruction stream serves two blocks and that overhead is shared:
//   * sums over 32 lanes: four DPP steps inside the 16-lane rows, then v_permlane16_swap (gfx950) exchanges the two rows of each
//     half, and every lane of a half holds its block's total (no read-lane, no select);
//   * the y-neighbour of row 2j is row 2j+1 of the same lane and vice versa: 3 LDS reads per cell instead of 4;
//   * LDS rows are stored in the order 0,2,4,6,8 | -1,1,3,5,7 (pitch 8, no x halo): the four rows a half-wave touches in any of its
//     six reads / two writes always fall into four different 8-bank groups, and the x-1 / x+1 reads of the edge lanes go to one
//     zero cell at the bank the others leave free -- every DS access is conflict-free and single-width;
//   * a block that has converged (or is skipped, 14735) just stops updating x and r (its half is masked); the wave leaves the loop
//     when both are done.  Block i of the pair runs exactly the iteration the full-wave kernel runs; only the order of the 512-term
//     sums differs (16 per lane, then the lane tree).
__device__ __forceinline__ double half_sum(double v) {
  v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);  // row_half_mirror
  v += dpp_move<0x140>(v);  // row_mirror: every lane of a 16-lane row holds the row total
  const long long b = __builtin_bit_cast(long long, v);
  const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
  const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);  // rows 0<->1 and 2<->3
  const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const double a = __builtin_bit_cast(double, ((long long)rh[0] << 32) | (long long)rl[0]);
  const double c = __builtin_bit_cast(double, ((long long)rh[1] << 32) | (long long)rl[1]);
  return a + c;
}

template <bool FMA, bool HELM = false>
__global__ void __launch_bounds__(64) k_precond_pair(GridDev g, int pchunk, const double *in, double *out, double *__restrict__ block_sums, double nu, double dt,
                                                     int *__restrict__ iters_out) {
  __shared__ double P[2 * 8 * 80];
  typedef const volatile __attribute__((address_space(3))) double lds_cvd;
  const int l = threadIdx.x, half = l >> 5, li = l & 31, x = li & 7, yp = li >> 3;
  const int pi = ((int)blockIdx.x & 7) * pchunk + ((int)blockIdx.x >> 3);  // XCD-aware, as block_slot()
  const int bi = 2 * pi + half;
  const bool have = bi < g.nblocks;
  const int slot = have ? (g.list ? g.list[bi] : bi) : 0;
  for (int i = l; i < 1280; i += 64) P[i] = 0.0;
  double *Pb = P + half * 640;
  // row slots: even rows 0,2,4,6,8 -> 0..4, odd rows -1,1,3,5,7 -> 5..9; slots 4 (row 8) and 5 (row -1) stay zero
  const int s0 = yp, s1 = 6 + yp;                       // own rows y0 = 2 yp, y1 = 2 yp + 1
  double *W0 = Pb + s0 * 8 + x, *W1 = Pb + s1 * 8 + x;  // writes
  lds_cvd *Xm0 = (lds_cvd *)(Pb + (x == 0 ? 47 : s0 * 8 + x - 1)), *Xp0 = (lds_cvd *)(Pb + (x == 7 ? 40 : s0 * 8 + x + 1));
  lds_cvd *Xm1 = (lds_cvd *)(Pb + (x == 0 ? 47 : s1 * 8 + x - 1)), *Xp1 = (lds_cvd *)(Pb + (x == 7 ? 40 : s1 * 8 + x + 1));
  lds_cvd *Ym0 = (lds_cvd *)(Pb + (5 + yp) * 8 + x);    // row y0 - 1
  lds_cvd *Yp1 = (lds_cvd *)(Pb + (yp + 1) * 8 + x);    // row y1 + 1
  const double hq = block_h(g, slot), invh = 1 / hq;     // main.cpp:14723
  double centre = -6.0;
  if constexpr (HELM) centre = -6.0 - hq * hq / nu / dt;
  const size_t o0 = (size_t)slot * 512 + (2 * yp) * 8 + x;  // cell (x, y0, z = 0); y1: + 8; z: + 64
  double r0[8], r1[8], p0[8], p1[8], x0[8], x1[8], A0[8], A1[8];
  double rr = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    r0[z] = have ? invh * in[o0 + z * 64] : 0.0;
    r1[z] = have ? invh * in[o0 + z * 64 + 8] : 0.0;
    rr = mad<FMA>(r0[z], r0[z], rr);
    rr = mad<FMA>(r1[z], r1[z], rr);
    p0[z] = r0[z]; p1[z] = r1[z];
    x0[z] = 0; x1[z] = 0;
  }
  rr = half_sum(rr);
  const double kRel = 1e-7 * 1e-7, kAbs = 1e-16 * 1e-16;  // kSqrNorm{Rel,Abs}Criterion, 14619-14624
  const double sqrNorm0 = (double)1 / (512 * 512) * rr;    // 14734
  bool active = have && sqrNorm0 >= 1e-32;                  // else: block stays 0 (14735-14736)
  int kdone = 0;
  __syncthreads();
  for (int k = 0; k < 100; ++k) {                           // 14739
    if (!__any(active)) break;
    if (active) kdone = k + 1;
#pragma unroll
    for (int z = 0; z < 8; ++z) { W0[z * 80] = p0[z]; W1[z * 80] = p1[z]; }
    __syncthreads();
    double a2 = 0;
#pragma unroll
    for (int z = 0; z < 8; ++z) {                           // kernelPoissonGetZInner, 14662-14682
      double t = mad<FMA>(centre, p0[z], Xm0[z * 80] + Xp0[z * 80]);
      t += Ym0[z * 80];
      t += p1[z];
      t += z > 0 ? p0[z - 1] : 0.0;
      t += z < 7 ? p0[z + 1] : 0.0;
      A0[z] = t;
      a2 = mad<FMA>(p0[z], t, a2);
      double u = mad<FMA>(centre, p1[z], Xm1[z * 80] + Xp1[z * 80]);
      u += p0[z];
      u += Yp1[z * 80];
      u += z > 0 ? p1[z - 1] : 0.0;
      u += z < 7 ? p1[z + 1] : 0.0;
      A1[z] = u;
      a2 = mad<FMA>(p1[z], u, a2);
    }
    __syncthreads();
    a2 = half_sum(a2);
    const double a = cg_div<FMA>(rr, a2 + 1e-55);           // 14684
    double ss = 0;
    if (active) {
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        x0[z] = mad<FMA>(a, p0[z], x0[z]);                  // 14688
        x1[z] = mad<FMA>(a, p1[z], x1[z]);
        r0[z] = mad<FMA>(-a, A0[z], r0[z]);                 // subAndSumSqr, 14636-14638
        r1[z] = mad<FMA>(-a, A1[z], r1[z]);
      }
    }
#pragma unroll
    for (int z = 0; z < 8; ++z) { ss = mad<FMA>(r0[z], r0[z], ss); ss = mad<FMA>(r1[z], r1[z], ss); }
    ss = half_sum(ss);
    const double beta = cg_div<FMA>(ss, rr + 1e-55);        // 14690
    const double sqrNorm = (double)1 / (512 * 512) * ss;    // 14691
    if (sqrNorm < kRel * sqrNorm0 || sqrNorm < kAbs) active = false;  // 14692-14694: this block is done
#pragma unroll
    for (int z = 0; z < 8; ++z) { p0[z] = p_update<FMA>(beta, p0[z], r0[z]); p1[z] = p_update<FMA>(beta, p1[z], r1[z]); }  // 14698-14699
    rr = ss;
    if (rr <= 0) active = false;                            // 14741
  }
  if (!have) return;
  double sx = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    out[o0 + z * 64] = x0[z];
    out[o0 + z * 64 + 8] = x1[z];
    sx += x0[z];
    sx += x1[z];
  }
  if (iters_out && li == 0) iters_out[slot] = kdone;
  if (block_sums) {  // sum(z*h^3) of this block for the mean constraint of the LHS that follows (9283-9294)
    sx = half_sum(sx * (hq * hq * hq));
    if (li == 0) block_sums[slot] = sx;
  }
}

#endif  // CUP3D_TESTING

// ------------------------------------------------------------------ direct block solve
// The block preconditioner M^-1 is "solve sum6(z) - 6z = r/h on one 8^3 block with zero
// ghosts".  The reference evaluates it by CG to a 1e-7 relative residual (14704-14745);
// the same operator can be evaluated EXACTLY (to rounding) by fast diagonalisation:
// the 1-D operator tridiag(1,-2,1) with Dirichlet ends has the sine eigenvectors
// Q[k][j] = sqrt(2/9) sin(pi (j+1)(k+1)/9) (Q = Q^T = Q^-1) and eigenvalues
// lam_k = 2 cos(pi (k+1)/9) - 2, so  z = (Q x Q x Q) [ (Q x Q x Q) r / (lam_i+lam_j+lam_k) ].
// Six 8-point transforms per lane (40 FP64 ops each thanks to Q[k][7-j] = (-1)^k Q[k][j]),
// four LDS transposes, no reductions, no iteration, no divergence: ~260 FP64 operations per
// lane against ~124 per CG ITERATION.  Its result differs from the reference's CG result by
// the CG's own truncation error (<= cond * 1e-7), i.e. it is the same preconditioner
// evaluated more accurately; selected with cup3d_poisson_params.block_solver = 1.
// HELM: the block operator of the implicit diffusion, sum6(z) + (-6 - h^2/nu/dt) z (diffusion_kernels::getZImplParallel, 10534-10579), has
// the same eigenvectors and the eigenvalues lam_i + lam_j + lam_k - h^2/nu/dt.  The shift differs per block (h) and per call (dt, nu), so
// there is no table of reciprocals: every lane forms its eight divisors from the 1-D eigenvalues in cLam and divides (IEEE divisions: the
// solve stays a sequence of IEEE operations that is linear in r, so z(2^k r) == 2^k z(r) bit for bit).  Selected per sim with
// cup3d_diffusion_set_block_solver(sim, 1).
__constant__ double cQ[8][4];
__constant__ double cLam[8];      // lam_k = 2 cos(pi (k+1)/9) - 2 (HELM)
static double *g_invD = nullptr;  // [ky][kz][kx] = 1 / (lam_kx + lam_ky + lam_kz)

__device__ __forceinline__ void sine_transform8(const double (&v)[8], double (&o)[8]) {
  const double e0 = v[0] + v[7], e1 = v[1] + v[6], e2 = v[2] + v[5], e3 = v[3] + v[4];
  const double d0 = v[0] - v[7], d1 = v[1] - v[6], d2 = v[2] - v[5], d3 = v[3] - v[4];
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    o[k] = __builtin_fma(cQ[k][3], e3, __builtin_fma(cQ[k][2], e2, __builtin_fma(cQ[k][1], e1, cQ[k][0] * e0)));
    o[k + 1] = __builtin_fma(cQ[k + 1][3], d3, __builtin_fma(cQ[k + 1][2], d2, __builtin_fma(cQ[k + 1][1], d1, cQ[k + 1][0] * d0)));
  }
}

constexpr int kFdmLds = 64 * 9;  // transposes; pitch 9 doubles keeps every ds_read/write_b64 conflict-free
// the direct solve of one block by its wavefront: v[z] = (right-hand side / h) of cell (x = lane & 7, y = lane >> 3, z) on entry;
// out receives M^-1, block_sums[slot] (if any) sum(z h^3).  T: kFdmLds doubles of LDS nobody else is using.
// HELM: the eigenvalues are shifted by -shift (= h^2/nu/dt of this block) and invD is not read.
template <bool AG = false, bool HELM = false>
__device__ __forceinline__ void fdm_block(const GridDev &g, int slot, double (&v)[8], double *__restrict__ out, const double *__restrict__ invD,
                                          double *__restrict__ block_sums, double *T, double shift = 0.0) {
  const int l = threadIdx.x, lo = l & 7, hi = l >> 3;
  double w[8], scale[8];
  double rr = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    if constexpr (!HELM) scale[z] = invD[z * 64 + l];
    rr = __builtin_fma(v[z], v[z], rr);
  }
  rr = wave_sum(rr);
  const bool tiny = (double)1 / (512 * 512) * rr < 1e-32;  // the reference leaves such a block at 0 (14735-14736)
  // forward: z (registers), x, y
  sine_transform8(v, w);  // lane (x=lo, y=hi), register kz
#pragma unroll
  for (int k = 0; k < 8; ++k) T[(k * 8 + hi) * 9 + lo] = w[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = T[l * 9 + k];  // lane (y=lo, kz=hi), register x
  __syncthreads();
  sine_transform8(v, w);  // register kx
#pragma unroll
  for (int k = 0; k < 8; ++k) T[(hi * 8 + k) * 9 + lo] = w[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = T[l * 9 + k];  // lane (kx=lo, kz=hi), register y
  __syncthreads();
  sine_transform8(v, w);  // register ky
  if constexpr (HELM) {
    const double lxz = cLam[lo] + cLam[hi];  // this lane's kx and kz; cLam[k] below is the same for every lane
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = w[k] / ((lxz + cLam[k]) - shift);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] *= scale[k];
  }
  // inverse: y, x, z
  sine_transform8(w, v);  // register y, lane (kx, kz)
#pragma unroll
  for (int k = 0; k < 8; ++k) T[(hi * 8 + k) * 9 + lo] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = T[l * 9 + k];  // lane (y=lo, kz=hi), register kx
  __syncthreads();
  sine_transform8(w, v);  // register x
#pragma unroll
  for (int k = 0; k < 8; ++k) T[l * 9 + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = T[(k * 8 + hi) * 9 + lo];  // lane (x=lo, y=hi), register kz
  sine_transform8(w, v);  // register z
  double sx = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    const double r = tiny ? 0.0 : v[z];
    out[(size_t)slot * 512 + z * 64 + l] = r;
    sx += r;
  }
  if (block_sums) {
    const double hq = block_h(g, slot), h3 = hq * hq * hq;
    sx = wave_sum(sx * h3);
    if (l == 0) { if constexpr (AG) st_agent(block_sums + slot, sx); else block_sums[slot] = sx; }
  }
}
__global__ void __launch_bounds__(64) k_precond_fdm(GridDev g, const double *in, double *out, const double *__restrict__ invD,
                                                    double *__restrict__ block_sums) {
  __shared__ double T[kFdmLds];
  const int slot = block_slot(g);
  if (slot < 0) return;
  const int l = threadIdx.x;
  const double invh = 1 / block_h(g, slot);
  double v[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) v[z] = invh * in[(size_t)slot * 512 + z * 64 + l];
  fdm_block(g, slot, v, out, invD, block_sums, T);
}
// the same for the Helmholtz block operator of the implicit diffusion; the shift as cg_block<.., HELM> evaluates it.
// A template for its PLACE in the code object alone: the compiler emits the plain kernels in the order of their definitions and the
// instantiations behind them in the order of their first use, and this one's only use is the last thing in poisson.hip
// (launch_precond_fdm_helm), so it lands behind every other kernel and none of them moves.  Emitted where it is written, in front of the loop
// kernels, it shifted them by 4864 bytes, and bicgstab_loop1_cg (k_loop1_cg_w5, the same instructions) ran 1.4 % slower at 512^3: 3.922-3.965
// against 3.865-3.869 ms, release libraries alternating x3 on one box (profiles/helmholtz_direct_block_solve/).
template <int = 0>
__global__ void __launch_bounds__(64) k_precond_fdm_helm(GridDev g, const double *in, double *out, double nu, double dt) {
  __shared__ double T[kFdmLds];
  const int slot = block_slot(g);
  if (slot < 0) return;
  const int l = threadIdx.x;
  const double hq = block_h(g, slot), invh = 1 / hq;
  double v[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) v[z] = invh * in[(size_t)slot * 512 + z * 64 + l];
  fdm_block<false, true>(g, slot, v, out, nullptr, nullptr, T, hq * hq / nu / dt);
}

#ifdef CUP3D_TESTING
// TEST SUPPORT: the two wave-wide sums of one 64-value vector: out[0..63] = MFMA form per lane, out[64..127] = DPP form per lane
__global__ void __launch_bounds__(64) k_debug_wave_sum(const double *__restrict__ in, double *__restrict__ out) {
  const double v = in[threadIdx.x];
  out[threadIdx.x] = wave_sum_mfma(v);
  out[64 + threadIdx.x] = wave_sum(v);
}
// TEST SUPPORT: the reciprocal division of the production block CG (cg_div<true>) elementwise: out[i] = fast_div(n[i], d[i])
__global__ void __launch_bounds__(256) k_debug_cg_div(const double *__restrict__ n, const double *__restrict__ d, long count, double *__restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = fast_div(n[i], d[i]);
}
#endif

static int fdm_setup() {
  if (g_invD) return CUP3D_OK;
  double Q[8][4], lam[8], invD[512];
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 8; ++k) {
    lam[k] = 2.0 * std::cos(pi * (k + 1) / 9.0) - 2.0;
    for (int j = 0; j < 4; ++j) Q[k][j] = std::sqrt(2.0 / 9.0) * std::sin(pi * (j + 1) * (k + 1) / 9.0);
  }
  for (int ky = 0; ky < 8; ++ky)
    for (int kz = 0; kz < 8; ++kz)
      for (int kx = 0; kx < 8; ++kx) invD[ky * 64 + kz * 8 + kx] = 1.0 / (lam[kx] + lam[ky] + lam[kz]);
  CUP3D_HIP(hipMemcpyToSymbol(HIP_SYMBOL(cQ), Q, sizeof Q));
  CUP3D_HIP(hipMemcpyToSymbol(HIP_SYMBOL(cLam), lam, sizeof lam));
  CUP3D_HIP(hipMalloc((void **)&g_invD, sizeof invD));
  CUP3D_HIP(hipMemcpy(g_invD, invD, sizeof invD, hipMemcpyHostToDevice));
  return CUP3D_OK;
}

static int *cg_iters_buffer(Sim *s) {  // per-block CG iteration counts of the last launch (measurement only)
  if (!s->d_cg_iters && s->d_cg_iters.alloc((size_t)s->nb)) return nullptr;
  return s->d_cg_iters;
}

// Evaluation of the production block CG (EV bits of cg_block).  Round 6: 6 = single-width LDS reads (bit 2: 32 ds_read_b64 with immediate
// plane offsets instead of 16 half-rate ds_read2_b64 + 8 address adds per CG iteration) + reciprocal divisions (bit 4: v_rcp_f64, two
// Newton steps and a residual correction, within 1 ulp of the IEEE quotient, 8 instead of 12 instructions, twice per iteration).
// Rounds 2-5 ran EV 0: the variants had only been compared on the stand-alone kernel with an input that converges in three CG
// iterations (profiles/r02/probe_block_cg_variants_*.jsonl: all within 2 %).  Behind the loops on the solver's own inputs (27 CG
// iterations per block) the A/B on one box reads 9.17 -> 8.77 ms per BiCGSTAB iteration at 512^3 and 1.194 -> 1.142 at 256^3 (-4.3 %),
// with identical BiCGSTAB counts (profiles/r06/block_cg_evaluation_behind_the_loops/): bit 2 alone -2.5 % (bit-identical results),
// bit 4 alone -1.6 %, bit 8 (three-operand FMA for the p update) nothing.  Like the FMA contraction, the reciprocal division is a
// rounding-level deviation inside a block solve that is truncated at 1e-7; block_solver 2 stays the reference's association and IEEE division.
constexpr int kCgProduction = 6;

typedef void (*PrecondKernel)(GridDev, const double *, double *, double *, double, double, int *);
// the FMA block CG in evaluation `ev`: the release library holds kCgProduction alone, the testing one all sixteen (kernel_probe.py cgvar)
#ifdef CUP3D_TESTING
template <int... EV>
static PrecondKernel cg_evaluation(int ev, std::integer_sequence<int, EV...>) {
  static const PrecondKernel table[] = {k_precond<true, false, EV>...};
  return table[ev];
}
static PrecondKernel cg_evaluation(int ev) { return cg_evaluation(ev, std::make_integer_sequence<int, 16>()); }
#else
static PrecondKernel cg_evaluation(int) { return k_precond<true, false, kCgProduction>; }
#endif

int launch_precond(Sim *s, const double *in, double *out, bool want_sums) {
  GridDev g = s->gdev();
  double *sums = want_sums ? s->d_partials + (size_t)s->max_groups * 8 : nullptr;
  if (s->block_solver == 5) {  // one multigrid V-cycle (multigrid.hip); the LHS that follows sums the blocks itself
    s->sums_of = nullptr;
    return mg_vcycle(s, in, out);
  }
  if (s->block_solver == 1) {
    int rc = fdm_setup();
    if (rc) return rc;
    ProfileScope ps("poisson_block_fdm");
    hipLaunchKernelGGL(k_precond_fdm, dim3(launch_groups(g)), dim3(64), 0, stream(), g, in, out, g_invD, sums);
    CUP3D_HIP(hipGetLastError());
    s->sums_of = want_sums ? out : nullptr;
    return CUP3D_OK;
  }
  ProfileScope ps("poisson_block_cg");
  // Production (block_solver 0, kCgProduction) contracts a*b+c into FMAs here (and only here) and divides by reciprocal + correction
  // (within 1 ulp); wave sums by DPP (the matrix-pipe sums described above k_precond were measured slower and exist in the testing
  // flavour only).  Its result sits behind two wave reductions per iteration whose summation order already differs from the CPU's, and the
  // CG's own truncation is 1e-7, so the contraction is a tolerance-level deviation (tests bound it against the reference's z).
  // block_solver 2 = the reference's association (no contraction).
  const dim3 G(launch_groups(g)), B(64);
  int *it = profile_on() ? cg_iters_buffer(s) : nullptr;  // for the FP64 roofline of bench.py (cup3d_profile_block_cg_iterations)
  PrecondKernel k = nullptr;
  switch (s->block_solver) {
    case 0: {  // production: kCgProduction, or (tuning) the evaluation selected with cup3d_debug_set_option("cg_variant", 8 + bits)
      int ev = kCgProduction;
#ifdef CUP3D_TESTING
      if (debug_option("cg_variant") >= 8) ev = debug_option("cg_variant") - 8;
      if (ev >= 16) { set_error("unknown cg_variant"); return CUP3D_EINVAL; }
#endif
      k = cg_evaluation(ev);
      break;
    }
    case 2: k = k_precond<false, false, 0>; break;
#ifdef CUP3D_TESTING
    case 3: k = cg_evaluation(0); break;  // EV 0: production's evaluation of rounds 1-5 (FMA contraction, IEEE divisions, ds_read2_b64), kept for A/B
    case 4: {  // two blocks per wavefront (A/B timing)
      const int pchunk = ((g.nblocks + 1) / 2 + 7) / 8;
      hipLaunchKernelGGL((k_precond_pair<true, false>), dim3(8 * pchunk), B, 0, stream(), g, pchunk, in, out, sums, 0.0, 0.0, it);
      break;
    }
#else
    case 3: case 4: return not_in_release("block_solver 3 / 4 (A/B variants of the block CG)");
#endif
    default: set_error("unknown block_solver %d", s->block_solver); return CUP3D_EINVAL;
  }
  if (k) hipLaunchKernelGGL(k, G, B, 0, stream(), g, in, out, sums, 0.0, 0.0, it);
  CUP3D_HIP(hipGetLastError());
  s->sums_of = want_sums ? out : nullptr;  // block sums of `out` are fresh: the next LHS of `out` reuses them
  return CUP3D_OK;
}

static int launch_precond_fdm_helm(Sim *s, const double *in, double *out, const HelmholtzOp &op);  // at the end of poisson.hip (see k_precond_fdm_helm)

int launch_precond_diffusion(Sim *s, const double *in, double *out, const HelmholtzOp &op) {
  GridDev g = s->gdev();
  if (s->diffusion_block_solver == 1) return launch_precond_fdm_helm(s, in, out, op);  // cup3d_diffusion_set_block_solver: the direct solve
  ProfileScope ps("diffusion_block_cg");
  if (s->block_solver != 2) hipLaunchKernelGGL((k_precond<true, true, kCgProduction>), dim3(launch_groups(g)), dim3(64), 0, stream(), g, in, out, (double *)nullptr, op.nu, op.dt, (int *)nullptr);
  else hipLaunchKernelGGL((k_precond<false, true, 0>), dim3(launch_groups(g)), dim3(64), 0, stream(), g, in, out, (double *)nullptr, op.nu, op.dt, (int *)nullptr);
  CUP3D_HIP(hipGetLastError());
  s->sums_of = nullptr;
  return CUP3D_OK;
}

}  // namespace cup3d
