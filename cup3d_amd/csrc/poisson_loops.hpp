// The fused loop kernels (vector loop + LHS tile + block solve in one launch).
// Part of poisson.hip's translation unit: included there once, in order; not a stand-alone header.
#pragma once

namespace cup3d {

// ------------------------------------------------------------------ vector loop + block preconditioner in ONE launch
// Per BiCGSTAB iteration the reference runs   loop 1 -> z ;  zhat = M^-1 z ;  v = A zhat   and   loop 2 -> w ;  what = M^-1 w ;  t = A what.
// The fused vector loops are HBM-bound (6.2 TB/s, nothing for the FP64 units to do), the block CG that consumes their output is
// bound by FP64 issue and LDS (0.1 of the HBM roof) -- run back to back they each leave the other resource idle, and together they
// are 93 % of an iteration.  Here one wavefront owns one block from start to end: it streams the block's 512 cells of the 11 (12)
// input vectors, writes the 7 (4) updated ones, keeps the block of z (w) in registers and runs the block CG on it straight away;
// while it iterates, the other wavefronts of the SIMD are in their streaming phase, so the two bounds overlap instead of adding.
// The arithmetic per cell is that of k_loop1 / k_loop2 and of cg_block, unchanged; the dot products are summed per block first
// (wave tree) and the per-block values by k_sums_finish, another order than the grid-stride partials of the unfused kernels.
// block_dots layout: [K][nb].
struct Loop1Args { double alpha, beta, omega; };
struct Loop2Args { double alpha, omega; };

#define NTL(v, j) __builtin_nontemporal_load(&(v)[j])
#define NTS(v, j, val) __builtin_nontemporal_store((val), &(v)[j])

// ---- the LHS application folded into the loop kernel that needs its result (uniform grids)
// Per iteration the reference applies  v = A zhat  after the first loop and  t = A what  after the second (14489, 14549), and each
// loop then streams t and v like any other vector.  On the device that was two launches of k_lhs (16 B/cell each, 12 % of an
// iteration, with the all-reduce tucked behind them).  With FLHS the wavefront that owns a block builds the ghosted tile of the
// block's what (first loop) / zhat (second loop) in LDS -- its own column of 8 planes plus the six face slabs, fetched from the
// neighbour slots, the domain-face rule (zero-gradient: own face cell) or the halo slabs of other ranks, i.e. what load_scalar_tile
// does for a 256-thread workgroup -- evaluates  h (xm + xp + ym + yp + zm + zp - 6 c)  in k_lhs's association (BIT-IDENTICAL t and
// v), uses the value in place of the streamed one and stores it for the other loop.  One stream fewer to read, no k_lhs launch.
// Tile layout: 10 planes (0 and 9: the z ghosts) of pitch 96 doubles = 10 rows of 8 (rows 0 and 9: the y ghosts) + 8 x-minus ghosts
// + 8 x-plus ghosts.  960 doubles; the block CG's LDS (zeroed again when the CG starts) is inside it.  Every stencil operand is one
// ds_read_b64 with an immediate plane offset: nothing is carried in registers from plane to plane.
constexpr int kLoopPrio = 0;  // LhsIn::prio of the production launch (measured: profiles/r03)
constexpr int kTilePitch = 96, kTileLds = 10 * kTilePitch;
static_assert(kTileLds >= kCgLds && kTileLds >= kFdmLds, "the block solve reuses the tile's LDS");
struct LhsIn {
  const double *halo;   // face slabs received from other ranks (Sim::halo_recv)
  const double *total;  // sum(u h^3) over all ranks, for the mean-constraint row (9283-9326); device memory
  int mode;             // bMeanConstraint as ComputeLHS uses it: 0 none, 1 corner row = total, 2 += total h^3 everywhere, 3 corner row = u
  int corner_slot;      // slot of the block with index (0,0,0) on this rank, or -1
  int prio;             // wave priority (s_setprio) while the wavefront streams its block; back to 0 when the block CG starts
  const double *invD;   // DIRECT form of the block solve (block_solver 1): 1 / (lam_kx + lam_ky + lam_kz), [ky][kz][kx]; else unused
  // early all-reduce over ranks (solve(): early): *total is valid once *mean_flag has reached mean_seq -- the wavefronts that USE the total
  // wait for that (mode 1: the corner block's only); nullptr: the total was complete before the launch
  const unsigned *mean_flag;
  int mean_wait;        // which value: 1 = 2 (seq - 1) + 1 (first loop: the total of the previous iteration's second loop), 2 = 2 seq (second loop); seq = SolverCtl::seq
  unsigned *fail;       // pinned: raised when that wait gives up (10 s)
};
struct TileRegs { double c[8], gv[6]; };
// the 14 loads of a tile in two groups: the block's own column (needs nothing but the slot) and the six face slabs (need the
// neighbour table first); the caller issues the first plane of its streams between the two, then commits
__device__ __forceinline__ void tile_issue_own(int slot, const double *__restrict__ f, int l, TileRegs &R) {
  const double *own = f + (size_t)slot * 512;
#pragma unroll
  for (int z = 0; z < 8; ++z) R.c[z] = own[z * 64 + l];
}
__device__ __forceinline__ void tile_issue_faces(const GridDev &g, int slot, const double *__restrict__ f, const double *__restrict__ halo, int l, TileRegs &R) {
  const double *own = f + (size_t)slot * 512;
#pragma unroll
  for (int face = 0; face < 6; ++face) {
    const int n = g.nbr[slot * 6 + face];
    int nb_cell, own_cell, lds;
    face1(face, l, nb_cell, own_cell, lds);
    const double *__restrict__ base = n >= kNbrHalo ? halo + (size_t)(n - kNbrHalo) * 64 : (n >= 0 ? f + (size_t)n * 512 : own);
    R.gv[face] = base[n >= kNbrHalo ? l : (n >= 0 ? nb_cell : own_cell)];
  }
}
__device__ __forceinline__ void tile_commit(const TileRegs &R, double *T, int l) {
  const int base = ((l >> 3) + 1) * 8 + (l & 7), a1 = l & 7, a2 = (l >> 3) + 1;
#pragma unroll
  for (int z = 0; z < 8; ++z) T[(z + 1) * kTilePitch + base] = R.c[z];
  T[a2 * kTilePitch + 80 + a1] = R.gv[0];  // x faces: lane = (a1 = y, z = a2 - 1)
  T[a2 * kTilePitch + 88 + a1] = R.gv[1];
  T[a2 * kTilePitch + a1] = R.gv[2];       // y faces: lane = (a1 = x, z = a2 - 1) -> rows 0 and 9
  T[a2 * kTilePitch + 72 + a1] = R.gv[3];
  T[base] = R.gv[4];                       // z faces: lane = (x, y) -> planes 0 and 9
  T[9 * kTilePitch + base] = R.gv[5];
  __syncthreads();
}
// per-lane tile offsets of the x neighbours (the edge lanes read the ghost slots behind the rows)
struct TileIdx { int base, ixm, ixp; };
__device__ __forceinline__ TileIdx tile_idx(int l) {
  const int x = l & 7, y = l >> 3, base = (y + 1) * 8 + x;
  return TileIdx{base, x > 0 ? base - 1 : 80 + y, x < 7 ? base + 1 : 88 + y};
}
// the mean-constraint fix-ups of ComputeLHS (9299-9326), decided once per wavefront so that the plane loop stays one basic block
// (a branch per plane makes the compiler keep every stream's address in a VGPR pair: +34 registers)
struct LhsFix {
  double total, add;  // sum(u h^3) over all ranks; total * h^3 (mode 2)
  bool add_mean;      // mode 2: t += total h^3 in every cell (9314)
  bool row_total;     // this lane holds the corner cell (plane 0) and mode 1: t = total (9299-9304)
  bool row_self;      // ... and mode > 2: t = u (9316-9325)
};
__device__ __forceinline__ LhsFix lhs_fix(const LhsIn &L, const SolverCtl *ctl, int slot, int l, double h) {
  LhsFix f;
  const bool uses_total = L.mode == 2 || (L.mode == 1 && slot == L.corner_slot);  // wave-uniform
  if (uses_total && L.mean_flag) {
    const unsigned want = L.mean_wait == 1 ? 2 * (ctl->seq - 1) + 1 : 2 * ctl->seq;
    const long long t0 = wall_clock64();
    while ((int)(__hip_atomic_load(L.mean_flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
      __builtin_amdgcn_s_sleep(8);
      if (wall_clock64() - t0 > 1000000000LL) { if (l == 0) __hip_atomic_store(L.fail, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
    }
  }
  f.total = uses_total ? ld_agent(L.total) : 0.0;
  f.add = f.total * (h * h * h);
  f.add_mean = L.mode == 2;
  const bool corner = slot == L.corner_slot && l == 0;
  f.row_total = corner && L.mode == 1;
  f.row_self = corner && L.mode > 2;
  return f;
}
// KernelLHSPoisson (9211-9214) for the cell of lane l in plane zz, in k_lhs's association; cc = the cell's own value
template <int ZZ>
__device__ __forceinline__ double tile_lhs(const double *T, const TileIdx &ix, double &cc, double h, const LhsFix &f) {
  // volatile LDS pointers (address space kept): one ds_read_b64 per operand, in this order, plane offset in the instruction
  typedef const volatile __attribute__((address_space(3))) double lds_cvd;
  lds_cvd *Q = (lds_cvd *)(T + (ZZ + 1) * kTilePitch);
  cc = Q[ix.base];
  double t = Q[ix.ixm] + Q[ix.ixp];
  t += Q[ix.base - 8];
  t += Q[ix.base + 8];
  t += Q[ix.base - kTilePitch];
  t += Q[ix.base + kTilePitch];
  t = h * (t - 6.0 * cc);
  if (ZZ == 0) {  // the corner cell is cell 0 of its block: selects, no branches
    t = f.row_total ? f.total : t;
    t = f.row_self ? cc : t;
  }
  const double t2 = t + f.add;
  return f.add_mean ? t2 : t;
}

// (The two bodies below repeat their scaffolding -- LOAD_PLANE, the tile prologue, the tail around the block solve.  Factored into
//  __forceinline__ helpers the register allocation moves: k_loop2_cg_w4 takes 130 registers, 3 wavefronts per SIMD.  So it stays written out.)
// DIRECT: the block solve behind the loop is the fast diagonalisation (fdm_block: the same M^-1, exact instead of by CG -- block_solver 1,
// bench.py's `alt`), not the reference's CG: no iteration, no reductions, so the kernel is what the streams alone allow
// TOT: the kernel totals its per-block values itself (Arrive; the early all-reduce over ranks) -- else a launch of k_sums_finish does
template <bool FMA, int EV, bool FLHS, bool DIRECT = false, bool TOT = false>
__device__ __forceinline__ void loop1_cg_body(const GridDev &g, const Vecs &V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb,
                                              double *block_sums, int *__restrict__ iters_out, const LhsIn &L, const LoopSums *__restrict__ Z) {
  __shared__ double P[FLHS ? kTileLds : (DIRECT ? kFdmLds : kCgLds)];
  const int slot = block_slot(g);
  if (slot < 0) return;
  if (ctl->state != kRun) return;  // enqueued ahead of a stop or a restart (see SolverCtl)
  const Loop1Args a{ctl->alpha, ctl->beta, ctl->omega};
  const int l = threadIdx.x;
  const double hq = block_h(g, slot), invh = 1 / hq;
  double r[8], d0 = 0, d1 = 0;
  // plane zz + 1 is requested before plane zz is computed and stored (two planes = 22 x 512 B per wavefront in flight): the loads
  // may alias the stores as far as the compiler knows, so the order has to be written out
  // (block base pointers are wave-uniform -> scalar registers; the per-lane part of every address is one 32-bit offset)
  const size_t bo = (size_t)slot * 512;
  // FLHS: what comes from the tile and t is computed from it -- streams 6 and 8 are not loaded
  enum { iRHAT, iW, iSHAT, iZ, iPHAT, iS, iWHAT, iZHAT, iT, iV, iR, NS };
  const double *const src[NS] = {V.v[RHAT] + bo, V.v[W_] + bo, V.v[SHAT] + bo, V.v[Z_] + bo, V.v[PHAT] + bo, V.v[S_] + bo, V.v[WHAT] + bo, V.v[ZHAT] + bo,
                                 V.v[T_] + bo, V.v[V_] + bo, V.v[R_] + bo};
  double *const oP = V.v[PHAT] + bo, *const oS = V.v[S_] + bo, *const oSH = V.v[SHAT] + bo, *const oZ = V.v[Z_] + bo, *const oQ = V.v[Q_] + bo,
               *const oQH = V.v[QHAT] + bo, *const oY = V.v[Y_] + bo, *const oT = V.v[T_] + bo;
  double in[2][NS];
#define LOAD_PLANE(buf, off)                                                            \
  _Pragma("unroll") for (int i = 0; i < NS; ++i)                                        \
    if (!(FLHS && (i == iWHAT || i == iT))) in[buf][i] = NTL(src[i], off);
  TileIdx ix{0, 0, 0};
  LhsFix fx{};
  TileRegs tr;
  if constexpr (FLHS) {  // the tile's loads first, the first plane of the streams right behind them, then the tile goes to LDS
    fx = lhs_fix(L, ctl, slot, l, hq);
    tile_issue_own(slot, V.v[WHAT], l, tr);
    ix = tile_idx(l);
  }
  // (a streaming wavefront's loads and stores go out ahead of the arithmetic of the wavefronts that sit in their block CG)
  if (L.prio == 1) __builtin_amdgcn_s_setprio(1); else if (L.prio == 2) __builtin_amdgcn_s_setprio(2); else if (L.prio == 3) __builtin_amdgcn_s_setprio(3);
  LOAD_PLANE(0, l)
  if constexpr (FLHS) {
    tile_issue_faces(g, slot, V.v[WHAT], L.halo, l, tr);  // (before or behind the first plane: no measurable difference, profiles/r03)
    tile_commit(tr, P, l);
  }
#pragma unroll
  for (int zz = 0; zz < 8; ++zz) {  // first fused loop, 14454-14464, on plane zz of this block
    const int j = zz * 64 + l;
    if (zz < 7) { LOAD_PLANE((zz + 1) & 1, j + 64) }
    const double *c = in[zz & 1];
    double what = c[iWHAT], t = c[iT];
    if constexpr (FLHS) {
      t = zz == 0 ? tile_lhs<0>(P, ix, what, hq, fx) : tile_lhs<1>(P + (zz - 1) * kTilePitch, ix, what, hq, fx);   // t = A what, 14549
      NTS(oT, j, t);                                                              // the second loop streams it
    }
    const double rhat = c[iRHAT], w = c[iW], shat0 = c[iSHAT], z0 = c[iZ];
    const double phat = rhat + a.beta * (c[iPHAT] - a.omega * shat0);
    const double sv = w + a.beta * (c[iS] - a.omega * z0);
    const double shat = what + a.beta * (shat0 - a.omega * c[iZHAT]);
    const double z = t + a.beta * (z0 - a.omega * c[iV]);
    const double q = c[iR] - a.alpha * sv;
    const double qhat = rhat - a.alpha * shat;
    const double y = w - a.alpha * z;
    NTS(oP, j, phat); NTS(oS, j, sv); NTS(oSH, j, shat); NTS(oZ, j, z); NTS(oQ, j, q); NTS(oQH, j, qhat); NTS(oY, j, y);
    d0 += q * y;
    d1 += y * y;
    r[zz] = invh * z;  // the right-hand side of the block solve, main.cpp:14723
  }
#undef LOAD_PLANE
  d0 = wave_sum(d0);
  d1 = wave_sum(d1);
  if constexpr (TOT) {
    if (l == 0) { st_agent(block_dots + slot, d0); st_agent(block_dots + nb + slot, d1); }
    arrive<2>(Z->dots, slot, Z->then);  // q.y, y.y are complete when the last block passes here: the totals exist one block solve before the kernel ends
  } else if (l == 0) { block_dots[slot] = d0; block_dots[nb + slot] = d1; }
  if (L.prio) __builtin_amdgcn_s_setprio(0);
  if constexpr (FLHS) __syncthreads();  // the tile is read no more: the block solve takes over its LDS
  if constexpr (DIRECT) fdm_block<TOT>(g, slot, r, V.v[ZHAT], L.invD, block_sums, P);
  else cg_block<FMA, false, EV, TOT>(g, slot, r, V.v[ZHAT], block_sums, 0.0, 0.0, iters_out, P);  // zhat = M^-1 z, 14488
  if constexpr (TOT) if (Z->mean.vals) arrive<1>(Z->mean, slot, NoThen());  // sum(zhat h^3) for the mean-constraint row of v = A zhat
}
// (with the LHS inside the compiler takes 110 registers -> 4 wavefronts per SIMD; held to 5 wavefronts it fits 94 without a spill and is
//  SLOWER: 0.54 instead of 0.51 ms at 256^3, 3.96 instead of 3.93 at 512^3 -- profiles/r03)
template <bool FMA, int EV, bool FLHS>
__global__ void __launch_bounds__(64) k_loop1_cg(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums,
                                                 int *__restrict__ iters_out, LhsIn L, const LoopSums *__restrict__ Z) {
  loop1_cg_body<FMA, EV, FLHS>(g, V, ctl, block_dots, nb, block_sums, iters_out, L, Z);
}
// The same kernel held to 5 wavefronts per SIMD (94 registers, no spill; the 7.5 KB tile allows 21 per CU).  Round 3 measured this
// SLOWER with the ds_read2_b64 form of the block CG; with the single-width reads of round 6, which leave the LDS headroom for a fifth
// wavefront, it is 3 % FASTER at 512^3 (3.78 against 3.90 ms, 262 144 blocks = 51 rounds of wavefronts) and 1.5 % slower at 256^3
// (0.512 against 0.505 ms: 6.4 rounds, the tail of the last round weighs more) -- profiles/r06/loop1_five_waves/.  Production takes it
// from kFiveWavesFrom blocks per launch; same body, same bits.
constexpr int kFiveWavesFrom = 131072;
template <bool FMA, int EV, bool FLHS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
k_loop1_cg_w5(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums, int *__restrict__ iters_out, LhsIn L, const LoopSums *__restrict__ Z) {
  loop1_cg_body<FMA, EV, FLHS>(g, V, ctl, block_dots, nb, block_sums, iters_out, L, Z);
}
// block_solver 1: first loop + the direct block solve (`alt`)
template <bool FLHS>
__global__ void __launch_bounds__(64) k_loop1_fdm(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums,
                                                  LhsIn L, const LoopSums *__restrict__ Z) {
  loop1_cg_body<true, 0, FLHS, true>(g, V, ctl, block_dots, nb, block_sums, nullptr, L, Z);
}

template <bool FMA, int EV, bool FLHS, bool DIRECT = false, bool TOT = false>
__device__ __forceinline__ void loop2_cg_body(const GridDev &g, const Vecs &V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb,
                                              double *block_sums, int *__restrict__ iters_out, const LhsIn &L, const LoopSums *__restrict__ Z) {
  __shared__ double P[FLHS ? kTileLds : (DIRECT ? kFdmLds : kCgLds)];
  const int slot = block_slot(g);
  if (slot < 0) return;
  if (ctl->state != kRun) return;
  const Loop2Args a{ctl->alpha, ctl->omega};
  // the two x buffers are v[X_] and v[XOPT] for the whole solve; which one holds x and which one receives the update is the struct's
  const int xc = ctl->xcur, xw = ctl_xwrite(*ctl);
  const double *const xin = xc ? V.v[XOPT] : V.v[X_];
  const int l = threadIdx.x;
  const double hq = block_h(g, slot), invh = 1 / hq;
  double r[8], acc[6] = {0, 0, 0, 0, 0, 0};
  const size_t bo = (size_t)slot * 512;
  // FLHS: zhat comes from the tile and v is computed from it -- streams 7 and 9 are not loaded
  enum { iQHAT, iY, iR0, iX, iPHAT, iQ, iWHAT, iZHAT, iT, iV, iS, iZ, NS };
  const double *const src[NS] = {V.v[QHAT] + bo, V.v[Y_] + bo, V.v[R0] + bo, xin + bo, V.v[PHAT] + bo, V.v[Q_] + bo, V.v[WHAT] + bo, V.v[ZHAT] + bo,
                                 V.v[T_] + bo, V.v[V_] + bo, V.v[S_] + bo, V.v[Z_] + bo};
  double *const oX = (xw ? V.v[XOPT] : V.v[X_]) + bo, *const oR = V.v[R_] + bo, *const oRH = V.v[RHAT] + bo, *const oW = V.v[W_] + bo, *const oV = V.v[V_] + bo;
  double in[2][NS];
#define LOAD_PLANE(buf, off)                                                            \
  _Pragma("unroll") for (int i = 0; i < NS; ++i)                                        \
    if (!(FLHS && (i == iZHAT || i == iV))) in[buf][i] = NTL(src[i], off);
  TileIdx ix{0, 0, 0};
  LhsFix fx{};
  TileRegs tr;
  if constexpr (FLHS) {  // the tile's loads first, the first plane of the streams right behind them, then the tile goes to LDS
    fx = lhs_fix(L, ctl, slot, l, hq);
    tile_issue_own(slot, V.v[ZHAT], l, tr);
    ix = tile_idx(l);
  }
  if (L.prio == 1) __builtin_amdgcn_s_setprio(1); else if (L.prio == 2) __builtin_amdgcn_s_setprio(2); else if (L.prio == 3) __builtin_amdgcn_s_setprio(3);
  LOAD_PLANE(0, l)
  if constexpr (FLHS) {
    tile_issue_faces(g, slot, V.v[ZHAT], L.halo, l, tr);  // (before or behind the first plane: no measurable difference, profiles/r03)
    tile_commit(tr, P, l);
  }
#pragma unroll
  for (int zz = 0; zz < 8; ++zz) {  // second fused loop, 14503-14515
    const int j = zz * 64 + l;
    if (zz < 7) { LOAD_PLANE((zz + 1) & 1, j + 64) }
    const double *c = in[zz & 1];
    double zhat = c[iZHAT], v = c[iV];
    if constexpr (FLHS) {
      v = zz == 0 ? tile_lhs<0>(P, ix, zhat, hq, fx) : tile_lhs<1>(P + (zz - 1) * kTilePitch, ix, zhat, hq, fx);   // v = A zhat, 14489
      NTS(oV, j, v);                                                              // the next first loop streams it
    }
    const double qhat = c[iQHAT], y = c[iY], r0 = c[iR0];
    const double x = c[iX] + a.alpha * c[iPHAT] + a.omega * qhat;
    const double rv = c[iQ] - a.omega * y;
    const double rhat = qhat - a.omega * (c[iWHAT] - a.alpha * zhat);
    const double w = y - a.omega * (c[iT] - a.alpha * v);
    NTS(oX, j, x); NTS(oR, j, rv); NTS(oRH, j, rhat); NTS(oW, j, w);
    acc[0] += r0 * rv;
    acc[1] += r0 * w;
    acc[2] += r0 * c[iS];
    acc[3] += r0 * c[iZ];
    acc[4] += rv * rv;   // norm_1
    acc[5] += r0 * r0;   // norm_2
    r[zz] = invh * w;
  }
#undef LOAD_PLANE
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double t = wave_sum(acc[i]);
    if constexpr (TOT) {
      if (l == 0) st_agent(block_dots + (size_t)i * nb + slot, t);
      if (i == 4 && l == 0) st_agent(block_dots + (size_t)6 * nb + slot, t);  // norm = the same sum as norm_1 (14512-14514)
    } else {
      if (l == 0) block_dots[(size_t)i * nb + slot] = t;
      if (i == 4 && l == 0) block_dots[(size_t)6 * nb + slot] = t;  // norm = the same sum as norm_1 (14512-14514)
    }
  }
  if constexpr (TOT) arrive<7>(Z->dots, slot, Z->then);  // the seven of 14546: complete while the block solves still run
  if (L.prio) __builtin_amdgcn_s_setprio(0);
  if constexpr (FLHS) __syncthreads();
  if constexpr (DIRECT) fdm_block<TOT>(g, slot, r, V.v[WHAT], L.invD, block_sums, P);
  else cg_block<FMA, false, EV, TOT>(g, slot, r, V.v[WHAT], block_sums, 0.0, 0.0, iters_out, P);  // what = M^-1 w, 14548
  if constexpr (TOT) if (Z->mean.vals) arrive<1>(Z->mean, slot, NoThen());  // sum(what h^3) for the mean-constraint row of t = A what
}
// WITHOUT the LHS inside (FLHS = false: multi-level meshes, the no_fuse_lhs A/B): held to 96 registers (2 of the 122 the body asks for
// are spilled, outside the CG loop) -> 5 wavefronts per SIMD: 3.63-3.70 ms instead of 3.75 at 512^3, 0.457-0.461 instead of 0.497 at
// 256^3 (profiles/r02/probe_fused_kernel_occupancy.jsonl).  The same test on the other side -- the first kernel or the stand-alone block
// CG held to 80 registers for 6 wavefronts -- loses (12-14 spills inside the loops: 5.3 ms instead of 3.88; CG 0.43 instead of 0.40).
// (With FLHS held to 96 it spills 30 registers inside the plane loop: uniform grids take k_loop2_cg_w4 / k_loop2_cg_w5 below.)
template <bool FMA, int EV, bool FLHS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
k_loop2_cg(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums, int *__restrict__ iters_out, LhsIn L, const LoopSums *__restrict__ Z) {
  loop2_cg_body<FMA, EV, FLHS>(g, V, ctl, block_dots, nb, block_sums, iters_out, L, Z);
}
// Uniform grids (FLHS = true), launches below kLoop2FiveWavesFrom blocks and the reference's association (block_solver 2): the register
// allocation the compiler picks on its own, 128 registers -> 4 wavefronts per SIMD, no spills.  PRODUCTION until k_loop2_cg_w5 (below) took
// over the large launches.  (Also the "loop2_four_waves" A/B of the FLHS = false form.)
template <bool FMA, int EV, bool FLHS>
__global__ void __launch_bounds__(64) k_loop2_cg_w4(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums,
                                                    int *__restrict__ iters_out, LhsIn L, const LoopSums *__restrict__ Z) {
  loop2_cg_body<FMA, EV, FLHS>(g, V, ctl, block_dots, nb, block_sums, iters_out, L, Z);
}

// The second loop with the LHS inside at 5 wavefronts per SIMD (FLHS = true, block CG, per-block sums totalled by k_sums_finish: the form
// production launches on uniform grids).  loop2_cg_body held to 96 registers spills 124 B per lane inside the plane loop, so this is a
// body of its own: the same arithmetic per cell in the same order, the same stores, the same per-block sums -- every vector is the same
// bits as k_loop2_cg_w4's -- in 88 registers without scratch.  (A copy, not a helper shared with loop2_cg_body: an edit to that body moves
// the pinned allocation of the four kernels built from it, and helpers move it too -- see the note above loop1_cg_body.)
//  * Where the registers went: nothing but the tail reads the six running sums, so the optimiser SINKS their multiply-adds out of the
//    plane loop to behind it -- and keeps r0, s, z, rv and w of all eight planes alive for that (the spills, and a vmcnt(0) wait in front
//    of each).  An empty asm that names the six sums at the end of every plane makes them values the plane has to produce: the loop
//    then holds two planes of streams, r[] and the sums, as written.  (Making the lane offset opaque per plane, a scheduling barrier per plane and
//    r[] parked in the dead tile plane were tried on top: 88, 88 and 84 registers, none needed; every load takes scalar base + one
//    32-bit lane offset as it is.)
//  * No wave-priority branches (production runs kLoopPrio = 0).
template <bool FMA, int EV>
__device__ __forceinline__ void loop2_cg5_body(const GridDev &g, const Vecs &V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb,
                                               double *block_sums, int *__restrict__ iters_out, const LhsIn &L) {
  __shared__ double P[kTileLds];
  const int slot = block_slot(g);
  if (slot < 0) return;
  if (ctl->state != kRun) return;
  const Loop2Args a{ctl->alpha, ctl->omega};
  const int xc = ctl->xcur, xw = ctl_xwrite(*ctl);
  const double *const xin = xc ? V.v[XOPT] : V.v[X_];
  const int l = threadIdx.x;
  const double hq = block_h(g, slot), invh = 1 / hq;
  double r[8], acc[6] = {0, 0, 0, 0, 0, 0};
  const size_t bo = (size_t)slot * 512;
  // zhat comes from the tile and v is computed from it: ten streams are loaded
  enum { iQHAT, iY, iR0, iX, iPHAT, iQ, iWHAT, iT, iS, iZ, NS };
  const double *const src[NS] = {V.v[QHAT] + bo, V.v[Y_] + bo, V.v[R0] + bo, xin + bo, V.v[PHAT] + bo, V.v[Q_] + bo, V.v[WHAT] + bo, V.v[T_] + bo,
                                 V.v[S_] + bo, V.v[Z_] + bo};
  double *const oX = (xw ? V.v[XOPT] : V.v[X_]) + bo, *const oR = V.v[R_] + bo, *const oRH = V.v[RHAT] + bo, *const oW = V.v[W_] + bo, *const oV = V.v[V_] + bo;
  double in[2][NS];
  // (the lane's part of the address as a 32-bit BYTE offset: with the element index the offset is widened to 64 bits per stream and
  //  the kernel is back at 96 registers and 12 B of scratch)
#define LOAD_PLANE(buf, off)                                                                      \
  {                                                                                               \
    const unsigned o = (unsigned)(off) * 8u;                                                      \
    _Pragma("unroll") for (int i = 0; i < NS; ++i)                                                \
      in[buf][i] = __builtin_nontemporal_load((const double *)((const char *)src[i] + o));        \
  }
  // the tile's loads first, the first plane of the streams right behind them, then the tile goes to LDS
  const LhsFix fx = lhs_fix(L, ctl, slot, l, hq);
  TileRegs tr;
  tile_issue_own(slot, V.v[ZHAT], l, tr);
  const TileIdx ix = tile_idx(l);
  LOAD_PLANE(0, l)
  tile_issue_faces(g, slot, V.v[ZHAT], L.halo, l, tr);
  tile_commit(tr, P, l);
#pragma unroll
  for (int zz = 0; zz < 8; ++zz) {  // second fused loop, 14503-14515
    const int j = zz * 64 + l;
    if (zz < 7) { LOAD_PLANE((zz + 1) & 1, j + 64) }
    const double *c = in[zz & 1];
    double zhat;
    const double v = zz == 0 ? tile_lhs<0>(P, ix, zhat, hq, fx) : tile_lhs<1>(P + (zz - 1) * kTilePitch, ix, zhat, hq, fx);   // v = A zhat, 14489
    NTS(oV, j, v);                                                                // the next first loop streams it
    const double qhat = c[iQHAT], y = c[iY], r0 = c[iR0];
    const double x = c[iX] + a.alpha * c[iPHAT] + a.omega * qhat;
    const double rv = c[iQ] - a.omega * y;
    const double rhat = qhat - a.omega * (c[iWHAT] - a.alpha * zhat);
    const double w = y - a.omega * (c[iT] - a.alpha * v);
    NTS(oX, j, x); NTS(oR, j, rv); NTS(oRH, j, rhat); NTS(oW, j, w);
    acc[0] += r0 * rv;
    acc[1] += r0 * w;
    acc[2] += r0 * c[iS];
    acc[3] += r0 * c[iZ];
    acc[4] += rv * rv;   // norm_1
    acc[5] += r0 * r0;   // norm_2
    r[zz] = invh * w;
#pragma unroll
    for (int i = 0; i < 6; ++i) asm volatile("" : "+v"(acc[i]));  // this plane's sums are formed HERE (see above); no instruction
  }
#undef LOAD_PLANE
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double t = wave_sum(acc[i]);
    if (l == 0) block_dots[(size_t)i * nb + slot] = t;
    if (i == 4 && l == 0) block_dots[(size_t)6 * nb + slot] = t;  // norm = the same sum as norm_1 (14512-14514)
  }
  __syncthreads();  // the tile is read no more: the block solve takes over its LDS
  cg_block<FMA, false, EV>(g, slot, r, V.v[WHAT], block_sums, 0.0, 0.0, iters_out, P);  // what = M^-1 w, 14548
}
// PRODUCTION on uniform grids (what bench.py's `value` runs) for launches of >= kLoop2FiveWavesFrom blocks; below that k_loop2_cg_w4.
// Measured, one box, k_loop2_cg_w5 against k_loop2_cg_w4 (profiles/loop2_five_waves/): release libraries of the parent commit and of this
// one, five alternating runs of the driver's command at 512^3: 3.699-3.712 against 3.844-3.879 ms (median -4.2 %; the iteration
// 8.055-8.085 against 8.174-8.204 ms, -1.45 %: the first loop kernel behind it takes 3.72-3.73 instead of 3.68-3.69).  The threshold scan
// (testing build, `loop2_five_waves` 1 against 2, two passes): 384^3 (110 592 blocks) 1.520-1.523 against 1.606-1.609 ms; 320^3 (64 000)
// 0.873-0.874 against 0.918-0.919; 256^3 (32 768) 0.444-0.445 against 0.468-0.469; 192^3 (13 824) 0.201 against 0.209; 128^3 (4 096 blocks =
// one round of wavefronts at either occupancy) 0.080 against 0.081-0.082, the iteration 0.230-0.232 either way.  Unlike the first kernel
// there is no crossover: the threshold is the smallest launch at which the gain is outside the run-to-run range.
constexpr int kLoop2FiveWavesFrom = 13824;
template <bool FMA, int EV, bool FLHS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
k_loop2_cg_w5(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums, int *__restrict__ iters_out, LhsIn L, const LoopSums *__restrict__ Z) {
  static_assert(FLHS, "the five-wavefront form of the second loop has the LHS inside");
  loop2_cg5_body<FMA, EV>(g, V, ctl, block_dots, nb, block_sums, iters_out, L);
}

// The two kernels of an iteration with the totals INSIDE (TOT; uniform grids, block CG): the early all-reduce over ranks (solve(): `early`).
// The second one is held to 128 registers (the compiler would take 136 -> 3 wavefronts per SIMD): one 8-byte value is parked in scratch
// before the plane loop and fetched back when the block CG starts, never inside a loop.
template <bool FMA, int EV>
__global__ void __launch_bounds__(64) k_loop1_cg_tot(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums, int *__restrict__ iters_out, LhsIn L,
                                                     const LoopSums *__restrict__ Z) {
  loop1_cg_body<FMA, EV, true, false, true>(g, V, ctl, block_dots, nb, block_sums, iters_out, L, Z);
}
template <bool FMA, int EV>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_loop2_cg_tot(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums, int *__restrict__ iters_out, LhsIn L, const LoopSums *__restrict__ Z) {
  loop2_cg_body<FMA, EV, true, false, true>(g, V, ctl, block_dots, nb, block_sums, iters_out, L, Z);
}

// block_solver 1: second loop + the direct block solve (`alt`)
template <bool FLHS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) k_loop2_fdm(GridDev g, Vecs V, const SolverCtl *__restrict__ ctl, double *block_dots, long nb, double *block_sums,
                                                  LhsIn L, const LoopSums *__restrict__ Z) {
  loop2_cg_body<true, 0, FLHS, true>(g, V, ctl, block_dots, nb, block_sums, nullptr, L, Z);
}

// ------------------------------------------------------------------ which loop kernel runs
// Two families, one signature each (the direct solve has no iteration count to report; given the argument all the same, k_loop?_fdm<true>
// come out with another scalar register allocation).  which: 1 / 2 = first / second loop; own_lhs: the launch forms v = A zhat / t = A what
// itself (FLHS); early: it totals its per-block values itself (the early all-reduce: uniform grids only, so own_lhs holds); nblocks: of this launch.
typedef void (*LoopKernelFdm)(GridDev, Vecs, const SolverCtl *, double *, long, double *, LhsIn, const LoopSums *);
static LoopKernelFdm loop_kernel_fdm(int which, bool own_lhs) {  // block_solver 1: the direct block solve behind the loop
  if (which == 1) return own_lhs ? k_loop1_fdm<true> : k_loop1_fdm<false>;
  return own_lhs ? k_loop2_fdm<true> : k_loop2_fdm<false>;
}
typedef void (*LoopKernel)(GridDev, Vecs, const SolverCtl *, double *, long, double *, int *, LhsIn, const LoopSums *);
static LoopKernel loop_kernel(int which, int block_solver, bool own_lhs, bool early, int nblocks) {  // block_solver 0 / 2: the block CG behind the loop
  constexpr int P = kCgProduction;
#ifdef CUP3D_TESTING  // A/B of the occupancy of the production kernels, test builds only
  if (block_solver == 0 && !early) {
    const int five = debug_option("loop1_five_waves");  // 1 = always, 2 = never
    if (which == 1 && own_lhs && five) return five == 1 ? k_loop1_cg_w5<true, P, true> : k_loop1_cg<true, P, true>;
    if (which == 2 && !own_lhs && debug_option("loop2_four_waves")) return k_loop2_cg_w4<true, P, false>;
    const int five2 = debug_option("loop2_five_waves");  // 1 = always, 2 = never
    if (which == 2 && own_lhs && five2) return five2 == 1 ? k_loop2_cg_w5<true, P, true> : k_loop2_cg_w4<true, P, true>;
  }
#endif
  const bool fma = block_solver == 0;  // the production block CG; else (block_solver 2) the reference's association
  if (which == 1) {
    if (early) return fma ? k_loop1_cg_tot<true, P> : k_loop1_cg_tot<false, 0>;
    if (!fma) return own_lhs ? k_loop1_cg<false, 0, true> : k_loop1_cg<false, 0, false>;
    if (!own_lhs) return k_loop1_cg<true, P, false>;
    return nblocks >= kFiveWavesFrom ? k_loop1_cg_w5<true, P, true> : k_loop1_cg<true, P, true>;
  }
  // with the LHS inside, loop2_cg_body asks for 128 registers: 4 wavefronts per SIMD without spills (k_loop2_cg_w4; held to 96 it
  // spills 30 registers inside the plane loop); the production launch has a body of its own that fits 5 (k_loop2_cg_w5)
  if (early) return fma ? k_loop2_cg_tot<true, P> : k_loop2_cg_tot<false, 0>;
  if (!fma) return own_lhs ? k_loop2_cg_w4<false, 0, true> : k_loop2_cg<false, 0, false>;
  if (!own_lhs) return k_loop2_cg<true, P, false>;
  return nblocks >= kLoop2FiveWavesFrom ? k_loop2_cg_w5<true, P, true> : k_loop2_cg_w4<true, P, true>;
}

}  // namespace cup3d
