// Pressure Poisson solve and projection on the device.
//
//   cup3d_preconditioner   <- poisson_kernels::getZImplParallel      main.cpp:14704-14745
//   cup3d_poisson_solve    <- PoissonSolverAMR::solve                main.cpp:14363-14616
//   cup3d_pressure_project <- PressureProjection::operator()         main.cpp:15061-15160
//
// The solver is the reference's pipelined, preconditioned BiCGSTAB, restated step for
// step (same recurrences, same 50-iteration true-residual refresh, same breakdown
// restart, same x_opt bookkeeping, same stopping rule) with the vectors resident in
// HBM as flat [block][512] slabs -- which IS the block layout, so the reference's six
// scatter/gather copies per iteration (9372-9392, 9342-9363) do not exist here.  An
// iteration is two launches (LHS + vector loop + block CG each: k_loop1_cg, k_loop2_cg);
// the scalar recurrences live on the device (SolverCtl) and the host only watches; every
// 50th iteration is four launches of k_refresh; over ranks the all-reduces can start early.
// Elementwise updates keep the reference's association (no FMA contraction); only the
// summation ORDER of the dot products and of the block-CG inner products differs
// from the CPU, so pressure agrees to solver tolerance, not bitwise.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <utility>

#include "sim.hpp"
#include "tile.hpp"
#include "tile7.hpp"
// the device side, by subject: one translation unit (cQ, g_invD and the static helpers are shared), in dependency order
#include "poisson_block.hpp"    // cg_block, k_precond*, fdm_block, launch_precond*
#include "poisson_ctl.hpp"      // SolverCtl, ctl_step1 / ctl_step2, k_ctl_*
#include "poisson_totals.hpp"   // Arrive, DotsThen, LoopSums, k_sums_finish
#include "poisson_vector.hpp"   // Vecs, the plain vector kernels, Reducer
#include "poisson_loops.hpp"    // the fused loop kernels and which of them runs
#include "poisson_refresh.hpp"  // k_refresh, k_refresh_pointwise

namespace cup3d {

static int ensure_vectors(Sim *s) {
  int rc;
  if (!s->d_block_dots && (rc = s->d_block_dots.alloc_zeroed((size_t)7 * s->nb, stream(), s))) return rc;
  // Arrive: [dots | mean] x (n1 + n2 + 1) counters + 2 flags; (7 + 1) x (n1 + n2) partial sums.  Each allocation is guarded by its OWN
  // pointer (one guard over four allocations left the later ones null for ever when one of them failed once)
  {
    const size_t n1 = ((size_t)s->nb + 63) / 64, n2 = (n1 + 63) / 64, ncnt = 2 * (n1 + n2 + 1) + 2;
    if (!s->d_arrive_sums && (rc = s->d_arrive_sums.alloc_zeroed(8 * (n1 + n2) + 8, stream(), s))) return rc;
    if (!s->d_arrive && (rc = s->d_arrive.alloc_zeroed(ncnt, stream()))) { s->d_arrive.reset(); return rc; }  // never kept unzeroed
    if (!s->d_loop_sums && (rc = s->d_loop_sums.alloc(2))) return rc;
    if (!s->h_early_fail_dev) {
      if (!s->h_early_fail && (rc = s->h_early_fail.alloc(1, hipHostMallocMapped | hipHostMallocCoherent))) return rc;
      *s->h_early_fail = 0;
      if ((rc = s->h_early_fail.device_alias(&s->h_early_fail_dev))) return rc;
    }
  }
  if (!s->h_ctl_dev) {  // the solver's scalar struct (device) and the pinned ring its outcome reaches the host through; each guarded by itself
    if (!s->d_ctl && (rc = s->d_ctl.alloc(sizeof(SolverCtl)))) return rc;
    if (!s->h_ctl) {
      if ((rc = s->h_ctl.alloc(4 * sizeof(CtlSlot), hipHostMallocMapped | hipHostMallocCoherent))) return rc;
      memset(s->h_ctl, 0, 4 * sizeof(CtlSlot));
    }
    if ((rc = s->h_ctl.device_alias(&s->h_ctl_dev))) return rc;
  }
  if (s->sv[0]) return CUP3D_OK;
  for (int i = 0; i < NVEC; ++i)
    if ((rc = s->sv[i].alloc_zeroed((size_t)s->nvis * 512, stream(), s))) return rc;  // nvis: the LHS reads ghost blocks of any of them on a rank view
  return CUP3D_OK;
}

#define LAUNCH_VEC(kern, ...) hipLaunchKernelGGL(kern, dim3(G), dim3(256), 0, stream(), __VA_ARGS__)
// few-stream pointwise kernels without partial sums: these want the wide grid (0.88 vs 1.26 ms for k_loop1_phat at 512^3)
#define LAUNCH_VEC_S(kern, ...) hipLaunchKernelGGL(kern, dim3(Gs), dim3(256), 0, stream(), __VA_ARGS__)
#define TRY(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// the host waits for the outcome of a fused iteration: slot seq & 3 of the pinned ring carries `seq` once the struct is in place
static int wait_status(Sim *s, unsigned seq, SolverCtl *out) {
  const CtlSlot *sl = s->h_ctl.as<const CtlSlot>() + (seq & 3);
  const volatile unsigned *flag = &sl->seq;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 1; *flag != seq; ++spin) {
    __builtin_ia32_pause();
    if ((spin & 0x3fff) == 0) {  // every ~16k polls: have the streams drained (or failed) without the slot being written?
      if (s->h_early_fail && *(volatile unsigned *)s->h_early_fail) {
        set_error("BiCGSTAB: a device-side wait of the early all-reduce gave up after 10 s (%s): the loop kernel it waits for never delivered",
                  *(volatile unsigned *)s->h_early_fail == 1 ? "the communication stream waiting for the dot products" : "the corner block's wavefront waiting for the mean-constraint total");
        return CUP3D_ESTATE;
      }
      hipError_t e = hipStreamQuery(stream());
      if (e == hipSuccess && s->comm_stream) e = hipStreamQuery(s->comm_stream);
      if (e == hipSuccess) {
        if (*flag == seq) break;
        set_error("BiCGSTAB: the device finished without reporting iteration status %u", seq);
        return CUP3D_ESTATE;
      }
      if (e != hipErrorNotReady) return hip_fail(e, "hipStreamQuery", __FILE__, __LINE__);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  memcpy(out, (const void *)&sl->c, sizeof(SolverCtl));
  stats_host_wait(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return CUP3D_OK;
}

static long long wall_clock_ticks_per_ms() {  // wall_clock64 (100 MHz on CDNA3 / CDNA4)
  static const long long rate = [] {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0) return (long long)khz;
    return 100000LL;
  }();
  return rate;
}

// One solve: PoissonSolverAMR::solve, or with helm != nullptr DiffusionSolver::solve (main.cpp:6896-7146) -- the same routine on the
// Helmholtz operator of one velocity component, with no mean constraint and no cap on the breakdown restarts.
// Everything the steps of a solve share lives here; what only one mode needs stays local to that mode's function.
struct Solver {
  Sim *const s;
  const cup3d_poisson_params &P;
  const HelmholtzOp *const helm;
  const bool checksum;  // cup3d_poisson_path_checksum: no solve, one iteration's kernels on hand-made input (path_checksum())

  Vecs V;
  double *XB[2];  // the two x buffers; SolverCtl::xcur / xopt say which is which
  long N;
  unsigned G, Gs;  // grids of LAUNCH_VEC / LAUNCH_VEC_S
  GridDev gd;
  Reducer red;
  SolverCtl hs;  // the host's copy of the scalars: current whenever no fused iteration is in flight
  SolverCtl *d_ctl;
  CtlSlot *ring;
  double *sums;  // per-block sum(u h^3) of the block solves' output, for the mean-constraint row; nullptr: not wanted
  int *cg_it;
  unsigned *dots_flag, *mean_flag;  // early: raised when the dot products / the mean-constraint total of a loop are in device memory

  // what kind of solve this is: decided once, in setup()
  int mc;             // bMeanConstraint
  bool want_sums;     // the LHS takes its mean-constraint row from block sums the block solve leaves behind
  bool direct_solve;  // block_solver 1
  bool fuse;          // vector loop + block solve in one launch (k_loop1_cg / k_loop2_cg, k_loop?_fdm)
  bool flhs;          // ... which also forms v = A zhat / t = A what (uniform grids)
  bool flhs_ml;       // ... on a multi-level mesh for the blocks without a coarse/fine face (A/B, test builds)
  bool fuse_refresh;  // the every-50th iteration as four launches of k_refresh
  bool direct;        // the totals reach the host without an all-reduce
  bool split;         // several ranks: inner blocks while the face slabs travel, then the rest
  bool early;         // several ranks: the all-reduces start when the last block leaves its vector phase

  // the mean-constraint total of `what` for the first fused loop (FLHS): d_red[7] after a fused iteration (k_sums_finish<7, true>),
  // d_red[8] after a host-driven LHS(WHAT, T_) (k_mean_finish inside launch_lhs); of `zhat` for the second loop it is d_red[2]
  const double *what_total;
  bool first_after_host;  // the next fused iteration follows a host-driven LHS(WHAT, T_): its total is complete before the launch

  // what cup3d_debug_solver_state reports besides the scalars (test builds; nothing in the release build): q.y, y.y of the last
  // iteration where the host saw them (host-driven iterations: the fused ones step omega on the device and the second loop's totals
  // take their place in d_red), and the iteration count at the last restart
#ifdef CUP3D_TESTING
  double dbg_qy[2] = {NAN, NAN};
  int dbg_restart_iter = -1;
  void dbg_first_totals(const double *t) { dbg_qy[0] = t ? t[0] : NAN; dbg_qy[1] = t ? t[1] : NAN; }
  void dbg_restarted() { dbg_restart_iter = hs.iter; }
  int dbg_save() {
    auto &D = s->dbg_solver;
    const double io[16] = {hs.alpha, hs.beta, hs.omega, hs.r0r_prev, hs.norm, hs.init_norm, hs.min_norm, hs.tol, hs.tol_rel, (double)hs.state,
                           (double)hs.restarts, (double)hs.max_restarts, (double)hs.xcur, (double)hs.xopt, (double)hs.iter,
                           hs.iter > 0 && dbg_restart_iter == hs.iter ? 1.0 : 0.0};
    memcpy(D.io, io, sizeof io);
    CUP3D_HIP(hipStreamSynchronize(stream()));
    CUP3D_HIP(hipMemcpy(D.totals, s->d_red + kRedDots, 7 * sizeof(double), hipMemcpyDeviceToHost));
    D.totals[7] = dbg_qy[0]; D.totals[8] = dbg_qy[1];
    D.valid = true;
    return CUP3D_OK;
  }
#else
  void dbg_first_totals(const double *) {}
  void dbg_restarted() {}
  int dbg_save() { return CUP3D_OK; }
#endif

  Solver(Sim *sim, const cup3d_poisson_params &params, const HelmholtzOp *op, bool path_checksum_mode)
      : s(sim), P(params), helm(op), checksum(path_checksum_mode), red{sim} {}

  int LHS(int in, int out) {  // _lhs, 9365-9393 / 6836-6875
    return helm ? launch_lhs_diffusion(s, V.v[in], V.v[out], *helm) : launch_lhs(s, V.v[in], V.v[out], mc);
  }
  int PRE(int in, int out) {  // _preconditioner, 9334-9364 / 6804-6835
    return helm ? launch_precond_diffusion(s, V.v[in], V.v[out], *helm) : launch_precond(s, V.v[in], V.v[out], mc > 0 && mc <= 2);
  }
  // host-driven launches address x through V: v[X_] = the buffer the next update of x writes, xin = the one that holds x
  void x_ptrs() { const int xw = ctl_xwrite(hs); V.v[X_] = XB[xw]; V.v[XOPT] = XB[1 - xw]; V.xin = XB[hs.xcur]; }
  int lhs_mode() const { return mc > 2 ? 3 : mc; }  // LhsIn::mode of a kernel that forms the LHS itself

  // buffers, and every decision about the route this solve takes
  int setup() {
    TRY(ensure_vectors(s));
    s->block_solver = P.block_solver;
    for (int i = 0; i < NVEC; ++i) V.v[i] = s->sv[i];
    XB[0] = s->sv[X_]; XB[1] = s->sv[XOPT];
    N = s->nb * 512L;
    G = vec_groups(N); Gs = vec_groups_simple(N);
    mc = helm ? 0 : P.mean_constraint;
    want_sums = mc > 0 && mc <= 2;
    const bool block_cg = P.block_solver == 0 || P.block_solver == 2;
    direct_solve = P.block_solver == 1;
    // vector loop + block CG in one launch (k_loop1_cg / k_loop2_cg): the production path of the pressure solver with the block CG
    // block_solver 1 (the direct block solve, `alt`): the same two kernels with fdm_block behind the loops ("no_fuse_fdm": A/B, round 3's launches)
    fuse = !helm && (block_cg || (direct_solve && !debug_option("no_fuse_fdm"))) && !debug_option("no_fuse");
    if (fuse && direct_solve) TRY(fdm_setup());
    sums = want_sums ? s->d_partials + (size_t)s->max_groups * 8 : nullptr;
    cg_it = profile_on() ? cg_iters_buffer(s) : nullptr;
    gd = s->gdev();
    d_ctl = s->d_ctl.as<SolverCtl>();
    ring = reinterpret_cast<CtlSlot *>(s->h_ctl_dev);
    direct = red.direct();
    split = s->grid->nranks > 1;
    // FLHS: v = A zhat and t = A what are formed inside the loop kernels (uniform grids; on multi-level meshes the LHS needs the
    // coarse/fine ghost slabs and the flux correction, so it stays a launch of its own)
    flhs = fuse && !s->grid->multilevel && !debug_option("no_fuse_lhs");
    // A/B, test builds only ("fuse_lhs_ml"): on a multi-level mesh (one rank) the blocks none of whose six faces is a coarse/fine interface
    // take the FLHS kernels too, and only the interface blocks keep k_lhs + ghost slabs + flux correction (launch_lhs on the interface
    // list).  Bit-identical t and v -- and NOT faster: each loop kernel becomes two launches (plain list, interface list), which costs what
    // the smaller k_lhs saves (1.574 -> 1.567 ms per iteration on the 39 369-block mesh of bench.py --amr, profiles/r04).  Measured, kept
    // out of the production path.
    flhs_ml = fuse && s->grid->multilevel && s->grid->nranks == 1 && s->n_plain > 0 && !debug_option("no_fuse_lhs") && debug_option("fuse_lhs_ml");
    // the every-50th iteration as four launches of k_refresh + two of k_refresh_pointwise (see there): uniform grids, one rank, block CG
    fuse_refresh = flhs && !checksum && s->grid->nranks == 1 && direct && block_cg && !debug_option("no_fuse_refresh");
    // Several ranks.  DEFAULT: when the loop kernel has ended, one all-reduce of its K totals (+ the mean-constraint total: two RCCL calls
    // per iteration where the reference makes four) on the communication stream, the recurrence step behind it, the next loop kernel
    // waits -- both all-reduces of an iteration are exposed.  EARLY (process-per-rank transports, CUP3D_EARLY_ALLREDUCE / "early_allreduce"):
    // the all-reduce of the dot products starts when the LAST BLOCK LEAVES ITS VECTOR PHASE (k_wait_totals holds the communication
    // stream until DotsThen raises the flag), i.e. it runs under the block solves of the kernel's last round; the mean-constraint total,
    // which exists only when the kernel has ended, follows in an all-reduce of its own that nobody waits for on the host or on the
    // compute stream: the ONE wavefront that needs it -- the corner block's, mode 1 -- waits for its flag inside the next loop kernel.
    // (mode 2 adds the total to every cell: there the next kernel as a whole waits, and early buys only the first half.)
    // What MPI_Iallreduce hides behind the preconditioner in the reference (14486-14490, 14546-14550) is hidden behind it here again.
    // The environment is read at every solve (a getenv against a solve of milliseconds): bench.py --gpus N times its alt_early_allreduce
    // region in the same process, after the default order has produced `value`.
    // (uniform grids only: on multi-level meshes the LHS is a launch of its own between the loops and reads the mean-constraint total itself)
    const char *const env = getenv("CUP3D_EARLY_ALLREDUCE");
    early = !direct && flhs && block_cg && comm() && !virtual_ranks() && !host_transport() && scalar_stream(s) != stream() &&
            ((env && atoi(env) != 0) || debug_option("early_allreduce"));
    const long n1 = (s->nb + 63) / 64, n2 = (n1 + 63) / 64;  // the two flags sit behind the counters of Arrive (ensure_vectors)
    dots_flag = s->d_arrive + 2 * (n1 + n2 + 1);
    mean_flag = dots_flag + 1;

    memset(&hs, 0, sizeof hs);
    hs.tol = P.tol; hs.tol_rel = P.tol_rel;
    hs.max_restarts = helm ? 0x7fffffff : P.max_restarts;
    hs.min_norm = 1e50;
    hs.xcur = 0; hs.xopt = -1;
    hs.state = kRun;
    x_ptrs();
    what_total = s->d_red + kRedMeanLhs;
    first_after_host = true;
    return CUP3D_OK;
  }

  // b, r, x, r0, rhat, w, what, t and the first alpha (14404-14443)
  int init() {
    const double eps = 1e-100;
    if ((mc == 1 || mc > 2) && s->grid->corner_slot >= 0)  // rhs(0,0,0) = 0, 14404-14407
      hipLaunchKernelGGL(k_set_one, dim3(1), dim3(1), 0, stream(), s->lhs, (size_t)s->grid->corner_slot * 512, 0.0);
    { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_solver_init, V, s->lhs, s->pres, N); }
    TRY(LHS(X_, R0));
    { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_resid0, V, N); }
    TRY(PRE(R0, RHAT)); TRY(LHS(RHAT, W_)); TRY(PRE(W_, WHAT)); TRY(LHS(WHAT, T_));
    { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC(k_dots_r0, V, N, red.out()); }
    TRY(red.begin(2)); TRY(red.wait());
    hs.alpha = s->h_red[0] / (s->h_red[1] + eps);  // 14443
    hs.r0r_prev = s->h_red[0];
    hs.norm = hs.init_norm = std::sqrt(s->h_red[0]);
    return early_setup();
  }

  // early: clean counters, and the two loops' LoopSums -- constant over this solve -- in device memory
  int early_setup() {
    if (!early) return CUP3D_OK;
    const long n1 = (s->nb + 63) / 64, n2 = (n1 + 63) / 64;
    unsigned *const cnt = s->d_arrive;
    // (a solve that ended in an error half way through a loop may have left tickets behind; the two flags behind the counters only ever grow;
    //  only the early kernels take tickets)
    CUP3D_HIP(hipMemsetAsync(cnt, 0, (size_t)(2 * (n1 + n2 + 1)) * sizeof(unsigned), stream()));
    auto arrive_args = [&](int which, const double *vals, double *out) {  // which 0: the dot products, 1: the block sums of the mean constraint
      double *gs = s->d_arrive_sums + (which ? 7 * (n1 + n2) : 0);
      unsigned *c = cnt + which * (n1 + n2 + 1);
      return Arrive{vals, gs, gs + (which ? 1 : 7) * n1, c, c + n1, c + n1 + n2, (long)s->nb, n1, n2, out};
    };
    LoopSums Z[2];
    for (int which = 1; which <= 2; ++which) {
      Z[which - 1].dots = arrive_args(0, s->d_block_dots, s->d_red + kRedDots);
      Z[which - 1].mean = arrive_args(1, sums, s->d_red + kRedEarlyMean + (which - 1));
      // (over ranks the struct is stepped behind the all-reduce, k_ctl_step; the path checksum wants totals only, nothing stepped or flagged)
      Z[which - 1].then = DotsThen{d_ctl, ring, which, 0, checksum ? nullptr : dots_flag};
    }
    hipLaunchKernelGGL(k_set_loop_sums, dim3(1), dim3(1), 0, stream(), s->d_loop_sums, Z[0], Z[1]);
    CUP3D_HIP(hipGetLastError());
    return CUP3D_OK;
  }

  // the restart of 14567-14593 / 7096-7120 (the breakdown was detected, and counted, by ctl_step2)
  int restart() {
    const double eps = 1e-100;
    { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_copy, V.v[R_], V.v[R0], N); }
    TRY(PRE(R0, RHAT)); TRY(LHS(RHAT, W_));
    { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC(k_dots_r0, V, N, red.out()); }
    TRY(red.begin(2));
    TRY(PRE(W_, WHAT)); TRY(LHS(WHAT, T_));
    TRY(red.wait());
    hs.alpha = s->h_red[0] / (s->h_red[1] + eps);
    hs.r0r_prev = s->h_red[0];
    hs.beta = 0.0;
    hs.omega = 0.0;
    hs.state = kRun;
    what_total = s->d_red + kRedMeanLhs;
    first_after_host = true;
    dbg_restarted();
    return CUP3D_OK;
  }

  // one iteration driven by the host: every 50th one (s, z and the true residual recomputed through _lhs), and all of them for the
  // block solvers without a fused kernel and for the Helmholtz solves
  int host_iteration(int k) {
    x_ptrs();
    if (k % 50 != 0) {
      ProfileScope ps("bicgstab_loop1");
      if (!debug_option("loops_no_nt")) LAUNCH_VEC(k_loop1<true>, V, N, hs.alpha, hs.beta, hs.omega, red.out());
      else LAUNCH_VEC(k_loop1<false>, V, N, hs.alpha, hs.beta, hs.omega, red.out());
    } else {
      { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_loop1_phat, V, N, hs.beta, hs.omega); }
      TRY(LHS(PHAT, S_)); TRY(PRE(S_, SHAT)); TRY(LHS(SHAT, Z_));
      { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC(k_loop1_tail, V, N, hs.alpha, red.out()); }
    }
    TRY(red.begin(2));         // MPI_Iallreduce(2), 14486
    TRY(PRE(Z_, ZHAT));        // overlapped with the reduction read-back, 14488-14489
    TRY(LHS(ZHAT, V_));
    TRY(red.wait());
    dbg_first_totals(s->h_red);
    ctl_step1(hs, s->h_red);   // 14493
    if (k % 50 != 0) {
      ProfileScope ps("bicgstab_loop2");
      if (!debug_option("loops_no_nt")) LAUNCH_VEC(k_loop2<true>, V, N, hs.alpha, hs.omega, red.out());
      else LAUNCH_VEC(k_loop2<false>, V, N, hs.alpha, hs.omega, red.out());
    } else {
      { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_loop2_x, V, N, hs.alpha, hs.omega); }
      TRY(LHS(X_, R_));        // v[X_] is where x was just written
      { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_true_resid, V, N); }
      TRY(PRE(R_, RHAT)); TRY(LHS(RHAT, W_));
      { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC(k_dots7, V, N, red.out()); }
    }
    TRY(red.begin(7));         // MPI_Iallreduce(7), 14546
    TRY(PRE(W_, WHAT));        // 14548-14549
    TRY(LHS(WHAT, T_));
    TRY(red.wait());
    ctl_step2(hs, s->h_red);   // 14558-14566, 14594-14601 (moves xcur to the buffer just written)
    if (hs.state == kRestart) TRY(restart());
    what_total = s->d_red + kRedMeanLhs;  // LHS(WHAT, T_) left sum(what h^3) there (k_mean_finish)
    first_after_host = true;
    return CUP3D_OK;
  }

  // one launch of k_refresh; the total of its input's h^3-weighted sum is in *L.total
  int refresh(int kind, const LhsIn &L) {
    ProfileScope ps("bicgstab_refresh");
    const GridDev g = s->gdev();
    hipLaunchKernelGGL(refresh_kernel(P.block_solver, kind), dim3(launch_groups(g)), dim3(64), 0, stream(), g, V, hs.alpha, (const double *)V.v[X_], s->d_block_dots,
                       (long)s->nb, sums, cg_it, L);
    CUP3D_HIP(hipGetLastError());
    s->sums_of = nullptr;
    s->mean_total_of = nullptr;
    return CUP3D_OK;
  }
  // The dot products of a refresh are summed by the kernels of the launch-by-launch form, in THEIR order (grid-stride partials: k_dots2 =
  // k_loop1_tail's two sums, k_dots7 itself), from the vectors k_refresh stored -- 0.35 + 1.27 ms per refresh for a solver that is bit for
  // bit the launch-by-launch one: the same omega, alpha, iterates, iteration and restart counts ("no_fuse_refresh", tests).  (k_refresh also
  // leaves per-block dot products behind, which this flow does not use: measured with them -- another order -- the iteration is 0.06 ms
  // cheaper and the driver's window takes 179 iterations per step instead of 171, profiles/r05.)
  int refresh_totals(int K) {
    {
      ProfileScope ps("bicgstab_vector");
      if (K == 2) LAUNCH_VEC(k_dots2, V, N, red.out());
      else LAUNCH_VEC(k_dots7, V, N, red.out());
      CUP3D_HIP(hipGetLastError());
    }
    TRY(red.begin(K));
    if (want_sums) TRY(launch_mean_total(s));
    return CUP3D_OK;
  }
  // the every-50th iteration as four launches of k_refresh + two of k_refresh_pointwise
  int refresh_iteration() {
    x_ptrs();
    const GridDev g = s->gdev();
    const dim3 GG(launch_groups(g));
    const double *const tot = s->d_red + kRedMeanLhs;
    const LhsIn Lin{s->halo_recv, tot, lhs_mode(), s->grid->corner_slot, 0, g_invD, nullptr, 0, nullptr};
    { ProfileScope ps("bicgstab_vector"); hipLaunchKernelGGL(k_refresh_pointwise<0>, GG, dim3(256), 0, stream(), g, V, hs.beta, hs.omega, sums); }  // phat, 14467
    if (want_sums) TRY(launch_mean_total(s));
    TRY(refresh(kRefS, Lin));              // s = A phat, shat = M^-1 s
    if (want_sums) TRY(launch_mean_total(s));
    TRY(refresh(kRefZ, Lin));              // z = A shat; q, qhat, y; q.y, y.y; zhat = M^-1 z
    TRY(refresh_totals(2));                // MPI_Iallreduce(2), 14486
    if (want_sums) { s->mean_total_of = V.v[ZHAT]; s->mean_total = tot; }
    TRY(LHS(ZHAT, V_));                    // v = A zhat, 14489
    TRY(red.wait());
    dbg_first_totals(s->h_red);
    ctl_step1(hs, s->h_red);               // 14493
    { ProfileScope ps("bicgstab_vector"); hipLaunchKernelGGL(k_refresh_pointwise<1>, GG, dim3(256), 0, stream(), g, V, hs.alpha, hs.omega, sums); }  // x, 14518
    if (want_sums) TRY(launch_mean_total(s));
    TRY(refresh(kRefR, Lin));              // r = b - A x, rhat = M^-1 r
    if (want_sums) TRY(launch_mean_total(s));
    TRY(refresh(kRefW, Lin));              // w = A rhat; the seven dot products; what = M^-1 w
    TRY(refresh_totals(7));                // MPI_Iallreduce(7), 14546
    TRY(red.wait());                       // (t = A what, 14549: the next iteration is a fused one and forms it from the tile of what)
    ctl_step2(hs, s->h_red);               // 14558-14566, 14594-14601 (moves xcur to the buffer just written)
    if (want_sums) { s->mean_total_of = V.v[WHAT]; s->mean_total = tot; }
    what_total = tot;                      // sum(what h^3): k_mean_finish left it in d_red[kRedMeanLhs], where the unfused LHS(WHAT, T_) leaves it
    first_after_host = true;
    if (hs.state == kRestart) TRY(restart());
    return CUP3D_OK;
  }

  // one loop kernel (loop_kernel() says which); over ranks: inner blocks while u's face slabs travel, then the rest
  int launch_loop(int which, const double *u, const LhsIn &L) {
    const LoopSums *const Z = s->d_loop_sums + (which - 1);
    if (flhs && split) TRY(halo_begin(s, u, 1, 1));
    for (int pass = 0; pass < ((flhs && split) || flhs_ml ? 2 : 1); ++pass) {
      const GridDev gp = flhs_ml ? (pass == 0 ? s->gdev_list(s->d_plain_list, s->n_plain) : s->gdev_list(s->d_iface_list, s->n_iface))
                                 : (flhs && split ? s->gdev(pass == 1, pass == 0) : gd);
      const bool own_lhs = flhs || (flhs_ml && pass == 0);  // does this launch form the LHS itself?
      if (pass == 1 && !flhs_ml) TRY(halo_finish(s));
      if (gp.nblocks == 0) continue;
      ProfileScope ps(direct_solve ? (which == 1 ? "bicgstab_loop1_fdm" : "bicgstab_loop2_fdm") : (which == 1 ? "bicgstab_loop1_cg" : "bicgstab_loop2_cg"));
      const dim3 GG(launch_groups(gp)), BB(64);
      if (direct_solve) hipLaunchKernelGGL(loop_kernel_fdm(which, own_lhs), GG, BB, 0, stream(), gp, V, (const SolverCtl *)d_ctl, s->d_block_dots, (long)s->nb, sums, L, Z);
      else hipLaunchKernelGGL(loop_kernel(which, P.block_solver, own_lhs, early, gp.nblocks), GG, BB, 0, stream(), gp, V, (const SolverCtl *)d_ctl, s->d_block_dots, (long)s->nb, sums, cg_it, L, Z);
      CUP3D_HIP(hipGetLastError());
    }
    return CUP3D_OK;
  }

  // the totals of the loop just enqueued (-> all ranks) -> the struct.  K = 2 / 7 dot products, step = 1 / 2 = which loop
  int after_loop(int K, int step, unsigned seq) {
    if (!early) {  // DEFAULT: one launch totals the K (+1) block-wise sums; on one rank its last workgroup steps the struct as well
      ProfileScope ps("bicgstab_dots_finish");
      const RedOut ro{s->d_partials, s->d_counters, s->d_red, nullptr, nullptr, 0u};
      const CtlThen then{d_ctl, ring, direct ? step : 0};
      const dim3 SG(debug_option("sums_groups") > 0 ? debug_option("sums_groups") : sums_groups(s->nb));
      hipLaunchKernelGGL(sums_kernel(K, want_sums), SG, dim3(256), 0, stream(), (const double *)s->d_block_dots, (long)s->nb, ro, (const double *)sums, then);
      CUP3D_HIP(hipGetLastError());
    }
    if (direct) return CUP3D_OK;
    hipStream_t cs = scalar_stream(s);
    const unsigned flag_value = seq * 2 + (unsigned)(step - 1);
    auto allreduce_and_step = [&](int count) -> int {  // on the communication stream: the totals over ranks, the recurrence step, the event the compute stream waits for
      TRY(allreduce(s, s->d_red, count, false, cs));
      hipLaunchKernelGGL(ctl_step_kernel(step), dim3(1), dim3(1), 0, cs, d_ctl, (const double *)s->d_red, ring);
      CUP3D_HIP(hipGetLastError());
      CUP3D_HIP(hipEventRecord(s->ev_a, cs));
      return CUP3D_OK;
    };
    if (!early) {
      if (cs != stream()) {
        CUP3D_HIP(hipEventRecord(s->ev_b, stream()));
        CUP3D_HIP(hipStreamWaitEvent(cs, s->ev_b, 0));
      }
      ProfileScope pc("comm_allreduce", cs);  // the all-reduce and the recurrence step behind it, as the communication stream sees them
      return allreduce_and_step(K + (want_sums ? 1 : 0));
    }
    if (s->nb == 0) {  // a rank without blocks launched nothing: its contribution is zero, and nobody but the host can raise the flag
      CUP3D_HIP(hipMemsetAsync(s->d_red + kRedDots, 0, (size_t)(K + 1) * sizeof(double), stream()));
      CUP3D_HIP(hipMemsetAsync(s->d_red + kRedEarlyMean, 0, 2 * sizeof(double), stream()));
      hipLaunchKernelGGL(k_raise, dim3(1), dim3(1), 0, stream(), dots_flag, flag_value);
    }
    hipLaunchKernelGGL(k_wait_totals, dim3(1), dim3(1), 0, cs, (const SolverCtl *)d_ctl, (const unsigned *)dots_flag, flag_value, s->h_early_fail_dev, 10000 * wall_clock_ticks_per_ms());
    {
      ProfileScope pc("comm_allreduce", cs);  // (behind the wait for the totals: the all-reduce and the step, not the time the loop kernel took to deliver)
      TRY(allreduce_and_step(K));
    }
    if (want_sums) {  // the mean-constraint total: complete when the kernel ends
      CUP3D_HIP(hipEventRecord(s->ev_b, stream()));
      CUP3D_HIP(hipStreamWaitEvent(cs, s->ev_b, 0));
      ProfileScope pc("comm_allreduce_mean", cs);
      TRY(allreduce(s, s->d_red + kRedEarlyMean + (step - 1), 1, false, cs));
      hipLaunchKernelGGL(k_raise, dim3(1), dim3(1), 0, cs, mean_flag, flag_value);
      CUP3D_HIP(hipGetLastError());
      if (mc == 2) CUP3D_HIP(hipEventRecord(s->ev_m, cs));  // every cell takes the total: the next kernel as a whole waits (scalars_ready)
    }
    return CUP3D_OK;
  }

  // a run of fused iterations starts (or starts again after a restart): the host's scalars go to the device, numbered for the next iteration.
  // early: nothing orders the communication stream behind the loop kernel any more (that is the point), so it must be ordered behind this
  // k_ctl_set explicitly: k_wait_totals and k_ctl_step read the struct (an unordered k_wait_totals saw the state of the PREVIOUS run -- kDone --
  // returned at once, and the all-reduce took stale totals: 1000 iterations without converging)
  int ctl_start() {
    hs.seq = s->ctl_seq + 1;  // the number the next enqueued iteration gets
    hipLaunchKernelGGL(k_ctl_set, dim3(1), dim3(1), 0, stream(), d_ctl, hs);
    if (!early) return CUP3D_OK;
    CUP3D_HIP(hipEventRecord(s->ev_b, stream()));
    CUP3D_HIP(hipStreamWaitEvent(scalar_stream(s), s->ev_b, 0));
    return CUP3D_OK;
  }
  // the compute stream waits for the struct stepped on the communication stream
  int scalars_ready() {
    if (!direct && scalar_stream(s) != stream()) {
      ProfileScope pw("comm_exposed_scalar_wait");  // compute stream idle until the all-reduced scalars are stepped (the exposed part of the all-reduce)
      CUP3D_HIP(hipStreamWaitEvent(stream(), s->ev_a, 0));
      if (early && want_sums && mc == 2) CUP3D_HIP(hipStreamWaitEvent(stream(), s->ev_m, 0));
    }
    return CUP3D_OK;
  }

  // one fused iteration, enqueued without waiting for anything: both loop kernels take their scalars from d_ctl
  int enqueue_fused(unsigned seq) {
    V.v[X_] = XB[0]; V.v[XOPT] = XB[1];  // fixed roles: the kernels pick by SolverCtl::xcur / xopt
    const int mode = !(flhs || flhs_ml) ? -1 : lhs_mode();
    const int prio = debug_option("loop_prio") ? debug_option("loop_prio") - 1 : kLoopPrio;  // tuning: option value = priority + 1
    // the mean-constraint row inside the kernels belongs to the corner block only if that block forms its own LHS
    const int corner_in = (flhs || (flhs_ml && s->corner_is_plain)) ? s->grid->corner_slot : -1;
    auto LHS_IFACE = [&](int in, int out) { return launch_lhs(s, V.v[in], V.v[out], mc, s->d_iface_list, s->n_iface); };
    // early all-reduce: the mean-constraint totals arrive in slots of their own behind a flag (after_loop); LhsIn::mean_wait = what the flag
    // must have reached before the corner block's wavefront may read the total
    const bool em = early && want_sums;
    const double *const total1 = em && !first_after_host ? s->d_red + kRedEarlyMean + 1 : what_total;
    const double *const total2 = em ? s->d_red + kRedEarlyMean : s->d_red + kRedDots + 2;
    TRY(launch_loop(1, V.v[WHAT], LhsIn{s->halo_recv, total1, mode, corner_in, prio, g_invD, em && !first_after_host ? mean_flag : nullptr, 1, s->h_early_fail_dev}));  // (t = A what,) loop 1, zhat = M^-1 z
    s->sums_of = want_sums ? V.v[ZHAT] : nullptr;
    TRY(after_loop(2, 1, seq));
    if (want_sums) { s->mean_total_of = V.v[ZHAT]; s->mean_total = total2; }
    if (flhs_ml) TRY(LHS_IFACE(ZHAT, V_));
    else if (!flhs) TRY(LHS(ZHAT, V_));
    TRY(scalars_ready());
    TRY(launch_loop(2, V.v[ZHAT], LhsIn{s->halo_recv, total2, mode, corner_in, prio, g_invD, em ? mean_flag : nullptr, 2, s->h_early_fail_dev}));  // (v = A zhat,) loop 2, what = M^-1 w
    s->sums_of = want_sums ? V.v[WHAT] : nullptr;
    TRY(after_loop(7, 2, seq));
    what_total = em ? s->d_red + kRedEarlyMean + 1 : s->d_red + kRedDots + 7;
    first_after_host = false;
    if (want_sums) { s->mean_total_of = V.v[WHAT]; s->mean_total = what_total; }
    if (flhs_ml) TRY(LHS_IFACE(WHAT, T_));  // t of the interface blocks for the next first loop; the others form theirs in that kernel
    else if (!flhs) TRY(LHS(WHAT, T_));
    TRY(scalars_ready());
    return CUP3D_OK;
  }

  // the iterations: host-driven ones one at a time, fused ones in runs the host watches from one iteration ahead
  int run() {
    int k = 0;
    while (k < P.max_iter && hs.state != kDone) {
      if (!fuse || k % 50 == 0) {
        TRY(fuse_refresh ? refresh_iteration() : host_iteration(k));
        ++k;
        continue;
      }
      // a run of fused iterations, up to the next multiple of 50: the host stays one iteration ahead of the device
      hs.state = kRun;
      TRY(ctl_start());
      int enq = k;  // next iteration to enqueue; k = next iteration whose outcome the host has not seen
      unsigned seq_of[2] = {0, 0};
      for (;;) {
        while (enq < P.max_iter && enq % 50 != 0 && enq - k < 2) {
          seq_of[enq & 1] = ++s->ctl_seq;
          TRY(enqueue_fused(seq_of[enq & 1]));
          ++enq;
        }
        if (k == enq) break;  // nothing in flight: a host iteration is next, or the cap is reached
        TRY(wait_status(s, seq_of[k & 1], &hs));
        dbg_first_totals(nullptr);
        ++k;
        if (hs.state == kDone) break;
        if (hs.state == kRestart) {  // what was enqueued ahead returned at once (state != kRun on the device)
          enq = k;
          x_ptrs();
          TRY(restart());
          TRY(ctl_start());
        }
      }
    }
    return CUP3D_OK;
  }

  // pres = x_opt, or the last iterate if none was recorded (14605-14615)
  int finish(cup3d_poisson_result *res) {
    const bool use_xopt = hs.xopt >= 0;
    { ProfileScope ps("bicgstab_vector"); LAUNCH_VEC_S(k_copy, XB[use_xopt ? hs.xopt : hs.xcur], s->pres, N); }
    CUP3D_HIP(hipGetLastError());
    stats_solver_iterations(hs.iter);
    if (res) {
      res->iterations = hs.iter;
      res->restarts = hs.restarts;
      res->norm0 = hs.init_norm;
      res->norm = hs.norm;
      res->used_xopt = use_xopt;
    }
    return dbg_save();
  }

  // cup3d_poisson_path_checksum: the work vectors are filled with a function of the global cell index, the scalars are set by hand and ONE
  // iteration's kernels run as they do inside a solve; sc[NVEC] receives the vectors' wrapping sums.
  // Every vector = a function of (vector, level, global cell index): the same cells hold the same bits however the blocks are spread over
  // ranks.  alpha, beta, omega by hand: no dot product (whose rounding depends on the partition) enters the update.
  int checksum_iteration(const int32_t *d_index, const int32_t *d_level, unsigned long long *sc) {
    for (int i = 0; i < NVEC; ++i) hipLaunchKernelGGL(k_selfcheck_fill, dim3((unsigned)s->nb), dim3(256), 0, stream(), s->sv[i], i, d_index, d_level, s->grid->level);
    hs.alpha = 0.75; hs.beta = 0.5; hs.omega = 0.625;  // exact in binary
    hs.xcur = 0; hs.xopt = -1; hs.state = kRun;
    hipLaunchKernelGGL(k_ctl_set, dim3(1), dim3(1), 0, stream(), d_ctl, hs);
    hipLaunchKernelGGL(k_set_one, dim3(1), dim3(1), 0, stream(), s->d_red, (size_t)kRedMeanLhs, 0.375);  // the mean-constraint total, by hand as well
    CUP3D_HIP(hipGetLastError());
    V.v[X_] = XB[0]; V.v[XOPT] = XB[1]; V.xin = XB[0];
    // with the LHS inside the loop kernels the mean-constraint row takes the hand-set total; the stand-alone LHS would reduce the
    // field for it (partition-dependent rounding), so there the row is left out: mode 0 gives the same bits on both routes
    const int mode = flhs ? lhs_mode() : (flhs_ml ? 0 : -1);
    const LhsIn L{s->halo_recv, s->d_red + kRedMeanLhs, mode, s->grid->corner_slot, kLoopPrio, g_invD, nullptr, 0, nullptr};
    auto LHS0 = [&](int in, int out) {  // (multi-level, one rank: the interface blocks only -- the plain ones form theirs in the loop kernels)
      return flhs_ml ? launch_lhs(s, V.v[in], V.v[out], 0, s->d_iface_list, s->n_iface) : launch_lhs(s, V.v[in], V.v[out], 0);
    };
    if (!flhs) TRY(LHS0(WHAT, T_));
    TRY(launch_loop(1, V.v[WHAT], L));
    if (!flhs) TRY(LHS0(ZHAT, V_));
    TRY(launch_loop(2, V.v[ZHAT], L));
    for (int i = 0; i < NVEC; ++i) TRY(checksum_array(s, s->sv[i], N, &sc[i]));
    return CUP3D_OK;
  }
  int path_checksum(unsigned long long *sc) {
    if (!fuse) { set_error("cup3d_poisson_path_checksum: block_solver %d has no fused loop kernels (0, 1 and 2 do)", P.block_solver); return CUP3D_EINVAL; }
    TRY(early_setup());
    Dev<int32_t> d_index, d_level;  // the blocks' positions and levels, for k_selfcheck_fill
    int rc = d_index.upload(s->grid->index.data(), (size_t)s->nb * 3, stream(), IfEmpty::null);
    if (!rc && s->grid->multilevel) rc = d_level.upload(s->grid->blevel.data(), (size_t)s->nb, stream(), IfEmpty::null);
    if (!rc) rc = checksum_iteration(d_index, d_level, sc);
    (void)hipStreamSynchronize(stream());  // the tables are freed on return
    return rc;
  }
};

static int solve(Sim *s, const cup3d_poisson_params &P, cup3d_poisson_result *res, const HelmholtzOp *helm = nullptr, unsigned long long *sc = nullptr) {
  Solver S(s, P, helm, sc != nullptr);
  TRY(S.setup());
  if (sc) return S.path_checksum(sc);
  TRY(S.init());
  TRY(S.run());
  return S.finish(res);
}

int solve_helmholtz(Sim *s, const cup3d_poisson_params &P, cup3d_poisson_result *res, const HelmholtzOp &op) { return solve(s, P, res, &op); }

}  // namespace cup3d

using namespace cup3d;

extern "C" {

__attribute__((visibility("hidden"))) int cup3d_grad_p_update(cup3d_sim_t *h, double dt);  // stencil.hip; not exported

void cup3d_poisson_default_params(cup3d_poisson_params *p) {
  if (!p) return;
  p->tol = 1e-6; p->tol_rel = 1e-4; p->mean_constraint = 1; p->max_iter = 1000; p->max_restarts = 100; p->block_solver = 0;
}

// MEASUREMENT SUPPORT: CG iterations of the last block-CG launch made while cup3d_profile_enable(1) was on, summed over the blocks
int cup3d_profile_block_cg_iterations(cup3d_sim_t *h, long *total, long *nblocks) {
  if (!h || !total || !nblocks) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  *total = 0;
  *nblocks = 0;
  if (!s->d_cg_iters) return CUP3D_OK;
  std::vector<int> v((size_t)s->nb);
  CUP3D_HIP(hipMemcpy(v.data(), s->d_cg_iters, v.size() * sizeof(int), hipMemcpyDeviceToHost));
  long t = 0;
  for (int x : v) t += x;
  *total = t;
  *nblocks = (long)s->nb;
  return CUP3D_OK;
}

// TEST SUPPORT (no GPU needed): the scalar recurrences of the solver, host side of the one pair of functions the device runs too.
// io[16] = alpha, beta, omega, r0r_prev, norm, init_norm, min_norm, tol, tol_rel, state, restarts, max_restarts, xcur, xopt, iter, (unused);
// step 1: totals[2] = q.y, y.y (main.cpp:14493); step 2: totals[7] = r0.r, r0.w, r0.s, r0.z, |r|^2 (norm_1), |r0|^2 (norm_2), |r|^2 (14558-14601)
#ifdef CUP3D_TESTING  // test / tuning support: not in the release library at all
int cup3d_debug_ctl_step(int step, double *io, const double *totals) {
  if (!io || !totals || (step != 1 && step != 2)) return CUP3D_EINVAL;
  SolverCtl c;
  c.alpha = io[0]; c.beta = io[1]; c.omega = io[2]; c.r0r_prev = io[3]; c.norm = io[4]; c.init_norm = io[5]; c.min_norm = io[6];
  c.tol = io[7]; c.tol_rel = io[8]; c.state = (int)io[9]; c.restarts = (int)io[10]; c.max_restarts = (int)io[11];
  c.xcur = (int)io[12]; c.xopt = (int)io[13]; c.iter = (int)io[14]; c.seq = 0;
  if (step == 1) ctl_step1(c, totals); else ctl_step2(c, totals);
  io[0] = c.alpha; io[1] = c.beta; io[2] = c.omega; io[3] = c.r0r_prev; io[4] = c.norm; io[5] = c.init_norm; io[6] = c.min_norm;
  io[9] = c.state; io[10] = c.restarts; io[12] = c.xcur; io[13] = c.xopt; io[14] = c.iter;
  return CUP3D_OK;
}

// TEST SUPPORT: what the last cup3d_poisson_solve on this sim left behind (include/cup3d_hip_testing.h says which entries are live)
int cup3d_debug_solver_state(cup3d_sim_t *h, double *io, double *totals) {
  if (!h || !io || !totals) return CUP3D_EINVAL;
  const Sim *s = reinterpret_cast<const Sim *>(h);
  if (!s->dbg_solver.valid) { set_error("cup3d_debug_solver_state: no cup3d_poisson_solve, cup3d_diffusion_solve or cup3d_advect_diffuse_implicit has completed on this sim"); return CUP3D_ESTATE; }
  memcpy(io, s->dbg_solver.io, sizeof s->dbg_solver.io);
  memcpy(totals, s->dbg_solver.totals, sizeof s->dbg_solver.totals);
  return CUP3D_OK;
}
int cup3d_debug_solver_vector(cup3d_sim_t *h, int which, double *host_out) {
  if (!h || !host_out || which < 0 || which >= NVEC) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (!s->dbg_solver.valid) { set_error("cup3d_debug_solver_vector: no cup3d_poisson_solve, cup3d_diffusion_solve or cup3d_advect_diffuse_implicit has completed on this sim"); return CUP3D_ESTATE; }
  // the two x buffers are sv[X_] and sv[XOPT]; SolverCtl::xcur / xopt (io[12], io[13]) say which holds x and which the snapshot
  const int xcur = (int)s->dbg_solver.io[12], xopt = (int)s->dbg_solver.io[13];
  int buf = which;
  if (which == X_) buf = xcur ? XOPT : X_;
  if (which == XOPT) {
    if (xopt < 0) { set_error("cup3d_debug_solver_vector: the solve recorded no x_opt"); return CUP3D_ESTATE; }
    buf = xopt ? XOPT : X_;
  }
  if (s->nb == 0) return CUP3D_OK;
  CUP3D_HIP(hipStreamSynchronize(stream()));
  CUP3D_HIP(hipMemcpy(host_out, s->sv[buf], (size_t)s->nb * 512 * sizeof(double), hipMemcpyDeviceToHost));
  return CUP3D_OK;
}
#endif

// TEST SUPPORT: see k_debug_wave_sum (in64 -> out128, host arrays)
#ifdef CUP3D_TESTING  // test / tuning support: not in the release library at all
int cup3d_debug_wave_sum(const double *in64, double *out128) {
  if (!in64 || !out128) return CUP3D_EINVAL;
  Dev<double> d;
  int rc = d.alloc(192);
  if (rc) return rc;
  CUP3D_HIP(hipMemcpy(d, in64, 64 * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_wave_sum, dim3(1), dim3(64), 0, stream(), d.get(), d + 64);
  CUP3D_HIP(hipStreamSynchronize(stream()));
  CUP3D_HIP(hipMemcpy(out128, d + 64, 128 * sizeof(double), hipMemcpyDeviceToHost));
  return CUP3D_OK;
}

// TEST SUPPORT: see k_debug_cg_div (host arrays of `count` doubles)
int cup3d_debug_cg_div(const double *n, const double *d, long count, double *out) {
  if (!n || !d || !out || count < 0 || count > (1L << 30)) return CUP3D_EINVAL;
  if (count == 0) return CUP3D_OK;
  const size_t bytes = (size_t)count * sizeof(double);
  Dev<double> b;
  int rc = b.alloc(3 * (size_t)count);
  if (rc) return rc;
  CUP3D_HIP(hipMemcpy(b, n, bytes, hipMemcpyHostToDevice));
  CUP3D_HIP(hipMemcpy(b + count, d, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_cg_div, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream(), b.get(), b + count, count, b + 2 * count);
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipStreamSynchronize(stream()));
  CUP3D_HIP(hipMemcpy(out, b + 2 * count, bytes, hipMemcpyDeviceToHost));
  return CUP3D_OK;
}

// TEST SUPPORT: the per-block CG iteration counts behind cup3d_profile_block_cg_iterations (slot order, nblocks of them)
int cup3d_debug_block_cg_iterations(cup3d_sim_t *h, int32_t *per_block) {
  if (!h || !per_block) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (!s->d_cg_iters) {
    set_error("cup3d_debug_block_cg_iterations: no block-CG launch was made on this sim while cup3d_profile_enable(1) was on");
    return CUP3D_ESTATE;
  }
  CUP3D_HIP(hipStreamSynchronize(stream()));
  CUP3D_HIP(hipMemcpy(per_block, s->d_cg_iters, (size_t)s->nb * sizeof(int), hipMemcpyDeviceToHost));
  return CUP3D_OK;
}
#endif

int cup3d_preconditioner(cup3d_sim_t *h, int block_solver) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  s->block_solver = block_solver;
  // in place: a block solve reads its block before it writes it; the multigrid cycle of a uniform grid, whose output doubles as the
  // finest iterate while the input is read again by every launch, stages its input first (mg_vcycle)
  return launch_precond(s, s->pres, s->pres, false);
}

int cup3d_poisson_path_checksum(cup3d_sim_t *h, int block_solver, int mean_constraint, unsigned long long *sums) {
  if (!h || !sums) return CUP3D_EINVAL;
  cup3d_poisson_params d;
  cup3d_poisson_default_params(&d);
  d.block_solver = block_solver;
  d.mean_constraint = mean_constraint;
  return solve(reinterpret_cast<Sim *>(h), d, nullptr, nullptr, sums);
}

int cup3d_poisson_solve(cup3d_sim_t *h, const cup3d_poisson_params *p, cup3d_poisson_result *r) {
  if (!h) return CUP3D_EINVAL;
  cup3d_poisson_params d;
  cup3d_poisson_default_params(&d);
  return solve(reinterpret_cast<Sim *>(h), p ? *p : d, r);
}

int cup3d_pressure_project(cup3d_sim_t *h, double dt, int step, const cup3d_poisson_params *pp, cup3d_poisson_result *r) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  cup3d_poisson_params P;
  cup3d_poisson_default_params(&P);
  if (pp) P = *pp;
  const long N = s->nb * 512L;
  const unsigned G = vec_groups(N), Gs = vec_groups_simple(N);
  const bool second_order = step > 2;  // sim.step > sim.step_2nd_start (= 2), main.cpp:15087, 15355
  // Several ranks: chi written on THIS rank although cup3d_sim_set_obstacles(0) told every rank that none holds an obstacle.  The flag does
  // not steer the sequence of collectives (chi_path() depends on what the ranks were told, which is the same everywhere), so it needs no
  // agreement BEFORE the operator -- that was one stream drain + one blocking all-reduce + one host wait per time step.  It rides along
  // with the mean-pressure all-reduce the operator performs anyway (15123) and every rank returns the error together at the end.
  const bool over_ranks = s->grid->nranks > 1;
  const double conflict = over_ranks && s->chi_conflict() ? 1.0 : 0.0;
  if (second_order) { ProfileScope ps("project_pointwise"); LAUNCH_VEC_S(k_copy, s->pres, s->pold, N); }  // pOld, 15075
  // tmpV = 0 (15076-15078) matters only as the udef lab of KernelPressureRHS; without obstacles the RHS kernel does not read it
  // (adding -0*fac*0 is the identity).  With a resident chi it does: unless the caller has placed udef there since the last
  // projection (upload / fill / cup3d_update_tmpv), tmpV still holds the previous step's gradP scratch and is cleared here.
  if (s->chi_path() && !s->udef_nonzero) TRY(cup3d_sim_fill(h, CUP3D_FIELD_TMPV, 0.0));
  TRY(cup3d_pressure_rhs(h, dt));
  s->udef_nonzero = false;
  if (second_order) {
    TRY(cup3d_div_pressure(h));
    ProfileScope ps("project_pointwise");
    LAUNCH_VEC_S(k_sub_divp, s->lhs, s->tmpV, s->pres, N);
  } else {
    TRY(cup3d_sim_fill(h, CUP3D_FIELD_PRES, 0.0));  // 15102-15106
  }
  TRY(solve(s, P, r));
  const double hh = s->grid->h, vv = hh * hh * hh;
  Reducer red{s};
  { ProfileScope ps("project_pointwise"); LAUNCH_VEC(k_mean_dots, s->pres, N, vv, s->d_hb, red.out()); }
  if (over_ranks) {  // + the chi-conflict flag of the ranks (above)
    hipLaunchKernelGGL(k_set_one, dim3(1), dim3(1), 0, stream(), s->d_red, (size_t)kRedDots + 2, conflict);
    TRY(red.begin(3));
  } else {
    TRY(red.begin(2));                                       // MPI_Allreduce(2), 15123
  }
  TRY(red.wait());
  if (over_ranks && s->h_red[2] != 0.0) {
    set_error(conflict != 0.0 ? "cup3d_pressure_project: chi was written on this rank but cup3d_sim_set_obstacles(0) says no rank holds an obstacle"
                              : "cup3d_pressure_project: another rank holds a chi although cup3d_sim_set_obstacles(0) told every rank that none does");
    return CUP3D_ESTATE;
  }
  const double avg = s->h_red[0] / s->h_red[1];              // 15126
  { ProfileScope ps("project_pointwise"); LAUNCH_VEC_S(k_shift_mean, s->pres, second_order ? s->pold : (const double *)nullptr, N, avg); }
  TRY(cup3d_grad_p_update(h, dt));                           // KernelGradP + vel += tmpV/h^3, 15146-15159
  CUP3D_HIP(hipGetLastError());
  return CUP3D_OK;
}

}  // extern "C"

namespace cup3d {

// The direct block solve of the implicit diffusion (launch_precond_diffusion with cup3d_diffusion_set_block_solver(sim, 1)).  LAST in this
// translation unit on purpose: it holds the only use of k_precond_fdm_helm, which puts that kernel behind every other one (see there).
static int launch_precond_fdm_helm(Sim *s, const double *in, double *out, const HelmholtzOp &op) {
  GridDev g = s->gdev();
  int rc = fdm_setup();
  if (rc) return rc;
  ProfileScope ps("diffusion_block_fdm");
  hipLaunchKernelGGL(k_precond_fdm_helm<>, dim3(launch_groups(g)), dim3(64), 0, stream(), g, in, out, op.nu, op.dt);
  CUP3D_HIP(hipGetLastError());
  s->sums_of = nullptr;
  return CUP3D_OK;
}

}  // namespace cup3d
