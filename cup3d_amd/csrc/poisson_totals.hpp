// Totals of per-block values -- inside the kernel that produces them (Arrive) or in a launch of their own (k_sums_finish).
// Part of poisson.hip's translation unit: included there once, in order; not a stand-alone header.
#pragma once

namespace cup3d {

// ------------------------------------------------------------------ totals of per-block values INSIDE the kernel that produces them
// Rounds 2-4 finished the dot products of a fused loop in a launch of their own (k_sums_finish: 64 / 256 workgroups over the [K][nb]
// per-block values, last workgroup totals and steps the scalars).  That launch -- 16-27 us plus the gap around it, twice per iteration --
// is what the per-rank share of the workload on 8 GPUs (256^3: 1.15 ms per iteration) feels most, and it pins the moment the totals exist
// to the END of the loop kernel, one block-CG phase later than they are complete.  Here the kernel finishes them itself: a wavefront
// that has written its block's values takes a ticket in the counter of its GROUP (64 consecutive slots); the last one of a group adds
// the group's 64 values (one per lane, wave tree) and takes a ticket in the counter of the SUPER-GROUP (64 groups); the last one there
// adds the 64 group sums; the last super-group adds the super-group sums, stores the K totals and runs `then` (the recurrence step on
// one rank; the flag the communication stream waits for over ranks).  Who is last varies from run to run, WHAT is added in which
// order does not: sums of fixed sets in a fixed tree -- deterministic.  Counters count over all launches of a loop (inner / boundary
// pass, plain / interface list): membership is by slot.  Release / acquire at agent scope as in grid_sum_finish (tile.hpp); the values
// of other wavefronts are read with agent-scope loads.
struct Arrive {
  const double *vals;      // [K][nb] per-block values
  double *g1, *g2;         // [K][n1], [K][n2]: sums of 64 blocks / of 64 groups
  unsigned *c1, *c2, *c3;  // arrivals per group [n1], per super-group [n2], super-groups done [1]; all zero between two loops
  long nb, n1, n2;
  double *out;             // [K] totals (device memory)
};
__device__ __forceinline__ unsigned ticket_of_wave(unsigned *counter) {  // lane 0's values are stored: take a ticket; every lane gets it
  unsigned t = 0;
  if (threadIdx.x == 0) {
    stores_done();
    t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return (unsigned)__builtin_amdgcn_readfirstlane((int)t);
}
// a ticket taken by a wavefront that speaks for a whole GROUP: its sums were written by agent-scope stores as well, but they are read by a
// wavefront on ANOTHER XCD a moment later, so this rare path (1 wavefront in 64) pays for the full agent-scope release (L2 write-back)
__device__ __forceinline__ unsigned ticket_of_group(unsigned *counter) {
  unsigned t = 0;
  if (threadIdx.x == 0) {
    __threadfence();
    t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return (unsigned)__builtin_amdgcn_readfirstlane((int)t);
}
template <int K, class Then>
__device__ __forceinline__ void arrive(const Arrive &A, int slot, Then then) {
  const int l = threadIdx.x;
  const long g = slot >> 6, first = g << 6;
  const unsigned gsize = (unsigned)(A.nb - first < 64 ? A.nb - first : 64);
  if (ticket_of_wave(A.c1 + g) != gsize - 1) return;  // (the loads below are issued after the ticket has come back: control dependence)
  __threadfence();                                    // ... and behind an agent-scope acquire (the last arrivers only: 1 wavefront in 64)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum((unsigned)l < gsize ? ld_agent(A.vals + (size_t)k * A.nb + first + l) : 0.0);
    if (l == 0) st_agent(A.g1 + (size_t)k * A.n1 + g, v);
  }
  const long sg = g >> 6, gfirst = sg << 6;
  const unsigned sgsize = (unsigned)(A.n1 - gfirst < 64 ? A.n1 - gfirst : 64);
  if (l == 0) st_agent(A.c1 + g, 0u);
  if (ticket_of_group(A.c2 + sg) != sgsize - 1) return;
  __threadfence();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum((unsigned)l < sgsize ? ld_agent(A.g1 + (size_t)k * A.n1 + gfirst + l) : 0.0);
    if (l == 0) st_agent(A.g2 + (size_t)k * A.n2 + sg, v);
  }
  if (l == 0) st_agent(A.c2 + sg, 0u);
  if (ticket_of_group(A.c3) != (unsigned)A.n2 - 1) return;
  __threadfence();
  double tot[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double v = 0;
    for (long j = l; j < A.n2; j += 64) v += ld_agent(A.g2 + (size_t)k * A.n2 + j);
    tot[k] = wave_sum(v);
    if (l == 0) st_agent(A.out + k, tot[k]);
  }
  if (l == 0) {
    st_agent(A.c3, 0u);
    then(tot);
  }
}
// what the wavefront that completes the dot products does with them
struct DotsThen {
  SolverCtl *ctl; CtlSlot *ring;
  int which;         // 1: first loop (q.y, y.y -> omega, 14493), 2: second loop (the seven of 14546 -> 14558-14601)
  int step;          // != 0: one rank -- step the solver's scalars (ctl_step1 / ctl_step2) and, after the second loop, publish them to the host's ring; 0: totals only
  unsigned *flag;    // several ranks, early all-reduce: raised to 2 seq + which - 1 once the totals are in device memory (k_wait_totals on the communication stream)
  __device__ __forceinline__ void operator()(const double *tot) const;
};
struct LoopSums {  // what a fused loop kernel needs to total its per-block values; constant over a solve, in DEVICE memory (Sim::d_loop_sums): the
                   // kernels take a pointer -- as a by-value argument its 25 words stayed live across the plane loop and cost the occupancy
  Arrive dots;     // K = 2 (first loop) / 7 (second loop) dot products, complete when the last block leaves its vector phase
  Arrive mean;     // K = 1: sum(zhat h^3) / sum(what h^3) of the block solves (mean-constraint row, 9283-9326), complete when the kernel ends; vals == nullptr: not wanted
  DotsThen then;
};
__device__ __forceinline__ void DotsThen::operator()(const double *tot) const {
  const unsigned it = ctl->seq;
  if (step != 0 && ctl->state == kRun) {  // (every wavefront that came this far saw kRun; only this one changes it)
    SolverCtl c = *ctl;
    if (which == 1) ctl_step1(c, tot); else ctl_step2(c, tot);
    *ctl = c;
    if (which == 2) ctl_publish(ctl, ring, it);
  }
  if (flag) {  // the totals (this lane's own agent-scope stores) before the flag: a full agent-scope release, once per launch
    __threadfence();
    st_agent(flag, 2 * it + (unsigned)(which - 1));
  }
}
struct NoThen { __device__ __forceinline__ void operator()(const double *) const {} };
__global__ void k_set_loop_sums(LoopSums *dst, LoopSums a, LoopSums b) { dst[0] = a; dst[1] = b; }

// DEFAULT totalling of a fused loop's per-block values: K sums of nb values each ([K][nb]) finished in one launch of 64 / 256 workgroups,
// the last one to arrive totals the partials (grid_sum_finish, tile.hpp).  MEAN: one more sum rides along -- the per-block sums of
// zhat h^3 / what h^3 the fused kernel left in mean_src; the total lands in ro.out[K], where the LHS application that follows takes its
// mean-constraint row from (no k_mean_finish launch, and over ranks no second all-reduce: the total travels with the dot products).
// step 1 / 2: one rank -- the last workgroup also steps the solver's scalar struct with the totals (ctl_step1 / ctl_step2) and, after
// the second loop, publishes it to the host's status ring; step 0: totals only (several ranks: the all-reduce comes first, k_ctl_step).
// (Round 5 measured the alternative -- the loop kernels totalling these values themselves, Arrive above -- on one GPU: the launches it saves
//  (16-27 us each) are paid back by the loop kernels (agent-scope stores whose completion a wavefront must wait for before it takes its
//  ticket, +2 % on the second kernel at 512^3, +7-9 % on the smaller kernels of a multi-level mesh): neutral at 256^3, a loss elsewhere.  So
//  this launch stays the default and the in-kernel totals serve what only they can do: the early all-reduce.)
struct CtlThen {
  SolverCtl *ctl; CtlSlot *ring; int step;
  __device__ __forceinline__ void operator()(const double *tot) const {
    if (step == 0 || ctl->state != kRun) return;  // (an iteration enqueued ahead of a stop / restart summed stale partials: dropped)
    SolverCtl c = *ctl;
    const unsigned it = c.seq;
    if (step == 1) ctl_step1(c, tot); else ctl_step2(c, tot);
    *ctl = c;
    if (step == 2) ctl_publish(ctl, ring, it);
  }
};
inline int sums_groups(int64_t nb) { return nb >= (1 << 17) ? 256 : 64; }  // (0.027 instead of 0.051 ms per launch at 512^3, 0.016 instead of 0.014 at 256^3: profiles/r03)
template <int K, bool MEAN>
__global__ void __launch_bounds__(256) k_sums_finish(const double *__restrict__ v, long nb, RedOut ro, const double *__restrict__ mean_src, CtlThen then) {
  static_assert(K + (MEAN ? 1 : 0) <= kRedDotsEnd - kRedDots, "the totals of a loop must fit the kRedDots range of Sim::d_red");
  double acc[K + (MEAN ? 1 : 0)];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nb; i += (long)gridDim.x * 256) t += v[(size_t)k * nb + i];
    acc[k] = t;
  }
  if (MEAN) {
    double t = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nb; i += (long)gridDim.x * 256) t += mean_src[i];
    acc[K] = t;
  }
  grid_sum_finish<K + (MEAN ? 1 : 0)>(acc, ro, then);
}

typedef void (*SumsKernel)(const double *, long, RedOut, const double *, CtlThen);
static SumsKernel sums_kernel(int K, bool mean) {  // K = 2 / 7: the dot products of the first / second loop
  if (K == 2) return mean ? k_sums_finish<2, true> : k_sums_finish<2, false>;
  return mean ? k_sums_finish<7, true> : k_sums_finish<7, false>;
}

// several ranks, all-reduce started EARLY (solve(): early): the communication stream holds this one-thread kernel in front of the
// all-reduce; it returns when the loop kernel's last block has left its vector phase and the totals are in device memory (DotsThen
// raises *flag to seq) -- one block-solve phase before that kernel ends, so the all-reduce and the recurrence step behind it run while
// the compute stream is still busy.  Bounded: if the flag never comes (a loop kernel that died), *fail is raised and the stream moves on.
__global__ void k_wait_totals(const SolverCtl *ctl, const unsigned *flag, unsigned seq, unsigned *fail, long long limit_ticks) {
  // an iteration enqueued ahead of a stop or a restart: its loop kernels return at once and nobody will raise the flag.  (The struct is
  // stepped on THIS stream only, k_ctl_step: what this kernel reads is what those loop kernels read.)
  if (ctl->state != kRun) return;
  const long long t0 = wall_clock64();
  while ((int)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - seq) < 0) {
    __builtin_amdgcn_s_sleep(32);
    if (wall_clock64() - t0 > limit_ticks) { __hip_atomic_store(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return; }
  }
}
__global__ void k_raise(unsigned *flag, unsigned seq) { __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace cup3d
