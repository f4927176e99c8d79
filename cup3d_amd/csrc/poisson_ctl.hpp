// The scalar recurrences of the solver.
// Part of poisson.hip's translation unit: included there once, in order; not a stand-alone header.
#pragma once

namespace cup3d {

// ------------------------------------------------------------------ the scalar recurrences, resident on the device
// The scalars of PoissonSolverAMR::solve -- alpha, beta, omega, r0r_prev (14443, 14493, 14558-14564), the breakdown test (14566), the
// x_opt bookkeeping (14594-14600) and the stopping rule (14601) -- as ONE struct and ONE pair of functions compiled for host and
// device.  In the fused iterations (k % 50 != 0) the struct lives in device memory: the kernel that totals the dot products (or, over
// ranks, a one-thread kernel behind the all-reduce) steps it, the next loop kernel reads alpha / beta / omega from it, and the host
// only WATCHES: it enqueues iteration k + 1 before it has seen the outcome of iteration k, through a ring of pinned status slots.  A
// launch never waits for the host.  When the outcome is "converged" or "serious breakdown", the kernels of the iteration enqueued
// ahead find state != kRun and return at once; the host then finishes, or runs the restart (14567-14593) and re-enqueues.
// The every-50th iterations (true-residual refresh through _lhs) and the other block solvers step the same struct on the host.
enum { kRun = 0, kDone = 1, kRestart = 2 };
struct SolverCtl {
  double alpha, beta, omega, r0r_prev;
  double norm, init_norm, min_norm;
  double tol, tol_rel;
  int state;
  int restarts, max_restarts;
  int xcur, xopt;  // which of the two x buffers holds x / the best iterate so far (x_opt; -1: none yet)
  int iter;        // iterations completed
  unsigned seq;    // sequence number of the fused iteration in flight (the host's Sim::ctl_seq numbering: k_ctl_set places it, ctl_step2 advances
                   // it): the slot of the status ring and the values of the early all-reduce's flags derive from it, so that the kernels of an
                   // iteration take NO per-iteration argument
};
struct CtlSlot { SolverCtl c; unsigned seq; unsigned pad; };  // pinned status ring, slot = seq & 3
// x is updated in place unless the buffer that holds it is also the x_opt snapshot: then the update goes to the other buffer
// (x_opt = x without a copy: x is read once and written once by the second loop anyway)
__host__ __device__ inline int ctl_xwrite(const SolverCtl &c) { return c.xopt == c.xcur ? 1 - c.xcur : c.xcur; }
// after the first loop's dot products (q.y, y.y): 14493
__host__ __device__ inline void ctl_step1(SolverCtl &c, const double *t) { c.omega = t[0] / (t[1] + 1e-100); }
// after the second loop's seven (14546): 14558-14566, 14594-14601.  The restart itself (kernel launches) is the host's.
__host__ __device__ inline void ctl_step2(SolverCtl &c, const double *t) {
  const double eps = 1e-100;
  const double r0r = t[0], r0w = t[1], r0s = t[2], r0z = t[3], norm_1 = t[4], norm_2 = t[5];
  const double norm = sqrt(t[6]);
  const double omega = c.omega;
  double alpha = c.alpha;
  const double beta = alpha / (omega + eps) * r0r / (c.r0r_prev + eps);  // 14558
  alpha = r0r / (r0w + beta * r0s - beta * omega * r0z);                 // 14559
  double alphat = 1.0 / (omega + eps) + r0w / (r0r + eps) - beta * omega * r0z / (r0r + eps);
  alphat = 1.0 / (alphat + eps);
  if (fabs(alphat) < 10 * fabs(alpha)) alpha = alphat;                   // 14563-14564
  c.alpha = alpha;
  c.beta = beta;
  c.r0r_prev = r0r;
  c.norm = norm;
  c.xcur = ctl_xwrite(c);  // x lives where the second loop wrote it
  c.iter++;
  c.seq++;
  int state = kRun;
  if (r0r * r0r < 1e-16 * norm_1 * norm_2 && c.restarts < c.max_restarts) {  // serious breakdown, 14566-14567
    c.restarts++;
    state = kRestart;
  }
  if (norm < c.min_norm) {  // 14594-14600
    c.min_norm = norm;
    c.xopt = c.xcur;
  }
  if (norm < c.tol || norm / (c.init_norm + eps) < c.tol_rel) state = kDone;  // 14601
  c.state = state;
}
__device__ __forceinline__ void ctl_publish(const SolverCtl *c, CtlSlot *ring, unsigned seq) {
  CtlSlot *sl = ring + (seq & 3);
  sl->c = *c;
  __threadfence_system();
  __hip_atomic_store(&sl->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// several ranks: the totals are all-reduced first (communication stream); this one-thread kernel behind the all-reduce steps the
// struct -- identically on every rank, the all-reduced bits are the same everywhere -- and the compute stream waits for its event
template <int STEP>
__global__ void k_ctl_step(SolverCtl *ctl, const double *__restrict__ tot, CtlSlot *ring) {
  if (ctl->state != kRun) return;  // an iteration enqueued ahead of a stop / restart: nothing happened, nothing to step
  SolverCtl c = *ctl;
  const unsigned it = c.seq;
  if (STEP == 1) ctl_step1(c, tot); else ctl_step2(c, tot);
  *ctl = c;
  if (STEP == 2) ctl_publish(ctl, ring, it);
}
typedef void (*CtlStepKernel)(SolverCtl *, const double *, CtlSlot *);
static CtlStepKernel ctl_step_kernel(int step) { return step == 1 ? k_ctl_step<1> : k_ctl_step<2>; }
__global__ void k_ctl_set(SolverCtl *ctl, SolverCtl v) { *ctl = v; }

}  // namespace cup3d
