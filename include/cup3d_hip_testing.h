/* cup3d_hip_testing.h -- TEST / TUNING SUPPORT of libcup3d_hip_testing.so (built with -DCUP3D_TESTING).  NOT part of the drop-in
 * boundary (include/cup3d_hip.h): nothing here replaces a reference interface.  The release library (libcup3d_hip.so) does not export any of these
 * names (tests/test_host_indexing.py checks their absence).
 */
#ifndef CUP3D_HIP_TESTING_H
#define CUP3D_HIP_TESTING_H
#include "cup3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* kernel variants / ablations by name (0 = production behaviour) */
CUP3D_API int cup3d_debug_set_option(const char *name, int value);
/* several ranks' sims in one process on one GPU: exchanges become no-ops filled by cup3d_debug_halo_pull */
CUP3D_API int cup3d_debug_virtual_ranks(int on);
CUP3D_API int cup3d_debug_halo_pull(cup3d_sim_t *dst, cup3d_sim_t *const *peers, int npeers, int field, int nc, int w);
/* in-process communicator over `nranks` host threads (one Sim per thread-rank, ordinary entry points); 0 tears it down */
CUP3D_API int cup3d_debug_virtual_comm(int nranks);
/* a single Runge-Kutta stage of cup3d_advect_diffuse; the ghost slabs of the interface faces of a multi-level mesh */
CUP3D_API int cup3d_debug_advdiff_stage(cup3d_sim_t *, int rk, double dt, double nu, const double uinf[3]);
CUP3D_API int cup3d_debug_amr_slabs(cup3d_sim_t *, int field, int w, double *out);
CUP3D_API int cup3d_debug_wave_sum(const double *in64, double *out128);
/* fast_div, the reciprocal division of the production block CG (v_rcp_f64, two Newton steps, one residual correction), elementwise:
 * out[i] = n[i] / d[i] within 1 ulp; host arrays */
CUP3D_API int cup3d_debug_cg_div(const double *n, const double *d, long count, double *out);
/* per-block CG iterations of the last block-CG launch made on this sim while cup3d_profile_enable(1) was on (slot order; nblocks values) */
CUP3D_API int cup3d_debug_block_cg_iterations(cup3d_sim_t *, int32_t *per_block);
/* the solver's scalar recurrences (SolverCtl, poisson_ctl.hpp) stepped on the host -- the same functions the device runs; no GPU needed.
 * io[16] = alpha, beta, omega, r0r_prev, norm, init_norm, min_norm, tol, tol_rel, state (0 run, 1 done, 2 restart), restarts,
 * max_restarts, xcur, xopt, iter; step 1 takes totals[2] (main.cpp:14493), step 2 totals[7] (14558-14601) */
CUP3D_API int cup3d_debug_ctl_step(int step, double *io, const double *totals);
/* What the last cup3d_poisson_solve on this sim left behind -- with max_iter = m and tol = tol_rel = 0 that is the solver's state after
 * exactly m iterations (tests/test_gpu_bicgstab_iteration.py).  Saved by the testing build when a solve returns; CUP3D_ESTATE before one has.
 * The Helmholtz solves leave the same record: after cup3d_diffusion_solve, or after the last of the three solves of
 * cup3d_advect_diffuse_implicit (component 2), the read-outs describe that solve (tests/test_gpu_helmholtz_iteration.py).  Every
 * iteration of such a solve is host-driven, so t = A what is live and q.y, y.y are reported after each; io[11] reads 2147483647
 * (DiffusionSolver::solve has no cap on its restarts, whatever cup3d_poisson_params::max_restarts says).
 *
 * cup3d_debug_solver_vector: one work vector, slot order, nblocks*512 doubles (host memory).  `which` counts the logical vectors in
 * the order of poisson_vector.hpp: 0 phat, 1 rhat, 2 shat, 3 what, 4 zhat, 5 qhat, 6 s, 7 w, 8 z, 9 t, 10 v, 11 q, 12 r, 13 y, 14 x, 15 r0,
 * 16 b, 17 x_opt.  The two x buffers swap roles during a solve (SolverCtl::xcur / xopt, ctl_xwrite); 14 and 17 are resolved to the
 * buffer that holds the iterate / the snapshot (17: CUP3D_ESTATE when the solve recorded none).
 *   LIVE when a solve returns: every vector but t, with the values of main.cpp:14404-14616 after that iteration.  t = A what (14549)
 *   is live only where the LHS is a launch of its own (multi-level meshes, block solvers without a fused kernel, "no_fuse",
 *   "no_fuse_lhs") or after a restart; where the loop kernels form the LHS themselves (uniform grids) the first loop of the NEXT
 *   iteration forms it, so t is then the t of the iteration before (A what_{m-1}), and after an every-50th iteration in its
 *   k_refresh form it is older still.  v is A zhat of the last iteration everywhere.
 *
 * cup3d_debug_solver_state: io[16] in the layout of cup3d_debug_ctl_step, as Solver::finish holds it; io[15] = 1 when the last
 * iteration ended in the restart of 14567-14593.  totals[9] = the first seven doubles of the reduction buffer when the solve
 * returned, then q.y, y.y:
 *   [0..6]  r0.r, r0.w, r0.s, r0.z, |r|^2, |r0|^2, |r|^2 the scalars were last stepped from (14546; all-reduced over ranks).  The first
 *           loop's totals share [0], [1] and are gone by then.  After a restart [0], [1] hold r0.r0 and r0.w of 14578-14581 instead
 *           ([2..6] stay); after max_iter = 0 they hold r0.r0, r0.w of 14436-14440 and the rest is not meaningful.
 *   [7], [8] q.y, y.y (14486) where the host stepped omega from them: host-driven iterations (every 50th, block solvers without a
 *           fused kernel, "no_fuse").  NaN after a fused iteration: there the kernel that totals them steps omega on the device and
 *           the second loop's totals overwrite them. */
CUP3D_API int cup3d_debug_solver_vector(cup3d_sim_t *, int which, double *host_out);
CUP3D_API int cup3d_debug_solver_state(cup3d_sim_t *, double *io, double *totals);
/* the multigrid option's level hierarchies of all `nranks` ranks for the leaf ownership `owner[nblocks]` of a global multi-level mesh,
 * checked against each other (tables in range, exchange plans symmetric node for node, every ancestor's octants complete); no GPU */
CUP3D_API int cup3d_debug_mg_plan_check(const cup3d_grid_t *mesh, const int32_t *owner, int nranks);
/* the local slots whose kernels run before the halo exchange has completed (cup3d_grid_ninner of them); no GPU */
CUP3D_API int cup3d_debug_grid_inner_blocks(const cup3d_grid_t *grid_or_view, int32_t *slots);
/* a rank's TENSORIAL view of a mesh (cup3d_grid_rank_view gives the star-stencil one): what cup3d_adapt_migrate and
 * cup3d_grad_chi_on_tmp_over_ranks build internally -- edge / corner neighbours are ghosts too, whole blocks travel; no GPU */
CUP3D_API int cup3d_debug_grid_rank_view_tensorial(const cup3d_grid_t *mesh, const int32_t *owner, int rank, int nranks, cup3d_grid_t **view);

/* HOST-MEMORY TRANSPORT in RCCL's place: one process per rank as in production, but every exchange of the library (face slabs, ghost
 * blocks, face fluxes, block migration, scalar all-reduces) is staged through host memory and carried by the CALLER's transport --
 * the reference's own MPI in the test harness (oracle/ref_harness.cpp).  RCCL refuses two ranks on one device; this lets the
 * multi-rank code of the C++ shim and of the library run as real processes on a one-GPU box.  Blocking and slow by design.
 *   exchange:  for every peer p: send_bytes[p] bytes at sendbuf + send_off[p] go to p, recv_bytes[p] bytes from p land at
 *              recvbuf + recv_off[p] (the caller's rank has zero bytes both ways); host memory
 *   allreduce: n doubles in place, sum (is_max = 0) or max */
typedef struct {
  void *ctx;
  int (*exchange)(void *ctx, const void *sendbuf, const long *send_off, const long *send_bytes, void *recvbuf, const long *recv_off,
                  const long *recv_bytes);
  int (*allreduce)(void *ctx, double *buf, int n, int is_max);
} cup3d_host_transport;
CUP3D_API int cup3d_debug_host_transport(int rank, int nranks, const cup3d_host_transport *t); /* t = NULL: remove it */

#ifdef __cplusplus
}
#endif
#endif
