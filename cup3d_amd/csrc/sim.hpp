// Device mirror of SimulationData's five block grids (main.cpp:6603-6607) plus the
// solver work vectors of PoissonSolverAMR (main.cpp:9394-9411), for one rank.
//
// HBM layout: every field is one slab  [block slot][component][z][y][x]  of FP64
// (SoA per block: 4 KiB per component per block), slots in m_vInfo order.  Ghost
// cells are never materialised in HBM: kernels stage the ghosted tile of a block in
// LDS straight from the neighbour slots (this replaces BlockLab::load, 3623-3743).
// Face slabs owned by other ranks live in `halo_*` buffers filled by RCCL.
// Every buffer is an owner member (devmem.hpp): it goes with its Sim, and what is not listed anywhere cannot be forgotten there.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cup3d_hip.h"
#ifdef CUP3D_TESTING
#include "../../include/cup3d_hip_testing.h"  // the test-support entry points are exported (CUP3D_API) from the testing build only
#endif
#include "grid.hpp"

#include "devmem.hpp"  // set_error, CUP3D_HIP; Dev<T>, DevGrow, Pinned<T>: every buffer below is owned by type and goes with its Sim

namespace cup3d {

hipStream_t stream();  // compute stream (cup3d_set_stream)
// Two flavours of the library are built from these sources (Makefile): libcup3d_hip.so, the release build, and
// libcup3d_hip_testing.so (-DCUP3D_TESTING), which adds what tests and tuning scans need and a deployment does not: the debug-option
// map read on launch paths, the in-process "virtual" communicator (comm.hip), the evaluation variants of the block CG.  In the
// release build debug_option() is a constant 0 and the variant branches fold away.
#ifdef CUP3D_TESTING
int debug_option(const char *name);  // cup3d_debug_set_option; 0 when unset (production behaviour)
#else
constexpr int debug_option(const char *) { return 0; }
#endif
int not_in_release(const char *what);  // sets the error text, returns CUP3D_ESTATE
bool profile_on();                   // cup3d_profile_enable

// ---- per-kernel timing (cup3d_profile_*) ----
struct ProfileScope {
  explicit ProfileScope(const char *name);        // events on the compute stream
  ProfileScope(const char *name, hipStream_t st);  // ... on `st` (the communication stream: "comm_*" entries)
  ~ProfileScope();
  int idx;
  hipEvent_t start;
  hipStream_t st;
};

// ---- run statistics (cup3d_stats_*): what crossed ranks and how long the host waited for the device
void stats_host_wait(double seconds);
void stats_solver_iterations(long n);
void stats_halo(size_t bytes_sent);
void stats_allreduce();
void stats_field_download(size_t bytes);  // field data handed to the host outside cup3d_sim_download* (cup3d_sim_labs)

struct Comm;  // RCCL state (comm.cpp)
Comm *comm();  // nullptr when single rank
bool virtual_ranks();  // test mode (cup3d_debug_virtual_ranks)
bool host_transport();  // test mode (cup3d_debug_host_transport): exchanges staged through host memory and the caller's transport

// Device-side description of the topology, passed by value to kernels.
struct GridDev {
  const int32_t *nbr;   // [nb][6]
  const int32_t *list;  // optional block list (inner / boundary); nullptr = all blocks
  int nblocks;          // number of blocks this launch covers
  int chunk;            // ceil(nblocks / 8): blocks per XCD
  double h;
  // multi-level meshes: per-block spacing (nullptr on uniform grids) and the face-flux arrays of the
  // interface faces [(e*nc + c)][64] the kernel must fill (e = nbr - kNbrHalo); see amr.hip
  const double *hb;
  double *flux;
  // multi-level meshes: 1 for the blocks that have a coarse-side interface face, i.e. whose result the flux correction still edits;
  // the advect-diffuse stage leaves their raw increment in tmpV and fuses the Runge-Kutta update for all the others
  const unsigned char *raw;
};
__device__ __forceinline__ double block_h(const GridDev &g, int slot) { return g.hb ? g.hb[slot] : g.h; }

// The 16 doubles of Sim::d_red, by user.  The ranges must stay disjoint: the solver's scalars at kRedDots are live from one loop
// kernel to the next, and a checksum or a multigrid cycle may run in between.
enum RedSlot : int {
  kRedDots = 0,      // [0, 8): totals of the 2 / 7 dot products of a BiCGSTAB loop, the mean-constraint total riding along behind them
                     //         ([2] after loop 1, [7] after loop 2); outside a solve: max|u| ([0]), the penalisation's 6 sums + status ([0, 7))
  kRedDotsEnd = 8,
  kRedMeanLhs = 8,   // [8]: sum(p h^3) of a stand-alone LHS application (k_mean_finish, stencil.hip)
  kRedEarlyMean = 9, // [9], [10]: several ranks, early all-reduce: sum(zhat h^3) / sum(what h^3) of a fused loop, all-reduced on their own behind a flag
  kRedChecksum = 12, // [12]: cup3d_sim_checksum's 64-bit accumulator
  kRedMg = 14,       // [14]: coarsest-level sum of the multigrid cycle over ranks (multigrid.hip)
  kRedSize = 16
};
static_assert(kRedDotsEnd <= kRedMeanLhs && kRedMeanLhs < kRedEarlyMean && kRedEarlyMean + 2 <= kRedChecksum && kRedChecksum < kRedMg && kRedMg < kRedSize, "Sim::d_red slots overlap");

struct Sim {
  const Grid *grid = nullptr;
  int64_t nb = 0;    // local blocks: what the kernels sweep and what crosses the host boundary
  int64_t nvis = 0;  // block slots of every field array: nb + the ghost blocks of a rank view (Grid::rank_view), else nb
  // topology on device
  Dev<int32_t> d_nbr, d_inner, d_boundary, d_send_faces;
  // fields
  Dev<double> vel, vel2, tmpV;    // [nb][3][512]
  Dev<double> pres, lhs, chi;     // [nb][512]
  Dev<double> pold;
  bool chi_nonzero = false;   // chi was uploaded / filled non-zero: the pressure RHS reads chi and udef (= tmpV)
  bool udef_nonzero = false;  // tmpV holds the udef of the NEXT projection (uploaded, filled or cup3d_update_tmpv since the last one)
  // cup3d_sim_set_obstacles: does ANY rank hold an obstacle (the reference's obstacle_vector is replicated, every rank knows)?
  // -1 = not told: several ranks then always take the chi / udef path of the pressure right-hand side, because its udef exchange is a
  // collective and chi_nonzero is per-rank state
  int obstacles_global = -1;
  // one rank: told "obstacles" or chi was written (a chi filled by hand after set_obstacles(0) still counts -- never silently dropped);
  // several ranks: as told, the same on every rank (told 0 with a written chi is refused by cup3d_pressure_project, chi_conflict())
  bool chi_path() const { return grid->nranks == 1 ? (obstacles_global == 1 || chi_nonzero) : obstacles_global != 0; }
  bool chi_conflict() const { return grid->nranks > 1 && obstacles_global == 0 && chi_nonzero; }
  int block_solver = 0;  // cup3d_poisson_params.block_solver of the running solve
  int diffusion_block_solver = 0;  // cup3d_diffusion_set_block_solver: 0 = block CG, 1 = direct solve (launch_precond_diffusion)
  int scalar_bc_dir = -1;  // >= 0 while a Helmholtz solve of the implicit diffusion runs: domain-face rule of the scalar tiles
  // solver vectors (allocated on first solve), each [nb][512]
  Dev<double> sv[18];
  // reductions
  Dev<double> d_partials;  // [max_groups][8]
  Dev<double> d_red;       // [kRedSize] final reduced scalars, see RedSlot
  const double *sums_of = nullptr;  // vector whose per-block sums (mean constraint) are current in d_partials' tail
  Pinned<double> h_red;       // pinned host mirror
  double *h_red_dev = nullptr;   // the same memory as the device sees it (kernels store the reduced scalars there directly)
  Dev<unsigned> d_counters;  // [4] tickets of grid_sum_finish (tile.hpp), zero between launches
  Dev<int> d_cg_iters;       // [nb] CG iterations per block of the last block-CG launch (only while profiling)
  Dev<double> d_block_dots;  // [7][nb] per-block dot products of the fused loop + block-CG kernels (poisson.hip)
  // ... and what totals them inside those kernels (Arrive, poisson.hip): group / super-group sums, arrival counters, the two flags the
  // communication stream (dots) and the corner block's wavefront (mean-constraint total) wait for when the all-reduce starts early
  Dev<double> d_arrive_sums;
  Dev<unsigned> d_arrive;
  Dev<struct LoopSums> d_loop_sums;  // [2] (poisson.hip)
  Pinned<unsigned> h_early_fail;
  unsigned *h_early_fail_dev = nullptr;  // pinned: a bounded device-side wait of the early all-reduce gave up
  void *mg = nullptr;              // level hierarchy of the multigrid preconditioner (multigrid.hip), built on first use
  struct LabTables *labs = nullptr;  // tables and staging buffer of cup3d_sim_labs (labs.hip), built on first use
  struct LabsView *labs_view = nullptr;  // cup3d_sim_labs_over_ranks: the rank's tensorial view, its tables, the ghost pool (labs.hip)
  struct ForcesScratch *forces = nullptr;  // cup3d_compute_forces: tile scratch and staged surface arrays, grow-only (obstacles_forces.hip)
  // what the last successful cup3d_create_obstacles left on the device, per obstacle of that call: slots, geom, sdfLab, chi and the
  // corrected udef -- what cup3d_prevent_colliding_obstacles and the resident operators (cup3d_*_resident) read, with the latter's plan
  // once one of them has run (obstacles.hpp, obstacles_create.hip); nullptr: nothing retained
  struct RetainedObstacles *retained = nullptr;
  int max_groups = 0;
  // staging for host transfers
  Dev<double> d_stage;
  Pinned<double> h_stage;  // pinned; two buffers of stage_blocks vector blocks each, like d_stage
  hipEvent_t ev_stage[2] = {nullptr, nullptr};
  size_t stage_blocks = 0;
  bool stage_ready = false;  // every staging resource exists (a failed ensure_stage keeps what it made; the next call makes the rest)
  Dev<int32_t> d_stage_slots;
  Pinned<int32_t> h_stage_slots;  // block lists of the partial transfers (cup3d_sim_*_block_list)
  // multi-level mesh tables (amr.hip); all nullptr / 0 on uniform grids
  Dev<int32_t> d_amr_faces, d_amr_fine, d_nbr27, d_index;
  Dev<int32_t> d_restrict_list, d_prolong_list, d_fix_list[3];
  const double *mean_total_of = nullptr, *mean_total = nullptr;  // the vector whose sum(p h^3) total is already in *mean_total (device)
  unsigned red_seq = 0;  // last sequence number handed to a reduction kernel (Reducer, poisson.hip)
  // BiCGSTAB's scalar recurrences on the device (SolverCtl, poisson.hip): the struct, and the pinned ring its outcome reaches the host through
  Dev<void> d_ctl;
  Pinned<void> h_ctl;
  void *h_ctl_dev = nullptr;
  unsigned ctl_seq = 0;
#ifdef CUP3D_TESTING
  // cup3d_debug_solver_state / cup3d_debug_solver_vector: the scalars (layout of cup3d_debug_ctl_step) and the totals the last
  // cup3d_poisson_solve on this sim ended with (Solver::finish, poisson.hip); test builds only
  struct { bool valid = false; double io[16]; double totals[9]; } dbg_solver;
#endif
  unsigned n_restrict = 0, n_prolong = 0;
  Dev<int32_t> d_fix_blocks;  // [n_fix_blocks][6]: per block with a corrected (coarse-side) face, the interface face behind each of its six faces or -1
  unsigned n_fix_blocks = 0;
  unsigned n_restrict_inner = 0, n_prolong_inner = 0;  // leading entries of the two lists that belong to inner blocks (rank views)
  struct { const double *field = nullptr; int nc = 0, w = 0, bc_dir = -1; double *slabs = nullptr; bool open = false; } pending_fill;  // halo_begin -> halo_finish
  Dev<int32_t> d_send_blocks, d_send_flux;  // rank views: exchange plans (comm.hip)
  // ... and the sub-box form of the ghost-block exchange (Grid::ghost_box / send_box), per stencil-width class: boxes, the offset (in cells
  // per component) of every block's cells in the packed message, the staging buffer the messages arrive in before they are scattered
  Dev<unsigned char> d_send_box[2], d_ghost_box[2];
  Dev<long long> d_send_off[2], d_ghost_off[2];
  Dev<double> box_recv;
  Dev<unsigned char> d_raw_mask;  // [nb], see GridDev::raw
  Dev<int32_t> d_raw_list;        // the blocks with raw_mask set
  // multi-level mesh on one rank: blocks with an interface face (coarse/fine: ghost slabs, face fluxes, flux correction) and the rest,
  // whose six faces are same-level blocks or domain faces -- for those the LHS application lives inside the fused loop kernels (poisson.hip)
  Dev<int32_t> d_iface_list, d_plain_list;
  unsigned n_iface = 0, n_plain = 0;
  bool corner_is_plain = false;  // the block of the mean-constraint row (grid->corner_slot) is in the plain list
  unsigned n_raw = 0;
  Dev<double> d_hb, d_flux;
  // halo buffers (multi-rank)
  Dev<double> halo_recv, halo_send;  // n faces x 3 comps x 3 layers x 64
  size_t bytes = 0;  // cup3d_sim_device_bytes: what the allocations that name this Sim as `charge` hold (devmem.hpp)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_h1 = nullptr, ev_h2 = nullptr, ev_m = nullptr;
  hipEvent_t ev_vc_pack = nullptr, ev_vc_done = nullptr;  // virtual communicator (tests): "my send buffer is packed" / "my copies are enqueued"
  // cup3d_compute_dissipation / cup3d_fix_mass_flux (diagnostics.hip), made by the first call of either: h and origin of every local
  // block [nb][4], and the blocks' rows of sums [nb + 1][20] (the last row: this rank's totals)
  Dev<double> d_diag_geom, d_diag_rows;

  GridDev gdev(bool boundary_only = false, bool inner_only = false) const;
  GridDev gdev_list(const int32_t *list, unsigned n) const;  // the same over an explicit block list
  double *field(int id, int *ncomp) const;
};

inline size_t &ledger(Sim *s) { return s->bytes; }
// wrapping 64-bit sum of the bit patterns of n doubles (independent of launch geometry and of the sharding); synchronises
int checksum_array(Sim *s, const double *p, long n, unsigned long long *sum);
Sim *sim_comm_only(const Grid *g, hipStream_t comm_stream);  // exchange-only Sim of a coarse multigrid level (sim.hip)
void sim_comm_only_destroy(Sim *s);

// halo exchange of the face slabs of `field` (ncomp components, w ghost layers); no-op on one rank
int halo_exchange(Sim *s, const double *field, int ncomp, int w);
// overlapped form: begin on the communication stream, finish = compute stream waits for the slabs
int halo_begin(Sim *s, const double *field, int ncomp, int w);
int halo_finish(Sim *s);
// sum / max all-reduce of n doubles resident in device memory; no-op on one rank
int allreduce(Sim *s, double *d_buf, int n, bool is_max, hipStream_t st);
// collective status agreement before the first exchange of a collective entry point: every rank passes its local outcome, all get the
// worst one back (comm.hip); no-op on one rank
int agree(Sim *s, int rc, const char *where);
bool scalars_cross_ranks(const Sim *s);   // does allreduce() do anything for this sim?
hipStream_t scalar_stream(const Sim *s);  // the stream all-reduces are enqueued on (communication stream where there is one)
// rank views of a multi-level mesh: face-flux arrays of remote fine faces -> ghost face range of d_flux (before k_flux_fix)
int view_exchange_flux(Sim *s, int nfc);
// ... and whole blocks of `field` -> ghost slot range, before the ghost slabs of a stencil kernel are built (no-op elsewhere)
int view_exchange_blocks(Sim *s, double *field, int nc, int w);  // w: width of the star stencil that will read them (1 or 3)
// generic exchange of `per`-double items between ranks (own rank included), peer-major buffers; compute stream
int exchange_items(Sim *s, const double *sendbuf, const std::vector<int64_t> &send_count, double *recvbuf, const std::vector<int64_t> &recv_count, size_t per);
// the pack / unpack kernels of the ghost-block exchange and the NaN fill of "poison_ghosts" for a caller outside comm.hip.  Whole blocks ...
int launch_pack_blocks(const double *field, const int32_t *slots, int nc, double *out, unsigned n, hipStream_t st);
int launch_unpack_blocks(const double *in, const int32_t *slots, int nc, double *field, unsigned n, hipStream_t st);
// ... sub-boxes: block i of `slots` contributes the cells of box[i] at offset off[i] * nc of the message; they arrive in box[i] of block row i
int launch_pack_boxes(const double *field, const int32_t *slots, const unsigned char *box, const long long *off, int nc, double *out, unsigned n, hipStream_t st);
int launch_unpack_boxes(double *blocks, const unsigned char *box, const long long *off, int nc, const double *in, unsigned n, hipStream_t st);
int launch_nan_fill(double *p, size_t n_doubles, hipStream_t st);
// The grid of a sim as a mesh object: a uniform grid is read as the one-level mesh it is (Grid::as_mesh), which lives as long as this
// does; a mesh is itself.  nullptr: the error text is set ("<who>: ..."), the caller returns CUP3D_EINVAL.
struct MeshOf {
  std::unique_ptr<Grid> tmp;
  const Grid *get(const Grid *g, const char *who) {
    try {
      if (!g->multilevel) { tmp = g->as_mesh(); g = tmp.get(); }
    } catch (const std::exception &e) { set_error("%s: %s", who, e.what()); return nullptr; }
    return g;
  }
};
// A field of a sim on the rank's TENSORIAL view of a mesh spread over ranks: F[slot of tv][nc][512], the local blocks copied, the ghost blocks
// fetched whole from their owners.  Two steps around the caller's agree(): stage() is what one rank can get wrong alone, exchange() the collective.
struct ViewField {
  std::unique_ptr<Grid> tv;
  Dev<double> F, pack;
  Dev<int32_t> d_send;
  size_t per = 0;  // doubles per block
  // the view of (mesh, owner) for the rank of `s`, whose `field` (nc components) holds its local blocks (`not_mine`: the error text where
  // not); `plan`: what else of the caller's can throw before anything is allocated; then buffers, local blocks and the packed send list
  template <class Plan>
  int stage(const Grid *mesh, const int32_t *owner, const Sim *s, const double *field, int nc, const char *who, const char *not_mine, Plan &&plan) {
    try {
      tv = mesh->rank_view(owner, s->grid->rank, s->grid->nranks, /*tensorial=*/true);
      if (tv->n_local != s->nb) throw std::invalid_argument(not_mine);
      plan();
    } catch (const std::exception &e) {
      set_error("%s: %s", who, e.what());
      return CUP3D_EINVAL;
    }
    per = (size_t)nc * 512;
    int rc;
    if ((rc = F.alloc(tv->Z.size() * per)) || (rc = pack.alloc(std::max<size_t>(tv->send_blocks.size(), 1) * per)) || (rc = d_send.upload(tv->send_blocks, stream(), IfEmpty::null))) return rc;
    CUP3D_HIP(hipMemcpyAsync(F, field, (size_t)s->nb * per * sizeof(double), hipMemcpyDeviceToDevice, stream()));
    return launch_pack_blocks(F, d_send, nc, pack, (unsigned)tv->send_blocks.size(), stream());
  }
  // the ghost blocks arrive behind the local ones; synchronises
  int exchange(Sim *s) {
    if (int rc = exchange_items(s, pack, tv->send_block_count, F + (size_t)tv->n_local * per, tv->recv_block_count, per)) return rc;
    CUP3D_HIP(hipStreamSynchronize(stream()));
    return CUP3D_OK;
  }
};

void vcomm_register(Sim *s);    // in-process test communicator (comm.hip)
void vcomm_unregister(Sim *s);

// multi-level meshes: ghost slabs of every interface face of `field` for a w-deep star stencil -> slabs;
// flux correction of `out` (out_nc components per block, the first nfc corrected) from s->d_flux
int amr_fill_ghosts(Sim *s, const double *field, int ncomp, int w, double *slabs, int part = 0);  // part 0: every face, 1: inner blocks' faces, 2: boundary blocks' faces
int amr_flux_fix(Sim *s, int nfc, double *out, int out_nc);

// kernels' launchers shared across translation units
// list != nullptr: only the `nlist` blocks listed (and the mean-constraint fix-ups of those blocks only; needs the total of p to be known
// already, Sim::mean_total_of == p) -- the interface blocks of a multi-level mesh, while the loop kernels form the LHS of all others
int launch_lhs(Sim *s, const double *p, double *out, int mean_constraint, const int32_t *list = nullptr, unsigned nlist = 0);
int launch_precond(Sim *s, const double *in, double *out, bool want_sums);
int launch_mean_total(Sim *s);  // total of the block sums in d_partials' tail -> d_red[kRedMeanLhs] (stencil.hip)
// block_solver 5: one multigrid V-cycle from a zero guess as M^-1 (multigrid.hip; an alternative, not the reference's algorithm)
int mg_vcycle(Sim *s, const double *in, double *out);
void mg_destroy(Sim *s);
void labs_destroy(Sim *s);  // what cup3d_sim_labs and cup3d_sim_labs_over_ranks built on first use (labs.hip)
void forces_destroy(Sim *s);  // the scratch of cup3d_compute_forces (obstacles_forces.hip)
void retained_destroy(Sim *s);  // the obstacle blocks cup3d_create_obstacles keeps (obstacles_create.hip)
// implicit diffusion (DiffusionSolver, main.cpp:6719-7147): Helmholtz operator of velocity component `direction`
struct HelmholtzOp { int direction; double dt, nu; };
int launch_lhs_diffusion(Sim *s, const double *p, double *out, const HelmholtzOp &op);
int launch_precond_diffusion(Sim *s, const double *in, double *out, const HelmholtzOp &op);
int solve_helmholtz(Sim *s, const cup3d_poisson_params &P, cup3d_poisson_result *res, const HelmholtzOp &op);
int launch_diffusion_rhs(Sim *s);
int launch_advect_implicit(Sim *s, double dt, double nu, const double uinf[3]);

}  // namespace cup3d
