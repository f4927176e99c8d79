/* cup3d_hip.h — C ABI of the MI355X-native (HIP, gfx950) implementation of CUP3D's
 * per-block stencil + pressure-Poisson hot path.
 *
 * Every entry point names the reference interface it replaces (slitvinov/CUP3D,
 * main.cpp:LINE).  Plain pointers and sizes only; all functions return 0 on success
 * and a negative CUP3D_E* code on failure (the reference has no return codes: it
 * abort()s / MPI_Abort()s, main.cpp:1098, 15265 — the C++ shim in
 * cup3d_amd/host/cup3d_hip_operators.h turns a non-zero status into the same).
 * cup3d_last_error() returns a human readable message for the calling thread.
 *
 * Host block memory at this boundary is the reference's own:
 *   ScalarBlock = double[8][8][8]      (z,y,x; 4096 B,  main.cpp:5882-5919, 6586)
 *   VectorBlock = double[8][8][8][3]   (AoS u,v,w; 12288 B, main.cpp:6590)
 * in m_vInfo order (sorted by blockID_2, main.cpp:943-964).  On the device every
 * field is a slab [block][component][z][y][x] (SoA per block).
 */
#ifndef CUP3D_HIP_H
#define CUP3D_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: these entry points -- and nothing else -- are exported */
#ifndef CUP3D_API
#define CUP3D_API __attribute__((visibility("default")))
#endif

#define CUP3D_OK 0
#define CUP3D_EINVAL (-1)   /* bad argument */
#define CUP3D_EDEVICE (-2)  /* HIP error / no usable GPU */
#define CUP3D_ENOMEM (-3)
#define CUP3D_ECOMM (-4)    /* RCCL error */
#define CUP3D_ESTATE (-5)   /* call out of order */

CUP3D_API const char *cup3d_last_error(void);
CUP3D_API const char *cup3d_version(void);

/* enum BCflag { freespace, periodic, wall }  (main.cpp:6081) */
enum { CUP3D_BC_FREESPACE = 0, CUP3D_BC_PERIODIC = 1, CUP3D_BC_WALL = 2 };
/* fields of SimulationData (main.cpp:6603-6607) */
enum { CUP3D_FIELD_CHI = 0, CUP3D_FIELD_PRES = 1, CUP3D_FIELD_VEL = 2, CUP3D_FIELD_TMPV = 3, CUP3D_FIELD_LHS = 4 };

/* ---------------------------------------------------------------------------
 * Indexing (host, integer, bit-exact contract).
 * Replaces class SpaceFillingCurve (main.cpp:95-319) and Info::setup (384-420).
 * ------------------------------------------------------------------------- */
typedef struct cup3d_sfc cup3d_sfc_t;
CUP3D_API int cup3d_sfc_create(int bpdx, int bpdy, int bpdz, int level_max, cup3d_sfc_t **out);   /* ctor 196-236 */
CUP3D_API void cup3d_sfc_destroy(cup3d_sfc_t *);
CUP3D_API long long cup3d_sfc_forward(const cup3d_sfc_t *, int level, int i, int j, int k);       /* 237-255 */
CUP3D_API void cup3d_sfc_inverse(const cup3d_sfc_t *, long long Z, int level, int ijk[3]);        /* 256-276 */
CUP3D_API long long cup3d_sfc_encode(const cup3d_sfc_t *, int level, const int index[3]);         /* 287-318 (blockID_2) */
/* Info::setup neighbour / child / parent ids: nei[27] as Znei[i+1][j+1][k+1] */
CUP3D_API void cup3d_sfc_info(const cup3d_sfc_t *, int level, const int index[3], long long nei[27], long long child[8],
                    long long *parent);

/* ---------------------------------------------------------------------------
 * Block topology of one rank (host).  Replaces the parts of Grid / GridMPI the hot
 * path needs: block ownership by contiguous Hilbert ranges (GridMPI ctor,
 * main.cpp:2959-2986), m_vInfo ordering (FillPos 943-964), neighbour lookup
 * (Info::Znei + Tree().rank(), 384-420, 840-855) and the inner/halo block split of
 * SynchronizerMPI_AMR::_Setup (1979-2286) reduced to what face-only stencils need.
 * ------------------------------------------------------------------------- */
typedef struct cup3d_grid cup3d_grid_t;
/* uniform grid at `level` (< level_max) of a bpd[0] x bpd[1] x bpd[2] level-0 block box;
 * maxextent = SimulationData::maxextent (15401); bc[d] per axis; this rank owns the
 * Z range of GridMPI's constructor. */
CUP3D_API int cup3d_grid_create_uniform(const int bpd[3], int level_max, int level, double maxextent, const int bc[3],
                              int rank, int nranks, cup3d_grid_t **out);
/* multi-level (AMR) mesh on one rank from its leaf blocks (level, Z) in any order: the block set Grid::m_vInfo holds
 * after MeshAdaptation::Adapt (main.cpp:5086-5159).  Blocks are ordered by blockID_2; the octree states
 * (Exists / CheckCoarser / CheckFiner, 321-330) follow from the leaf set; the mesh must be 2:1 balanced. */
CUP3D_API int cup3d_grid_create_mesh(const int bpd[3], int level_max, double maxextent, const int bc[3], long nleaves,
                           const int32_t *levels, const int64_t *Zs, cup3d_grid_t **out);
/* interface faces of a multi-level mesh (faces whose same-level neighbour does not exist, FluxCorrection::prepare
 * 676-711): faces2[e] = {6*slot + face, kind} with kind 0 = neighbour coarser, 1 = neighbour finer; fine4[e] = interface-face
 * indices of the four finer blocks' opposite faces (FillCase 601-661), -1 for kind 0; nbr27[slot][27] = neighbour states
 * (same-level slot, CUP3D_NBR_COARSER + slot, CUP3D_NBR_SKIPPED, CUP3D_NBR_FINER).  Any output may be NULL. */
#define CUP3D_NBR_COARSER 0x20000000
#define CUP3D_NBR_SKIPPED (-1)
#define CUP3D_NBR_FINER (-3)
CUP3D_API long cup3d_grid_ninterface_faces(const cup3d_grid_t *);
CUP3D_API int cup3d_grid_interface(const cup3d_grid_t *, int32_t *faces2, int32_t *fine4, int32_t *nbr27);
/* Mesh adaptation decisions (integer contract; one rank).  cup3d_grid_valid_states = MeshAdaptation::ValidStates
 * (main.cpp:5330-5492): in/out states[nblocks] in {-1 Compress, 0 Leave, 1 Refine} (e.g. from cup3d_tag_blocks):
 * refinement propagates to coarser neighbours to keep the mesh 2:1 balanced, unbalanced or partial compressions are
 * dropped.  cup3d_grid_adapted = the mesh MeshAdaptation::Adapt (5086-5159) produces from valid states (a new grid object,
 * always of the multi-level kind); cup3d_adapt_transfer (below) moves the field data. */
CUP3D_API int cup3d_grid_valid_states(const cup3d_grid_t *, signed char *states);
CUP3D_API int cup3d_grid_adapted(const cup3d_grid_t *, const signed char *states, cup3d_grid_t **out);
/* Ownership of the adapted mesh's leaves on several ranks = what MeshAdaptation::Adapt + LoadBalancer (main.cpp:4660-5022, 5086-5159)
 * leave behind: children on the refined parent's rank, a compressed octet's parent on the rank of its base block (even indices;
 * PrepareCompression 4729-4804), then Balance_Diffusion (4805-4905: (my - neighbour)/4 blocks to each neighbour) or, when
 * max/min > 1.01 or a rank is empty, Balance_Global (4906-5021: even cut of the rank-major order).  `mesh`: all leaves of all ranks
 * (cup3d_grid_create_mesh), owner[nblocks] their ranks, states the valid states, adapted = cup3d_grid_adapted(mesh, states);
 * new_owner[nblocks of adapted].  cup3d_adapt_migrate (below) moves the field data accordingly. */
CUP3D_API int cup3d_grid_adapted_owners(const cup3d_grid_t *mesh, const int32_t *owner, const signed char *states, int nranks,
                              const cup3d_grid_t *adapted, int32_t *new_owner);
/* One rank's view of a multi-level mesh whose leaves are spread over several ranks (what SynchronizerMPI_AMR::_Setup 1979-2286 and
 * FluxCorrectionMPI::prepare 2680-2824 derive from the shared octree): block slots [0, nlocal) are the rank's own leaves, then GHOST
 * leaves -- every remote leaf the neighbour tables of a local block refer to -- ordered by (owner, global order); interface faces:
 * the local blocks' first, then the fine faces of ghost blocks whose fluxes / cells the local coarse-side faces need.  The tables
 * (cup3d_grid_neighbours, cup3d_grid_interface) are the global ones renumbered, so a kernel reads through them what it would read on
 * one rank once the two exchanges of cup3d_grid_view_plan have run; cup3d_sim_create on a view allocates the ghost slots and the
 * operators run those exchanges over RCCL (ghost blocks before a stencil kernel -- of each only the sub-box the stencil's consumers read,
 * cup3d_grid_view_boxes; whole blocks for the tensorial tiles of mesh adaptation --, face fluxes after a flux-corrected one). */
CUP3D_API int cup3d_grid_rank_view(const cup3d_grid_t *mesh, const int32_t *owner, int rank, int nranks, cup3d_grid_t **view);
/* out: local blocks, ghost blocks, local interface faces, ghost faces, blocks sent per exchange, face-flux arrays sent per exchange */
CUP3D_API int cup3d_grid_view_sizes(const cup3d_grid_t *view, long out[6]);
/* any pointer may be NULL.  global_slot[nlocal+nghost], global_face[nfaces]: position in the global mesh; send_blocks[]: local slots in
 * peer-major order (each peer's run in that peer's ghost order), counts per rank; the same for the face-flux arrays */
CUP3D_API int cup3d_grid_view_plan(const cup3d_grid_t *view, int32_t *global_slot, int32_t *global_face, int32_t *send_blocks, long *send_block_count,
                         long *recv_block_count, int32_t *send_flux_faces, long *send_flux_count, long *recv_flux_count);
/* The sub-box form of the ghost-block exchange (what SynchronizerMPI_AMR ships: face sub-boxes and coarse shadow cells, main.cpp:1832-1966,
 * 2423-2544): of every ghost block only the bounding box of the cells the rank's star-stencil consumers read travels -- the w layers behind
 * a shared face, the 2w layers a restriction averages, the cells of the coarse shadow patch of an interpolation.  width_class 0: stencil
 * width 1, 1: width 3.  ghost_box[nghost][6], send_box[blocks sent][6] = lo x, y, z, hi x, y, z (hi exclusive; all zero: nothing of the
 * block is read); send_cells[nranks] / recv_cells[nranks]: cells per component to / from every rank.  Any pointer may be NULL. */
CUP3D_API int cup3d_grid_view_boxes(const cup3d_grid_t *view, int width_class, unsigned char *ghost_box, unsigned char *send_box, long *send_cells, long *recv_cells);
CUP3D_API void cup3d_grid_destroy(cup3d_grid_t *);
CUP3D_API long cup3d_grid_nblocks(const cup3d_grid_t *);        /* local blocks = m_vInfo.size() */
CUP3D_API long cup3d_grid_nblocks_global(const cup3d_grid_t *);
CUP3D_API long cup3d_grid_nhalo_faces(const cup3d_grid_t *);    /* remote face slabs this rank receives */
CUP3D_API long cup3d_grid_ninner(const cup3d_grid_t *);         /* blocks with no remote neighbour (Synchronizer inner_blocks) */
/* per local block, m_vInfo order: tab6 = level, Z, index[3], blockID_2 ; geom4 = h, origin[3] (Info 331-346) */
CUP3D_API int cup3d_grid_tables(const cup3d_grid_t *, long long *tab6, double *geom4);
/* face neighbour table nbr[nblocks][6] (faces x-,x+,y-,y+,z-,z+): >=0 local slot,
 * CUP3D_NBR_HALO + e = remote slab e, CUP3D_NBR_BC - bc = domain face with that BC */
#define CUP3D_NBR_HALO 0x40000000
#define CUP3D_NBR_BC (-1)
CUP3D_API int cup3d_grid_neighbours(const cup3d_grid_t *, int32_t *nbr);
/* halo-exchange plan (what SynchronizerMPI_AMR::_Setup computes, 1979-2286): for peer
 * p in [0,nranks): number of face slabs sent to / received from p; send_faces[s] =
 * local_slot*6+face of the s-th slab sent (peer-major, then (Z,face) of the sender's
 * block); received slabs are numbered in the same peer-major order. */
CUP3D_API int cup3d_grid_halo_plan(const cup3d_grid_t *, long *send_count, long *recv_count, int32_t *send_faces);
CUP3D_API long cup3d_grid_nsend_faces(const cup3d_grid_t *);

/* Simulation::calcMaxTimestep (main.cpp:15254-15305), explicit diffusion, CFL > 0;
 * updates coefU when step > step_2nd_start. */
CUP3D_API double cup3d_calc_max_timestep(double hmin, double umax, double nu, double cfl, int step, int rampup, double dt_old,
                               double coefU[3]);
/* the same with sim.implicitDiffusion: the diffusive limit becomes 0.1 once step > 10 (15269-15273) */
CUP3D_API double cup3d_calc_max_timestep2(double hmin, double umax, double nu, double cfl, int step, int rampup, double dt_old,
                                double coefU[3], int implicit_diffusion);

/* ---------------------------------------------------------------------------
 * Device side.
 * ------------------------------------------------------------------------- */
CUP3D_API int cup3d_device_count(int *n);
CUP3D_API int cup3d_device_init(int device);            /* hipSetDevice; fails loudly unless the device is gfx950 */
CUP3D_API int cup3d_set_stream(void *hip_stream);       /* compute stream for all launches (NULL = default stream) */
CUP3D_API int cup3d_device_synchronize(void);

/* RCCL communicator owned by the library (replaces sim.comm's role on the hot path:
 * halo Isend/Irecv 2370/2402 and the Allreduce/Iallreduce sites 8620, 9295, 14442,
 * 14486, 14546, 14584, 15123).  id is the 128-byte ncclUniqueId from rank 0. */
/* COLLECTIVES AND ERRORS.  On a grid that spans several ranks every operator entry point is a collective: all ranks call it, in the
 * same order (the library issues its RCCL calls from one stream per rank in that order).  A non-zero status on ONE rank -- a bad
 * argument, a HIP error -- leaves the others inside the collective, exactly as a failing rank does under the reference's MPI: treat any
 * non-zero status as fatal for the job, as the reference does (MPI_Abort at 8444, 15265, 15289; the C++ shim's CUP3D_HIP_CALL and
 * torch.distributed.run's process group do that for their hosts).  There is no rank-local error recovery. */
/* ENVIRONMENT (read once per process, the same on every rank).  CUP3D_RCCL_LIBRARY=<path>: the RCCL to dlopen instead of the one the
 * process has loaded / the loader finds.  CUP3D_EARLY_ALLREDUCE=1: the two all-reduces of a BiCGSTAB iteration (main.cpp:14486, 14546) start
 * when the loop kernel's last block has left its vector phase instead of when the kernel has ended -- they then run under its block solves,
 * as MPI_Iallreduce runs under the preconditioner in the reference; uniform grids, block CG, one process per device; the dot products are
 * added in another (deterministic) order than by default.  Off unless set. */
CUP3D_API int cup3d_comm_unique_id(void *id128);
CUP3D_API int cup3d_comm_init(int rank, int nranks, const void *id128);
CUP3D_API int cup3d_comm_finalize(void);

typedef struct cup3d_sim cup3d_sim_t; /* device mirror of SimulationData's five grids + solver vectors */
CUP3D_API int cup3d_sim_create(const cup3d_grid_t *, cup3d_sim_t **out);
CUP3D_API void cup3d_sim_destroy(cup3d_sim_t *);
CUP3D_API size_t cup3d_sim_device_bytes(const cup3d_sim_t *);
/* host <-> device; host side is the reference's block memory: either one pointer per
 * block (Info::block, main.cpp:343, 877-884) or one contiguous array [nb][8][8][8][nc] */
CUP3D_API int cup3d_sim_upload_blocks(cup3d_sim_t *, int field, const void *const *block_ptrs);
CUP3D_API int cup3d_sim_download_blocks(cup3d_sim_t *, int field, void *const *block_ptrs);
/* the same for a subset: only the n listed block slots move (slots[i] <-> block_ptrs[i]).  Lets the host-side obstacle operators
 * (UpdateObstacles / Penalization, which touch only the blocks an obstacle covers, 13841-13912) run between two device operators
 * without a full-field round trip */
CUP3D_API int cup3d_sim_upload_block_list(cup3d_sim_t *, int field, long n, const int32_t *slots, const void *const *block_ptrs);
CUP3D_API int cup3d_sim_download_block_list(cup3d_sim_t *, int field, long n, const int32_t *slots, void *const *block_ptrs);
/* BlockLab::load + post_load (main.cpp:3623-3787) for the listed blocks: tiles [n][L][L][L][nc], L = 8 + 2*width,
 * box [-width, width+1), width 1..4; slots = NULL: all local blocks in slot order.
 * scalar_dir: -1 = the field's own lab (VectorLab for vel/tmpV, ScalarLab for scalar fields);
 *             0..2 = scalar field as BlockLabBC<.., direction> (implicit diffusion).
 * The tile is the reference's Matrix3D: x fastest, component innermost; same-level ghosts copied, finer neighbours averaged down,
 * coarser ones interpolated (TestInterp / the finite-difference mode), domain faces last, bit for bit.  tensorial = 0 with width <= 2
 * is the star tile: its edge and corner ghosts, which the reference leaves undefined, are quiet NaN.  What lets a host functor that
 * needs the [s,e) tiles of a few blocks (ComputeForces reads [-4,5) around an obstacle, 12250-12503) get them without downloading
 * a field: 98 304 B per [-4,5) vector tile.  Repeated and unordered slots are allowed.  Both variants launch the same kernel on the
 * compute stream (cup3d_set_stream); the host variant stages through a bounded device buffer of the sim, counts its bytes in
 * cup3d_run_stats.field_bytes_downloaded and synchronises before it returns; the device variant is stream-ordered and does not.
 * CUP3D_EINVAL, nothing touched: width outside 1..4, unknown field, NULL output, slot outside [0, nblocks), n != nblocks with
 * slots = NULL, scalar_dir >= 0 on a vector field, a sim on a rank view or on one rank's share of a uniform grid (tiles whose
 * neighbours live on another rank come from cup3d_sim_labs_over_ranks below). */
CUP3D_API int cup3d_sim_labs(cup3d_sim_t *, int field, long n, const int32_t *slots, int width, int tensorial, int scalar_dir, double *host_out);
CUP3D_API int cup3d_sim_labs_device(cup3d_sim_t *, int field, long n, const int32_t *slots, int width, int tensorial, int scalar_dir, void *device_out);
/* The same tiles on a mesh spread over ranks: what BlockLabMPI::load (main.cpp:4648-4658) gets from SynchronizerMPI_AMR::fetch
 * (2423-2544).  mesh / owner: the GLOBAL multi-level mesh object and the rank of every leaf, as for cup3d_adapt_migrate; the sim is this
 * rank's, on its cup3d_grid_rank_view of that mesh or on its share of a uniform grid (cup3d_grid_create_uniform(.., rank, nranks): pass
 * the same level as a one-level mesh from cup3d_grid_create_mesh, owner = the contiguous Z-range partition).  slots are LOCAL slots of
 * the sim exactly as for cup3d_sim_labs (NULL with n = nblocks: every local block; repeated and unordered slots allowed); width,
 * tensorial, scalar_dir, the tile layout and the NaN cells of star tiles are those of cup3d_sim_labs, and a tile does not depend on how
 * the mesh is partitioned.  COLLECTIVE: every rank of the communicator calls it with the same field, width and tensorial and its own
 * n / slots; a rank that needs nothing passes n = 0 (slots and the output may then be NULL).  Only what the requested tiles read
 * travels, and of each remote block only the bounding box of the cells read: per call each rank sends every owner one double per ghost
 * block of its tensorial view (the box, 0 for nothing), then the owners send the boxes' cells; both count in
 * cup3d_run_stats.halo_bytes_sent.  The view and its tables are kept in the sim between calls while mesh and owner say the same
 * (compared by content).  Errors one rank can find on its own -- NULL mesh / owner, a rank view in `mesh`'s place, an owner out of range,
 * a bad width / field / slot / scalar_dir, a sim whose local blocks are not, (level, Z) by (level, Z), this rank's leaves of `mesh` -- are
 * agreed over the ranks before anything is exchanged: every rank returns the failure and nothing has been touched.  The call waits for
 * the received requests on the host; the device variant's tiles are stream-ordered on the compute stream behind that.  On one rank
 * both give what cup3d_sim_labs gives. */
CUP3D_API int cup3d_sim_labs_over_ranks(cup3d_sim_t *, const cup3d_grid_t *mesh, const int32_t *owner, int field, long n, const int32_t *slots, int width,
                                        int tensorial, int scalar_dir, double *host_out);
CUP3D_API int cup3d_sim_labs_over_ranks_device(cup3d_sim_t *, const cup3d_grid_t *mesh, const int32_t *owner, int field, long n, const int32_t *slots,
                                               int width, int tensorial, int scalar_dir, void *device_out);
CUP3D_API int cup3d_sim_upload(cup3d_sim_t *, int field, const double *blocks);
CUP3D_API int cup3d_sim_download(cup3d_sim_t *, int field, double *blocks);
CUP3D_API int cup3d_sim_fill(cup3d_sim_t *, int field, double value);
/* raw device pointer of a field slab [nb][nc][512] (for zero-copy hosts).  The VEL pointer is valid until the next operator that
 * advects (cup3d_advect_diffuse, cup3d_advect_diffuse_implicit, cup3d_advect_implicit): those write the new velocity into a second
 * buffer and swap the two, so re-query it after every such call; the other fields never move. */
CUP3D_API int cup3d_sim_device_ptr(cup3d_sim_t *, int field, void **ptr);
/* A host that WRITES a field through that pointer must say so afterwards: the library tracks two facts the operators branch on --
 * "chi is non-zero" (KernelPressureRHS then reads chi and udef, main.cpp:14858-14871) and "tmpV holds the udef of the next
 * projection" (otherwise cup3d_pressure_project clears tmpV as the reference does at 15076-15078) -- and upload / fill /
 * cup3d_update_tmpv set them, stores through a raw pointer cannot.  CHI and TMPV are the fields that matter; others are accepted. */
CUP3D_API int cup3d_sim_mark_written(cup3d_sim_t *, int field);
/* Does ANY rank hold an obstacle?  The reference's obstacle_vector is replicated on every rank (sim.obstacle_vector->nObstacles(),
 * main.cpp:15081), so the host knows without communicating; the same value on every rank (it decides whether the collective udef
 * exchange of the pressure right-hand side runs).  1: chi / udef path (KernelPressureRHS 14858-14871); 0: obstacle-free path, no udef
 * exchange, tmpV not cleared; -1 (default): not told -- one rank decides by "chi was written", several ranks always take the chi path.
 * A chi written (upload / fill / mark_written) is never dropped silently: on one rank it takes the chi path even after 0; on several
 * ranks cup3d_pressure_project refuses the combination on EVERY rank: CUP3D_ESTATE on all of them together, agreed inside the
 * mean-pressure all-reduce the operator performs anyway (15123) -- i.e. AFTER the Poisson solve.  The simulation state is then
 * UNDEFINED (pres, the previous-pressure copy, lhs and tmpV have been overwritten; vel has not been projected): the host must end the
 * run or re-upload its fields, exactly as after the MPI_Abort the reference answers an inconsistent run with (15265, 15289). */
CUP3D_API int cup3d_sim_set_obstacles(cup3d_sim_t *, int any_rank_has_obstacles);
/* Wrapping 64-bit sum of the bit patterns of every FP64 value of the rank's own blocks of `field` (ghost blocks of a rank view
 * excluded).  Integer addition commutes, so the sum of the ranks' values is independent of the partition: bench.py all-gathers it
 * after the first AdvectionDiffusion and compares it with the constant the CPU oracle produced for the same step (the stencil
 * operators are bit-exact under any sharding; the reference's own partition is main.cpp:2970-2986). */
CUP3D_API int cup3d_sim_checksum(cup3d_sim_t *, int field, unsigned long long *sum);

/* AdvectionDiffusion::operator()(dt) (main.cpp:9640-9728): low-storage RK3 of
 * KernelAdvectDiffuse (9461-9549) on vel, scratch tmpV; fused into 3 launches. */
CUP3D_API int cup3d_advect_diffuse(cup3d_sim_t *, double dt, double nu, const double uinf[3]);
/* findMaxU (main.cpp:8603-8623) incl. the MAX all-reduce */
CUP3D_API int cup3d_max_u(cup3d_sim_t *, const double uinf[3], double *umax);
/* ExternalForcing::operator() (main.cpp:10581-10596): vel.u[0] += 8*uMax*nu/H/H*dt */
CUP3D_API int cup3d_external_forcing(cup3d_sim_t *, double umax_forced, double nu, double H, double dt);

typedef struct {
  double tol;          /* sim.PoissonErrorTol     (-poissonTol, 1e-6)    */
  double tol_rel;      /* sim.PoissonErrorTolRel  (-poissonTolRel, 1e-4) */
  int mean_constraint; /* sim.bMeanConstraint     (-bMeanConstraint, 1)  */
  int max_iter;        /* 1000 (main.cpp:14449) */
  int max_restarts;    /* 100  (main.cpp:14374) */
  int block_solver;    /* how the block preconditioner M^-1 (getZImplParallel, 14704-14745) is evaluated:
                          0 = the reference's block-local CG, iteration for iteration, as the device evaluates it fastest: a*b+c
                              contracted to FMA (wave-wide sums by DPP reductions, divisions by v_rcp_f64 + Newton steps, within
                              1 ulp of IEEE).  Differs from the reference's z
                              by less than the CG's own 1e-7 truncation (tests: measured against block_solver 2 and the reference);
                          1 = direct block solve by fast diagonalisation (same operator, exact to rounding);
                          2 = the block CG in the reference's association: no FMA contraction (only the ORDER of the 512-term sums
                              differs from the CPU); slower, for parity checks;
                          3, 4 = A/B timing variants (3: 0's evaluation of rounds 1-5, IEEE divisions; 4: two blocks per wavefront), libcup3d_hip_testing.so only;
                          5 = NOT the reference's preconditioner: one geometric-multigrid V(2,2)-cycle (red-black Gauss-Seidel in LDS,
                              summed-residual restriction, piecewise-constant prolongation) on the hierarchy of uniform block grids --
                              same operator, same stopping rule, same converged pressure to solver tolerance, O(10) instead of O(150)
                              iterations; uniform grids (over several ranks ONE cycle coupled over the ranks: every level is partitioned
                              like the solver's grid and its iterate crosses ranks as face slabs before each launch that reads
                              ghosts) and multi-level meshes (the octree's levels; over ranks: rank views, ghost nodes exchanged before
                              every launch that reads them); bench.py: `alt_multigrid` only */
} cup3d_poisson_params;
typedef struct {
  int iterations; /* BiCGSTAB iterations performed (= 7-double reductions, main.cpp:14546) */
  int restarts;
  double norm0, norm; /* ||r0||, last ||r|| */
  int used_xopt;
} cup3d_poisson_result;
CUP3D_API void cup3d_poisson_default_params(cup3d_poisson_params *);

/* ComputeLHS::operator() (main.cpp:9273-9327): lhs = h*(sum6 - 6p) of pres + mean constraint */
CUP3D_API int cup3d_compute_lhs(cup3d_sim_t *, int mean_constraint);
/* poisson_kernels::getZImplParallel (main.cpp:14704-14745): block preconditioner on pres, in place;
 * block_solver as in cup3d_poisson_params -- EVERY value works in place, 5 (one multigrid V-cycle) included: pres holds M^-1 of
 * what it held, on uniform grids and multi-level meshes, on one rank and over ranks */
CUP3D_API int cup3d_preconditioner(cup3d_sim_t *, int block_solver);
/* PoissonSolverBase::solve() (main.cpp:8921-8928; PoissonSolverAMR::solve 14363-14616):
 * RHS in lhs, initial guess and result in pres; lhs is clobbered. */
CUP3D_API int cup3d_poisson_solve(cup3d_sim_t *, const cup3d_poisson_params *, cup3d_poisson_result *);
/* KernelPressureRHS via compute<> (main.cpp:15083-15085): lhs from vel, tmpV(=udef), chi */
CUP3D_API int cup3d_pressure_rhs(cup3d_sim_t *, double dt);
/* KernelDivPressure (main.cpp:15088): tmpV.u[0] = h * lap(pres) */
CUP3D_API int cup3d_div_pressure(cup3d_sim_t *);
/* KernelGradP (main.cpp:15146): tmpV = -0.5*dt*h^2 * central grad(pres) */
CUP3D_API int cup3d_grad_p(cup3d_sim_t *, double dt);
/* PressureProjection::operator()(dt) (main.cpp:15061-15160), obstacle-free or with
 * chi/udef already resident: tmpV must hold udef (upload / fill / cup3d_update_tmpv after the previous projection); if it was not
 * touched since, it is zeroed as at 15076-15078. */
CUP3D_API int cup3d_pressure_project(cup3d_sim_t *, double dt, int step, const cup3d_poisson_params *, cup3d_poisson_result *);

/* ---------------------------------------------------------------------------
 * Mesh-adaptation block operators (data movement of MeshAdaptation, main.cpp:5023-5583) for
 * whole-mesh transitions between two uniform levels l (coarse) and l+1 (fine) of the same box.
 * The integer decisions (which blocks to refine, 2:1 balancing, load balancing) stay on the host.
 * ------------------------------------------------------------------------- */
/* "restrict": MeshAdaptation::compress (5272-5329): every sibling octet of `fine` -> its parent block of `coarse` */
CUP3D_API int cup3d_restrict(cup3d_sim_t *fine, cup3d_sim_t *coarse, int field);
/* "prolong": refine_1 + RefineBlocks (5227-5249, 5493-5565): every block of `coarse` -> its eight children in `fine` */
CUP3D_API int cup3d_prolong(cup3d_sim_t *coarse, cup3d_sim_t *fine, int field);
/* TagLoadedBlock (5566-5582) + level clamps (5207-5211): states[nblocks] in {-1 Compress, 0 Leave, 1 Refine} (enum State, 320);
 * any mesh (uniform or multi-level).  With ComputeVorticity this is the device half of Simulation::adaptMesh's decision input
 * (15180-15183, obstacle-free: GradChiOnTmp only reads chi); ValidStates' 2:1 balancing of the tags stays on the host. */
CUP3D_API int cup3d_tag_blocks(cup3d_sim_t *, int field, double rtol, double ctol, signed char *states);
/* field `field` of `src` onto the mesh of `dst` (MeshAdaptation::Adapt for one grid, basic = false): blocks present in both
 * are copied, children of a refined block come from refine_1 + RefineBlocks (5227-5249, 5493-5565: 2nd-order Taylor
 * expansion from the parent's tensorial [-1,2) tile on the OLD mesh, coarse/fine ghosts included), the parent of a
 * compressed octet from compress (5272-5329).  Every block of dst must be a block, a child or the parent of blocks of src. */
CUP3D_API int cup3d_adapt_transfer(cup3d_sim_t *src, cup3d_sim_t *dst, int field);
/* The same over ranks: MeshAdaptation::Adapt plus the block traffic of the LoadBalancer (PrepareCompression 4729-4804, Balance_Diffusion
 * 4805-4905, Balance_Global 4906-5021) for one field.  old_mesh / new_mesh: the GLOBAL mesh objects before and after (cup3d_grid_adapted),
 * old_owner / new_owner: the rank of every leaf (new_owner from cup3d_grid_adapted_owners); src / dst: this rank's sims on its views of
 * the two (cup3d_grid_rank_view).  Collective over the ranks of the communicator.  Each block of the new mesh is built by the rank that
 * owns its origin in the old mesh (the leaf itself, the refined parent, or the base block of a compressed octet) and sent straight to its
 * new owner; the result equals the one-rank cup3d_adapt_transfer bit for bit, block by block. */
CUP3D_API int cup3d_adapt_migrate(const cup3d_grid_t *old_mesh, const int32_t *old_owner, cup3d_sim_t *src, const cup3d_grid_t *new_mesh,
                        const int32_t *new_owner, cup3d_sim_t *dst, int field);
/* Obstacle operators (the obstacles themselves -- geometry, i.e. the signed distance and the deformation velocity, and the rigid-body
 * integration -- stay on the host; cup3d_create_obstacles below turns the signed distance into chi, surface points and corrected udef).
 * One cup3d_obstacle = the ObstacleBlocks of one Obstacle on this rank in the reference's own layout (struct ObstacleBlock,
 * main.cpp:7256-7263) plus its rigid motion. */
typedef struct {
  long nblocks;          /* number of non-null entries of Obstacle::obstacleBlocks */
  const int32_t *slots;  /* [nblocks] their block slots (= Info::blockID) */
  const double *chi;     /* [nblocks][8][8][8]     ObstacleBlock::chi */
  const double *udef;    /* [nblocks][8][8][8][3]  ObstacleBlock::udef */
  double cm[3], vel[3], omega[3]; /* getCenterOfMass(), getTranslationVelocity(), getAngularVelocity() */
  double force[3], torque[3];     /* out of cup3d_penalization: Obstacle::force / torque (13932-13937) */
} cup3d_obstacle;
/* Penalization::operator() without the collision model (14330-14340): KernelPenalization (13841-13912) on the resident vel with
 * the resident chi, obstacle after obstacle, then kernelFinalizePenalizationForce (13913-13938).  The collision model it begins with
 * (preventCollidingObstacles, 14329) is cup3d_prevent_colliding_obstacles below: call that first where bodies may touch. */
CUP3D_API int cup3d_penalization(cup3d_sim_t *, double dt, double lambda, int implicit_penalization, int nobstacles, cup3d_obstacle *obstacles);
/* kernelUpdateTmpV (14948-14979): tmpV += udef where chi <= the obstacle's chi; call after clearing tmpV and before
 * cup3d_pressure_rhs / cup3d_pressure_project (15066-15085) */
CUP3D_API int cup3d_update_tmpv(cup3d_sim_t *, int nobstacles, const cup3d_obstacle *obstacles);
/* UpdateObstacles::operator() (13812-13837): the operator between the forcing and Penalization (setupOperators 15229-15246) that turns
 * the freshly advected velocity inside an obstacle into the obstacle's translation and angular velocity -- the two that
 * cup3d_penalization takes.  Per obstacle, obstacles one after the other (13739):
 *   KernelIntegrateFluidMomenta<0/1>::visit (13637-13734) on the device from the resident vel and the staged chi / udef: per ObstacleBlock
 *     the 29 sums in the order kernelFinalizeObstacleVel packs M (13748-13777) -- V, FX FY FZ, TX TY TZ, J0..J5, then GfX, GpX GpY GpZ,
 *     Gj0..Gj5, GuX GuY GuZ, GaX GaY GaZ -- cells added in iz, iy, ix order, those with chi <= 0 skipped, in the reference's association:
 *     bit for bit what the reference leaves in the ObstacleBlock.  Without implicit_penalization only the first 13 are computed.
 *   one download of [nblocks][29] doubles (counted in cup3d_run_stats.field_bytes_downloaded) instead of the blocks' velocity;
 *   kernelFinalizeObstacleVel (13737-13811) on the host: the block rows added in ascending slot order whatever order `slots` has (the
 *     reference's loop with one thread), the all-reduce over ranks (13783), penalM / penalCM / penalJ / penalLmom / penalAmom by the two
 *     branches of 13796-13808;
 *   Obstacle::computeVelocities (12921-13068) on the host: the 6 x 6 matrix as written there, the bForcedInSimFrame / bBlockRotation row
 *     edits, a dense LU with partial pivoting of this library's own (no GSL).
 * On return obstacles[k].vel / omega hold the new transVel / angVel -- forced components equal vel_imposed, blocked rotations are 0,
 * everything else is the computed value (13039-13068) -- and the same array goes straight into cup3d_penalization.  vel is only read.
 * LEFT TO THE HOST: the force / torque of 13030-13038 (Penalization overwrites them), bBreakSymmetry's edit of transVel_imposed
 * (12961-12966: pass the edited value), the collision override (13069 ff.: the stored velocities of cup3d_prevent_colliding_obstacles while
 * collision_counter > 0), and the asserts on mass and J (13788-13794).
 * COLLECTIVE like cup3d_penalization: every rank calls it with the same nobstacles; a rank that holds none of an obstacle's blocks passes
 * nblocks = 0.  Per obstacle the 29 totals and an error flag cross the ranks as two all-reduces of at most 16 values from a device buffer
 * of the call's own: a rank whose own arguments fail returns its own code, the others CUP3D_ECOMM, and every rank returns.
 * CUP3D_EINVAL, nothing touched (neither motion[] nor obstacles[k].vel / omega, of any obstacle of the call): a null handle, dt <= 0,
 * nobstacles < 0, null obstacles or motion with nobstacles > 0, nblocks < 0, a null array with nblocks > 0, a slot outside [0, nblocks of
 * the sim), and -- after the all-reduce, so on every rank alike -- a total volume totals[0] <= DBL_EPSILON (the reference's
 * assert(M[0] > EPS), 13795).  nobstacles = 0 is a no-op. */
typedef struct {
  int forced[3];           /* Obstacle::bForcedInSimFrame */
  int block_rotation[3];   /* Obstacle::bBlockRotation */
  double vel_imposed[3];   /* Obstacle::transVel_imposed */
  double *block_sums;      /* out, may be NULL: [nblocks][29], order above; columns 13..28 written only with implicit_penalization */
  double totals[29];       /* out: M after the sum over blocks and ranks (13783); 13..28 are 0 without implicit_penalization */
  double vel_computed[3], omega_computed[3];   /* out: transVel_computed / angVel_computed (13022-13027) */
} cup3d_obstacle_motion;
CUP3D_API int cup3d_update_obstacles(cup3d_sim_t *, double dt, double lambda, int implicit_penalization, int nobstacles,
                                     cup3d_obstacle *obstacles, cup3d_obstacle_motion *motion);
/* The grid half of CreateObstacles::operator() (main.cpp:13596-13619), the first operator of the obstacle step: what the host's geometry
 * left in ObstacleBlock::sdfLab and ObstacleBlock::udef becomes everything the operators above take -- the blocks' chi, the resident chi
 * field, the momentum-corrected udef, the centre of mass and the surface list cup3d_compute_forces reads.  One cup3d_obstacle_shape = the
 * ObstacleBlocks of one Obstacle on this rank.  In the reference's order, obstacles one after the other:
 *   the resident chi of every block of the sim is set to 0 (13596-13600);
 *   KernelCharacteristicFunction::operate (13298-13403) on the device, one wavefront per ObstacleBlock: chi by the |sdf| > h test or the
 *     band formula, resident chi = std::max(chi, resident), the four sums mass, CoM_x, CoM_y, CoM_z over all 512 cells in z, y, x order,
 *     and the surface points -- one-sided gradH at index 0 and 7, the < 1e-12 and Delta > EPS tests, dchi = -delta * gradU (7426-7428)
 *     -- in the reference's push_back order: cells in z, y, x, blocks in the order listed.  Bit for bit what the reference computes;
 *   kernelComputeGridCoM (13406-13425) on the host: block rows added in ascending slot order, all-reduced;
 *   _kernelIntegrateUdefMomenta (13426-13488) on the device with that centre of mass and transvel_correction as passed in (oldCorrVel):
 *     per block V, FX FY FZ, TX TY TZ, J0..J5, cells with chi <= 0 skipped, bit for bit;
 *   kernelAccumulateUdefMomenta (13495-13550) on the host: rows in ascending slot order, all-reduced, invertSym with its detJ guard;
 *   kernelRemoveUdefMomenta (13551-13588) on the device, then chi, udef and the surface come back.
 * DOWNLOADS (cup3d_run_stats.field_bytes_downloaded), per obstacle of nblocks blocks and npoints = first[nblocks] surface points:
 * nblocks * (4*8 + 4) for the blocks' mass / CoM rows and point counts, nblocks * 13*8 for their momenta, nblocks * 2048*8 for chi and
 * udef, npoints * (3*4 + 4*8) for ijk, dchi and delta: only the points that exist cross the host boundary.
 * LEFT TO THE HOST: updateUinf, update() and create() (the geometry: sdfLab and udef), finalize() (empty in Obstacle), the MeshChanged /
 * StaticObstacles gate (13592-13594), and ObstacleBlock::allocate_surface.
 * COLLECTIVE like cup3d_update_obstacles: every rank calls it with the same nobstacles; a rank that holds none of an obstacle's blocks
 * passes nblocks = 0.  Per obstacle the 4 and the 13 totals travel with an error flag in two all-reduces of at most 16 values from a
 * device buffer of the call's own: a rank whose own arguments are refused still takes part and returns its own code, the others
 * CUP3D_ECOMM, and every rank returns.
 * CUP3D_EINVAL: a null handle, nobstacles < 0, null shapes with nobstacles > 0, nblocks < 0, a null slots / sdf / udef / chi / first /
 * ijk / dchi / delta with nblocks > 0, a slot outside [0, nblocks of the sim) -- all checked before anything is written, on the device or
 * the host -- and, after the all-reduces and so on every rank alike, com_totals[0] <= DBL_EPSILON or udef_totals[0] <= DBL_EPSILON (the
 * reference's asserts, 13420 and 13520).  A refused call writes nothing of the caller's, for any obstacle of the call; after one of the
 * two volume failures, and after CUP3D_ECOMM, the resident chi is UNSPECIFIED (cleared, with some obstacles of the call already entered).
 * nobstacles = 0 is a no-op that clears nothing (13590). */
typedef struct {
  long nblocks;
  const int32_t *slots;  /* as in cup3d_obstacle; distinct within one obstacle, as its ObstacleBlocks are */
  const double *sdf;     /* in  [nblocks][10][10][10]  ObstacleBlock::sdfLab, index [z+1][y+1][x+1] */
  double *udef;          /* in/out [nblocks][8][8][8][3]: kernelRemoveUdefMomenta applied */
  double *chi;           /* out [nblocks][8][8][8] */
  double transvel_correction[3];  /* in/out: read as oldCorrVel (13436), written at 13533-13535 */
  double angvel_correction[3];    /* out 13542-13547 */
  double cm[3], mass, J[6];       /* out: centerOfMass 13421-13423, mass 13532, J 13536-13541 */
  double com_totals[4], udef_totals[13];  /* out: com[] after 13419, M[] after 13519 */
  double *block_com;     /* out, may be NULL [nblocks][4]: mass, CoM_x, CoM_y, CoM_z */
  double *block_momenta; /* out, may be NULL [nblocks][13]: V FX FY FZ TX TY TZ J0..J5 */
  int32_t *first;        /* out [nblocks+1] CSR, blocks in the order listed */
  int32_t *ijk;          /* out [.][3], caller-sized for 512*nblocks points, the first first[nblocks] written */
  double *dchi, *delta;  /* out, same sizing: surface_data::dchidx,y,z ([.][3]) and delta */
} cup3d_obstacle_shape;
CUP3D_API int cup3d_create_obstacles(cup3d_sim_t *, int nobstacles, cup3d_obstacle_shape *shapes);
/* Penalization::preventCollidingObstacles (main.cpp:14009-14324), the collision model Penalization::operator() begins with (14329): call
 * it between cup3d_update_obstacles and cup3d_penalization.  It reads what the last successful cup3d_create_obstacles of this sim KEEPS
 * on the device per obstacle of that call -- slots, geom [n][4], sdfLab [n][10][10][10], chi [n][8][8][8] and the corrected udef
 * [n][8][8][8][3], counted in cup3d_sim_device_bytes, replaced by the next successful call, dropped by a refused or failed one, freed by
 * cup3d_sim_destroy -- so no field is uploaded and 20 doubles per obstacle come back (cup3d_run_stats.field_bytes_downloaded).
 *   The CollisionInfo sums (14037-14142) on the device, one wavefront per obstacle i: for j = 0..N-1, j != i, the blocks both obstacles
 *     hold in ascending slot order whatever order the lists have, cells in z, y, x order, those with iChi <= 0 or jChi <= 0 skipped; iM,
 *     iPos, ivec, jM, jPos, jvec run on across the blocks and across j; iMom / jMom are those of the first cell whose |Mom|^2 beats
 *     imagmax / jmagmax with the strict `>`, the two maxima restart at 0 for every j and iMom / jMom persist when no cell beats 0, as
 *     written.  Bit for bit the reference's loop with one thread.
 *   On the host: buffermax and the MPI_MAX all-reduce (14143-14153), the iok / jok test with its 1e-10 (14154-14182), the MPI_SUM of
 *     20 N (14183), then the pairs i < j in order with one thread (14208-14323) -- the tolerance and 0.2 tests, the push onto
 *     bCollisionID, the normal, projVel <= 0, the contact point, the 1e10 mass of a forced body, ComputeJ and ElasticCollision as written
 *     (13939-14007, the 1e-21 terms included) -- and later pairs see the velocities earlier pairs wrote.
 * COLLECTIVE like cup3d_update_obstacles: every rank calls it with the same nobstacles.  Both all-reduces go in pieces of at most 16
 * values from a device buffer of the call's own; an error flag rides with the first piece: a rank whose own arguments fail returns its
 * own code, the others CUP3D_ECOMM, and every rank returns.
 * CUP3D_EINVAL: a null handle, dt <= 0, nobstacles < 0, null obstacles / ncollided / any with nobstacles > 0.  CUP3D_ESTATE: nothing
 * retained, or nobstacles differs from the retained count.  A refused call writes nothing of the caller's.  nobstacles = 0 is a no-op
 * and nobstacles = 1 finds nothing.  LEFT TO THE HOST: the override of 13069-13077 while collision_counter > 0 (UpdateObstacles). */
typedef struct {
  double cm[3], mass, J[6];      /* centerOfMass, mass, J as cup3d_create_obstacles returned them */
  int forced[3];                 /* bForcedInSimFrame */
  double vel[3], omega[3];       /* in/out: transVel, angVel */
  double collision_vel[3], collision_omega[3], collision_counter; /* in/out: u/v/w_collision, ox/oy/oz_collision, collision_counter;
                                    written only for an obstacle of a resolved pair (14309-14322) */
  double sums[20];               /* out: CollisionInfo after both all-reduces, member order of 14015-14034 */
} cup3d_obstacle_collision;
/* collided: may be NULL, room for nobstacles*(nobstacles-1) ints; *ncollided ints written = sim.bCollisionID (pushed at 14249-14250,
 * i.e. BEFORE the projVel test, as written); *any = whether sim.bCollision was set */
CUP3D_API int cup3d_prevent_colliding_obstacles(cup3d_sim_t *, double dt, int nobstacles, cup3d_obstacle_collision *obstacles,
                                                int32_t *collided, int *ncollided, int *any);
/* The three operators between AdvectionDiffusion and the Poisson solve on the RETAINED set: UpdateObstacles::operator() (13812-13837),
 * Penalization::operator() without the collision model (14330-14340: KernelPenalization 13841-13912 and kernelFinalizePenalizationForce
 * 13913-13938) and kernelUpdateTmpV (14948-14979, 15066-15085).  They compute, bit for bit, what cup3d_update_obstacles,
 * cup3d_penalization and cup3d_update_tmpv compute from the chi and corrected udef that cup3d_create_obstacles returned -- but read them
 * where that call left them on the device (see cup3d_prevent_colliding_obstacles), so no field byte goes up, nothing is allocated per
 * call, and every operator is ONE launch and at most one download whatever the number of obstacles.  Obstacle k of a call is obstacle k of
 * the last successful cup3d_create_obstacles: its blocks in the order listed there, its chi and corrected udef as that call left them.
 *   The plan.  The first of the three to run after a cup3d_create_obstacles builds a plan of the retained set and keeps it with the set
 *     (counted in cup3d_sim_device_bytes from then on, dropped with the set).  Row r = row_base[k] + i stands for block i of obstacle k;
 *     with N obstacles, R rows and S distinct slots the plan holds N * (32 + 72) bytes (the obstacles' four array pointers; cm, vel, omega
 *     of the call), R * (3 * 4 + 29 * 8) bytes (obstacle and block of a row, the slot-major list, the call's block rows) and (S + 1) * 4
 *     bytes (where each slot's rows begin).  A rank with R = 0 holds an empty plan and launches nothing.
 *   cup3d_update_obstacles_resident: KernelIntegrateFluidMomenta, one wavefront per row, cells in the reference's order; one download
 *     of [R][29] doubles (cup3d_run_stats.field_bytes_downloaded); then per obstacle what cup3d_update_obstacles does on the host -- its
 *     own code: rows added in ascending slot order, the all-reduce, the volume check, computeVelocities -- with motion[k].block_sums (may
 *     be NULL) [retained nblocks][29] in the order the obstacle's blocks were listed.  body[k].cm is read, body[k].vel / omega written.
 *   cup3d_penalization_resident: one workgroup per distinct slot walks the obstacles that hold the slot in ascending k and penalises
 *     the slot's cells for each -- a thread keeps its two cells, so obstacle k + 1 sees what obstacle k wrote, the reference's order
 *     (13849-13852); a block's six sums are reduced by the tree of cup3d_penalization.  One download of [R][6] doubles; force / torque as
 *     kernelFinalizePenalizationForce adds them.  body[k].cm / vel / omega are read, force / torque written.
 *   cup3d_update_tmpv_resident: the same schedule, tmpV += udef where chi <= the obstacle's chi, obstacle after obstacle.  No download.
 *     Call after clearing tmpV and before cup3d_pressure_rhs / cup3d_pressure_project, like cup3d_update_tmpv.
 * COLLECTIVE like the calls they stand for (cup3d_update_tmpv_resident is not): every rank calls with the same nobstacles; per obstacle,
 * in obstacle order, two all-reduces of at most 16 values (29 totals and the flag) resp. one of 7 (6 sums and the flag); a rank that
 * holds none of an obstacle's blocks takes part with zeros; a rank that fails -- nothing retained, say -- returns its own code, the
 * others CUP3D_ECOMM, and every rank returns.
 * CUP3D_EINVAL: a null handle, dt <= 0 or NaN, nobstacles < 0, null body / motion with nobstacles > 0, and -- after the all-reduce -- a
 * total volume totals[0] <= DBL_EPSILON as in cup3d_update_obstacles.  CUP3D_ESTATE: no cup3d_create_obstacles has left its blocks on the
 * device, or nobstacles differs from the retained count.  A refused call writes nothing of the caller's and launches nothing; nothing of
 * the caller's is written before every obstacle of the call has passed.  nobstacles = 0 is a no-op. */
typedef struct {
  double cm[3], vel[3], omega[3];  /* in; vel / omega are written by cup3d_update_obstacles_resident */
  double force[3], torque[3];      /* out of cup3d_penalization_resident */
} cup3d_obstacle_body;
CUP3D_API int cup3d_update_obstacles_resident(cup3d_sim_t *, double dt, double lambda, int implicit_penalization, int nobstacles,
                                              cup3d_obstacle_body *bodies, cup3d_obstacle_motion *motion);
CUP3D_API int cup3d_penalization_resident(cup3d_sim_t *, double dt, double lambda, int implicit_penalization, int nobstacles,
                                          cup3d_obstacle_body *bodies);
CUP3D_API int cup3d_update_tmpv_resident(cup3d_sim_t *, int nobstacles);
/* ComputeForces::operator() without Obstacle::computeForces (main.cpp:12496-12503): KernelComputeForces::visit (12273-12493) on the
 * device.  One cup3d_obstacle_surface = the ObstacleBlocks of one Obstacle on this rank that have surface points (nPoints > 0; 12280
 * skips the others) with their surface_data as a CSR list: block i owns points [first[i], first[i+1]), ijk = surface_data::ix, iy, iz,
 * dchi = surface_data::dchidx, dchidy, dchidz.  Per point: the unit normal, the 5-step march along it (12323-12341), one-sided first
 * derivatives of vel with their 6-, 3- and 2-point branches, second and mixed derivatives, the Taylor shift back to the surface cell
 * (12420-12437) and everything from 12438 to 12491, in the reference's association -- including, as written there, the `sx` of the
 * 2-point dveldy branch (12364) and the precedence of the mixed fallback, sx*sy*(a-b) - (c-d) (12394-12395, 12406-12407, 12418-12419).
 * points: the 19 arrays the functor writes, [19][npoints] in the order pX pY pZ P fX fY fZ fxV fyV fzV omegaX omegaY omegaZ vxDef vX
 * vyDef vY vzDef vZ (it never writes fxP / fyP / fzP).  qoi: per block the 19 sums in ObstacleBlock::sumQoI order (7289-7307), points
 * added in order i = 0..nPoints-1 as the reference adds them, bit for bit.  IN/OUT: visit() zeroes eleven of them at entry (12283-12293:
 * forcex, forcex_V, forcex_P, torquex/y/z, thrust, drag, Pout, defPower, pLocom); forcey, forcez, forcey_P, forcez_P, forcey_V, forcez_V,
 * PoutBnd and defPowerBnd go on from the value passed in. */
typedef struct {
  long nblocks;            /* ObstacleBlocks of this obstacle with nPoints > 0 on this rank */
  const int32_t *slots;    /* [nblocks] */
  const int32_t *first;    /* [nblocks+1] */
  const int32_t *ijk;      /* [npoints][3] */
  const double *dchi;      /* [npoints][3] */
  const double *udef;      /* [nblocks][8][8][8][3] */
  double cm[3], vel[3], omega[3];
  double *points;          /* out [19][npoints], order above */
  double *qoi;             /* in/out [nblocks][19], sumQoI order */
} cup3d_obstacle_surface;
/* Obstacles one after another (12270-12271).  Per obstacle the [-4,5) tensorial tiles of vel and chi of `slots` are built by the kernel
 * of cup3d_sim_labs_device into a grow-only scratch buffer of the sim (counted in cup3d_sim_device_bytes; at most 512 blocks' tiles,
 * 64 MiB, at a time: longer lists go through it chunk by chunk), pres is read from the resident field, and points and qoi come back
 * with one download each (counted in cup3d_run_stats.field_bytes_downloaded): 19 doubles per point and per block cross PCIe instead of
 * the 131 072 B per block the tiles would.  vel, chi and pres are only read.  nblocks = 0 and nobstacles = 0 are no-ops.
 * CUP3D_EINVAL, nothing touched: a null array with nblocks > 0, a slot outside [0, nblocks of the sim), first not non-decreasing from 0,
 * an ijk outside [0, 8), a sim on a rank view or on one rank's share of a uniform grid. */
CUP3D_API int cup3d_compute_forces(cup3d_sim_t *, double nu, int nobstacles, cup3d_obstacle_surface *obstacles);
/* The same on a mesh spread over ranks (mesh / owner as for cup3d_sim_labs_over_ranks, whose device variant supplies the tiles).
 * COLLECTIVE: every rank calls it with the same nobstacles; a rank that holds none of an obstacle's blocks passes nblocks = 0.  Every
 * rank makes the same number of tile calls per obstacle -- the largest block count of a rank, read off `owner`, cut into chunks of 4096
 * blocks (a scratch of at most 512 MiB, allocated only as far as the rank's share of the obstacle needs it) -- so an obstacle may list
 * at most as many blocks as the rank holds.  COST: that number does not shrink with the obstacle.  A rank of up to 4096 blocks makes one
 * round, i.e. two calls of cup3d_sim_labs_over_ranks_device, per obstacle; 512^3 on 8 ranks (32 768 blocks per rank) makes 8 rounds, and a
 * round in which no rank asks for a tile still agrees and exchanges an empty request.  It adds no collective of its own: the sum of the 19 values over blocks
 * and ranks stays the host's (Obstacle::computeForces, MPI_Allreduce at 13087).  A rank whose own arguments are refused still takes
 * part in the tile calls, asking for nothing, and then returns CUP3D_EINVAL with nothing touched; the other ranks finish. */
CUP3D_API int cup3d_compute_forces_over_ranks(cup3d_sim_t *, const cup3d_grid_t *mesh, const int32_t *owner, double nu, int nobstacles,
                                              cup3d_obstacle_surface *obstacles);
/* ComputeForces::operator() WITH Obstacle::computeForces (12496-12503, 13079-13115) on the RETAINED set: the last operator of the step
 * (setupOperators, 15244).  It computes, bit for bit, what cup3d_compute_forces computes on the surface list and corrected udef that
 * cup3d_create_obstacles returned, but nothing of that goes up: udef is read where that call left it, and the surface list is rebuilt
 * on the device from the retained sdfLab and chi by the statements that made it (13355-13400).  Obstacle k of a call is obstacle k of
 * the last successful cup3d_create_obstacles.
 *   The surface plan.  The first call after a cup3d_create_obstacles builds it and keeps it with the set (counted in
 *     cup3d_sim_device_bytes from then on, dropped with the set; it builds the plan of the resident operators above too if none of them
 *     has run).  A surface row is a listed block with surface points, in obstacle order and then listed order.  With N obstacles, Rs
 *     surface rows, S distinct slots among them and P points it holds N * 8 bytes (where each obstacle's sdfLab lies), Rs * (5 * 4 + 19 * 8)
 *     + 4 bytes (obstacle, block, tile and slot-major place of a row, where each row's points begin; the blocks' nineteen sums) and
 *     P * (3 * 4 + 3 * 8) bytes (ijk, dchi); S costs nothing on the device -- the slot list and where each slot's rows begin stay on the
 *     host.  A rank with Rs = 0 holds an empty plan and launches nothing.
 *   The nineteen sums of a block (7289-7307) live in the plan: zero when it is built, as ObstacleBlock's members are after create
 *     (7311-7319, 7279-7284); each call restarts eleven and lets eight run on (12283-12293), so the second call after one
 *     cup3d_create_obstacles returns what cup3d_compute_forces returns when handed the first call's qoi.
 *   Tiles.  The [-4,5) tiles of vel and chi are built once per DISTINCT slot per call, 512 slots at a time (4096 over ranks), into the
 *     scratch of cup3d_compute_forces: two tile calls and one launch per chunk, all obstacles together.
 *   Out, per obstacle: points (may be NULL) [19][points of the obstacle on this rank] and qoi (may be NULL) [blocks with points][19], both
 *     in the order of cup3d_compute_forces on shape.surface; totals[19] = the rows added in ascending slot order -- obstacleBlocks is
 *     indexed by blockID, so that is the loop of 13082-13086 -- then summed over the ranks (13087); Pthrust, Pdrag, EffPDef, EffPDefBnd
 *     as 13108-13114 write them from totals and vel.
 *   cup3d_run_stats: field_bytes_uploaded stays 0; field_bytes_downloaded grows by Rs * 19 * 8 (one download of all rows), and by
 *     19 * 8 bytes per point of every obstacle that passes points (one strided copy per such obstacle, straight into its array, once
 *     every obstacle has passed).  If no obstacle passes points they are neither stored nor allocated.
 * cup3d_compute_forces_resident_over_ranks is COLLECTIVE: every rank calls it with the same nobstacles; the tiles come from
 * cup3d_sim_labs_over_ranks_device, in the same number of rounds on every rank PER CALL -- the largest block count of a rank, read off
 * `owner`, in chunks of 4096 -- not per obstacle as in cup3d_compute_forces_over_ranks; then per obstacle, in obstacle order, two
 * all-reduces (19 totals and the flag, at most 16 values each).  A rank whose own arguments fail still takes part in all of them,
 * asking for no tile; it returns its own code, the others CUP3D_ECOMM, and every rank returns.
 * CUP3D_EINVAL: a null handle, nobstacles < 0, a null array with nobstacles > 0, null mesh / owner, the one-rank call on a rank view or
 * on one rank's share of a uniform grid.  CUP3D_ESTATE: no cup3d_create_obstacles has left its blocks on the device, nobstacles differs
 * from the retained count, or a table of the plan fails its bound.  A refused call writes nothing of the caller's and launches nothing;
 * the caller's structs are written only when every obstacle has passed.  nobstacles = 0 is a no-op. */
typedef struct {
  double cm[3], vel[3], omega[3];   /* in */
  double *points;                   /* out, may be NULL: [19][points of obstacle k on this rank], order of cup3d_compute_forces */
  double *qoi;                      /* out, may be NULL: [blocks with points][19], listed order */
  double totals[19];                /* out: surfForce[3] presForce[3] viscForce[3] surfTorque[3] drag thrust Pout PoutBnd defPower defPowerBnd
                                       pLocom (13089-13107) */
  double Pthrust, Pdrag, EffPDef, EffPDefBnd;   /* out, 13108-13114 */
} cup3d_obstacle_forces;
CUP3D_API int cup3d_compute_forces_resident(cup3d_sim_t *, double nu, int nobstacles, cup3d_obstacle_forces *obstacles);
CUP3D_API int cup3d_compute_forces_resident_over_ranks(cup3d_sim_t *, const cup3d_grid_t *mesh, const int32_t *owner, double nu, int nobstacles,
                                                       cup3d_obstacle_forces *obstacles);
/* Implicit diffusion: AdvectionDiffusionImplicit (main.cpp:7148-7157, 10030-10119), selected by -implicitDiffusion (15231-15232).
 * One call = euler(dt): KernelAdvect, the explicit-diffusion guess, KernelDiffusionRHS and one DiffusionSolver::solve per velocity
 * component.  `params`: tol / tol_rel = sim.DiffusionErrorTol / DiffusionErrorTolRel (15369-15370), max_iter; mean_constraint,
 * max_restarts and block_solver are ignored (DiffusionSolver has no mean constraint, no restart cap and its own block CG; how that
 * block preconditioner is evaluated is a setting of the sim, cup3d_diffusion_set_block_solver below).
 * results[3] (may be NULL): per-component solver statistics.  pres is used as scratch and restored; tmpV and lhs are clobbered.
 * KernelAdvect (9849-10029) updates vel IN PLACE in the reference while other blocks still build their ghosted tiles from it, so
 * the reference's own result depends on block order and thread timing; this implementation reads every tile from the velocity
 * on entry (the order-independent reading).  Everything else is the reference's arithmetic. */
CUP3D_API int cup3d_advect_diffuse_implicit(cup3d_sim_t *, double dt, double nu, const double uinf[3], const cup3d_poisson_params *params,
                                  cup3d_poisson_result results[3]);
/* its parts, for tests and for callers that interleave their own operators:
 * compute<VectorLab>(KernelAdvect(sim, dt), vel, tmpV) (10038): tmpV <- facD*lap(vel), vel <- vel + facA*(u.grad)u/h^3 */
CUP3D_API int cup3d_advect_implicit(cup3d_sim_t *, double dt, double nu, const double uinf[3]);
/* compute<VectorLab>(KernelDiffusionRHS(sim), vel, tmpV) (10057, 9729-9848): tmpV <- h*lap(vel) */
CUP3D_API int cup3d_diffusion_rhs(cup3d_sim_t *);
/* DiffusionSolver::_lhs (6836-6875) with mydirection = direction: lhs <- h*(sum6 - 6 pres) - h^3/(dt nu)*pres on the
 * BlockLabBC<ScalarGrid, .., direction> tile (wall: ghost = -face cell; freespace: negated behind the faces normal to direction) */
CUP3D_API int cup3d_diffusion_lhs(cup3d_sim_t *, int direction, double dt, double nu);
/* diffusion_kernels::getZImplParallel (10534-10579): pres <- block-local CG solve with centre coefficient -6 - h^2/nu/dt, in place */
CUP3D_API int cup3d_diffusion_preconditioner(cup3d_sim_t *, double dt, double nu);
/* how DiffusionSolver's block preconditioner (diffusion_kernels::getZImplParallel, main.cpp:10534-10579) is evaluated by
   cup3d_diffusion_preconditioner, cup3d_diffusion_solve and cup3d_advect_diffuse_implicit on this sim:
   0 = the reference's block CG (default; association as today), 1 = direct solve by fast diagonalisation (exact to rounding). */
CUP3D_API int cup3d_diffusion_set_block_solver(cup3d_sim_t *, int block_solver);
/* DiffusionSolver::solve (6896-7146): right-hand side in lhs (clobbered), initial guess and result in pres */
CUP3D_API int cup3d_diffusion_solve(cup3d_sim_t *, int direction, double dt, double nu, const cup3d_poisson_params *params, cup3d_poisson_result *result);
/* ComputeVorticity::operator() (8726-8746, KernelVorticity 8624-8645): tmpV <- curl(vel); any mesh */
CUP3D_API int cup3d_compute_vorticity(cup3d_sim_t *);

/* ComputeDissipation::operator() (main.cpp:10436-10447; KernelDissipation 10347-10434): the 20 integrals RDX[0..19] of vel, pres, chi;
 * any mesh, one rank or a share / rank view (then incl. the SUM all-reduce of 10443).  block_sums: NULL or [nblocks][20], this rank's per-block sums.
 * In the reference's order: vorticity integral x3, linear impulse x3, momentum x3, angular impulse x3, angular momentum x3 (about
 * extents/2), pressure power, viscous power, helicity, kinetic energy, integral of |omega|.  The reference computes and drops them.
 * Every summand is the reference's expression (hCube = pow(h, 3)); the sums are ordered: a block adds its cells in iz, iy, ix order onto
 * 0.0, a rank its blocks in slot order onto 0.0, the ranks by the all-reduce -- the reference's one-thread result on a one-block grid.
 * chi is read as it stands (zero unless written).  The first call of this or of cup3d_fix_mass_flux allocates (nblocks * 24 + 20) doubles. */
CUP3D_API int cup3d_compute_dissipation(cup3d_sim_t *, double nu, const double extents[3], double qoi[20], double *block_sums);
/* FixMassFlux::operator() (main.cpp:12199-12248): the mean of u + uinf[0] over the volume (avgUx_nonUniform 12199-12216, divided by the
 * volume before the SUM all-reduce of 12224; same ordered sums as above, h*h*h here), then vel.u[0] += 6 * scale * y/H * (1 - y/H) in
 * place, scale = 6 * (2/3 umax_forced - mean), H = extents[1].  Nothing is printed: *out (may be NULL) receives the numbers. */
typedef struct { double u_avg_msr, u_avg, delta_u, scale, re_tau; } cup3d_mass_flux;   /* the five numbers of the printf at 12229-12234 */
CUP3D_API int cup3d_fix_mass_flux(cup3d_sim_t *, double umax_forced, double nu, double dt, const double extents[3], const double uinf[3], cup3d_mass_flux *out);

/* compute<ScalarLab>(GradChiOnTmp(sim), sim.chi) (main.cpp:15182, 8540-8600): tmpV (the vorticity left by cup3d_compute_vorticity) edited
 * from the resident chi on its tensorial [-2,3) tile -- blocks with an obstacle surface within reach are flagged (1e10), cells deep
 * inside a body cleared, vorticity capped on level levelMaxVorticity - 1.  With cup3d_compute_vorticity before and cup3d_tag_blocks
 * after, this is the decision input of Simulation::adaptMesh (15180-15183) for runs with obstacles.  One rank. */
CUP3D_API int cup3d_grad_chi_on_tmp(cup3d_sim_t *, double Rtol, double Ctol, int level_max_vorticity);
/* ... on a mesh spread over ranks (collective; mesh / owner as for cup3d_adapt_migrate): the chi blocks behind edges, corners and finer
 * neighbours that other ranks own arrive first, by the plan of the rank's tensorial view (SynchronizerMPI_AMR with a tensorial stencil) */
CUP3D_API int cup3d_grad_chi_on_tmp_over_ranks(cup3d_sim_t *, const cup3d_grid_t *mesh, const int32_t *owner, double Rtol, double Ctol, int level_max_vorticity);

/* per-kernel device time accounting (hipEvents on the compute stream) */
CUP3D_API int cup3d_profile_enable(int on);
CUP3D_API int cup3d_profile_reset(void);
/* fills up to max entries; returns the number of distinct kernels in *n */
typedef struct { char name[48]; long launches; double total_ms; } cup3d_profile_entry;
/* run statistics since the last reset, this process: what the rank handed to RCCL (the payload of the reference's MPI_Isend at
 * main.cpp:2402 and of its MPI_(I)allreduce sites) and how long the host thread sat waiting for device results (the reference's
 * MPI_Waitall / MPI_Wait, 2324, 14490, 14550) */
typedef struct {
  long halo_exchanges;      /* face-slab / ghost-block / face-flux exchanges started */
  double halo_bytes_sent;   /* bytes of those this rank sent */
  long allreduces;          /* scalar all-reduces issued */
  long host_waits;          /* times the host waited for scalars of the device */
  double host_wait_seconds; /* ... and for how long in total */
  long solver_iterations;   /* BiCGSTAB iterations (Poisson and Helmholtz solves) */
  double field_bytes_uploaded;   /* field data that crossed the host boundary (cup3d_sim_upload*, PCIe host -> device) ... */
  double field_bytes_downloaded; /* ... and back (cup3d_sim_download*): what the drop-in adds to a step of the host's time loop */
} cup3d_run_stats;
CUP3D_API int cup3d_stats_reset(void);
CUP3D_API int cup3d_stats_read(cup3d_run_stats *);
CUP3D_API int cup3d_profile_read(cup3d_profile_entry *entries, int max, int *n);
/* VERIFICATION SUPPORT: the bits of the Poisson path under any sharding of the blocks (bench.py's config.checksum at every N).
 * Fills PoissonSolverAMR's 18 work vectors (main.cpp:14382-14399) with a function of (vector, level, global cell index) only, sets
 * alpha, beta, omega (and the mean-constraint total) BY HAND and runs the kernels of ONE BiCGSTAB iteration exactly as
 * cup3d_poisson_solve launches them -- t = A what (14549), loop 1 (14453-14464), zhat = M^-1 z (14488, getZImplParallel 14704-14745),
 * v = A zhat (14489), loop 2 (14502-14515), what = M^-1 w (14548): the fused kernels, the width-1 scalar halo exchanges, the
 * inner / boundary split -- with no dot product feeding back.  The stencil and the block-local solve do not see the partition, so
 * sums[18] (wrapping 64-bit sums of each vector's bit patterns over the rank's blocks, vector order of poisson.hip), added over the
 * ranks mod 2^64, are the same at every N.  block_solver 0, 1 or 2 (the solvers with fused kernels); clobbers the work vectors only. */
CUP3D_API int cup3d_poisson_path_checksum(cup3d_sim_t *, int block_solver, int mean_constraint, unsigned long long *sums18);
/* CG iterations of the last block-CG launch made while cup3d_profile_enable(1) was on, summed over the rank's blocks (the flop count
 * behind bench.py's FP64 roofline of the block preconditioner, getZImplParallel main.cpp:14704-14745) */
CUP3D_API int cup3d_profile_block_cg_iterations(cup3d_sim_t *, long *total, long *nblocks);

#ifdef __cplusplus
}
#endif
#endif
