// cup3d_hip_operators.h — C++ host side of the drop-in: the reference's plugin surface
// (class Operator, main.cpp:6678-6684; class PoissonSolverBase, 8921-8928) implemented on
// top of the C ABI of include/cup3d_hip.h.
//
// Include this header in a translation unit AFTER the reference's declarations (e.g. after
// `#include "main.cpp"` with `main` renamed).  Nothing in main.cpp is
// modified: cup3d_hip::install(simulation) swaps the AdvectionDiffusion and
// PressureProjection entries of sim.pipeline (built by Simulation::setupOperators,
// 15229-15246) and sim.pressureSolver for the HIP-backed ones below.
//
// Data ownership stays with the reference: the five GridMPI objects own the block memory
// (one posix_memalign per block, 877-884).  Each operator uploads the blocks it reads
// (Info::block pointers, m_vInfo order), runs on the GPU and downloads what the reference
// would have written, so every CPU-side operator in between (obstacles, penalisation,
// mesh adaptation, dump) keeps working unchanged.  The device mirror is rebuilt whenever
// the block list changes.  Errors follow the reference's convention: print and MPI_Abort.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../include/cup3d_hip.h"
#ifdef CUP3D_HIP_SHIM_TEST_TRANSPORT  // test builds only (oracle/Makefile: ref_tool_hip_mpi_testing, linked against libcup3d_hip_testing.so)
#include "../../include/cup3d_hip_testing.h"
#endif

namespace cup3d_hip {

#ifdef CUP3D_HIP_SHIM_TEST_TRANSPORT
// The library's exchanges carried by the host's own MPI through host memory instead of RCCL (cup3d_debug_host_transport): RCCL
// refuses two ranks on one device, so this is how the multi-rank branch below runs as real MPI processes on a one-GPU box.
// Selected at run time with CUP3D_HIP_HOST_TRANSPORT=1; a production build of the shim does not contain it.
struct HostTransport {
  MPI_Comm comm;
  static int exchange(void *ctx, const void *sb, const long *so, const long *sn, void *rb, const long *ro, const long *rn) {
    MPI_Comm c = static_cast<HostTransport *>(ctx)->comm;
    int size = 1;
    MPI_Comm_size(c, &size);
    std::vector<MPI_Request> rq;
    for (int p = 0; p < size; ++p)
      if (rn[p]) { rq.emplace_back(); MPI_Irecv((char *)rb + ro[p], (int)rn[p], MPI_BYTE, p, 4711, c, &rq.back()); }
    for (int p = 0; p < size; ++p)
      if (sn[p]) { rq.emplace_back(); MPI_Isend((const char *)sb + so[p], (int)sn[p], MPI_BYTE, p, 4711, c, &rq.back()); }
    return MPI_Waitall((int)rq.size(), rq.data(), MPI_STATUSES_IGNORE) == MPI_SUCCESS ? 0 : 1;
  }
  static int allreduce(void *ctx, double *buf, int n, int is_max) {
    MPI_Comm c = static_cast<HostTransport *>(ctx)->comm;
    return MPI_Allreduce(MPI_IN_PLACE, buf, n, MPI_DOUBLE, is_max ? MPI_MAX : MPI_SUM, c) == MPI_SUCCESS ? 0 : 1;
  }
};
#endif

inline void die(const char *what, int rc) {
  fprintf(stderr, "cup3d_hip: %s failed (%d): %s\n", what, rc, cup3d_last_error());
  fflush(0);
  MPI_Abort(MPI_COMM_WORLD, 1);
}
#define CUP3D_HIP_CALL(x)                       \
  do {                                          \
    const int rc_ = (x);                        \
    if (rc_ != CUP3D_OK) ::cup3d_hip::die(#x, rc_); \
  } while (0)

// Device mirror of one SimulationData: topology + the five fields.
class DeviceMirror {
public:
  explicit DeviceMirror(SimulationData &s) : sim(s) {}
  ~DeviceMirror() { release(); }
  DeviceMirror(const DeviceMirror &) = delete;

  cup3d_sim_t *handle() {
    ensure();
    return dsim;
  }
  // resident mode (install(sim, true) / CUP3D_HIP_RESIDENT=1): between AdvectionDiffusionHIP and PressureProjectionHIP the
  // velocity stays in HBM (no download / upload), see install()
  bool resident = false;      // allowed at all: decided by install() from the pipeline
  bool vel_on_device = false; // the device copy of vel is newer than the host's
  // resident ACROSS steps (install(sim, 2) / CUP3D_HIP_RESIDENT=2): after PressureProjectionHIP the host holds a copy of the
  // device's vel and pres; as long as nobody but the intercepted operators writes those two fields on the host, the next step need
  // not send them up again (3.2 + 1.1 GB per step at 512^3).  That "as long as" is a CONTRACT with the host code: the reference's own
  // step writes vel / pres only inside the operators this header replaces or wraps and in adaptMesh (which changes the block list:
  // ensure() notices and drops the flags); any other writer -- an initial condition, a restart, a test harness loading a field --
  // must call invalidate().  Off by default for that reason.
  bool across_steps = false;
  bool host_vel_clean = false, host_pres_clean = false;  // host copy == device copy
  // DEVICE-LED (install(sim, 3) / CUP3D_HIP_RESIDENT=3): vel and pres live in HBM from one step to the next and the host copy is only
  // refreshed on demand (sync_host(): before adaptMesh, a dump, or anything else on the host that reads them).  Needs the ONE edit of
  // the reference this shim cannot make from outside: Simulation::calcMaxTimestep (15254-15305) reads the host velocity through
  // findMaxU (15259) every step, so the time loop must call cup3d_hip::calcMaxTimestep(simulation, mirror) instead -- the same
  // function with the maximum taken on the device.  Obstacle-free pipelines only: ComputeForces reads the
  // host fields every step (12250-12495), so with obstacles the mode falls back to `across_steps`.
  bool device_led = false;
  bool dev_current = false;  // the device copies of vel and pres are newer than the host's
  long chi_uploaded_step = -1;  // sim.step at which PressureProjectionHIP last sent chi up (ComputeForcesHIP reads it on the device)
  void invalidate() { host_vel_clean = host_pres_clean = false; dev_current = false; chi_uploaded_step = -1; }
  void sync_host() {
    if (!dev_current) return;
    download(CUP3D_FIELD_VEL);
    download(CUP3D_FIELD_PRES);
    dev_current = false;
    host_vel_clean = host_pres_clean = true;
  }
  void upload(int field) {
    ensure();
    const std::vector<Info> &I = infos(field);
    ptrs.resize(I.size());
    for (size_t i = 0; i < I.size(); ++i) ptrs[i] = I[i].block;
    CUP3D_HIP_CALL(cup3d_sim_upload_blocks(dsim, field, (const void *const *)ptrs.data()));
  }
  void download(int field) {
    const std::vector<Info> &I = infos(field);
    ptrs.resize(I.size());
    for (size_t i = 0; i < I.size(); ++i) ptrs[i] = I[i].block;
    CUP3D_HIP_CALL(cup3d_sim_download_blocks(dsim, field, (void *const *)ptrs.data()));
  }
  // Partial transfers of the blocks an obstacle covers (non-null ObstacleBlock of any obstacle): the host-side obstacle operators
  // between AdvectionDiffusion and PressureProjection read and write the velocity in exactly those blocks
  // (KernelIntegrateFluidMomenta 13637-13641, KernelPenalization 13853-13861), so in resident mode only they cross PCIe.
  void download_obstacle_blocks(int field) {
    obstacle_blocks(field);
    CUP3D_HIP_CALL(cup3d_sim_download_block_list(dsim, field, (long)oslots.size(), oslots.data(), (void *const *)ptrs.data()));
  }
  void upload_obstacle_blocks(int field) {
    obstacle_blocks(field);
    CUP3D_HIP_CALL(cup3d_sim_upload_block_list(dsim, field, (long)oslots.size(), oslots.data(), (const void *const *)ptrs.data()));
  }

  // The global mesh object and the rank of every leaf, for the entry points that take them (cup3d_compute_forces_over_ranks).  Only a
  // mirror with keep_global_mesh set (install() with CUP3D_HIP_FORCES=1) holds on to what ensure() gathered for the rank view; every
  // other mirror frees it there, as before, and gathers it here on first use -- as does a uniform grid still in GridMPI's initial
  // partition, for which ensure() gathers nothing.  COLLECTIVE when it gathers: every rank must ask.
  bool keep_global_mesh = false;
  void global_mesh(const cup3d_grid_t **mesh, const int32_t **owner) {
    ensure();
    if (!gmesh) gather_mesh();
    *mesh = gmesh;
    *owner = gowner.data();
  }

private:
  SimulationData &sim;
  cup3d_grid_t *grid = nullptr;
  cup3d_grid_t *gmesh = nullptr;
  std::vector<int32_t> gowner;
  cup3d_sim_t *dsim = nullptr;
  std::vector<long long> signature;  // (level, Z) of every local block the mirror was built for
  std::vector<void *> ptrs;
  std::vector<int32_t> oslots;
  bool device_ready = false;

  void obstacle_blocks(int field) {
    ensure();
    const std::vector<Info> &I = infos(field);
    oslots.clear();
    ptrs.clear();
    for (size_t i = 0; i < I.size(); ++i)
      for (const auto &ob : sim.obstacle_vector->getObstacleVector())
        if (ob->getObstacleBlocks()[I[i].blockID] != nullptr) {
          oslots.push_back((int32_t)i);
          ptrs.push_back(I[i].block);
          break;
        }
  }

  const std::vector<Info> &infos(int field) {
    switch (field) {
      case CUP3D_FIELD_CHI: return sim.chiInfo();
      case CUP3D_FIELD_PRES: return sim.presInfo();
      case CUP3D_FIELD_VEL: return sim.velInfo();
      case CUP3D_FIELD_TMPV: return sim.tmpVInfo();
      default: return sim.lhsInfo();
    }
  }
  void release() {
    if (dsim) cup3d_sim_destroy(dsim);
    if (grid) cup3d_grid_destroy(grid);
    if (gmesh) cup3d_grid_destroy(gmesh);
    dsim = nullptr;
    grid = nullptr;
    gmesh = nullptr;
    gowner.clear();
  }
  // every rank assembles the global leaf list with its owners -- the information the reference keeps in Grid::Octree on every rank
  // (815-855) -- as a mesh object (gmesh) and the owner of each of its leaves (gowner)
  void gather_mesh() {
    const std::vector<Info> &I = sim.velInfo();
    int rank = 0, size = 1;
    MPI_Comm_rank(sim.comm, &rank);
    MPI_Comm_size(sim.comm, &size);
    const int bpd[3] = {sim.bpdx, sim.bpdy, sim.bpdz};
    const int bc[3] = {(int)sim.BCx_flag, (int)sim.BCy_flag, (int)sim.BCz_flag};
    int nloc = (int)I.size();
    std::vector<int> counts(size), displs(size);
    MPI_Allgather(&nloc, 1, MPI_INT, counts.data(), 1, MPI_INT, sim.comm);
    long total = 0;
    for (int r = 0; r < size; ++r) { displs[r] = (int)(2 * total); total += counts[r]; counts[r] *= 2; }
    std::vector<long long> mine(2 * (size_t)nloc), all(2 * (size_t)total);
    for (int i = 0; i < nloc; ++i) { mine[2 * i] = I[i].level; mine[2 * i + 1] = I[i].Z; }
    MPI_Allgatherv(mine.data(), 2 * nloc, MPI_LONG_LONG, all.data(), counts.data(), displs.data(), MPI_LONG_LONG, sim.comm);
    std::vector<int32_t> lv((size_t)total), own_in((size_t)total);
    std::vector<int64_t> zs((size_t)total);
    for (int r = 0, k = 0; r < size; ++r)
      for (int i = 0; i < counts[r] / 2; ++i, ++k) { lv[k] = (int32_t)all[2 * k]; zs[k] = all[2 * k + 1]; own_in[k] = r; }
    CUP3D_HIP_CALL(cup3d_grid_create_mesh(bpd, sim.levelMax, sim.maxextent, bc, total, lv.data(), zs.data(), &gmesh));
    // the mesh object orders the leaves by blockID_2: owners follow through (level, Z)
    std::vector<long long> tab(6 * (size_t)total);
    std::vector<double> geom(4 * (size_t)total);
    CUP3D_HIP_CALL(cup3d_grid_tables(gmesh, tab.data(), geom.data()));
    std::map<std::pair<long long, long long>, int32_t> owner_of;
    for (long k = 0; k < total; ++k) owner_of[{lv[k], zs[k]}] = own_in[k];
    gowner.resize((size_t)total);
    for (long k = 0; k < total; ++k) gowner[k] = owner_of[{tab[6 * k], tab[6 * k + 1]}];
  }
  void ensure() {
    const std::vector<Info> &I = sim.velInfo();
    bool same = dsim != nullptr && signature.size() == 2 * I.size();
    for (size_t i = 0; same && i < I.size(); ++i) same = signature[2 * i] == I[i].level && signature[2 * i + 1] == I[i].Z;
    if (same) return;
    release();
    invalidate();  // a new block list: nothing of the old mirror is current
    int rank = 0, size = 1;
    MPI_Comm_rank(sim.comm, &rank);
    MPI_Comm_size(sim.comm, &size);
    if (!device_ready) {
      int ndev = 0;
      CUP3D_HIP_CALL(cup3d_device_count(&ndev));
      CUP3D_HIP_CALL(cup3d_device_init(ndev > 0 ? rank % ndev : 0));  // one process per GPU
#ifdef CUP3D_HIP_SHIM_TEST_TRANSPORT
      if (size > 1 && getenv("CUP3D_HIP_HOST_TRANSPORT")) {
        static HostTransport ht;
        ht.comm = sim.comm;
        const cup3d_host_transport t = {&ht, &HostTransport::exchange, &HostTransport::allreduce};
        CUP3D_HIP_CALL(cup3d_debug_host_transport(rank, size, &t));
      } else
#endif
      if (size > 1) {  // bootstrap the library's RCCL communicator over the host MPI
        unsigned char id[128] = {0};
        if (rank == 0) CUP3D_HIP_CALL(cup3d_comm_unique_id(id));
        MPI_Bcast(id, 128, MPI_BYTE, 0, sim.comm);
        CUP3D_HIP_CALL(cup3d_comm_init(rank, size, id));
      }
      device_ready = true;
    }
    const int level = I.empty() ? sim.levelStart : I[0].level;
    const int bpd[3] = {sim.bpdx, sim.bpdy, sim.bpdz};
    const int bc[3] = {(int)sim.BCx_flag, (int)sim.BCy_flag, (int)sim.BCz_flag};  // enum BCflag == CUP3D_BC_*
    // the device topology must be the reference's own: same blocks, same order, same h
    auto matches = [&](cup3d_grid_t *g) {
      const long nb = cup3d_grid_nblocks(g);
      if ((size_t)nb != I.size()) return false;
      std::vector<long long> tab(6 * (size_t)nb);
      std::vector<double> geom(4 * (size_t)nb);
      CUP3D_HIP_CALL(cup3d_grid_tables(g, tab.data(), geom.data()));
      for (long i = 0; i < nb; ++i)
        if (!(tab[6 * i] == I[i].level && tab[6 * i + 1] == I[i].Z && tab[6 * i + 5] == I[i].blockID_2 && geom[4 * i] == I[i].h)) return false;
      return true;
    };
    // (1) one level, every rank still owning its contiguous Hilbert range (GridMPI's initial partition, 2970-2986): face-slab halos
    int not_uniform = 0;
    for (const Info &b : I) not_uniform |= b.level != level;
    if (!not_uniform) {
      CUP3D_HIP_CALL(cup3d_grid_create_uniform(bpd, sim.levelMax, level, sim.maxextent, bc, rank, size, &grid));
      if (!matches(grid)) { not_uniform = 1; cup3d_grid_destroy(grid); grid = nullptr; }
    }
    if (size > 1) {  // the choice of transport is collective
      int any = 0;
      MPI_Allreduce(&not_uniform, &any, 1, MPI_INT, MPI_MAX, sim.comm);
      if (any && grid) { cup3d_grid_destroy(grid); grid = nullptr; }
      not_uniform = any;
    }
    if (not_uniform && size == 1) {
      // (2) multi-level mesh after MeshAdaptation on one rank: the leaves of m_vInfo; coarse/fine ghosts and flux correction run on
      // the device (amr.hip)
      std::vector<int32_t> lv(I.size());
      std::vector<int64_t> zs(I.size());
      for (size_t i = 0; i < I.size(); ++i) { lv[i] = I[i].level; zs[i] = I[i].Z; }
      CUP3D_HIP_CALL(cup3d_grid_create_mesh(bpd, sim.levelMax, sim.maxextent, bc, (long)I.size(), lv.data(), zs.data(), &grid));
    } else if (not_uniform) {
      // (3) multi-level mesh (or a one-level mesh the LoadBalancer has re-dealt) spread over ranks: every rank assembles the global
      // leaf list with its owners (gather_mesh) and takes its view of it: ghost blocks + the two exchange plans (whole ghost blocks
      // before a stencil kernel, face fluxes after a corrected one;
      // what SynchronizerMPI_AMR::_Setup 1979-2286 and FluxCorrectionMPI::prepare 2680-2824 derive from the octree)
      gather_mesh();
      CUP3D_HIP_CALL(cup3d_grid_rank_view(gmesh, gowner.data(), rank, size, &grid));
      if (!keep_global_mesh) {  // nobody will ask for them: one int32 per leaf of the whole mesh and the mesh object go back
        cup3d_grid_destroy(gmesh);
        gmesh = nullptr;
        std::vector<int32_t>().swap(gowner);
      }
    }
    if (!matches(grid)) {
      fprintf(stderr, "cup3d_hip: device topology differs from the host grid (blocks %ld vs %zu)\n", cup3d_grid_nblocks(grid), I.size());
      fflush(0);
      MPI_Abort(sim.comm, 1);
    }
    CUP3D_HIP_CALL(cup3d_sim_create(grid, &dsim));
    // the block solve of the implicit diffusion's Helmholtz solves: 0 block CG (default), 1 direct; a setting of the sim, so every rebuild sets it
    if (const char *e = getenv("CUP3D_HIP_DIFFUSION_BLOCK_SOLVER")) CUP3D_HIP_CALL(cup3d_diffusion_set_block_solver(dsim, atoi(e)));
    signature.resize(2 * I.size());
    for (size_t i = 0; i < I.size(); ++i) {
      signature[2 * i] = I[i].level;
      signature[2 * i + 1] = I[i].Z;
    }
  }
};

inline cup3d_poisson_params poisson_params(const SimulationData &sim) {
  cup3d_poisson_params p;
  cup3d_poisson_default_params(&p);
  p.tol = sim.PoissonErrorTol;
  p.tol_rel = sim.PoissonErrorTolRel;
  p.mean_constraint = sim.bMeanConstraint;
  if (const char *e = getenv("CUP3D_HIP_BLOCK_SOLVER")) p.block_solver = atoi(e);  // 0 block CG (default), 1 direct
  return p;
}

// AdvectionDiffusion::operator()(dt), main.cpp:9640-9728
class AdvectionDiffusionHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  DeviceMirror &dev;

public:
  AdvectionDiffusionHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d) : Operator(s), devp(d), dev(*d) {}
  void operator()(const Real dt) override {
    (void)dt;  // KernelAdvectDiffuse reads sim.dt (9465), which advance() passes as dt
    dev.handle();  // (re)builds the mirror when the block list changed, which drops the clean flags
    if (!(dev.dev_current || (dev.across_steps && dev.host_vel_clean))) dev.upload(CUP3D_FIELD_VEL);
    dev.host_vel_clean = false;  // the device is about to move on
    const double uinf[3] = {sim.uinf[0], sim.uinf[1], sim.uinf[2]};
    CUP3D_HIP_CALL(cup3d_advect_diffuse(dev.handle(), sim.dt, sim.nu, uinf));
    if (dev.resident) {
      // nobody on the host reads vel / tmpV before the projection except the obstacle operators, which get the blocks they touch
      // from UpdateObstaclesHIP (install() checked the pipeline)
      dev.vel_on_device = true;
      return;
    }
    dev.download(CUP3D_FIELD_VEL);
    dev.download(CUP3D_FIELD_TMPV);
  }
};

// AdvectionDiffusionImplicit::operator()(dt), main.cpp:10030-10119 (-implicitDiffusion 1): one upwind-advection kernel, one
// 7-point kernel and three Helmholtz solves (DiffusionSolver) on the device.  sim.pres is only scratch there and is restored
// (10108-10117), so the host copy is simply left alone.  The reference's KernelAdvect updates vel in place while other blocks
// still read it; the device reads every tile from the velocity on entry (include/cup3d_hip.h), so on more than one block the two
// agree to O(dt) of the advective increment, not to round-off.
class AdvectionDiffusionImplicitHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  DeviceMirror &dev;

public:
  cup3d_poisson_result last[3];
  AdvectionDiffusionImplicitHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d) : Operator(s), devp(d), dev(*d) {}
  void operator()(const Real dt) override {
    (void)dt;  // euler(sim.dt), 10119
    dev.handle();
    if (!(dev.across_steps && dev.host_vel_clean)) dev.upload(CUP3D_FIELD_VEL);
    dev.host_vel_clean = false;
    const double uinf[3] = {sim.uinf[0], sim.uinf[1], sim.uinf[2]};
    cup3d_poisson_params p;
    cup3d_poisson_default_params(&p);
    p.tol = sim.DiffusionErrorTol;
    p.tol_rel = sim.DiffusionErrorTolRel;
    CUP3D_HIP_CALL(cup3d_advect_diffuse_implicit(dev.handle(), sim.dt, sim.nu, uinf, &p, last));
    if (dev.resident) {
      dev.vel_on_device = true;
      return;
    }
    dev.download(CUP3D_FIELD_VEL);
    dev.download(CUP3D_FIELD_TMPV);
  }
};

// ExternalForcing::operator()(dt), main.cpp:10581-10596: on the device while the velocity is resident there, else the
// reference's own operator
class ExternalForcingHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  std::shared_ptr<Operator> cpu;

public:
  ExternalForcingHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d, std::shared_ptr<Operator> original) : Operator(s), devp(d), cpu(original) {}
  void operator()(const Real dt) override {
    if (!devp->vel_on_device) { (*cpu)(dt); return; }
    const int dir = sim.BCy_flag == wall ? 1 : 2;  // 10582-10583
    CUP3D_HIP_CALL(cup3d_external_forcing(devp->handle(), sim.uMax_forced, sim.nu, sim.extents[dir], dt));
  }
};

// FixMassFlux::operator()(dt), main.cpp:12218-12248 (-bFixMassFlux 1): on the device while the velocity is resident there -- the mean of
// u + uinf[0] and the parabolic correction of vel.u[0], cup3d_fix_mass_flux -- else the reference's own operator.  The library prints
// nothing: the reference's five lines (12229-12234) are printed here, on rank 0, from the numbers it returns.
// Installed only with CUP3D_HIP_MASSFLUX=1 (install()).
class FixMassFluxHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  std::shared_ptr<Operator> cpu;

public:
  cup3d_mass_flux last;
  FixMassFluxHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d, std::shared_ptr<Operator> original) : Operator(s), devp(d), cpu(original), last() {}
  void operator()(const Real dt) override {
    if (!devp->vel_on_device) { (*cpu)(dt); return; }
    const double extents[3] = {sim.extents[0], sim.extents[1], sim.extents[2]}, uinf[3] = {sim.uinf[0], sim.uinf[1], sim.uinf[2]};
    CUP3D_HIP_CALL(cup3d_fix_mass_flux(devp->handle(), sim.uMax_forced, sim.nu, sim.dt, extents, uinf, &last));  // reTau reads sim.dt, 12226
    if (sim.rank == 0) {
      printf("Measured <Ux>_V = %25.16e,\n"
             "target   <Ux>_V = %25.16e,\n"
             "delta    <Ux>_V = %25.16e,\n"
             "scale           = %25.16e,\n"
             "Re_tau          = %25.16e,\n",
             last.u_avg_msr, last.u_avg, last.delta_u, last.scale, last.re_tau);
    }
  }
};

// UpdateObstacles::operator()(dt), main.cpp:13812-13837, is the first host operator after the advection step that reads the
// velocity -- in the blocks an obstacle covers only.  While the velocity is resident on the device this wrapper fetches exactly
// those blocks, then runs the reference's own operator; Penalization (next in the pipeline) updates the same blocks on the host and
// PressureProjectionHIP sends them back.
class UpdateObstaclesHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  std::shared_ptr<Operator> cpu;

public:
  UpdateObstaclesHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d, std::shared_ptr<Operator> original) : Operator(s), devp(d), cpu(original) {}
  void operator()(const Real dt) override {
    if (devp->vel_on_device && sim.obstacle_vector->nObstacles() > 0) devp->download_obstacle_blocks(CUP3D_FIELD_VEL);
    (*cpu)(dt);
  }
};

// PoissonSolverBase::solve(), main.cpp:8921-8928 (contract of PoissonSolverAMR::solve, 14363-14616:
// RHS in sim.lhs, initial guess and result in sim.pres)
class PoissonSolverHIP : public PoissonSolverBase {
  SimulationData &sim;
  std::shared_ptr<DeviceMirror> devp;
  DeviceMirror &dev;

public:
  cup3d_poisson_result last{};
  PoissonSolverHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d) : sim(s), devp(d), dev(*d) {}
  void solve() override {
    dev.upload(CUP3D_FIELD_LHS);
    dev.upload(CUP3D_FIELD_PRES);
    const cup3d_poisson_params p = poisson_params(sim);
    CUP3D_HIP_CALL(cup3d_poisson_solve(dev.handle(), &p, &last));
    dev.download(CUP3D_FIELD_PRES);
    dev.host_pres_clean = true;
  }
};

// PressureProjection::operator()(dt), main.cpp:15061-15160
class PressureProjectionHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  DeviceMirror &dev;
  std::shared_ptr<PoissonSolverHIP> solver;
  bool had_obstacles = false;

public:
  cup3d_poisson_result last{};
  PressureProjectionHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d)
      : Operator(s), devp(d), dev(*d), solver(std::make_shared<PoissonSolverHIP>(s, d)) {
    sim.pressureSolver = solver;  // as at main.cpp:15058-15059
  }
  void operator()(const Real dt) override {
    const bool obstacles = sim.obstacle_vector->nObstacles() > 0;
    if (obstacles) {
      // tmpV = 0; kernelUpdateTmpV(sim) (15066-15082) with the reference's own host code -- the ObstacleBlocks live there -- then chi
      // and tmpV (= udef) go up: the device right-hand side reads both (KernelPressureRHS 14849-14875)
      for (auto &info : sim.tmpVInfo()) ((VectorBlock *)info.block)->clear();
      kernelUpdateTmpV(sim);
      dev.upload(CUP3D_FIELD_TMPV);
      dev.upload(CUP3D_FIELD_CHI);
      dev.chi_uploaded_step = sim.step;
      had_obstacles = true;
    } else if (had_obstacles) {
      CUP3D_HIP_CALL(cup3d_sim_fill(dev.handle(), CUP3D_FIELD_CHI, 0.0));
      had_obstacles = false;
    }
    CUP3D_HIP_CALL(cup3d_sim_set_obstacles(dev.handle(), obstacles ? 1 : 0));  // obstacle_vector is replicated: the same on every rank
    if (!dev.vel_on_device) dev.upload(CUP3D_FIELD_VEL);
    else if (obstacles) dev.upload_obstacle_blocks(CUP3D_FIELD_VEL);  // what UpdateObstacles / Penalization changed on the host
    dev.vel_on_device = false;
    if (!(dev.dev_current || (dev.across_steps && dev.host_pres_clean))) dev.upload(CUP3D_FIELD_PRES);
    const cup3d_poisson_params p = poisson_params(sim);
    CUP3D_HIP_CALL(cup3d_pressure_project(dev.handle(), dt, sim.step, &p, &last));
    if (dev.device_led && !obstacles) {  // nothing comes down: the next step starts from the device copies (see DeviceMirror::device_led)
      dev.dev_current = true;
      dev.host_vel_clean = dev.host_pres_clean = false;
      return;
    }
    dev.dev_current = false;
    dev.download(CUP3D_FIELD_VEL);
    dev.download(CUP3D_FIELD_PRES);
    dev.host_vel_clean = dev.host_pres_clean = true;
    // gradP scratch, as the reference leaves it (15146).  Nothing reads it on the host before it is overwritten (AdvectionDiffusion
    // clears tmpV first, 9702-9706; adaptMesh's ComputeVorticity and the projection's own prologue fill it) -- the resident modes
    // leave the host copy stale (3.2 GB per step at 512^3)
    if (!dev.resident) dev.download(CUP3D_FIELD_TMPV);
  }
};

// ComputeForces::operator()(dt), main.cpp:12496-12503, with KernelComputeForces (12250-12494) on the device: the [-4,5) tiles of vel and
// chi around the blocks an obstacle's surface touches are built there and only the 19 per-point arrays and the 19 sums of each such
// block come back.  Installed only with CUP3D_HIP_FORCES=1 (install()).
class ComputeForcesHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  DeviceMirror &dev;

  static constexpr int nQoI = 19;
  // the nineteen members in ObstacleBlock::sumQoI order (7289-7307)
  static void qoi_members(ObstacleBlock &o, Real *q[nQoI]) {
    Real *m[nQoI] = {&o.forcex,   &o.forcey,   &o.forcez,   &o.forcex_P, &o.forcey_P, &o.forcez_P,    &o.forcex_V, &o.forcey_V,    &o.forcez_V, &o.torquex,
                     &o.torquey,  &o.torquez,  &o.drag,     &o.thrust,   &o.Pout,     &o.PoutBnd,     &o.defPower, &o.defPowerBnd, &o.pLocom};
    for (int k = 0; k < nQoI; ++k) q[k] = m[k];
  }
  // the nineteen per-point arrays in the order of cup3d_obstacle_surface::points
  static void point_arrays(ObstacleBlock &o, Real *a[nQoI]) {
    Real *m[nQoI] = {o.pX, o.pY, o.pZ, o.P, o.fX, o.fY, o.fZ, o.fxV, o.fyV, o.fzV, o.omegaX, o.omegaY, o.omegaZ, o.vxDef, o.vX, o.vyDef, o.vY, o.vzDef, o.vZ};
    for (int k = 0; k < nQoI; ++k) a[k] = m[k];
  }

public:
  ComputeForcesHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d) : Operator(s), devp(d), dev(*d) {}
  void operator()(const Real dt) override {
    (void)dt;
    if (sim.obstacle_vector->nObstacles() == 0) return;  // 12497-12498
    static_assert(sizeof(Real) == sizeof(double), "the device operators are FP64");
    dev.handle();
    // the functor reads vel, chi and pres: whatever the device does not hold in its current state goes up first.  host_vel_clean /
    // host_pres_clean ("host copy == device copy") are trusted here in EVERY mode, not only under across_steps as the other operators
    // do: directly behind PressureProjectionHIP in the pipeline (15243-15244), which has just downloaded both, that is right.  It is the
    // across_steps contract all the same: a host that writes vel or pres and then calls this operator on its own must call
    // DeviceMirror::invalidate() first, or the device evaluates the fields it still holds.
    if (!(dev.dev_current || dev.host_vel_clean)) dev.upload(CUP3D_FIELD_VEL);
    if (!(dev.dev_current || dev.host_pres_clean)) dev.upload(CUP3D_FIELD_PRES);
    if (dev.chi_uploaded_step != sim.step) { dev.upload(CUP3D_FIELD_CHI); dev.chi_uploaded_step = sim.step; }
    const std::vector<Info> &I = sim.velInfo();
    const auto &obstacles = sim.obstacle_vector->getObstacleVector();
    const size_t nobst = obstacles.size();
    struct Packed {
      std::vector<ObstacleBlock *> blocks;
      std::vector<int32_t> slots, first, ijk;
      std::vector<double> dchi, udef, points, qoi;
    };
    std::vector<Packed> packed(nobst);
    std::vector<cup3d_obstacle_surface> surf(nobst);
    for (size_t k = 0; k < nobst; ++k) {
      Packed &P = packed[k];
      const std::vector<ObstacleBlock *> &ob = obstacles[k]->getObstacleBlocks();
      P.first.push_back(0);
      for (size_t i = 0; i < I.size(); ++i) {  // block slot i of the mirror is m_vInfo entry i
        ObstacleBlock *o = ob[I[i].blockID];
        if (o == nullptr || o->nPoints == 0) continue;  // 12278-12281
        P.blocks.push_back(o);
        P.slots.push_back((int32_t)i);
        for (int p = 0; p < o->nPoints; ++p) {
          const surface_data *sd = o->surface[p];
          P.ijk.insert(P.ijk.end(), {(int32_t)sd->ix, (int32_t)sd->iy, (int32_t)sd->iz});
          P.dchi.insert(P.dchi.end(), {(double)sd->dchidx, (double)sd->dchidy, (double)sd->dchidz});
        }
        P.first.push_back((int32_t)(P.ijk.size() / 3));
        const double *u = &o->udef[0][0][0][0];
        P.udef.insert(P.udef.end(), u, u + 8 * 8 * 8 * 3);
        Real *q[nQoI];
        qoi_members(*o, q);
        for (int m = 0; m < nQoI; ++m) P.qoi.push_back(*q[m]);  // eight of them carry on (12283-12293)
      }
      P.points.resize((size_t)nQoI * (P.ijk.size() / 3));
      cup3d_obstacle_surface &S = surf[k];
      S.nblocks = (long)P.slots.size();
      S.slots = P.slots.data();
      S.first = P.first.data();
      S.ijk = P.ijk.data();
      S.dchi = P.dchi.data();
      S.udef = P.udef.data();
      const std::array<Real, 3> cm = obstacles[k]->getCenterOfMass(), ut = obstacles[k]->getTranslationVelocity(), om = obstacles[k]->getAngularVelocity();
      for (int d = 0; d < 3; ++d) { S.cm[d] = cm[d]; S.vel[d] = ut[d]; S.omega[d] = om[d]; }
      S.points = P.points.data();
      S.qoi = P.qoi.data();
    }
    int size = 1;
    MPI_Comm_size(sim.comm, &size);
    if (size > 1) {
      const cup3d_grid_t *mesh = nullptr;
      const int32_t *owner = nullptr;
      dev.global_mesh(&mesh, &owner);
      CUP3D_HIP_CALL(cup3d_compute_forces_over_ranks(dev.handle(), mesh, owner, sim.nu, (int)nobst, surf.data()));
    } else {
      CUP3D_HIP_CALL(cup3d_compute_forces(dev.handle(), sim.nu, (int)nobst, surf.data()));
    }
    for (size_t k = 0; k < nobst; ++k) {
      Packed &P = packed[k];
      const size_t np = P.ijk.size() / 3;
      for (size_t b = 0; b < P.blocks.size(); ++b) {
        ObstacleBlock &o = *P.blocks[b];
        Real *a[nQoI], *q[nQoI];
        point_arrays(o, a);
        qoi_members(o, q);
        for (int m = 0; m < nQoI; ++m) {
          for (int p = 0; p < o.nPoints; ++p) a[m][p] = P.points[(size_t)m * np + P.first[b] + p];
          *q[m] = P.qoi[b * nQoI + m];
        }
      }
    }
    sim.obstacle_vector->computeForces();  // 12502: the sums over blocks and ranks (MPI_Allreduce, 13087) stay the host's
  }
};

// CreateObstacles::operator()(dt), main.cpp:13589-13621, with everything after obstacle_vector->create() on the device
// (cup3d_create_obstacles): the geometry -- updateUinf, update, create, which leave sdfLab and udef in the ObstacleBlocks -- stays the
// reference's, and so do the MeshChanged / StaticObstacles gate and finalize().  The blocks' chi, corrected udef, mass / CoM rows, the 13
// momenta, the surface points and the obstacle's centre of mass, mass, J and corrections come back into the reference's own objects;
// the chi field stays on the device and its obstacle blocks are copied into the host grid, which the call has cleared.
// Installed only with CUP3D_HIP_CREATE=1 (install()).
class CreateObstaclesHIP : public Operator {
  std::shared_ptr<DeviceMirror> devp;
  DeviceMirror &dev;

public:
  CreateObstaclesHIP(SimulationData &s, std::shared_ptr<DeviceMirror> d) : Operator(s), devp(d), dev(*d) {}
  void operator()(const Real dt) override {
    (void)dt;
    if (sim.obstacle_vector->nObstacles() == 0) return;  // 13590-13591
    if (sim.MeshChanged == false && sim.StaticObstacles) return;
    sim.MeshChanged = false;
    static_assert(sizeof(Real) == sizeof(double), "the device operators are FP64");
    std::vector<Info> &chiInfo = sim.chiInfo();
    for (size_t i = 0; i < chiInfo.size(); ++i) ((ScalarBlock *)chiInfo[i].block)->clear();  // 13596-13600: the host copy
    sim.uinf = sim.obstacle_vector->updateUinf();
    sim.obstacle_vector->update();
    sim.obstacle_vector->create();
    dev.handle();
    const auto &obstacles = sim.obstacle_vector->getObstacleVector();
    const size_t nobst = obstacles.size();
    struct Packed {
      std::vector<ObstacleBlock *> blocks;
      std::vector<int32_t> slots, first, ijk;
      std::vector<double> sdf, udef, chi, com, momenta, dchi, delta;
    };
    std::vector<Packed> packed(nobst);
    std::vector<cup3d_obstacle_shape> shapes(nobst);
    for (size_t k = 0; k < nobst; ++k) {
      Packed &P = packed[k];
      const std::vector<ObstacleBlock *> &ob = obstacles[k]->getObstacleBlocks();
      for (size_t i = 0; i < chiInfo.size(); ++i) {  // block slot i of the mirror is m_vInfo entry i
        ObstacleBlock *o = ob[chiInfo[i].blockID];
        if (o == nullptr) continue;  // 13304-13305
        P.blocks.push_back(o);
        P.slots.push_back((int32_t)i);
        const double *d = &o->sdfLab[0][0][0], *u = &o->udef[0][0][0][0];
        P.sdf.insert(P.sdf.end(), d, d + 10 * 10 * 10);
        P.udef.insert(P.udef.end(), u, u + 8 * 8 * 8 * 3);
      }
      const size_t n = P.blocks.size();
      P.chi.resize(n * 512);
      P.com.resize(n * 4);
      P.momenta.resize(n * 13);
      P.first.resize(n + 1);
      P.ijk.resize(n * 512 * 3);
      P.dchi.resize(n * 512 * 3);
      P.delta.resize(n * 512);
      cup3d_obstacle_shape &S = shapes[k];
      S.nblocks = (long)n;
      S.slots = P.slots.data();
      S.sdf = P.sdf.data();
      S.udef = P.udef.data();
      S.chi = P.chi.data();
      for (int d = 0; d < 3; ++d) S.transvel_correction[d] = obstacles[k]->transVel_correction[d];  // oldCorrVel, 13436
      S.block_com = P.com.data();
      S.block_momenta = P.momenta.data();
      S.first = P.first.data();
      S.ijk = P.ijk.data();
      S.dchi = P.dchi.data();
      S.delta = P.delta.data();
    }
    CUP3D_HIP_CALL(cup3d_create_obstacles(dev.handle(), (int)nobst, shapes.data()));
    for (size_t k = 0; k < nobst; ++k) {
      Packed &P = packed[k];
      const cup3d_obstacle_shape &S = shapes[k];
      for (size_t b = 0; b < P.blocks.size(); ++b) {
        ObstacleBlock &o = *P.blocks[b];
        std::copy(P.chi.begin() + b * 512, P.chi.begin() + (b + 1) * 512, &o.chi[0][0][0]);
        std::copy(P.udef.begin() + b * 1536, P.udef.begin() + (b + 1) * 1536, &o.udef[0][0][0][0]);
        o.mass = P.com[4 * b];  // 13307-13310, 13350-13353
        o.CoM_x = P.com[4 * b + 1];
        o.CoM_y = P.com[4 * b + 2];
        o.CoM_z = P.com[4 * b + 3];
        const double *m = &P.momenta[13 * b];  // 13441-13445
        o.V = m[0];
        o.FX = m[1]; o.FY = m[2]; o.FZ = m[3];
        o.TX = m[4]; o.TY = m[5]; o.TZ = m[6];
        o.J0 = m[7]; o.J1 = m[8]; o.J2 = m[9]; o.J3 = m[10]; o.J4 = m[11]; o.J5 = m[12];
        for (int32_t p = P.first[b]; p < P.first[b + 1]; ++p) {  // ObstacleBlock::write (7422-7431) with dchi already formed
          o.nPoints++;
          o.surface.push_back(new surface_data(P.ijk[3 * p], P.ijk[3 * p + 1], P.ijk[3 * p + 2], P.dchi[3 * p], P.dchi[3 * p + 1], P.dchi[3 * p + 2], P.delta[p]));
        }
        o.allocate_surface();  // 13401
      }
      for (int d = 0; d < 3; ++d) {
        obstacles[k]->centerOfMass[d] = S.cm[d];  // 13421-13423
        obstacles[k]->transVel_correction[d] = S.transvel_correction[d];  // 13533-13535
        obstacles[k]->angVel_correction[d] = S.angvel_correction[d];  // 13542-13547
      }
      obstacles[k]->mass = S.mass;  // 13532
      for (int q = 0; q < 6; ++q) obstacles[k]->J[q] = S.J[q];  // 13536-13541
    }
    dev.download_obstacle_blocks(CUP3D_FIELD_CHI);  // the rest of the host's chi is the zero it was cleared to
    dev.chi_uploaded_step = sim.step;
    sim.obstacle_vector->finalize();  // 13620
  }
};

// One DeviceMirror per SimulationData, shared by every HIP-backed operator / solver built for it.
inline std::shared_ptr<DeviceMirror> mirror_of(SimulationData &sim) {
  static std::map<SimulationData *, std::weak_ptr<DeviceMirror>> reg;
  std::shared_ptr<DeviceMirror> m = reg[&sim].lock();
  if (!m) { m = std::make_shared<DeviceMirror>(sim); reg[&sim] = m; }
  return m;
}

// makePoissonSolver (main.cpp:14747-14758) with the slot the reference reserves for a GPU solver filled in: -poissonSolver
// "cuda_iterative" (the reference's own name for it, 14750) or "hip_iterative" gives the device solver behind PoissonSolverBase;
// every other value is handed to the reference's factory unchanged ("iterative" -> PoissonSolverAMR, unknown -> its error).
inline std::shared_ptr<PoissonSolverBase> makePoissonSolver(SimulationData &s) {
  if (s.poissonSolver == "cuda_iterative" || s.poissonSolver == "hip_iterative") return std::make_shared<PoissonSolverHIP>(s, mirror_of(s));
  return ::makePoissonSolver(s);
}

struct Installed {
  std::shared_ptr<DeviceMirror> mirror;
  std::shared_ptr<Operator> advdiff;  // AdvectionDiffusionHIP, or AdvectionDiffusionImplicitHIP with -implicitDiffusion 1
  std::shared_ptr<ExternalForcingHIP> forcing;
  std::shared_ptr<FixMassFluxHIP> mass_flux;  // only with CUP3D_HIP_MASSFLUX=1
  std::shared_ptr<UpdateObstaclesHIP> update_obstacles;
  std::shared_ptr<PressureProjectionHIP> projection;
  std::shared_ptr<ComputeForcesHIP> forces;  // only with CUP3D_HIP_FORCES=1
  std::shared_ptr<CreateObstaclesHIP> create_obstacles;  // only with CUP3D_HIP_CREATE=1
};

// Swap the hot-path operators of an initialised Simulation for the HIP-backed ones.
// resident (default: environment CUP3D_HIP_RESIDENT, 0 / 1 / 2): 1 = keep the velocity in HBM between AdvectionDiffusion and
// PressureProjection; 2 = also skip the uploads of vel and pres at the next step while the host copies are known to be current
// (DeviceMirror::across_steps: read its contract).  Allowed only if every operator the reference put between the two (setupOperators 15229-15246) is
// ExternalForcing (then run on the device too) or one of the obstacle operators: UpdateObstacles and Penalization touch the
// velocity only in the blocks an obstacle covers, so those blocks alone make the round trip (UpdateObstaclesHIP fetches them,
// PressureProjectionHIP sends them back); without obstacles both return immediately (13813-13814, 14327-14328).  With
// FixMassFlux in between, every operator round-trips in full as before -- unless CUP3D_HIP_MASSFLUX=1 (environment): FixMassFlux
// (15236-15237) is then replaced by FixMassFluxHIP, which runs on the device while the velocity is resident there, and counts as a device
// operator for this rule, so that a channel run (-bFixMassFlux 1) can stay resident.  Without the variable nothing changes.
// CUP3D_HIP_FORCES=1 (environment): ComputeForces (15244) is replaced by ComputeForcesHIP as well; without it that entry of the
// pipeline stays the reference's own.  CUP3D_HIP_CREATE=1: CreateObstacles (15230) is replaced by CreateObstaclesHIP in the same way.
inline Installed install(SimulationData &sim, int resident = -1) {
  Installed r;
  r.mirror = mirror_of(sim);
  if (resident < 0) {
    const char *e = getenv("CUP3D_HIP_RESIDENT");
    resident = e ? atoi(e) : 0;
  }
  const char *massflux_env = getenv("CUP3D_HIP_MASSFLUX");
  const bool massflux = massflux_env && atoi(massflux_env) == 1;
  bool between = false, safe = true;
  for (auto &op : sim.pipeline) {
    if (std::dynamic_pointer_cast<AdvectionDiffusion>(op) || std::dynamic_pointer_cast<AdvectionDiffusionImplicit>(op)) between = true;
    else if (std::dynamic_pointer_cast<PressureProjection>(op)) between = false;
    else if (between && !(std::dynamic_pointer_cast<ExternalForcing>(op) || std::dynamic_pointer_cast<UpdateObstacles>(op) ||
                          std::dynamic_pointer_cast<Penalization>(op) || (massflux && std::dynamic_pointer_cast<FixMassFlux>(op))))
      safe = false;
  }
  r.mirror->resident = resident != 0 && safe;
  r.mirror->across_steps = resident >= 2 && safe;
  r.mirror->device_led = resident >= 3 && safe;
  const char *forces_env = getenv("CUP3D_HIP_FORCES");
  const bool forces = forces_env && atoi(forces_env) == 1;
  if (forces) r.mirror->keep_global_mesh = true;
  const char *create_env = getenv("CUP3D_HIP_CREATE");
  const bool create = create_env && atoi(create_env) == 1;
  for (auto &op : sim.pipeline) {
    if (forces && std::dynamic_pointer_cast<ComputeForces>(op)) {
      r.forces = std::make_shared<ComputeForcesHIP>(sim, r.mirror);
      op = r.forces;
    } else if (create && std::dynamic_pointer_cast<CreateObstacles>(op)) {
      r.create_obstacles = std::make_shared<CreateObstaclesHIP>(sim, r.mirror);
      op = r.create_obstacles;
    } else if (std::dynamic_pointer_cast<AdvectionDiffusion>(op)) {
      r.advdiff = std::make_shared<AdvectionDiffusionHIP>(sim, r.mirror);
      op = r.advdiff;
    } else if (std::dynamic_pointer_cast<AdvectionDiffusionImplicit>(op)) {  // setupOperators 15231-15232
      r.advdiff = std::make_shared<AdvectionDiffusionImplicitHIP>(sim, r.mirror);
      op = r.advdiff;
    } else if (r.mirror->resident && std::dynamic_pointer_cast<ExternalForcing>(op)) {
      r.forcing = std::make_shared<ExternalForcingHIP>(sim, r.mirror, op);
      op = r.forcing;
    } else if (massflux && r.mirror->resident && std::dynamic_pointer_cast<FixMassFlux>(op)) {
      r.mass_flux = std::make_shared<FixMassFluxHIP>(sim, r.mirror, op);
      op = r.mass_flux;
    } else if (r.mirror->resident && std::dynamic_pointer_cast<UpdateObstacles>(op)) {
      r.update_obstacles = std::make_shared<UpdateObstaclesHIP>(sim, r.mirror, op);
      op = r.update_obstacles;
    } else if (std::dynamic_pointer_cast<PressureProjection>(op)) {
      r.projection = std::make_shared<PressureProjectionHIP>(sim, r.mirror);
      op = r.projection;
    }
  }
  return r;
}

// Device-led replacement for simulation.calcMaxTimestep() (main.cpp:15254-15305; DeviceMirror::device_led).  Nothing of the
// reference's function is restated here: the maximum comes from cup3d_max_u (findMaxU incl. its MAX all-reduce, 8603-8623, exact) and
// the time-step rule and the pressure-extrapolation coefficients from the library (cup3d_calc_max_timestep2, pinned against the
// reference by tests/test_host_indexing.py); this function only moves the results into SimulationData.
inline Real calcMaxTimestep(Simulation &S, DeviceMirror &dev) {
  SimulationData &sim = S.sim;
  // host copy current (first step, after an adaptation, obstacle runs), or a fixed-dt run (CFL <= 0: nothing for the library to choose)
  if (!dev.dev_current) return S.calcMaxTimestep();
  if (!(sim.CFL > 0)) { dev.sync_host(); return S.calcMaxTimestep(); }
  auto stop = [&](const char *why, double value) {
    if (sim.rank == 0) fprintf(stderr, "cup3d_hip::calcMaxTimestep: %s (%g) at step %d -- stopping the run\n", why, value, sim.step);
    MPI_Abort(sim.comm, 1);
  };
  const double uinf[3] = {sim.uinf[0], sim.uinf[1], sim.uinf[2]};
  double umax = 0, coef[3] = {sim.coefU[0], sim.coefU[1], sim.coefU[2]};
  CUP3D_HIP_CALL(cup3d_max_u(dev.handle(), uinf, &umax));
  if (umax > sim.uMax_allowed) stop("velocity maximum above -uMax_allowed", umax);
  const double previous = sim.dt;
  const double dt = cup3d_calc_max_timestep2(sim.hmin, umax, sim.nu, sim.CFL, sim.step, sim.rampup, previous, coef, sim.implicitDiffusion ? 1 : 0);
  if (!(dt > 0)) stop("non-positive time step", dt);
  sim.uMax_measured = umax;
  sim.dt_old = previous;
  sim.dt = dt;
  for (int i = 0; i < 3; ++i) sim.coefU[i] = coef[i];
  if (sim.DLM > 0) sim.lambda = sim.DLM / dt;
  if (sim.rank == 0) printf("main.cpp: step: %d, time: %f\n", sim.step, sim.time);  // the progress line the reference's loop prints from here
  return sim.dt;
}
// ... and the companion of Simulation::advance (15306-15326) in that mode: adaptMesh (15314) and dump (15307-15313) read the host fields
inline bool advance(Simulation &S, DeviceMirror &dev, const Real dt) {
  SimulationData &sim = S.sim;
  if ((sim.dumpTime > 0 && sim.time >= sim.nextDumpTime) || sim.step % 20 == 0 || sim.step < 10) dev.sync_host();
  return S.advance(dt);
}

}  // namespace cup3d_hip
