// Ghosted block tiles for consumers outside the library: cup3d_sim_labs[_device] on one rank (k_labs), cup3d_sim_labs_over_ranks[_device]
// on a mesh spread over ranks (k_labs_view).  What a tile is and the phases A-F that build it: labs.hpp.
#include <cstring>
#include "labs.hpp"

namespace cup3d {

// k_labs_view's block source: slots [0, n_local) of the rank's tensorial view are rows of the sim's own field array, read in place; a
// ghost slot is a row of the call's ghost pool, found through pool_of (-1: not fetched -- row 0 of the pool, which holds NaN, so that
// a read the request plan did not foresee shows in the tile instead of leaving the buffer).
struct LabSrcView {
  const double *__restrict__ field;
  const double *__restrict__ pool;      // [1 + fetched ghosts][nc][512]
  const int32_t *__restrict__ pool_of;  // [nghost]
  int n_local;
  __device__ __forceinline__ const double *blk(int slot, int nc, int c) const {
    if (slot < n_local) return field + ((size_t)slot * nc + c) * 512;
    return pool + ((size_t)(pool_of[slot - n_local] + 1) * nc + c) * 512;
  }
};

#define LABS_SLOT slots ? slots[blockIdx.x] : first + (int)blockIdx.x
#define LABS_AFTER_SLOT double *__restrict__ tile = out + (size_t)blockIdx.x * L3 * nc;
template <int W>
__global__ void __launch_bounds__(256) k_labs(LabDev a, const int32_t *__restrict__ slots, int first, int star, const double *__restrict__ src, int nc,
                                              double *__restrict__ out) {
#include "labs_setup.hpp"
  for (int c = 0; c < nc; ++c) {
#include "labs_phases.hpp"
    // F. the tile leaves in the reference's layout; what the reference leaves undefined leaves as NaN
    for (int e = t; e < L3; e += 256) {
      double v = lab[e];
      if (W <= 2 && star) {
        const int x = e % L - W, y = (e / L) % L - W, z = e / (L * L) - W;
        if ((x < 0 || x > 7) + (y < 0 || y > 7) + (z < 0 || z > 7) > 1) v = __builtin_nan("");
      }
      tile[(size_t)e * nc + c] = v;
    }
    __syncthreads();
  }
}

// the same as k_labs for the local blocks of a rank's tensorial view: tables of the view, ghost blocks in the pool
#undef LABS_BLOCK
#undef LABS_CELL
#define LABS_BLOCK(slot, c) src.blk(slot, nc, c)
#define LABS_CELL(slot, c, i) src.blk(slot, nc, c)[i]
template <int W>
__global__ void __launch_bounds__(256) k_labs_view(LabDev a, const int32_t *__restrict__ slots, int first, int star, LabSrcView src, int nc, double *__restrict__ out) {
#include "labs_setup.hpp"
  for (int c = 0; c < nc; ++c) {
#include "labs_phases.hpp"
    // F, as in k_labs
    for (int e = t; e < L3; e += 256) {
      double v = lab[e];
      if (W <= 2 && star) {
        const int x = e % L - W, y = (e / L) % L - W, z = e / (L * L) - W;
        if ((x < 0 || x > 7) + (y < 0 || y > 7) + (z < 0 || z > 7) > 1) v = __builtin_nan("");
      }
      tile[(size_t)e * nc + c] = v;
    }
    __syncthreads();
  }
}
#undef LABS_SLOT
#undef LABS_AFTER_SLOT
#undef LABS_BLOCK
#undef LABS_CELL

void finer_tables(const Grid *mo, int64_t nloc, std::vector<int32_t> &finer_row, std::vector<int32_t> &finer) {
  finer_row.assign((size_t)nloc, -1);
  for (int64_t b = 0; b < nloc; ++b) {
    bool any = false;
    for (int c = 0; c < 27; ++c) any = any || mo->nbr27[27 * (size_t)b + c] == kNbrFiner;
    if (!any) continue;
    finer_row[b] = (int32_t)(finer.size() / 216);
    finer.resize(finer.size() + 216, -1);
    int32_t *row = finer.data() + finer.size() - 216;
    const int l = mo->blevel[b];
    for (int icode = 0; icode < 27; ++icode) {
      if (mo->nbr27[27 * (size_t)b + icode] != kNbrFiner) continue;
      const int code[3] = {icode % 3 - 1, (icode / 3) % 3 - 1, icode / 9 - 1};
      for (int q = 0; q < 8; ++q) {
        int fi[3];
        bool used = true;
        for (int d = 0; d < 3; ++d) {
          const int bit = (q >> d) & 1;
          if (code[d] != 0 && bit) used = false;
          fi[d] = 2 * mo->index[3 * (size_t)b + d] + (code[d] < 0 ? -1 : (code[d] > 0 ? 2 : bit));
        }
        if (used) row[icode * 8 + q] = mo->leaf(l + 1, fi);
      }
    }
  }
  if (finer.empty()) finer.assign(216, -1);
}

// ==== cup3d_sim_labs / cup3d_sim_labs_device: the host side of k_labs
constexpr size_t kLabStageBytes = (size_t)64 << 20;  // device staging buffer of the host variant
constexpr long kLabSlotCap = 8192;                   // listed tiles per launch (the smallest tile, 10^3 doubles, fills the buffer with as many)

struct LabTables {
  LabIndex tab;
  Dev<int32_t> d_slots;     // slot list of one launch: device copy,
  Pinned<int32_t> h_slots;  // pinned host copy
  hipEvent_t ev_slots = nullptr;                   // the upload that last read h_slots
  bool slots_in_flight = false;
  Dev<double> stage;
  ~LabTables() { if (ev_slots) (void)hipEventDestroy(ev_slots); }
};

static void labs_view_destroy(Sim *s);
void labs_destroy(Sim *s) {
  labs_view_destroy(s);  // the cached view, its tables and the ghost pool of cup3d_sim_labs_over_ranks
  delete s->labs;
  s->labs = nullptr;
}

// tables of k_labs, built when the first tile is asked for
static int labs_prepare(Sim *s, bool want_stage) {
  if (!s->labs) {
    MeshOf mesh;
    const Grid *mo = mesh.get(s->grid, "cup3d_sim_labs");
    if (!mo) return CUP3D_EINVAL;
    s->labs = new LabTables();
    LabTables *T = s->labs;
    auto build = [&]() -> int {
      int rc = T->tab.build(mo, mo->nblocks(), "cup3d_sim_labs");
      if (rc) return rc;
      s->bytes += T->tab.bytes;
      if ((rc = T->d_slots.alloc(kLabSlotCap, s)) || (rc = T->h_slots.alloc(kLabSlotCap, hipHostMallocDefault))) return rc;
      CUP3D_HIP(hipEventCreateWithFlags(&T->ev_slots, hipEventDisableTiming));
      return CUP3D_OK;
    };
    const size_t before = s->bytes;
    const int rc = build();
    if (rc) {  // all or nothing, on the ledger too
      delete s->labs;
      s->labs = nullptr;
      s->bytes = before;
      return rc;
    }
  }
  if (want_stage && !s->labs->stage) return s->labs->stage.alloc(kLabStageBytes / sizeof(double), s);
  return CUP3D_OK;
}

// tiles [t0, t0 + m) of the request -> out (device), on the compute stream; m <= kLabSlotCap when slots are listed
static int labs_launch(Sim *s, const double *f, int nc, long t0, long m, const int32_t *slots, int w, int tensorial, int bc_comp, double *out) {
  LabTables *T = s->labs;
  const LabDev a = T->tab.dev(s->grid, nc == 1 ? bc_comp : -1);
  const int32_t *d_slots = nullptr;
  if (slots) {
    if (T->slots_in_flight) CUP3D_HIP(hipEventSynchronize(T->ev_slots));  // the pinned copy is free again
    memcpy(T->h_slots, slots + t0, (size_t)m * sizeof(int32_t));
    CUP3D_HIP(hipMemcpyAsync(T->d_slots, T->h_slots, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, stream()));
    CUP3D_HIP(hipEventRecord(T->ev_slots, stream()));
    T->slots_in_flight = true;
    d_slots = T->d_slots;
  }
  const int star = tensorial ? 0 : 1;
  ProfileScope ps("labs");
  switch (w) {
    case 1: hipLaunchKernelGGL(k_labs<1>, dim3((unsigned)m), dim3(256), 0, stream(), a, d_slots, (int)t0, star, f, nc, out); break;
    case 2: hipLaunchKernelGGL(k_labs<2>, dim3((unsigned)m), dim3(256), 0, stream(), a, d_slots, (int)t0, star, f, nc, out); break;
    case 3: hipLaunchKernelGGL(k_labs<3>, dim3((unsigned)m), dim3(256), 0, stream(), a, d_slots, (int)t0, star, f, nc, out); break;
    default: hipLaunchKernelGGL(k_labs<4>, dim3((unsigned)m), dim3(256), 0, stream(), a, d_slots, (int)t0, star, f, nc, out); break;
  }
  CUP3D_HIP(hipGetLastError());
  return CUP3D_OK;
}

// the checks both entry points share; nothing is allocated or launched before they pass
static int labs_check(Sim *s, int field, long n, const int32_t *slots, int width, int scalar_dir, const void *out, const double **f, int *nc, bool over_ranks = false) {
  if (!out && !(over_ranks && n == 0)) { set_error("cup3d_sim_labs: null output"); return CUP3D_EINVAL; }
  *f = s->field(field, nc);
  if (!*f) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
  if (width < 1 || width > 4) { set_error("cup3d_sim_labs: width %d; the tiles are pinned for the boxes [-w, w+1), w = 1..4", width); return CUP3D_EINVAL; }
  if (scalar_dir < -1 || scalar_dir > 2) { set_error("cup3d_sim_labs: scalar_dir %d (expected -1, 0, 1 or 2)", scalar_dir); return CUP3D_EINVAL; }
  if (scalar_dir >= 0 && *nc == 3) { set_error("cup3d_sim_labs: scalar_dir %d on a vector field (it selects BlockLabBC<.., direction> for a scalar)", scalar_dir); return CUP3D_EINVAL; }
  if (!over_ranks && (s->grid->n_local >= 0 || s->grid->nranks > 1)) {
    set_error("cup3d_sim_labs: this sim holds one rank's share of a grid spread over %d ranks; tiles whose neighbours live on another rank are out of scope "
              "(they need the tensorial ghost-block exchange at stencil width: cup3d_sim_labs_over_ranks)", s->grid->nranks);
    return CUP3D_EINVAL;
  }
  if (n < 0 || (!slots && n != (long)s->nb && !(over_ranks && n == 0))) { set_error("cup3d_sim_labs: n = %ld (slots = NULL asks for all %ld local blocks)", n, (long)s->nb); return CUP3D_EINVAL; }
  if (slots)
    for (long i = 0; i < n; ++i)
      if (slots[i] < 0 || slots[i] >= s->nb) { set_error("block slot %d out of range", (int)slots[i]); return CUP3D_EINVAL; }
  return CUP3D_OK;
}

// ==== cup3d_sim_labs_over_ranks / cup3d_sim_labs_over_ranks_device.  The same tiles when the mesh is spread over ranks: what BlockLabMPI::load
// (main.cpp:4648-4658) gets from SynchronizerMPI_AMR::fetch (2423-2544).  The sim lives on its rank view of the mesh or on its share of a
// uniform grid; the tiles are built through the tables of the rank's TENSORIAL view (every same-level, coarser and finer leaf of the
// 27-point neighbourhood is a ghost slot there), which is derived once per (mesh, owner) and kept in the sim.  Per call:
//   needs    Grid::lab_boxes replays phases A and B of the kernel (labs_phases.hpp) for the requested blocks: per ghost block the box of cells read;
//   request  one double per ghost block (the box as an exact integer, 0: nothing) travels to the block's owner -- the view's block plan
//            with the two count vectors swapped -- and comes back to the host, so that owner and receiver know every message's length;
//   data     the owner packs the boxes (k_pack_boxes), one exchange of nc doubles per cell, the receiver scatters them into a pool that
//            holds the fetched ghost blocks only (k_unpack_boxes; pool_of[ghost] -> pool row);
//   tiles    k_labs_view reads local blocks from the sim's field array in place and ghost blocks from the pool.
// Everything crosses ranks through agree() and exchange_items() (RCCL, the host transport, the in-process test communicator).
struct LabsView {
  // the cache key is CONTENT: the leaves of the mesh and the owner of each (a pointer can be freed and reused)
  std::vector<int32_t> key_level, key_owner;
  std::vector<int64_t> key_Z;
  std::unique_ptr<Grid> tv;
  LabIndex tab;  // tables of k_labs_view (local rows of tv)
  // one call's plan, host side (members: the uploads read them after the functions that fill them returned) ...
  std::vector<uint8_t> gbox, sbox, rbox;
  std::vector<double> h_req, h_got;
  std::vector<int32_t> pool_of, tile_slots;
  std::vector<long long> soff, roff;
  std::vector<int64_t> send_cells, recv_cells;
  // ... and device side
  DevGrow d_req, d_got, d_pool_of, d_sslots, d_sbox, d_soff, d_rbox, d_roff, d_pack, d_recv, d_pool, d_slots, d_stage;
};

static void labs_view_destroy(Sim *s) {
  LabsView *V = s->labs_view;
  if (!V) return;
  s->bytes -= V->tab.bytes;
  delete V;  // the grow-only buffers take their own bytes off
  s->labs_view = nullptr;
}

// the rank's tensorial view of (mesh, owner) with its device tables: the cached one when mesh and owner still say the same
static int labs_view_get(Sim *s, const Grid *gm, const int32_t *owner, LabsView **out) {
  const Grid *g = s->grid;
  const size_t nbg = (size_t)gm->nblocks();
  LabsView *V = s->labs_view;
  if (V && V->key_level == gm->blevel && V->key_Z == gm->Z && V->key_owner.size() == nbg && std::equal(V->key_owner.begin(), V->key_owner.end(), owner)) {
    *out = V;
    return CUP3D_OK;
  }
  labs_view_destroy(s);
  std::unique_ptr<Grid> tv;
  try {
    for (int d = 0; d < 3; ++d)
      if (gm->bpd[d] != g->bpd[d] || gm->bc[d] != g->bc[d]) throw std::invalid_argument("mesh and sim belong to different boxes");
    if (gm->level_max != g->level_max) throw std::invalid_argument("mesh and sim belong to different boxes");
    tv = gm->rank_view(owner, g->rank, g->nranks, /*tensorial=*/true);
    // the sim's blocks are this rank's leaves of the mesh, one by one and in the same order
    if (tv->n_local != s->nb) throw std::invalid_argument("the sim does not hold this rank's blocks of the mesh");
    for (int64_t b = 0; b < s->nb; ++b)
      if (tv->blevel[b] != (g->multilevel ? g->blevel[b] : g->level) || tv->Z[b] != g->Z[b]) throw std::invalid_argument("the sim's blocks are not this rank's leaves of the mesh (level, Z)");
  } catch (const std::exception &e) {
    set_error("cup3d_sim_labs_over_ranks: %s", e.what());
    return CUP3D_EINVAL;
  }
  V = new LabsView();
  s->labs_view = V;
  const int rc = V->tab.build(tv.get(), tv->n_local, "cup3d_sim_labs_over_ranks");
  s->bytes += V->tab.bytes;  // labs_view_destroy takes them off again
  if (rc) {
    labs_view_destroy(s);
    return rc;
  }
  V->key_level = gm->blevel;
  V->key_Z = gm->Z;
  V->key_owner.assign(owner, owner + nbg);
  V->tv = std::move(tv);
  *out = V;
  return CUP3D_OK;
}

// a box of cells of one block as an exact integer (six 4-bit fields; 0: nothing) and back; false: not a box inside a block
static double box_encode(const uint8_t *b) {
  return (double)(b[0] | (b[1] << 4) | (b[2] << 8) | (b[3] << 12) | (b[4] << 16) | (b[5] << 20));
}
static bool box_decode(double v, uint8_t *b, int64_t *vol) {
  if (!(v >= 0.0 && v < 16777216.0) || v != (double)(long)v) return false;
  const long k = (long)v;
  *vol = 1;
  for (int i = 0; i < 6; ++i) b[i] = (uint8_t)((k >> (4 * i)) & 15);
  if (k == 0) { *vol = 0; return true; }
  for (int d = 0; d < 3; ++d) {
    if (b[d] >= b[3 + d] || b[3 + d] > 8) return false;
    *vol *= b[3 + d] - b[d];
  }
  return true;
}

static int labs_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh_h, const int32_t *owner, int field, long n, const int32_t *slots, int width, int tensorial,
                           int scalar_dir, void *out, bool to_host) {
  if (!h) return CUP3D_EINVAL;  // (without the sim there is no communicator to tell the other ranks through)
  Sim *s = reinterpret_cast<Sim *>(h);
  const Grid *gm = reinterpret_cast<const Grid *>(mesh_h);
  const double *f = nullptr;
  int nc = 0;
  LabsView *V = nullptr;
  // what one rank can get wrong on its own; the ranks agree on the outcome before anything is exchanged
  auto local_part = [&]() -> int {
    if (!mesh_h || !owner) { set_error("cup3d_sim_labs_over_ranks: null argument"); return CUP3D_EINVAL; }
    int rc = labs_check(s, field, n, slots, width, scalar_dir, out, &f, &nc, /*over_ranks=*/true);
    if (rc) return rc;
    if (!gm->multilevel || gm->n_local >= 0) { set_error("cup3d_sim_labs_over_ranks needs the GLOBAL mesh object (cup3d_grid_create_mesh), not a rank view"); return CUP3D_EINVAL; }
    if ((rc = labs_view_get(s, gm, owner, &V))) return rc;
    const Grid *tv = V->tv.get();
    try {
      tv->lab_boxes(n ? slots : nullptr, n, width, V->gbox);
    } catch (const std::exception &e) {
      set_error("cup3d_sim_labs_over_ranks: %s", e.what());
      return CUP3D_EINVAL;
    }
    const size_t ng = (size_t)tv->nghost();
    V->h_req.resize(ng);
    for (size_t g = 0; g < ng; ++g) V->h_req[g] = box_encode(V->gbox.data() + 6 * g);
    V->h_got.assign(tv->send_blocks.size(), 0.0);
    if ((rc = V->d_req.upload(V->h_req, stream(), s)) || (rc = V->d_got.need(std::max<size_t>(V->h_got.size(), 1) * sizeof(double), s))) return rc;
    if (n && slots) {
      V->tile_slots.assign(slots, slots + n);
      if ((rc = V->d_slots.upload(V->tile_slots, stream(), s))) return rc;
    }
    return CUP3D_OK;
  };
  int rc = agree(s, local_part(), "cup3d_sim_labs_over_ranks");
  if (rc) return rc;
  const Grid *tv = V->tv.get();
  const int nranks = tv->nranks;
  const size_t ng = (size_t)tv->nghost(), nsend = tv->send_blocks.size();
  // ---- request: my ghosts' boxes -> their owners; what comes back is what I have to pack
  {
    ProfileScope ps("labs_request");
    if ((rc = exchange_items(s, V->d_req.as<const double>(), tv->recv_block_count, V->d_got.as<double>(), tv->send_block_count, 1))) return rc;
    if (nsend) CUP3D_HIP(hipMemcpyAsync(V->h_got.data(), V->d_got.get(), nsend * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));
  }
  // ---- the two sides of the data exchange
  V->send_cells.assign(nranks, 0);
  V->recv_cells.assign(nranks, 0);
  std::vector<int32_t> pslots;
  V->sbox.clear(); V->soff.clear(); V->rbox.clear(); V->roff.clear();
  V->pool_of.assign(ng, -1);
  long long so = 0, ro = 0;
  {
    size_t i = 0;
    for (int p = 0; p < nranks; ++p)
      for (int64_t k = 0; k < tv->send_block_count[p]; ++k, ++i) {
        uint8_t b[6];
        int64_t vol;
        if (!box_decode(V->h_got[i], b, &vol)) { set_error("cup3d_sim_labs_over_ranks: rank %d asked for something that is not a box of cells", p); return CUP3D_ESTATE; }
        if (!vol) continue;
        pslots.push_back(tv->send_blocks[i]);
        V->sbox.insert(V->sbox.end(), b, b + 6);
        V->soff.push_back(so);
        so += vol;
        V->send_cells[p] += vol;
      }
  }
  int32_t nrows = 0;
  for (size_t g = 0; g < ng; ++g) {
    const uint8_t *b = V->gbox.data() + 6 * g;
    const int64_t vol = (int64_t)(b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
    if (!vol) continue;
    V->pool_of[g] = nrows++;
    V->rbox.insert(V->rbox.end(), b, b + 6);
    V->roff.push_back(ro);
    ro += vol;
    V->recv_cells[tv->ghost_owner[g]] += vol;
  }
  const size_t per = (size_t)nc * 512;
  const size_t pool_doubles = ((size_t)nrows + 1) * per;
  {
    ProfileScope ps("labs_data");
    if ((rc = V->d_sslots.upload(pslots, stream(), s)) || (rc = V->d_sbox.upload(V->sbox, stream(), s)) || (rc = V->d_soff.upload(V->soff, stream(), s)) ||
        (rc = V->d_rbox.upload(V->rbox, stream(), s)) || (rc = V->d_roff.upload(V->roff, stream(), s)) || (rc = V->d_pool_of.upload(V->pool_of, stream(), s)) ||
        (rc = V->d_pack.need(std::max<size_t>((size_t)so * nc, 1) * sizeof(double), s)) || (rc = V->d_recv.need(std::max<size_t>((size_t)ro * nc, 1) * sizeof(double), s)) ||
        (rc = V->d_pool.need(pool_doubles * sizeof(double), s)))
      return rc;
    CUP3D_HIP(hipStreamSynchronize(stream()));  // pslots is a local: its upload has read it
    if ((rc = launch_pack_boxes(f, V->d_sslots.as<const int32_t>(), V->d_sbox.as<const unsigned char>(), V->d_soff.as<const long long>(), nc, V->d_pack.as<double>(),
                                (unsigned)pslots.size(), stream())))
      return rc;
    if ((rc = exchange_items(s, V->d_pack.as<const double>(), V->send_cells, V->d_recv.as<double>(), V->recv_cells, (size_t)nc))) return rc;
    // row 0 of the pool is what a ghost block that was not fetched reads as: NaN.  "poison_ghosts" (tests): so does every cell of a
    // fetched block that did not travel, as after the star exchange
    if ((rc = launch_nan_fill(V->d_pool.as<double>(), debug_option("poison_ghosts") ? pool_doubles : per, stream()))) return rc;
    if ((rc = launch_unpack_boxes(V->d_pool.as<double>() + per, V->d_rbox.as<const unsigned char>(), V->d_roff.as<const long long>(), nc, V->d_recv.as<const double>(),
                                  (unsigned)nrows, stream())))
      return rc;
  }
  // ---- tiles
  if (n == 0) {
    CUP3D_HIP(hipStreamSynchronize(stream()));
    return CUP3D_OK;
  }
  const LabDev a = V->tab.dev(s->grid, nc == 1 ? scalar_dir : -1);
  LabSrcView src{f, V->d_pool.as<const double>(), V->d_pool_of.as<const int32_t>(), (int)tv->n_local};
  const int star = tensorial ? 0 : 1;
  const size_t L = 8 + 2 * (size_t)width, tile = L * L * L * nc;
  long cap = n;
  if (to_host) {
    if ((rc = V->d_stage.need(std::min<size_t>(kLabStageBytes, (size_t)n * tile * sizeof(double)), s))) return rc;
    cap = std::max<long>(1, (long)(kLabStageBytes / (tile * sizeof(double))));
  }
  for (long t0 = 0; t0 < n; t0 += cap) {  // the host variant goes through its bounded staging buffer chunk by chunk
    const long m = std::min(cap, n - t0);
    double *dst = to_host ? V->d_stage.as<double>() : (double *)out + (size_t)t0 * tile;
    const int32_t *sl = slots ? V->d_slots.as<const int32_t>() + t0 : nullptr;
    {
      ProfileScope ps("labs_view");
      switch (width) {
        case 1: hipLaunchKernelGGL(k_labs_view<1>, dim3((unsigned)m), dim3(256), 0, stream(), a, sl, (int)t0, star, src, nc, dst); break;
        case 2: hipLaunchKernelGGL(k_labs_view<2>, dim3((unsigned)m), dim3(256), 0, stream(), a, sl, (int)t0, star, src, nc, dst); break;
        case 3: hipLaunchKernelGGL(k_labs_view<3>, dim3((unsigned)m), dim3(256), 0, stream(), a, sl, (int)t0, star, src, nc, dst); break;
        default: hipLaunchKernelGGL(k_labs_view<4>, dim3((unsigned)m), dim3(256), 0, stream(), a, sl, (int)t0, star, src, nc, dst); break;
      }
    }
    CUP3D_HIP(hipGetLastError());
    if (to_host) {
      CUP3D_HIP(hipMemcpyAsync((double *)out + (size_t)t0 * tile, V->d_stage.get(), (size_t)m * tile * sizeof(double), hipMemcpyDeviceToHost, stream()));
      CUP3D_HIP(hipStreamSynchronize(stream()));
    }
  }
  if (to_host) stats_field_download((size_t)n * tile * sizeof(double));
  return CUP3D_OK;
}

}  // namespace cup3d
using namespace cup3d;
extern "C" {
int cup3d_sim_labs_device(cup3d_sim_t *h, int field, long n, const int32_t *slots, int width, int tensorial, int scalar_dir, void *device_out) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const double *f;
  int nc, rc;
  if ((rc = labs_check(s, field, n, slots, width, scalar_dir, device_out, &f, &nc)) || (rc = labs_prepare(s, false))) return rc;
  const size_t L = 8 + 2 * (size_t)width, per = L * L * L * nc;
  for (long t0 = 0; t0 < n; t0 += kLabSlotCap) {
    const long m = std::min(kLabSlotCap, n - t0);
    if ((rc = labs_launch(s, f, nc, t0, m, slots, width, tensorial, scalar_dir, (double *)device_out + (size_t)t0 * per))) return rc;
  }
  return CUP3D_OK;
}

int cup3d_sim_labs(cup3d_sim_t *h, int field, long n, const int32_t *slots, int width, int tensorial, int scalar_dir, double *host_out) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const double *f;
  int nc, rc;
  if ((rc = labs_check(s, field, n, slots, width, scalar_dir, host_out, &f, &nc)) || (rc = labs_prepare(s, true))) return rc;
  const size_t L = 8 + 2 * (size_t)width, per = L * L * L * nc;
  const long cap = std::max<long>(1, std::min<long>(kLabSlotCap, (long)(kLabStageBytes / (per * sizeof(double)))));
  for (long t0 = 0; t0 < n; t0 += cap) {  // the staging buffer is bounded: large requests go through it chunk by chunk
    const long m = std::min(cap, n - t0);
    if ((rc = labs_launch(s, f, nc, t0, m, slots, width, tensorial, scalar_dir, s->labs->stage))) return rc;
    CUP3D_HIP(hipMemcpyAsync(host_out + (size_t)t0 * per, s->labs->stage, (size_t)m * per * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));
  }
  stats_field_download((size_t)n * per * sizeof(double));
  return CUP3D_OK;
}

int cup3d_sim_labs_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, int field, long n, const int32_t *slots, int width, int tensorial,
                              int scalar_dir, double *host_out) {
  return labs_over_ranks(h, mesh, owner, field, n, slots, width, tensorial, scalar_dir, host_out, true);
}

int cup3d_sim_labs_over_ranks_device(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, int field, long n, const int32_t *slots, int width,
                                     int tensorial, int scalar_dir, void *device_out) {
  return labs_over_ranks(h, mesh, owner, field, n, slots, width, tensorial, scalar_dir, device_out, false);
}
}  // extern "C"
