// Mesh-adaptation block operators on the device: the data-movement part of MeshAdaptation (main.cpp:5023-5583), bit-exact with the
// reference (tests/test_gpu_adapt.py).  Its two arithmetic rules are stated once: compress8 <- compress 5272-5329 (8-cell mean with the
// reference's association), refine_cell <- refine_1 + RefineBlocks 5227-5249, 5493-5565 (2nd-order Taylor expansion from the [-1,2) tile).
//   whole-mesh transitions between two uniform levels l and l+1: cup3d_restrict (k_restrict), cup3d_prolong (k_prolong: 26 same-level
//     neighbours + ordered domain-face passes), cup3d_tag_blocks <- TagLoadedBlock 5566-5582 + the level clamps of TagBlocksVector 5207-5211;
//   any old mesh to any new one (cup3d_adapt_transfer on one rank, cup3d_adapt_migrate over ranks): a leaf is copied (k_copy_blocks), the parent
//     of an octet compressed (k_compress_blocks), the children of a leaf refined from its ghosted tile (k_refine: the lab phases at W = 1).
#include "labs.hpp"
#include "tile.hpp"

namespace cup3d {

// compress, main.cpp:5298-5302: mean of the 2x2x2 cells with low corner (i, j, kk) of the block component `b`, in the reference's pairing
__device__ __forceinline__ double compress8(const double *b, int i, int j, int kk) {
#define B(a, bb, cc) b[((kk + (cc)) * 8 + (j + (bb))) * 8 + (i + (a))]
  return 0.125 * ((B(0, 0, 0) + B(1, 1, 1)) + (B(1, 0, 0) + B(0, 1, 1)) + (B(0, 1, 0) + B(1, 0, 1)) + (B(1, 1, 0) + B(0, 0, 1)));
#undef B
}

// RefineBlocks, main.cpp:5493-5565, for ONE coarse cell (x, y, z): the nine derivatives from its 3x3x3 neighbourhood in the ghosted tile
// `lab` (indexed through lix(x, y, z)), and the eight fine cells, low corner (i, j, kk) of component `b` of the child block that holds them
template <class Ix>
__device__ __forceinline__ void refine_cell(const double *lab, Ix lix, int x, int y, int z, double *b, int i, int j, int kk) {
#define Lb(a, bb, cc) lab[lix(x + (a), y + (bb), z + (cc))]
  const double dudx = 0.5 * (Lb(1, 0, 0) - Lb(-1, 0, 0));
  const double dudy = 0.5 * (Lb(0, 1, 0) - Lb(0, -1, 0));
  const double dudz = 0.5 * (Lb(0, 0, 1) - Lb(0, 0, -1));
  const double dudx2 = (Lb(1, 0, 0) + Lb(-1, 0, 0)) - 2.0 * Lb(0, 0, 0);
  const double dudy2 = (Lb(0, 1, 0) + Lb(0, -1, 0)) - 2.0 * Lb(0, 0, 0);
  const double dudz2 = (Lb(0, 0, 1) + Lb(0, 0, -1)) - 2.0 * Lb(0, 0, 0);
  const double dudxdy = 0.25 * ((Lb(1, 1, 0) + Lb(-1, -1, 0)) - (Lb(1, -1, 0) + Lb(-1, 1, 0)));
  const double dudxdz = 0.25 * ((Lb(1, 0, 1) + Lb(-1, 0, -1)) - (Lb(1, 0, -1) + Lb(-1, 0, 1)));
  const double dudydz = 0.25 * ((Lb(0, 1, 1) + Lb(0, -1, -1)) - (Lb(0, 1, -1) + Lb(0, -1, 1)));
  const double u = Lb(0, 0, 0), q2 = 0.03125 * (dudx2 + dudy2 + dudz2);
#undef Lb
#define B(a, bb, cc) b[((kk + (cc)) * 8 + (j + (bb))) * 8 + (i + (a))]
  B(0, 0, 0) = u + 0.25 * (-(1.0) * dudx - dudy - dudz) + q2 + 0.0625 * (dudxdy + dudxdz + dudydz);
  B(1, 0, 0) = u + 0.25 * (dudx - dudy - dudz) + q2 + 0.0625 * (-(1.0) * dudxdy - dudxdz + dudydz);
  B(0, 1, 0) = u + 0.25 * (-(1.0) * dudx + dudy - dudz) + q2 + 0.0625 * (-(1.0) * dudxdy + dudxdz - dudydz);
  B(1, 1, 0) = u + 0.25 * (dudx + dudy - dudz) + q2 + 0.0625 * (dudxdy - dudxdz - dudydz);
  B(0, 0, 1) = u + 0.25 * (-(1.0) * dudx - dudy + dudz) + q2 + 0.0625 * (dudxdy - dudxdz - dudydz);
  B(1, 0, 1) = u + 0.25 * (dudx - dudy + dudz) + q2 + 0.0625 * (-(1.0) * dudxdy + dudxdz - dudydz);
  B(0, 1, 1) = u + 0.25 * (-(1.0) * dudx + dudy + dudz) + q2 + 0.0625 * (-(1.0) * dudxdy - dudxdz + dudydz);
  B(1, 1, 1) = u + 0.25 * (dudx + dudy + dudz) + q2 + 0.0625 * (dudxdy + dudxdz + dudydz);
#undef B
}

// coarse cell (cx,cy,cz) <- mean of the 2x2x2 fine cells of child (cx>>2, cy>>2, cz>>2)
__global__ void __launch_bounds__(256) k_restrict(const double *__restrict__ fine, double *__restrict__ coarse, const int32_t *__restrict__ child,
                                                  int nc) {
  const int pb = blockIdx.x, t = threadIdx.x;
  for (int k = 0; k < 2; ++k) {
    const int cell = k * 256 + t, cx = cell & 7, cy = (cell >> 3) & 7, cz = cell >> 6;
    const int fs = child[pb * 8 + (cz >> 2) * 4 + (cy >> 2) * 2 + (cx >> 2)];
    const int i = 2 * (cx & 3), j = 2 * (cy & 3), kk = 2 * (cz & 3);
    for (int c = 0; c < nc; ++c) coarse[((size_t)pb * nc + c) * 512 + cell] = compress8(fine + ((size_t)fs * nc + c) * 512, i, j, kk);
  }
}

__device__ __forceinline__ int lix10(int x, int y, int z) { return ((z + 1) * 10 + (y + 1)) * 10 + (x + 1); }  // k_prolong's [10][10][10] tile

// one workgroup per coarse block; NC components staged as [NC][10][10][10] in LDS
template <int NC>
__global__ void __launch_bounds__(256) k_prolong(const double *__restrict__ coarse, double *__restrict__ fine, const int32_t *__restrict__ nbr27,
                                                 const int32_t *__restrict__ nbr6, const int32_t *__restrict__ child) {
  __shared__ double lab[NC * 1000];
  const int pb = blockIdx.x, t = threadIdx.x;
  // 1. centre + the 26 neighbours that BlockLab::load copies (3690-3725); skipped regions start at 0
  for (int e = t; e < 1000; e += 256) {
    const int lx = e % 10 - 1, ly = (e / 10) % 10 - 1, lz = e / 100 - 1;
    const int cx = lx < 0 ? -1 : (lx > 7 ? 1 : 0), cy = ly < 0 ? -1 : (ly > 7 ? 1 : 0), cz = lz < 0 ? -1 : (lz > 7 ? 1 : 0);
    const int n = nbr27[pb * 27 + (cx + 1) + 3 * (cy + 1) + 9 * (cz + 1)];
    const int cell = ((lz - 8 * cz) * 8 + (ly - 8 * cy)) * 8 + (lx - 8 * cx);
#pragma unroll
    for (int c = 0; c < NC; ++c) lab[c * 1000 + e] = n >= 0 ? coarse[((size_t)n * NC + c) * 512 + cell] : 0.0;
  }
  __syncthreads();
  // 2. domain faces in the reference's order x-,x+,y-,y+,z-,z+ (6513-6551 / 6561-6581): the whole ghost
  //    slab behind the face, edge strips included, from the face cell with the same transverse coordinates
  for (int f = 0; f < 6; ++f) {
    const int n = nbr6[pb * 6 + f];  // < 0: domain face, boundary condition -1-n
    if (n < 0) {
      const int d = f >> 1, side = f & 1, ghost = side ? 8 : -1, face = side ? 7 : 0, d1 = (d + 1) % 3, d2 = (d + 2) % 3;
      if (t < 100) {
        int p[3], q[3];
        p[d] = ghost; q[d] = face;
        p[d1] = q[d1] = t % 10 - 1;
        p[d2] = q[d2] = t / 10 - 1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          double v = lab[c * 1000 + lix10(q[0], q[1], q[2])];
          if (NC == 3 && (n == -3 || c == d)) v = -v;  // wall: all components; freespace: the normal one
          lab[c * 1000 + lix10(p[0], p[1], p[2])] = v;
        }
      }
      __syncthreads();
    }
  }
  // 3. RefineBlocks
  for (int k = 0; k < 2; ++k) {
    const int cell = k * 256 + t, x = cell & 7, y = (cell >> 3) & 7, z = cell >> 6;
    const int fs = child[pb * 8 + (z >> 2) * 4 + (y >> 2) * 2 + (x >> 2)];
    const int i = 2 * (x & 3), j = 2 * (y & 3), kk = 2 * (z & 3);
#pragma unroll
    for (int c = 0; c < NC; ++c) refine_cell(lab + c * 1000, lix10, x, y, z, fine + ((size_t)fs * NC + c) * 512, i, j, kk);
  }
}

// TagLoadedBlock: Linf of |magnitude| per block -> Refine (1) / Compress (-1) / Leave (0)
__global__ void __launch_bounds__(256) k_tag(const double *__restrict__ f, int nc, double rtol, double ctol, int clamp_refine, int clamp_compress,
                                             signed char *__restrict__ states) {
  __shared__ double red[4];
  const int b = blockIdx.x, t = threadIdx.x;
  double linf = 0.0;
  for (int k = 0; k < 2; ++k) {
    const int cell = k * 256 + t;
    double m;
    if (nc == 1) m = f[(size_t)b * 512 + cell];  // ScalarElement::magnitude, 5783
    else {
      double s1 = 0.0;
      for (int c = 0; c < nc; ++c) { const double u = f[((size_t)b * nc + c) * 512 + cell]; s1 += u * u; }
      m = sqrt(s1);  // VectorElement::magnitude, 5873-5879
    }
    linf = fmax(linf, fabs(m));
  }
  linf = wave_max(linf);
  if ((t & 63) == 0) red[t >> 6] = linf;
  __syncthreads();
  if (t == 0) {
    linf = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    signed char st = linf > rtol ? 1 : (linf < ctol ? -1 : 0);
    if (st == 1 && clamp_refine) st = 0;    // already at levelMax-1 (5207-5211)
    if (st == -1 && clamp_compress) st = 0; // already at level 0
    states[b] = st;
  }
}

static int child_table(const Sim *coarse, const Sim *fine, std::vector<int32_t> &tab) {
  const Grid *gc = coarse->grid, *gf = fine->grid;
  if (gc->multilevel || gf->multilevel) { set_error("restrict/prolong/tag operate on uniform levels (whole-mesh transitions)"); return CUP3D_EINVAL; }
  bool same = gc->level + 1 == gf->level && gc->level_max == gf->level_max;
  for (int d = 0; d < 3; ++d) same = same && gc->bpd[d] == gf->bpd[d] && gc->bc[d] == gf->bc[d];
  if (!same) { set_error("restrict/prolong need two sims of the same box at levels l and l+1"); return CUP3D_EINVAL; }
  tab.resize(8 * (size_t)coarse->nb);
  for (int64_t pb = 0; pb < coarse->nb; ++pb)
    for (int K = 0; K < 2; ++K)
      for (int J = 0; J < 2; ++J)
        for (int I = 0; I < 2; ++I) {
          const int32_t s = gf->slot_of_index(2 * gc->index[3 * pb] + I, 2 * gc->index[3 * pb + 1] + J, 2 * gc->index[3 * pb + 2] + K);
          if (s < 0) { set_error("a child block lives on another rank: partitions of the two levels are not aligned"); return CUP3D_ESTATE; }
          tab[8 * pb + K * 4 + J * 2 + I] = s;
        }
  return CUP3D_OK;
}

// ---- any old mesh to any new one: the eight children of a refined block.  One workgroup per refined parent builds the parent's tensorial
// [-1,2) tile on the OLD mesh in LDS exactly as BlockLab::load does (phases A-E at W = 1; a scalar is never negated at a domain
// face: bc_comp = -1), one component at a time, and expands it.
// items[n][9]: parent slot (old mesh), eight child slots (new mesh, child = I + 2J + 4K)
template <int NC>
__global__ void __launch_bounds__(256) k_refine(LabDev a, const int32_t *__restrict__ items, const double *__restrict__ src, double *__restrict__ dst) {
  constexpr int W = 1, nc = NC;
#define LABS_SLOT items[9 * blockIdx.x]
#include "labs_setup.hpp"
#undef LABS_SLOT
  for (int c = 0; c < nc; ++c) {
#include "labs_phases.hpp"  // through LABS_BLOCK / LABS_CELL of labs.hpp, which read `src` and `nc` of this scope
    for (int k = 0; k < 2; ++k) {
      const int cell = k * 256 + t, x = cell & 7, y = (cell >> 3) & 7, z = cell >> 6;
      const int fs = items[9 * blockIdx.x + 1 + (z >> 2) * 4 + (y >> 2) * 2 + (x >> 2)];
      const int i = 2 * (x & 3), j = 2 * (y & 3), kk = 2 * (z & 3);
      refine_cell(lab, lix, x, y, z, dst + ((size_t)fs * NC + c) * 512, i, j, kk);
    }
    __syncthreads();  // the next component reuses lab[]
  }
}

// unchanged blocks: copy; parents of compressed octets: compress -- pairs[n][2] = dst slot, src slot;
// octets[n][9] = dst slot, eight src slots (child = I + 2J + 4K)
__global__ void __launch_bounds__(256) k_copy_blocks(const int32_t *__restrict__ pairs, const double *__restrict__ src, double *__restrict__ dst, int nc) {
  const int d = pairs[2 * blockIdx.x], s = pairs[2 * blockIdx.x + 1];
  for (int i = threadIdx.x; i < 512 * nc; i += 256) dst[(size_t)d * 512 * nc + i] = src[(size_t)s * 512 * nc + i];
}
__global__ void __launch_bounds__(256) k_compress_blocks(const int32_t *__restrict__ octets, const double *__restrict__ src, double *__restrict__ dst, int nc) {
  const int pb = octets[9 * blockIdx.x], t = threadIdx.x;
  for (int k = 0; k < 2; ++k) {
    const int cell = k * 256 + t, cx = cell & 7, cy = (cell >> 3) & 7, cz = cell >> 6;
    const int fs = octets[9 * blockIdx.x + 1 + (cz >> 2) * 4 + (cy >> 2) * 2 + (cx >> 2)];
    const int i = 2 * (cx & 3), j = 2 * (cy & 3), kk = 2 * (cz & 3);
    for (int c = 0; c < nc; ++c) dst[((size_t)pb * nc + c) * 512 + cell] = compress8(src + ((size_t)fs * nc + c) * 512, i, j, kk);
  }
}

// The data movement of MeshAdaptation::Adapt, shared by the one-rank and the multi-rank entry points.
// `mo`: the OLD mesh as this rank sees it (a whole mesh, or a tensorial rank view whose ghost slots of `fs` hold the owners' data);
// `blocks`: the blocks to produce, each with the slot of `fd` it goes to.  A block is a leaf of the old mesh (copied), a child of
// one (refined) or the parent of an octet of them (compressed).
struct NewBlock { int level, idx[3]; int32_t dst; };
static int adapt_produce(const Grid *mo, const std::vector<NewBlock> &blocks, const double *fs, double *fd, int nc) {
  std::vector<int32_t> pairs, octets, items;
  try {
    std::vector<int32_t> item_of((size_t)mo->Z.size(), -1);
    for (const NewBlock &nbk : blocks) {
      const int l = nbk.level;
      const int *idx = nbk.idx;
      const int32_t same = mo->leaf(l, idx);
      if (same >= 0) { pairs.push_back(nbk.dst); pairs.push_back(same); continue; }
      const int pidx[3] = {idx[0] >> 1, idx[1] >> 1, idx[2] >> 1};
      const int32_t par = l > 0 ? mo->leaf(l - 1, pidx) : -1;
      if (par >= 0) {
        if (par >= mo->nblocks()) throw std::invalid_argument("a refined block is not local to the rank that has to refine it");
        if (item_of[par] < 0) {
          item_of[par] = (int32_t)(items.size() / 9);
          items.push_back(par);
          for (int q = 0; q < 8; ++q) items.push_back(-1);
        }
        items[9 * (size_t)item_of[par] + 1 + (idx[0] & 1) + 2 * (idx[1] & 1) + 4 * (idx[2] & 1)] = nbk.dst;
        continue;
      }
      octets.push_back(nbk.dst);
      for (int q = 0; q < 8; ++q) {
        const int ci[3] = {2 * idx[0] + (q & 1), 2 * idx[1] + ((q >> 1) & 1), 2 * idx[2] + (q >> 2)};
        const int32_t cb = l + 1 < mo->level_max ? mo->leaf(l + 1, ci) : -1;
        if (cb < 0) throw std::invalid_argument("a block of the new mesh is neither a block, a child nor the parent of blocks of the old mesh");
        octets.push_back(cb);
      }
    }
    // children of one parent are produced together or not at all on one rank; slots that stay -1 are children another rank's
    // list holds -- impossible, since all eight go where the parent is refined
    for (size_t i = 0; i < items.size(); ++i)
      if (items[i] < 0) throw std::invalid_argument("a refined block lacks some of its children in the new mesh");
  } catch (const std::exception &e) {
    set_error("mesh adaptation: %s", e.what());
    return CUP3D_EINVAL;
  }
  LabIndex tab;
  Dev<int32_t> d_pairs, d_octets, d_items;
  int rc;
  if (!items.empty()) {
    if ((rc = tab.build(mo, mo->nblocks(), "mesh adaptation"))) return rc;
    // phase A of k_refine averages down every finer leaf behind a refined parent: entry [code][octant] of the parent's row is read
    // unless the octant is an upper one along an axis the code leaves the block by
    for (size_t it = 0; it < items.size(); it += 9) {
      const int32_t pb = items[it], r = tab.h_finer_row[pb];
      for (int i = 0; r >= 0 && i < 216; ++i) {
        const int icode = i >> 3, q = i & 7;
        const bool read = !((q & 1) && icode % 3 != 1) && !((q & 2) && (icode / 3) % 3 != 1) && !((q & 4) && icode / 9 != 1);
        if (read && mo->nbr27[27 * (size_t)pb + icode] == kNbrFiner && tab.h_finer[216 * (size_t)r + i] < 0) {
          set_error("mesh adaptation: a finer neighbour of a refined block is not visible on this rank");
          return CUP3D_EINVAL;
        }
      }
    }
  }
  if ((rc = d_pairs.upload(pairs, stream(), IfEmpty::null)) || (rc = d_octets.upload(octets, stream(), IfEmpty::null)) || (rc = d_items.upload(items, stream(), IfEmpty::null))) return rc;
  ProfileScope ps("adapt_transfer");
  if (!pairs.empty()) hipLaunchKernelGGL(k_copy_blocks, dim3((unsigned)(pairs.size() / 2)), dim3(256), 0, stream(), d_pairs.get(), fs, fd, nc);
  if (!octets.empty()) hipLaunchKernelGGL(k_compress_blocks, dim3((unsigned)(octets.size() / 9)), dim3(256), 0, stream(), d_octets.get(), fs, fd, nc);
  if (!items.empty()) {
    const LabDev a = tab.dev(mo, -1);
    const unsigned n = (unsigned)(items.size() / 9);
    if (nc == 3) hipLaunchKernelGGL(k_refine<3>, dim3(n), dim3(256), 0, stream(), a, (const int32_t *)d_items, fs, fd);
    else hipLaunchKernelGGL(k_refine<1>, dim3(n), dim3(256), 0, stream(), a, (const int32_t *)d_items, fs, fd);
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipStreamSynchronize(stream()));  // the index tables above are freed on return
  return CUP3D_OK;
}

}  // namespace cup3d
using namespace cup3d;
extern "C" {

int cup3d_restrict(cup3d_sim_t *fine_h, cup3d_sim_t *coarse_h, int field) {
  if (!fine_h || !coarse_h) return CUP3D_EINVAL;
  Sim *fine = reinterpret_cast<Sim *>(fine_h), *coarse = reinterpret_cast<Sim *>(coarse_h);
  std::vector<int32_t> tab;
  int rc = child_table(coarse, fine, tab), nc, nc2;
  if (rc) return rc;
  const double *src = fine->field(field, &nc);
  double *dst = coarse->field(field, &nc2);
  if (!src || !dst) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
  Dev<int32_t> d_tab;
  if ((rc = d_tab.upload(tab, IfEmpty::null))) return rc;
  {
    ProfileScope ps("restrict_blocks");
    hipLaunchKernelGGL(k_restrict, dim3((unsigned)coarse->nb), dim3(256), 0, stream(), src, dst, d_tab.get(), nc);
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipStreamSynchronize(stream()));  // the table is freed on return
  return CUP3D_OK;
}

int cup3d_prolong(cup3d_sim_t *coarse_h, cup3d_sim_t *fine_h, int field) {
  if (!fine_h || !coarse_h) return CUP3D_EINVAL;
  Sim *fine = reinterpret_cast<Sim *>(fine_h), *coarse = reinterpret_cast<Sim *>(coarse_h);
  std::vector<int32_t> tab;
  int rc = child_table(coarse, fine, tab), nc, nc2;
  if (rc) return rc;
  const double *src = coarse->field(field, &nc);
  double *dst = fine->field(field, &nc2);
  if (!src || !dst) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
  std::vector<int32_t> n27 = coarse->grid->neighbours27();
  for (int32_t v : n27)
    if (v == -2) { set_error("cup3d_prolong: a neighbour block lives on another rank (multi-rank mesh adaptation is not wired yet)"); return CUP3D_ESTATE; }
  Dev<int32_t> d_tab, d_n27;
  if ((rc = d_tab.upload(tab, IfEmpty::null)) || (rc = d_n27.upload(n27, IfEmpty::null))) return rc;
  {
    ProfileScope ps("prolong_blocks");
    if (nc == 3) hipLaunchKernelGGL(k_prolong<3>, dim3((unsigned)coarse->nb), dim3(256), 0, stream(), src, dst, d_n27.get(), coarse->d_nbr.get(), d_tab.get());
    else hipLaunchKernelGGL(k_prolong<1>, dim3((unsigned)coarse->nb), dim3(256), 0, stream(), src, dst, d_n27.get(), coarse->d_nbr.get(), d_tab.get());
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipStreamSynchronize(stream()));  // the tables are freed on return
  return CUP3D_OK;
}

int cup3d_tag_blocks(cup3d_sim_t *h, int field, double rtol, double ctol, signed char *states) {
  if (!h || !states) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  int nc;
  const double *f = s->field(field, &nc);
  if (!f) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
  const Grid *gr = s->grid;
  Dev<signed char> d_states;
  int rc = d_states.alloc((size_t)s->nb);
  if (rc) return rc;
  {
    ProfileScope ps("tag_blocks");
    // multi-level meshes: the level clamps differ per block and are applied on the host below
    hipLaunchKernelGGL(k_tag, dim3((unsigned)s->nb), dim3(256), 0, stream(), f, nc, rtol, ctol,
                       (!gr->multilevel && gr->level == gr->level_max - 1) ? 1 : 0, (!gr->multilevel && gr->level == 0) ? 1 : 0, d_states.get());
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipMemcpyAsync(states, d_states, (size_t)s->nb, hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipStreamSynchronize(stream()));
  if (gr->multilevel)
    for (int64_t b = 0; b < s->nb; ++b) {  // TagBlocksVector, main.cpp:5207-5211
      if (states[b] == 1 && gr->blevel[b] == gr->level_max - 1) states[b] = 0;
      if (states[b] == -1 && gr->blevel[b] == 0) states[b] = 0;
    }
  return CUP3D_OK;
}

int cup3d_adapt_transfer(cup3d_sim_t *src_h, cup3d_sim_t *dst_h, int field) {
  if (!src_h || !dst_h) return CUP3D_EINVAL;
  Sim *src = reinterpret_cast<Sim *>(src_h), *dst = reinterpret_cast<Sim *>(dst_h);
  int nc, nc2;
  const double *fs = src->field(field, &nc);
  double *fd = dst->field(field, &nc2);
  if (!fs || !fd) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
  if (src->grid->n_local >= 0 || dst->grid->n_local >= 0) { set_error("cup3d_adapt_transfer: meshes spread over ranks go through cup3d_adapt_migrate"); return CUP3D_EINVAL; }
  MeshOf old_mesh, new_mesh;
  const Grid *mo = old_mesh.get(src->grid, "cup3d_adapt_transfer"), *mn = mo ? new_mesh.get(dst->grid, "cup3d_adapt_transfer") : nullptr;
  if (!mn) return CUP3D_EINVAL;
  for (int d = 0; d < 3; ++d)
    if (mo->bpd[d] != mn->bpd[d] || mo->bc[d] != mn->bc[d] || mo->level_max != mn->level_max) { set_error("cup3d_adapt_transfer: the two meshes belong to different boxes"); return CUP3D_EINVAL; }
  std::vector<NewBlock> blocks((size_t)mn->nblocks());
  for (int64_t b = 0; b < mn->nblocks(); ++b)
    blocks[b] = NewBlock{mn->blevel[b], {mn->index[3 * b], mn->index[3 * b + 1], mn->index[3 * b + 2]}, (int32_t)b};
  return adapt_produce(mo, blocks, fs, fd, nc);
}

// ---- the same over ranks: MeshAdaptation::Adapt + the block traffic of the LoadBalancer (PrepareCompression 4729-4804, Balance_Diffusion
// 4805-4905, Balance_Global 4906-5021).  The reference refines where the parent lives, gathers an octet on the rank of its base block,
// compresses there, then ships whole blocks to even out the load; the END STATE -- every block of the adapted mesh, filled from the old
// mesh's data, on the rank cup3d_grid_adapted_owners names -- is produced here in one hop: the rank that owns the ORIGIN of a new block
// (the leaf itself, the refined parent, or the base block of the octet) builds it from its tensorial view of the old mesh and sends it
// straight to the new owner.  Refinement and compression are block-local operations on identical inputs, so the fields equal the
// one-rank adaptation bit for bit, wherever the blocks end up.
int cup3d_adapt_migrate(const cup3d_grid_t *old_mesh_h, const int32_t *old_owner, cup3d_sim_t *src_h, const cup3d_grid_t *new_mesh_h,
                        const int32_t *new_owner, cup3d_sim_t *dst_h, int field) {
  if (!src_h || !dst_h) return CUP3D_EINVAL;  // (without the sims there is no communicator to tell the other ranks through)
  Sim *src = reinterpret_cast<Sim *>(src_h), *dst = reinterpret_cast<Sim *>(dst_h);
  const Grid *om = reinterpret_cast<const Grid *>(old_mesh_h), *nm = reinterpret_cast<const Grid *>(new_mesh_h);
  const int me = src->grid->rank, nranks = src->grid->nranks;
  int nc = 0, nc2 = 0;
  const double *fs = nullptr;
  double *fd = nullptr;
  ViewField old;                            // the old field on this rank's tensorial view of the old mesh
  std::vector<NewBlock> mine;               // what this rank produces, ordered by (consumer, new global slot)
  std::vector<int64_t> send_count(nranks, 0), recv_count(nranks, 0);
  std::vector<int32_t> recv_slots;          // local slots of dst in arrival order: by (producer, new global slot)
  Dev<double> prod, recv;
  Dev<int32_t> d_recv_slots;
  // everything this rank can get wrong on its own -- arguments, the plan, allocations -- happens in here; the ranks then agree on the
  // outcome BEFORE the first exchange, so that a bad call on one rank returns an error on every rank instead of blocking the others
  auto local_part = [&]() -> int {
    if (!old_mesh_h || !old_owner || !new_mesh_h || !new_owner) { set_error("cup3d_adapt_migrate: null argument"); return CUP3D_EINVAL; }
    fs = src->field(field, &nc);
    fd = dst->field(field, &nc2);
    if (!fs || !fd) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
    if (!om->multilevel || !nm->multilevel || om->n_local >= 0 || nm->n_local >= 0) { set_error("cup3d_adapt_migrate needs the two GLOBAL mesh objects"); return CUP3D_EINVAL; }
    if (dst->grid->rank != me || dst->grid->nranks != nranks) { set_error("cup3d_adapt_migrate: the two sims belong to different ranks"); return CUP3D_EINVAL; }
    auto plan = [&] {
      std::vector<std::vector<NewBlock>> by_consumer(nranks);
      std::vector<std::vector<int32_t>> by_producer(nranks);
      int32_t my_slot = 0;
      for (int64_t b = 0; b < nm->nblocks(); ++b) {
        const int l = nm->blevel[b];
        const int idx[3] = {nm->index[3 * b], nm->index[3 * b + 1], nm->index[3 * b + 2]};
        int32_t origin = om->leaf(l, idx);
        if (origin < 0 && l > 0) { const int pi[3] = {idx[0] >> 1, idx[1] >> 1, idx[2] >> 1}; origin = om->leaf(l - 1, pi); }
        if (origin < 0 && l + 1 < om->level_max) { const int ci[3] = {2 * idx[0], 2 * idx[1], 2 * idx[2]}; origin = om->leaf(l + 1, ci); }
        if (origin < 0) throw std::invalid_argument("a block of the new mesh is neither a block, a child nor the parent of blocks of the old mesh");
        const int producer = old_owner[origin], consumer = new_owner[b];
        if (producer < 0 || producer >= nranks || consumer < 0 || consumer >= nranks) throw std::invalid_argument("owner out of range");
        if (producer == me) by_consumer[consumer].push_back(NewBlock{l, {idx[0], idx[1], idx[2]}, 0});
        if (consumer == me) by_producer[producer].push_back(my_slot++);
      }
      if (my_slot != dst->nb) throw std::invalid_argument("the destination sim does not hold this rank's blocks of the new mesh");
      for (int p = 0; p < nranks; ++p) {
        send_count[p] = (int64_t)by_consumer[p].size();
        recv_count[p] = (int64_t)by_producer[p].size();
        for (NewBlock &nbk : by_consumer[p]) { nbk.dst = (int32_t)mine.size(); mine.push_back(nbk); }
        recv_slots.insert(recv_slots.end(), by_producer[p].begin(), by_producer[p].end());
      }
    };
    int rc = old.stage(om, old_owner, src, fs, nc, "cup3d_adapt_migrate", "the source sim does not hold this rank's blocks of the old mesh", plan);
    if (rc || (rc = prod.alloc(std::max<size_t>(mine.size(), 1) * old.per)) || (rc = recv.alloc(std::max<size_t>(recv_slots.size(), 1) * old.per))) return rc;
    return CUP3D_OK;
  };
  int rc = agree(src, local_part(), "cup3d_adapt_migrate");
  if (rc) return rc;
  if ((rc = old.exchange(src))) return rc;
  // producing the new blocks is rank-local again (kernels, table uploads): agree once more before they travel
  if ((rc = agree(src, adapt_produce(old.tv.get(), mine, old.F, prod, nc), "cup3d_adapt_migrate (produce)"))) return rc;
  if ((rc = exchange_items(src, prod, send_count, recv, recv_count, old.per))) return rc;
  if (!recv_slots.empty()) {
    if ((rc = d_recv_slots.upload(recv_slots, stream(), IfEmpty::null))) return rc;
    if ((rc = launch_unpack_blocks(recv, d_recv_slots, nc, fd, (unsigned)recv_slots.size(), stream()))) return rc;
  }
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return CUP3D_OK;
}

}  // extern "C"
