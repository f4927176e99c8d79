// ==== Ghosted block tiles: BlockLab::load + post_load (main.cpp:3623-3787) for one block, ONE implementation for every consumer of a
// tensorial (or star) tile: cup3d_sim_labs / cup3d_sim_labs_device (k_labs, labs.hip), cup3d_sim_labs_over_ranks (k_labs_view,
// labs.hip), the refinement of mesh adaptation (k_refine, adapt.hip: the [-1,2) tile) and GradChiOnTmp (k_grad_chi, grad_chi.hip: the
// [-2,3) tile).  It uses the device helpers of amr_interp.hpp -- avg_down8 / avg_block, fd_mode_av / fd_mode_blend (with interp1d),
// test_interp -- so a bit-exactness fix to the reference's ghost rules lands once.  (k_ghosts, amr.hip, builds star slabs in another
// shape, for the solver's hot path, and stays on its own.)  Here: what those kernels and their host sides share.
//
// The stencil kernels build the three tile shapes they need in LDS and never hand them out; this is the general operation for a
// consumer OUTSIDE the library (the kernel-functor protocol of compute<Lab>): block b with its ghosts for the box [-w, w+1)^3,
// w = 1..4, star or tensorial, in the reference's Matrix3D layout [L][L][L][nc] (x fastest, component innermost, L = 8 + 2w).
// One workgroup per tile, one component at a time in LDS (16^3 fine cells + the 10^3 coarse shadow tile = 40 768 B), in the
// reference's order:
//   A. interior copy, SameLevelExchange (3823-3876), FineToCoarseExchange = AverageDown of the finer leaves (3907-4065);
//   B. the coarse shadow tile m_CoarsenedBlock: coarser leaves copied (CoarseFineExchange 4066-4170), same-level neighbours
//      averaged down (FillCoarseVersion 4171-4235; every one of them -- the cells the UseCoarseStencil rule 3788-3822 would leave
//      out are read by no interpolation: tests/test_gpu_labs.py::test_tiles_equal_the_reference, the reference's own tiles on four
//      meshes, is the test that a violation would turn red), the block's own average-down (post_load 3750-3778);
//   C. _apply_bc on the coarse tile (3781): ordered passes x, y, z, each over the whole ghost slab;
//   D. CoarseFineInterpolation (4236-4614): TestInterp everywhere behind a coarser neighbour, then the finite-difference mode with
//      the 1/15 blend on the two layers next to a FACE (it overwrites TestInterp there, as in the reference);
//   E. _apply_bc on the fine tile: ordered passes x, y, z, each over the whole ghost slab, transverse ghosts of earlier passes included;
//   F. the cells the reference leaves undefined -- edge and corner ghosts of a star tile with w <= 2, where use_averages (3618-3621)
//      does not hold -- leave as quiet NaN, so that a consumer that reads them sees it.
// A tile with w >= 3 is built tensorially by the reference whatever the stencil says (use_averages), so `tensorial` only decides F.
// The kernels read blocks only: they neither need nor touch the ghost slabs the stencil kernels keep behind kNbrHalo.
#pragma once
#include <stdexcept>
#include <utility>
#include "amr_interp.hpp"
#include "sim.hpp"

namespace cup3d {

struct LabDev {
  const int32_t *n27;        // [nb][27]
  const int32_t *index;      // [nb][3]
  const int32_t *level;      // [nb]
  const int32_t *finer_row;  // [nb]: row of `finer`, or -1
  const int32_t *finer;      // [rows][27][8]
  int bpd[3], bc[3];
  int bc_comp;  // scalar fields: -1 = zero-gradient domain faces (ScalarLab); k = element of BlockLabBC<.., direction k>
};

constexpr int kLabCoarse = 10;  // coarse shadow tile: coarse cells [-3, 7)^3 (w = 4 reads [-3, 6])
__device__ __forceinline__ int cix10(int X, int Y, int Z) { return ((Z + 3) * kLabCoarse + (Y + 3)) * kLabCoarse + (X + 3); }

// domain-face rule of one tile value: the vector lab negates every component at a wall and the normal one at a freespace face
// (6107-6503), the scalar lab copies (6561-6581), the scalar of BlockLabBC<.., direction k> behaves as component k of a vector
__device__ __forceinline__ double lab_bc_value(double v, int nc, int c, int bc_comp, int bc_kind, int d) {
  const int cc = nc == 3 ? c : bc_comp;
  return (cc >= 0 && (bc_kind == CUP3D_BC_WALL || cc == d)) ? -v : v;
}

// The set-up (labs_setup.hpp) and phases A-E for one component (labs_phases.hpp) live once and are included as text into the four
// kernels, which differ in where the blocks of a tile's neighbourhood live and in what they do with the finished tile.  k_labs, one
// rank: every slot is a row of the field array `src` of `nc` components; phase F stores the tile.  k_refine and k_grad_chi read such
// rows too and keep the tile in LDS for their operator: that block source is the one defined here.  k_labs_view, a mesh spread over
// ranks, replaces it with its own (LabSrcView, labs.hip).
#define LABS_BLOCK(slot, c) (src + ((size_t)(slot) * nc + (c)) * 512)
#define LABS_CELL(slot, c, i) src[((size_t)(slot) * nc + (c)) * 512 + (i)]

// The finer leaves behind every kNbrFiner position of the blocks [0, nloc) of `mo`, by octant of the block (bits of x, y, z >= 4):
// finer_row[b] = the block's row of finer[rows][27][8] (-1: no finer neighbour), -1 in the row where nothing is read.  Throws what Grid::leaf throws.
void finer_tables(const Grid *mo, int64_t nloc, std::vector<int32_t> &finer_row, std::vector<int32_t> &finer);

// The five index tables of a LabDev on the device, for the blocks [0, nloc) of `mo` (a multi-level mesh object: the mesh itself on one
// rank, a rank's tensorial view over ranks).  One owner for the four users: cup3d_sim_labs and cup3d_sim_labs_over_ranks keep theirs in
// the sim, mesh adaptation and GradChiOnTmp build one per call and let it go after their stream synchronise.
struct LabIndex {
  Dev<int32_t> n27, index, level, finer_row, finer;
  std::vector<int32_t> h_finer_row, h_finer;  // the two tables `mo` does not hold, on the host
  size_t bytes = 0;                           // of the five tables
  int build(const Grid *mo, int64_t nloc, const char *who) {
    try {
      finer_tables(mo, nloc, h_finer_row, h_finer);
    } catch (const std::exception &e) {
      set_error("%s: %s", who, e.what());
      return CUP3D_EINVAL;
    }
    const std::pair<Dev<int32_t> *, const std::vector<int32_t> *> tables[] = {{&n27, &mo->nbr27}, {&index, &mo->index}, {&level, &mo->blevel}, {&finer_row, &h_finer_row}, {&finer, &h_finer}};
    for (const auto &[d, v] : tables) {
      int rc = d->upload(*v, IfEmpty::one);
      if (rc) return rc;
      bytes += v->size() * sizeof(int32_t);
    }
    return CUP3D_OK;
  }
  // box and boundary conditions come from `g`: the sim's grid, or the mesh object itself
  LabDev dev(const Grid *g, int bc_comp) const {
    return LabDev{n27, index, level, finer_row, finer, {g->bpd[0], g->bpd[1], g->bpd[2]}, {g->bc[0], g->bc[1], g->bc[2]}, bc_comp};
  }
};

}  // namespace cup3d
