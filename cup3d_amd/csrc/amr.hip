// Multi-level (AMR) meshes on the device: ghost reconstruction at coarse/fine faces and flux correction.
//
// The stencil kernels never see the mesh hierarchy.  Before a kernel runs, two small kernels write, for every
// interface face (a face whose same-level neighbour does not exist), the ghost slab the kernel will read -- in
// the same slab format and through the same `nbr >= kNbrHalo` indirection as the RCCL halo slabs of a
// multi-rank run:
//   * neighbour finer  -> "restrict": 8-cell AverageDown of the fine leaves (BlockLab::FineToCoarseExchange,
//     main.cpp:3907-4065, AverageDown 3877-3882);
//   * neighbour coarser -> "prolong": BlockLab::CoarseFineInterpolation (4236-4614).  Only what a star-shaped
//     stencil reads is built: layers 1-2 behind the face use the finite-difference mode (1-D quadratic
//     interpolation along both tangential axes + mixed term on the coarse layer next to the face, blended with
//     two own cells, 4374-4612); layer 3 (stencil [-3,4) only) uses TestInterp (3883-3906) on the 3x3x3 coarse
//     neighbourhood, which needs the coarse shadow tile (m_CoarsenedBlock) behind the face including its
//     tangential ghosts: coarser leaves copied (CoarseFineExchange 4066-4170), same-level neighbours averaged
//     down (FillCoarseVersion 4171-4235), domain faces mirrored (_apply_bc on the coarse tile, 3781).
// After the kernel, k_flux_fix applies FluxCorrectionMPI::FillBlockCases (2825-2935) to the coarse side.
// All arithmetic keeps the reference's association (-ffp-contract=off): results are bit-identical to it.
#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <utility>

#include "sim.hpp"
#include "tile.hpp"

namespace cup3d {

struct AmrDev {
  const int32_t *faces;  // [ne][2]: 6*slot + face, kind
  const int32_t *fine;   // [ne][4]
  const int32_t *nbr27;  // [nb][27]
  const int32_t *nbr;    // [nb][6]
  const int32_t *index;  // [nb][3]
  int bc_comp;           // scalar fields: -1 = zero-gradient domain faces (BlockLabNeumann3D); k = element of BlockLabBC<.., direction k>
};

__device__ __forceinline__ double avg_down8(const double v[8]) {  // AverageDown, main.cpp:3877-3882
  return 0.125 * (v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6] + v[7]);
}
// the 2x2x2 cells with low corner (x,y,z) of a block component, in AverageDown's argument order (x slowest)
__device__ __forceinline__ double avg_block(const double *__restrict__ blk, int x, int y, int z) {
  double v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = blk[(z + (q & 1)) * 64 + (y + ((q >> 1) & 1)) * 8 + (x + (q >> 2))];
  return avg_down8(v);
}

// ---- neighbour finer: slab[(e*nc + c)*W + gl][a2*8 + a1]
template <int W>
__device__ __forceinline__ void ghost_restrict_face(const AmrDev &a, int e, const double *__restrict__ field, int nc,
                                                       double *__restrict__ slabs) {
  const int lane = threadIdx.x;
  const int sf = a.faces[2 * e], f = sf % 6, d = f >> 1, side = f & 1;
  const int a1 = lane & 7, a2 = lane >> 3;
  const int fe = a.fine[4 * e + (a1 >> 2) + 2 * (a2 >> 2)];
  const int fslot = a.faces[2 * fe] / 6;
  const int t1 = 2 * (a1 & 3), t2 = 2 * (a2 & 3);
  for (int c = 0; c < nc; ++c) {
    const double *__restrict__ blk = field + ((size_t)fslot * nc + c) * 512;
#pragma unroll
    for (int gl = 0; gl < W; ++gl) {
      const int n0 = side ? 2 * gl : 6 - 2 * gl;
      const int x = d == 0 ? n0 : t1, y = d == 1 ? n0 : (d == 0 ? t1 : t2), z = d == 2 ? n0 : t2;
      slabs[(((size_t)e * nc + c) * W + gl) * 64 + lane] = avg_block(blk, x, y, z);
    }
  }
}

// ---- neighbour coarser
__constant__ double kCoefPlus[9] = {-0.09375, 0.4375, 0.15625, 0.15625, -0.5625, 0.90625, -0.09375, 0.4375, 0.15625};   // d_coef_plus, 3485-3486
__constant__ double kCoefMinus[9] = {0.15625, -0.5625, 0.90625, -0.09375, 0.4375, 0.15625, 0.15625, 0.4375, -0.09375};  // d_coef_minus, 3487-3488

// 1-D quadratic interpolation at coarse position p (0..3) along one tangential axis of the 6x6 patch layer
// (stride `st` between neighbours along that axis), main.cpp:4419-4441; pm = positions used by the mixed term
__device__ __forceinline__ double interp1d(const double *__restrict__ P0, int p, int st, const double *__restrict__ coef, int &pp, int &pm) {
  if (p != 0 && p != 3) {
    pp = p + 1; pm = p - 1;
    return (coef[6] * P0[-st] + coef[8] * P0[st]) + coef[7] * P0[0];
  } else if (p == 0) {
    pp = p + 1; pm = p;
    return (coef[0] * P0[2 * st] + coef[1] * P0[st]) + coef[2] * P0[0];
  }
  pp = p; pm = p - 1;
  return (coef[3] * P0[-2 * st] + coef[4] * P0[-st]) + coef[5] * P0[0];
}

// CoarseFineInterpolation, finite-difference mode (main.cpp:4419-4600): the coarse-side value `av` of a fine ghost cell -- the two 1-D
// quadratic interpolations along the face's tangential axes plus the mixed term -- from the coarse layer behind the face.  P0 = the coarse
// cell that holds the ghost cell, (p1, p2) its tangential position (0..3), st1 / st2 the strides of the layer along the two axes, bit1 /
// bit2 which child of the coarse cell the ghost cell is.  ONE definition for the two callers (the ghost slabs of the star stencils,
// ghost_prolong_face; phase D of the ghosted tiles, labs_phases.hpp): a bit-exactness fix lands once.
__device__ __forceinline__ double fd_mode_av(const double *__restrict__ P0, int p1, int p2, int st1, int st2, int bit1, int bit2) {
  const double dd1 = 0.25 * (2 * bit1 - 1), dd2 = 0.25 * (2 * bit2 - 1);
  const double *coef1 = dd1 > 0 ? kCoefPlus : kCoefMinus, *coef2 = dd2 > 0 ? kCoefPlus : kCoefMinus;
  int pp1, pm1, pp2, pm2;
  const double x1D = interp1d(P0, p1, st1, coef1, pp1, pm1);
  const double x2D = interp1d(P0, p2, st2, coef2, pp2, pm2);
  double mixed_coef = 1.0;
  if (p1 != 0 && p1 != 3) mixed_coef *= 0.5;
  if (p2 != 0 && p2 != 3) mixed_coef *= 0.5;
#define PC(i, j) P0[((i) - p1) * st1 + ((j) - p2) * st2]
  const double mixed = mixed_coef * dd1 * dd2 * ((PC(pm1, pm2) + PC(pp1, pp2)) - (PC(pp1, pm2) + PC(pm1, pp2)));
#undef PC
  return (x1D + x2D) + mixed;
}
// ... blended with the block's own two cells behind the face (bv: the face cell, cv: the one behind it), main.cpp:4601-4608
__device__ __forceinline__ double fd_mode_blend(double av, double bv, double cv, int layer) {
  return layer == 0 ? (1.0 / 15.0) * (8.0 * av + (10.0 * bv - 3.0 * cv)) : (1.0 / 15.0) * (24.0 * av + (-15.0 * bv + 6 * cv));
}
// TestInterp (main.cpp:3883-3906): second-order Taylor expansion around a coarse cell; Cc(i, j, k) = the 3x3x3 coarse cells around it
// (1, 1, 1 = the cell itself), bit[d] = which child along d
template <class F>
__device__ __forceinline__ double test_interp(F Cc, const int (&bit)[3]) {
  const double dudx = 0.125 * (Cc(2, 1, 1) - Cc(0, 1, 1));
  const double dudy = 0.125 * (Cc(1, 2, 1) - Cc(1, 0, 1));
  const double dudz = 0.125 * (Cc(1, 1, 2) - Cc(1, 1, 0));
  const double dudxdy = 0.015625 * (Cc(0, 0, 1) + Cc(2, 2, 1) - Cc(2, 0, 1) - Cc(0, 2, 1));
  const double dudxdz = 0.015625 * (Cc(0, 1, 0) + Cc(2, 1, 2) - Cc(2, 1, 0) - Cc(0, 1, 2));
  const double dudydz = 0.015625 * (Cc(1, 0, 0) + Cc(1, 2, 2) - Cc(1, 2, 0) - Cc(1, 0, 2));
  const double lap = Cc(1, 1, 1) + 0.03125 * (Cc(0, 1, 1) + Cc(2, 1, 1) + Cc(1, 0, 1) + Cc(1, 2, 1) + Cc(1, 1, 0) + Cc(1, 1, 2) + (-6.0) * Cc(1, 1, 1));
  const double sx = bit[0] ? 1.0 : -1.0, sy = bit[1] ? 1.0 : -1.0, sz = bit[2] ? 1.0 : -1.0;
  return lap + sx * dudx + sy * dudy + sz * dudz + (sx * sy) * dudxdy + (sx * sz) * dudxdz + (sy * sz) * dudydz;
}

template <int W>
__device__ __forceinline__ void ghost_prolong_face(const AmrDev &a, int e, const double *__restrict__ field, int nc,
                                                      double *__restrict__ slabs) {
  __shared__ double patch[W][36];  // coarse shadow tile behind the face: [layer][(Z+1)*6 + (Y+1)], Y/Z in [-1,4] along (a1,a2)
  const int lane = threadIdx.x;
  const int sf = a.faces[2 * e], slot = sf / 6, f = sf % 6, ax = f >> 1, side = f & 1;
  const int ax1 = ax == 0 ? 1 : 0, ax2 = ax == 2 ? 1 : 2;  // tangential axes (fast, slow) = the reference's (y,z)/(x,z)/(x,y)
  const int par[3] = {a.index[3 * slot] & 1, a.index[3 * slot + 1] & 1, a.index[3 * slot + 2] & 1};
  const bool is_vector = nc == 3;
  const int a1i = lane & 7, a2i = lane >> 3;
  for (int c = 0; c < nc; ++c) {
    __syncthreads();
    // ---- coarse shadow values
    for (int i = lane; i < W * 36; i += 64) {
      const int L = i / 36, r = i - 36 * L;
      int P[3], code[3];
      P[ax] = side ? 4 + L : -1 - L;
      P[ax1] = r % 6 - 1;
      P[ax2] = r / 6 - 1;
      code[ax] = side ? 1 : -1;
      bool flip = false;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int t = k ? ax2 : ax1;
        int rg = P[t] < 0 ? -1 : (P[t] > 3 ? 1 : 0);
        if (rg != 0) {
          const int n = a.nbr[slot * 6 + 2 * t + (rg > 0)];
          if (n < 0) {  // domain face: _apply_bc on the coarse tile copies the face cell with the same transverse coordinates
            P[t] = rg < 0 ? 0 : 3;
            rg = 0;
            // wall: all components; freespace: the normal one.  A scalar of BlockLabBC<ScalarGrid, .., direction> (the Helmholtz
            // solves of the implicit diffusion, main.cpp:6853-6862) behaves as component `direction` of a vector
            const int cc = is_vector ? c : a.bc_comp;
            if ((is_vector || a.bc_comp >= 0) && (n == -3 || cc == t)) flip = !flip;
          }
        }
        code[t] = rg;
      }
      const int v = a.nbr27[slot * 27 + (code[0] + 1) + 3 * (code[1] + 1) + 9 * (code[2] + 1)];
      double val = 0.0;
      if (v >= kNbrCoarser) {  // CoarseFineExchange: cell of the coarser leaf
        const double *__restrict__ blk = field + ((size_t)(v - kNbrCoarser) * nc + c) * 512;
        const int q0 = (par[0] * 4 + P[0] + 8) & 7, q1 = (par[1] * 4 + P[1] + 8) & 7, q2 = (par[2] * 4 + P[2] + 8) & 7;
        val = blk[q2 * 64 + q1 * 8 + q0];
      } else if (v >= 0) {  // FillCoarseVersion: same-level neighbour averaged down
        const double *__restrict__ blk = field + ((size_t)v * nc + c) * 512;
        val = avg_block(blk, 2 * P[0] - 8 * code[0], 2 * P[1] - 8 * code[1], 2 * P[2] - 8 * code[2]);
      }
      patch[L][r] = flip ? -val : val;
    }
    __syncthreads();
    // ---- layers 1 (and 2): finite-difference mode
    const double *__restrict__ own = field + ((size_t)slot * nc + c) * 512;
    int cb[3], cc[3];
    cb[ax] = side ? 7 : 0; cc[ax] = side ? 6 : 1;
    cb[ax1] = cc[ax1] = a1i;
    cb[ax2] = cc[ax2] = a2i;
    const double bv = own[cb[2] * 64 + cb[1] * 8 + cb[0]], cv = own[cc[2] * 64 + cc[1] * 8 + cc[0]];
    const int p1 = a1i >> 1, p2 = a2i >> 1;
    const double av = fd_mode_av(&patch[0][(p2 + 1) * 6 + (p1 + 1)], p1, p2, 1, 6, a1i & 1, a2i & 1);
    double *__restrict__ out = slabs + ((size_t)e * nc + c) * W * 64 + lane;
    out[0] = fd_mode_blend(av, bv, cv, 0);
    if (W == 3) {
      out[64] = fd_mode_blend(av, bv, cv, 1);
      // ---- layer 3: TestInterp around the coarse cell two layers behind the face
      auto Cc = [&](int i, int j, int k) -> double {
        const int off[3] = {i, j, k};
        const int L = side ? off[ax] : 2 - off[ax];
        return patch[L][(p2 + off[ax2]) * 6 + (p1 + off[ax1])];
      };
      int bit[3];
      bit[ax] = side ? 0 : 1;  // the fine layer is the upper child of the coarse cell below the block, the lower one above it
      bit[ax1] = a1i & 1;
      bit[ax2] = a2i & 1;
      out[128] = test_interp(Cc, bit);
    }
  }
}

// ---- flux correction of the coarse side, one launch per normal direction (x, then y, then z: FillCase_2 order): rounds 1-4's form, kept in the
// TESTING build as the A/B and bit-for-bit cross-check of k_flux_fix_blocks below ("flux_fix_by_direction").
// out[cell] += own face flux + ((f00 + f10) + (f01 + f11)) of the fine faces; flux arrays [(e*nfc + c)][a2*8+a1]
#ifdef CUP3D_TESTING
__global__ void __launch_bounds__(64) k_flux_fix(AmrDev a, const int32_t *__restrict__ list, const double *__restrict__ flux, int nfc,
                                                 double *__restrict__ out, int out_nc) {
  const int e = list[blockIdx.x], lane = threadIdx.x;
  const int sf = a.faces[2 * e], slot = sf / 6, f = sf % 6, d = f >> 1, side = f & 1;
  const int a1 = lane & 7, a2 = lane >> 3, j = side ? 7 : 0;
  const int cell = d == 0 ? a2 * 64 + a1 * 8 + j : (d == 1 ? a2 * 64 + j * 8 + a1 : j * 64 + a2 * 8 + a1);
  const int fe = a.fine[4 * e + (a1 >> 2) + 2 * (a2 >> 2)];
  const int i2 = 2 * (a1 & 3), i1 = 2 * (a2 & 3);
  for (int c = 0; c < nfc; ++c) {
    const double *__restrict__ F = flux + ((size_t)fe * nfc + c) * 64;
    const double avg = (F[i2 + i1 * 8] + F[i2 + 1 + i1 * 8]) + (F[i2 + (i1 + 1) * 8] + F[i2 + 1 + (i1 + 1) * 8]);
    const double coarse = flux[((size_t)e * nfc + c) * 64 + lane] + avg;
    double *__restrict__ o = out + ((size_t)slot * out_nc + c) * 512 + cell;
    *o = (*o + coarse) + 0.0;  // + 0.0: the three further FillCase_2 calls on the cleared face
  }
}
#endif

// ONE launch for the ghost slabs of a stencil: workgroups [0, nr) restrict (neighbour finer), [nr, nr + np) interpolate (neighbour
// coarser).  These launches are a few microseconds of work each and sit between the loop kernels of every BiCGSTAB iteration on a
// multi-level mesh: what they cost is their number (rounds 1-4: two launches here, three in the flux correction below).
template <int W>
__global__ void __launch_bounds__(64) k_ghosts(AmrDev a, const int32_t *__restrict__ rlist, unsigned nr, const int32_t *__restrict__ plist, const double *__restrict__ field, int nc,
                                               double *__restrict__ slabs) {
  if (blockIdx.x < nr) ghost_restrict_face<W>(a, rlist[blockIdx.x], field, nc, slabs);
  else ghost_prolong_face<W>(a, plist[blockIdx.x - nr], field, nc, slabs);
}

// The flux correction in ONE launch: one wavefront per coarse-side BLOCK walks the block's corrected faces in the order x-, x+, y-, y+,
// z-, z+.  A cell lies on at most one face per direction, so every cell still receives its corrections direction by direction, x first
// (FillCase_2 order, 2918-2926) -- bit-identical to the three launches of k_flux_fix; the barrier between two faces orders the second
// face's read of a cell behind the first face's write of it (edge and corner cells of the block).
__global__ void __launch_bounds__(64) k_flux_fix_blocks(AmrDev a, const int32_t *__restrict__ tab /* [n][6]: interface face behind face f, -1 none */, const double *__restrict__ flux, int nfc,
                                                        double *out, int out_nc) {
  const int lane = threadIdx.x;
  const int a1 = lane & 7, a2 = lane >> 3;
  for (int f = 0; f < 6; ++f) {
    const int e = tab[6 * blockIdx.x + f];
    if (e < 0) continue;
    const int slot = a.faces[2 * e] / 6, d = f >> 1, j = (f & 1) ? 7 : 0;
    const int cell = d == 0 ? a2 * 64 + a1 * 8 + j : (d == 1 ? a2 * 64 + j * 8 + a1 : j * 64 + a2 * 8 + a1);
    const int fe = a.fine[4 * e + (a1 >> 2) + 2 * (a2 >> 2)];
    const int i2 = 2 * (a1 & 3), i1 = 2 * (a2 & 3);
    for (int c = 0; c < nfc; ++c) {
      const double *__restrict__ F = flux + ((size_t)fe * nfc + c) * 64;
      const double avg = (F[i2 + i1 * 8] + F[i2 + 1 + i1 * 8]) + (F[i2 + (i1 + 1) * 8] + F[i2 + 1 + (i1 + 1) * 8]);
      const double coarse = flux[((size_t)e * nfc + c) * 64 + lane] + avg;
      double *o = out + ((size_t)slot * out_nc + c) * 512 + cell;
      *o = (*o + coarse) + 0.0;  // + 0.0: the three further FillCase_2 calls on the cleared face
    }
    __syncthreads();
  }
}

// ==== Ghosted block tiles: BlockLab::load + post_load (main.cpp:3623-3787) for one block, ONE implementation for every consumer of a
// tensorial (or star) tile: cup3d_sim_labs / cup3d_sim_labs_device (k_labs), cup3d_sim_labs_over_ranks (k_labs_view), the refinement
// of mesh adaptation (k_refine, the [-1,2) tile) and GradChiOnTmp (k_grad_chi, the [-2,3) tile).  It uses the device helpers above --
// avg_down8 / avg_block, fd_mode_av / fd_mode_blend (with interp1d), test_interp -- so a bit-exactness fix to the reference's ghost
// rules lands once.  (k_ghosts above builds star slabs in another shape, for the solver's hot path, and stays on its own.)
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
// The kernel reads blocks only: it neither needs nor touches the ghost slabs the stencil kernels keep behind kNbrHalo.
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
// kernels below, which differ in where the blocks of a tile's neighbourhood live and in what they do with the finished tile.  k_labs,
// one rank: every slot is a row of the field array; phase F stores the tile.  k_labs_view, a mesh spread over ranks
// (cup3d_sim_labs_over_ranks): slots [0, n_local) of the rank's tensorial view are rows of the sim's own field array, read in place; a
// ghost slot is a row of the call's ghost pool, found through pool_of (-1: not fetched -- row 0 of the pool, which holds NaN, so that
// a read the request plan did not foresee shows in the tile instead of leaving the buffer).  k_refine and k_grad_chi (mesh adaptation)
// read rows of a field array, as k_labs does, and keep the tile in LDS for their operator.
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

#define LABS_BLOCK(slot, c) (src + ((size_t)(slot) * nc + (c)) * 512)
#define LABS_CELL(slot, c, i) src[((size_t)(slot) * nc + (c)) * 512 + (i)]
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
#undef LABS_SLOT
#undef LABS_AFTER_SLOT

// ---- mesh adaptation: the eight children of a refined block (refine_1 + RefineBlocks, main.cpp:5227-5249, 5493-5565).
// One workgroup per refined parent builds the parent's tensorial [-1,2) tile on the OLD mesh in LDS exactly as BlockLab::load
// does (phases A-E at W = 1; a scalar is never negated at a domain face: bc_comp = -1), one component at a time, and expands it.
// items[n][9]: parent slot (old mesh), eight child slots (new mesh, child = I + 2J + 4K)
template <int NC>
__global__ void __launch_bounds__(256) k_refine(LabDev a, const int32_t *__restrict__ items, const double *__restrict__ src, double *__restrict__ dst) {
  constexpr int W = 1, nc = NC;
#define LABS_SLOT items[9 * blockIdx.x]
#include "labs_setup.hpp"
#undef LABS_SLOT
  for (int c = 0; c < nc; ++c) {
#include "labs_phases.hpp"
    // RefineBlocks, 5493-5565
    for (int k = 0; k < 2; ++k) {
      const int cell = k * 256 + t, x = cell & 7, y = (cell >> 3) & 7, z = cell >> 6;
      const int fs = items[9 * blockIdx.x + 1 + (z >> 2) * 4 + (y >> 2) * 2 + (x >> 2)];
      const int i = 2 * (x & 3), j = 2 * (y & 3), kk = 2 * (z & 3);
#define Lb(a_, b_, c_) lab[lix(x + (a_), y + (b_), z + (c_))]
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
      double *b = dst + ((size_t)fs * NC + c) * 512;
#define B(a_, b_, c_) b[((kk + (c_)) * 8 + (j + (b_))) * 8 + (i + (a_))]
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
    __syncthreads();  // the next component reuses lab[]
  }
}

// ---- compute<ScalarLab>(GradChiOnTmp(sim), sim.chi), main.cpp:8540-8600: the chi-driven half of adaptMesh's tagging input.
// One workgroup per block builds the TENSORIAL [-2,3) tile of chi exactly as BlockLab::load does for that stencil (phases A-E at
// W = 2, zero-gradient domain faces: Neumann3D 5929-6004) and then applies the operator: the cap of the vorticity on level
// levelMaxVorticity - 1, the ordered scan (z, y, x over the block grown by `offset`) for the first cell with 1e-5 < chi < 0.9, which
// flags the block with 1e10 and ends the scan, and the clearing of interior cells with chi > 0.9 met before it.  The scan is
// evaluated in parallel through its one order dependence: the position of that first cell (an LDS atomicMin of the scan index).
__global__ void __launch_bounds__(256) k_grad_chi(LabDev a, int level_max, int lmv, double Rtol, double Ctol, const double *__restrict__ src, double *__restrict__ tmpV) {
  constexpr int W = 2, nc = 1;
  __shared__ int first;
#define LABS_SLOT (int)blockIdx.x
#include "labs_setup.hpp"
#undef LABS_SLOT
  if (t == 0) first = 0x7fffffff;
  {
    constexpr int c = 0;
#include "labs_phases.hpp"
  }
  // the operator
  double *T = tmpV + (size_t)pb * 1536;
  const int level = lev;
  if (level == lmv - 1 && lmv < level_max) {  // 8546-8557
    for (int c = t; c < 512; c += 256) {
      const double u0 = T[c], u1 = T[512 + c], u2 = T[1024 + c];
      if (sqrt(u0 * u0 + u1 * u1 + u2 * u2) >= Rtol) { T[c] = 0.5 * (Rtol + Ctol); T[512 + c] = 0.0; T[1024 + c] = 0.0; }
    }
  }
  const int off = level == level_max - 1 ? 2 : 1;
  for (int e = t; e < 1728; e += 256) {
    const int x = e % 12 - 2, y = (e / 12) % 12 - 2, z = e / 144 - 2;
    if (x < -off || x >= 8 + off || y < -off || y >= 8 + off || z < -off || z >= 8 + off) continue;
    double v = lab[e];
    v = v < 1.0 ? v : 1.0;
    v = v > 0.0 ? v : 0.0;
    if (v > 0.00001 && v < 0.9) atomicMin(&first, e);  // e grows in the reference's scan order (z, y, x)
  }
  __syncthreads();
  const int stop = first;
  for (int c = t; c < 512; c += 256) {
    const int x = c & 7, y = (c >> 3) & 7, z = c >> 6, e = lix(x, y, z);
    double v = lab[e];
    v = v < 1.0 ? v : 1.0;
    if (v > 0.9 && e < stop) { T[c] = 0.0; T[512 + c] = 0.0; T[1024 + c] = 0.0; }  // 8592-8597
  }
  __syncthreads();
  if (stop != 0x7fffffff && t < 6) {  // 8567-8590 (six distinct cells among the eight assignments)
    const int cx[6] = {3, 4, 3, 3, 4, 4}, cy[6] = {3, 3, 4, 3, 4, 3}, cz[6] = {3, 3, 3, 4, 4, 4};
    T[(cz[t] * 8 + cy[t]) * 8 + cx[t]] = 1e10;
  }
}
#undef LABS_BLOCK
#undef LABS_CELL

// the same as k_labs for the local blocks of a rank's tensorial view: tables of the view, ghost blocks in the pool
#define LABS_BLOCK(slot, c) src.blk(slot, nc, c)
#define LABS_CELL(slot, c, i) src.blk(slot, nc, c)[i]
#define LABS_SLOT slots ? slots[blockIdx.x] : first + (int)blockIdx.x
#define LABS_AFTER_SLOT double *__restrict__ tile = out + (size_t)blockIdx.x * L3 * nc;
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

// unchanged blocks: copy; parents of compressed octets: compress (5272-5329) -- pairs[n][2] = dst slot, src slot;
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
    for (int c = 0; c < nc; ++c) {
      const double *b = src + ((size_t)fs * nc + c) * 512;
#define B(a_, b_, c_) b[((kk + (c_)) * 8 + (j + (b_))) * 8 + (i + (a_))]
      dst[((size_t)pb * nc + c) * 512 + cell] =
          0.125 * ((B(0, 0, 0) + B(1, 1, 1)) + (B(1, 0, 0) + B(0, 1, 1)) + (B(0, 1, 0) + B(1, 0, 1)) + (B(1, 1, 0) + B(0, 0, 1)));  // 5298-5302
#undef B
    }
  }
}

// ---- host side
int amr_fill_ghosts(Sim *s, const double *field, int nc, int w, double *slabs, int part) {
  AmrDev a{s->d_amr_faces, s->d_amr_fine, s->d_nbr27, s->d_nbr, s->d_index, nc == 1 ? s->scalar_bc_dir : -1};
  ProfileScope ps("amr_ghosts");
  // both lists hold the faces of inner blocks first (sim_build): a rank view produces those while its ghost blocks travel
  const unsigned r0 = part == 2 ? s->n_restrict_inner : 0, r1 = part == 1 ? s->n_restrict_inner : s->n_restrict;
  const unsigned p0 = part == 2 ? s->n_prolong_inner : 0, p1 = part == 1 ? s->n_prolong_inner : s->n_prolong;
  if (r1 + p1 > r0 + p0) {  // one launch: the restricting faces first, then the interpolating ones
    const unsigned nr = r1 - r0, np = p1 - p0;
    if (w == 3) hipLaunchKernelGGL(k_ghosts<3>, dim3(nr + np), dim3(64), 0, stream(), a, (const int32_t *)s->d_restrict_list + r0, nr, (const int32_t *)s->d_prolong_list + p0, field, nc, slabs);
    else hipLaunchKernelGGL(k_ghosts<1>, dim3(nr + np), dim3(64), 0, stream(), a, (const int32_t *)s->d_restrict_list + r0, nr, (const int32_t *)s->d_prolong_list + p0, field, nc, slabs);
  }
  CUP3D_HIP(hipGetLastError());
  return CUP3D_OK;
}

int amr_flux_fix(Sim *s, int nfc, double *out, int out_nc) {
  AmrDev a{s->d_amr_faces, s->d_amr_fine, s->d_nbr27, s->d_nbr, s->d_index, -1};
  {  // rank views: the fluxes of fine faces owned by other ranks arrive first (FluxCorrectionMPI, main.cpp:2848-2945)
    int rc = view_exchange_flux(s, nfc);
    if (rc) return rc;
  }
  ProfileScope ps("amr_flux_fix");
#ifdef CUP3D_TESTING
  if (debug_option("flux_fix_by_direction")) {  // A/B and the bit-for-bit cross-check: rounds 1-4's three launches, x faces, then y, then z
    for (int d = 0; d < 3; ++d) {
      const unsigned n = (unsigned)s->grid->fix_faces[d].size();
      if (n) hipLaunchKernelGGL(k_flux_fix, dim3(n), dim3(64), 0, stream(), a, s->d_fix_list[d], s->d_flux, nfc, out, out_nc);
    }
    CUP3D_HIP(hipGetLastError());
    return CUP3D_OK;
  }
#endif
  if (s->n_fix_blocks) hipLaunchKernelGGL(k_flux_fix_blocks, dim3(s->n_fix_blocks), dim3(64), 0, stream(), a, (const int32_t *)s->d_fix_blocks, (const double *)s->d_flux, nfc, out, out_nc);
  CUP3D_HIP(hipGetLastError());
  return CUP3D_OK;
}

}  // namespace cup3d

using namespace cup3d;

namespace {
__global__ void __launch_bounds__(256) k_pack_blocks(const double *__restrict__ field, const int32_t *__restrict__ slots, int nc, double *__restrict__ out) {
  const double *src = field + (size_t)slots[blockIdx.x] * nc * 512;
  double *dst = out + (size_t)blockIdx.x * nc * 512;
  for (int i = threadIdx.x; i < nc * 512; i += 256) dst[i] = src[i];
}
__global__ void __launch_bounds__(256) k_unpack_blocks(const double *__restrict__ in, const int32_t *__restrict__ slots, int nc, double *__restrict__ field) {
  const double *src = in + (size_t)blockIdx.x * nc * 512;
  double *dst = field + (size_t)slots[blockIdx.x] * nc * 512;
  for (int i = threadIdx.x; i < nc * 512; i += 256) dst[i] = src[i];
}
}  // namespace

// The finer leaves behind every kNbrFiner position of the blocks [0, nloc) of `mo`, by octant of the block (bits of x, y, z >= 4):
// finer_row[b] = the block's row of finer[rows][27][8] (-1: no finer neighbour), -1 in the row where nothing is read.  Throws what
// Grid::leaf throws.
static void finer_tables(const Grid *mo, int64_t nloc, std::vector<int32_t> &finer_row, std::vector<int32_t> &finer) {
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

// ---- data movement of MeshAdaptation::Adapt, shared by the one-rank and the multi-rank entry points.
// `mo`: the OLD mesh as this rank sees it (a whole mesh, or a tensorial rank view whose ghost slots of `fs` hold the owners' data);
// `blocks`: the blocks to produce, each with the slot of `fd` it goes to.  A block is a leaf of the old mesh (copied), a child of
// one (refine_1 + RefineBlocks, 5227-5249, 5493-5565) or the parent of an octet of them (compress, 5272-5329).
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

extern "C" int cup3d_adapt_transfer(cup3d_sim_t *src_h, cup3d_sim_t *dst_h, int field) {
  if (!src_h || !dst_h) return CUP3D_EINVAL;
  Sim *src = reinterpret_cast<Sim *>(src_h), *dst = reinterpret_cast<Sim *>(dst_h);
  int nc, nc2;
  const double *fs = src->field(field, &nc);
  double *fd = dst->field(field, &nc2);
  if (!fs || !fd) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
  if (src->grid->n_local >= 0 || dst->grid->n_local >= 0) { set_error("cup3d_adapt_transfer: meshes spread over ranks go through cup3d_adapt_migrate"); return CUP3D_EINVAL; }
  std::unique_ptr<Grid> mo_tmp, mn_tmp;
  const Grid *mo = src->grid, *mn = dst->grid;
  std::vector<NewBlock> blocks;
  try {
    if (!mo->multilevel) { mo_tmp = mo->as_mesh(); mo = mo_tmp.get(); }
    if (!mn->multilevel) { mn_tmp = mn->as_mesh(); mn = mn_tmp.get(); }
    for (int d = 0; d < 3; ++d)
      if (mo->bpd[d] != mn->bpd[d] || mo->bc[d] != mn->bc[d] || mo->level_max != mn->level_max) throw std::invalid_argument("the two meshes belong to different boxes");
  } catch (const std::exception &e) {
    set_error("cup3d_adapt_transfer: %s", e.what());
    return CUP3D_EINVAL;
  }
  blocks.resize((size_t)mn->nblocks());
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
extern "C" int cup3d_adapt_migrate(const cup3d_grid_t *old_mesh_h, const int32_t *old_owner, cup3d_sim_t *src_h, const cup3d_grid_t *new_mesh_h,
                                   const int32_t *new_owner, cup3d_sim_t *dst_h, int field) {
  if (!src_h || !dst_h) return CUP3D_EINVAL;  // (without the sims there is no communicator to tell the other ranks through)
  Sim *src = reinterpret_cast<Sim *>(src_h), *dst = reinterpret_cast<Sim *>(dst_h);
  const Grid *om = reinterpret_cast<const Grid *>(old_mesh_h), *nm = reinterpret_cast<const Grid *>(new_mesh_h);
  const int me = src->grid->rank, nranks = src->grid->nranks;
  int nc = 0, nc2 = 0;
  const double *fs = nullptr;
  double *fd = nullptr;
  std::unique_ptr<Grid> tv;
  std::vector<NewBlock> mine;               // what this rank produces, ordered by (consumer, new global slot)
  std::vector<int64_t> send_count(nranks, 0), recv_count(nranks, 0);
  std::vector<int32_t> recv_slots;          // local slots of dst in arrival order: by (producer, new global slot)
  size_t per = 0;
  Dev<double> F, prod, recv, pack;
  Dev<int32_t> d_send, d_recv_slots;
  // everything this rank can get wrong on its own -- arguments, the plan, allocations -- happens in here; the ranks then agree on the
  // outcome BEFORE the first exchange, so that a bad call on one rank returns an error on every rank instead of blocking the others
  auto local_part = [&]() -> int {
    if (!old_mesh_h || !old_owner || !new_mesh_h || !new_owner) { set_error("cup3d_adapt_migrate: null argument"); return CUP3D_EINVAL; }
    fs = src->field(field, &nc);
    fd = dst->field(field, &nc2);
    if (!fs || !fd) { set_error("unknown field id %d", field); return CUP3D_EINVAL; }
    if (!om->multilevel || !nm->multilevel || om->n_local >= 0 || nm->n_local >= 0) { set_error("cup3d_adapt_migrate needs the two GLOBAL mesh objects"); return CUP3D_EINVAL; }
    if (dst->grid->rank != me || dst->grid->nranks != nranks) { set_error("cup3d_adapt_migrate: the two sims belong to different ranks"); return CUP3D_EINVAL; }
    try {
      tv = om->rank_view(old_owner, me, nranks, /*tensorial=*/true);
      if (tv->n_local != src->nb) throw std::invalid_argument("the source sim does not hold this rank's blocks of the old mesh");
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
    } catch (const std::exception &e) {
      set_error("cup3d_adapt_migrate: %s", e.what());
      return CUP3D_EINVAL;
    }
    per = (size_t)nc * 512;
    const size_t nvis = tv->Z.size();
    int rc;
    if ((rc = F.alloc(nvis * per)) || (rc = prod.alloc(std::max<size_t>(mine.size(), 1) * per)) || (rc = recv.alloc(std::max<size_t>(recv_slots.size(), 1) * per)) ||
        (rc = pack.alloc(std::max<size_t>(tv->send_blocks.size(), 1) * per)) || (rc = d_send.upload(tv->send_blocks, stream(), IfEmpty::null)))
      return rc;
    // the old field on the tensorial view: local blocks (the ghost blocks arrive from their owners below)
    CUP3D_HIP(hipMemcpyAsync(F, fs, (size_t)src->nb * per * sizeof(double), hipMemcpyDeviceToDevice, stream()));
    if (!tv->send_blocks.empty())
      hipLaunchKernelGGL(k_pack_blocks, dim3((unsigned)tv->send_blocks.size()), dim3(256), 0, stream(), (const double *)F, d_send.get(), nc, pack.get());
    CUP3D_HIP(hipGetLastError());
    return CUP3D_OK;
  };
  int rc = agree(src, local_part(), "cup3d_adapt_migrate");
  if (rc) return rc;
  if ((rc = exchange_items(src, pack, tv->send_block_count, F + (size_t)tv->n_local * per, tv->recv_block_count, per))) return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));
  // producing the new blocks is rank-local again (kernels, table uploads): agree once more before they travel
  if ((rc = agree(src, adapt_produce(tv.get(), mine, F, prod, nc), "cup3d_adapt_migrate (produce)"))) return rc;
  if ((rc = exchange_items(src, prod, send_count, recv, recv_count, per))) return rc;
  if (!recv_slots.empty()) {
    if ((rc = d_recv_slots.upload(recv_slots, stream(), IfEmpty::null))) return rc;
    hipLaunchKernelGGL(k_unpack_blocks, dim3((unsigned)recv_slots.size()), dim3(256), 0, stream(), (const double *)recv, d_recv_slots.get(), nc, fd);
    CUP3D_HIP(hipGetLastError());
  }
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return CUP3D_OK;
}

// compute<ScalarLab>(GradChiOnTmp(sim), sim.chi) (main.cpp:15182, 8540-8600): edits tmpV (= the vorticity of ComputeVorticity) from
// the resident chi; with cup3d_compute_vorticity before and cup3d_tag_blocks after it, adaptMesh's decision input is complete for
// runs with obstacles.  `mo`: a multi-level mesh object whose first `nloc` slots are the blocks of `tmpV` (the mesh itself on one
// rank, the rank's TENSORIAL view over ranks -- the tensorial chi tile reaches edge / corner neighbours); `chi` lives on mo's slots.
static int grad_chi_run(const Grid *mo, int64_t nloc, const double *chi, double *tmpV, double Rtol, double Ctol, int level_max_vorticity) {
  LabIndex tab;
  int rc = tab.build(mo, nloc, "cup3d_grad_chi_on_tmp");
  if (rc) return rc;
  {
    ProfileScope ps("grad_chi_on_tmp");
    hipLaunchKernelGGL(k_grad_chi, dim3((unsigned)nloc), dim3(256), 0, stream(), tab.dev(mo, -1), mo->level_max, level_max_vorticity, Rtol, Ctol, chi, tmpV);
  }
  CUP3D_HIP(hipGetLastError());
  CUP3D_HIP(hipStreamSynchronize(stream()));  // the tables above are freed on return
  return CUP3D_OK;
}

extern "C" int cup3d_grad_chi_on_tmp(cup3d_sim_t *h, double Rtol, double Ctol, int level_max_vorticity) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (s->grid->nranks > 1) { set_error("cup3d_grad_chi_on_tmp: a mesh spread over ranks goes through cup3d_grad_chi_on_tmp_over_ranks (its chi tile needs edge / corner ghost blocks)"); return CUP3D_ESTATE; }
  std::unique_ptr<Grid> tmp;
  const Grid *mo = s->grid;
  try {
    if (!mo->multilevel) { tmp = mo->as_mesh(); mo = tmp.get(); }
  } catch (const std::exception &e) {
    set_error("cup3d_grad_chi_on_tmp: %s", e.what());
    return CUP3D_EINVAL;
  }
  return grad_chi_run(mo, mo->nblocks(), s->chi, s->tmpV, Rtol, Ctol, level_max_vorticity);
}

// The same on a mesh spread over ranks: `mesh` / `owner` are the global mesh object and the rank of every leaf (as for
// cup3d_adapt_migrate); chi of the edge / corner / finer neighbours other ranks own arrives first (the plan of the rank's tensorial view),
// then the one-rank kernel runs on the rank's blocks.  Collective: every rank calls it.
extern "C" int cup3d_grad_chi_on_tmp_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh_h, const int32_t *owner, double Rtol, double Ctol, int level_max_vorticity) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const Grid *gm = reinterpret_cast<const Grid *>(mesh_h);
  const int me = s->grid->rank, nranks = s->grid->nranks;
  std::unique_ptr<Grid> tv;
  Dev<double> F, pack;
  Dev<int32_t> d_send;
  auto local_part = [&]() -> int {  // what one rank can get wrong on its own; the ranks agree on the outcome before anything is exchanged
    if (!mesh_h || !owner) { set_error("cup3d_grad_chi_on_tmp_over_ranks: null argument"); return CUP3D_EINVAL; }
    if (!gm->multilevel || gm->n_local >= 0) { set_error("cup3d_grad_chi_on_tmp_over_ranks needs the GLOBAL mesh object"); return CUP3D_EINVAL; }
    try {
      tv = gm->rank_view(owner, me, nranks, /*tensorial=*/true);
      if (tv->n_local != s->nb) throw std::invalid_argument("the sim does not hold this rank's blocks of the mesh");
    } catch (const std::exception &e) {
      set_error("cup3d_grad_chi_on_tmp_over_ranks: %s", e.what());
      return CUP3D_EINVAL;
    }
    const size_t nvis = tv->Z.size();
    int rc;
    if ((rc = F.alloc(nvis * 512)) || (rc = pack.alloc(std::max<size_t>(tv->send_blocks.size(), 1) * 512)) || (rc = d_send.upload(tv->send_blocks, stream(), IfEmpty::null))) return rc;
    CUP3D_HIP(hipMemcpyAsync(F, s->chi, (size_t)s->nb * 512 * sizeof(double), hipMemcpyDeviceToDevice, stream()));
    if (!tv->send_blocks.empty())
      hipLaunchKernelGGL(k_pack_blocks, dim3((unsigned)tv->send_blocks.size()), dim3(256), 0, stream(), (const double *)F, d_send.get(), 1, pack.get());
    CUP3D_HIP(hipGetLastError());
    return CUP3D_OK;
  };
  int rc = agree(s, local_part(), "cup3d_grad_chi_on_tmp_over_ranks");
  if (rc) return rc;
  if ((rc = exchange_items(s, pack, tv->send_block_count, F + (size_t)tv->n_local * 512, tv->recv_block_count, 512))) return rc;
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return grad_chi_run(tv.get(), tv->n_local, F, s->tmpV, Rtol, Ctol, level_max_vorticity);
}

// TEST SUPPORT: the ghost slabs of every interface face for `field` and a w-deep stencil, [(e*nc + c)*w + gl][64]
#ifdef CUP3D_TESTING  // test / tuning support: not in the release library at all
extern "C" int cup3d_debug_amr_slabs(cup3d_sim_t *h, int field, int w, double *out) {
  if (!h || !out || (w != 1 && w != 3)) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (!s->grid->multilevel) { set_error("cup3d_debug_amr_slabs: not a multi-level mesh"); return CUP3D_EINVAL; }
  int nc;
  const double *f = s->field(field, &nc);
  if (!f) return CUP3D_EINVAL;
  int rc = amr_fill_ghosts(s, f, nc, w, s->halo_recv);
  if (rc) return rc;
  CUP3D_HIP(hipMemcpyAsync(out, s->halo_recv, (size_t)s->grid->n_amr_faces() * nc * w * 64 * sizeof(double), hipMemcpyDeviceToHost, stream()));
  CUP3D_HIP(hipStreamSynchronize(stream()));
  return CUP3D_OK;
}
#endif

// ==== cup3d_sim_labs / cup3d_sim_labs_device: the host side of k_labs (the kernels and what they do: "ghosted block tiles" above)
namespace cup3d {

// ---- host side
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

// tables of k_labs, built when the first tile is asked for: a uniform grid is read as the one-level mesh it is (Grid::as_mesh)
static int labs_prepare(Sim *s, bool want_stage) {
  if (!s->labs) {
    std::unique_ptr<Grid> tmp;
    const Grid *mo = s->grid;
    try {
      if (!mo->multilevel) { tmp = mo->as_mesh(); mo = tmp.get(); }
    } catch (const std::exception &e) {
      set_error("cup3d_sim_labs: %s", e.what());
      return CUP3D_EINVAL;
    }
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

}  // namespace cup3d

extern "C" int cup3d_sim_labs_device(cup3d_sim_t *h, int field, long n, const int32_t *slots, int width, int tensorial, int scalar_dir, void *device_out) {
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

extern "C" int cup3d_sim_labs(cup3d_sim_t *h, int field, long n, const int32_t *slots, int width, int tensorial, int scalar_dir, double *host_out) {
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

// ==== cup3d_sim_labs_over_ranks / cup3d_sim_labs_over_ranks_device.  The same tiles when the mesh is spread over ranks: what BlockLabMPI::load
// (main.cpp:4648-4658) gets from SynchronizerMPI_AMR::fetch (2423-2544).  The sim lives on its rank view of the mesh or on its share of a
// uniform grid; the tiles are built through the tables of the rank's TENSORIAL view (every same-level, coarser and finer leaf of the
// 27-point neighbourhood is a ghost slot there), which is derived once per (mesh, owner) and kept in the sim.  Per call:
//   needs    Grid::lab_boxes replays phases A and B of the kernel (labs_body.hpp) for the requested blocks: per ghost block the box of cells read;
//   request  one double per ghost block (the box as an exact integer, 0: nothing) travels to the block's owner -- the view's block plan
//            with the two count vectors swapped -- and comes back to the host, so that owner and receiver know every message's length;
//   data     the owner packs the boxes (k_pack_boxes), one exchange of nc doubles per cell, the receiver scatters them into a pool that
//            holds the fetched ghost blocks only (k_unpack_boxes; pool_of[ghost] -> pool row);
//   tiles    k_labs_view reads local blocks from the sim's field array in place and ghost blocks from the pool.
// Everything crosses ranks through agree() and exchange_items() (RCCL, the host transport, the in-process test communicator).
namespace cup3d {

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

extern "C" int cup3d_sim_labs_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, int field, long n, const int32_t *slots, int width,
                                         int tensorial, int scalar_dir, double *host_out) {
  return labs_over_ranks(h, mesh, owner, field, n, slots, width, tensorial, scalar_dir, host_out, true);
}

extern "C" int cup3d_sim_labs_over_ranks_device(cup3d_sim_t *h, const cup3d_grid_t *mesh, const int32_t *owner, int field, long n, const int32_t *slots, int width,
                                                int tensorial, int scalar_dir, void *device_out) {
  return labs_over_ranks(h, mesh, owner, field, n, slots, width, tensorial, scalar_dir, device_out, false);
}
