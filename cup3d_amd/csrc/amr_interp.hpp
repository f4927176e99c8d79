// The reference's coarse/fine arithmetic, one device helper per rule: AverageDown, the finite-difference mode of
// CoarseFineInterpolation and TestInterp.  ONE definition for the two consumers -- the ghost slabs of the star stencils (amr.hip:
// ghost_restrict_face, ghost_prolong_face) and phases A, B and D of the ghosted tiles (labs_phases.hpp) -- so a bit-exactness fix to
// the reference's ghost rules lands once.  All arithmetic keeps the reference's association (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

namespace cup3d {

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

// Tables in constant memory: defined in the device pass of every translation unit that includes this (each code object carries its own
// pair), only declared in the host pass, which never reads them, so the host objects do not collide at link time.  (`static` lets the
// compiler fold the values into the instructions: other code and register figures than the ones the tile kernels are pinned to.)
#ifdef __HIP_DEVICE_COMPILE__
__constant__ double kCoefPlus[9] = {-0.09375, 0.4375, 0.15625, 0.15625, -0.5625, 0.90625, -0.09375, 0.4375, 0.15625};   // d_coef_plus, 3485-3486
__constant__ double kCoefMinus[9] = {0.15625, -0.5625, 0.90625, -0.09375, 0.4375, 0.15625, 0.15625, 0.4375, -0.09375};  // d_coef_minus, 3487-3488
#else
extern __constant__ double kCoefPlus[9], kCoefMinus[9];
#endif

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

}  // namespace cup3d
