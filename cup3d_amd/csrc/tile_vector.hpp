// The ghosted 10^3 tile of a vector block field in LDS (stencil [-1,2)), all three components, shared by the stencil kernels that read
// whole velocity gradients (stencil.hip: vorticity, diffusion right-hand side) and the flow diagnostics (diagnostics.hip).  Kept apart from
// tile7.hpp, which the Poisson solver's translation unit includes.
#pragma once
#include "tile7.hpp"

namespace cup3d {

// all three components with ghosts behind all six faces (VectorLab with BlockLabBC: wall negates every component,
// freespace the one normal to the face, main.cpp:6137-6153, 6384-6394)
__device__ __forceinline__ void load_vector_tile(const GridDev &g, int slot, const double *__restrict__ f, const double *__restrict__ halo, double *tile) {
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const double *own = f + (size_t)slot * 1536;
  int x, y, z0, cell0;
  thread_cells(t, x, y, z0, cell0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    tile[c * kT + tix(x, y, z0)] = own[c * 512 + cell0];
    tile[c * kT + tix(x, y, z0 + 4)] = own[c * 512 + 256 + cell0];
  }
  for (int u = wave; u < 18; u += 4) {  // (face, component) units of 64 ghosts
    const int face = u / 3, c = u - 3 * face;
    const int n = g.nbr[slot * 6 + face];
    int nb_cell, own_cell, lds;
    face1(face, lane, nb_cell, own_cell, lds);
    double v;
    if (n >= kNbrHalo) v = halo[((size_t)(n - kNbrHalo) * 3 + c) * 64 + lane];
    else if (n >= 0) v = f[(size_t)n * 1536 + c * 512 + nb_cell];
    else { v = own[c * 512 + own_cell]; if (n == -3 || c == (face >> 1)) v = -v; }
    tile[c * kT + lds] = v;
  }
}

}  // namespace cup3d
