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
// (The interpolation rules themselves live in amr_interp.hpp, shared with the ghosted block tiles of labs.hpp.)
#include "amr_interp.hpp"
#include "sim.hpp"

namespace cup3d {

struct AmrDev {
  const int32_t *faces;  // [ne][2]: 6*slot + face, kind
  const int32_t *fine;   // [ne][4]
  const int32_t *nbr27;  // [nb][27]
  const int32_t *nbr;    // [nb][6]
  const int32_t *index;  // [nb][3]
  int bc_comp;           // scalar fields: -1 = zero-gradient domain faces (BlockLabNeumann3D); k = element of BlockLabBC<.., direction k>
};

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

// TEST SUPPORT: the ghost slabs of every interface face for `field` and a w-deep stencil, [(e*nc + c)*w + gl][64]
#ifdef CUP3D_TESTING  // test / tuning support: not in the release library at all
extern "C" int cup3d_debug_amr_slabs(cup3d_sim_t *h, int field, int w, double *out) {
  using namespace cup3d;
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
