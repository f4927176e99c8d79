// The SET-UP of a kernel that assembles ghosted block tiles (k_labs<W>, k_labs_view<W>: labs.hip; k_refine<NC>: adapt.hip; k_grad_chi: grad_chi.hip), included as
// text at the top of the kernel's body; labs_phases.hpp, included after it, assembles one component.  (A __device__ function template
// on the block source was the first form; inlined, it compiled k_labs to other register figures than the ones
// tests/test_labs_kernel_resources.py holds it to -- 5 and 4 scalar registers parked in VGPR lanes at w = 2 and 3 instead of 2 --
// whichever way the source was passed.  Included as text, k_labs is token for token the kernel it was.)  The includer provides
//   W                                 the box [-W, W+1)^3, 1..4, a constant expression
//   a                                 the LabDev of the mesh
//   LABS_SLOT                         the block slot of this workgroup
//   LABS_AFTER_SLOT                   optional: a statement that goes right behind `pb`.  k_labs declares its output pointer there: declared
//                                     behind the set-up instead, k_labs<2> parks 4 scalar registers in VGPR lanes, not 2
// and gets: lab[] (the fine tile), Ct[] (the coarse shadow tile), t, pb, n27, fin, idx, par, lev, has_coarse, dom, lix(x, y, z).
  constexpr int L = 8 + 2 * W, L3 = L * L * L, C3 = kLabCoarse * kLabCoarse * kLabCoarse;
  __shared__ double lab[L3];
  __shared__ double Ct[C3];
  const int t = threadIdx.x;
  const int pb = LABS_SLOT;
#ifdef LABS_AFTER_SLOT
  LABS_AFTER_SLOT
#endif
  const int32_t *n27 = a.n27 + 27 * (size_t)pb;
  const int32_t *fin = a.finer_row[pb] >= 0 ? a.finer + (size_t)a.finer_row[pb] * 216 : nullptr;
  const int idx[3] = {a.index[3 * pb], a.index[3 * pb + 1], a.index[3 * pb + 2]};
  const int par[3] = {idx[0] & 1, idx[1] & 1, idx[2] & 1};
  const int lev = a.level[pb];
  bool has_coarse = false;
  for (int i = 0; i < 27; ++i) has_coarse = has_coarse || n27[i] >= kNbrCoarser;
  // domain faces of this block: bit f of `dom` (f = x-, x+, y-, y+, z-, z+) where a boundary condition sits behind the face
  int dom = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (a.bc[d] == CUP3D_BC_PERIODIC) continue;
    if (idx[d] == 0) dom |= 1 << (2 * d);
    if (idx[d] == (a.bpd[d] << lev) - 1) dom |= 2 << (2 * d);
  }
  auto lix = [](int x, int y, int z) { return ((z + W) * L + (y + W)) * L + (x + W); };
