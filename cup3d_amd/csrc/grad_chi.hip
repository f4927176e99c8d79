// compute<ScalarLab>(GradChiOnTmp(sim), sim.chi), main.cpp:8540-8600 (called at 15182): the chi-driven half of adaptMesh's tagging
// input.  It edits tmpV (= the vorticity of ComputeVorticity) from the resident chi; with cup3d_compute_vorticity before and
// cup3d_tag_blocks after it, adaptMesh's decision input is complete for runs with obstacles.
#include "labs.hpp"

namespace cup3d {

// One workgroup per block builds the TENSORIAL [-2,3) tile of chi exactly as BlockLab::load does for that stencil (the lab phases of
// labs.hpp at W = 2, zero-gradient domain faces: Neumann3D 5929-6004) and then applies the operator: the cap of the vorticity on level
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
#include "labs_phases.hpp"  // through LABS_BLOCK / LABS_CELL of labs.hpp, which read `src` and `nc` of this scope
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

// `mo`: a multi-level mesh object whose first `nloc` slots are the blocks of `tmpV` (the mesh itself on one rank, the rank's TENSORIAL
// view over ranks -- the tensorial chi tile reaches edge / corner neighbours); `chi` lives on mo's slots.
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

}  // namespace cup3d
using namespace cup3d;
extern "C" {
int cup3d_grad_chi_on_tmp(cup3d_sim_t *h, double Rtol, double Ctol, int level_max_vorticity) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  if (s->grid->nranks > 1) { set_error("cup3d_grad_chi_on_tmp: a mesh spread over ranks goes through cup3d_grad_chi_on_tmp_over_ranks (its chi tile needs edge / corner ghost blocks)"); return CUP3D_ESTATE; }
  MeshOf mesh;
  const Grid *mo = mesh.get(s->grid, "cup3d_grad_chi_on_tmp");
  if (!mo) return CUP3D_EINVAL;
  return grad_chi_run(mo, mo->nblocks(), s->chi, s->tmpV, Rtol, Ctol, level_max_vorticity);
}

// The same on a mesh spread over ranks: `mesh` / `owner` are the global mesh object and the rank of every leaf (as for
// cup3d_adapt_migrate); chi of the edge / corner / finer neighbours other ranks own arrives first (the plan of the rank's tensorial view),
// then the one-rank kernel runs on the rank's blocks.  Collective: every rank calls it.
int cup3d_grad_chi_on_tmp_over_ranks(cup3d_sim_t *h, const cup3d_grid_t *mesh_h, const int32_t *owner, double Rtol, double Ctol, int level_max_vorticity) {
  if (!h) return CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const Grid *gm = reinterpret_cast<const Grid *>(mesh_h);
  ViewField chi;
  auto local_part = [&]() -> int {  // what one rank can get wrong on its own; the ranks agree on the outcome before anything is exchanged
    if (!mesh_h || !owner) { set_error("cup3d_grad_chi_on_tmp_over_ranks: null argument"); return CUP3D_EINVAL; }
    if (!gm->multilevel || gm->n_local >= 0) { set_error("cup3d_grad_chi_on_tmp_over_ranks needs the GLOBAL mesh object"); return CUP3D_EINVAL; }
    return chi.stage(gm, owner, s, s->chi, 1, "cup3d_grad_chi_on_tmp_over_ranks", "the sim does not hold this rank's blocks of the mesh", [] {});
  };
  int rc = agree(s, local_part(), "cup3d_grad_chi_on_tmp_over_ranks");
  if (rc) return rc;
  if ((rc = chi.exchange(s))) return rc;
  return grad_chi_run(chi.tv.get(), chi.tv->n_local, chi.F, s->tmpV, Rtol, Ctol, level_max_vorticity);
}
}  // extern "C"
