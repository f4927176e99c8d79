// Obstacle operators that sit between / inside the two hot-path operators: KernelPenalization
// (main.cpp:13841-13912) + kernelFinalizePenalizationForce (13913-13938), kernelUpdateTmpV (14948-14979), UpdateObstacles (13812-13837),
// ComputeForces (12273-12503) and the grid half of CreateObstacles (13596-13619).
// The obstacles themselves (geometry -- the signed distance and the deformation velocity -- and rigid-body integration) stay on the host;
// cup3d_create_obstacles turns the signed distance into chi, surface points and momentum-free udef, and the other kernels take the
// ObstacleBlocks of one obstacle at a time -- chi[8][8][8] and udef[8][8][8][3] in the reference's own (AoS) layout -- so the
// velocity does not have to leave HBM between AdvectionDiffusion and PressureProjection when obstacles are present.  The *_resident
// entry points run UpdateObstacles, Penalization, kernelUpdateTmpV and ComputeForces (with Obstacle::computeForces, 13079-13115) on the
// blocks cup3d_create_obstacles keeps, all obstacles at once.
// Velocities and tmpV are bit-exact with the reference; the penalisation force / torque sums are reductions (block totals summed in block
// order on the host, cells within a block in tree order on the device); the momenta of UpdateObstacles and the surface sums of
// ComputeForces are added in the reference's own order and are bit-exact per block.
//
// One translation unit per operator, each with its kernels, host half and entry points:
//   obstacles_penalization.hip  cup3d_penalization, cup3d_update_tmpv and their *_resident forms; the shared host helpers below
//   obstacles_update.hip        cup3d_update_obstacles, cup3d_update_obstacles_resident
//   obstacles_forces.hip        cup3d_compute_forces, cup3d_compute_forces_over_ranks and their *_resident forms
//   obstacles_create.hip        cup3d_create_obstacles; the retained set and its plan
//   obstacles_collisions.hip    cup3d_prevent_colliding_obstacles
// This header is theirs alone: what more than one of them uses.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "sim.hpp"
#include "tile.hpp"

namespace cup3d {

struct ObstItems {
  const int32_t *slots;  // [n] block slot of each ObstacleBlock
  const double *geom;    // [n][4]: h, origin[3] of that block (Info::h, Info::origin)
  const double *chi;     // [n][512]
  const double *udef;    // [n][512][3]
};

constexpr int kMomenta = 29;          // M of kernelFinalizeObstacleVel (13748-13777): V, FX FY FZ, TX TY TZ, J0..J5, then with implicit
constexpr int kMomentaExplicit = 13;  // penalisation GfX, GpX GpY GpZ, Gj0..Gj5, GuX GuY GuZ, GaX GaY GaZ
// J3..J5 and Gj3..Gj5 are accumulated with -= (13698-13700, 13720-13722)
constexpr unsigned kMomentaSubtracted = (1u << 10) | (1u << 11) | (1u << 12) | (1u << 20) | (1u << 21) | (1u << 22);

// Every device buffer of the obstacle operators is a Dev<void> sized in bytes, allocated and uploaded with IfEmpty::eight_bytes: an obstacle
// without blocks or surface points still hands the kernels a pointer that is not null.

// ---- host helpers the units share (obstacles_penalization.hip)

// rows[n][4] = h, origin[3] of the listed block slots (Info::h, Info::origin, main.cpp:1066-1068); CUP3D_EINVAL for a slot the sim
// does not hold
int block_geometry(const Sim *s, const int32_t *slots, long n, std::vector<double> &rows);

// the ObstacleBlocks of one obstacle -> device, freed with the four buffers
int stage(const Sim *s, const cup3d_obstacle &o, Dev<void> &slots, Dev<void> &geom, Dev<void> &chi, Dev<void> &udef, ObstItems *it);

// the first `width` columns of rows [n][stride] added in ascending slot order onto total[width]: the reference's loops over
// obstacleBlocks with one thread
void add_rows_in_slot_order(const int32_t *slots, long n, const double *rows, int stride, int width, double *total);

// What one all-reduce carries at most: the in-process communicator of the tests and the host transport refuse more (allreduce(), comm.hip)
constexpr int kAllreducePiece = 16;

// v[n] summed (or maxed) over the ranks, on the stream every RCCL call of the library uses, along with a flag -- 0, or 1 from a rank
// whose local part failed (local_rc != 0; it contributes zeros) -- so that one rank's failure is an error on every rank and leaves none
// inside a collective.  The values cross in pieces of at most kAllreducePiece; the flag is the last value of the FIRST piece, so every
// rank knows the outcome after it and all skip the remaining pieces together.  d_operand: n + 1 doubles on the device.
// Returns local_rc if this rank failed, CUP3D_ECOMM if another did ("who: obstacle k failed on .. other rank(s)", or "who: the call
// failed on another rank" for k < 0), else CUP3D_OK with the totals in v.  A sim whose scalars do not cross ranks: local_rc, v as it is.
int sums_over_ranks(Sim *s, double *d_operand, double *v, int n, bool is_max, int local_rc, const char *who, int k);

// ---- the blocks cup3d_create_obstacles keeps and how the resident operators walk them (obstacles_create.hip)

// How the resident operators (cup3d_update_obstacles_resident, cup3d_penalization_resident, cup3d_update_tmpv_resident) walk the
// retained set; built from the slots_h lists by the first of them to run after a cup3d_create_obstacles.
// Row r = row_base[k] + i stands for block i of obstacle k in the order listed.  The slot-major schedule lists, per distinct slot any
// obstacle holds, in ascending slot order, the rows of that slot in ascending k (an obstacle's slots are distinct: at most one row per
// obstacle): rows sched_rows[sched_first[j] .. sched_first[j + 1]) for the j-th slot.
struct ResidentPlan {
  long rows = 0, nslots = 0;
  std::vector<long> row_base;   // [N + 1]
  Dev<void> obst;                  // ObstItems [N]: the retained slots, geom, chi, udef of every obstacle
  Dev<void> row_obst, row_block;   // int32 [rows]: k and i of a row
  Dev<void> sched_first, sched_rows;  // int32 [nslots + 1], [rows]
  Dev<void> body;                  // double [N][9]: the call's cm, vel, omega of every obstacle
  Dev<void> out;                   // double [rows][29]: the call's block rows ([rows][6] for the penalisation forces)
  size_t bytes = 0;
};

// How cup3d_compute_forces_resident walks the surface of the retained set; built by its first call after a cup3d_create_obstacles, kept
// with the set like the ResidentPlan (which it needs: the obstacles' array pointers and rigid state are that plan's tables).
// A surface row stands for a listed block with surface points, first_h[i + 1] > first_h[i], in obstacle order and then listed order;
// its points are [row_first[r], row_first[r + 1]) of ijk / dchi, which k_retained_surface rebuilds from the retained sdfLab and chi.
// The distinct slots of the surface rows, ascending, are the tiles of a call: row_tile[r] is the place of row r's slot among them, and
// the slot-major schedule lists the rows of tile j, in ascending obstacle order, at sched_rows[sched_first[j] .. sched_first[j + 1]).
// With N obstacles, Rs surface rows and P points the device holds N * 8 + Rs * (5 * 4 + 19 * 8) + 4 + P * (3 * 4 + 3 * 8) bytes; the
// S distinct slots and where their rows begin stay on the host, which cuts the chunks.  Rs = 0: nothing, and nothing is launched.
struct SurfacePlan {
  long rows = 0, ntiles = 0, npoints = 0;  // Rs, S, P
  std::vector<long> row_base;              // [N + 1] first surface row of every obstacle
  std::vector<int32_t> row_slot;           // [Rs] the slot of a row, for the sums in slot order
  std::vector<int32_t> first_h;            // [Rs + 1] = row_first
  std::vector<int32_t> tile_slots;         // [S] ascending
  std::vector<int32_t> sched_first;        // [S + 1]
  Dev<void> sdf;                           // const double *[N]: the retained sdfLab of every obstacle
  Dev<void> row_obst, row_block, row_tile, sched_rows;  // int32 [Rs]
  Dev<void> row_first;                     // int32 [Rs + 1]
  Dev<void> ijk, dchi;                     // int32 [P][3], double [P][3]
  Dev<void> qoi;                           // double [Rs][19]: the blocks' nineteen sums, zero when the plan is built, kept between calls
  size_t bytes = 0;
};

// The ShapeWork buffers of the last successful cup3d_create_obstacles that the collision model and the resident operators read, moved
// here instead of freed.
struct RetainedObstacles {
  struct One {
    long nblocks = 0;
    std::vector<int32_t> slots_h;       // the caller's slot list, for the intersections and the plan
    std::vector<int32_t> first_h;       // [n + 1] the CSR of the obstacle's surface points over its listed blocks, for the surface plan
    Dev<void> slots, geom, sdf, chi, udef;  // [n], [n][4], [n][10][10][10], [n][8][8][8], [n][8][8][8][3] (corrected)
  };
  std::vector<One> obst;
  ResidentPlan *plan = nullptr;  // nullptr until a resident operator asks for it
  SurfacePlan *surface = nullptr;  // nullptr until cup3d_compute_forces_resident asks for it
  size_t bytes = 0;  // counted in Sim::bytes, the plans' included once they exist
  ~RetainedObstacles() { delete plan; delete surface; }
};

struct PlanItems {
  const ObstItems *obst;                  // [N]
  const int32_t *row_obst, *row_block;    // [rows]
  const int32_t *sched_first, *sched_rows;  // [nslots + 1], [rows]
  const double *body;                     // [N][9]: cm, vel, omega
};

// the retained set of a call of `nobst` obstacles, or why there is none
int retained_for(Sim *s, const char *who, int nobst, RetainedObstacles **out);
// the plan of the retained set, built on first use
int resident_plan(Sim *s, RetainedObstacles *R, ResidentPlan **out);
PlanItems plan_items(const ResidentPlan *P);

struct SurfacePlanItems {
  const int32_t *row_obst, *row_block, *row_tile, *row_first, *sched_rows;  // [Rs], [Rs], [Rs], [Rs + 1], [Rs]
  const int32_t *ijk;   // [P][3]
  const double *dchi;   // [P][3]
  double *qoi;          // [Rs][19]
  long npoints;         // P
};
// the surface plan of the retained set, built on first use: the tables, then ijk and dchi by k_retained_surface
int surface_plan(Sim *s, RetainedObstacles *R, SurfacePlan **out);
SurfacePlanItems surface_plan_items(const SurfacePlan *P);

// The plan's tables are written before the launch and only read by the kernels.  Read through the constant address space, a load at a
// wave-uniform index is a scalar load whatever the kernel stores in between, and what it returns -- the row, its obstacle, the obstacle's
// array pointers and rigid state -- stays in scalar registers; as plain global loads next to the stores to vel they would be vector
// loads, and every address formed from them a pair of vector registers.
template <class T>
using Constant = const T __attribute__((address_space(4)));
template <class T>
__device__ __forceinline__ Constant<T> *constant(const T *p) {
  return (Constant<T> *)p;
}
static_assert(sizeof(ObstItems) == 4 * sizeof(unsigned long long), "plan_obstacle reads an ObstItems as four 64-bit words");
__device__ __forceinline__ ObstItems plan_obstacle(const PlanItems &pl, int k) {
  Constant<unsigned long long> *w = constant(reinterpret_cast<const unsigned long long *>(pl.obst)) + 4 * (size_t)k;
  return ObstItems{reinterpret_cast<const int32_t *>(w[0]), reinterpret_cast<const double *>(w[1]), reinterpret_cast<const double *>(w[2]),
                   reinterpret_cast<const double *>(w[3])};
}

}  // namespace cup3d
