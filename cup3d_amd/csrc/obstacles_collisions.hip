// cup3d_prevent_colliding_obstacles.  Penalization::preventCollidingObstacles (main.cpp:14009-14324): the CollisionInfo sums
// (14037-14142) on the device from the blocks cup3d_create_obstacles retained, the two all-reduces and the pair loop with ComputeJ /
// ElasticCollision (13939-14007, 14143-14323) on the host.
// One wavefront per obstacle i, k_fluid_momenta's pattern.  For j = 0..N-1, j != i, it visits the blocks both obstacles hold in ascending
// slot order (the host intersects the two slot lists and uploads, per ordered pair, the index pairs into the two obstacles' retained
// arrays).  Per z-plane every lane evaluates one cell; a ballot of !(iChi <= 0) && !(jChi <= 0) says which cells the reference visits,
// and a plane without one is skipped.  The selected lanes leave their summands in LDS, then lanes 0..13 each add one of iM, iPos*, ivec*,
// jM, jPos*, jvec* over the plane in cell order onto a running total they keep in a register -- the totals run on across the blocks and
// across j, as `coll` does.  Lanes 14 and 15 scan the plane's imag / jmag in the same order with the reference's strict `>` against
// imagmax / jmagmax, which restart at 0 for every j, and take the momentum of a cell that wins from three further rows; coll.iMom* / jMom*
// persist across j when no later cell beats 0, as written.  No tree, no atomic: the 20 values are the reference's
// one-thread loop bit for bit.  The rows of sm are padded by one double as in k_fluid_momenta.
#include "obstacles.hpp"

namespace cup3d {

constexpr int kCollision = 20;  // CollisionInfo, member order of 14015-14034
constexpr int kCollisionRows = 22;  // 14 sums, imag, jmag, iMom[3], jMom[3]

struct CollisionObstacle {
  const double *geom, *sdf, *chi, *udef;  // the retained arrays of this obstacle
  double cm[3], vel[3], omega[3];         // centerOfMass, transVel, angVel
};

struct CollisionItems {
  const CollisionObstacle *obst;  // [N]
  const int32_t *first;           // [N*N+1]: the ordered pair (i, j) owns pairs [first[i*N+j], first[i*N+j+1])
  const int32_t *pairs;           // [.][2]: block index in i's arrays, block index in j's arrays; ascending slot
  int n;
};

// a value every lane of the wavefront holds alike, moved to scalar registers
__device__ __forceinline__ double wave_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
__device__ __forceinline__ const double *wave_uniform(const double *p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const double *)(((unsigned long long)hi << 32) | lo);
}

__global__ void __launch_bounds__(64) k_collision_sums(CollisionItems it, double *__restrict__ sums /* [N][20] */) {
  __shared__ double sm[kCollisionRows][65];
  const int i = blockIdx.x, lane = threadIdx.x;
  const CollisionObstacle *__restrict__ A = it.obst + i;
  const int ix = lane & 7, iy = lane >> 3;
  const double iU0 = wave_uniform(A->vel[0]), iU1 = wave_uniform(A->vel[1]), iU2 = wave_uniform(A->vel[2]);
  const double iomega0 = wave_uniform(A->omega[0]), iomega1 = wave_uniform(A->omega[1]), iomega2 = wave_uniform(A->omega[2]);
  const double iCx = wave_uniform(A->cm[0]), iCy = wave_uniform(A->cm[1]), iCz = wave_uniform(A->cm[2]);
  const double *__restrict__ iGeom = wave_uniform(A->geom), *__restrict__ iSdf = wave_uniform(A->sdf);
  const double *__restrict__ iChi = wave_uniform(A->chi), *__restrict__ iUdef = wave_uniform(A->udef);
  double acc = 0.0;  // lanes 0..13: the running sum of quantity `lane`; lane 14: imagmax, lane 15: jmagmax
  __shared__ double won[2][3];  // coll.iMom*, coll.jMom*: lane 14's and lane 15's own, no other lane touches them
  if (lane == 14 || lane == 15) won[lane - 14][0] = won[lane - 14][1] = won[lane - 14][2] = 0.0;
  const int mrow = 16 + 3 * (lane & 1);  // lane 14 reads the rows of iMom, lane 15 those of jMom
  for (int j = 0; j < it.n; ++j) {
    if (j == i) continue;
    const CollisionObstacle *__restrict__ B = it.obst + j;
    const double jU0 = wave_uniform(B->vel[0]), jU1 = wave_uniform(B->vel[1]), jU2 = wave_uniform(B->vel[2]);
    const double jomega0 = wave_uniform(B->omega[0]), jomega1 = wave_uniform(B->omega[1]), jomega2 = wave_uniform(B->omega[2]);
    const double jCx = wave_uniform(B->cm[0]), jCy = wave_uniform(B->cm[1]), jCz = wave_uniform(B->cm[2]);
    const double *__restrict__ jSdf = wave_uniform(B->sdf), *__restrict__ jChi = wave_uniform(B->chi), *__restrict__ jUdef = wave_uniform(B->udef);
    if (lane >= 14) acc = 0.0;  // imagmax = jmagmax = 0 (14063-14064)
    const int q0 = __builtin_amdgcn_readfirstlane(it.first[i * it.n + j]), q1 = __builtin_amdgcn_readfirstlane(it.first[i * it.n + j + 1]);
    for (int q = q0; q < q1; ++q) {
      const int bi = __builtin_amdgcn_readfirstlane(it.pairs[2 * q]), bj = __builtin_amdgcn_readfirstlane(it.pairs[2 * q + 1]);
      const double h = wave_uniform(iGeom[4 * bi]), ox = wave_uniform(iGeom[4 * bi + 1]), oy = wave_uniform(iGeom[4 * bi + 2]), oz = wave_uniform(iGeom[4 * bi + 3]);
      const double *__restrict__ iSDF = iSdf + (size_t)bi * 1000;
      const double *__restrict__ jSDF = jSdf + (size_t)bj * 1000;
#pragma unroll 1
      for (int iz = 0; iz < 8; ++iz) {
        const int c = iz * 64 + lane;
        const double iX = iChi[(size_t)bi * 512 + c], jX = jChi[(size_t)bj * 512 + c];
        const bool visited = !(iX <= 0.0) && !(jX <= 0.0);  // `if (iChi[z][y][x] <= 0.0 || jChi[z][y][x] <= 0.0) continue;`
        const unsigned long long mask = __ballot(visited);
        if (mask == 0ull) continue;  // the same in every lane
        if (visited) {
          const double p[3] = {ox + h * (ix + 0.5), oy + h * (iy + 0.5), oz + h * (iz + 0.5)};
          sm[0][lane] = 1.0;
          sm[1][lane] = p[0];
          sm[2][lane] = p[1];
          sm[3][lane] = p[2];
          sm[7][lane] = 1.0;
          sm[8][lane] = p[0];
          sm[9][lane] = p[1];
          sm[10][lane] = p[2];
          const double *iU = iUdef + ((size_t)bi * 512 + c) * 3;
          const double iMomX = iU0 + iomega1 * (p[2] - iCz) - iomega2 * (p[1] - iCy) + iU[0];
          const double iMomY = iU1 + iomega2 * (p[0] - iCx) - iomega0 * (p[2] - iCz) + iU[1];
          const double iMomZ = iU2 + iomega0 * (p[1] - iCy) - iomega1 * (p[0] - iCx) + iU[2];
          sm[14][lane] = iMomX * iMomX + iMomY * iMomY + iMomZ * iMomZ;  // imag
          sm[16][lane] = iMomX;
          sm[17][lane] = iMomY;
          sm[18][lane] = iMomZ;
          __builtin_amdgcn_sched_barrier(0);  // one group's loads at a time: 64 registers, eight wavefronts per SIMD
          const double *jU = jUdef + ((size_t)bj * 512 + c) * 3;
          const double jMomX = jU0 + jomega1 * (p[2] - jCz) - jomega2 * (p[1] - jCy) + jU[0];
          const double jMomY = jU1 + jomega2 * (p[0] - jCx) - jomega0 * (p[2] - jCz) + jU[1];
          const double jMomZ = jU2 + jomega0 * (p[1] - jCy) - jomega1 * (p[0] - jCx) + jU[2];
          sm[15][lane] = jMomX * jMomX + jMomY * jMomY + jMomZ * jMomZ;  // jmag
          sm[19][lane] = jMomX;
          sm[20][lane] = jMomY;
          sm[21][lane] = jMomZ;
          __builtin_amdgcn_sched_barrier(0);  // one group's loads at a time: 64 registers, eight wavefronts per SIMD
          const int s0 = ((iz + 1) * 10 + (iy + 1)) * 10 + (ix + 1);  // sdfLab[z+1][y+1][x+1]
          const double ivecX = iSDF[s0 + 1] - iSDF[s0 - 1], ivecY = iSDF[s0 + 10] - iSDF[s0 - 10], ivecZ = iSDF[s0 + 100] - iSDF[s0 - 100];
          const double normi = 1.0 / (sqrt(ivecX * ivecX + ivecY * ivecY + ivecZ * ivecZ) + 1e-21);
          sm[4][lane] = ivecX * normi;
          sm[5][lane] = ivecY * normi;
          sm[6][lane] = ivecZ * normi;
          __builtin_amdgcn_sched_barrier(0);  // one group's loads at a time: 64 registers, eight wavefronts per SIMD
          const double jvecX = jSDF[s0 + 1] - jSDF[s0 - 1], jvecY = jSDF[s0 + 10] - jSDF[s0 - 10], jvecZ = jSDF[s0 + 100] - jSDF[s0 - 100];
          const double normj = 1.0 / (sqrt(jvecX * jvecX + jvecY * jvecY + jvecZ * jvecZ) + 1e-21);
          sm[11][lane] = jvecX * normj;
          sm[12][lane] = jvecY * normj;
          sm[13][lane] = jvecZ * normj;
        }
        __syncthreads();
        if (lane < 16) {
#pragma unroll 1
          for (unsigned long long m = mask; m; m &= m - 1ull) {  // the visited cells in ascending order, i.e. z, y, x
            const int k = __ffsll((long long)m) - 1;
            const double x = sm[lane][k];
            if (lane < 14) {
              acc += x;
            } else if (x > acc) {  // 14120-14125, 14133-14138
              acc = x;
              won[lane - 14][0] = sm[mrow][k];
              won[lane - 14][1] = sm[mrow + 1][k];
              won[lane - 14][2] = sm[mrow + 2][k];
            }
          }
        }
        __syncthreads();
      }
    }
  }
  // lane -> member of CollisionInfo: iM iPos[3] | iMom[3] | ivec[3] jM jPos[3] | jMom[3] | jvec[3]
  double *out = sums + (size_t)i * kCollision;
  if (lane < 4) out[lane] = acc;
  else if (lane < 11) out[lane + 3] = acc;
  else if (lane < 14) out[lane + 6] = acc;
  else if (lane < 16) {
    const int at = lane == 14 ? 4 : 14;
    out[at] = won[lane - 14][0];
    out[at + 1] = won[lane - 14][1];
    out[at + 2] = won[lane - 14][2];
  }
}

namespace {
// ComputeJ (13939-13966)
void compute_j(const double *Rc, const double *R, const double *N, const double *I, double *J) {
  const double m00 = I[0], m01 = I[3], m02 = I[4], m11 = I[1], m12 = I[5], m22 = I[2];
  double a00 = m22 * m11 - m12 * m12;
  double a01 = m02 * m12 - m22 * m01;
  double a02 = m01 * m12 - m02 * m11;
  double a11 = m22 * m00 - m02 * m02;
  double a12 = m01 * m02 - m00 * m12;
  double a22 = m00 * m11 - m01 * m01;
  const double determinant = 1.0 / ((m00 * a00) + (m01 * a01) + (m02 * a02));
  a00 *= determinant;
  a01 *= determinant;
  a02 *= determinant;
  a11 *= determinant;
  a12 *= determinant;
  a22 *= determinant;
  const double aux_0 = (Rc[1] - R[1]) * N[2] - (Rc[2] - R[2]) * N[1];
  const double aux_1 = (Rc[2] - R[2]) * N[0] - (Rc[0] - R[0]) * N[2];
  const double aux_2 = (Rc[0] - R[0]) * N[1] - (Rc[1] - R[1]) * N[0];
  J[0] = a00 * aux_0 + a01 * aux_1 + a02 * aux_2;
  J[1] = a01 * aux_0 + a11 * aux_1 + a12 * aux_2;
  J[2] = a02 * aux_0 + a12 * aux_1 + a22 * aux_2;
}

// ElasticCollision (13967-14007)
void elastic_collision(double m1, double m2, const double *I1, const double *I2, const double *v1, const double *v2, const double *o1, const double *o2,
                       const double *C1, const double *C2, double NX, double NY, double NZ, double CX, double CY, double CZ, const double *vc1,
                       const double *vc2, double *hv1, double *hv2, double *ho1, double *ho2) {
  const double e = 1.0;
  const double N[3] = {NX, NY, NZ};
  const double C[3] = {CX, CY, CZ};
  const double k1[3] = {N[0] / m1, N[1] / m1, N[2] / m1};
  const double k2[3] = {-N[0] / m2, -N[1] / m2, -N[2] / m2};
  double J1[3], J2[3];
  compute_j(C, C1, N, I1, J1);
  compute_j(C, C2, N, I2, J2);
  const double nom = (e + 1) * ((vc1[0] - vc2[0]) * N[0] + (vc1[1] - vc2[1]) * N[1] + (vc1[2] - vc2[2]) * N[2]);
  const double denom = -(1.0 / m1 + 1.0 / m2) +
                       -((J1[1] * (C[2] - C1[2]) - J1[2] * (C[1] - C1[1])) * N[0] + (J1[2] * (C[0] - C1[0]) - J1[0] * (C[2] - C1[2])) * N[1] +
                         (J1[0] * (C[1] - C1[1]) - J1[1] * (C[0] - C1[0])) * N[2]) -
                       ((J2[1] * (C[2] - C2[2]) - J2[2] * (C[1] - C2[1])) * N[0] + (J2[2] * (C[0] - C2[0]) - J2[0] * (C[2] - C2[2])) * N[1] +
                        (J2[0] * (C[1] - C2[1]) - J2[1] * (C[0] - C2[0])) * N[2]);
  const double impulse = nom / (denom + 1e-21);
  for (int d = 0; d < 3; ++d) {
    hv1[d] = v1[d] + k1[d] * impulse;
    hv2[d] = v2[d] + k2[d] * impulse;
    ho1[d] = o1[d] + J1[d] * impulse;
    ho2[d] = o2[d] - J2[d] * impulse;
  }
}
}  // namespace

}  // namespace cup3d

using namespace cup3d;

extern "C" int cup3d_prevent_colliding_obstacles(cup3d_sim_t *h, double dt, int nobst, cup3d_obstacle_collision *obst, int32_t *collided, int *ncollided,
                                                 int *any) {
  if (!h || nobst < 0) return CUP3D_EINVAL;
  if (nobst == 0) return dt > 0 ? CUP3D_OK : CUP3D_EINVAL;
  Sim *s = reinterpret_cast<Sim *>(h);
  const size_t N = (size_t)nobst;
  const bool cross = scalars_cross_ranks(s);
  std::vector<double> coll(kCollision * N, 0.0);  // collisions[i], then `buffer`
  // what this rank can get wrong travels with the first all-reduce, so that the other ranks are not left inside it
  auto local_part = [&]() -> int {
    if (!(dt > 0) || !obst || !ncollided || !any) { set_error("cup3d_prevent_colliding_obstacles: dt <= 0 or a null argument"); return CUP3D_EINVAL; }
    RetainedObstacles *R;
    int rc;
    if ((rc = retained_for(s, "cup3d_prevent_colliding_obstacles", nobst, &R))) return rc;
    // per obstacle the positions of its blocks in ascending slot order; per ordered pair (i, j) the blocks both hold
    std::vector<std::vector<int32_t>> order(N);
    for (size_t k = 0; k < N; ++k) {
      const std::vector<int32_t> &sl = R->obst[k].slots_h;
      order[k].resize(sl.size());
      for (size_t b = 0; b < sl.size(); ++b) order[k][b] = (int32_t)b;
      std::stable_sort(order[k].begin(), order[k].end(), [&](int32_t a, int32_t b) { return sl[a] < sl[b]; });
    }
    std::vector<int32_t> first(N * N + 1, 0), pairs;
    for (size_t i = 0; i < N; ++i)
      for (size_t j = 0; j < N; ++j) {
        if (i != j) {
          const std::vector<int32_t> &si = R->obst[i].slots_h, &sj = R->obst[j].slots_h;
          size_t a = 0, b = 0;
          while (a < order[i].size() && b < order[j].size()) {
            const int32_t x = si[order[i][a]], y = sj[order[j][b]];
            if (x < y) ++a;
            else if (y < x) ++b;
            else { pairs.push_back(order[i][a]); pairs.push_back(order[j][b]); ++a; ++b; }
          }
        }
        first[i * N + j + 1] = (int32_t)(pairs.size() / 2);
      }
    std::vector<CollisionObstacle> co(N);
    for (size_t k = 0; k < N; ++k) {
      const RetainedObstacles::One &o = R->obst[k];
      co[k].geom = o.geom.as<const double>();
      co[k].sdf = o.sdf.as<const double>();
      co[k].chi = o.chi.as<const double>();
      co[k].udef = o.udef.as<const double>();
      for (int d = 0; d < 3; ++d) { co[k].cm[d] = obst[k].cm[d]; co[k].vel[d] = obst[k].vel[d]; co[k].omega[d] = obst[k].omega[d]; }
    }
    Dev<void> d_obst, d_first, d_pairs, d_sums;
    if ((rc = d_obst.upload(co.data(), N * sizeof(CollisionObstacle), stream(), IfEmpty::eight_bytes)) || (rc = d_first.upload(first.data(), first.size() * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) ||
        (rc = d_pairs.upload(pairs.data(), pairs.size() * sizeof(int32_t), stream(), IfEmpty::eight_bytes)) || (rc = d_sums.alloc(coll.size() * sizeof(double), IfEmpty::eight_bytes)))
      return rc;
    const CollisionItems it{d_obst.as<const CollisionObstacle>(), d_first.as<const int32_t>(), d_pairs.as<const int32_t>(), nobst};
    {
      ProfileScope ps("collision_sums");
      hipLaunchKernelGGL(k_collision_sums, dim3((unsigned)N), dim3(64), 0, stream(), it, d_sums.as<double>());
    }
    CUP3D_HIP(hipGetLastError());
    CUP3D_HIP(hipMemcpyAsync(coll.data(), d_sums.get(), coll.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    CUP3D_HIP(hipStreamSynchronize(stream()));  // co, first and pairs are locals
    stats_field_download(coll.size() * sizeof(double));
    return CUP3D_OK;
  };
  int rc = local_part();
  if (rc) std::fill(coll.begin(), coll.end(), 0.0);
  // buffermax (14144-14151), MPI_MAX over the ranks (14152); maxi / maxj of 14156-14159 are the same expressions
  std::vector<double> own_max(2 * N), buffermax(2 * N);
  for (size_t i = 0; i < N; ++i) {
    const double *c = &coll[kCollision * i];
    own_max[2 * i] = c[4] * c[4] + c[5] * c[5] + c[6] * c[6];
    own_max[2 * i + 1] = c[14] * c[14] + c[15] * c[15] + c[16] * c[16];
  }
  buffermax = own_max;
  Dev<void> red;  // the all-reduce operand of this call: the 2 N maxima and the error flag (sums_over_ranks), then the 20 N sums
  if (cross) {
    const int rc2 = red.alloc(std::max(2 * N + 1, kCollision * N) * sizeof(double), IfEmpty::eight_bytes);
    if (rc2) return rc ? rc : rc2;
  }
  if ((rc = sums_over_ranks(s, red.as<double>(), buffermax.data(), (int)(2 * N), true, rc, "cup3d_prevent_colliding_obstacles", -1))) return rc;
  for (size_t i = 0; i < N; ++i) {  // 14154-14182
    double *c = &coll[kCollision * i];
    const bool iok = std::fabs(own_max[2 * i] - buffermax[2 * i]) < 1e-10;
    const bool jok = std::fabs(own_max[2 * i + 1] - buffermax[2 * i + 1]) < 1e-10;
    for (int d = 0; d < 3; ++d) {
      c[4 + d] = iok ? c[4 + d] : 0;
      c[14 + d] = jok ? c[14 + d] : 0;
    }
  }
  if (cross) {  // MPI_SUM of 20 N (14183)
    double *d = red.as<double>();
    hipStream_t cs = scalar_stream(s);
    int rc2;
    CUP3D_HIP(hipMemcpyAsync(d, coll.data(), coll.size() * sizeof(double), hipMemcpyHostToDevice, cs));
    for (size_t at = 0; at < coll.size(); at += kAllreducePiece)
      if ((rc2 = allreduce(s, d + at, (int)std::min<size_t>(kAllreducePiece, coll.size() - at), false, cs))) return rc2;
    CUP3D_HIP(hipMemcpyAsync(coll.data(), d, coll.size() * sizeof(double), hipMemcpyDeviceToHost, cs));
    CUP3D_HIP(hipStreamSynchronize(cs));
  }
  // 14208-14323 with one thread: pairs i < j in order, later pairs see the velocities earlier pairs wrote.  The caller's structs are
  // written only once every pair has passed.
  std::vector<cup3d_obstacle_collision> out(obst, obst + N);
  std::vector<int32_t> ids;
  bool hit = false;
  for (size_t i = 0; i < N; ++i)
    for (size_t j = i + 1; j < N; ++j) {
      cup3d_obstacle_collision &si = out[i], &sj = out[j];
      const double m1 = si.mass, m2 = sj.mass;
      const double v1[3] = {si.vel[0], si.vel[1], si.vel[2]}, o1[3] = {si.omega[0], si.omega[1], si.omega[2]};
      const double v2[3] = {sj.vel[0], sj.vel[1], sj.vel[2]}, o2[3] = {sj.omega[0], sj.omega[1], sj.omega[2]};
      const double *I1 = si.J, *I2 = sj.J, *C1 = si.cm, *C2 = sj.cm;
      const double *c = &coll[kCollision * i], *co = &coll[kCollision * j];
      const double iM = c[0], iPosX = c[1], iPosY = c[2], iPosZ = c[3], iMomX = c[4], iMomY = c[5], iMomZ = c[6], ivecX = c[7], ivecY = c[8], ivecZ = c[9];
      const double jM = c[10], jPosX = c[11], jPosY = c[12], jPosZ = c[13], jMomX = c[14], jMomY = c[15], jMomZ = c[16], jvecX = c[17], jvecY = c[18],
                   jvecZ = c[19];
      const double tolerance = 0.001;
      if (iM < tolerance || jM < tolerance) continue;
      if (co[0] < tolerance || co[10] < tolerance) continue;
      if (std::fabs(iPosX / iM - co[1] / co[0]) > 0.2 || std::fabs(iPosY / iM - co[2] / co[0]) > 0.2 || std::fabs(iPosZ / iM - co[3] / co[0]) > 0.2) continue;
      hit = true;  // sim.bCollision
      ids.push_back((int32_t)i);
      ids.push_back((int32_t)j);
      const double norm_i = std::sqrt(ivecX * ivecX + ivecY * ivecY + ivecZ * ivecZ);
      const double norm_j = std::sqrt(jvecX * jvecX + jvecY * jvecY + jvecZ * jvecZ);
      const double mX = ivecX / norm_i - jvecX / norm_j;
      const double mY = ivecY / norm_i - jvecY / norm_j;
      const double mZ = ivecZ / norm_i - jvecZ / norm_j;
      const double inorm = 1.0 / std::sqrt(mX * mX + mY * mY + mZ * mZ);
      const double NX = mX * inorm, NY = mY * inorm, NZ = mZ * inorm;
      const double projVel = (jMomX - iMomX) * NX + (jMomY - iMomY) * NY + (jMomZ - iMomZ) * NZ;
      if (projVel <= 0) continue;
      const double inv_iM = 1.0 / iM, inv_jM = 1.0 / jM;
      const double iPX = iPosX * inv_iM, iPY = iPosY * inv_iM, iPZ = iPosZ * inv_iM;
      const double jPX = jPosX * inv_jM, jPY = jPosY * inv_jM, jPZ = jPosZ * inv_jM;
      const double CX = 0.5 * (iPX + jPX), CY = 0.5 * (iPY + jPY), CZ = 0.5 * (iPZ + jPZ);
      const double vc1[3] = {iMomX, iMomY, iMomZ}, vc2[3] = {jMomX, jMomY, jMomZ};
      double ho1[3], ho2[3], hv1[3], hv2[3];
      const bool iforced = si.forced[0] || si.forced[1] || si.forced[2];
      const bool jforced = sj.forced[0] || sj.forced[1] || sj.forced[2];
      const double m1_i = iforced ? 1e10 * m1 : m1;
      const double m2_j = jforced ? 1e10 * m2 : m2;
      elastic_collision(m1_i, m2_j, I1, I2, v1, v2, o1, o2, C1, C2, NX, NY, NZ, CX, CY, CZ, vc1, vc2, hv1, hv2, ho1, ho2);
      for (int d = 0; d < 3; ++d) {
        si.vel[d] = si.collision_vel[d] = hv1[d];
        sj.vel[d] = sj.collision_vel[d] = hv2[d];
        si.omega[d] = si.collision_omega[d] = ho1[d];
        sj.omega[d] = sj.collision_omega[d] = ho2[d];
      }
      si.collision_counter = 0.01 * dt;
      sj.collision_counter = 0.01 * dt;
    }
  for (size_t i = 0; i < N; ++i) {
    obst[i] = out[i];
    for (int q = 0; q < kCollision; ++q) obst[i].sums[q] = coll[kCollision * i + q];
  }
  if (collided)
    for (size_t q = 0; q < ids.size(); ++q) collided[q] = ids[q];
  *ncollided = (int)ids.size();
  *any = hit ? 1 : 0;
  return CUP3D_OK;
}
