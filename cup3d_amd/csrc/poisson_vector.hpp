// The work vectors, the plain (grid-stride) vector kernels and the reductions that end on the host.
// Part of poisson.hip's translation unit: included there once, in order; not a stand-alone header.
#pragma once

namespace cup3d {

enum { PHAT, RHAT, SHAT, WHAT, ZHAT, QHAT, S_, W_, Z_, T_, V_, Q_, R_, Y_, X_, R0, B_, XOPT, NVEC };

// ------------------------------------------------------------------ fused BiCGSTAB vector kernels
struct Vecs {
  double *v[NVEC];
  const double *xin;  // where the second loop reads x from: v[X_], or the x_opt snapshot right after one was taken (see solve())
};

#define GRID_STRIDE(j, n) for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < (n); j += (long)gridDim.x * 256)
// 16 B per lane (double2): n is a multiple of 512
#define GRID_STRIDE2(j, n) for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < (n) / 2; j += (long)gridDim.x * 256)
// NT: nontemporal (streaming) accesses -- every vector is touched once per launch and the 19 GB working set cannot stay in L2
template <bool NT>
__device__ __forceinline__ double2 ld2(const double *v, long j) {
  if constexpr (!NT) return reinterpret_cast<const double2 *>(v)[j];
  const double *p = v + 2 * j;
  double2 r;
  r.x = __builtin_nontemporal_load(p);
  r.y = __builtin_nontemporal_load(p + 1);
  return r;
}
template <bool NT>
__device__ __forceinline__ void st2(double *v, long j, double2 val) {
  if constexpr (!NT) { reinterpret_cast<double2 *>(v)[j] = val; return; }
  double *p = v + 2 * j;
  __builtin_nontemporal_store(val.x, p);
  __builtin_nontemporal_store(val.y, p + 1);
}
#define LD2(v) ld2<NT>(v, j)
#define ST2(v, val) st2<NT>(v, j, val)
__device__ __forceinline__ double2 operator+(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 operator-(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 operator*(double s, double2 a) { return make_double2(s * a.x, s * a.y); }
__device__ __forceinline__ double dot2(double2 a, double2 b, double acc) { acc += a.x * b.x; acc += a.y * b.y; return acc; }

// b = r = rhs, x = pres   (main.cpp:14408-14415)
__global__ void __launch_bounds__(256) k_solver_init(Vecs V, const double *__restrict__ rhs, const double *__restrict__ pres, long n) {
  GRID_STRIDE(j, n) { const double b = rhs[j]; V.v[B_][j] = b; V.v[R_][j] = b; V.v[X_][j] = pres[j]; }
}
// r0 = r - r0 ; r = r0   (14419-14422)
__global__ void __launch_bounds__(256) k_resid0(Vecs V, long n) {
  GRID_STRIDE(j, n) { const double d = V.v[R_][j] - V.v[R0][j]; V.v[R0][j] = d; V.v[R_][j] = d; }
}
// r0.r0, r0.w  (14436-14440 and 14578-14581)
__global__ void __launch_bounds__(256) k_dots_r0(Vecs V, long n, RedOut ro) {
  double acc[2] = {0, 0};
  GRID_STRIDE(j, n) { const double a = V.v[R0][j]; acc[0] += a * a; acc[1] += a * V.v[W_][j]; }
  grid_sum_finish<2>(acc, ro);
}
// first fused loop, k % 50 != 0   (14454-14464)
template <bool NT>
__global__ void __launch_bounds__(256) k_loop1(Vecs V, long n, double alpha, double beta, double omega, RedOut ro) {
  double acc[2] = {0, 0};
  GRID_STRIDE2(j, n) {
    const double2 rhat = LD2(V.v[RHAT]), w = LD2(V.v[W_]), shat0 = LD2(V.v[SHAT]), z0 = LD2(V.v[Z_]);
    const double2 phat = rhat + beta * (LD2(V.v[PHAT]) - omega * shat0);
    const double2 s = w + beta * (LD2(V.v[S_]) - omega * z0);
    const double2 shat = LD2(V.v[WHAT]) + beta * (shat0 - omega * LD2(V.v[ZHAT]));
    const double2 z = LD2(V.v[T_]) + beta * (z0 - omega * LD2(V.v[V_]));
    const double2 q = LD2(V.v[R_]) - alpha * s;
    const double2 qhat = rhat - alpha * shat;
    const double2 y = w - alpha * z;
    ST2(V.v[PHAT], phat); ST2(V.v[S_], s); ST2(V.v[SHAT], shat); ST2(V.v[Z_], z); ST2(V.v[Q_], q); ST2(V.v[QHAT], qhat); ST2(V.v[Y_], y);
    acc[0] = dot2(q, y, acc[0]);
    acc[1] = dot2(y, y, acc[1]);
  }
  grid_sum_finish<2>(acc, ro);
}
// k % 50 == 0 variants   (14467-14480)
__global__ void __launch_bounds__(256) k_loop1_phat(Vecs V, long n, double beta, double omega) {
  GRID_STRIDE(j, n) V.v[PHAT][j] = V.v[RHAT][j] + beta * (V.v[PHAT][j] - omega * V.v[SHAT][j]);
}
__global__ void __launch_bounds__(256) k_loop1_tail(Vecs V, long n, double alpha, RedOut ro) {
  double acc[2] = {0, 0};
  GRID_STRIDE(j, n) {
    const double q = V.v[R_][j] - alpha * V.v[S_][j];
    const double qhat = V.v[RHAT][j] - alpha * V.v[SHAT][j];
    const double y = V.v[W_][j] - alpha * V.v[Z_][j];
    V.v[Q_][j] = q; V.v[QHAT][j] = qhat; V.v[Y_][j] = y;
    acc[0] += q * y;
    acc[1] += y * y;
  }
  grid_sum_finish<2>(acc, ro);
}
// second fused loop, k % 50 != 0   (14503-14515)
template <bool NT>
__global__ void __launch_bounds__(256) k_loop2(Vecs V, long n, double alpha, double omega, RedOut ro) {
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  GRID_STRIDE2(j, n) {
    const double2 qhat = LD2(V.v[QHAT]), y = LD2(V.v[Y_]), r0 = LD2(V.v[R0]);
    const double2 x = LD2(V.xin) + alpha * LD2(V.v[PHAT]) + omega * qhat;
    const double2 r = LD2(V.v[Q_]) - omega * y;
    const double2 rhat = qhat - omega * (LD2(V.v[WHAT]) - alpha * LD2(V.v[ZHAT]));
    const double2 w = y - omega * (LD2(V.v[T_]) - alpha * LD2(V.v[V_]));
    ST2(V.v[X_], x); ST2(V.v[R_], r); ST2(V.v[RHAT], rhat); ST2(V.v[W_], w);
    acc[0] = dot2(r0, r, acc[0]);
    acc[1] = dot2(r0, w, acc[1]);
    acc[2] = dot2(r0, LD2(V.v[S_]), acc[2]);
    acc[3] = dot2(r0, LD2(V.v[Z_]), acc[3]);
    acc[4] = dot2(r, r, acc[4]);    // norm_1
    acc[5] = dot2(r0, r0, acc[5]);  // norm_2
    acc[6] = dot2(r, r, acc[6]);    // norm
  }
  grid_sum_finish<7>(acc, ro);
}
// k % 50 == 0 variants   (14518-14537)
__global__ void __launch_bounds__(256) k_loop2_x(Vecs V, long n, double alpha, double omega) {
  GRID_STRIDE(j, n) V.v[X_][j] = V.xin[j] + alpha * V.v[PHAT][j] + omega * V.v[QHAT][j];
}
__global__ void __launch_bounds__(256) k_true_resid(Vecs V, long n) {
  GRID_STRIDE(j, n) V.v[R_][j] = V.v[B_][j] - V.v[R_][j];
}
// q.y, y.y of the refresh (14478-14480) from the q and y that k_refresh<kRefZ> stored: k_loop1_tail's two sums, thread for thread and term for term
__global__ void __launch_bounds__(256) k_dots2(Vecs V, long n, RedOut ro) {
  double acc[2] = {0, 0};
  GRID_STRIDE(j, n) {
    const double q = V.v[Q_][j], y = V.v[Y_][j];
    acc[0] += q * y;
    acc[1] += y * y;
  }
  grid_sum_finish<2>(acc, ro);
}
__global__ void __launch_bounds__(256) k_dots7(Vecs V, long n, RedOut ro) {
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  GRID_STRIDE(j, n) {
    const double r0 = V.v[R0][j], r = V.v[R_][j];
    acc[0] += r0 * r;
    acc[1] += r0 * V.v[W_][j];
    acc[2] += r0 * V.v[S_][j];
    acc[3] += r0 * V.v[Z_][j];
    acc[4] += r * r;
    acc[5] += r0 * r0;
    acc[6] += r * r;
  }
  grid_sum_finish<7>(acc, ro);
}
__global__ void __launch_bounds__(256) k_copy(const double *__restrict__ src, double *__restrict__ dst, long n) {
  GRID_STRIDE(j, n) dst[j] = src[j];
}
__global__ void k_set_one(double *p, size_t i, double v) { p[i] = v; }
// cup3d_poisson_path_checksum: vector `vec` of block blockIdx.x, a function of (vec, level, global cell index) -- integer hashing and one
// exact scaling, so the bits are the same on every device and under every sharding; values in [-1, 1)
__global__ void __launch_bounds__(256) k_selfcheck_fill(double *__restrict__ v, int vec, const int32_t *__restrict__ index, const int32_t *__restrict__ level, int level0) {
  const int b = blockIdx.x;
  const unsigned lv = (unsigned)(level ? level[b] : level0);
  for (int c = threadIdx.x; c < 512; c += 256) {
    const unsigned gx = (unsigned)index[3 * b] * 8u + (c & 7), gy = (unsigned)index[3 * b + 1] * 8u + ((c >> 3) & 7), gz = (unsigned)index[3 * b + 2] * 8u + (c >> 6);
    unsigned hsh = gx * 73856093u ^ gy * 19349663u ^ gz * 83492791u ^ (unsigned)(vec + 1) * 2654435761u ^ (lv + 1u) * 40503u;
    hsh ^= hsh >> 15; hsh *= 2246822519u; hsh ^= hsh >> 13; hsh *= 3266489917u; hsh ^= hsh >> 16;
    // a smooth part (so that the block solve sees a right-hand side like the solver's) + the hashed part
    const double smooth = (double)((int)((gx + 2 * gy + 3 * gz + 5u * (unsigned)vec) & 63u) - 32) * (1.0 / 64.0);
    v[(size_t)b * 512 + c] = 0.5 * smooth + (double)((int)(hsh & 0xfffffu) - 0x80000) * (1.0 / 2097152.0);
  }
}
// lhs -= tmpV.u[0] ; pres = 0   (main.cpp:15090-15099)
__global__ void __launch_bounds__(256) k_sub_divp(double *__restrict__ lhs, const double *__restrict__ tmpV, double *__restrict__ pres, long n) {
  GRID_STRIDE(j, n) { lhs[j] -= tmpV[(j >> 9) * 1536 + (j & 511)]; pres[j] = 0; }
}
// sum(p*vv), sum(vv)   (15111-15121)
__global__ void __launch_bounds__(256) k_mean_dots(const double *__restrict__ p, long n, double vv, const double *__restrict__ hb,
                                                   RedOut ro) {
  double acc[2] = {0, 0};
  GRID_STRIDE(j, n) {
    if (hb) { const double h = hb[j >> 9]; vv = h * h * h; }
    acc[0] += p[j] * vv; acc[1] += vv;
  }
  grid_sum_finish<2>(acc, ro);
}
// p -= avg ; (p += pOld)   (15127-15145)
__global__ void __launch_bounds__(256) k_shift_mean(double *__restrict__ p, const double *__restrict__ pold, long n, double avg) {
  GRID_STRIDE(j, n) { double v = p[j] - avg; if (pold) v += pold[j]; p[j] = v; }
}

static unsigned vec_groups_simple(long n) {
  long g = (n + 255) / 256;
  return (unsigned)(g > 2048 ? 2048 : g);
}
static unsigned vec_groups(long n) {
  long g = (n + 255) / 256;
  // One 256-thread workgroup per CU: with 18 concurrent streams per loop, fewer in-flight wavefronts keep the DRAM pages of each
  // stream open longer -- measured at 512^3 (profiles/r01/probe_bicgstab_loops_512.jsonl): 2048 groups 3.50 / 3.42 ms for the two
  // fused loops, 512 groups 3.18 / 2.86, 256 groups 3.08 / 2.82 (6.3 / 6.1 TB/s, the copy ceiling of the chip).
  const int cap = debug_option("vec_groups") > 0 ? debug_option("vec_groups") : 256;  // tuning knob; <= Sim::max_groups
  return (unsigned)(g > cap ? cap : g);
}

// several ranks: the all-reduced totals (device) -> the pinned host mirror, then the sequence word the host spins on
__global__ void k_publish_totals(const double *__restrict__ d, int k, double *__restrict__ host, unsigned *flag, unsigned seq) {
  if ((int)threadIdx.x < k) host[threadIdx.x] = d[threadIdx.x];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Reducer {
  Sim *s;
  // where the kernel that ends with grid_sum_finish puts its totals: d_red always; the pinned host mirror directly when no
  // all-reduce has to run in between
  bool direct() const { return !(s->grid->nranks > 1 || (debug_option("force_allreduce") && comm())); }
  // The totals reach the host through pinned memory followed by a sequence word that wait() spins on -- a few microseconds instead
  // of the wake-up latency of hipEventSynchronize, which at <= 256^3 per GPU (the 8-GPU share of the 512^3 workload) is what the LHS
  // enqueued behind the reduction no longer hides.  direct: written by the reducing kernel itself; several ranks: by
  // k_publish_totals behind the all-reduce on the communication stream
  RedOut out() {
    if (!direct()) return RedOut{s->d_partials, s->d_counters, s->d_red, nullptr, nullptr, 0u};
    return RedOut{s->d_partials, s->d_counters, s->d_red, s->h_red_dev, reinterpret_cast<unsigned *>(s->h_red_dev + 16), ++s->red_seq};
  }
  // the k totals are in d_red when the work enqueued so far completes: all-reduce (communication stream), start the read-back
  int begin(int k) {
    if (direct()) {
      CUP3D_HIP(hipEventRecord(s->ev_a, stream()));
      return CUP3D_OK;
    }
    // MPI_Iallreduce (14486, 14546): on the communication stream, so that the preconditioner + LHS enqueued next on the compute
    // stream overlap it; every RCCL call of the library is issued from that one stream, in the same order on all ranks
    hipStream_t cs = scalar_stream(s);
    if (cs != stream()) {
      CUP3D_HIP(hipEventRecord(s->ev_b, stream()));
      CUP3D_HIP(hipStreamWaitEvent(cs, s->ev_b, 0));
    }
    ProfileScope pc("comm_allreduce", cs);
    int rc = allreduce(s, s->d_red, k, false, cs);
    if (rc) return rc;
    hipLaunchKernelGGL(k_publish_totals, dim3(1), dim3(64), 0, cs, (const double *)s->d_red, k, s->h_red_dev, reinterpret_cast<unsigned *>(s->h_red_dev + 16), ++s->red_seq);
    CUP3D_HIP(hipGetLastError());
    CUP3D_HIP(hipEventRecord(s->ev_a, cs));
    return CUP3D_OK;
  }
  int wait() {
    const volatile unsigned *flag = reinterpret_cast<const volatile unsigned *>(s->h_red + 16);
    const unsigned want = s->red_seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 1; *flag != want; ++spin) {
      __builtin_ia32_pause();
      if ((spin & 0x3fff) == 0) {  // every ~16k polls: has the stream finished (or failed) without raising the flag?
        const hipError_t e = hipEventQuery(s->ev_a);
        if (e == hipSuccess) break;  // completed: the totals are in place (an event wait makes them visible as well)
        if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery", __FILE__, __LINE__);
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    stats_host_wait(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return CUP3D_OK;
  }
};

}  // namespace cup3d
