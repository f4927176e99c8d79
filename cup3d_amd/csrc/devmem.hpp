// Who owns device and pinned host memory.  This is the only file of csrc/ that calls the four runtime functions that allocate and
// release it; everything else holds one of the three move-only owners below as a member of a heap object with an explicit destroy call
// (Sim, Multigrid, LabTables, ...) or as a local.
//
// No owner may have static or thread storage duration: its destructor would run after the HIP runtime has been torn down.
// The few process-lifetime allocations (g_invD, g_comm.d_flag, the profiler's events) stay raw pointers, released where they always were.
//
// The ledger rule: an allocation is counted in Sim::bytes (cup3d_sim_device_bytes) if and only if the Sim is passed as `charge`, by its
// size in bytes, at the moment it succeeds.  DevGrow always charges and takes its bytes off again when it lets go.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/cup3d_hip.h"

namespace cup3d {

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);
#define CUP3D_HIP(call)                                                        \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) return ::cup3d::hip_fail(e_, #call, __FILE__, __LINE__); \
  } while (0)

struct Sim;
size_t &ledger(Sim *s);  // Sim::bytes (sim.hpp)

// What an allocation or upload of ZERO elements leaves behind; a request that is not empty is never rounded up.  Callers differ and
// kernels depend on it (GridDev::list == nullptr means "all blocks"; an index table is dereferenced at [0] unconditionally), so every
// call site of upload() says which.
enum class IfEmpty : size_t {
  null = 0,         // nothing: the pointer stays nullptr
  one = 1,          // one element nobody reads
  eight_bytes = 8,  // Dev<void> only: eight bytes, what the obstacle staging has always allocated
};

// ---- device memory: n elements of T (Dev<void>: n bytes, read through as<U>())
template <class T>
class Dev {
 public:
  using Elem = std::conditional_t<std::is_void_v<T>, unsigned char, T>;
  Dev() = default;
  Dev(const Dev &) = delete;
  Dev &operator=(const Dev &) = delete;
  Dev(Dev &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Dev &operator=(Dev &&o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
  ~Dev() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  template <class U>
  U *as() const { return static_cast<U *>(p_); }
  size_t size() const { return n_; }  // elements
  size_t bytes() const { return n_ * sizeof(Elem); }

  // elements held after a request for n under `rule`
  static constexpr size_t held(size_t n, IfEmpty rule) { return n ? n : (size_t)rule; }
  int alloc(size_t n, IfEmpty rule, Sim *charge = nullptr) {
    reset();
    if (rule == IfEmpty::eight_bytes && !std::is_void_v<T>) { set_error("IfEmpty::eight_bytes on a typed Dev: the rule counts bytes"); return CUP3D_EINVAL; }
    n = held(n, rule);
    if (!n) return CUP3D_OK;
    CUP3D_HIP(hipMalloc((void **)&p_, n * sizeof(Elem)));
    n_ = n;
    if (charge) ledger(charge) += bytes();
    return CUP3D_OK;
  }
  int alloc(size_t n, Sim *charge = nullptr) { return alloc(n, IfEmpty::null, charge); }
  int alloc_zeroed(size_t n, hipStream_t st, Sim *charge = nullptr) {
    reset();
    CUP3D_HIP(hipMalloc((void **)&p_, n * sizeof(Elem)));
    n_ = n;
    CUP3D_HIP(hipMemsetAsync(p_, 0, bytes(), st));
    if (charge) ledger(charge) += bytes();
    return CUP3D_OK;
  }
  // n elements of src -> a fresh allocation, copied asynchronously on `st` (src must outlive the copy) ...
  int upload(const T *src, size_t n, hipStream_t st, IfEmpty rule, Sim *charge = nullptr) {
    int rc = alloc(n, rule, charge);
    if (rc) return rc;
    if (n) CUP3D_HIP(hipMemcpyAsync(p_, src, n * sizeof(Elem), hipMemcpyHostToDevice, st));
    return CUP3D_OK;
  }
  int upload(const std::vector<Elem> &v, hipStream_t st, IfEmpty rule) { return upload(v.data(), v.size(), st, rule); }
  // ... or with a blocking copy
  int upload(const std::vector<Elem> &v, IfEmpty rule) {
    int rc = alloc(v.size(), rule);
    if (rc) return rc;
    if (!v.empty()) CUP3D_HIP(hipMemcpy(p_, v.data(), v.size() * sizeof(Elem), hipMemcpyHostToDevice));
    return CUP3D_OK;
  }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};

// ---- a device buffer of bytes that only grows, charged to the ledger of the Sim it serves for as long as it holds memory.  The Sim
// must outlive it (it is a member of something the Sim's destroy hooks delete).
class DevGrow {
 public:
  DevGrow() = default;
  DevGrow(const DevGrow &) = delete;
  DevGrow &operator=(const DevGrow &) = delete;
  DevGrow(DevGrow &&o) noexcept : b_(std::move(o.b_)), s_(std::exchange(o.s_, nullptr)) {}
  DevGrow &operator=(DevGrow &&o) noexcept { std::swap(b_, o.b_); std::swap(s_, o.s_); return *this; }
  ~DevGrow() { release(); }
  void release() {
    if (b_) ledger(s_) -= b_.bytes();
    b_.reset();
  }
  int need(size_t bytes, Sim *s) {
    if (bytes <= b_.bytes()) return CUP3D_OK;
    release();
    s_ = s;
    return b_.alloc(bytes, s);
  }
  // an empty source still asks for `if_empty` bytes (the pointer is never null afterwards); a vector, for one element
  int upload(const void *src, size_t bytes, size_t if_empty, hipStream_t st, Sim *s) {
    int rc = need(bytes ? bytes : if_empty, s);
    if (rc) return rc;
    if (bytes) CUP3D_HIP(hipMemcpyAsync(b_.get(), src, bytes, hipMemcpyHostToDevice, st));
    return CUP3D_OK;
  }
  template <class E>
  int upload(const std::vector<E> &v, hipStream_t st, Sim *s) { return upload(v.data(), v.size() * sizeof(E), sizeof(E), st, s); }
  void *get() const { return b_.get(); }
  template <class U>
  U *as() const { return b_.template as<U>(); }
  size_t bytes() const { return b_.bytes(); }

 private:
  Dev<void> b_;
  Sim *s_ = nullptr;
};

// ---- pinned host memory: n elements of T (Pinned<void>: n bytes), allocated with the given hipHostMalloc flags
template <class T>
class Pinned {
 public:
  using Elem = std::conditional_t<std::is_void_v<T>, unsigned char, T>;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  Pinned(Pinned &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  Pinned &operator=(Pinned &&o) noexcept { std::swap(p_, o.p_); return *this; }
  ~Pinned() { reset(); }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  template <class U>
  U *as() const { return static_cast<U *>(p_); }
  int alloc(size_t n, unsigned flags) {
    reset();
    CUP3D_HIP(hipHostMalloc((void **)&p_, n * sizeof(Elem), flags));
    return CUP3D_OK;
  }
  // the same memory as the device sees it (hipHostMallocMapped)
  int device_alias(T **out) const {
    CUP3D_HIP(hipHostGetDevicePointer((void **)out, p_, 0));
    return CUP3D_OK;
  }

 private:
  T *p_ = nullptr;
};

template <class O, class P>
constexpr bool is_owner_of = !std::is_copy_constructible_v<O> && !std::is_copy_assignable_v<O> && std::is_nothrow_move_constructible_v<O> &&
                             std::is_nothrow_move_assignable_v<O> && std::is_convertible_v<O, P> && std::is_same_v<decltype(std::declval<O>().get()), P>;
static_assert(is_owner_of<Dev<double>, double *> && is_owner_of<Dev<void>, void *>, "Dev<T>: move-only, nothrow-movable, converts to T*");
static_assert(is_owner_of<Pinned<double>, double *> && is_owner_of<Pinned<void>, void *>, "Pinned<T>: move-only, nothrow-movable, converts to T*");
static_assert(Dev<void>::held(4, IfEmpty::eight_bytes) == 4 && Dev<void>::held(0, IfEmpty::eight_bytes) == 8 && Dev<int>::held(0, IfEmpty::one) == 1 &&
                  Dev<int>::held(3, IfEmpty::one) == 3 && Dev<int>::held(0, IfEmpty::null) == 0, "IfEmpty applies to an empty request only");
static_assert(!std::is_copy_constructible_v<DevGrow> && !std::is_copy_assignable_v<DevGrow> && std::is_nothrow_move_constructible_v<DevGrow> &&
                  std::is_nothrow_move_assignable_v<DevGrow>, "DevGrow: move-only, nothrow-movable");

}  // namespace cup3d
