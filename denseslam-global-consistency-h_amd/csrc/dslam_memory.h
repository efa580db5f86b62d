// dslam_memory.h -- the owners of every device, page-locked and event allocation behind the handles of dslam_internal.h.
// Move-only (std::swap exchanges two of them without a HIP call); each converts to the raw pointer / hipEvent_t the launchers
// use.  An allocating call returns the library's error code through hip_fail with the CALLER's file:line and replaces what
// the owner held only when it succeeded, so a failed (re)allocation leaves the owner as it was.  Destructors ignore errors.
// Buffers that have to exist as a whole are a struct of owners: build one aside, move-assign it when every member exists.
#pragma once
#include <hip/hip_runtime.h>

namespace dslam {

int hip_fail(hipError_t err, const char *what, const char *file, int line);

#define DSLAM_TRY(expr) do { if (const int _rc = (expr)) return _rc; } while (0)

template <typename T> struct ElemBytes { static constexpr size_t value = sizeof(T); };
template <> struct ElemBytes<void> { static constexpr size_t value = 1; };

// what the three owners share: one pointer-like handle, null = empty, given up by Release::free
template <typename H, typename Release>
class Owner {
 public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  ~Owner() { reset(); }
  operator H() const { return h_; }
  H get() const { return h_; }
  H operator->() const { return h_; }
  void reset() { if (h_) Release::free(h_); h_ = nullptr; }

 protected:
  void adopt(H h) { reset(); h_ = h; }
 private:
  H h_ = nullptr;
};
struct ReleaseDevice { static void free(void *p) { (void)hipFree(p); } };
struct ReleaseHost { static void free(void *p) { (void)hipHostFree(p); } };
struct ReleaseEvent { static void free(hipEvent_t ev) { (void)hipEventDestroy(ev); } };

// n elements of T in device memory (T = void: n bytes)
template <typename T>
struct DeviceBuffer : Owner<T *, ReleaseDevice> {
  int alloc(size_t n, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    void *p = nullptr;
    const hipError_t err = hipMalloc(&p, n * ElemBytes<T>::value);
    if (err != hipSuccess) return hip_fail(err, "hipMalloc", file, line);
    this->adopt(static_cast<T *>(p));
    return 0;
  }
  // ... and zeroed by a memset queued on `stream`
  int alloc_zeroed(size_t n, hipStream_t stream, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    DSLAM_TRY(alloc(n, file, line));
    const hipError_t err = hipMemsetAsync(this->get(), 0, n * ElemBytes<T>::value, stream);
    return err == hipSuccess ? 0 : hip_fail(err, "hipMemsetAsync", file, line);
  }
};

// n elements of T in page-locked host memory (T = void: n bytes); device(): the address kernels use for a buffer that was
// allocated with hipHostMallocMapped
template <typename T>
struct PinnedBuffer : Owner<T *, ReleaseHost> {
  int alloc(size_t n, unsigned flags = hipHostMallocDefault, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    void *p = nullptr, *d = nullptr;
    hipError_t err = hipHostMalloc(&p, n * ElemBytes<T>::value, flags);
    if (err != hipSuccess) return hip_fail(err, "hipHostMalloc", file, line);
    if ((flags & hipHostMallocMapped) && (err = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) {
      (void)hipHostFree(p);
      return hip_fail(err, "hipHostGetDevicePointer", file, line);
    }
    this->adopt(static_cast<T *>(p));
    dev_ = static_cast<T *>(d);
    return 0;
  }
  T *device() const { return this->get() ? dev_ : nullptr; }
 private:
  T *dev_ = nullptr;
};

struct Event : Owner<hipEvent_t, ReleaseEvent> {
  int create(unsigned flags = hipEventDisableTiming, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    hipEvent_t ev = nullptr;
    const hipError_t err = hipEventCreateWithFlags(&ev, flags);
    if (err != hipSuccess) return hip_fail(err, "hipEventCreateWithFlags", file, line);
    adopt(ev);
    return 0;
  }
};

}  // namespace dslam
