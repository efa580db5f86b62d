// A stand-in for <hip/hip_runtime.h> with just the calls csrc/dslam_memory.h makes, for tests/test_memory_owners.py: every
// allocation is a host malloc entered in a table.  It counts what is live, aborts the program on a double free or a free
// of a pointer it did not hand out, and fails the n-th allocating call from now on request (hipstub::fail_at).
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

typedef int hipError_t;
typedef struct hipstubEvent *hipEvent_t;
typedef struct hipstubStream *hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipEventDefault = 0, hipEventDisableTiming = 2 };

namespace hipstub {
inline std::set<void *> &live_set() { static std::set<void *> s; return s; }
inline long &countdown() { static long n = 0; return n; }     // the n-th allocating call from now fails (0: none)
inline long &calls() { static long n = 0; return n; }         // allocating and freeing calls so far
inline long live() { return (long)live_set().size(); }
inline void fail_at(long n) { countdown() = n; }
inline hipError_t take(void **out, size_t bytes) {
  calls()++;
  if (countdown() > 0 && --countdown() == 0) { *out = nullptr; return hipErrorOutOfMemory; }
  *out = malloc(bytes ? bytes : 1);
  live_set().insert(*out);
  return hipSuccess;
}
inline hipError_t give(void *p, const char *who) {
  calls()++;
  if (!live_set().erase(p)) { fprintf(stderr, "%s: %p is not a live allocation (double free or foreign pointer)\n", who, p); abort(); }
  free(p);
  return hipSuccess;
}
}  // namespace hipstub

inline hipError_t hipMalloc(void **p, size_t bytes) { return hipstub::take(p, bytes); }
inline hipError_t hipFree(void *p) { return hipstub::give(p, "hipFree"); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return hipstub::take(p, bytes); }
inline hipError_t hipHostFree(void *p) { return hipstub::give(p, "hipHostFree"); }
inline hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned) { *dev = host; return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned) { return hipstub::take(reinterpret_cast<void **>(ev), 1); }
inline hipError_t hipEventDestroy(hipEvent_t ev) { return hipstub::give(ev, "hipEventDestroy"); }
inline hipError_t hipMemsetAsync(void *p, int byte, size_t bytes, hipStream_t) { memset(p, byte, bytes); return hipSuccess; }
