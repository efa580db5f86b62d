// The failure paths of csrc/dslam_memory.h, run on the CPU against the counting HIP stand-in next to this file
// (tests/test_memory_owners.py compiles and runs it).  `owners_check` checks the owners; `owners_check parent-guard` runs
// the same group check over a transcription of the guard batch_scratch used before the owners existed and must FAIL.
#include <cstring>
#include <utility>

#include "dslam_memory.h"

using namespace dslam;

static int g_fail_line = 0;
int dslam::hip_fail(hipError_t, const char *, const char *, int line) {
  g_fail_line = line;
  return -3;
}

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "CHECK failed, line %d: %s\n", __LINE__, #cond);       \
      return false;                                                          \
    }                                                                        \
  } while (0)

// ---- a lazily allocated group: five buffers and an event, the shape of batch_scratch ------------------------------------
constexpr int kGroupSize = 6;
struct Group {
  DeviceBuffer<int> a;
  DeviceBuffer<float> b;
  DeviceBuffer<unsigned char> c;
  DeviceBuffer<void> d;
  PinnedBuffer<double> e;
  Event ev;
};
struct Handle : Group {
  int other = 7;
};
static int held(const Handle &h) { return !!h.a + !!h.b + !!h.c + !!h.d + !!h.e + !!h.ev; }
static int group_allocate(Handle *h) {
  if (h->a) return 0;
  Group n;
  DSLAM_TRY(n.a.alloc(100));
  DSLAM_TRY(n.b.alloc(100));
  DSLAM_TRY(n.c.alloc_zeroed(64, nullptr));
  DSLAM_TRY(n.d.alloc(256));
  DSLAM_TRY(n.e.alloc(8, hipHostMallocMapped));
  DSLAM_TRY(n.ev.create());
  static_cast<Group &>(*h) = std::move(n);
  return 0;
}

// the parent's batch_scratch: raw pointers, the first of the group as the guard for all of it
struct RawHandle {
  int *a = nullptr;
  float *b = nullptr;
  unsigned char *c = nullptr;
  void *d = nullptr;
  double *e = nullptr;
  hipEvent_t ev = nullptr;
  ~RawHandle() {
    void *all[] = {a, b, c, d, e, ev};
    for (void *p : all)
      if (p) (void)hipFree(p);
  }
};
static int held(const RawHandle &h) { return !!h.a + !!h.b + !!h.c + !!h.d + !!h.e + !!h.ev; }
#define RAW_HIP(call) do { if ((call) != hipSuccess) return hip_fail(0, #call, __FILE__, __LINE__); } while (0)
static int group_allocate(RawHandle *h) {
  if (!h->a) {
    RAW_HIP(hipMalloc((void **)&h->a, 400));
    RAW_HIP(hipMalloc((void **)&h->b, 400));
    RAW_HIP(hipMalloc((void **)&h->c, 64));
    RAW_HIP(hipMalloc(&h->d, 256));
    RAW_HIP(hipHostMalloc((void **)&h->e, 64, hipHostMallocDefault));
    RAW_HIP(hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
  }
  return 0;
}

template <typename H>
static bool check_group() {
  for (int n = 1; n <= kGroupSize; n++) {
    {
      H h;
      const long before = hipstub::live();
      g_fail_line = 0;
      hipstub::fail_at(n);
      CHECK(group_allocate(&h) != 0);
      CHECK(g_fail_line != 0);                  // reported through the error hook, with the caller's line
      CHECK(held(h) == 0);                      // the handle holds nothing it did not hold before ...
      CHECK(hipstub::live() == before);         // ... and nothing is left over
      hipstub::fail_at(0);
      CHECK(group_allocate(&h) == 0);           // a retry allocates again
      CHECK(held(h) == kGroupSize);
      CHECK(hipstub::live() == before + kGroupSize);
      const long calls = hipstub::calls();
      CHECK(group_allocate(&h) == 0 && hipstub::calls() == calls);   // (and a third call finds the group)
    }
    CHECK(hipstub::live() == 0);
  }
  return true;
}

// ---- regrows --------------------------------------------------------------------------------------------------------
struct Staging {   // ensure_staging: keeps the old pair and its size on failure
  DeviceBuffer<char> dev;
  PinnedBuffer<char> host;
  size_t bytes = 0;
};
static int ensure_staging(Staging *s, size_t bytes) {
  if (bytes <= s->bytes) return 0;
  DeviceBuffer<char> dev;
  PinnedBuffer<char> host;
  DSLAM_TRY(dev.alloc(bytes));
  DSLAM_TRY(host.alloc(bytes));
  s->dev = std::move(dev);
  s->host = std::move(host);
  s->bytes = bytes;
  return 0;
}
struct Images {    // batch_depth / the mesh buffers: the old buffer goes first; empty and size 0 on failure
  DeviceBuffer<float> px;
  size_t n = 0;
};
static int ensure_images(Images *s, size_t n) {
  if (n <= s->n) return 0;
  s->px.reset();
  s->n = 0;
  DSLAM_TRY(s->px.alloc(n));
  s->n = n;
  return 0;
}
static bool check_regrow() {
  for (int n = 1; n <= 2; n++) {
    {
      Staging s;
      CHECK(ensure_staging(&s, 64) == 0 && s.bytes == 64 && hipstub::live() == 2);
      char *const dev = s.dev, *const host = s.host;
      memset(dev, 1, 64);
      hipstub::fail_at(n);
      CHECK(ensure_staging(&s, 128) != 0);
      CHECK(s.dev == dev && s.host == host && s.bytes == 64);   // pointer and size agree: both old
      CHECK(hipstub::live() == 2);
      memset(s.dev, 2, s.bytes);                                // (still a live allocation of that size)
      hipstub::fail_at(0);
      CHECK(ensure_staging(&s, 128) == 0 && s.bytes == 128 && s.dev && s.host && hipstub::live() == 2);
    }
    CHECK(hipstub::live() == 0);
  }
  {
    Images im;
    CHECK(ensure_images(&im, 16) == 0 && im.px && im.n == 16);
    hipstub::fail_at(1);
    CHECK(ensure_images(&im, 32) != 0);
    CHECK(!im.px && im.n == 0 && hipstub::live() == 0);         // pointer and size agree: both empty
    hipstub::fail_at(0);
    CHECK(ensure_images(&im, 32) == 0 && im.px && im.n == 32 && hipstub::live() == 1);
  }
  CHECK(hipstub::live() == 0);
  return true;
}

// ---- move, swap, borrowed memory --------------------------------------------------------------------------------------
static bool check_move_swap() {
  {
    DeviceBuffer<int> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(8) == 0);
    int *const pa = a, *const pb = b;
    const long calls = hipstub::calls();
    std::swap(a, b);
    CHECK(a == pb && b == pa && hipstub::calls() == calls);     // exchanged: no allocation, no free
    DeviceBuffer<int> c(std::move(a));
    CHECK(!a && c == pb && hipstub::calls() == calls && hipstub::live() == 2);
    b = std::move(c);                                           // (what b held is freed, exactly once)
    CHECK(!c && b == pb && hipstub::live() == 1);
    b.reset();
    b.reset();
    CHECK(!b && hipstub::live() == 0);
  }
  {
    PinnedBuffer<double> m, plain;
    CHECK(m.alloc(4, hipHostMallocMapped) == 0 && plain.alloc(4) == 0);
    double *const pm = m;
    CHECK(m.device() == pm && plain.device() == nullptr);
    std::swap(m, plain);
    CHECK(plain == pm && plain.device() == pm && m.device() == nullptr);
    PinnedBuffer<double> moved(std::move(plain));
    CHECK(moved.device() == pm && plain.device() == nullptr);
    Event e1, e2;
    CHECK(e1.create() == 0);
    const hipEvent_t raw = e1;
    std::swap(e1, e2);
    CHECK(!e1 && e2 == raw);
  }
  CHECK(hipstub::live() == 0);
  return true;
}
struct Scene {   // dslam_scene::voxels: the caller's buffer is looked at, never owned
  int *voxels = nullptr;
  DeviceBuffer<int> voxels_own;
};
static int scene_allocate(Scene *s, int *ext) {
  if (!ext) DSLAM_TRY(s->voxels_own.alloc(32));
  s->voxels = ext ? ext : s->voxels_own.get();
  return 0;
}
static bool check_borrowed() {
  static int callers[32];
  {
    Scene ext, own;
    CHECK(scene_allocate(&ext, callers) == 0 && ext.voxels == callers && !ext.voxels_own && hipstub::live() == 0);
    CHECK(scene_allocate(&own, nullptr) == 0 && own.voxels == own.voxels_own && hipstub::live() == 1);
  }   // (the stand-in aborts if `callers` reaches hipFree)
  CHECK(hipstub::live() == 0);
  return true;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "parent-guard")) return check_group<RawHandle>() ? 0 : 1;
  const bool ok = check_group<Handle>() && check_regrow() && check_move_swap() && check_borrowed();
  if (ok) printf("owners ok\n");
  return ok ? 0 : 1;
}
