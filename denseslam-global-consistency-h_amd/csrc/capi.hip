// capi.hip -- the C ABI of include/dslam_fusion.h: object lifetime, host<->device plumbing, and the
// composition of kernels into the ITMLib engine calls (ITMDenseMapper::ProcessFrame, ITMMainEngine::GetImage ...).
// No arithmetic of the hot path lives here; there is no CPU fallback: without a HIP device the engine cannot be
// created and every entry point fails.
#include <climits>
#include <cctype>
#include <cmath>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "dslam_internal.h"
#include "pack_host.h"

#pragma clang fp contract(off)

namespace dslam {

static thread_local std::string g_last_error;
void set_last_error(const std::string &msg) { g_last_error = msg; }
static std::atomic<unsigned long long> g_hip_failures{0};
unsigned long long hip_failure_count() { return g_hip_failures.load(std::memory_order_relaxed); }
int hip_fail(hipError_t err, const char *what, const char *file, int line) {
  g_hip_failures.fetch_add(1, std::memory_order_relaxed);
  char buf[512];
  snprintf(buf, sizeof(buf), "%s failed: %s (%s:%d)", what, hipGetErrorString(err), file, line);
  g_last_error = buf;
  return DSLAM_ERR_HIP;
}

// ORUtils::Matrix4::inv restated (cofactor expansion); identical expression order to the CPU oracle so both
// derive bit-identical inverse poses.  Host code: compiled with -ffp-contract=off.
bool invert_matrix(const float *m, float *dst) {
  float tmp[12], src[16], det;
  for (int i = 0; i < 4; i++) {
    src[i] = m[i * 4];
    src[i + 4] = m[i * 4 + 1];
    src[i + 8] = m[i * 4 + 2];
    src[i + 12] = m[i * 4 + 3];
  }
  tmp[0] = src[10] * src[15]; tmp[1] = src[11] * src[14]; tmp[2] = src[9] * src[15]; tmp[3] = src[11] * src[13];
  tmp[4] = src[9] * src[14]; tmp[5] = src[10] * src[13]; tmp[6] = src[8] * src[15]; tmp[7] = src[11] * src[12];
  tmp[8] = src[8] * src[14]; tmp[9] = src[10] * src[12]; tmp[10] = src[8] * src[13]; tmp[11] = src[9] * src[12];
  dst[0] = (tmp[0] * src[5] + tmp[3] * src[6] + tmp[4] * src[7]) - (tmp[1] * src[5] + tmp[2] * src[6] + tmp[5] * src[7]);
  dst[1] = (tmp[1] * src[4] + tmp[6] * src[6] + tmp[9] * src[7]) - (tmp[0] * src[4] + tmp[7] * src[6] + tmp[8] * src[7]);
  dst[2] = (tmp[2] * src[4] + tmp[7] * src[5] + tmp[10] * src[7]) - (tmp[3] * src[4] + tmp[6] * src[5] + tmp[11] * src[7]);
  dst[3] = (tmp[5] * src[4] + tmp[8] * src[5] + tmp[11] * src[6]) - (tmp[4] * src[4] + tmp[9] * src[5] + tmp[10] * src[6]);
  dst[4] = (tmp[1] * src[1] + tmp[2] * src[2] + tmp[5] * src[3]) - (tmp[0] * src[1] + tmp[3] * src[2] + tmp[4] * src[3]);
  dst[5] = (tmp[0] * src[0] + tmp[7] * src[2] + tmp[8] * src[3]) - (tmp[1] * src[0] + tmp[6] * src[2] + tmp[9] * src[3]);
  dst[6] = (tmp[3] * src[0] + tmp[6] * src[1] + tmp[11] * src[3]) - (tmp[2] * src[0] + tmp[7] * src[1] + tmp[10] * src[3]);
  dst[7] = (tmp[4] * src[0] + tmp[9] * src[1] + tmp[10] * src[2]) - (tmp[5] * src[0] + tmp[8] * src[1] + tmp[11] * src[2]);
  tmp[0] = src[2] * src[7]; tmp[1] = src[3] * src[6]; tmp[2] = src[1] * src[7]; tmp[3] = src[3] * src[5];
  tmp[4] = src[1] * src[6]; tmp[5] = src[2] * src[5]; tmp[6] = src[0] * src[7]; tmp[7] = src[3] * src[4];
  tmp[8] = src[0] * src[6]; tmp[9] = src[2] * src[4]; tmp[10] = src[0] * src[5]; tmp[11] = src[1] * src[4];
  dst[8] = (tmp[0] * src[13] + tmp[3] * src[14] + tmp[4] * src[15]) - (tmp[1] * src[13] + tmp[2] * src[14] + tmp[5] * src[15]);
  dst[9] = (tmp[1] * src[12] + tmp[6] * src[14] + tmp[9] * src[15]) - (tmp[0] * src[12] + tmp[7] * src[14] + tmp[8] * src[15]);
  dst[10] = (tmp[2] * src[12] + tmp[7] * src[13] + tmp[10] * src[15]) - (tmp[3] * src[12] + tmp[6] * src[13] + tmp[11] * src[15]);
  dst[11] = (tmp[5] * src[12] + tmp[8] * src[13] + tmp[11] * src[14]) - (tmp[4] * src[12] + tmp[9] * src[13] + tmp[10] * src[14]);
  dst[12] = (tmp[2] * src[10] + tmp[5] * src[11] + tmp[1] * src[9]) - (tmp[4] * src[11] + tmp[0] * src[9] + tmp[3] * src[10]);
  dst[13] = (tmp[8] * src[11] + tmp[0] * src[8] + tmp[7] * src[10]) - (tmp[6] * src[10] + tmp[9] * src[11] + tmp[1] * src[8]);
  dst[14] = (tmp[6] * src[9] + tmp[11] * src[11] + tmp[3] * src[8]) - (tmp[10] * src[11] + tmp[2] * src[8] + tmp[7] * src[9]);
  dst[15] = (tmp[10] * src[10] + tmp[4] * src[8] + tmp[9] * src[9]) - (tmp[8] * src[9] + tmp[11] * src[10] + tmp[5] * src[8]);
  det = src[0] * dst[0] + src[1] * dst[1] + src[2] * dst[2] + src[3] * dst[3];
  if (det == 0.0f) {
    for (int i = 0; i < 16; i++) dst[i] = 0.0f;
    return false;
  }
  for (int i = 0; i < 16; i++) dst[i] = dst[i] * (1.0f / det);
  return true;
}

// Map versions are drawn from one process-wide counter, so a version never repeats -- not even on a new scene that
// happens to be allocated where a destroyed one was (the GetImage memo compares scene pointer and version).
unsigned long long next_map_version() {
  static std::atomic<unsigned long long> counter{0};
  return ++counter;
}

// Every entry point that waits for the stream ends here: what a kernel reported through report_error (a tile count that
// never arrived, an allocation ray longer than the order key encodes) is returned by the first call that could know --
// the call itself on a synchronous engine, the next synchronising call (fence wait, read-back, dslam_engine_synchronize)
// on an asynchronous one.  Told once per occurrence; the scene's own flags stay set for dslam_get_stats.
int sync_check(dslam_engine *e) {
  // (taking the stream withdraws the permission to overlap k_mark, EngineStream, and that is meant: once the stream has drained
  // there is nothing left to run beside, and the auxiliary stream would only cost its launch and its wait)
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return device_errors(e);
}
// Two words: [0] report_error's, [1] k_mark's own (dslam_device.h report_error_own: k_mark may run beside another kernel of
// the engine, and two kernels must not update one word with a load and a store each).
// [2] is the word of the allocation sweep that runs on the auxiliary stream, for the same reason.  A call whose
// body the engine held back (dslam_engine::deferred) and that failed when it ran is told here too, once, in front of what
// kernels reported: it happened first.
int device_errors(dslam_engine *e) {
  if (e->deferred_rc) {
    const int rc = e->deferred_rc;
    e->deferred_rc = 0;
    set_last_error(e->deferred_error);
    return rc;
  }
  int *h = e->err_host;
  if (!h || (__atomic_load_n(h, __ATOMIC_RELAXED) | __atomic_load_n(h + 1, __ATOMIC_RELAXED) | __atomic_load_n(h + 2, __ATOMIC_RELAXED) |
             __atomic_load_n(h + 3, __ATOMIC_RELAXED)) == 0)
    return DSLAM_OK;
  // (each taken in one step: a report that lands now is the next call's)
  const int flags = __atomic_exchange_n(h, 0, __ATOMIC_RELAXED) | __atomic_exchange_n(h + 1, 0, __ATOMIC_RELAXED) |
                    __atomic_exchange_n(h + 2, 0, __ATOMIC_RELAXED) | __atomic_exchange_n(h + 3, 0, __ATOMIC_RELAXED);
  if (flags == 0) return DSLAM_OK;
  if (flags & 2) {
    set_last_error("a tile count of an ordered compaction never arrived (device made no progress?): the map state is undefined");
    return DSLAM_ERR_HIP;
  }
  set_last_error("allocation ray needed more steps than the order key encodes (non-rigid pose or mu/voxel_size changed?)");
  return DSLAM_ERR_UNSUPPORTED;
}

// Calls the engine holds back.  The caller's thread runs them, in call order, with the stream's hook
// disarmed; a body that fails does not stop the ones behind it (a caller that ignored the call's return value would have
// made them too), and the first failure waits in deferred_rc for the late-error path (device_errors).
static void run_held_calls(void *engine) { (void)flush_deferred(static_cast<dslam_engine *>(engine)); }
int flush_deferred(dslam_engine *e) {
  if (!e || e->flushing) return DSLAM_OK;
  if (e->deferred.empty()) {
    // (a ProcessFrame that failed behind its launches holds no tail, but may have left a front end on aux_stream: DESIGN.md 4i)
    if (e->front_pending) (void)settle_front(e);
    return DSLAM_OK;
  }
  e->flushing = true;
  e->stream.disarm();
  std::vector<std::function<int()>> bodies;
  bodies.swap(e->deferred);
  for (auto &body : bodies) {
    int rc = body();
    // A ProcessFrame's tail has left GetImage's front end on aux_stream.  The pipelined upload wants its copy
    // enqueued here: behind the fusion launch, in front of the GetImage that sits the auxiliary stream out.
    if (e->front_pending && e->after_tail) {
      const std::function<void()> hook = std::move(e->after_tail);
      e->after_tail = nullptr;
      hook();
    }
    if (rc != DSLAM_OK && e->deferred_rc == DSLAM_OK) {
      e->deferred_rc = rc;
      e->deferred_error = g_last_error;
    }
  }
  // ... and if no GetImage among the held calls waited for that front end, the thread does now: whatever comes next --
  // Decay, SlideWindow, a reset, DeProcessFrame, a wait, the batch, the caller with the engine's stream in its hands --
  // finds the record complete, never half-written, and the auxiliary stream empty.
  if (e->front_pending) {
    const int rc = settle_front(e);
    if (rc != DSLAM_OK && e->deferred_rc == DSLAM_OK) {
      e->deferred_rc = rc;
      e->deferred_error = g_last_error;
    }
  }
  e->flushing = false;
  return DSLAM_OK;
}
void defer_call(dslam_engine *e, std::function<int()> body) {
  e->deferred.push_back(std::move(body));
  e->stream.arm(run_held_calls, e);
}

int finish_call(dslam_engine *e) {
  if (!e->async_mode) return sync_check(e);
  return DSLAM_OK;
}

int tickets_resync(dslam_engine *e) {
  const unsigned long long seen = hip_failure_count();
  unsigned host[3] = {0, 0, 0};
  if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(host, e->ticket, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    set_last_error("ticket counters could not be read back after a HIP failure");
    return DSLAM_ERR_HIP;   // (hip_failures_seen stays behind: the next pass tries again)
  }
  e->ticket_base = host[0];
  e->ticket_base2 = host[1];
  e->ticket_base3 = host[2];
  e->hip_failures_seen = seen;
  return DSLAM_OK;
}

int ensure_scratch(dslam_engine *e, int entries, int local_blocks) {
  if (entries <= e->scratch_entries && local_blocks <= e->scratch_local_blocks) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  const int N = entries > e->scratch_entries ? entries : e->scratch_entries;
  const int L = local_blocks > e->scratch_local_blocks ? local_blocks : e->scratch_local_blocks;
  EngineScratch n;   // built aside: a failure leaves the engine with the complete old set
  n.scratch_entries = N; n.scratch_local_blocks = L;
  // order keys and allocType: cleared here once, kept clean by the allocation passes (scenes of different sizes share
  // them, so both start at fixed addresses: a pass only ever touches [0, its entry count) of each)
  DSLAM_TRY(n.order_keys.alloc_zeroed(N, e->stream));
  DSLAM_TRY(n.alloc_type.alloc_zeroed(N, e->stream));
  DSLAM_TRY(n.block_coords.alloc(N));
  // the bitmaps of the allocation pass (whole tiles; the alternating sets start clean and are kept clean by the passes)
  n.bits_words = bit_tiles(N) * kBitTileWords;
  for (int k = 0; k < 2; k++) {
    DSLAM_TRY(n.bits_q1[k].alloc_zeroed(n.bits_words, e->stream));
    DSLAM_TRY(n.bits_q2[k].alloc_zeroed(n.bits_words, e->stream));
    DSLAM_TRY(n.bits_mark[k].alloc_zeroed(n.bits_words, e->stream));
  }
  DSLAM_TRY(n.bits_retest.alloc_zeroed(n.bits_words, e->stream));
  int tiles = num_tiles(N > L ? N : L);
  if (tiles < bit_tiles(N) * (kBitTileWords / 32)) tiles = bit_tiles(N) * (kBitTileWords / 32);  // (room for tiles as small as 1024 entries)
  DSLAM_TRY(n.agg.alloc_zeroed((size_t)tiles * 3, e->stream));
  n.agg_tiles = tiles;
  n.pend_cap = N < L ? N : L;
  DSLAM_TRY(n.pend_entry.alloc(n.pend_cap)); DSLAM_TRY(n.pend_entry_idx.alloc(n.pend_cap)); DSLAM_TRY(n.pend_offset.alloc(n.pend_cap));
  DSLAM_TRY(n.pend_count.alloc_zeroed(4, e->stream));
  DSLAM_TRY(n.hidden_pos.alloc(N));
  DSLAM_TRY(n.tile_counts.alloc((size_t)tiles * 2)); DSLAM_TRY(n.tile_offsets.alloc((size_t)tiles * 2));
  const size_t list_len = (size_t)(N > L ? N : L);
  DSLAM_TRY(n.list_a.alloc(list_len)); DSLAM_TRY(n.list_b.alloc(list_len));
  DSLAM_TRY(n.list_c.alloc(list_len)); DSLAM_TRY(n.list_d.alloc(list_len));
  DSLAM_TRY(n.pos_scratch.alloc(L));
  DSLAM_TRY(n.rem_flags.alloc_zeroed(N, e->stream)); DSLAM_TRY(n.freed_flags.alloc_zeroed(N, e->stream));
  DSLAM_TRY(n.rem_cand.alloc_zeroed((size_t)L + 16, e->stream));
  DSLAM_TRY(n.maint_flags.alloc_zeroed(4, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  static_cast<EngineScratch &>(*e) = std::move(n);
  return DSLAM_OK;
}

// regrow: on failure the old pair and its size stay
static int ensure_staging(dslam_engine *e, size_t bytes) {
  if (bytes <= e->staging_bytes) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  DeviceBuffer<char> dev;
  PinnedBuffer<char> host;
  DSLAM_TRY(dev.alloc(bytes)); DSLAM_TRY(host.alloc(bytes));
  e->staging_dev = std::move(dev); e->staging_host = std::move(host); e->staging_bytes = bytes;
  return DSLAM_OK;
}

}  // namespace dslam

using namespace dslam;

extern "C" {

const char *dslam_last_error(void) { return g_last_error.c_str(); }
const char *dslam_version(void) { return "dslam_fusion 0.1 (gfx950)"; }

// ---- an engine outlives the handles made from it ---------------------------------------------------------------
// Every destroy call of a scene, render state, view or frame store selects the engine's device and waits for its
// stream, so the engine object and its streams must be there for it.  A create call adopts its handle the moment the
// handle points at the engine (so the destroy call that clears away a half-built one balances it), every destroy call
// releases it; dslam_engine_destroy frees the engine only if no handle is left, and otherwise leaves that to the last
// release.  Plain counters: the engine and its handles are used from one thread (dslam_fusion.h, conventions).
static std::atomic<int> g_live_engines{0};   // engine objects not yet freed (dslam_debug_live_engines)
static void engine_adopt(dslam_engine *e) { e->children++; }
// Fences the caller still holds forget the engine, destroyed ones go -- except those a view still waits on: they stay
// attached until that view lets go, which the engine waits for anyway.  The invariant this rests on: lent_count > 0 only
// while a VIEW of this engine holds the fence in up_lender (dslam_view_destroy lets go of both before it releases the
// engine), so lent_count > 0 implies children > 0 through that view -- `children` counts every handle kind and is only
// the guard for the final call (engine_free, children == 0, where nothing can be lent any more and every fence goes).
// A fence kept this way still names the closed engine: dslam_fence_wait reads its error word through it, which is sound
// because the object lives exactly as long as the fence stays attached.
static void engine_detach_fences(dslam_engine *e) {
  std::vector<dslam_fence *> kept;
  for (dslam_fence *f : e->fences) {
    if (f->lent_count > 0 && e->children > 0) kept.push_back(f);
    else if (f->zombie) delete f;
    else f->engine = nullptr;   // the caller still holds it: its destroy call must not look for this engine
  }
  e->fences.swap(kept);
  e->last_fence = nullptr;
}
static void engine_free(dslam_engine *e) {
  (void)hipSetDevice(e->device);
  engine_detach_fences(e);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->aux_stream) (void)hipStreamDestroy(e->aux_stream);
  if (e->stream.peek()) (void)hipStreamDestroy(e->stream.peek());
  delete e;
  g_live_engines.fetch_sub(1, std::memory_order_relaxed);
}
static void engine_release(dslam_engine *e) {
  if (--e->children == 0 && e->closed) engine_free(e);
}

static int engine_allocate(dslam_engine *e) {
  DSLAM_HIP(hipStreamCreateWithFlags(e->stream.create_into(), hipStreamNonBlocking));
  DSLAM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  DSLAM_HIP(hipStreamCreateWithFlags(&e->aux_stream, hipStreamNonBlocking));
  DSLAM_TRY(e->start_stamp.alloc(16, hipHostMallocCoherent));
  e->start_stamp[0] = 0; e->start_stamp[1] = 0;   // ([1]: the start of the selection behind a sweep on aux_stream)
  e->pinned_bytes = 64 * 1024;
  DSLAM_TRY(e->pinned.alloc(e->pinned_bytes));
  memset(e->pinned, 0, e->pinned_bytes);
  DSLAM_TRY(e->misc_counter.alloc(16));
  DSLAM_TRY(e->map_table.alloc(DSLAM_MAX_RENDER_MAPS * kMapDescriptorBytes));
  DSLAM_TRY(e->ticket.alloc(16));
  DSLAM_HIP(hipMemset(e->ticket, 0, 16 * sizeof(unsigned)));
  e->ticket_base = 0;
  e->hip_failures_seen = hip_failure_count();
  DSLAM_TRY(e->err_host.alloc(16));
  DSLAM_TRY(e->sweep_done.create());
  e->err_host[0] = 0; e->err_host[1] = 0; e->err_host[2] = 0; e->err_host[3] = 0;
  return DSLAM_OK;
}

int dslam_device_numa_node(int device_index, int *node_out) {
  if (!node_out) return DSLAM_ERR_INVALID;
  *node_out = -1;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_last_error("no HIP device: libdslam_fusion has no CPU path");
    return DSLAM_ERR_NO_DEVICE;
  }
  DSLAM_REQUIRE(device_index >= 0 && device_index < n, "device index out of range");
  char bus[64] = {0};
  DSLAM_HIP(hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, device_index));
  for (char *c = bus; *c; c++) *c = (char)tolower(*c);
  char path[160];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
  if (FILE *f = fopen(path, "r")) {
    int node = -1;
    if (fscanf(f, "%d", &node) == 1) *node_out = node;
    fclose(f);
  }
  return DSLAM_OK;   // (-1: the platform does not say)
}

int dslam_engine_create(int device_index, dslam_engine **out) {
  if (!out) return DSLAM_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_last_error("no HIP device: libdslam_fusion has no CPU path");
    return DSLAM_ERR_NO_DEVICE;
  }
  DSLAM_REQUIRE(device_index >= 0 && device_index < n, "device index out of range");
  DSLAM_HIP(hipSetDevice(device_index));
  dslam_engine *e = new dslam_engine();
  g_live_engines.fetch_add(1, std::memory_order_relaxed);
  e->device = device_index;
  if (const char *v = getenv("DSLAM_SPECULATIVE_FRONT_END")) e->speculate_front = atoi(v) != 0;
  if (const char *v = getenv("DSLAM_OVERLAP_MARK")) e->overlap_mark = atoi(v) != 0;
  if (const char *v = getenv("DSLAM_OVERLAP_SWEEP")) e->overlap_sweep = atoi(v) != 0;
  if (!e->overlap_mark) e->overlap_sweep = false;
  if (const char *v = getenv("DSLAM_OVERLAP_FRONT")) e->overlap_front = atoi(v) != 0;
  if (!e->overlap_sweep) e->overlap_front = false;
  if (const char *v = getenv("DSLAM_FRONT_BEHIND_TAIL")) e->front_behind_tail = atoi(v) != 0;
  if (const char *v = getenv("DSLAM_SWEEP_DONE_EVENT")) e->sweep_done_by_event = atoi(v) != 0;
  const int rc = engine_allocate(e);
  if (rc) {
    (void)dslam_engine_destroy(e);
    return rc;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_index) == hipSuccess) e->sm_count = prop.multiProcessorCount;
  *out = e;
  return DSLAM_OK;
}

int dslam_engine_destroy(dslam_engine *e) {
  if (!e) return DSLAM_OK;
  (void)hipSetDevice(e->device);
  flush_deferred(e);   // (on its own device: held calls launch kernels)
  if (e->closed) return DSLAM_OK;   // (a second destroy of an engine its handles keep alive: nothing left to do)
  if (e->stream.peek()) (void)hipStreamSynchronize(e->stream.peek());
  if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
  if (e->aux_stream) (void)hipStreamSynchronize(e->aux_stream);
  if (e->children > 0) {   // handles are left: their destroy calls need the object and its streams
    engine_detach_fences(e);
    e->closed = true;
    return DSLAM_OK;
  }
  engine_free(e);
  return DSLAM_OK;
}

int dslam_debug_live_engines(int *out) {
  DSLAM_REQUIRE(out, "null argument");
  *out = g_live_engines.load(std::memory_order_relaxed);
  return DSLAM_OK;
}

int dslam_selftest_division(dslam_engine *e, long long samples, long long *mismatches_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && mismatches_out && samples > 0, "bad argument");
  unsigned long long *dev = reinterpret_cast<unsigned long long *>(e->misc_counter + 4);  // 8-byte aligned slot
  int rc = launch_selftest_division(e, samples, dev);
  if (rc) return rc;
  DSLAM_HIP(hipMemcpyAsync(e->pinned, dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  *mismatches_out = (long long)*reinterpret_cast<unsigned long long *>(e->pinned.get());
  return DSLAM_OK;
}

int dslam_debug_set_render_tile_budget(dslam_engine *e, int budget) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && budget > 0, "bad argument");
  e->render_tile_budget = budget;
  return DSLAM_OK;
}

int dslam_debug_set_push_job_min(dslam_engine *e, int min_visible_blocks) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && min_visible_blocks >= 0, "bad argument");
  e->push_job_min = min_visible_blocks;
  return DSLAM_OK;
}

int dslam_debug_stream_launches(dslam_engine *e, long long *count_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && count_out, "bad argument");
  *count_out = e->stream_launches;
  return DSLAM_OK;
}

int dslam_debug_front_end_counts(dslam_engine *e, long long *computed_out, long long *adopted_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && computed_out && adopted_out, "null argument");
  *computed_out = e->front_launches;
  *adopted_out = e->front_adoptions;
  return DSLAM_OK;
}
int dslam_debug_mark_overlap_counts(dslam_engine *e, long long *overlapped_out, long long *in_stream_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && overlapped_out && in_stream_out, "null argument");
  *overlapped_out = e->mark_overlapped;
  *in_stream_out = e->mark_in_stream;
  return DSLAM_OK;
}
int dslam_debug_sweep_overlap_counts(dslam_engine *e, long long *overlapped_out, long long *in_stream_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && overlapped_out && in_stream_out, "null argument");
  *overlapped_out = e->sweep_overlapped;
  *in_stream_out = e->sweep_in_stream;
  return DSLAM_OK;
}
int dslam_debug_front_overlap_counts(dslam_engine *e, long long *on_aux_out, long long *in_launch_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && on_aux_out && in_launch_out, "null argument");
  *on_aux_out = e->front_on_aux;
  *in_launch_out = e->front_in_launch;
  return DSLAM_OK;
}
int dslam_debug_icp_sums(dslam_engine *e, double out[29]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  DSLAM_REQUIRE(e->icp_have_sums, "no tracker evaluation has run on this engine");
  memcpy(out, e->icp_last_sums, sizeof e->icp_last_sums);
  return DSLAM_OK;
}
int dslam_debug_inject_device_error(dslam_engine *e, dslam_scene *s, int bits) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && s->engine == e && (bits == 1 || bits == 2 || bits == 3), "bad argument");
  int rc = launch_inject_error(e, s, bits);
  if (rc) return rc;
  return finish_call(e);
}

int dslam_engine_set_async(dslam_engine *e, int async_mode) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null engine");
  e->async_mode = async_mode != 0;
  return DSLAM_OK;
}
int dslam_engine_synchronize(dslam_engine *e) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null engine");
  return sync_check(e);  // (every pipelined upload is waited for by a kernel of this stream)
}

// ---- fences --------------------------------------------------------------------------------------------------
int dslam_fence_create(dslam_engine *e, dslam_fence **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  *out = nullptr;
  dslam_fence *f = new dslam_fence();
  f->engine = e;
  if (const int rc = f->ev.create()) { delete f; return rc; }
  e->fences.push_back(f);
  *out = f;
  return DSLAM_OK;
}
static void fence_free(dslam_fence *f) {
  if (f->engine) {
    auto &v = f->engine->fences;
    v.erase(std::remove(v.begin(), v.end(), f), v.end());
  }
  delete f;
}
// a view stops waiting on the fence event it had borrowed for landing buffer b
static void release_lender(dslam_view *v, int b) {
  dslam_fence *f = v->up_lender[b];
  v->up_lender[b] = nullptr;
  if (f && --f->lent_count == 0 && f->zombie) fence_free(f);
}
int dslam_fence_destroy(dslam_fence *f) {
  if (f) flush_deferred(f->engine);   // (a record of this fence may still be held back)
  if (!f) return DSLAM_OK;
  if (f->engine && f->engine->last_fence == f) f->engine->last_fence = nullptr;
  if (f->engine && f->lent_count > 0) { f->zombie = true; return DSLAM_OK; }  // (a view still waits on its event)
  fence_free(f);
  return DSLAM_OK;
}
static int fence_record_now(dslam_engine *e, dslam_fence *f) {
  f->record_held = false;
  DSLAM_HIP(hipEventRecord(f->ev, e->stream.peek()));   // (a marker touches no buffer: EngineStream)
  f->recorded = true;
  f->view_reads_at_record = e->view_reads;
  e->last_fence = f;
  return DSLAM_OK;
}
// Behind calls the engine holds back the record is held back too: the fence must sit behind their kernels.
// Waiting for such a fence, or asking it, hands everything to the GPU first.
int dslam_fence_record(dslam_engine *e, dslam_fence *f) {
  DSLAM_REQUIRE(e && f && f->engine == e, "fence belongs to a different engine");
  if (e->deferred.empty()) return fence_record_now(e, f);
  f->record_held = true;
  defer_call(e, [e, f]() { return fence_record_now(e, f); });
  return DSLAM_OK;
}
int dslam_fence_wait(dslam_fence *f) {
  DSLAM_REQUIRE(f, "null fence");
  if (f->record_held) flush_deferred(f->engine);
  if (f->recorded) DSLAM_HIP(hipEventSynchronize(f->ev));
  return f->engine ? device_errors(f->engine) : DSLAM_OK;   // (what kernels in front of the fence reported, see sync_check)
}
int dslam_fence_query(dslam_fence *f, int *done) {
  DSLAM_REQUIRE(f && done, "null argument");
  *done = 1;
  if (f->record_held) flush_deferred(f->engine);
  if (f->recorded) {
    const hipError_t err = hipEventQuery(f->ev);
    if (err == hipErrorNotReady) *done = 0;
    else if (err != hipSuccess) return hip_fail(err, "hipEventQuery", __FILE__, __LINE__);
  }
  return DSLAM_OK;
}
// (a caller that has the stream may order work of its own by it, which a k_mark on another queue would not respect: no overlap
// on this engine from here on)
void *dslam_engine_stream(dslam_engine *e) {
  flush_deferred(e);
  if (!e) return nullptr;
  e->stream_lent = true;
  return (void *)static_cast<hipStream_t>(e->stream);
}

// ---- scene ---------------------------------------------------------------------------------------------------
// Every device / pinned allocation of a handle lives in an owner (dslam_memory.h) that is a member of the handle: deleting the
// handle frees whatever is there, so no error path leaks, and a half-built object is simply deleted by its create call.
static int scene_allocate(dslam_engine *e, dslam_scene *s, void *ext_voxels) {
  DSLAM_TRY(s->hash.alloc(s->n_entries));
  if (!ext_voxels) DSLAM_TRY(s->voxels_own.alloc((size_t)s->p.num_local_blocks * kBlock3));
  s->voxels = ext_voxels ? reinterpret_cast<uint2 *>(ext_voxels) : s->voxels_own.get();
  DSLAM_TRY(s->alloc_list.alloc(s->p.num_local_blocks));
  DSLAM_TRY(s->excess_list.alloc(s->p.num_excess));
  DSLAM_TRY(s->last_seen.alloc(s->p.num_local_blocks));
  DSLAM_TRY(s->masks.alloc((size_t)s->p.num_local_blocks * 2 * s->history_words));
  DSLAM_TRY(s->counters.alloc(1));
  DSLAM_TRY(s->alloc_bits.alloc((size_t)bit_tiles(s->n_entries) * kBitTileWords));
  if (s->p.use_swapping) {
    DSLAM_TRY(s->swap_state.alloc(s->n_entries));
    DSLAM_TRY(s->swap1_bits.alloc((size_t)bit_tiles(s->n_entries) * kBitTileWords));
    DSLAM_TRY(s->slot_dev.alloc(s->n_entries));
    DSLAM_HIP(hipMemsetAsync(s->slot_dev, 0xff, (size_t)s->n_entries * sizeof(int), e->stream));  // -1 everywhere
    DSLAM_TRY(s->next_slot_host.alloc(16));
    *s->next_slot_host = 0;
    DSLAM_TRY(s->slab_ptrs_dev.alloc(kMaxSlabs));
  }
  int rc = ensure_scratch(e, s->n_entries, s->p.num_local_blocks);
  if (rc) return rc;
  if ((rc = launch_scene_reset(e, s))) return rc;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

int dslam_scene_create(dslam_engine *e, const dslam_scene_params *p, void *ext_voxels, dslam_scene **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && p && out, "null argument");
  *out = nullptr;
  DSLAM_HIP(hipSetDevice(e->device));
  dslam_scene *s = new dslam_scene();
  s->version = next_map_version();
  s->engine = e;
  engine_adopt(e);
  s->p = *p;
  if (s->p.num_local_blocks <= 0) s->p.num_local_blocks = DSLAM_DEFAULT_LOCAL_BLOCK_NUM;
  if (s->p.num_buckets <= 0) s->p.num_buckets = DSLAM_DEFAULT_BUCKET_NUM;
  if (s->p.num_excess <= 0) s->p.num_excess = DSLAM_DEFAULT_EXCESS_LIST_SIZE;
  if (s->p.history_words <= 0) s->p.history_words = 4;
  s->history_words = s->p.history_words;
  if ((s->p.num_buckets & (s->p.num_buckets - 1)) || ((s->p.num_buckets + s->p.num_excess) & 15) ||
      s->p.max_w < 1 || s->p.max_w > 255 || !(s->p.voxel_size > 0) || !(s->p.mu > 0)) {
    delete s;
    engine_release(e);
    set_last_error("invalid scene parameters (buckets must be a power of two, entries a multiple of 16, 1<=max_w<=255)");
    return DSLAM_ERR_INVALID;
  }
  // the march's 32-bit byte offsets (raycast.hip, gather_taps_batched) reach slot DSLAM_MAX_LOCAL_BLOCKS - 1 and no further
  if (s->p.num_local_blocks > DSLAM_MAX_LOCAL_BLOCKS) {
    const int asked = s->p.num_local_blocks;
    delete s;
    engine_release(e);
    char msg[160];
    snprintf(msg, sizeof msg, "num_local_blocks %d exceeds DSLAM_MAX_LOCAL_BLOCKS (%d blocks, 4 GiB of voxels)", asked,
             DSLAM_MAX_LOCAL_BLOCKS);
    set_last_error(msg);
    return DSLAM_ERR_INVALID;
  }
  s->n_entries = s->p.num_buckets + s->p.num_excess;
  const int rc = scene_allocate(e, s, ext_voxels);
  if (rc) {
    (void)dslam_scene_destroy(s);  // frees whatever was allocated before the failure (last_error is kept)
    return rc;
  }
  *out = s;
  return DSLAM_OK;
}

// the scene's FrontEndRecord with buffers the size of r's (GetImage adopts them by exchanging pointers with its render
// state, so they are sized like a render state's: render_state_allocate)
static int front_end_for(dslam_engine *e, dslam_scene *s, const dslam_render_state *r, FrontEndRecord **out) {
  FrontEndRecord *f = s->front.get();
  if (f && f->w == r->w && f->h == r->h && f->n_local == r->n_local && f->n_entries == r->n_entries) {
    *out = f;
    return DSLAM_OK;
  }
  DSLAM_HIP(hipStreamSynchronize(e->stream));   // (the old buffers may still be in use)
  s->front.reset();
  // attached to the scene only complete: a failed allocation leaves the scene without a record, never with part of one
  std::unique_ptr<FrontEndRecord> n(new FrontEndRecord());
  n->w = r->w; n->h = r->h; n->n_local = r->n_local; n->n_entries = r->n_entries;
  DSLAM_TRY(n->visible_ids.alloc(n->n_local));
  DSLAM_TRY(n->proj_boxes.alloc(n->n_local)); DSLAM_TRY(n->proj_z.alloc(n->n_local)); DSLAM_TRY(n->proj_req.alloc(n->n_local));
  DSLAM_TRY(n->proj_wg_tiles.alloc((size_t)(n->n_entries / 1024 + 1024)));
  DSLAM_TRY(n->range.alloc((size_t)n->w * n->h));
  DSLAM_TRY(n->counters.alloc_zeroed(1, e->stream));
  s->front = std::move(n);
  *out = s->front.get();
  return DSLAM_OK;
}

int dslam_scene_destroy(dslam_scene *s) {
  if (!s) return DSLAM_OK;
  (void)hipSetDevice(s->engine->device);
  flush_deferred(s->engine);   // (on its own device: held calls launch kernels)
  (void)hipStreamSynchronize(s->engine->stream);
  dslam_engine *e = s->engine;
  delete s;
  engine_release(e);
  return DSLAM_OK;
}

// the host's share of a reset map: rings, decay cursors, frame counter (dslam_scene_reset, dslam_unpack_scene)
static void reset_host_cursors(dslam_scene *s) {
  for (int q = 0; q < 2; q++) { s->ring_head[q] = 0; s->ring_next[q] = 0; s->decay_cursor[q] = 0; }
  s->frame_counter = 0;
}

int dslam_scene_reset(dslam_engine *e, dslam_scene *s) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  int rc = launch_scene_reset(e, s);
  if (rc) return rc;
  reset_host_cursors(s);
  if (s->slot_dev) {  // the slabs stay; their slots are dealt again from the start (the counters were just zeroed)
    DSLAM_HIP(hipMemsetAsync(s->slot_dev, 0xff, (size_t)s->n_entries * sizeof(int), e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    *s->next_slot_host = 0;
    s->slot_bound = 0;
  }
  return finish_call(e);
}

int dslam_scene_get_params(const dslam_scene *s, dslam_scene_params *out) {
  DSLAM_REQUIRE(s && out, "null argument");
  *out = s->p;
  return DSLAM_OK;
}

int dslam_scene_set_shard(dslam_scene *s, int shard, int num_shards, int chunk_blocks) {
  if (s) flush_deferred(s->engine);
  DSLAM_REQUIRE(s && num_shards >= 1 && shard >= 0 && shard < num_shards && chunk_blocks >= 1, "bad shard spec");
  // A rank that does not own a block still swaps its (stale) copy of it out to ITS host store during the batch, and
  // the exchange moves device blocks only: the ranks' global caches would drift apart.  Refused, not silently wrong.
  DSLAM_REQUIRE(!(s->p.use_swapping && num_shards > 1), "a scene with host swapping cannot be sharded (the host store is per rank)");
  s->shard = shard; s->num_shards = num_shards; s->chunk_blocks = chunk_blocks;
  return DSLAM_OK;
}

int dslam_scene_set_shard_range(dslam_scene *s, int first_block, int num_blocks) {
  if (s) flush_deferred(s->engine);
  DSLAM_REQUIRE(s && first_block >= 0, "bad shard range");
  DSLAM_REQUIRE(!(s->p.use_swapping && num_blocks >= 0), "a scene with host swapping cannot be sharded (the host store is per rank)");
  s->shard_first = first_block; s->shard_count = num_blocks;
  return DSLAM_OK;
}

// ---- which blocks a sharded batch touched, and moving exactly those (csrc/shard.hip) ------------------------------
int dslam_scene_track_dirty(dslam_engine *e, dslam_scene *s, int enable) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  if (enable) {
    const size_t n = (size_t)s->p.num_local_blocks;
    if (!s->dirty) {
      SceneDirty d;   // (the scene gets the three together or none)
      DSLAM_TRY(d.dirty.alloc(n)); DSLAM_TRY(d.dirty_list.alloc(n)); DSLAM_TRY(d.dirty_counts.alloc(128));
      static_cast<SceneDirty &>(*s) = std::move(d);
    }
    DSLAM_HIP(hipMemsetAsync(s->dirty, 0, n, e->stream));
    s->dirty_shards = 0;
  }
  s->dirty_tracking = enable != 0;
  return finish_call(e);
}

int dslam_shard_dirty_plan(dslam_engine *e, dslam_scene *s, int num_shards, int chunk_blocks, int32_t *counts_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && counts_out, "null argument");
  return launch_dirty_plan(e, s, num_shards, chunk_blocks, counts_out);
}

int dslam_shard_dirty_pack(dslam_engine *e, const dslam_scene *s, int shard, void *send_dev, int capacity_blocks) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  int rc = launch_dirty_pack(e, s, shard, send_dev, capacity_blocks);
  if (rc) return rc;
  return finish_call(e);
}

int dslam_shard_dirty_unpack(dslam_engine *e, dslam_scene *s, int skip_shard, const void *recv_dev, int stride_blocks) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map changes: GetImage memos of this scene are stale
  int rc = launch_dirty_unpack(e, s, skip_shard, recv_dev, stride_blocks);
  if (rc) return rc;
  return finish_call(e);
}

// ---- render state / view --------------------------------------------------------------------------------------
static int render_state_allocate(dslam_engine *e, dslam_render_state *r) {
  const size_t npix = (size_t)r->w * r->h;
  DSLAM_TRY(r->visible_ids.alloc(r->n_local));
  DSLAM_TRY(r->vis_hint.alloc(16));
  *r->vis_hint = 0;
  DSLAM_TRY(r->visible_type.alloc_zeroed(r->n_entries, e->stream));
  DSLAM_TRY(r->vis_bits.alloc_zeroed((size_t)bit_tiles(r->n_entries) * kBitTileWords, e->stream));
  DSLAM_TRY(r->range.alloc_zeroed(npix, e->stream)); DSLAM_TRY(r->raycast.alloc_zeroed(npix, e->stream));
  DSLAM_TRY(r->image_rgba.alloc_zeroed(npix, e->stream)); DSLAM_TRY(r->image_float.alloc_zeroed(npix, e->stream));
  DSLAM_TRY(r->proj_boxes.alloc(r->n_local)); DSLAM_TRY(r->proj_z.alloc(r->n_local)); DSLAM_TRY(r->proj_req.alloc(r->n_local));
  DSLAM_TRY(r->proj_wg_tiles.alloc((size_t)(r->n_entries / 1024 + 1024)));
  DSLAM_TRY(r->counters.alloc_zeroed(1, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

int dslam_render_state_create(dslam_engine *e, const dslam_scene *s, int w, int h, dslam_render_state **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out && w > 0 && h > 0, "bad argument");
  *out = nullptr;
  dslam_render_state *r = new dslam_render_state();
  r->engine = e; engine_adopt(e); r->w = w; r->h = h; r->n_entries = s->n_entries; r->n_local = s->p.num_local_blocks;
  const int rc = render_state_allocate(e, r);
  if (rc) {
    (void)dslam_render_state_destroy(r);
    return rc;
  }
  *out = r;
  return DSLAM_OK;
}

int dslam_render_state_destroy(dslam_render_state *r) {
  if (!r) return DSLAM_OK;
  (void)hipSetDevice(r->engine->device);
  flush_deferred(r->engine);   // (on its own device: held calls launch kernels)
  (void)hipStreamSynchronize(r->engine->stream);
  dslam_engine *e = r->engine;
  delete r;
  engine_release(e);
  return DSLAM_OK;
}

static int view_allocate(dslam_engine *e, dslam_view *v) {
  const int w_rgb = v->w_rgb, h_rgb = v->h_rgb, w_d = v->w_d, h_d = v->h_d;
  // (the RGBA image and the int16 depth image in ONE allocation, the depth image at the next 256-byte boundary: a frame whose two
  // host images sit back to back the same way -- every 640x480 frame out of dslam_host_alloc -- goes up as one copy)
  const size_t c_round = ((size_t)w_rgb * h_rgb * sizeof(uchar4) + 255) & ~(size_t)255;
  DSLAM_TRY(v->rgba.alloc((c_round + (size_t)w_d * h_d * sizeof(short) + sizeof(uchar4) - 1) / sizeof(uchar4)));
  v->raw_depth = reinterpret_cast<short *>(reinterpret_cast<char *>(v->rgba.get()) + c_round);
  DSLAM_TRY(v->depth_own.alloc_zeroed((size_t)w_d * h_d, e->stream));
  v->depth = v->depth_own;
  v->rgba_src = v->rgba; v->raw_src = v->raw_depth;
  DSLAM_HIP(hipMemsetAsync(v->rgba, 0, (size_t)w_rgb * h_rgb * sizeof(uchar4), e->stream));
  DSLAM_HIP(hipMemsetAsync(v->raw_depth, 0, (size_t)w_d * h_d * sizeof(short), e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

int dslam_view_create(dslam_engine *e, int w_rgb, int h_rgb, int w_d, int h_d, dslam_view **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out && w_rgb > 0 && h_rgb > 0 && w_d > 0 && h_d > 0, "bad argument");
  *out = nullptr;
  dslam_view *v = new dslam_view();
  v->engine = e; engine_adopt(e); v->w_rgb = w_rgb; v->h_rgb = h_rgb; v->w_d = w_d; v->h_d = h_d;
  const int rc = view_allocate(e, v);
  if (rc) {
    (void)dslam_view_destroy(v);
    return rc;
  }
  *out = v;
  return DSLAM_OK;
}

int dslam_view_destroy(dslam_view *v) {
  if (!v) return DSLAM_OK;
  (void)hipSetDevice(v->engine->device);
  flush_deferred(v->engine);   // (on its own device: held calls launch kernels)
  (void)hipStreamSynchronize(v->engine->stream);
  if (v->engine->copy_stream) (void)hipStreamSynchronize(v->engine->copy_stream);
  for (int b = 0; b < 2; b++) release_lender(v, b);
  dslam_engine *e = v->engine;
  delete v;
  engine_release(e);
  return DSLAM_OK;
}

// common tail of the UpdateView entry points: remember the sources; with useBilateralFilter the float depth image
// is produced now (conversion + five filter passes), otherwise lazily by the next consumer
static int finish_view_update(dslam_engine *e, dslam_view *v, const void *rgba_dev, const void *depth_dev, float a,
                              float b, double timestamp, int use_bilateral) {
  int rc = launch_view_convert(e, v, rgba_dev, depth_dev, a, b);
  if (rc) return rc;
  if (use_bilateral) {
    DSLAM_REQUIRE(v->w_d >= 5 && v->h_d >= 5, "bilateral filter needs an image of at least 5x5");
    if ((rc = launch_bilateral(e, v))) return rc;
    e->view_reads++;  // (the filter reads the landing buffer: a fence recorded before it does not cover it)
  }
  v->timestamp = timestamp;
  return finish_call(e);
}

// ---- page-locked host buffers for the caller's input images ---------------------------------------------------
// Upstream ORUtils::MemoryBlock allocates its host side with cudaMallocHost whenever the block also has a device
// side; dslam_host_alloc gives the ITMLib mirror the same thing without it having to link the HIP runtime.  The
// engine remembers the ranges, so an upload from one of them can skip the staging copy.
static std::mutex g_pinned_mu;
static std::vector<std::pair<const char *, size_t>> g_pinned_ranges;
// Buffers of up to kArenaMax bytes are carved out of page-locked arenas one behind the other (256-byte granules), so that
// images a caller allocates in a row -- InfiniTamDriver's rgb_itm_ and raw_depth_itm_ (InfiniTamDriver.h:103-104), the bench's
// frame ring -- are CONTIGUOUS in host memory: dslam_view_update then moves a frame with one copy instead of two (one DMA
// start-up less per frame: what the pipelined upload path already did for callers that laid their frames out that way by
// hand).  An arena goes back to the runtime when its last buffer is freed.
namespace {
constexpr size_t kArenaMax = 8u << 20, kArenaBytes = 32u << 20;
struct PinnedArena { char *base; size_t used; int live; };
std::vector<PinnedArena> g_arenas;
}  // namespace

int dslam_host_alloc(size_t bytes, void **out) {
  DSLAM_REQUIRE(out, "null argument");
  const size_t need = ((bytes ? bytes : 1) + 255) & ~(size_t)255;
  std::lock_guard<std::mutex> lock(g_pinned_mu);
  void *p = nullptr;
  if (need <= kArenaMax) {
    if (g_arenas.empty() || g_arenas.back().used + need > kArenaBytes) {
      void *base = nullptr;
      DSLAM_HIP(hipHostMalloc(&base, kArenaBytes, hipHostMallocDefault));
      g_arenas.push_back({static_cast<char *>(base), 0, 0});
    }
    PinnedArena &a = g_arenas.back();
    p = a.base + a.used;
    a.used += need;
    a.live++;
  } else {
    DSLAM_HIP(hipHostMalloc(&p, need, hipHostMallocDefault));
  }
  memset(p, 0, bytes);
  g_pinned_ranges.emplace_back(static_cast<const char *>(p), bytes ? bytes : 1);
  *out = p;
  return DSLAM_OK;
}

int dslam_host_free(void *p) {
  if (!p) return DSLAM_OK;
  std::lock_guard<std::mutex> lock(g_pinned_mu);
  size_t i = 0;
  while (i < g_pinned_ranges.size() && g_pinned_ranges[i].first != p) i++;
  DSLAM_REQUIRE(i < g_pinned_ranges.size(), "dslam_host_free: pointer was not returned by dslam_host_alloc");
  g_pinned_ranges.erase(g_pinned_ranges.begin() + i);
  for (size_t k = 0; k < g_arenas.size(); k++) {
    PinnedArena &a = g_arenas[k];
    if (static_cast<char *>(p) >= a.base && static_cast<char *>(p) < a.base + kArenaBytes) {
      if (--a.live == 0) {   // (the arena that is being filled is kept while it has room: its next buffer may come at once)
        if (k + 1 == g_arenas.size() && a.used < kArenaBytes) { a.used = 0; return DSLAM_OK; }
        char *base = a.base;
        g_arenas.erase(g_arenas.begin() + k);
        DSLAM_HIP(hipHostFree(base));
      }
      return DSLAM_OK;
    }
  }
  DSLAM_HIP(hipHostFree(p));
  return DSLAM_OK;
}

static bool in_pinned_range(const void *p, size_t bytes) {
  const char *c = static_cast<const char *>(p);
  std::lock_guard<std::mutex> lock(g_pinned_mu);
  for (const auto &r : g_pinned_ranges)
    if (c >= r.first && c + bytes <= r.first + r.second) return true;
  return false;
}

// Async engine + page-locked RGBA / depth images: the copy runs on the engine's copy stream into landing buffer b of
// the view while the compute stream is still reading buffer b ^ 1 (the previous frame's kernels, enqueued earlier).
//   up_consumed[b]  recorded on the compute stream at the NEXT update, i.e. behind every kernel that reads buffer b;
//                   the copy that refills b (two updates later) may only start once it has passed
//   up_done[b]      recorded on the copy stream behind the copy; this frame's kernels may only start once it has passed
// Both conditions are awaited by the HOST (the calling thread sits out the copy, ~40 us per 640x480 frame, while the
// GPU works on the previous frame), not by hipStreamWaitEvent: on this runtime a cross-stream wait in front of a
// frame's kernels cost the compute stream ~30 us per frame (197 vs 167 us per step), more than the copy it hides;
// DSLAM_PIPELINE_STREAM_WAITS=1 selects that variant for measurement.
// *rgba_out / *raw_out receive the buffers the view reads from now on.
static int upload_view_pipelined(dslam_engine *e, dslam_view *v, const uint8_t *rgba_host, const int16_t *depth_host,
                                 const void **rgba_out, const void **raw_out) {
  static const bool stream_waits = getenv("DSLAM_PIPELINE_STREAM_WAITS") && atoi(getenv("DSLAM_PIPELINE_STREAM_WAITS")) != 0;
  const size_t c_bytes = (size_t)v->w_rgb * v->h_rgb * 4, d_bytes = (size_t)v->w_d * v->h_d * 2;
  if (!v->up_rgba[0]) {
    ViewLanding n;   // (the view gets both buffers and their events together or nothing)
    for (int b = 0; b < 2; b++) {
      // one allocation per landing buffer (RGBA image, then the depth image): a caller that keeps a frame's two images
      // back to back gets ONE copy per frame
      DSLAM_TRY(n.up_rgba[b].alloc((c_bytes + d_bytes + sizeof(uchar4) - 1) / sizeof(uchar4)));
      DSLAM_TRY(n.up_done[b].create()); DSLAM_TRY(n.up_consumed[b].create());
    }
    static_cast<ViewLanding &>(*v) = std::move(n);
    for (int b = 0; b < 2; b++) v->up_raw[b] = reinterpret_cast<short *>(reinterpret_cast<char *>(v->up_rgba[b].get()) + c_bytes);
  }
  const int b = v->up_next;
  v->up_next ^= 1;
  // Calls the engine holds back (a ProcessFrame's tail, the GetImage and the fence record behind it) are handed
  // to the GPU HERE, in front of the copy: the thread has nothing else to do until the copy's target is free and the copy
  // has landed, and the GPU gets the frame's fusion launch while the previous march still runs.  The copy then starts when
  // the auxiliary stream's pass is over -- beside that pass (k_mark above all) it lengthens the march, measured.
  // DSLAM_COPY_BEFORE_HELD_CALLS=1, a measurement's switch, enqueues the copy first and runs the held calls while it is in
  // flight (the thread sits out the upload and the auxiliary stream together; 3 % slower on the bench).
  // (Where the held tail leaves GetImage's front end on the auxiliary stream the copy goes BETWEEN the held calls: below.)
  // Either way the copy's target must be free.  The event that says so sits behind the previous GetImage's march; the stamp
  // the last allocation pass saw arrive proves the same earlier (every kernel that read a view and was called for by then
  // is complete), so in the steady state nobody waits for the march here.
  static const bool copy_first = getenv("DSLAM_COPY_BEFORE_HELD_CALLS") && atoi(getenv("DSLAM_COPY_BEFORE_HELD_CALLS")) != 0;
  auto enqueue_copy = [&]() -> int {
    if (reinterpret_cast<const uint8_t *>(depth_host) == rgba_host + c_bytes) {
      DSLAM_HIP(hipMemcpyAsync(v->up_rgba[b], rgba_host, c_bytes + d_bytes, hipMemcpyHostToDevice, e->copy_stream));
    } else {
      DSLAM_HIP(hipMemcpyAsync(v->up_rgba[b], rgba_host, c_bytes, hipMemcpyHostToDevice, e->copy_stream));
      DSLAM_HIP(hipMemcpyAsync(v->up_raw[b], depth_host, d_bytes, hipMemcpyHostToDevice, e->copy_stream));
    }
    return DSLAM_OK;
  };
  // Where the held ProcessFrame's tail leaves GetImage's front end on aux_stream, the copy is enqueued right
  // behind that tail -- the fusion launch is enqueued, k_mark and the sweep are over -- and the held GetImage sits out the
  // auxiliary stream and enqueues its march and the fence record while the copy is in flight.  Only if the target is known to
  // be free without a wait (the stamp's proof, above); otherwise, and on every other path, the copy follows the held calls.
  // DSLAM_COPY_BEHIND_HELD_CALLS=1, a measurement's switch, keeps it behind them always.
  static const bool copy_behind = getenv("DSLAM_COPY_BEHIND_HELD_CALLS") && atoi(getenv("DSLAM_COPY_BEHIND_HELD_CALLS")) != 0;
  bool copied = false;
  int copy_rc = DSLAM_OK;
  if (stream_waits || !copy_first) {
    if (!stream_waits && !copy_behind)
      e->after_tail = [&]() {
        if (v->up_used[b] && v->up_reads[b] > e->view_reads_done) return;
        copy_rc = enqueue_copy();
        copied = true;
      };
    flush_deferred(e);
    e->after_tail = nullptr;
  }
  if (copy_rc) return copy_rc;
  if (!copied) {
    if (v->up_used[b] && v->up_reads[b] > e->view_reads_done) {
      if (stream_waits) {
        DSLAM_HIP(hipStreamWaitEvent(e->copy_stream, v->up_consumed_by[b], 0));
      } else {
        flush_deferred(e);   // (the GPU is never kept waiting for the thread's wait)
        DSLAM_HIP(hipEventSynchronize(v->up_consumed_by[b]));
      }
    }
    DSLAM_TRY(enqueue_copy());
  }
  flush_deferred(e);   // (copy_first: now)
  // The other buffer's "consumed" mark, behind the held calls: the fusion launch that reads that buffer and the caller's
  // fence the mark borrows are only enqueued by them.
  if (v->up_used[b ^ 1]) {
    dslam_fence *f = e->last_fence;
    release_lender(v, b ^ 1);
    if (f && f->recorded && f->view_reads_at_record == e->view_reads) {
      // the caller's fence sits behind every kernel that read buffer b ^ 1 (no view was read since it was recorded)
      f->lent_count++;
      v->up_lender[b ^ 1] = f;
      v->up_consumed_by[b ^ 1] = f->ev;
    } else {
      DSLAM_HIP(hipEventRecord(v->up_consumed[b ^ 1], e->stream.peek()));   // (a marker touches no buffer: EngineStream)
      v->up_consumed_by[b ^ 1] = v->up_consumed[b ^ 1];
    }
    v->up_reads[b ^ 1] = e->view_reads;
  }
  if (stream_waits) {
    DSLAM_HIP(hipEventRecord(v->up_done[b], e->copy_stream));
    DSLAM_HIP(hipStreamWaitEvent(e->stream, v->up_done[b], 0));
  } else {
    // (the copy stream holds nothing but this frame's copy; waiting for the STREAM returns 8 us earlier than recording an event
    // behind the copy and waiting for that: 41 against 49 us for the 1.84 MB of a 640x480 frame, profiles/experiments/upload_bench.hip)
    DSLAM_HIP(hipStreamSynchronize(e->copy_stream));
  }
  v->up_used[b] = true;
  *rgba_out = v->up_rgba[b];
  *raw_out = v->up_raw[b];
  return DSLAM_OK;
}

static int upload_view_host(dslam_engine *e, dslam_view *v, const uint8_t *colour_host, int colour_channels,
                            const int16_t *depth_host) {
  const size_t c_bytes = (size_t)v->w_rgb * v->h_rgb * colour_channels, d_bytes = (size_t)v->w_d * v->h_d * 2;
  int rc = ensure_staging(e, (size_t)v->w_rgb * v->h_rgb * 4 + d_bytes);
  if (rc) return rc;
  const void *colour_src, *depth_src;
  if (!e->async_mode && in_pinned_range(colour_host, c_bytes) && in_pinned_range(depth_host, d_bytes)) {
    // page-locked caller buffers and a call that only returns once the stream has drained: DMA straight from them
    colour_src = colour_host; depth_src = depth_host;
  } else {
    // the caller may reuse its buffers right after the call (CvToItm rewrites them every frame), so stage through
    // pinned memory; in async mode the previous upload must have drained before the staging buffer is rewritten
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    memcpy(e->staging_host, colour_host, c_bytes);
    memcpy((char *)e->staging_host.get() + c_bytes, depth_host, d_bytes);
    colour_src = e->staging_host; depth_src = (char *)e->staging_host.get() + c_bytes;
  }
  void *colour_dst = colour_channels == 4 ? (void *)v->rgba : e->staging_dev;
  if (colour_channels == 4 && static_cast<const char *>(depth_src) == static_cast<const char *>(colour_src) + c_bytes &&
      reinterpret_cast<char *>(v->raw_depth) == reinterpret_cast<char *>(v->rgba.get()) + c_bytes) {
    DSLAM_HIP(hipMemcpyAsync(v->rgba, colour_src, c_bytes + d_bytes, hipMemcpyHostToDevice, e->stream));   // (one DMA instead of two: -8 us)
  } else {
    DSLAM_HIP(hipMemcpyAsync(colour_dst, colour_src, c_bytes, hipMemcpyHostToDevice, e->stream));
    DSLAM_HIP(hipMemcpyAsync(v->raw_depth, depth_src, d_bytes, hipMemcpyHostToDevice, e->stream));
  }
  if (colour_channels == 3) return launch_bgr_to_rgba(e, e->staging_dev, v->rgba, v->w_rgb * v->h_rgb);
  return DSLAM_OK;
}

int dslam_view_update(dslam_engine *e, dslam_view *v, const uint8_t *rgba_host, const int16_t *depth_host, float a,
                      float b, double timestamp, int use_bilateral) {
  DSLAM_REQUIRE(e && v && rgba_host && depth_host, "null argument");
  if (e->async_mode && in_pinned_range(rgba_host, (size_t)v->w_rgb * v->h_rgb * 4) &&
      in_pinned_range(depth_host, (size_t)v->w_d * v->h_d * 2)) {
    const void *rgba_dev = nullptr, *raw_dev = nullptr;
    int rc = upload_view_pipelined(e, v, rgba_host, depth_host, &rgba_dev, &raw_dev);
    if (rc) return rc;
    return finish_view_update(e, v, rgba_dev, raw_dev, a, b, timestamp, use_bilateral);
  }
  flush_deferred(e);
  int rc = upload_view_host(e, v, rgba_host, 4, depth_host);
  if (rc) return rc;
  return finish_view_update(e, v, v->rgba, v->raw_depth, a, b, timestamp, use_bilateral);
}

int dslam_view_update_device(dslam_engine *e, dslam_view *v, const void *rgba_dev, const void *depth_dev, float a,
                             float b, double timestamp, int use_bilateral) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && rgba_dev && depth_dev, "null argument");
  return finish_view_update(e, v, rgba_dev, depth_dev, a, b, timestamp, use_bilateral);
}

int dslam_view_update_bgr(dslam_engine *e, dslam_view *v, const uint8_t *bgr_host, const int16_t *depth_host, float a,
                          float b, double timestamp, int use_bilateral) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && bgr_host && depth_host, "null argument");
  int rc = upload_view_host(e, v, bgr_host, 3, depth_host);
  if (rc) return rc;
  return finish_view_update(e, v, v->rgba, v->raw_depth, a, b, timestamp, use_bilateral);
}

int dslam_view_update_bgr_device(dslam_engine *e, dslam_view *v, const void *bgr_dev, const void *depth_dev, float a,
                                 float b, double timestamp, int use_bilateral) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && bgr_dev && depth_dev, "null argument");
  DSLAM_REQUIRE(((uintptr_t)bgr_dev & 3) == 0, "bgr image must be 4-byte aligned");
  int rc = launch_bgr_to_rgba(e, bgr_dev, v->rgba, v->w_rgb * v->h_rgb);
  if (rc) return rc;
  return finish_view_update(e, v, v->rgba, depth_dev, a, b, timestamp, use_bilateral);
}

int dslam_view_update_dataset(dslam_engine *e, dslam_view *v, const uint8_t *colour_host, int channels,
                              const int16_t *depth_raw_host, int depth_format, float max_depth_m, float a, float b,
                              double timestamp, int use_bilateral) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && colour_host && depth_raw_host, "null argument");
  DSLAM_REQUIRE(channels == 3 || channels == 4, "colour_channels must be 3 (BGR) or 4 (RGBA)");
  DSLAM_REQUIRE(depth_format >= DSLAM_DEPTH_MM && depth_format <= DSLAM_DEPTH_RGBD_X5, "unknown depth format");
  int rc = upload_view_host(e, v, colour_host, channels, depth_raw_host);
  if (rc) return rc;
  if (depth_format != DSLAM_DEPTH_MM && (rc = launch_dataset_depth(e, v->raw_depth, v->w_d * v->h_d, depth_format, max_depth_m))) return rc;
  return finish_view_update(e, v, v->rgba, v->raw_depth, a, b, timestamp, use_bilateral);
}

int dslam_download_view_raw_depth(dslam_engine *e, const dslam_view *v, int16_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && out, "null argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  DSLAM_HIP(hipMemcpyAsync(out, v->raw_src, (size_t)v->w_d * v->h_d * 2, hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

int dslam_download_view_rgba(dslam_engine *e, const dslam_view *v, uint8_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && out, "null argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  DSLAM_HIP(hipMemcpyAsync(out, v->rgba_src, (size_t)v->w_rgb * v->h_rgb * 4, hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

// ---- keyframe store (fusion-frame database payload resident in HBM) -------------------------------------------
int dslam_frame_store_create(dslam_engine *e, int w_rgb, int h_rgb, int w_d, int h_d, int capacity, dslam_frame_store **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out && w_rgb > 0 && h_rgb > 0 && w_d > 0 && h_d > 0 && capacity > 0, "bad argument");
  std::unique_ptr<dslam_frame_store> fs(new dslam_frame_store());
  fs->engine = e; fs->w_rgb = w_rgb; fs->h_rgb = h_rgb; fs->w_d = w_d; fs->h_d = h_d; fs->capacity = capacity;
  // slots are padded to 256 bytes so every image starts on an aligned address whatever the image size
  fs->rgba_bytes = ((size_t)w_rgb * h_rgb * 4 + 255) & ~(size_t)255;
  fs->depth_bytes = ((size_t)w_d * h_d * 2 + 255) & ~(size_t)255;
  DSLAM_TRY(fs->rgba.alloc(fs->rgba_bytes * capacity)); DSLAM_TRY(fs->depth.alloc(fs->depth_bytes * capacity));
  engine_adopt(e);   // (only a complete store is a handle: a half-built one goes with `fs`, without a destroy call)
  *out = fs.release();
  return DSLAM_OK;
}

int dslam_frame_store_destroy(dslam_frame_store *fs) {
  if (!fs) return DSLAM_OK;
  (void)hipSetDevice(fs->engine->device);
  flush_deferred(fs->engine);   // (on its own device: held calls launch kernels)
  (void)hipStreamSynchronize(fs->engine->stream);
  dslam_engine *e = fs->engine;
  delete fs;
  engine_release(e);
  return DSLAM_OK;
}

static int store_slot_ok(const dslam_engine *e, const dslam_frame_store *fs, int slot) {
  DSLAM_REQUIRE(e && fs && fs->engine == e, "frame store belongs to a different engine");
  DSLAM_REQUIRE(slot >= 0 && slot < fs->capacity, "frame store slot out of range");
  return DSLAM_OK;
}

static int store_put_host(dslam_engine *e, dslam_frame_store *fs, int slot, const uint8_t *colour, int channels, const int16_t *depth) {
  int rc = store_slot_ok(e, fs, slot);
  if (rc) return rc;
  DSLAM_REQUIRE(colour && depth, "null argument");
  const size_t c_bytes = (size_t)fs->w_rgb * fs->h_rgb * channels, d_bytes = (size_t)fs->w_d * fs->h_d * 2;
  if ((rc = ensure_staging(e, (size_t)fs->w_rgb * fs->h_rgb * 4 + d_bytes))) return rc;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  memcpy(e->staging_host, colour, c_bytes);
  memcpy((char *)e->staging_host.get() + c_bytes, depth, d_bytes);
  unsigned char *rgba_dst = fs->rgba + fs->rgba_bytes * slot;
  DSLAM_HIP(hipMemcpyAsync(channels == 4 ? (void *)rgba_dst : e->staging_dev, e->staging_host, c_bytes, hipMemcpyHostToDevice, e->stream));
  DSLAM_HIP(hipMemcpyAsync(fs->depth + fs->depth_bytes * slot, (char *)e->staging_host.get() + c_bytes, d_bytes, hipMemcpyHostToDevice, e->stream));
  if (channels == 3 && (rc = launch_bgr_to_rgba(e, e->staging_dev, (uchar4 *)rgba_dst, fs->w_rgb * fs->h_rgb))) return rc;
  return finish_call(e);
}

int dslam_frame_store_put(dslam_engine *e, dslam_frame_store *fs, int slot, const uint8_t *rgba_host, const int16_t *depth_host) {
  flush_deferred(e);
  return store_put_host(e, fs, slot, rgba_host, 4, depth_host);
}
int dslam_frame_store_put_bgr(dslam_engine *e, dslam_frame_store *fs, int slot, const uint8_t *bgr_host, const int16_t *depth_host) {
  flush_deferred(e);
  return store_put_host(e, fs, slot, bgr_host, 3, depth_host);
}

int dslam_frame_store_put_view(dslam_engine *e, dslam_frame_store *fs, int slot, const dslam_view *v) {
  flush_deferred(e);
  int rc = store_slot_ok(e, fs, slot);
  if (rc) return rc;
  DSLAM_REQUIRE(v && v->engine == e, "null argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  DSLAM_REQUIRE(v->w_rgb == fs->w_rgb && v->h_rgb == fs->h_rgb && v->w_d == fs->w_d && v->h_d == fs->h_d, "view and frame store sizes differ");
  DSLAM_HIP(hipMemcpyAsync(fs->rgba + fs->rgba_bytes * slot, v->rgba_src, (size_t)fs->w_rgb * fs->h_rgb * 4, hipMemcpyDeviceToDevice, e->stream));
  DSLAM_HIP(hipMemcpyAsync(fs->depth + fs->depth_bytes * slot, v->raw_src, (size_t)fs->w_d * fs->h_d * 2, hipMemcpyDeviceToDevice, e->stream));
  return finish_call(e);
}

int dslam_frame_store_get(dslam_engine *e, const dslam_frame_store *fs, int slot, uint8_t *rgba_out, int16_t *depth_out) {
  flush_deferred(e);
  int rc = store_slot_ok(e, fs, slot);
  if (rc) return rc;
  if (rgba_out) DSLAM_HIP(hipMemcpyAsync(rgba_out, fs->rgba + fs->rgba_bytes * slot, (size_t)fs->w_rgb * fs->h_rgb * 4, hipMemcpyDeviceToHost, e->stream));
  if (depth_out) DSLAM_HIP(hipMemcpyAsync(depth_out, fs->depth + fs->depth_bytes * slot, (size_t)fs->w_d * fs->h_d * 2, hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

int dslam_frame_store_device_ptrs(const dslam_frame_store *fs, int slot, void **rgba_dev, void **depth_dev) {
  DSLAM_REQUIRE(fs && slot >= 0 && slot < fs->capacity, "frame store slot out of range");
  if (rgba_dev) *rgba_dev = fs->rgba + fs->rgba_bytes * slot;
  if (depth_dev) *depth_dev = fs->depth + fs->depth_bytes * slot;
  return DSLAM_OK;
}

int dslam_view_update_from_store(dslam_engine *e, dslam_view *v, const dslam_frame_store *fs, int slot, float a, float b,
                                 double timestamp, int use_bilateral) {
  flush_deferred(e);
  int rc = store_slot_ok(e, fs, slot);
  if (rc) return rc;
  DSLAM_REQUIRE(v && v->engine == e, "null argument");
  DSLAM_REQUIRE(v->w_rgb == fs->w_rgb && v->h_rgb == fs->h_rgb && v->w_d == fs->w_d && v->h_d == fs->h_d, "view and frame store sizes differ");
  return finish_view_update(e, v, fs->rgba + fs->rgba_bytes * slot, fs->depth + fs->depth_bytes * slot, a, b, timestamp, use_bilateral);
}

// ---- the visible list of a keyframe's fusion, kept with the keyframe ------------------------------------------------
static const size_t kListHeader = 64;  // (a RenderCounters-shaped count block, padded)

int dslam_frame_store_enable_lists(dslam_engine *e, dslam_frame_store *fs, const dslam_scene *s) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && fs && s && fs->engine == e, "bad argument");
  if (fs->lists && fs->list_cap >= s->p.num_local_blocks && fs->list_entries == s->n_entries) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  // regrow: on failure the old lists, their sizes and has_list[] / list_ptr[] stay as they were
  const size_t list_bytes = (kListHeader + (size_t)s->p.num_local_blocks * (sizeof(int) + sizeof(short4)) + 255) & ~(size_t)255;
  DeviceBuffer<unsigned char> lists;
  DSLAM_TRY(lists.alloc(list_bytes * fs->capacity));
  fs->lists = std::move(lists);
  fs->list_cap = s->p.num_local_blocks;
  fs->list_entries = s->n_entries;   // the lists hold entry ids of a table of this size (checked wherever a list is read)
  fs->list_bytes = list_bytes;
  fs->has_list.assign(fs->capacity, 0);
  fs->list_ptr.resize(fs->capacity);
  for (int i = 0; i < fs->capacity; i++) fs->list_ptr[i] = fs->lists + fs->list_bytes * i;
  fs->batch_lists.reset();   // (sized for the old lists)
  fs->batch_list_ptr.clear();
  return DSLAM_OK;
}

static unsigned char *list_slot(const dslam_frame_store *fs, int slot) { return fs->list_ptr[slot]; }

int dslam_frame_store_put_visible_list(dslam_engine *e, dslam_frame_store *fs, int slot, const dslam_scene *s,
                                       const dslam_render_state *r) {
  flush_deferred(e);
  int rc = store_slot_ok(e, fs, slot);
  if (rc) return rc;
  DSLAM_REQUIRE(s && r && fs->lists, "dslam_frame_store_enable_lists has not been called");
  DSLAM_REQUIRE(fs->list_cap >= r->n_local, "the store's lists are smaller than this render state's visible list");
  DSLAM_REQUIRE(fs->list_entries == s->n_entries && r->n_entries == s->n_entries, "the store's lists were enabled for a table of another size");
  unsigned char *base = list_slot(fs, slot);
  rc = launch_store_visible_list(e, s, r, base, reinterpret_cast<int *>(base + kListHeader),
                                 reinterpret_cast<short4 *>(base + kListHeader + (size_t)fs->list_cap * sizeof(int)), fs->list_cap);
  if (rc) return rc;
  fs->has_list[slot] = 1;
  return finish_call(e);
}

int dslam_deprocess_frame_stored(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_frame_store *fs, int slot,
                                 const float M_d[16], const float intr_d[4], const float M_rgb[16], const float intr_rgb[4]) {
  flush_deferred(e);
  int rc = store_slot_ok(e, fs, slot);
  if (rc) return rc;
  DSLAM_REQUIRE(s && v && M_d && intr_d && s->engine == e && v->engine == e, "bad argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  DSLAM_REQUIRE(fs->lists && fs->has_list[slot], "no visible list was stored for this keyframe slot");
  DSLAM_REQUIRE(fs->list_entries == s->n_entries, "the stored list belongs to a table of another size");   // (its ids index this scene's table)
  s->version = next_map_version();  // the map changes: GetImage memos of this scene are stale
  const unsigned char *base = list_slot(fs, slot);
  rc = launch_integrate_list(e, s, v, base, reinterpret_cast<const int *>(base + kListHeader),
                             reinterpret_cast<const short4 *>(base + kListHeader + (size_t)fs->list_cap * sizeof(int)), M_d, intr_d,
                             M_rgb, intr_rgb, true);
  if (rc) return rc;
  return finish_call(e);
}

// ---- the re-integration batch, block-major (integrate.hip) ---------------------------------------------------------------
namespace {
constexpr int kBatchMax = 32;   // keyframes per launch of the block kernel: two operation bits each in a 64-bit mask
}  // namespace

// A batch that stops after its first mutation (only a HIP failure can do that: every argument was checked before) leaves
// allocation passes applied whose blocks were never de- or re-integrated: the map is neither the old nor the new one.
// The header says so; what can be kept consistent is: the render state's list is re-derived by its next pass, and the
// keyframes of the chunk lose their stored lists (a later batch refuses them instead of de-integrating from stale lists).
static int batch_failed(dslam_scene *s, dslam_render_state *r, dslam_frame_store *fs, const int32_t *slots, int K, int rc) {
  s->alloc_born = nullptr;
  r->types_follow_list = false;
  r->memo_valid = false;
  for (int k = 0; k < K; k++) fs->has_list[slots[k]] = 0;
  return rc;
}

static int batch_scratch(dslam_engine *e, dslam_scene *s, dslam_frame_store *fs) {
  const size_t L = (size_t)s->p.num_local_blocks;
  const size_t npix = (size_t)fs->w_d * fs->h_d;
  if (s->batch_depth_pixels < npix) {   // (1.2 MB per 640x480 keyframe: 39 MB for the 32 of a chunk)
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    // regrow: the old images go first (they can be large); on failure the scene has no images and batch_depth_pixels == 0
    s->batch_depth.reset();
    s->batch_depth_pixels = 0;
    DSLAM_TRY(s->batch_depth.alloc((size_t)kBatchMax * npix));
    s->batch_depth_pixels = npix;
  }
  if (!s->batch_born) {
    SceneBatch n;   // (the scene gets the whole group or nothing: batch_born is the guard for all of it)
    DSLAM_TRY(n.batch_born.alloc(L)); DSLAM_TRY(n.batch_opmask.alloc(L)); DSLAM_TRY(n.batch_slot_entry.alloc(L));
    DSLAM_TRY(n.batch_marks.alloc_zeroed(L * 64, e->stream));   // (every batch leaves them zero again)
    DSLAM_TRY(n.batch_order.alloc(8 * L));
    DSLAM_TRY(n.batch_counters.alloc(16));   // [0..8): blocks per class, [8]: block-operations
    DSLAM_TRY(n.batch_ops_dev.alloc(2 * kBatchMax)); DSLAM_TRY(n.batch_lists_dev.alloc(3 * kBatchMax));
    DSLAM_TRY(n.batch_staging.alloc(2 * kBatchMax * sizeof(BatchOp) + 3 * kBatchMax * sizeof(BatchListRef)));
    DSLAM_TRY(n.batch_staging_ev.create());
    static_cast<SceneBatch &>(*s) = std::move(n);
  }
  if (!fs->batch_lists) {
    DeviceBuffer<unsigned char> lists;
    DSLAM_TRY(lists.alloc_zeroed(fs->list_bytes * kBatchMax, e->stream));   // (the count headers)
    fs->batch_lists = std::move(lists);
    fs->batch_list_ptr.resize(kBatchMax);
    for (int i = 0; i < kBatchMax; i++) fs->batch_list_ptr[i] = fs->batch_lists + fs->list_bytes * i;
  }
  (void)e;
  return DSLAM_OK;
}

int dslam_reintegrate_batch(dslam_engine *e, dslam_scene *s, dslam_view *v, dslam_render_state *r, dslam_frame_store *fs,
                            int n, const int32_t *slots, const float *old_M, const float *new_M, const float intr[4],
                            float affine_a, float affine_b) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && v && r && fs && intr && n >= 0 && (n == 0 || (slots && old_M && new_M)), "null argument");
  DSLAM_REQUIRE(s->engine == e && v->engine == e && r->engine == e && fs->engine == e, "objects belong to a different engine");
  DSLAM_REQUIRE(fs->lists, "dslam_frame_store_enable_lists has not been called");
  DSLAM_REQUIRE(v->w_rgb == fs->w_rgb && v->h_rgb == fs->h_rgb && v->w_d == fs->w_d && v->h_d == fs->h_d, "view and frame store sizes differ");
  DSLAM_REQUIRE(fs->list_cap >= r->n_local, "the store's lists are smaller than this render state's visible list");
  DSLAM_REQUIRE(fs->list_entries == s->n_entries && r->n_entries == s->n_entries, "the store's lists / the render state belong to a table of another size");
  if (s->p.use_swapping || s->p.stop_integrating_at_max_w || v->w_rgb != v->w_d || v->h_rgb != v->h_d) {
    set_last_error("dslam_reintegrate_batch: scenes with host swapping or stopIntegratingAtMaxW and views with a separate colour "
                   "camera take the per-keyframe calls (dslam_deprocess_frame_stored + dslam_process_frame)");
    return DSLAM_ERR_UNSUPPORTED;
  }
  for (int k = 0; k < n; k++) {
    DSLAM_REQUIRE(slots[k] >= 0 && slots[k] < fs->capacity, "frame store slot out of range");
    DSLAM_REQUIRE(fs->has_list[slots[k]], "no visible list was stored for a keyframe of the batch");
    for (int j = 0; j < k; j++) DSLAM_REQUIRE(slots[j] != slots[k], "a keyframe appears twice in the batch");
  }
  // everything that can be refused is refused here, before anything changes: what launch_allocate checks per pass
  // (table size above, an invertible pose, the order key's range) for every keyframe of the batch
  for (int k = 0; k < n; k++) {
    float inv[16];
    if (!invert_matrix(new_M + 16 * (size_t)k, inv)) { set_last_error("dslam_reintegrate_batch: a new pose matrix is singular"); return DSLAM_ERR_INVALID; }
  }
  { int cap; const int rc_cap = alloc_step_cap(s, v->w_d, v->h_d, &cap); if (rc_cap) return rc_cap; }
  int rc = batch_scratch(e, s, fs);   // (n = 0: a set-up call -- the buffers exist before the first batch needs them)
  if (rc) return rc;
  if ((rc = ensure_scratch(e, s->n_entries, s->p.num_local_blocks))) return rc;
  if (n == 0) return DSLAM_OK;
  e->view_reads++;  // (see dslam_engine::last_fence)
  s->version = next_map_version();  // the map changes: GetImage memos of this scene are stale
  r->memo_valid = false;
  const size_t L = (size_t)s->p.num_local_blocks;
  const size_t ids_off = kListHeader, pos_off = kListHeader + (size_t)fs->list_cap * sizeof(int);
  for (int first = 0; first < n; first += kBatchMax) {
    const int K = (n - first) < kBatchMax ? (n - first) : kBatchMax;
    DSLAM_HIP(hipMemsetAsync(s->batch_born, 0, L * sizeof(int), e->stream));
    DSLAM_HIP(hipMemsetAsync(s->batch_counters, 0, 16 * sizeof(int), e->stream));
    // (built in page-locked memory: the copies are queued behind the allocation passes and nothing waits for them here)
    DSLAM_HIP(hipEventSynchronize(s->batch_staging_ev));   // the previous batch's copies have left the buffer
    BatchOp *ops = reinterpret_cast<BatchOp *>(s->batch_staging.get());
    BatchListRef *lists = reinterpret_cast<BatchListRef *>(ops + 2 * kBatchMax);   // [2K, 3K): the lists whose block positions are filled in at the end
    // phase 1: the allocation passes of the K re-fusions, in keyframe order (they read the table and the keyframes' depth
    // images, not the voxels); every pass' list goes to a scratch buffer, the blocks it allocates are stamped
    s->alloc_born = s->batch_born;
    int n_pos_jobs = 0;
    // a list buffer (header, ids, positions) as the kernels take it
    auto list_ref = [&](const unsigned char *b, bool with_pos) {
      return BatchListRef{reinterpret_cast<const RenderCounters *>(b), reinterpret_cast<const int *>(b + ids_off),
                          with_pos ? reinterpret_cast<const short4 *>(b + pos_off) : nullptr};
    };
    float *const view_depth = v->depth;
    for (int k = 0; k < K; k++) {
      const int slot = slots[first + k];
      const void *rgba = fs->rgba + fs->rgba_bytes * slot, *raw = fs->depth + fs->depth_bytes * slot;
      if ((rc = launch_view_convert(e, v, rgba, raw, affine_a, affine_b))) break;
      // the pass derives the keyframe's metric depth image (as UpdateView would) -- into the batch's own image k, where
      // both operations of the keyframe read it in the block launch
      v->depth = s->batch_depth + (size_t)k * s->batch_depth_pixels;
      s->alloc_born_stamp = k + 1;
      // the pass writes its list straight into the scratch list of keyframe k; the last one into the render state's own
      // (what the loop of per-keyframe calls leaves there), from where it is copied
      unsigned char *nb = fs->batch_list_ptr[k];
      const bool last_pass = first + k == n - 1;
      if ((rc = launch_allocate(e, s, v, r, new_M + 16 * (size_t)(first + k), intr, 0, last_pass ? nullptr : reinterpret_cast<int *>(nb + ids_off),
                                last_pass ? nullptr : nb)))
        break;
      int bit = 0, frame = 0;
      if ((rc = prepare_push_visible_list(e, s, 1, &bit, &frame))) break;   // (ProcessFrame(isDefusion) queues on ring 1)
      if (last_pass) {
        if ((rc = launch_store_visible_list(e, s, r, nb, reinterpret_cast<int *>(nb + ids_off), reinterpret_cast<short4 *>(nb + pos_off),
                                            fs->list_cap)))
          break;
      } else {
        lists[2 * K + n_pos_jobs++] = list_ref(nb, true);
      }
      const unsigned char *ob = list_slot(fs, slot);
      BatchOp &d = ops[2 * k], &f = ops[2 * k + 1];
      memcpy(d.M.m, old_M + 16 * (size_t)(first + k), 64);
      memcpy(f.M.m, new_M + 16 * (size_t)(first + k), 64);
      d.depth = f.depth = v->depth; d.rgba = f.rgba = static_cast<const uchar4 *>(rgba);
      d.push_bit = d.push_frame = 0; f.push_bit = bit; f.push_frame = frame;
      lists[2 * k] = list_ref(ob, true);
      lists[2 * k + 1] = list_ref(nb, false);
    }
    s->alloc_born = nullptr;
    v->depth = view_depth;
    v->depth_dirty = true;   // (the view's own float image was not written: its next consumer derives it)
    if (rc) return batch_failed(s, r, fs, slots + first, K, rc);
    // phase 2: which operations touch which block, then every touched block once
    DSLAM_HIP(hipMemcpyAsync(s->batch_ops_dev, ops, 2 * (size_t)K * sizeof(BatchOp), hipMemcpyHostToDevice, e->stream));
    DSLAM_HIP(hipMemcpyAsync(s->batch_lists_dev, lists, 3 * (size_t)K * sizeof(BatchListRef), hipMemcpyHostToDevice, e->stream));
    DSLAM_HIP(hipEventRecord(s->batch_staging_ev, e->stream));
    if ((rc = launch_batch_ops(e, s->batch_lists_dev, 2 * K, s, s->batch_born, s->batch_marks, s->batch_opmask, s->batch_slot_entry,
                               s->batch_order, s->batch_counters)))
      return batch_failed(s, r, fs, slots + first, K, rc);
    if ((rc = launch_reintegrate_blocks(e, s, v->w_d, v->h_d, v->w_rgb, v->h_rgb, intr, s->batch_ops_dev,
                                        s->batch_opmask, s->batch_slot_entry, s->batch_order, s->batch_counters, 1, 2 * K)))
      return batch_failed(s, r, fs, slots + first, K, rc);
    if ((rc = launch_store_list_positions(e, s, s->batch_lists_dev + 2 * K, n_pos_jobs)))
      return batch_failed(s, r, fs, slots + first, K, rc);
    // the lists of the re-fusions become the keyframes' stored lists: the buffers trade places
    for (int k = 0; k < K; k++) std::swap(fs->list_ptr[slots[first + k]], fs->batch_list_ptr[k]);
  }
  return finish_call(e);
}

int dslam_reintegrate_batch_stats(dslam_engine *e, const dslam_scene *s, int32_t *blocks_out, int32_t *block_operations_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && s->engine == e, "null argument");
  DSLAM_REQUIRE(s->batch_counters, "no batch has run on this scene");
  int host[16];
  DSLAM_HIP(hipMemcpyAsync(host, s->batch_counters, sizeof(host), hipMemcpyDeviceToHost, e->stream));
  const int rc = sync_check(e);
  if (rc) return rc;
  int blocks = 0;
  for (int c = 0; c < 8; c++) blocks += host[c];
  if (blocks_out) *blocks_out = blocks;
  if (block_operations_out) *block_operations_out = host[8];
  return DSLAM_OK;
}

// ---- depthPostProcessing -------------------------------------------------------------------------------------
static int depth_post_args(dslam_engine *e, const void *curr, const void *prev, int w, int h, const float *Tpc,
                           const float *intr) {
  DSLAM_REQUIRE(e && curr && prev && Tpc && intr, "null argument");
  DSLAM_REQUIRE(w > 0 && h > 0, "bad image size");
  return DSLAM_OK;
}

int dslam_depth_post_processing_device(dslam_engine *e, void *curr_dev, const void *prev_dev, int w, int h,
                                       const float Tpc[16], const float intr[4], float threshold, float area,
                                       int *count_out) {
  flush_deferred(e);
  int rc = depth_post_args(e, curr_dev, prev_dev, w, h, Tpc, intr);
  if (rc) return rc;
  int *count_dev = e->misc_counter;
  if ((rc = launch_depth_post(e, (short *)curr_dev, (const unsigned short *)prev_dev, w, h, Tpc, intr, threshold, area, count_dev))) return rc;
  if (count_out) {
    DSLAM_HIP(hipMemcpyAsync(e->pinned, count_dev, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    *count_out = *(int *)e->pinned.get();
    return DSLAM_OK;
  }
  return finish_call(e);
}

int dslam_depth_post_processing(dslam_engine *e, int16_t *curr_host, const int16_t *prev_host, int w, int h,
                                const float Tpc[16], const float intr[4], float threshold, float area,
                                int *count_out) {
  flush_deferred(e);
  int rc = depth_post_args(e, curr_host, prev_host, w, h, Tpc, intr);
  if (rc) return rc;
  const size_t d_bytes = (size_t)w * h * 2;
  if ((rc = ensure_staging(e, 2 * d_bytes))) return rc;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  memcpy(e->staging_host, curr_host, d_bytes);
  memcpy((char *)e->staging_host.get() + d_bytes, prev_host, d_bytes);
  DSLAM_HIP(hipMemcpyAsync(e->staging_dev, e->staging_host, 2 * d_bytes, hipMemcpyHostToDevice, e->stream));
  int *count_dev = e->misc_counter;
  if ((rc = launch_depth_post(e, (short *)e->staging_dev.get(), (const unsigned short *)((char *)e->staging_dev.get() + d_bytes), w, h, Tpc,
                              intr, threshold, area, count_dev)))
    return rc;
  DSLAM_HIP(hipMemcpyAsync(e->staging_host, e->staging_dev, d_bytes, hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipMemcpyAsync(e->pinned, count_dev, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  memcpy(curr_host, e->staging_host, d_bytes);
  if (count_out) *count_out = *(int *)e->pinned.get();
  return DSLAM_OK;
}

// ---- fusion --------------------------------------------------------------------------------------------------
int dslam_set_fusion_weight_params(dslam_engine *e, const dslam_weight_params *w) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && w, "null argument");
  // newW <= 255: the voxel weight is one byte and k_integrate indexes its reciprocal table with w_depth + newW <= 510
  DSLAM_REQUIRE(!w->depth_weighting || (w->max_distance > 0 && w->max_new_w >= 1 && w->max_new_w <= 255),
                "bad weight params (need max_distance > 0 and 1 <= max_new_w <= 255)");
  e->wp = *w;
  return DSLAM_OK;
}

static int check_frame_args(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_render_state *r,
                            const float *M, const float *intr) {
  DSLAM_REQUIRE(e && s && v && r && M && intr, "null argument");
  DSLAM_REQUIRE(s->engine == e && v->engine == e && r->engine == e, "objects belong to a different engine");
  e->view_reads++;  // (see dslam_engine::last_fence)
  return DSLAM_OK;
}

int dslam_allocate_scene_from_depth(dslam_engine *e, dslam_scene *s, const dslam_view *v, dslam_render_state *r,
                                    const float M_d[16], const float intr[4], int only_visible) {
  flush_deferred(e);
  int rc = check_frame_args(e, s, v, r, M_d, intr);
  if (rc) return rc;
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  rc = launch_allocate(e, s, v, r, M_d, intr, only_visible);
  if (rc) return rc;
  return finish_call(e);
}

int dslam_integrate_into_scene(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_render_state *r,
                               const float M_d[16], const float intr_d[4], const float M_rgb[16],
                               const float intr_rgb[4]) {
  flush_deferred(e);
  int rc = check_frame_args(e, s, v, r, M_d, intr_d);
  if (rc) return rc;
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  rc = launch_integrate(e, s, v, r, M_d, intr_d, M_rgb, intr_rgb, false);
  if (rc) return rc;
  return finish_call(e);
}

// What is left of a ProcessFrame behind its allocation pass, with its arguments by value: it may run after the call has
// returned (dslam_engine::deferred), when the caller's arrays are gone.
namespace {
struct FrameTail {
  dslam_engine *e; dslam_scene *s; const dslam_view *v; dslam_render_state *r;
  float M_d[16], intr_d[4], M_rgb[16], intr_rgb[4];
  bool has_M_rgb, has_intr_rgb;
  int is_defusion;
  FrontEndRecord *front;
  unsigned long long version;   // the scene's version for this call
};
int frame_tail(const FrameTail &t) {
  dslam_engine *e = t.e;
  int rc;
  // The sweep of this pass ran on aux_stream (4h) and the engine may put the front end there as well (4i): the fusion launch
  // is then the plain one.  Only as a held call: flush_deferred sees to it that the front end is waited for.
  // Either the pass launched it behind its sweep (front_at_pass), or -- the measurement's order -- it goes behind this launch.
  const int front_on_aux = !(e->overlap_front && e->publish_due && e->flushing && t.front != nullptr) ? 0 : e->front_at_pass ? 2 : 1;
  e->front_at_pass = false;
  if ((rc = finish_overlapped_allocate(e, t.s))) return rc;
  if ((rc = launch_integrate(e, t.s, t.v, t.r, t.M_d, t.intr_d, t.has_M_rgb ? t.M_rgb : nullptr, t.has_intr_rgb ? t.intr_rgb : nullptr, false,
                             t.is_defusion, t.front, front_on_aux)))
    return rc;
  if (t.front && t.front->valid) {
    t.front->version = t.version;
    memcpy(t.front->M, t.M_d, sizeof(t.front->M));
    memcpy(t.front->intr, t.intr_d, sizeof(t.front->intr));
  }
  if (t.s->p.use_swapping) {
    if ((rc = launch_swap_in(e, t.s, t.r))) return rc;
    if ((rc = launch_swap_out(e, t.s, t.r, false))) return rc;
  }
  return finish_call(e);
}
}  // namespace

int dslam_process_frame(dslam_engine *e, dslam_scene *s, const dslam_view *v, dslam_render_state *r,
                        const float M_d[16], const float intr_d[4], const float M_rgb[16], const float intr_rgb[4],
                        int only_visible, int is_defusion) {
  flush_deferred(e);
  int rc = check_frame_args(e, s, v, r, M_d, intr_d);
  if (rc) return rc;
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  // GetImage's front end for this pose (FrontEndRecord): not with swapping, whose passes change the table behind the fusion
  FrontEndRecord *front = nullptr;
  if (s->front) s->front->valid = false;
  if (e->speculate_front && !s->p.use_swapping && r->n_entries == s->n_entries && (rc = front_end_for(e, s, r, &front))) return rc;
  bool publish_left = false;
  if ((rc = launch_allocate(e, s, v, r, M_d, intr_d, only_visible, nullptr, nullptr, &publish_left, front))) return rc;
  FrameTail tail{e, s, v, r, {}, {}, {}, {}, M_rgb != nullptr, intr_rgb != nullptr, is_defusion ? 1 : 0, front, s->version};
  memcpy(tail.M_d, M_d, sizeof(tail.M_d));
  memcpy(tail.intr_d, intr_d, sizeof(tail.intr_d));
  if (M_rgb) memcpy(tail.M_rgb, M_rgb, sizeof(tail.M_rgb));
  if (intr_rgb) memcpy(tail.intr_rgb, intr_rgb, sizeof(tail.intr_rgb));
  if (publish_left) {
    // k_mark and the sweep run on the auxiliary stream beside the previous GetImage's march; the call returns,
    // and the thread comes back for the rest when it has something to sit out (upload_view_pipelined) or touches the engine.
    defer_call(e, [tail]() { return frame_tail(tail); });
    return DSLAM_OK;
  }
  return frame_tail(tail);
}

int dslam_deprocess_frame(dslam_engine *e, dslam_scene *s, const dslam_view *v, dslam_render_state *r,
                          const float M_d[16], const float intr_d[4], const float M_rgb[16], const float intr_rgb[4]) {
  flush_deferred(e);
  int rc = check_frame_args(e, s, v, r, M_d, intr_d);
  if (rc) return rc;
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  if ((rc = launch_allocate(e, s, v, r, M_d, intr_d, 1))) return rc;
  if ((rc = launch_integrate(e, s, v, r, M_d, intr_d, M_rgb, intr_rgb, true))) return rc;
  return finish_call(e);
}

// ---- depth tracker -------------------------------------------------------------------------------------------
int dslam_track_camera(dslam_engine *e, const dslam_view *v, dslam_render_state *r, const float scene_pose_M[16],
                       float pose_M[16], const float intr[4], const dslam_tracker_params *params,
                       dslam_tracker_result *result) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && r && scene_pose_M && pose_M && intr && params, "null argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  DSLAM_REQUIRE(v->engine == e && r->engine == e, "objects belong to a different engine");
  return launch_track_camera(e, v, r, scene_pose_M, pose_M, intr, params, result);
}

// ---- what the calls that take maps and transforms check alike ----------------------------------------------------------
namespace {

// a rigid transform (column-major 4 x 4): every entry finite, the rotation block orthonormal to 1e-4
int check_rigid_transform(const float *T, const char *what) {
  for (int k = 0; k < 16; k++) DSLAM_REQUIRE(std::isfinite(T[k]), std::string(what) + " is not finite");
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double dot = 0.0;
      for (int k = 0; k < 3; k++) dot += (double)T[a * 4 + k] * (double)T[b * 4 + k];
      DSLAM_REQUIRE(fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-4, std::string(what) + ": the rotation block is not orthonormal");
    }
  return DSLAM_OK;
}

// The map list (scenes[], T_map_from_world[], num_maps) of the call `call`; the caller has checked the pointers.  Where the
// calls differ: min_maps; rigid -- no scene twice and every transform rigid (check_rigid_transform),
// otherwise a scene may repeat and any transform invert_matrix inverts passes; max_local_blocks -- the most
// num_local_blocks a scene may have (the composite render's visible-list capacity), 0: any; max_maps -- the longest list
// (DSLAM_MAX_RENDER_MAPS for every call but the view survey).
int check_map_list(dslam_engine *e, const char *call, const dslam_scene *const *scenes, const float *T, int num_maps, int min_maps,
                   bool rigid, int max_local_blocks = 0, int max_maps = DSLAM_MAX_RENDER_MAPS) {
  auto msg = [call](const std::string &what) { return std::string(call) + ": " + what; };
  DSLAM_REQUIRE(num_maps >= min_maps && num_maps <= max_maps,
                msg("num_maps must be " + std::to_string(min_maps) + " .. " +
                    (max_maps == DSLAM_MAX_RENDER_MAPS ? std::string("DSLAM_MAX_RENDER_MAPS") : std::to_string(max_maps))));
  for (int i = 0; i < num_maps; i++) {
    const dslam_scene *s = scenes[i];
    DSLAM_REQUIRE(s, msg("a scene in the list is NULL"));
    DSLAM_REQUIRE(s->engine == e, msg("a scene in the list belongs to another engine"));
    if (rigid)
      for (int j = 0; j < i; j++) DSLAM_REQUIRE(scenes[j] != s, msg("a scene is listed twice"));
    // (dslam_scene_create admits only voxel_size > 0 and mu > 0, so equal values are equal bytes)
    DSLAM_REQUIRE(s->p.voxel_size == scenes[0]->p.voxel_size && s->p.mu == scenes[0]->p.mu,
                  msg("all maps of the list need the same voxel_size and mu"));
    DSLAM_REQUIRE(max_local_blocks == 0 || s->p.num_local_blocks <= max_local_blocks,
                  msg("the render state's visible-list capacity is below a scene's num_local_blocks"));
    float inv[16];
    if (rigid) DSLAM_TRY(check_rigid_transform(T + 16 * i, "a map transform"));
    else DSLAM_REQUIRE(invert_matrix(T + 16 * i, inv), msg("a map transform is singular"));
  }
  return DSLAM_OK;
}

// dslam_register_params with the zeros replaced by the defaults (params NULL: all defaults)
int default_register_params(const dslam_register_params *params, dslam_register_params *rp) {
  *rp = {0.0f, 0.0f, 0, 0, 0.0f, 0.0f};
  if (params) *rp = *params;
  DSLAM_REQUIRE(rp->band >= 0.0f && rp->residual_gate >= 0.0f && rp->max_evaluations >= 0 && rp->min_valid >= 0 &&
                    rp->term_rotation >= 0.0f && rp->term_translation_voxels >= 0.0f,
                "a registration parameter is negative (or not a number)");
  if (rp->band == 0.0f) rp->band = 0.5f;
  if (rp->residual_gate == 0.0f) rp->residual_gate = 0.75f;
  if (rp->max_evaluations == 0) rp->max_evaluations = 30;
  if (rp->min_valid == 0) rp->min_valid = 500;
  if (rp->term_rotation == 0.0f) rp->term_rotation = 1e-5f;
  if (rp->term_translation_voxels == 0.0f) rp->term_translation_voxels = 1e-3f;
  return DSLAM_OK;
}

// dslam_track_sdf_params with the zeros replaced by the defaults (params NULL: all defaults), checked against the view's size
int default_track_sdf_params(const dslam_view *v, const dslam_track_sdf_params *params, dslam_track_sdf_params *out) {
  dslam_track_sdf_params tp = {0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0};
  if (params) tp = *params;
  DSLAM_REQUIRE(tp.no_hierarchy_levels >= 0 && tp.run_till_level >= 0 && tp.max_evaluations >= 0 && tp.min_valid >= 0 &&
                    tp.residual_gate >= 0.0f && tp.term_rotation >= 0.0f && tp.term_translation_voxels >= 0.0f,
                "a tracking parameter is negative (or not a number)");
  if (tp.no_hierarchy_levels == 0) tp.no_hierarchy_levels = 3;
  if (tp.max_evaluations == 0) tp.max_evaluations = 10;
  if (tp.min_valid == 0) tp.min_valid = 500;
  if (tp.residual_gate == 0.0f) tp.residual_gate = 0.75f;
  if (tp.term_rotation == 0.0f) tp.term_rotation = 1e-5f;
  if (tp.term_translation_voxels == 0.0f) tp.term_translation_voxels = 1e-3f;
  DSLAM_REQUIRE(tp.no_hierarchy_levels <= DSLAM_TRACKER_MAX_LEVELS, "no_hierarchy_levels must be 1 .. DSLAM_TRACKER_MAX_LEVELS");
  DSLAM_REQUIRE((v->w_d >> (tp.no_hierarchy_levels - 1)) > 0 && (v->h_d >> (tp.no_hierarchy_levels - 1)) > 0,
                "too many hierarchy levels for this image size");
  DSLAM_REQUIRE(tp.run_till_level < tp.no_hierarchy_levels, "run_till_level is not one of the levels");
  *out = tp;
  return DSLAM_OK;
}

// what dslam_score_camera_poses and dslam_track_camera_sdf_starts check alike: dslam_track_camera_sdf's checks, on a pose list
int check_pose_list_call(dslam_engine *e, const char *call, const dslam_view *v, const dslam_scene *const *scenes, const float *T,
                         int num_maps, const float *poses_M, int num_poses, const float *intr) {
  DSLAM_REQUIRE(num_poses >= 1 && num_poses <= DSLAM_MAX_TRACK_STARTS,
                std::string(call) + ": the number of poses must be 1 .. DSLAM_MAX_TRACK_STARTS");
  DSLAM_TRY(check_map_list(e, call, scenes, T, num_maps, 1, true));
  DSLAM_REQUIRE(v->engine == e, "the view belongs to another engine");
  DSLAM_REQUIRE(v->updated, "the view was never updated");
  for (int k = 0; k < num_poses; k++) DSLAM_TRY(check_rigid_transform(poses_M + 16 * k, "a pose of the list"));
  for (int k = 0; k < 4; k++) DSLAM_REQUIRE(std::isfinite(intr[k]), "the intrinsics are not finite");
  return DSLAM_OK;
}

int copy_sums(const SumChannel &ch, const char *none, double out[33]) {
  DSLAM_REQUIRE(ch.have_sums, none);
  memcpy(out, ch.last_sums, sizeof ch.last_sums);
  return DSLAM_OK;
}

}  // namespace

// ---- depth-to-SDF tracker over all local maps --------------------------------------------------------------------

int dslam_track_camera_sdf(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T_map_from_world,
                           int num_maps, float pose_M[16], const float intr[4], const dslam_track_sdf_params *params,
                           dslam_track_sdf_result *result) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && scenes && T_map_from_world && pose_M && intr && result, "null argument");
  DSLAM_TRY(check_map_list(e, "dslam_track_camera_sdf", scenes, T_map_from_world, num_maps, 1, true));
  DSLAM_REQUIRE(v->engine == e, "the view belongs to another engine");
  DSLAM_REQUIRE(v->updated, "the view was never updated");
  DSLAM_TRY(check_rigid_transform(pose_M, "the start pose"));
  for (int k = 0; k < 4; k++) DSLAM_REQUIRE(std::isfinite(intr[k]), "the intrinsics are not finite");
  dslam_track_sdf_params tp;
  DSLAM_TRY(default_track_sdf_params(v, params, &tp));
  e->view_reads++;  // (see dslam_engine::last_fence)
  return launch_track_camera_sdf(e, v, scenes, T_map_from_world, num_maps, pose_M, intr, &tp, result);
}

int dslam_debug_track_sdf_sums(dslam_engine *e, double out[33]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  return copy_sums(e->track_sdf_sums, "no depth-to-SDF tracking evaluation has run on this engine", out);
}

// ---- depth-to-SDF tracker with a photometric term -------------------------------------------------------------------

int dslam_track_camera_sdf_rgb(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T_map_from_world,
                               int num_maps, float pose_M[16], const float intr[4], const dslam_track_sdf_rgb_params *params,
                               dslam_track_sdf_rgb_result *result) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && scenes && T_map_from_world && pose_M && intr && result, "null argument");
  DSLAM_TRY(check_map_list(e, "dslam_track_camera_sdf_rgb", scenes, T_map_from_world, num_maps, 1, true));
  DSLAM_REQUIRE(v->engine == e, "the view belongs to another engine");
  DSLAM_REQUIRE(v->updated, "the view was never updated");
  DSLAM_REQUIRE(v->w_rgb == v->w_d && v->h_rgb == v->h_d, "the view's colour and depth images differ in size");
  DSLAM_TRY(check_rigid_transform(pose_M, "the start pose"));
  for (int k = 0; k < 4; k++) DSLAM_REQUIRE(std::isfinite(intr[k]), "the intrinsics are not finite");
  dslam_track_sdf_rgb_params rp;
  memset(&rp, 0, sizeof rp);
  if (params) rp = *params;
  DSLAM_TRY(default_track_sdf_params(v, params ? &params->base : nullptr, &rp.base));
  DSLAM_REQUIRE(rp.colour_weight >= 0.0f && rp.colour_gate >= 0.0f, "colour_weight or colour_gate is negative (or not a number)");
  DSLAM_REQUIRE(rp.colour_levels >= 0 && rp.colour_levels <= rp.base.no_hierarchy_levels - rp.base.run_till_level,
                "colour_levels is negative or above the levels run");
  if (rp.colour_weight == 0.0f) rp.colour_weight = 1.0f;
  if (rp.colour_gate == 0.0f) rp.colour_gate = 0.25f;
  if (rp.colour_levels == 0) rp.colour_levels = 1;
  e->view_reads++;  // (see dslam_engine::last_fence)
  return launch_track_camera_sdf_rgb(e, v, scenes, T_map_from_world, num_maps, pose_M, intr, &rp, result);
}

int dslam_debug_track_sdf_rgb_sums(dslam_engine *e, double out[35]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  DSLAM_REQUIRE(e->track_sdf_rgb_sums.have_sums, "no photometric depth-to-SDF tracking evaluation has run on this engine");
  memcpy(out, e->track_sdf_rgb_sums.last_sums, sizeof e->track_sdf_rgb_sums.last_sums);
  return DSLAM_OK;
}

int dslam_debug_track_sdf_rgb_grey(dslam_engine *e, const dslam_view *v, int level, float *out_host) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && out_host, "null argument");
  DSLAM_REQUIRE(v->engine == e, "the view belongs to another engine");
  return download_track_sdf_rgb_grey(e, v, level, out_host);
}

// ---- depth-to-SDF tracking from many start poses at once -----------------------------------------------------------

int dslam_score_camera_poses(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T_map_from_world,
                             int num_maps, const float *poses_M, int num_poses, const float intr[4], int level,
                             float residual_gate, dslam_pose_score *scores_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && scenes && T_map_from_world && poses_M && intr && scores_out, "null argument");
  DSLAM_TRY(check_pose_list_call(e, "dslam_score_camera_poses", v, scenes, T_map_from_world, num_maps, poses_M, num_poses, intr));
  DSLAM_REQUIRE(level >= 0 && level < DSLAM_TRACKER_MAX_LEVELS && (v->w_d >> level) > 0 && (v->h_d >> level) > 0,
                "level is not a level of this view's pyramid");
  DSLAM_REQUIRE(residual_gate >= 0.0f, "residual_gate is negative (or not a number)");
  if (residual_gate == 0.0f) residual_gate = 0.75f;
  e->view_reads++;  // (see dslam_engine::last_fence)
  return launch_score_camera_poses(e, v, scenes, T_map_from_world, num_maps, poses_M, num_poses, intr, level, residual_gate,
                                   scores_out);
}

int dslam_track_camera_sdf_starts(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes,
                                  const float *T_map_from_world, int num_maps, float *poses_M, int num_starts, const float intr[4],
                                  const dslam_track_sdf_params *params, dslam_track_sdf_result *results) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && scenes && T_map_from_world && poses_M && intr && results, "null argument");
  DSLAM_TRY(check_pose_list_call(e, "dslam_track_camera_sdf_starts", v, scenes, T_map_from_world, num_maps, poses_M, num_starts, intr));
  dslam_track_sdf_params tp;
  DSLAM_TRY(default_track_sdf_params(v, params, &tp));
  e->view_reads++;  // (see dslam_engine::last_fence)
  return launch_track_camera_sdf_starts(e, v, scenes, T_map_from_world, num_maps, poses_M, num_starts, intr, &tp, results);
}

int dslam_debug_track_sdf_start_sums(dslam_engine *e, int start, double out[33]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  const std::vector<double> &last = e->track_starts.last_sums;
  DSLAM_REQUIRE(!last.empty(), "no dslam_track_camera_sdf_starts has run on this engine");
  DSLAM_REQUIRE(start >= 0 && (size_t)start < last.size() / kRegSums, "start is not one of the most recent call's starts");
  memcpy(out, &last[(size_t)start * kRegSums], kRegSums * sizeof(double));
  return DSLAM_OK;
}

int dslam_select_start_poses(const dslam_pose_score *scores, int num, int min_valid, int max_keep, int32_t *kept_out,
                             int32_t *num_kept_out) {
  DSLAM_REQUIRE(scores && kept_out && num_kept_out, "null argument");
  DSLAM_REQUIRE(num >= 1 && min_valid >= 0 && max_keep >= 0, "num must be at least 1, min_valid and max_keep not negative");
  select_start_poses(scores, num, min_valid, max_keep, kept_out, num_kept_out);
  return DSLAM_OK;
}

int dslam_camera_pose_lattice(const float pose_M[16], const dslam_pose_lattice *l, float *poses_out, int capacity,
                              int32_t *count_out) {
  DSLAM_REQUIRE(pose_M && l && poses_out && count_out, "null argument");
  *count_out = 0;
  DSLAM_REQUIRE(l->nr >= 0 && l->nt[0] >= 0 && l->nt[1] >= 0 && l->nt[2] >= 0, "a lattice count is negative");
  long long count = 2LL * l->nr + 1;
  for (int a = 0; a < 3; a++) count = std::min(count * (2LL * l->nt[a] + 1), (long long)INT32_MAX);
  *count_out = (int32_t)count;
  DSLAM_REQUIRE(l->step_t >= 0.0f && l->step_r >= 0.0f && std::isfinite(l->step_t) && std::isfinite(l->step_r),
                "a lattice step is negative or not finite");
  if (l->nr > 0) {
    const double len2 = (double)l->axis[0] * l->axis[0] + (double)l->axis[1] * l->axis[1] + (double)l->axis[2] * l->axis[2];
    DSLAM_REQUIRE(std::isfinite(len2) && len2 > 0.0, "the lattice's rotation axis is zero or not finite");
  }
  DSLAM_TRY(check_rigid_transform(pose_M, "the lattice's centre pose"));
  DSLAM_REQUIRE(capacity >= 0 && count <= (long long)capacity, "the lattice has more nodes than poses_out holds");
  camera_pose_lattice(pose_M, *l, poses_out);
  return DSLAM_OK;
}

// ---- decay / sliding window ----------------------------------------------------------------------------------
int dslam_decay(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_weight, int min_age, int force_all) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  int rc = launch_decay(e, s, r, max_weight, min_age, force_all, 0);
  if (rc) return rc;
  return finish_call(e);
}
int dslam_decay_defusion_part(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_weight, int min_age,
                              int force_all) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  int rc = launch_decay(e, s, r, max_weight, min_age, force_all, 1);
  if (rc) return rc;
  return finish_call(e);
}
int dslam_slide_window(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_age) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  if (max_age < 0) max_age = 0;
  while (s->ring_next[0] - s->ring_head[0] > max_age) {
    int rc = launch_slide_pop(e, s, r, 0);
    if (rc) return rc;
  }
  return finish_call(e);
}
int dslam_slide_window_defusion_part(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_age, int max_size) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  (void)max_age;
  if (max_size < 0) max_size = 0;
  while (s->ring_next[1] - s->ring_head[1] > max_size) {
    int rc = launch_slide_pop(e, s, r, 1);
    if (rc) return rc;
  }
  return finish_call(e);
}

// ---- swapping ------------------------------------------------------------------------------------------------
int dslam_swap_in(dslam_engine *e, dslam_scene *s, dslam_render_state *r) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && s->p.use_swapping, "scene was created without swapping");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  int rc = launch_swap_in(e, s, r);
  if (rc) return rc;
  return finish_call(e);
}
int dslam_swap_out(dslam_engine *e, dslam_scene *s, dslam_render_state *r) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && s->p.use_swapping, "scene was created without swapping");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  if (r) r->memo_valid = false;
  int rc = launch_swap_out(e, s, r, false);
  if (rc) return rc;
  return finish_call(e);
}
int dslam_save_to_global_memory(dslam_engine *e, dslam_scene *s) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && s->p.use_swapping, "scene was created without swapping");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  int rc = launch_save_to_global(e, s);
  if (rc) return rc;
  return finish_call(e);
}

// ---- visualisation -------------------------------------------------------------------------------------------
// raycastResult / the lists behind it are about to be rewritten: the GetImage memo (dslam_render_state::memo_*) is stale
static void drop_memo(dslam_render_state *r) { r->memo_valid = false; }

int dslam_find_visible_blocks(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                              const float intr[4]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && M && intr, "null argument");
  drop_memo(r);
  r->types_follow_list = false;
  int rc = launch_find_visible(e, s, r, M, intr);
  if (rc) return rc;
  return finish_call(e);
}
int dslam_count_visible_blocks(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, int min_id,
                               int max_id, int *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && out, "null argument");
  return launch_count_visible(e, s, r, min_id, max_id, out);
}
int dslam_create_expected_depths(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                                 const float intr[4]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && M && intr, "null argument");
  drop_memo(r);
  int rc = launch_expected_depths(e, s, r, M, intr);
  if (rc) return rc;
  return finish_call(e);
}

static int image_out(dslam_engine *e, dslam_render_state *r, int type, uint8_t *out_rgba, float *out_float) {
  const size_t npix = (size_t)r->w * r->h;
  if (out_rgba || out_float) {
    DSLAM_REQUIRE(!(out_rgba && out_float), "pass only one output buffer");
    if (type == DSLAM_IMAGE_DEPTH) {
      DSLAM_REQUIRE(out_float, "DSLAM_IMAGE_DEPTH renders into the float output");
      DSLAM_HIP(hipMemcpyAsync(out_float, r->image_float, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    } else {
      DSLAM_REQUIRE(out_rgba, "this image type renders into the rgba output");
      DSLAM_HIP(hipMemcpyAsync(out_rgba, r->image_rgba, npix * 4, hipMemcpyDeviceToHost, e->stream));
    }
    return sync_check(e);  // host buffers are valid on return
  }
  return finish_call(e);
}

int dslam_render_image(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                       const float intr[4], int type, uint8_t *out_rgba, float *out_float) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && M && intr, "null argument");
  drop_memo(r);
  DSLAM_REQUIRE(type >= 0 && type <= DSLAM_IMAGE_DEPTH, "unknown image type");
  int rc = launch_render(e, s, r, M, intr, type);
  if (rc) return rc;
  return image_out(e, r, type, out_rgba, out_float);
}

// FindVisibleBlocks + CreateExpectedDepths + march for (scene version, pose, intrinsics), unless the render state
// still holds exactly that (see dslam_render_state::memo_*); then the image of the requested type.
static int get_image_on_device(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                               const float *intr, int type, void *direct_out = nullptr) {
  // a map whose voxel blocks live in caller memory can change behind the engine's back: never memoised
  const bool hit = r->memo_valid && s->voxels_own && r->memo_scene == s && r->memo_version == s->version &&
                   r->memo_budget == e->render_tile_budget && memcmp(r->memo_M, M, sizeof(r->memo_M)) == 0 &&
                   memcmp(r->memo_intr, intr, sizeof(r->memo_intr)) == 0;
  int rc;
  if (hit) return launch_render(e, s, r, M, intr, type, true, direct_out);
  drop_memo(r);
  r->types_follow_list = false;  // FindVisibleBlocks replaces this render state's list
  if ((rc = launch_find_visible_and_depths(e, s, r, M, intr))) return rc;
  if ((rc = launch_render(e, s, r, M, intr, type, false, direct_out))) return rc;
  r->memo_valid = true; r->memo_scene = s; r->memo_version = s->version; r->memo_budget = e->render_tile_budget;
  memcpy(r->memo_M, M, sizeof(r->memo_M));
  memcpy(r->memo_intr, intr, sizeof(r->memo_intr));
  return DSLAM_OK;
}

// Where the kernels of a GetImage call store the image: a page-locked output image (dslam_host_alloc) is written by the
// render kernel itself (no copy behind the kernel); null: into the render state's image
static void *direct_image(const dslam_render_state *r, int type, uint8_t *out_rgba, float *out_float) {
  void *out = type == DSLAM_IMAGE_DEPTH ? (void *)out_float : (void *)out_rgba;
  const size_t bytes = (size_t)r->w * r->h * 4;
  return out && !(out_rgba && out_float) && in_pinned_range(out, bytes) ? out : nullptr;
}
// ... and the rest of its way to the caller once they are enqueued
static int deliver_image(dslam_engine *e, dslam_render_state *r, int type, uint8_t *out_rgba, float *out_float,
                         const void *direct) {
  // synchronous engine: the image is there on return (what the reference's callers assume); async engine: the
  // caller pipelines and learns from a fence (dslam_fence_*) when the kernel has stored the last pixel
  if (direct) return finish_call(e);
  return image_out(e, r, type, out_rgba, out_float);
}

namespace {
struct ImageCall {
  dslam_engine *e; const dslam_scene *s; dslam_render_state *r;
  float M[16], intr[4];
  int type;
  uint8_t *out_rgba; float *out_float;
  void *direct;
};
int get_image_body(const ImageCall &c) {
  dslam_engine *e = c.e;
  const unsigned stamp_before = e->stamp_seq;
  DSLAM_TRY(get_image_on_device(e, c.s, c.r, c.M, c.intr, c.type, c.direct));
  DSLAM_TRY(deliver_image(e, c.r, c.type, c.out_rgba, c.out_float, c.direct));
  // Everything this call enqueued from its stamped range pass on -- that pass and the march -- shares no buffer with k_mark
  // (hazard table): the next allocation pass may run its k_mark beside them.  Not if the call waited for its
  // image (a synchronous engine, an output buffer that is not page-locked): the stream is empty then.
  const bool enqueued_only = e->async_mode && (c.direct || (!c.out_rgba && !c.out_float));
  if (e->stamp_seq != stamp_before && enqueued_only) e->stream.grant();
  return DSLAM_OK;
}
}  // namespace

int dslam_get_image(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                    const float intr[4], int type, uint8_t *out_rgba, float *out_float) {
  DSLAM_REQUIRE(e && s && r && M && intr, "null argument");
  DSLAM_REQUIRE(type >= 0 && type <= DSLAM_IMAGE_DEPTH, "unknown image type");
  ImageCall c{e, s, r, {}, {}, type, out_rgba, out_float, direct_image(r, type, out_rgba, out_float)};
  memcpy(c.M, M, sizeof(c.M));
  memcpy(c.intr, intr, sizeof(c.intr));
  // A call that would only enqueue goes behind the calls the engine holds back (a ProcessFrame's tail), with
  // its arguments by value; one that hands the image over on return runs them first.
  if (!e->deferred.empty() && e->async_mode && (c.direct || (!out_rgba && !out_float))) {
    defer_call(e, [c]() { return get_image_body(c); });
    return DSLAM_OK;
  }
  flush_deferred(e);
  return get_image_body(c);
}

int dslam_get_image_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                          dslam_render_state *r, const float M[16], const float intr[4], int type, uint8_t *out_rgba,
                          float *out_float) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && scenes && T_map_from_world && r && M && intr, "null argument");
  DSLAM_REQUIRE(type >= 0 && type <= DSLAM_IMAGE_DEPTH, "unknown image type");
  DSLAM_REQUIRE(r->engine == e, "the render state belongs to another engine");
  float inv[16];
  DSLAM_REQUIRE(invert_matrix(M, inv), "pose matrix is singular");
  DSLAM_TRY(check_map_list(e, "dslam_get_image_multi", scenes, T_map_from_world, num_maps, 1, false, r->n_local));
  drop_memo(r);   // (and nothing is memoised for several maps)
  void *direct = direct_image(r, type, out_rgba, out_float);
  DSLAM_TRY(launch_render_multi(e, scenes, T_map_from_world, num_maps, r, M, intr, type, direct));
  return deliver_image(e, r, type, out_rgba, out_float, direct);
}

int dslam_get_depth_image_int16(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                                const float intr[4], int scale, int16_t *out_host) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && M && intr && out_host && scale > 0, "bad argument");
  int rc;
  if ((rc = get_image_on_device(e, s, r, M, intr, DSLAM_IMAGE_DEPTH))) return rc;
  // the RGBA image buffer of the render state is idle in this mode: it takes the int16 image (2 of its 4 bytes per pixel)
  const int n = r->w * r->h;
  short *tmp = reinterpret_cast<short *>(r->image_rgba.get());
  if ((rc = launch_depth_to_int16(e, r->image_float, tmp, n, scale))) return rc;
  DSLAM_HIP(hipMemcpyAsync(out_host, tmp, (size_t)n * 2, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

int dslam_create_icp_maps(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                          const float intr[4], float *out_points, float *out_normals) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && r && M && intr, "null argument");
  drop_memo(r);
  int rc;
  if ((rc = launch_expected_depths(e, s, r, M, intr))) return rc;
  if ((rc = launch_icp_maps(e, s, r, M, intr))) return rc;
  const size_t bytes = (size_t)r->w * r->h * sizeof(float4);
  if (out_points) DSLAM_HIP(hipMemcpyAsync(out_points, r->icp_points, bytes, hipMemcpyDeviceToHost, e->stream));
  if (out_normals) DSLAM_HIP(hipMemcpyAsync(out_normals, r->icp_normals, bytes, hipMemcpyDeviceToHost, e->stream));
  if (out_points || out_normals) return sync_check(e);
  return finish_call(e);
}

int dslam_download_raycast_image(dslam_engine *e, const dslam_render_state *r, uint8_t *out_rgba) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r && out_rgba, "null argument");
  DSLAM_REQUIRE(r->raycast_image, "dslam_create_icp_maps has not run on this render state");
  DSLAM_HIP(hipMemcpyAsync(out_rgba, r->raycast_image, (size_t)r->w * r->h * 4, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

int dslam_download_icp_maps(dslam_engine *e, const dslam_render_state *r, float *out_points, float *out_normals) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r, "null argument");
  DSLAM_REQUIRE(r->icp_points && r->icp_normals, "dslam_create_icp_maps has not run on this render state");
  const size_t bytes = (size_t)r->w * r->h * sizeof(float4);
  if (out_points) DSLAM_HIP(hipMemcpyAsync(out_points, r->icp_points, bytes, hipMemcpyDeviceToHost, e->stream));
  if (out_normals) DSLAM_HIP(hipMemcpyAsync(out_normals, r->icp_normals, bytes, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

// ---- meshing export --------------------------------------------------------------------------------------------
int dslam_mesh_scene(dslam_engine *e, const dslam_scene *s, int max_triangles, int with_colour, int *out_num_triangles) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out_num_triangles, "null argument");
  if (max_triangles <= 0) max_triangles = s->p.num_local_blocks * 32;  // ITMMesh::noMaxTriangles
  int rc = launch_mesh_scene(e, s, max_triangles, with_colour, out_num_triangles);
  if (rc) return rc;
  return finish_call(e);
}

int dslam_mesh_scene_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                           int max_triangles, int with_colour, int *out_num_triangles, int32_t *out_map_triangles) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && scenes && T_map_from_world && out_num_triangles, "null argument");
  DSLAM_TRY(check_map_list(e, "dslam_mesh_scene_multi", scenes, T_map_from_world, num_maps, 1, false));
  long long blocks = 0;
  for (int i = 0; i < num_maps; i++) blocks += scenes[i]->p.num_local_blocks;
  if (max_triangles <= 0) max_triangles = (int)std::min<long long>(blocks * 32, INT_MAX);  // the maps' noMaxTriangles together
  DSLAM_TRY(launch_mesh_scene_multi(e, scenes, T_map_from_world, num_maps, max_triangles, with_colour, out_num_triangles,
                                    out_map_triangles));
  return finish_call(e);
}

// ---- map registration ------------------------------------------------------------------------------------------
int dslam_register_maps(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst, float X_dst_from_src[16],
                        const dslam_register_params *params, dslam_register_result *result) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && src && dst && X_dst_from_src && result, "null argument");
  DSLAM_REQUIRE(src->engine == e && dst->engine == e, "a scene belongs to another engine");
  DSLAM_REQUIRE(src->p.voxel_size == dst->p.voxel_size && src->p.mu == dst->p.mu,
                "the two maps of a registration need the same voxel_size and mu");
  for (int i = 0; i < 16; i++) DSLAM_REQUIRE(std::isfinite(X_dst_from_src[i]), "the start transform is not finite");
  float inv[16];
  DSLAM_REQUIRE(invert_matrix(X_dst_from_src, inv), "the start transform is singular");
  dslam_register_params rp;
  DSLAM_TRY(default_register_params(params, &rp));
  return launch_register_maps(e, src, dst, X_dst_from_src, &rp, result);
}

int dslam_debug_register_sums(dslam_engine *e, double out[33]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  return copy_sums(e->reg_sums, "no registration evaluation has run on this engine", out);
}

int dslam_register_graph(dslam_engine *e, const dslam_scene *const *scenes, float *T_map_from_world, int num_maps,
                         const int32_t *pairs, int num_pairs, int anchor, const dslam_register_params *params,
                         dslam_register_graph_result *result, dslam_register_pair_result *pair_results) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && scenes && T_map_from_world && pairs && result, "null argument");
  DSLAM_TRY(check_map_list(e, "dslam_register_graph", scenes, T_map_from_world, num_maps, 2, true));
  DSLAM_REQUIRE(num_pairs >= 1 && num_pairs <= DSLAM_MAX_REGISTER_PAIRS, "num_pairs must be 1 .. DSLAM_MAX_REGISTER_PAIRS");
  DSLAM_REQUIRE(anchor >= 0 && anchor < num_maps, "the anchor is not a map of the list");
  for (int p = 0; p < num_pairs; p++) {
    const int s = pairs[2 * p], d = pairs[2 * p + 1];
    DSLAM_REQUIRE(s >= 0 && s < num_maps && d >= 0 && d < num_maps, "a pair names a map that is not in the list");
    DSLAM_REQUIRE(s != d, "a pair names one map twice");
    for (int q = 0; q < p; q++) DSLAM_REQUIRE(pairs[2 * q] != s || pairs[2 * q + 1] != d, "an ordered pair is given twice");
  }
  dslam_register_params rp;
  DSLAM_TRY(default_register_params(params, &rp));
  return launch_register_graph(e, scenes, T_map_from_world, num_maps, pairs, num_pairs, anchor, &rp, result, pair_results);
}

int dslam_debug_register_graph_sums(dslam_engine *e, int pair, double out[33]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  DSLAM_REQUIRE(!e->reg_graph_sums.empty(), "no joint registration has run on this engine");
  DSLAM_REQUIRE(pair >= 0 && (size_t)pair < e->reg_graph_sums.size() / 33, "the pair index is out of range");
  memcpy(out, e->reg_graph_sums.data() + (size_t)pair * 33, 33 * sizeof(double));
  return DSLAM_OK;
}

// ---- overlap survey and pair selection ------------------------------------------------------------------------------
int dslam_survey_overlaps(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                          int32_t *live_blocks_out, int32_t *shared_blocks_out, int32_t *shared_octants_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && scenes && T_map_from_world && live_blocks_out && shared_octants_out, "null argument");
  DSLAM_TRY(check_map_list(e, "dslam_survey_overlaps", scenes, T_map_from_world, num_maps, 2, true));
  return launch_survey_overlaps(e, scenes, T_map_from_world, num_maps, live_blocks_out, shared_blocks_out, shared_octants_out);
}

int dslam_select_register_pairs(const int32_t *live_blocks, const int32_t *shared_octants, int num_maps,
                                const dslam_pair_select_params *params, int32_t *pairs_out, int32_t *component_out,
                                dslam_pair_select_result *result) {
  DSLAM_REQUIRE(live_blocks && shared_octants && pairs_out && component_out && result, "null argument");
  DSLAM_REQUIRE(num_maps >= 2 && num_maps <= DSLAM_MAX_RENDER_MAPS, "num_maps must be 2 .. DSLAM_MAX_RENDER_MAPS");
  dslam_pair_select_params sp = {0, 0, 0, 0};
  if (params) sp = *params;
  DSLAM_REQUIRE(sp.min_shared_octants >= 0 && sp.one_direction >= 0 && sp.max_pairs >= 0, "a selection parameter is negative");
  if (sp.min_shared_octants == 0) sp.min_shared_octants = 64;
  if (sp.max_pairs == 0) sp.max_pairs = DSLAM_MAX_REGISTER_PAIRS;
  DSLAM_REQUIRE(sp.max_pairs <= DSLAM_MAX_REGISTER_PAIRS, "max_pairs is above DSLAM_MAX_REGISTER_PAIRS");
  DSLAM_REQUIRE(sp.max_pairs >= num_maps - 1, "max_pairs is below num_maps - 1: a spanning set of pairs would not fit");
  select_register_pairs(live_blocks, shared_octants, num_maps, sp, pairs_out, component_out, result);
  return DSLAM_OK;
}

// ---- view survey and map selection ----------------------------------------------------------------------------------
namespace {

// what dslam_view_frustum_planes rejects (and dslam_survey_views with it)
int check_survey_view(const dslam_survey_view &v, float voxel_size) {
  DSLAM_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0f, "voxel_size must be positive and finite");
  DSLAM_TRY(check_rigid_transform(v.M, "a view's pose"));
  for (int k = 0; k < 4; k++) DSLAM_REQUIRE(std::isfinite(v.intrinsics[k]), "a view's intrinsics are not finite");
  DSLAM_REQUIRE(v.intrinsics[0] > 0.0f && v.intrinsics[1] > 0.0f, "a view's focal lengths must be positive");
  DSLAM_REQUIRE(v.width >= 1 && v.height >= 1, "a view's image size must be at least 1 x 1");
  DSLAM_REQUIRE(std::isfinite(v.near_m) && std::isfinite(v.far_m) && v.near_m >= 0.0f && v.far_m >= 0.0f,
                "a view's near and far distances must be finite and not negative");
  DSLAM_REQUIRE(v.far_m == 0.0f || v.far_m > v.near_m, "a view's far plane must lie beyond its near plane (or be 0: none)");
  return DSLAM_OK;
}

}  // namespace

int dslam_view_frustum_planes(const dslam_survey_view *view, float voxel_size, float out[28]) {
  DSLAM_REQUIRE(view && out, "null argument");
  DSLAM_TRY(check_survey_view(*view, voxel_size));
  view_frustum_planes(*view, voxel_size, out);
  return DSLAM_OK;
}

int dslam_survey_views(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                       const dslam_survey_view *views, int num_views, const dslam_view_survey_params *params,
                       int32_t *live_blocks_out, int32_t *reach_blocks_out, int32_t *nearest_out, int32_t *farthest_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && scenes && T_map_from_world && views && live_blocks_out && reach_blocks_out, "null argument");
  DSLAM_TRY(check_map_list(e, "dslam_survey_views", scenes, T_map_from_world, num_maps, 1, true, 0, DSLAM_MAX_SURVEY_MAPS));
  DSLAM_REQUIRE(num_views >= 1 && num_views <= DSLAM_MAX_SURVEY_VIEWS, "num_views must be 1 .. DSLAM_MAX_SURVEY_VIEWS");
  const float margin = params ? params->margin_voxels : 0.0f;
  DSLAM_REQUIRE(std::isfinite(margin) && margin >= 0.0f, "the margin is negative (or not a number)");
  float planes[DSLAM_MAX_SURVEY_VIEWS * 28];
  for (int v = 0; v < num_views; v++) {
    DSLAM_TRY(check_survey_view(views[v], scenes[0]->p.voxel_size));
    view_frustum_planes(views[v], scenes[0]->p.voxel_size, planes + 28 * v);
  }
  const float rho = (float)(6.92820323027550917 + (double)(margin == 0.0f ? 2.0f : margin));
  return launch_survey_views(e, scenes, T_map_from_world, num_maps, planes, num_views, rho, live_blocks_out, reach_blocks_out,
                             nearest_out, farthest_out);
}

int dslam_debug_survey_views_launches(dslam_engine *e, long long *count_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && count_out, "null argument");
  *count_out = e->view_survey_launches;
  return DSLAM_OK;
}

int dslam_select_view_maps(const int32_t *reach_blocks, const int32_t *nearest, int num_views, int num_maps,
                           const dslam_view_select_params *params, int32_t *maps_out, dslam_view_select_result *result) {
  DSLAM_REQUIRE(reach_blocks && nearest && maps_out && result, "null argument");
  DSLAM_REQUIRE(num_views >= 1 && num_views <= DSLAM_MAX_SURVEY_VIEWS, "num_views must be 1 .. DSLAM_MAX_SURVEY_VIEWS");
  DSLAM_REQUIRE(num_maps >= 1 && num_maps <= DSLAM_MAX_SURVEY_MAPS, "num_maps must be 1 .. DSLAM_MAX_SURVEY_MAPS");
  dslam_view_select_params sp = {0, 0, -1, 0};
  if (params) sp = *params;
  DSLAM_REQUIRE(sp.min_blocks >= 0 && sp.max_maps >= 0 && sp.always_keep >= -1 && sp.pad >= 0, "a selection parameter is negative");
  DSLAM_REQUIRE(sp.always_keep < num_maps, "always_keep is not one of the maps");
  if (sp.min_blocks == 0) sp.min_blocks = 1;
  if (sp.max_maps == 0) sp.max_maps = DSLAM_MAX_RENDER_MAPS;
  DSLAM_REQUIRE(sp.max_maps <= DSLAM_MAX_RENDER_MAPS, "max_maps is above DSLAM_MAX_RENDER_MAPS");
  select_view_maps(reach_blocks, nearest, num_views, num_maps, sp, maps_out, result);
  return DSLAM_OK;
}

// ---- the maps at any point or along any ray ---------------------------------------------------------------------------
namespace {

// what the four query calls check alike; max_range: NULL for points, else in: the caller's, out: the default in place of 0
int check_query_call(dslam_engine *e, const char *call, const dslam_scene *const *scenes, const float *T, int num_maps,
                     const void *in, int n, int what, const void *out, float *max_range) {
  DSLAM_REQUIRE(e && scenes && T, "null argument");
  DSLAM_TRY(check_map_list(e, call, scenes, T, num_maps, 1, true));
  DSLAM_REQUIRE(n >= 0 && n <= DSLAM_QUERY_MAX_ELEMENTS, std::string(call) + ": n must be 0 .. DSLAM_QUERY_MAX_ELEMENTS");
  DSLAM_REQUIRE((what & ~(DSLAM_QUERY_SDF | DSLAM_QUERY_GRADIENT | DSLAM_QUERY_COLOUR)) == 0, std::string(call) + ": unknown bits in `what`");
  DSLAM_REQUIRE(max_range || (what & DSLAM_QUERY_SDF), std::string(call) + ": `what` must include DSLAM_QUERY_SDF");
  if (max_range) {
    const float limit = (float)DSLAM_QUERY_MAX_RAY_VOXELS * scenes[0]->p.voxel_size;
    DSLAM_REQUIRE(std::isfinite(*max_range) && *max_range >= 0.0f && *max_range <= limit,
                  std::string(call) + ": max_range must be 0 (the limit) .. DSLAM_QUERY_MAX_RAY_VOXELS x voxel_size");
    if (*max_range == 0.0f) *max_range = limit;
  }
  DSLAM_REQUIRE(n == 0 || (in && out), std::string(call) + ": null array");
  return DSLAM_OK;
}

}  // namespace

int dslam_query_points(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                       const float *points_host, int n, int what, dslam_point_sample *out_host) {
  flush_deferred(e);
  DSLAM_TRY(check_query_call(e, "dslam_query_points", scenes, T_map_from_world, num_maps, points_host, n, what, out_host, nullptr));
  if (n == 0) return DSLAM_OK;
  DSLAM_TRY(launch_query(e, scenes, T_map_from_world, num_maps, false, points_host, n, 0.0f, what, out_host, true));
  return sync_check(e);
}

int dslam_query_points_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                              const void *points_dev, int n, int what, void *out_dev) {
  flush_deferred(e);
  DSLAM_TRY(check_query_call(e, "dslam_query_points_device", scenes, T_map_from_world, num_maps, points_dev, n, what, out_dev, nullptr));
  DSLAM_REQUIRE(((uintptr_t)points_dev & 3) == 0 && ((uintptr_t)out_dev & 15) == 0, "points must be 4-byte, results 16-byte aligned");
  if (n == 0) return DSLAM_OK;
  DSLAM_TRY(launch_query(e, scenes, T_map_from_world, num_maps, false, points_dev, n, 0.0f, what, out_dev, false));
  return finish_call(e);
}

int dslam_cast_rays(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                    const float *rays_host, int n, float max_range, int what, dslam_ray_hit *out_host) {
  flush_deferred(e);
  DSLAM_TRY(check_query_call(e, "dslam_cast_rays", scenes, T_map_from_world, num_maps, rays_host, n, what, out_host, &max_range));
  if (n == 0) return DSLAM_OK;
  DSLAM_TRY(launch_query(e, scenes, T_map_from_world, num_maps, true, rays_host, n, max_range, what, out_host, true));
  return sync_check(e);
}

int dslam_cast_rays_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                           const void *rays_dev, int n, float max_range, int what, void *out_dev) {
  flush_deferred(e);
  DSLAM_TRY(check_query_call(e, "dslam_cast_rays_device", scenes, T_map_from_world, num_maps, rays_dev, n, what, out_dev, &max_range));
  DSLAM_REQUIRE(((uintptr_t)rays_dev & 15) == 0 && ((uintptr_t)out_dev & 15) == 0, "rays and results must be 16-byte aligned");
  if (n == 0) return DSLAM_OK;
  DSLAM_TRY(launch_query(e, scenes, T_map_from_world, num_maps, true, rays_dev, n, max_range, what, out_dev, false));
  return finish_call(e);
}

// ---- occupancy and exact distance grids ---------------------------------------------------------------------------------
int dslam_grid_from_box(const float *lo_m, const float *hi_m, float voxel_size, int cell, dslam_grid *out) {
  DSLAM_REQUIRE(lo_m && hi_m && out, "null argument");
  DSLAM_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0f, "dslam_grid_from_box: voxel_size must be finite and positive");
  DSLAM_REQUIRE(cell >= 1 && cell <= DSLAM_GRID_MAX_CELL, "dslam_grid_from_box: cell must be 1 .. DSLAM_GRID_MAX_CELL");
  dslam_grid g;
  memset(&g, 0, sizeof g);
  g.cell = cell;
  for (int a = 0; a < 3; a++) {
    DSLAM_REQUIRE(std::isfinite(lo_m[a]) && std::isfinite(hi_m[a]) && hi_m[a] >= lo_m[a], "dslam_grid_from_box: the box must be finite with hi >= lo");
    const double o = floor((double)lo_m[a] / (double)voxel_size);
    const double d = std::max(1.0, ceil(((double)hi_m[a] / (double)voxel_size - o) / (double)cell));
    // (checked as doubles, before any conversion)
    DSLAM_REQUIRE(o >= -1048576.0 && d <= (double)DSLAM_GRID_MAX_DIM && o + (double)cell * d <= 1048576.0,
                  "dslam_grid_from_box: the box exceeds the grid's limits");
    g.origin[a] = (int32_t)o;
    g.dims[a] = (int32_t)d;
  }
  DSLAM_REQUIRE(grid_ok(g), "dslam_grid_from_box: the box exceeds the grid's limits");
  *out = g;
  return DSLAM_OK;
}

namespace {

// what the six grid calls check alike, and the call they make.  scenes NULL: the transform alone; transform false: the marking alone
int distance_field_call(dslam_engine *e, const char *call, const dslam_scene *const *scenes, const float *T, int num_maps, bool marking,
                        const dslam_grid *grid, int min_weight, float occupied_below, const void *states_in, bool transform, int seeds,
                        int max_cells, int format, float voxel_size, void *states_out, void *dist_out, bool host) {
  flush_deferred(e);
  auto msg = [call](const char *what) { return std::string(call) + ": " + what; };
  DSLAM_REQUIRE(e && grid, "null argument");
  DistanceFieldCall c;
  memset(&c, 0, sizeof c);
  if (marking) {
    DSLAM_REQUIRE(scenes && T, "null argument");
    DSLAM_TRY(check_map_list(e, call, scenes, T, num_maps, 1, true));
    DSLAM_REQUIRE(min_weight >= 0 && min_weight <= 255, msg("min_weight must be 0 .. 255"));
    const float mu = scenes[0]->p.mu;
    DSLAM_REQUIRE(std::isfinite(occupied_below) && fabsf(occupied_below) < mu, msg("occupied_below must be finite with |occupied_below| < mu"));
    c.scenes = scenes; c.T = T; c.num_maps = num_maps;
    c.min_weight = min_weight == 0 ? 1 : min_weight;
    c.thr = (int)floor((double)occupied_below / (double)mu * 32767.0);
    voxel_size = scenes[0]->p.voxel_size;
  }
  DSLAM_REQUIRE(grid_ok(*grid), msg("the grid is outside the limits (cell, dims, cells, the +-2^20 voxel range) or its pad is not 0"));
  if (transform) {
    DSLAM_REQUIRE(seeds >= 1 && seeds <= 3, msg("seeds must be DSLAM_SEED_OCCUPIED, DSLAM_SEED_UNKNOWN or both"));
    DSLAM_REQUIRE(max_cells >= 0 && max_cells <= DSLAM_DIST_MAX_CELLS, msg("max_cells must be 0 .. DSLAM_DIST_MAX_CELLS"));
    DSLAM_REQUIRE(format == DSLAM_DIST_SQUARED_CELLS || format == DSLAM_DIST_METRES, msg("unknown format"));
    DSLAM_REQUIRE(format != DSLAM_DIST_METRES || (std::isfinite(voxel_size) && voxel_size > 0.0f), msg("voxel_size must be finite and positive"));
  }
  if (!marking) DSLAM_REQUIRE(states_in && dist_out, msg("null array"));
  else if (!transform) DSLAM_REQUIRE(states_out, msg("null array"));
  else DSLAM_REQUIRE(states_out || dist_out, msg("states_out and dist_out are both NULL"));
  if (!host)
    DSLAM_REQUIRE(((uintptr_t)states_in & 15) == 0 && ((uintptr_t)states_out & 15) == 0 && ((uintptr_t)dist_out & 15) == 0,
                  msg("device arrays must be 16-byte aligned"));
  c.grid = *grid;
  c.states_in = states_in;
  c.transform = transform;
  c.seeds = seeds; c.max_cells = max_cells; c.format = format;
  c.voxel_size = voxel_size;
  c.states_out = states_out; c.dist_out = dist_out;
  c.host = host;
  DSLAM_TRY(launch_distance_field(e, c));
  return host ? sync_check(e) : finish_call(e);
}

}  // namespace

int dslam_mark_occupancy(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                         const dslam_grid *grid, int min_weight, float occupied_below, uint8_t *states_out_host) {
  return distance_field_call(e, "dslam_mark_occupancy", scenes, T_map_from_world, num_maps, true, grid, min_weight, occupied_below,
                             nullptr, false, 0, 0, 0, 0.0f, states_out_host, nullptr, true);
}

int dslam_mark_occupancy_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                                const dslam_grid *grid, int min_weight, float occupied_below, void *states_out_dev) {
  return distance_field_call(e, "dslam_mark_occupancy_device", scenes, T_map_from_world, num_maps, true, grid, min_weight,
                             occupied_below, nullptr, false, 0, 0, 0, 0.0f, states_out_dev, nullptr, false);
}

int dslam_distance_transform(dslam_engine *e, const dslam_grid *grid, const uint8_t *states_host, int seeds, int max_cells, int format,
                             float voxel_size, void *dist_out_host) {
  return distance_field_call(e, "dslam_distance_transform", nullptr, nullptr, 0, false, grid, 0, 0.0f, states_host, true, seeds,
                             max_cells, format, voxel_size, nullptr, dist_out_host, true);
}

int dslam_distance_transform_device(dslam_engine *e, const dslam_grid *grid, const void *states_dev, int seeds, int max_cells,
                                    int format, float voxel_size, void *dist_out_dev) {
  return distance_field_call(e, "dslam_distance_transform_device", nullptr, nullptr, 0, false, grid, 0, 0.0f, states_dev, true, seeds,
                             max_cells, format, voxel_size, nullptr, dist_out_dev, false);
}

int dslam_distance_field(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                         const dslam_grid *grid, int min_weight, float occupied_below, int seeds, int max_cells, int format,
                         uint8_t *states_out_host, void *dist_out_host) {
  return distance_field_call(e, "dslam_distance_field", scenes, T_map_from_world, num_maps, true, grid, min_weight, occupied_below,
                             nullptr, true, seeds, max_cells, format, 0.0f, states_out_host, dist_out_host, true);
}

int dslam_distance_field_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                                const dslam_grid *grid, int min_weight, float occupied_below, int seeds, int max_cells, int format,
                                void *states_out_dev, void *dist_out_dev) {
  return distance_field_call(e, "dslam_distance_field_device", scenes, T_map_from_world, num_maps, true, grid, min_weight,
                             occupied_below, nullptr, true, seeds, max_cells, format, 0.0f, states_out_dev, dist_out_dev, false);
}

int dslam_debug_distance_field_phases(dslam_engine *e, int enable, float out_ms[4]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null argument");
  return distance_field_phases(e, enable, out_ms);
}

// ---- semi-global stereo matching ------------------------------------------------------------------------------------
namespace {

int check_stereo_calib(const dslam_stereo_calib *c) {
  DSLAM_REQUIRE(std::isfinite(c->focal_length_px) && c->focal_length_px > 0.0f && std::isfinite(c->baseline_m) && c->baseline_m > 0.0f &&
                    std::isfinite(c->scale) && c->scale > 0.0f,
                "the calibration's focal_length_px, baseline_m and scale must be finite and positive");
  DSLAM_REQUIRE(std::isfinite(c->min_depth_m) && std::isfinite(c->max_depth_m) && c->min_depth_m >= 0.0f && c->max_depth_m >= c->min_depth_m,
                "the calibration needs 0 <= min_depth_m <= max_depth_m");
  DSLAM_REQUIRE(c->max_depth_m * 1000.0f < 32767.0f, "max_depth_m * 1000 must stay below 32767: the depth image is int16 millimetres");
  return DSLAM_OK;
}

// what the stereo calls check alike, and the call they make
int stereo_call(dslam_engine *e, dslam_stereo *st, const StereoCall &c) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && st, "null argument");
  DSLAM_REQUIRE(st->engine == e, "the stereo matcher belongs to another engine");
  const bool match = c.left || c.right, convert = c.calib || c.depth_out;
  if (c.S_host) DSLAM_REQUIRE(c.disp_out, "null argument");
  else if (match) DSLAM_REQUIRE(c.left && c.right && (convert || c.disp_out), "null argument");
  else DSLAM_REQUIRE(c.disp_in, "null argument");
  if (convert || !(match || c.S_host)) {
    DSLAM_REQUIRE(c.calib && c.depth_out, "null argument");
    DSLAM_TRY(check_stereo_calib(c.calib));
  }
  if (!c.host)
    DSLAM_REQUIRE(((uintptr_t)c.left & 15) == 0 && ((uintptr_t)c.right & 15) == 0 && ((uintptr_t)c.disp_in & 15) == 0 &&
                      ((uintptr_t)c.disp_out & 15) == 0 && ((uintptr_t)c.depth_out & 15) == 0,
                  "device arrays must be 16-byte aligned");
  DSLAM_TRY(launch_stereo(e, st, c));
  return c.host ? sync_check(e) : finish_call(e);
}

}  // namespace

int dslam_stereo_create(dslam_engine *e, int width, int height, const dslam_stereo_params *params, dslam_stereo **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  DSLAM_REQUIRE(width >= 1 && width <= DSLAM_STEREO_MAX_SIZE && height >= 1 && height <= DSLAM_STEREO_MAX_SIZE,
                "width and height must be 1 .. DSLAM_STEREO_MAX_SIZE");
  std::unique_ptr<dslam_stereo> st(new dslam_stereo());
  DSLAM_TRY(stereo_resolve_params(params, st.get()));
  st->engine = e; st->w = width; st->h = height;
  DSLAM_TRY(stereo_allocate(e, st.get()));
  engine_adopt(e);   // (only a complete matcher is a handle, as a fern index)
  *out = st.release();
  return DSLAM_OK;
}

int dslam_stereo_destroy(dslam_stereo *st) {
  if (!st) return DSLAM_OK;
  (void)hipSetDevice(st->engine->device);
  flush_deferred(st->engine);   // (on its own device: held calls launch kernels)
  (void)hipStreamSynchronize(st->engine->stream);
  dslam_engine *e = st->engine;
  delete st;
  engine_release(e);
  return DSLAM_OK;
}

int dslam_stereo_get_params(const dslam_stereo *st, dslam_stereo_params *params_out) {
  DSLAM_REQUIRE(st && params_out, "null argument");
  *params_out = st->p;
  return DSLAM_OK;
}

int dslam_stereo_match(dslam_engine *e, dslam_stereo *st, const uint8_t *left_host, const uint8_t *right_host, uint16_t *disp_out_host) {
  DSLAM_REQUIRE(left_host && right_host && disp_out_host, "null argument");
  return stereo_call(e, st, StereoCall{left_host, right_host, nullptr, nullptr, nullptr, disp_out_host, nullptr, true});
}

int dslam_stereo_match_device(dslam_engine *e, dslam_stereo *st, const void *left_dev, const void *right_dev, void *disp_out_dev) {
  DSLAM_REQUIRE(left_dev && right_dev && disp_out_dev, "null argument");
  return stereo_call(e, st, StereoCall{left_dev, right_dev, nullptr, nullptr, nullptr, disp_out_dev, nullptr, false});
}

int dslam_disparity_to_depth(dslam_engine *e, dslam_stereo *st, const uint16_t *disp_host, const dslam_stereo_calib *calib,
                             int16_t *depth_mm_out_host) {
  DSLAM_REQUIRE(disp_host && calib && depth_mm_out_host, "null argument");
  return stereo_call(e, st, StereoCall{nullptr, nullptr, nullptr, disp_host, calib, nullptr, depth_mm_out_host, true});
}

int dslam_disparity_to_depth_device(dslam_engine *e, dslam_stereo *st, const void *disp_dev, const dslam_stereo_calib *calib,
                                    void *depth_mm_out_dev) {
  DSLAM_REQUIRE(disp_dev && calib && depth_mm_out_dev, "null argument");
  return stereo_call(e, st, StereoCall{nullptr, nullptr, nullptr, disp_dev, calib, nullptr, depth_mm_out_dev, false});
}

int dslam_stereo_depth(dslam_engine *e, dslam_stereo *st, const uint8_t *left_host, const uint8_t *right_host,
                       const dslam_stereo_calib *calib, int16_t *depth_mm_out_host, uint16_t *disp_out_host) {
  DSLAM_REQUIRE(left_host && right_host && calib && depth_mm_out_host, "null argument");
  return stereo_call(e, st, StereoCall{left_host, right_host, nullptr, nullptr, calib, disp_out_host, depth_mm_out_host, true});
}

int dslam_stereo_depth_device(dslam_engine *e, dslam_stereo *st, const void *left_dev, const void *right_dev,
                              const dslam_stereo_calib *calib, void *depth_mm_out_dev, void *disp_out_dev) {
  DSLAM_REQUIRE(left_dev && right_dev && calib && depth_mm_out_dev, "null argument");
  return stereo_call(e, st, StereoCall{left_dev, right_dev, nullptr, nullptr, calib, disp_out_dev, depth_mm_out_dev, false});
}

int dslam_debug_stereo_download(dslam_engine *e, dslam_stereo *st, int what, void *out_host) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && st && out_host, "null argument");
  DSLAM_REQUIRE(st->engine == e, "the stereo matcher belongs to another engine");
  DSLAM_REQUIRE(what == DSLAM_STEREO_CENSUS_LEFT || what == DSLAM_STEREO_CENSUS_RIGHT || what == DSLAM_STEREO_S, "unknown `what`");
  DSLAM_REQUIRE(st->matched, "the stereo matcher has not matched a pair yet");
  DSLAM_TRY(stereo_download(e, st, what, out_host));
  return sync_check(e);
}

int dslam_debug_stereo_select(dslam_engine *e, dslam_stereo *st, const uint16_t *S_host, uint16_t *disp_out_host) {
  DSLAM_REQUIRE(S_host && disp_out_host, "null argument");
  return stereo_call(e, st, StereoCall{nullptr, nullptr, S_host, nullptr, nullptr, disp_out_host, nullptr, true});
}

int dslam_debug_stereo_phases(dslam_engine *e, dslam_stereo *st, int enable, float out_ms[5]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && st, "null argument");
  DSLAM_REQUIRE(st->engine == e, "the stereo matcher belongs to another engine");
  return stereo_phases(e, st, enable, out_ms);
}

// ---- sparse stereo scene flow ---------------------------------------------------------------------------------------
namespace {

// what every dslam_sflow_* call on a handle checks first
int check_sflow(dslam_engine *e, dslam_sflow *sf) {
  DSLAM_REQUIRE(e && sf, "null argument");
  DSLAM_REQUIRE(sf->engine == e, "the scene-flow matcher belongs to another engine");
  return DSLAM_OK;
}

int sflow_push_call(dslam_engine *e, dslam_sflow *sf, const void *left, const void *right, int replace, bool host) {
  flush_deferred(e);
  DSLAM_TRY(check_sflow(e, sf));
  DSLAM_REQUIRE(left, "null argument");
  if (!host) DSLAM_REQUIRE(((uintptr_t)left & 15) == 0 && ((uintptr_t)right & 15) == 0, "device arrays must be 16-byte aligned");
  DSLAM_TRY(launch_sflow_push(e, sf, SflowPush{left, right, replace != 0, host}));
  return host ? sync_check(e) : finish_call(e);
}

int sflow_match_call(dslam_engine *e, dslam_sflow *sf, int method, int set, void *out, int capacity, void *count, bool host) {
  flush_deferred(e);
  DSLAM_TRY(check_sflow(e, sf));
  DSLAM_REQUIRE(count && (out || capacity == 0), "null argument");
  DSLAM_REQUIRE(method >= 0 && method <= 2 && (set == 0 || set == 1), "method must be 0, 1 or 2 and set 0 or 1");
  DSLAM_REQUIRE(capacity >= 0, "capacity must not be negative");
  if (!host) DSLAM_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)count & 15) == 0, "device arrays must be 16-byte aligned");
  DSLAM_TRY(launch_sflow_match(e, sf, SflowMatch{method, set, out, count, capacity, host}));
  return host ? sync_check(e) : finish_call(e);
}

}  // namespace

int dslam_sflow_create(dslam_engine *e, int width, int height, const dslam_sflow_params *params, dslam_sflow **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  std::unique_ptr<dslam_sflow> sf(new dslam_sflow());
  DSLAM_TRY(sflow_resolve_params(params, width, height, sf.get()));
  sf->engine = e;
  DSLAM_TRY(sflow_allocate(e, sf.get()));
  engine_adopt(e);   // (only a complete matcher is a handle)
  *out = sf.release();
  return DSLAM_OK;
}

int dslam_sflow_destroy(dslam_sflow *sf) {
  if (!sf) return DSLAM_OK;
  (void)hipSetDevice(sf->engine->device);
  flush_deferred(sf->engine);
  (void)hipStreamSynchronize(sf->engine->stream);
  dslam_engine *e = sf->engine;
  delete sf;
  engine_release(e);
  return DSLAM_OK;
}

int dslam_sflow_get_params(const dslam_sflow *sf, dslam_sflow_params *params_out) {
  DSLAM_REQUIRE(sf && params_out, "null argument");
  *params_out = sf->p;
  return DSLAM_OK;
}

int dslam_sflow_push(dslam_engine *e, dslam_sflow *sf, const uint8_t *left_host, const uint8_t *right_host, int replace) {
  return sflow_push_call(e, sf, left_host, right_host, replace, true);
}

int dslam_sflow_push_device(dslam_engine *e, dslam_sflow *sf, const void *left_dev, const void *right_dev, int replace) {
  return sflow_push_call(e, sf, left_dev, right_dev, replace, false);
}

int dslam_sflow_match(dslam_engine *e, dslam_sflow *sf, int method, int set, int32_t *out_host, int capacity, int32_t *count_out) {
  return sflow_match_call(e, sf, method, set, out_host, capacity, count_out, true);
}

int dslam_sflow_match_device(dslam_engine *e, dslam_sflow *sf, int method, int set, void *out_dev, int capacity, void *count_dev) {
  return sflow_match_call(e, sf, method, set, out_dev, capacity, count_dev, false);
}

int dslam_sflow_features(dslam_engine *e, dslam_sflow *sf, int image, int set, void *out_host, int capacity, int32_t *count_out) {
  flush_deferred(e);
  DSLAM_TRY(check_sflow(e, sf));
  DSLAM_REQUIRE(count_out && (out_host || capacity == 0), "null argument");
  DSLAM_REQUIRE(image >= DSLAM_SFLOW_IMAGE_1C && image <= DSLAM_SFLOW_IMAGE_2P && (set == 0 || set == 1), "unknown image or set");
  DSLAM_REQUIRE(capacity >= 0, "capacity must not be negative");
  DSLAM_TRY(sflow_features(e, sf, image, set, out_host, capacity, count_out));
  return sync_check(e);
}

int dslam_debug_sflow_download(dslam_engine *e, dslam_sflow *sf, int side, int filter, void *out_host) {
  flush_deferred(e);
  DSLAM_TRY(check_sflow(e, sf));
  DSLAM_REQUIRE(out_host, "null argument");
  DSLAM_REQUIRE((side == 0 || side == 1) && filter >= DSLAM_SFLOW_FILTER_DU && filter <= DSLAM_SFLOW_FILTER_F2, "unknown side or filter");
  DSLAM_REQUIRE(sf->pushes > 0, "the scene-flow matcher has not been given a frame yet");
  DSLAM_TRY(sflow_download(e, sf, side, filter, out_host));
  return sync_check(e);
}

int dslam_debug_sflow_phases(dslam_engine *e, dslam_sflow *sf, int enable, float out_ms[6]) {
  flush_deferred(e);
  DSLAM_TRY(check_sflow(e, sf));
  return sflow_phases(e, sf, enable, out_ms);
}

// ---- fern keyframe index --------------------------------------------------------------------------------------------
namespace {

// what every dslam_fern_* call that takes a window rejects
int check_fern_window(int first_id, int last_id, int k) {
  DSLAM_REQUIRE(k >= 1 && k <= DSLAM_FERN_MAX_MATCHES, "k must be 1 .. DSLAM_FERN_MAX_MATCHES");
  DSLAM_REQUIRE(first_id >= 0 && last_id >= 0 && first_id <= last_id, "the id window must satisfy 0 <= first_id <= last_id");
  return DSLAM_OK;
}

int check_fern_view(const dslam_engine *e, const dslam_fern_index *idx, const dslam_view *v) {
  DSLAM_REQUIRE(idx->engine == e, "the fern index belongs to another engine");
  DSLAM_REQUIRE(v->engine == e, "the view belongs to another engine");
  DSLAM_REQUIRE(v->updated, "the view was never updated");
  DSLAM_REQUIRE(v->w_d == idx->w && v->h_d == idx->h, "the view's depth size is not the fern index's");
  DSLAM_REQUIRE(idx->p.channels == 1 || (v->w_rgb == idx->w && v->h_rgb == idx->h),
                "a fern index with a grey channel needs the view's RGB size to equal its depth size");
  return DSLAM_OK;
}

}  // namespace

int dslam_fern_index_create(dslam_engine *e, int width_d, int height_d, const dslam_fern_params *params, int capacity,
                            dslam_fern_index **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out, "null argument");
  DSLAM_REQUIRE(width_d > 0 && height_d > 0 && (long long)width_d * height_d < (1ll << 30), "bad image size");
  DSLAM_REQUIRE(capacity >= 1 && capacity <= (1 << 22), "capacity must be 1 .. 4194304");
  dslam_fern_params p = {0, 0, 0, 0, 0, 0u};
  if (params) p = *params;
  DSLAM_REQUIRE(p.num_ferns >= 0 && p.cell >= 0 && p.channels >= 0 && p.depth_min_mm >= 0 && p.depth_max_mm >= 0,
                "a fern parameter is negative");
  if (p.num_ferns == 0) p.num_ferns = 512;
  if (p.cell == 0) p.cell = 8;
  if (p.channels == 0) p.channels = 1;
  if (p.depth_min_mm == 0) p.depth_min_mm = 300;
  if (p.depth_max_mm == 0) p.depth_max_mm = 10000;
  DSLAM_REQUIRE(p.num_ferns % 8 == 0 && p.num_ferns <= 512, "num_ferns must be a multiple of 8 in 8 .. 512");
  DSLAM_REQUIRE(p.cell <= 32, "cell must be 1 .. 32");
  DSLAM_REQUIRE(p.channels <= 2, "channels must be 1 or 2");
  DSLAM_REQUIRE(p.depth_min_mm <= p.depth_max_mm && p.depth_max_mm <= 32767, "need depth_min_mm <= depth_max_mm <= 32767");
  DSLAM_REQUIRE(width_d / p.cell >= 1 && height_d / p.cell >= 1, "the cell is larger than the image");
  std::unique_ptr<dslam_fern_index> idx(new dslam_fern_index());
  idx->engine = e; idx->w = width_d; idx->h = height_d; idx->p = p; idx->capacity = capacity;
  idx->tw = width_d / p.cell; idx->th = height_d / p.cell;
  fern_build_table(p, idx->tw, idx->th, idx->table);
  DSLAM_TRY(fern_index_allocate(e, idx.get()));
  engine_adopt(e);   // (only a complete index is a handle, as a frame store)
  *out = idx.release();
  return DSLAM_OK;
}

int dslam_fern_index_destroy(dslam_fern_index *idx) {
  if (!idx) return DSLAM_OK;
  (void)hipSetDevice(idx->engine->device);
  flush_deferred(idx->engine);   // (on its own device: held calls launch kernels)
  (void)hipStreamSynchronize(idx->engine->stream);
  dslam_engine *e = idx->engine;
  delete idx;
  engine_release(e);
  return DSLAM_OK;
}

int dslam_fern_index_count(const dslam_fern_index *idx, int32_t *count_out) {
  DSLAM_REQUIRE(idx && count_out, "null argument");
  *count_out = idx->count;
  return DSLAM_OK;
}

int dslam_fern_index_table(const dslam_fern_index *idx, dslam_fern_params *params_out, int32_t *table_out) {
  DSLAM_REQUIRE(idx, "null argument");
  if (params_out) *params_out = idx->p;
  if (table_out) memcpy(table_out, idx->table.data(), idx->table.size() * sizeof(int32_t));
  return DSLAM_OK;
}

int dslam_fern_index_reset(dslam_engine *e, dslam_fern_index *idx) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && idx, "null argument");
  DSLAM_REQUIRE(idx->engine == e, "the fern index belongs to another engine");
  idx->count = 0;
  return DSLAM_OK;
}

int dslam_fern_encode(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, uint32_t code_out[DSLAM_FERN_CODE_DWORDS]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && idx && v && code_out, "null argument");
  DSLAM_TRY(check_fern_view(e, idx, v));
  e->view_reads++;  // (see dslam_engine::last_fence)
  return fern_encode_view(e, idx, v, code_out);
}

int dslam_fern_query(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, int first_id, int last_id, int k,
                     dslam_fern_match *matches_out, int32_t *num_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && idx && v && matches_out && num_out, "null argument");
  DSLAM_TRY(check_fern_view(e, idx, v));
  DSLAM_TRY(check_fern_window(first_id, last_id, k));
  e->view_reads++;  // (see dslam_engine::last_fence)
  return fern_query_view(e, idx, v, -1, first_id, last_id, k, matches_out, num_out, nullptr);
}

int dslam_fern_process(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, int harvest_min_dissimilarity, int first_id,
                       int last_id, int k, dslam_fern_match *matches_out, int32_t *num_out, int32_t *added_id_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && idx && v && matches_out && num_out && added_id_out, "null argument");
  DSLAM_TRY(check_fern_view(e, idx, v));
  DSLAM_TRY(check_fern_window(first_id, last_id, k));
  DSLAM_REQUIRE(harvest_min_dissimilarity >= 0, "the harvest threshold is negative");
  e->view_reads++;  // (see dslam_engine::last_fence)
  return fern_query_view(e, idx, v, harvest_min_dissimilarity, first_id, last_id, k, matches_out, num_out, added_id_out);
}

int dslam_fern_add_from_store(dslam_engine *e, dslam_fern_index *idx, const dslam_frame_store *fs, int first_slot, int num_slots,
                              int32_t *first_id_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && idx && fs && first_id_out, "null argument");
  DSLAM_REQUIRE(idx->engine == e, "the fern index belongs to another engine");
  DSLAM_REQUIRE(fs->engine == e, "frame store belongs to a different engine");
  DSLAM_REQUIRE(fs->w_d == idx->w && fs->h_d == idx->h, "the frame store's depth size is not the fern index's");
  DSLAM_REQUIRE(idx->p.channels == 1 || (fs->w_rgb == idx->w && fs->h_rgb == idx->h),
                "a fern index with a grey channel needs the store's RGB size to equal its depth size");
  DSLAM_REQUIRE(num_slots >= 1 && first_slot >= 0 && first_slot <= fs->capacity - num_slots, "the slots are not all in the frame store");
  DSLAM_REQUIRE(num_slots <= idx->capacity - idx->count, "the fern index has no room for that many codes");
  const int first_id = idx->count;
  DSLAM_TRY(fern_add_from_store(e, idx, fs, first_slot, num_slots));
  *first_id_out = first_id;
  return DSLAM_OK;
}

int dslam_fern_query_stored(dslam_engine *e, dslam_fern_index *idx, const int32_t *query_ids, int num_queries, int first_id,
                            int last_id, int k, dslam_fern_match *matches_out, int32_t *num_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && idx && query_ids && matches_out && num_out, "null argument");
  DSLAM_REQUIRE(idx->engine == e, "the fern index belongs to another engine");
  DSLAM_REQUIRE(num_queries >= 1 && num_queries <= DSLAM_FERN_MAX_QUERIES, "num_queries must be 1 .. DSLAM_FERN_MAX_QUERIES");
  DSLAM_TRY(check_fern_window(first_id, last_id, k));
  for (int q = 0; q < num_queries; q++)
    DSLAM_REQUIRE(query_ids[q] >= 0 && query_ids[q] < idx->count, "a query id is not a stored code");
  return fern_query_stored(e, idx, query_ids, num_queries, first_id, last_id, k, matches_out, num_out);
}

// ---- map merge --------------------------------------------------------------------------------------------------
namespace {

// what dslam_merge_maps, dslam_unmerge_maps and dslam_remerge_maps reject alike
int check_merge_scenes(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst) {
  DSLAM_REQUIRE(src->engine == e && dst->engine == e, "a scene belongs to another engine");
  DSLAM_REQUIRE(src != dst, "a map cannot be merged into itself");
  DSLAM_REQUIRE(memcmp(&src->p.voxel_size, &dst->p.voxel_size, sizeof(float)) == 0 && memcmp(&src->p.mu, &dst->p.mu, sizeof(float)) == 0,
                "the two maps of a merge need the same voxel_size and mu");
  DSLAM_REQUIRE(!src->p.use_swapping && !dst->p.use_swapping, "maps that use swapping cannot be merged");
  DSLAM_REQUIRE(src->num_shards == 1 && dst->num_shards == 1 && src->shard_count < 0 && dst->shard_count < 0,
                "sharded maps cannot be merged");
  return DSLAM_OK;
}

int check_merge_params(const dslam_scene *src, const dslam_merge_params *params, dslam_merge_params *mp) {
  DSLAM_REQUIRE((double)src->p.num_local_blocks * 512.0 < 4294967295.0, "the source has more blocks than the 32-bit order key can name");
  *mp = {0, 1};
  if (params) *mp = *params;
  DSLAM_REQUIRE(mp->max_passes >= 0, "max_passes is negative");
  if (mp->max_passes == 0) mp->max_passes = 16;
  return DSLAM_OK;
}

// the map changes: GetImage memos of this scene are stale
void map_changed(dslam_scene *dst) {
  dst->version = next_map_version();
  if (dst->front) dst->front->valid = false;
}

}  // namespace

int dslam_merge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float X_dst_from_src[16],
                     const dslam_merge_params *params, dslam_merge_result *result) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && src && dst && X_dst_from_src && result, "null argument");
  DSLAM_TRY(check_merge_scenes(e, src, dst));
  DSLAM_TRY(check_rigid_transform(X_dst_from_src, "the transform"));
  dslam_merge_params mp;
  DSLAM_TRY(check_merge_params(src, params, &mp));
  map_changed(dst);
  return launch_merge_maps(e, src, dst, X_dst_from_src, &mp, result);
}

int dslam_unmerge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float X_dst_from_src[16],
                       const dslam_unmerge_params *params, dslam_unmerge_result *result) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && src && dst && X_dst_from_src && result, "null argument");
  DSLAM_TRY(check_merge_scenes(e, src, dst));
  DSLAM_TRY(check_rigid_transform(X_dst_from_src, "the transform"));
  map_changed(dst);
  return launch_unmerge_maps(e, src, dst, X_dst_from_src, params ? params->with_colour : 1, result, false);
}

int dslam_remerge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float X_old[16],
                       const float X_new[16], const dslam_merge_params *params, dslam_unmerge_result *unmerged,
                       dslam_merge_result *merged) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && src && dst && X_old && X_new && unmerged && merged, "null argument");
  DSLAM_TRY(check_merge_scenes(e, src, dst));
  DSLAM_TRY(check_rigid_transform(X_old, "the old transform"));
  DSLAM_TRY(check_rigid_transform(X_new, "the new transform"));
  dslam_merge_params mp;
  DSLAM_TRY(check_merge_params(src, params, &mp));
  memset(unmerged, 0, sizeof *unmerged);
  memset(merged, 0, sizeof *merged);
  if (memcmp(X_old, X_new, 16 * sizeof(float)) == 0) return DSLAM_OK;
  map_changed(dst);
  // the unmerge is only enqueued: the merge behind it reuses the source's live list, and its first read-back is the wait
  DSLAM_TRY(launch_unmerge_maps(e, src, dst, X_old, mp.with_colour, unmerged, true));
  const int rc = launch_merge_maps(e, src, dst, X_new, &mp, merged, true);
  if (rc == DSLAM_OK) collect_unmerge_result(e, unmerged);
  return rc;
}

// ---- packed maps: the host half (pack_host.h) ------------------------------------------------------------------
int dslam_pack_layout(int32_t blocks, int32_t free_excess, int64_t *blocks_offset_out, int64_t *total_bytes_out) {
  DSLAM_REQUIRE(blocks_offset_out && total_bytes_out, "null argument");
  DSLAM_REQUIRE(blocks >= 0 && free_excess >= 0, "a packed map has no negative count");
  pack_layout(blocks, free_excess, blocks_offset_out, total_bytes_out);
  return DSLAM_OK;
}

int dslam_pack_header_read(const void *first_64_bytes, dslam_pack_info *out) {
  DSLAM_REQUIRE(first_64_bytes && out, "null argument");
  dslam_pack_info h;
  memcpy(&h, first_64_bytes, sizeof h);
  DSLAM_REQUIRE(pack_header_valid(h), "not the header of a packed map (magic, version, counts or layout)");
  *out = h;
  return DSLAM_OK;
}

// ---- packed maps: the device half (pack.hip) ---------------------------------------------------------------------
// the scene kinds neither call takes: their maps are more than resident entries plus a free excess list, or in motion
static int check_pack_scene(dslam_engine *e, const dslam_scene *s) {
  DSLAM_REQUIRE(s->engine == e, "the scene belongs to another engine");
  DSLAM_REQUIRE(!s->p.use_swapping, "a scene that uses swapping cannot be packed or unpacked into");
  DSLAM_REQUIRE(s->num_shards == 1 && s->shard_count < 0, "a sharded scene cannot be packed or unpacked into");
  DSLAM_REQUIRE(!s->alloc_born, "the scene's re-integration batch is being planned");
  return DSLAM_OK;
}

int dslam_device_alloc(dslam_engine *e, size_t bytes, void **out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out && bytes > 0, "bad argument");
  *out = nullptr;
  DSLAM_HIP(hipSetDevice(e->device));
  DSLAM_HIP(hipMalloc(out, bytes));
  return DSLAM_OK;
}
int dslam_device_free(dslam_engine *e, void *p) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null engine");
  if (!p) return DSLAM_OK;
  DSLAM_HIP(hipSetDevice(e->device));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  DSLAM_HIP(hipFree(p));
  return DSLAM_OK;
}

int dslam_pack_scene(dslam_engine *e, const dslam_scene *s, void *buf, int64_t capacity, dslam_pack_info *info_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && info_out, "null argument");
  DSLAM_TRY(check_pack_scene(e, s));
  DSLAM_HIP(hipSetDevice(e->device));
  dslam_pack_info info;
  memset(&info, 0, sizeof info);
  const int rc = launch_pack_scene(e, s, buf, capacity, &info);
  if (rc == DSLAM_OK || info.total_bytes > 0) *info_out = info;   // (total_bytes > 0: the counts were read)
  return rc;
}

int dslam_unpack_scene(dslam_engine *e, dslam_scene *s, const void *buf, int64_t bytes, dslam_pack_info *info_out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && buf, "null argument");
  DSLAM_TRY(check_pack_scene(e, s));
  DSLAM_REQUIRE(bytes >= kPackHeaderBytes, "shorter than the header of a packed map");
  DSLAM_HIP(hipSetDevice(e->device));
  void *buf_dev = nullptr;
  DSLAM_TRY(pack_buffer_address(e, buf, kPackHeaderBytes, &buf_dev));
  // the header: read by the host, judged as dslam_pack_header_read judges it, compared with the scene
  dslam_pack_info h;
  DSLAM_HIP(hipMemcpyAsync(e->pinned, buf_dev, sizeof h, hipMemcpyDefault, e->stream));
  DSLAM_TRY(sync_check(e));
  DSLAM_TRY(dslam_pack_header_read(e->pinned, &h));
  DSLAM_REQUIRE(h.num_buckets == s->p.num_buckets && h.num_excess == s->p.num_excess, "the packed map's table geometry is not the scene's");
  DSLAM_REQUIRE(memcmp(&h.voxel_size_bits, &s->p.voxel_size, 4) == 0 && memcmp(&h.mu_bits, &s->p.mu, 4) == 0,
                "the packed map's voxel_size or mu is not the scene's");
  DSLAM_REQUIRE(h.blocks <= s->p.num_local_blocks, "the packed map holds more blocks than the scene's pool");
  DSLAM_REQUIRE(bytes >= h.total_bytes, "the buffer is shorter than the packed map");
  DSLAM_TRY(pack_buffer_address(e, buf, h.total_bytes, &buf_dev));
  DSLAM_TRY(launch_unpack_validate(e, s, buf_dev, &h));
  // ---- the first write: from here on a failure leaves the scene reset ----
  map_changed(s);
  reset_host_cursors(s);
  int rc = launch_unpack_write(e, s, buf_dev, &h);
  if (rc == DSLAM_OK) rc = sync_check(e);
  if (rc != DSLAM_OK) {   // whatever failed (a HIP call, or a device report the wait heard): never a half-written scene
    const std::string why = g_last_error;
    if (launch_scene_reset(e, s) == DSLAM_OK) (void)hipStreamSynchronize(e->stream);
    g_last_error = why;
    return rc;
  }
  if (info_out) *info_out = h;
  return DSLAM_OK;
}

int dslam_debug_merge_phases(dslam_engine *e, int enable, double out_ms[5]) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null argument");
  if (out_ms) memcpy(out_ms, e->merge_phase_ms, sizeof e->merge_phase_ms);
  e->merge_phases_on = enable != 0;
  return DSLAM_OK;
}

int dslam_mesh_download(dslam_engine *e, float *out_positions, float *out_colours, int capacity_triangles) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && out_positions && capacity_triangles >= 0, "bad argument");
  DSLAM_REQUIRE(capacity_triangles >= e->mesh_triangles, "dslam_mesh_download: buffer smaller than the mesh");
  DSLAM_REQUIRE(!out_colours || e->mesh_has_colour, "dslam_mesh_download: the mesh was made without colours");
  const size_t bytes = (size_t)e->mesh_triangles * 9 * sizeof(float);
  if (bytes) {
    DSLAM_HIP(hipMemcpyAsync(out_positions, e->mesh_positions, bytes, hipMemcpyDeviceToHost, e->stream));
    if (out_colours) DSLAM_HIP(hipMemcpyAsync(out_colours, e->mesh_colours, bytes, hipMemcpyDeviceToHost, e->stream));
  }
  return sync_check(e);
}

// ---- read-back -----------------------------------------------------------------------------------------------
int dslam_get_stats(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, dslam_stats *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out, "null argument");
  char *host = reinterpret_cast<char *>(e->pinned.get());
  SceneCounters *sc = reinterpret_cast<SceneCounters *>(host);
  RenderCounters *rc = reinterpret_cast<RenderCounters *>(host + 128);
  DSLAM_HIP(hipMemcpyAsync(sc, s->counters, sizeof(SceneCounters), hipMemcpyDeviceToHost, e->stream));
  if (r) DSLAM_HIP(hipMemcpyAsync(rc, r->counters, sizeof(RenderCounters), hipMemcpyDeviceToHost, e->stream));
  const int rc_engine = sync_check(e);   // (what any scene of the engine reported since the last synchronising call)
  memset(out, 0, sizeof(*out));
  out->num_allocated_blocks = s->p.num_local_blocks;
  out->last_free_block_id = sc->last_free;
  out->last_free_excess_id = sc->last_free_ex;
  out->no_visible_entries = r ? rc->no_visible : 0;
  out->decayed_block_count = sc->decayed_blocks;
  out->slid_block_count = sc->slid_blocks;
  out->frame_counter = s->frame_counter;
  out->fusion_fifo_len = s->ring_next[0] - s->ring_head[0];
  out->defusion_fifo_len = s->ring_next[1] - s->ring_head[1];
  out->alloc_failures = sc->alloc_failures;
  out->last_swapped_in = sc->swapped_in;
  out->last_swapped_out = sc->swapped_out;
  if (sc->error_flags & 2) {
    set_last_error("a tile count of an ordered compaction never arrived (device made no progress?): the map state is undefined");
    return DSLAM_ERR_HIP;
  }
  if (sc->error_flags & 1) {
    set_last_error("allocation ray needed more steps than the order key encodes (non-rigid pose or mu/voxel_size changed?)");
    return DSLAM_ERR_UNSUPPORTED;
  }
  return rc_engine;
}

static int d2h(dslam_engine *e, void *dst, const void *src, size_t bytes) {
  DSLAM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}
static int h2d(dslam_engine *e, void *dst, const void *src, size_t bytes) {
  DSLAM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

int dslam_download_hash_table(dslam_engine *e, const dslam_scene *s, dslam_hash_entry *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out, "null argument");
  return d2h(e, out, s->hash, (size_t)s->n_entries * sizeof(HashEntry));
}
int dslam_download_voxel_blocks(dslam_engine *e, const dslam_scene *s, int first, int n, dslam_voxel *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out && first >= 0 && n >= 0 && first + n <= s->p.num_local_blocks, "bad block range");
  return d2h(e, out, s->voxels + (size_t)first * kBlock3, (size_t)n * kBlock3 * sizeof(uint2));
}
int dslam_download_allocation_list(dslam_engine *e, const dslam_scene *s, int32_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out, "null argument");
  return d2h(e, out, s->alloc_list, (size_t)s->p.num_local_blocks * sizeof(int));
}
int dslam_download_excess_list(dslam_engine *e, const dslam_scene *s, int32_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out, "null argument");
  return d2h(e, out, s->excess_list, (size_t)s->p.num_excess * sizeof(int));
}
int dslam_download_visible_ids(dslam_engine *e, const dslam_render_state *r, int32_t *out, int capacity, int *count) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r && out, "null argument");
  RenderCounters *rc = reinterpret_cast<RenderCounters *>(reinterpret_cast<char *>(e->pinned.get()) + 128);
  int st = d2h(e, rc, r->counters, sizeof(RenderCounters));
  if (st) return st;
  int n = rc->no_visible < capacity ? rc->no_visible : capacity;
  if (count) *count = rc->no_visible;
  if (n > 0) return d2h(e, out, r->visible_ids, (size_t)n * sizeof(int));
  return DSLAM_OK;
}
int dslam_download_visible_types(dslam_engine *e, const dslam_render_state *r, uint8_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r && out, "null argument");
  int rc = d2h(e, out, r->visible_type, r->n_entries);
  for (int i = 0; i < r->n_entries; i++) out[i] &= 0x7f;  // the device bytes carry the pass' generation bit
  return rc;
}
int dslam_download_range_image(dslam_engine *e, const dslam_render_state *r, float *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r && out, "null argument");
  return d2h(e, out, r->range, (size_t)r->w * r->h * sizeof(float2));
}
int dslam_download_raycast_result(dslam_engine *e, const dslam_render_state *r, float *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r && out, "null argument");
  return d2h(e, out, r->raycast, (size_t)r->w * r->h * sizeof(float4));
}
int dslam_download_view_depth(dslam_engine *e, const dslam_view *v, float *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && v && out, "null argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  int rc = ensure_view_depth(e, v);
  if (rc) return rc;
  return d2h(e, out, v->depth, (size_t)v->w_d * v->h_d * sizeof(float));
}
int dslam_download_swap_states(dslam_engine *e, const dslam_scene *s, uint8_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out && s->swap_state, "scene has no swap state");
  return d2h(e, out, s->swap_state, s->n_entries);
}
int dslam_download_last_seen(dslam_engine *e, const dslam_scene *s, int32_t *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && out, "null argument");
  return d2h(e, out, s->last_seen, (size_t)s->p.num_local_blocks * sizeof(int));
}
int dslam_download_stored_block(dslam_engine *e, const dslam_scene *s, int entry, dslam_voxel *out) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && s->slot_dev && entry >= 0 && entry < s->n_entries, "bad entry / no global cache");
  int slot = -1;  // (d2h waits for the stream: the swap kernels write the host slabs directly)
  int rc = d2h(e, &slot, s->slot_dev + entry, sizeof(int));
  if (rc) return rc;
  if (out) {
    if (slot >= 0) memcpy(out, s->slabs[slot >> kSlabShift] + (size_t)(slot & (kSlabBlocks - 1)) * (kBlock3 / 2), kBlock3 * sizeof(dslam_voxel));
    else memset(out, 0, kBlock3 * sizeof(dslam_voxel));
  }
  return slot >= 0 ? 1 : 0;
}
int dslam_download_alloc_scratch(dslam_engine *e, const dslam_scene *s, uint8_t *types, int16_t *coords) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && e->scratch_entries >= s->n_entries, "no allocation pass has run");
  int rc = 0;
  if (types) rc = d2h(e, types, e->alloc_type, s->n_entries);
  if (!rc && coords) rc = d2h(e, coords, e->block_coords, (size_t)s->n_entries * sizeof(short4));
  return rc;
}

int dslam_upload_scene_state(dslam_engine *e, dslam_scene *s, const dslam_hash_entry *hash, const int32_t *alloc_list,
                             int last_free, const int32_t *excess_list, int last_free_ex) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s, "null argument");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  int rc = 0;
  if (hash) {
    rc = h2d(e, s->hash, hash, (size_t)s->n_entries * sizeof(HashEntry));
    if (!rc) rc = launch_build_alloc_bits(e, s);
    if (!rc) rc = finish_call(e);
  }
  SceneCounters *sc = reinterpret_cast<SceneCounters *>(e->pinned.get());
  if (!rc && (alloc_list || excess_list)) {
    rc = d2h(e, sc, s->counters, sizeof(SceneCounters));
    if (!rc && alloc_list) {
      rc = h2d(e, s->alloc_list, alloc_list, (size_t)s->p.num_local_blocks * sizeof(int));
      sc->last_free = last_free;
    }
    if (!rc && excess_list) {
      rc = h2d(e, s->excess_list, excess_list, (size_t)s->p.num_excess * sizeof(int));
      sc->last_free_ex = last_free_ex;
    }
    if (!rc) rc = h2d(e, s->counters, sc, sizeof(SceneCounters));
  }
  return rc;
}
int dslam_upload_voxel_blocks(dslam_engine *e, dslam_scene *s, int first, int n, const dslam_voxel *host) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && host && first >= 0 && n >= 0 && first + n <= s->p.num_local_blocks, "bad block range");
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  return h2d(e, s->voxels + (size_t)first * kBlock3, host, (size_t)n * kBlock3 * sizeof(uint2));
}
int dslam_upload_visible_ids(dslam_engine *e, dslam_render_state *r, const int32_t *ids, int count) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && r && ids && count >= 0 && count <= r->n_local, "bad visible list");
  drop_memo(r);
  r->types_follow_list = false;
  int rc = h2d(e, r->visible_ids, ids, (size_t)count * sizeof(int));
  if (rc) return rc;
  RenderCounters *rcn = reinterpret_cast<RenderCounters *>(reinterpret_cast<char *>(e->pinned.get()) + 128);
  rc = d2h(e, rcn, r->counters, sizeof(RenderCounters));
  if (rc) return rc;
  rcn->no_visible = count;
  __atomic_store_n(r->vis_hint.get(), count, __ATOMIC_RELAXED);
  return h2d(e, r->counters, rcn, sizeof(RenderCounters));
}

// (a caller that asks for a buffer means to use it: held-back calls that write it are handed to the GPU first)
void *dslam_scene_voxel_blocks_dev(dslam_scene *s) { if (s) flush_deferred(s->engine); return s ? s->voxels : nullptr; }
void *dslam_scene_hash_table_dev(dslam_scene *s) { if (s) flush_deferred(s->engine); return s ? s->hash : nullptr; }
int dslam_scene_table_changed(dslam_engine *e, dslam_scene *s) {
  flush_deferred(e);
  DSLAM_REQUIRE(e && s && s->engine == e, "null argument");
  s->version = next_map_version();  // the map changed: GetImage memos of this scene are stale
  int rc = launch_build_alloc_bits(e, s);
  if (rc) return rc;
  return finish_call(e);
}
void *dslam_render_state_image_dev(dslam_render_state *r, int want_float) {
  if (!r) return nullptr;
  flush_deferred(r->engine);   // (a held-back GetImage may exchange this render state's buffers with a front-end record's)
  return want_float ? (void *)r->image_float : (void *)r->image_rgba;
}

// ---- instrumentation -----------------------------------------------------------------------------------------
int dslam_time_integrate(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_render_state *r,
                         const float M_d[16], const float intr[4], int iterations, float *out_ms, int *out_blocks) {
  flush_deferred(e);
  int rc = check_frame_args(e, s, v, r, M_d, intr);
  if (rc) return rc;
  s->version = next_map_version();  // the map may change: GetImage memos of this scene are stale
  DSLAM_REQUIRE(iterations > 0 && out_ms, "bad argument");
  e->view_reads++;  // (see dslam_engine::last_fence)
  Event a, b;
  DSLAM_TRY(a.create(hipEventDefault));
  DSLAM_TRY(b.create(hipEventDefault));
  const bool saved = e->timer_enabled;
  e->timer_enabled = false;
  rc = launch_integrate(e, s, v, r, M_d, intr, nullptr, nullptr, false);  // warm-up
  DSLAM_HIP(hipEventRecord(a, e->stream));
  for (int i = 0; i < iterations && !rc; i++) rc = launch_integrate(e, s, v, r, M_d, intr, nullptr, nullptr, false);
  DSLAM_HIP(hipEventRecord(b, e->stream));
  DSLAM_HIP(hipEventSynchronize(b));
  e->timer_enabled = saved;
  float ms = 0;
  DSLAM_HIP(hipEventElapsedTime(&ms, a, b));
  *out_ms = ms / iterations;
  if (out_blocks) {
    RenderCounters *rcn = reinterpret_cast<RenderCounters *>(reinterpret_cast<char *>(e->pinned.get()) + 128);
    int st = d2h(e, rcn, r->counters, sizeof(RenderCounters));
    if (st) return st;
    *out_blocks = rcn->no_visible;
  }
  return rc;
}

int dslam_kernel_timer_enable(dslam_engine *e, int enable) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null engine");
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  if (enable && e->ev_pool.empty()) {
    const size_t n = 2 * 8192;  // up to 8192 timed launches between reads
    DSLAM_REQUIRE(e->pinned_bytes >= 256 + 8192 * sizeof(int), "pinned mirror too small");
    DeviceBuffer<int> counts;
    std::vector<Event> pool(n);
    DSLAM_TRY(counts.alloc(8192));
    for (size_t i = 0; i < n; i++) DSLAM_TRY(pool[i].create(hipEventDefault));
    e->timer_counts_dev = std::move(counts);
    e->ev_pool = std::move(pool);
  }
  e->timer_enabled = enable != 0;
  e->ev_used = 0;
  e->timer_ms = 0; e->timer_launches = 0; e->timer_blocks = 0;
  return DSLAM_OK;
}

int dslam_kernel_timer_read(dslam_engine *e, double *out_ms, int64_t *out_launches, int64_t *out_blocks) {
  flush_deferred(e);
  DSLAM_REQUIRE(e, "null engine");
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  int *counts = reinterpret_cast<int *>(e->pinned.get()) + 64;
  if (e->ev_used > 0) {
    DSLAM_HIP(hipMemcpyAsync(counts, e->timer_counts_dev, (e->ev_used / 2) * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
  }
  for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
    float ms = 0;
    DSLAM_HIP(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
    e->timer_ms += ms;
    e->timer_launches++;
    e->timer_blocks += counts[i / 2];
  }
  e->ev_used = 0;
  if (out_ms) *out_ms = e->timer_ms;
  if (out_launches) *out_launches = e->timer_launches;
  if (out_blocks) *out_blocks = e->timer_blocks;
  return DSLAM_OK;
}

}  // extern "C"
