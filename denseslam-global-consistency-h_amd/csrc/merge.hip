// merge.hip -- fuse one local map into another on the device (dslam_merge_maps; ITMMainEngine::MergeLocalMap in the mirror).
//
// Reference: none.  The reference keeps its local maps apart for good; the law below is this project's own definition
// (include/dslam_fusion.h states it in full).  The source is only read.
//
//   X~ : source voxels -> destination voxels, Y~ its inverse; the first three rows, row-major, float32 (host: double).
//   1. push    every source voxel with w_depth > 0, in the order (rank r of its entry among the resident entries, linear
//              index l), key r * 512 + l + 1, names the destination block B = floor(X~ p + 0.5) >> 3 it falls into;
//   2. passes  k_merge_mark (merge_walk of merge_device.h, shared with unmerge.hip) looks every B up in the destination:
//              a hit sets the entry's bit in `touched`, a miss does atomicMax(keys[slot], key) on the slot
//              AllocateSceneFromDepth would use and sets the slot's request bits.
//              Three ordered selections (dslam_bits.h) then serve the requests in hash-index order: over q1 and over q2
//              to give every request its rank among those of its own type, over q1 | q2 to give it its rank among all --
//              with both the closed form of DESIGN.md section 3 says whether the pools still hold a block for it and
//              which.  The winner's B is recomputed from its key.  One small read-back per pass tells the host whether
//              another pass is needed (different blocks that asked for the same slot).
//   3. pull    k_merge_blocks (merge_pull of merge_device.h, shared with unmerge.hip): one workgroup per touched
//              destination block at a time (fixed grid, grid-stride over the ordered list of touched entries), lane t
//              the voxels 2t and 2t + 1 -- the block moves as 16-byte accesses.
//              Each voxel reads the source trilinearly at Y~ p' (merge_resample of merge_device.h, shared with unmerge.hip:
//              to_map / gather_cell / lerp8 of multimap_device.h), packs the result as a voxel and merges it with
//              combine_voxel (combine_device.h), as a swap-in does.
// No kernel here waits for another workgroup; the pass loop is bounded by max_passes on the host.
#include <chrono>
#include <cmath>
#include <cstring>

#include "combine_device.h"
#include "dslam_bits.h"
#include "merge_device.h"
#include "mesh_device.h"
#include "multimap_device.h"

#pragma clang fp contract(off)

namespace dslam {

__global__ void k_merge_begin(SceneCounters *cnt, MergeCounters *mc) {
  cnt->base_free = cnt->last_free;
  cnt->base_free_ex = cnt->last_free_ex;
  mc->requests = 0; mc->served1 = 0; mc->served2 = 0;
  mc->candidates = 0; mc->out_of_range = 0;
}

__global__ void k_merge_end(SceneCounters *cnt, const MergeCounters *mc) {
  const int succ = mc->served1 + mc->served2;   // every success takes exactly one voxel-block slot
  cnt->last_free = cnt->base_free - succ;
  cnt->base_free = cnt->base_free - succ;
  cnt->last_free_ex = cnt->base_free_ex - mc->served2;
}

struct MergeMarkParams : MergeWalkParams {
  unsigned *keys, *q1, *q2, *req, *touched;
  MergeCounters *mc;
};

// a hit sets the entry's bit in `touched`; a miss asks for the slot the probe stopped at, with the voxel's key
__global__ __launch_bounds__(kMergeThreads) void k_merge_mark(MergeMarkParams p) {
  merge_walk<2>(p, p.mc, [&](const MergeProbe &pr, int r, int l, int, int *) {
    if (pr.found) {
      merge_touch(p.touched, pr.h);
    } else {
      const unsigned bit = 1u << (pr.h & 31);
      atomicMax(&p.keys[pr.h], (unsigned)r * (unsigned)kBlock3 + (unsigned)l + 1u);
      atomicOr(&(pr.in_use ? p.q2 : p.q1)[pr.h >> 5], bit);
      atomicOr(&p.req[pr.h >> 5], bit);
    }
  });
}

// rank of a request among the requests of its own type
struct SelMergeRank {
  DSLAM_SEL_NO_LOAD
  int *ranks;
  __device__ bool test(int, const NoPayload &) const { return true; }
  __device__ void prologue() const {}
  __device__ int emit(int t, int rank, bool, const NoPayload &) const { ranks[t] = rank; return 0; }
  __device__ void finish(int) const {}
};

// the serve step: rank = requests of either type in front of this one, in hash-index order
struct SelMergeServe {
  DSLAM_SEL_NO_LOAD
  HashEntry *hash;           // the destination
  int num_buckets;
  const int *alloc_list, *excess_list;
  unsigned *alloc_bits, *touched;
  const unsigned *q2;
  unsigned *keys;
  const int *ranks;
  SceneCounters *cnt;
  MergeCounters *mc;
  const HashEntry *src_hash;
  const int *live_list;
  MultiMap fwd;
  int *born;
  int born_stamp;
  __device__ bool test(int, const NoPayload &) const { return true; }
  __device__ void prologue() const {}
  __device__ int emit(int t, int rank, bool, const NoPayload &) const {
    const bool is2 = (q2[t >> 5] >> (t & 31)) & 1u;
    const int own = ranks[t];
    const int k1 = is2 ? rank - own : own, k2 = is2 ? own : rank - own;
    // the winner: the block the largest key asked for (and the keys clean for the next pass)
    const unsigned kz = keys[t] - 1u;
    keys[t] = 0;
    int B[3];
    merge_target(fwd, load_entry(src_hash, live_list[kz >> 9]), (int)(kz & 511u), B);
    // voxel-block slots taken by all earlier requests in hash-index order (closed form)
    const int base_free = cnt->base_free, base_free_ex = cnt->base_free_ex;
    const int avail_vba = base_free + 1, avail_ex = base_free_ex + 1;
    const int vr = k1 + (k2 < avail_ex ? k2 : avail_ex);
    if (vr >= avail_vba || (is2 && k2 >= avail_ex)) return 0;
    const int slot = alloc_list[base_free - vr];
    int entry = t;
    if (is2) {
      const int ex_off = excess_list[base_free_ex - k2];
      hash[t].offset = ex_off + 1;
      entry = num_buckets + ex_off;
    }
    store_entry(hash, entry, B[0], B[1], B[2], 0, slot);
    bit_set(alloc_bits, entry);
    bit_set(touched, entry);
    if (born) born[slot] = born_stamp;
    atomicAdd(is2 ? &mc->served2 : &mc->served1, 1);
    return 0;
  }
  __device__ void finish(int) const {}
};

// p.changed: [gridDim.x] voxels changed, summed by the host
__global__ __launch_bounds__(kMergeThreads) void k_merge_blocks(MergeBlockParams p) {
  merge_pull<1>(p, [max_w = p.max_w](unsigned slo, unsigned shi, unsigned &dlo, unsigned &dhi, int *) { combine_voxel(slo, shi, dlo, dhi, max_w); });
}

// ---- host side ------------------------------------------------------------------------------------------------
int ensure_merge_scratch(dslam_engine *e, int src_entries, int dst_entries) {
  MergeScratch &have = e->merge;
  if (have.keys && have.src_entries >= src_entries && have.dst_entries >= dst_entries) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));   // (nothing in flight may still use the old set)
  MergeScratch m;
  m.src_entries = std::max(src_entries, have.src_entries);
  m.dst_entries = std::max(dst_entries, have.dst_entries);
  m.words = bit_tiles(m.dst_entries) * kBitTileWords;
  DSLAM_TRY(m.keys.alloc_zeroed((size_t)m.dst_entries, e->stream));
  DSLAM_TRY(m.bits.alloc((size_t)m.words * 4));
  DSLAM_TRY(m.ranks.alloc((size_t)m.dst_entries));
  DSLAM_TRY(m.touched_list.alloc((size_t)m.dst_entries));
  DSLAM_TRY(m.live_list.alloc((size_t)m.src_entries));
  DSLAM_TRY(m.counters.alloc_zeroed(1, e->stream));
  DSLAM_TRY(m.counters_host.alloc(2));
  DSLAM_TRY(m.changed.alloc((size_t)kMergeGrid * 4, hipHostMallocMapped));
  have = std::move(m);
  return DSLAM_OK;
}

namespace {

// dslam_debug_merge_phases: wall clock per phase, each closed by a wait for the stream (only when the hook is on)
struct PhaseClock {
  dslam_engine *e;
  std::chrono::steady_clock::time_point t0;
  explicit PhaseClock(dslam_engine *e_) : e(e_), t0(std::chrono::steady_clock::now()) {}
  int lap(int phase) {
    if (!e->merge_phases_on) return DSLAM_OK;
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    const auto t1 = std::chrono::steady_clock::now();
    e->merge_phase_ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return DSLAM_OK;
  }
};

}  // namespace

// src / dst / X / params already checked and defaulted by dslam_merge_maps; reuse_live: the source's live list and its
// count are those an unmerge of the same source has just left in the scratch (dslam_remerge_maps)
int launch_merge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float *X_in,
                      const dslam_merge_params *mp, dslam_merge_result *res, bool reuse_live) {
  MultiMap fwd, inv;
  DSLAM_TRY(merge_begin(e, src, dst, X_in, fwd, inv));
  MergeScratch &m = e->merge;
  const int N = dst->n_entries;
  unsigned *q1 = m.bits, *q2 = m.bits + m.words, *req = m.bits + 2 * (size_t)m.words, *touched = m.bits + 3 * (size_t)m.words;
  MergeCounters *mc = m.counters;

  for (double &ms : e->merge_phase_ms) ms = 0.0;
  PhaseClock clock(e);
  DSLAM_HIP(hipMemsetAsync(m.bits, 0, (size_t)m.words * 4 * sizeof(unsigned), e->stream));
  if (!reuse_live) DSLAM_TRY(launch_live_list(e, src, m.live_list, &mc->live));
  DSLAM_HIP(hipGetLastError());
  DSLAM_TRY(clock.lap(0));

  MergeMarkParams kp;
  merge_fill_walk(kp, e, src, dst, fwd);
  kp.keys = m.keys; kp.q1 = q1; kp.q2 = q2; kp.req = req; kp.touched = touched; kp.mc = mc;

  SelMergeRank rank;
  rank.ranks = m.ranks;
  SelMergeServe serve;
  serve.hash = dst->hash; serve.num_buckets = dst->p.num_buckets;
  serve.alloc_list = dst->alloc_list; serve.excess_list = dst->excess_list;
  serve.alloc_bits = dst->alloc_bits; serve.touched = touched; serve.q2 = q2; serve.keys = m.keys; serve.ranks = m.ranks;
  serve.cnt = dst->counters; serve.mc = mc;
  serve.src_hash = src->hash; serve.live_list = m.live_list; serve.fwd = fwd;
  serve.born = dst->alloc_born; serve.born_stamp = dst->alloc_born_stamp;

  memset(res, 0, sizeof *res);
  MergeCounters *host = m.counters_host;
  for (int pass = 0;; pass++) {
    if (pass > 0) DSLAM_HIP(hipMemsetAsync(m.bits, 0, (size_t)m.words * 3 * sizeof(unsigned), e->stream));
    hipLaunchKernelGGL(k_merge_begin, dim3(1), dim3(1), 0, e->stream, dst->counters.get(), mc);
    hipLaunchKernelGGL(k_merge_mark, dim3(kMergeGrid), dim3(kMergeThreads), 0, e->stream, kp);
    dbg_sync(e, "k_merge_mark");
    DSLAM_TRY(clock.lap(1));
    DSLAM_TRY(launch_bits_select(e, q1, N, rank, (int *)nullptr, N, (int *)nullptr, dst->counters));
    DSLAM_TRY(launch_bits_select(e, q2, N, rank, (int *)nullptr, N, (int *)nullptr, dst->counters));
    DSLAM_TRY(launch_bits_select(e, req, N, serve, (int *)nullptr, N, &mc->requests, dst->counters));
    hipLaunchKernelGGL(k_merge_end, dim3(1), dim3(1), 0, e->stream, dst->counters.get(), (const MergeCounters *)mc);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(clock.lap(2));
    DSLAM_HIP(hipMemcpyAsync(host, mc, sizeof(MergeCounters), hipMemcpyDeviceToHost, e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    DSLAM_TRY(clock.lap(4));
    const int served = host->served1 + host->served2;
    res->passes = pass + 1;
    res->blocks_allocated += served;
    if (pass == 0) {
      res->src_blocks = host->live;
      res->src_candidates = (int64_t)host->candidates;
      res->out_of_range = (int64_t)host->out_of_range;
    }
    if (host->requests == 0) break;
    if (served == 0 || res->passes >= mp->max_passes) {
      res->exhausted = 1;
      res->requests_unserved = host->requests - served;
      break;
    }
  }
  // (the ordered list of touched entries counts as selection work)
  DSLAM_TRY(merge_pull_touched(e, dst, inv, mp->with_colour, k_merge_blocks, "k_merge_blocks", m.changed.device(), [&] { return clock.lap(2); }));
  DSLAM_TRY(clock.lap(3));
  DSLAM_HIP(hipMemcpyAsync(host, mc, sizeof(MergeCounters), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  res->blocks_touched = host->touched;
  unsigned long long changed = 0;
  for (int g = 0; g < kMergeGrid; g++) changed += m.changed[g];
  res->voxels_changed = (int64_t)changed;
  DSLAM_TRY(clock.lap(4));
  return device_errors(e);
}

}  // namespace dslam
