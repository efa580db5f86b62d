// unmerge.hip -- take one local map out of another again on the device (dslam_unmerge_maps, and the removal half of
// dslam_remerge_maps; ITMMainEngine::UnmergeLocalMap / RemergeLocalMap in the mirror).
//
// Reference: none.  The law is this project's own (include/dslam_fusion.h states it in full): the
// inverse of dslam_merge_maps under the same X.  The source is only read; the destination's table, free lists, counters,
// alloc_bits and born stamps are not written.
//
//   1. push    as the merge's: every source voxel with w_depth > 0 names the destination block B it falls into
//              (merge_target of merge_device.h);
//   2. lookup  k_unmerge_mark looks every B up in the destination: a hit sets the entry's bit in `touched`, a miss counts
//              the voxels that asked (one lane probes for a run of neighbouring lanes with the same B and adds the run's
//              length).  Nothing is requested and nothing allocated, so there is one pass;
//   3. pull    k_unmerge_blocks: k_merge_blocks' shape (fixed grid, grid-stride over the ordered list of touched entries,
//              lane t the voxels 2t and 2t + 1 as one 16-byte access).  Each voxel resamples the source exactly as the
//              merge did (merge_resample) and takes the result out of the resident voxel with uncombine_voxel
//              (combine_device.h).  One row of three counts per workgroup goes to mapped host memory.
// No kernel here waits for another workgroup.
#include <cstring>

#include "combine_device.h"
#include "dslam_bits.h"
#include "merge_device.h"
#include "mesh_device.h"
#include "multimap_device.h"

#pragma clang fp contract(off)

namespace dslam {

// its own types: the selection kernels of this translation unit are not merge.hip's
struct SelLiveUnmerge : SelLive {};
struct SelUnmergeTouched {
  DSLAM_SEL_NO_LOAD
  __device__ bool test(int, const NoPayload &) const { return true; }
  __device__ void prologue() const {}
  __device__ int emit(int, int, bool, const NoPayload &) const { return 0; }
  __device__ void finish(int) const {}
};

__global__ void k_unmerge_begin(MergeCounters *mc) {
  mc->candidates = 0; mc->out_of_range = 0; mc->without_block = 0;
}

struct UnmergeMarkParams {
  const HashEntry *src_hash;
  const uint2 *src_voxels;
  const int *live_list;
  MultiMap fwd;              // T = X~ (its map pointers are not used)
  const HashEntry *dst_hash;
  unsigned mask;
  int num_buckets;
  unsigned *touched;
  MergeCounters *mc;
};

__global__ __launch_bounds__(kMergeThreads) void k_unmerge_mark(UnmergeMarkParams p) {
  const int live = p.mc->live;
  const int lane = threadIdx.x & 63;
  int n_cand = 0, n_oor = 0, n_miss = 0;
  // k_merge_mark's job order; the trip count is the same for every lane of a workgroup
  for (int job = blockIdx.x * 2; job < live * 2; job += (job & 1) ? gridDim.x * 2 - 1 : 1) {
    const int r = job >> 1, l = (int)threadIdx.x + kMergeThreads * (job & 1);
    const HashEntry he = load_entry(p.src_hash, p.live_list[r]);
    bool cand = false;
    int B[3] = {0, 0, 0};
    if (he.ptr >= 0) {  // (uniform; a live entry holds a block)
      const unsigned own = p.src_voxels[(size_t)he.ptr * kBlock3 + l].x;
      if (((own >> 16) & 0xffu) != 0u) {
        n_cand++;
        cand = merge_target(p.fwd, he, l, B);
        n_oor += cand ? 0 : 1;
      }
    }
    // a lane whose right neighbour asks for the same block leaves the probe to it; the prober answers for its whole run:
    // the lanes between the nearest lane to its left that probes itself or asks for nothing, and itself
    const int rc = __shfl_down((int)cand, 1, 64), rx = __shfl_down(B[0], 1, 64), ry = __shfl_down(B[1], 1, 64), rz = __shfl_down(B[2], 1, 64);
    const bool probes = cand && !(lane < 63 && rc && rx == B[0] && ry == B[1] && rz == B[2]);
    const unsigned long long ends = __ballot(probes || !cand);
    if (!probes) continue;
    const unsigned long long below = ends & ((1ull << lane) - 1ull);
    const int run = lane - (below ? 64 - __clzll((long long)below) : 0) + 1;
    int h = hash_index(B[0], B[1], B[2], p.mask);
    HashEntry e = load_entry(p.dst_hash, h);   // one 16-byte load per chain step
    bool found = e.pos[0] == B[0] && e.pos[1] == B[1] && e.pos[2] == B[2] && e.ptr >= -1;
    if (!found && e.ptr >= -1) {
      while (e.offset >= 1) {
        h = p.num_buckets + e.offset - 1;
        e = load_entry(p.dst_hash, h);
        if (e.pos[0] == B[0] && e.pos[1] == B[1] && e.pos[2] == B[2] && e.ptr >= -1) { found = true; break; }
      }
    }
    if (found) {
      const unsigned bit = 1u << (h & 31);
      if (!(p.touched[h >> 5] & bit)) atomicOr(&p.touched[h >> 5], bit);
    } else {
      n_miss += run;
    }
  }
  // integer counts: the order of the additions does not matter
  for (int d = 32; d > 0; d >>= 1) {
    n_cand += __shfl_xor(n_cand, d, 64); n_oor += __shfl_xor(n_oor, d, 64); n_miss += __shfl_xor(n_miss, d, 64);
  }
  if (lane == 0 && n_cand) {
    atomicAdd(&p.mc->candidates, (unsigned long long)n_cand);
    if (n_oor) atomicAdd(&p.mc->out_of_range, (unsigned long long)n_oor);
    if (n_miss) atomicAdd(&p.mc->without_block, (unsigned long long)n_miss);
  }
}

// p.changed: [gridDim.x][3] -- voxels changed, depth halves underweight, colour halves underweight; p.max_w is not used
__global__ __launch_bounds__(kMergeThreads) void k_unmerge_blocks(MergeBlockParams p) {
  const int n = p.mc->touched;
  const VolumeRef vol = volume_of(p.src);
  const int tid = threadIdx.x;
  const int x = (tid & 3) * 2, y = (tid >> 2) & 7, z = tid >> 5;
  int changed = 0, under_d = 0, under_c = 0;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const HashEntry he = load_entry(p.dst_hash, p.touched_list[i]);
    if (he.ptr < 0) continue;  // (uniform; a touched entry holds a block)
    uint4 *blk = p.dst_voxels + (size_t)he.ptr * (kBlock3 / 2);
    const uint4 was = blk[tid];
    uint4 d = was;
    const int px = he.pos[0] * kBlock + x, py = he.pos[1] * kBlock + y, pz = he.pos[2] * kBlock + z;
    const uint2 s0 = merge_resample(p, vol, px, py, pz);
    const uint2 s1 = merge_resample(p, vol, px + 1, py, pz);
    uncombine_voxel(s0.x, s0.y, d.x, d.y, under_d, under_c);
    uncombine_voxel(s1.x, s1.y, d.z, d.w, under_d, under_c);
    const int c = (int)(d.x != was.x || d.y != was.y) + (int)(d.z != was.z || d.w != was.w);
    if (c) blk[tid] = d;
    changed += c;
  }
  // one row per workgroup, summed by the host in index order (a workgroup without a block writes its zeros)
  __shared__ int red[kMergeThreads / 64][3];
  for (int dlt = 32; dlt > 0; dlt >>= 1) {
    changed += __shfl_xor(changed, dlt, 64); under_d += __shfl_xor(under_d, dlt, 64); under_c += __shfl_xor(under_c, dlt, 64);
  }
  if ((tid & 63) == 0) { red[tid >> 6][0] = changed; red[tid >> 6][1] = under_d; red[tid >> 6][2] = under_c; }
  __syncthreads();
  if (tid < 3) {
    unsigned long long v = 0;
    for (int w = 0; w < kMergeThreads / 64; w++) v += (unsigned long long)red[w][tid];
    p.changed[(size_t)blockIdx.x * 3 + tid] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
// the unmerge's rows in MergeScratch::changed lie behind the merge's counts, its read-back in counters_host[1]: a merge
// enqueued behind a deferred unmerge (dslam_remerge_maps) overwrites neither
void collect_unmerge_result(dslam_engine *e, dslam_unmerge_result *res) {
  MergeScratch &m = e->merge;
  const MergeCounters *host = m.counters_host.get() + 1;
  memset(res, 0, sizeof *res);
  res->src_blocks = host->live;
  res->blocks_touched = host->touched;
  res->src_candidates = (int64_t)host->candidates;
  res->out_of_range = (int64_t)host->out_of_range;
  res->candidates_without_block = (int64_t)host->without_block;
  const unsigned long long *rows = m.changed.get() + kMergeGrid;
  unsigned long long sum[3] = {0, 0, 0};
  for (int g = 0; g < kMergeGrid; g++)
    for (int k = 0; k < 3; k++) sum[k] += rows[(size_t)g * 3 + k];
  res->voxels_changed = (int64_t)sum[0];
  res->depth_underweight = (int64_t)sum[1];
  res->colour_underweight = (int64_t)sum[2];
}

int launch_unmerge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float *X_in, int with_colour,
                        dslam_unmerge_result *res, bool defer) {
  DSLAM_TRY(ensure_scratch(e, std::max(src->n_entries, dst->n_entries), std::max(src->p.num_local_blocks, dst->p.num_local_blocks)));
  DSLAM_TRY(ensure_merge_scratch(e, src->n_entries, dst->n_entries));
  MergeScratch &m = e->merge;
  const int N = dst->n_entries;
  unsigned *touched = m.bits + 3 * (size_t)m.words;
  MergeCounters *mc = m.counters;

  MultiMap fwd, inv;
  merge_transforms(src, X_in, fwd, inv);

  DSLAM_HIP(hipMemsetAsync(touched, 0, (size_t)m.words * sizeof(unsigned), e->stream));
  SelLiveUnmerge live;
  live.hash = src->hash;
  DSLAM_TRY(launch_bits_select(e, src->alloc_bits, src->n_entries, live, m.live_list, src->n_entries, &mc->live, src->counters));

  UnmergeMarkParams kp;
  memset(&kp, 0, sizeof kp);
  kp.src_hash = src->hash; kp.src_voxels = src->voxels; kp.live_list = m.live_list;
  kp.fwd = fwd;
  kp.dst_hash = dst->hash; kp.mask = (unsigned)(dst->p.num_buckets - 1); kp.num_buckets = dst->p.num_buckets;
  kp.touched = touched; kp.mc = mc;
  hipLaunchKernelGGL(k_unmerge_begin, dim3(1), dim3(1), 0, e->stream, mc);
  hipLaunchKernelGGL(k_unmerge_mark, dim3(kMergeGrid), dim3(kMergeThreads), 0, e->stream, kp);
  dbg_sync(e, "k_unmerge_mark");

  SelUnmergeTouched sel_touched;
  DSLAM_TRY(launch_bits_select(e, touched, N, sel_touched, m.touched_list, N, &mc->touched, dst->counters));
  MergeBlockParams bp;
  memset(&bp, 0, sizeof bp);
  bp.dst_hash = dst->hash; bp.dst_voxels = reinterpret_cast<uint4 *>(dst->voxels);
  bp.touched_list = m.touched_list; bp.mc = mc;
  bp.src = inv;
  bp.max_w = dst->p.max_w; bp.with_colour = with_colour;
  bp.changed = m.changed.device() + kMergeGrid;
  hipLaunchKernelGGL(k_unmerge_blocks, dim3(kMergeGrid), dim3(kMergeThreads), 0, e->stream, bp);
  dbg_sync(e, "k_unmerge_blocks");
  DSLAM_HIP(hipGetLastError());
  DSLAM_HIP(hipMemcpyAsync(m.counters_host.get() + 1, mc, sizeof(MergeCounters), hipMemcpyDeviceToHost, e->stream));
  if (defer) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  collect_unmerge_result(e, res);
  return device_errors(e);
}

}  // namespace dslam
