// unmerge.hip -- take one local map out of another again on the device (dslam_unmerge_maps, and the removal half of
// dslam_remerge_maps; ITMMainEngine::UnmergeLocalMap / RemergeLocalMap in the mirror).
//
// Reference: none.  The law is this project's own (include/dslam_fusion.h states it in full): the
// inverse of dslam_merge_maps under the same X.  The source is only read; the destination's table, free lists, counters,
// alloc_bits and born stamps are not written.
//
//   1. push    as the merge's: every source voxel with w_depth > 0 names the destination block B it falls into
//              (merge_target of merge_device.h);
//   2. lookup  k_unmerge_mark (merge_walk of merge_device.h) looks every B up in the destination: a hit sets the entry's
//              bit in `touched`, a miss counts the voxels that asked (one lane probes for a run of neighbouring lanes
//              with the same B and adds the run's length).  Nothing is requested and nothing allocated, so there is one
//              pass;
//   3. pull    k_unmerge_blocks: k_merge_blocks' shape, stated once as merge_pull of merge_device.h (fixed grid,
//              grid-stride over the ordered list of touched entries, lane t the voxels 2t and 2t + 1 as one 16-byte
//              access).  Each voxel resamples the source exactly as the
//              merge did (merge_resample) and takes the result out of the resident voxel with uncombine_voxel
//              (combine_device.h).  One row of three counts per workgroup goes to mapped host memory.
// No kernel here waits for another workgroup.
#include <cstring>

#include "combine_device.h"
#include "dslam_internal.h"
#include "merge_device.h"
#include "mesh_device.h"
#include "multimap_device.h"

#pragma clang fp contract(off)

namespace dslam {

__global__ void k_unmerge_begin(MergeCounters *mc) {
  mc->candidates = 0; mc->out_of_range = 0; mc->without_block = 0;
}

struct UnmergeMarkParams : MergeWalkParams {
  unsigned *touched;
  MergeCounters *mc;
};

// a hit sets the entry's bit in `touched`; a miss counts the voxels the prober answers for
__global__ __launch_bounds__(kMergeThreads) void k_unmerge_mark(UnmergeMarkParams p) {
  merge_walk<3>(p, p.mc, [&](const MergeProbe &pr, int, int, int run, int *n) {
    if (pr.found) merge_touch(p.touched, pr.h);
    else n[2] += run;
  });
}

// p.changed: [gridDim.x][3] -- voxels changed, depth halves underweight, colour halves underweight; p.max_w is not used
__global__ __launch_bounds__(kMergeThreads) void k_unmerge_blocks(MergeBlockParams p) {
  merge_pull<3>(p, [](unsigned slo, unsigned shi, unsigned &dlo, unsigned &dhi, int *n) { uncombine_voxel(slo, shi, dlo, dhi, n[1], n[2]); });
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
  MultiMap fwd, inv;
  DSLAM_TRY(merge_begin(e, src, dst, X_in, fwd, inv));
  MergeScratch &m = e->merge;
  unsigned *touched = m.bits + 3 * (size_t)m.words;
  MergeCounters *mc = m.counters;

  DSLAM_HIP(hipMemsetAsync(touched, 0, (size_t)m.words * sizeof(unsigned), e->stream));
  DSLAM_TRY(launch_live_list(e, src, m.live_list, &mc->live));

  UnmergeMarkParams kp;
  merge_fill_walk(kp, e, src, dst, fwd);
  kp.touched = touched; kp.mc = mc;
  hipLaunchKernelGGL(k_unmerge_begin, dim3(1), dim3(1), 0, e->stream, mc);
  hipLaunchKernelGGL(k_unmerge_mark, dim3(kMergeGrid), dim3(kMergeThreads), 0, e->stream, kp);
  dbg_sync(e, "k_unmerge_mark");

  DSLAM_TRY(merge_pull_touched(e, dst, inv, with_colour, k_unmerge_blocks, "k_unmerge_blocks", m.changed.device() + kMergeGrid, [] { return (int)DSLAM_OK; }));
  DSLAM_HIP(hipMemcpyAsync(m.counters_host.get() + 1, mc, sizeof(MergeCounters), hipMemcpyDeviceToHost, e->stream));
  if (defer) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  collect_unmerge_result(e, res);
  return device_errors(e);
}

}  // namespace dslam
