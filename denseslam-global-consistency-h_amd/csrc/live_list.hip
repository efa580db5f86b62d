// live_list.hip -- a bitmap of the hash table as an ordered list, for every call that walks a map's resident entries.
//
// The live list of a scene is its alloc_bits as a list: every entry with ptr >= 0, ascending (an entry whose bit is set
// but whose block is swapped out, ptr == -1, is not listed).  The mesh and the composite mesh, the pairwise and the
// joint registration, merge and unmerge, the overlap survey and pack all read it; the merge and the unmerge also want
// their `touched` bitmap as a list.  Both are one launch of k_bits_select (dslam_bits.h), and this is the only
// translation unit that instantiates that kernel for them: the shared library holds each of the two once, and a new
// caller calls a function instead of instantiating a kernel of its own.
#include "dslam_bits.h"

namespace dslam {

namespace {

// every entry with a resident block
struct SelLive {
  DSLAM_SEL_NO_LOAD
  const HashEntry *hash;
  __device__ bool test(int t, const NoPayload &) const { return hash[t].ptr >= 0; }
  __device__ void prologue() const {}
  __device__ int emit(int, int, bool, const NoPayload &) const { return 0; }
  __device__ void finish(int) const {}
};

// every set bit
struct SelSetBits {
  DSLAM_SEL_NO_LOAD
  __device__ bool test(int, const NoPayload &) const { return true; }
  __device__ void prologue() const {}
  __device__ int emit(int, int, bool, const NoPayload &) const { return 0; }
  __device__ void finish(int) const {}
};

}  // namespace

int launch_live_list(dslam_engine *e, const dslam_scene *s, int *list_out, int *count_out) {
  return launch_bits_select(e, s->alloc_bits, s->n_entries, SelLive{s->hash}, list_out, s->n_entries, count_out, s->counters);
}

int launch_bits_list(dslam_engine *e, const unsigned *bits, int n_entries, int *list_out, int *count_out, SceneCounters *err_cnt) {
  return launch_bits_select(e, bits, n_entries, SelSetBits(), list_out, n_entries, count_out, err_cnt);
}

int fill_live_lists(dslam_engine *e, const dslam_scene *const *scenes, int n, const std::vector<int> &wanted,
                    std::vector<int> &list_offset, std::vector<int> &live) {
  list_offset.assign(n, -1);
  live.assign(n, 0);
  long long entries = 0;
  int max_entries = 0, max_blocks = 0;
  for (int i : wanted) {
    list_offset[i] = (int)entries;
    entries += scenes[i]->n_entries;
  }
  for (int i = 0; i < n; i++) {
    max_entries = std::max(max_entries, scenes[i]->n_entries);
    max_blocks = std::max(max_blocks, scenes[i]->p.num_local_blocks);
  }
  DSLAM_REQUIRE(entries <= 0x7fffffffLL, "the maps' hash tables together exceed the survey's 31-bit list index");
  DSLAM_TRY(ensure_scratch(e, max_entries, max_blocks));
  LiveLists &ll = e->live_lists;
  if (!ll.live_list || ll.entries < (int)entries) {
    DSLAM_HIP(hipStreamSynchronize(e->stream));   // (nothing in flight may still use the old set)
    LiveLists grown;
    grown.entries = std::max((int)entries, ll.entries);
    DSLAM_TRY(grown.live_list.alloc((size_t)grown.entries));
    DSLAM_TRY(grown.live_counts.alloc_zeroed((size_t)DSLAM_MAX_RENDER_MAPS, e->stream));
    DSLAM_TRY(grown.live_counts_host.alloc((size_t)DSLAM_MAX_RENDER_MAPS));
    ll = std::move(grown);
  }
  for (int i : wanted) DSLAM_TRY(launch_live_list(e, scenes[i], ll.live_list + list_offset[i], ll.live_counts + i));
  DSLAM_HIP(hipGetLastError());
  DSLAM_HIP(hipMemcpyAsync(ll.live_counts_host, ll.live_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  for (int i : wanted) live[i] = std::min(std::max(ll.live_counts_host[i], 0), scenes[i]->n_entries);
  return DSLAM_OK;
}

}  // namespace dslam
