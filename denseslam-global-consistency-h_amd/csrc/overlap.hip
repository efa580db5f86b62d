// overlap.hip -- which local maps overlap, and the pairs to register (dslam_survey_overlaps, dslam_select_register_pairs;
// ITMMainEngine::SurveyLocalMapOverlaps / AlignAllLocalMaps in the mirror).
//
// Reference: none.  The law is this project's own (include/dslam_fusion.h states it in full): for
// every ordered pair (s, d) of N maps, the 8 octant centres c = 8 B + (1.5 + 4 o) of every resident block B of s are
// taken to d's voxel frame by X~_sd = T~_d inv(T~_s) (register_host.h: section 15's pair transform), and an octant is
// shared when d holds a resident block at floor(q) >> 3.  Only hash entries are read, never a voxel; all maps are only
// read; the counts are integers, so the result is exact and the same on every run.
//
// Device work per call: one ordered compaction of the resident entries of every map (fill_live_lists, live_list.hip) into
// the engine's live lists, one read-back of the counts, one copy of the call's tables to the device, and k_survey_overlaps,
// once: a fixed grid of kSurveyGrid workgroups, cut by the host into one contiguous range per SOURCE map in proportion to
// the live counts (split_workgroups, the rule of dslam_register_graph with maps in place of pairs).  A source's live
// blocks are taken eight at a time; an item is (group of eight blocks, destination map), and wave v of workgroup w of a
// range of G takes the items (w - first) * 4 + v, + 4 G, ...: the destination of an item is wave-uniform, so the map's
// descriptor and the pair's transform are read with scalar indices, as k_register_graph reads its job table.  Lane l of
// the wave takes octant l & 7 of block l >> 3 of the group: the eight probes of a block fall into one destination block
// or its neighbours, so they share bucket heads.  A ballot gives the item's counts (shared octants: its population;
// shared blocks: its non-zero bytes); lane 0 adds them to the workgroup's 2 N counters in LDS.  One row of 2 N int32 per
// workgroup in mapped page-locked memory (a workgroup without an item writes zeros); the host adds each source's rows.
// No global atomics, no workgroup waits for another, no scratch memory.
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "dslam_internal.h"
#include "mesh_device.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {

constexpr int kSurveyGrid = 512;      // workgroups: two per CU of an MI355X
constexpr int kSurveyThreads = 256;
constexpr int kSurveyWaves = kSurveyThreads / 64;
constexpr int kSurveyGroup = 8;       // source blocks per item: 8 blocks x 8 octants = one wave

// one map of a survey, as the kernel reads it: as a destination (table) and as a source (list, workgroups)
struct SurveyMap {
  const HashEntry *hash;
  int num_buckets, n_entries;
  unsigned mask;
  int list_offset;           // its resident entries: live_list[list_offset .. list_offset + live)
  int live;
  int first_wg, num_wg;      // the workgroups that walk it as a source
  int pad;
};
// X~_sd, rounded: pair s * N + d
struct SurveyPair {
  float T[12];
  int identity;
  int pad[3];
};

struct SurveyParams {
  const int *wg_map;         // [gridDim.x] the source map of each workgroup
  const SurveyMap *maps;     // [N]
  const SurveyPair *pairs;   // [N][N]
  const int *live_list;
  int num_maps;
  int *rows;                 // [gridDim.x][2 N]: shared blocks, then shared octants, per destination
};


// Does the map hold a resident entry at block (bx, by, bz)?  The ordinary walk -- bucket head, then the excess chain --
// with two guards a well-formed table never meets: a link that leaves the table ends the walk, and so does a chain longer
// than the excess area (an uploaded table may hold anything).
__device__ __forceinline__ bool holds_block(const SurveyMap &m, int bx, int by, int bz) {
  int idx = hash_index(bx, by, bz, m.mask);
  for (int steps = m.n_entries - m.num_buckets; ; steps--) {
    const HashEntry he = load_entry(m.hash, idx);
    if (he.pos[0] == bx && he.pos[1] == by && he.pos[2] == bz && he.ptr >= 0) return true;
    if (he.offset < 1 || steps <= 0) return false;
    idx = m.num_buckets + he.offset - 1;
    if ((unsigned)idx >= (unsigned)m.n_entries) return false;
  }
}

__global__ __launch_bounds__(kSurveyThreads) void k_survey_overlaps(SurveyParams p) {
  __shared__ int s_counts[2 * DSLAM_MAX_RENDER_MAPS];
  const int n = p.num_maps;
  if ((int)threadIdx.x < 2 * n) s_counts[threadIdx.x] = 0;
  __syncthreads();
  // (split_workgroups hands out the whole grid, so every workgroup has a source)
  const int src = __builtin_amdgcn_readfirstlane(p.wg_map[blockIdx.x]);
  const SurveyMap &sm = p.maps[src];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int live = sm.live;
  const int groups = (live + kSurveyGroup - 1) / kSurveyGroup;
  const long long items = (long long)groups * n;
  const long long stride = (long long)sm.num_wg * kSurveyWaves;
  const int o = lane & 7;
  const float ox = 1.5f + 4.0f * (float)(o & 1), oy = 1.5f + 4.0f * (float)((o >> 1) & 1), oz = 1.5f + 4.0f * (float)(o >> 2);
  int have_group = -1;
  bool resident = false;
  float cx = 0.0f, cy = 0.0f, cz = 0.0f;
  for (long long item = (long long)((int)blockIdx.x - sm.first_wg) * kSurveyWaves + wave; item < items; item += stride) {
    const int g = (int)(item / n), d = (int)(item - (long long)g * n);   // (wave-uniform)
    if (d == src) continue;   // (the diagonal is a definition, not a probe)
    if (g != have_group) {
      have_group = g;
      const int b = g * kSurveyGroup + (lane >> 3);
      resident = false;
      if (b < live) {
        const HashEntry he = load_entry(sm.hash, p.live_list[sm.list_offset + b]);
        resident = he.ptr >= 0;   // (a live entry holds a block)
        // exact in float32: |8 B + 5.5| < 2^19
        cx = (float)(he.pos[0] * kBlock) + ox;
        cy = (float)(he.pos[1] * kBlock) + oy;
        cz = (float)(he.pos[2] * kBlock) + oz;
      }
    }
    const SurveyMap &dm = p.maps[d];
    const SurveyPair &X = p.pairs[src * n + d];
    float qx = cx, qy = cy, qz = cz;
    if (!X.identity) {
      qx = ((X.T[0] * cx + X.T[1] * cy) + X.T[2] * cz) + X.T[3];
      qy = ((X.T[4] * cx + X.T[5] * cy) + X.T[6] * cz) + X.T[7];
      qz = ((X.T[8] * cx + X.T[9] * cy) + X.T[10] * cz) + X.T[11];
    }
    const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
    // D = cell >> 3 lies in [-32768, 32767] exactly when the cell lies in [-262144, 262143]; anything else -- a NaN
    // included -- is not shared, and the casts below stay defined
    bool shared = resident && fx >= -262144.0f && fx < 262144.0f && fy >= -262144.0f && fy < 262144.0f && fz >= -262144.0f &&
                  fz < 262144.0f;
    if (shared) shared = holds_block(dm, (int)fx >> 3, (int)fy >> 3, (int)fz >> 3);
    const unsigned long long m = __ballot(shared);
    if (lane == 0 && m) {
      int blocks = 0;
#pragma unroll
      for (int k = 0; k < kSurveyGroup; k++) blocks += ((m >> (8 * k)) & 0xffull) != 0ull;
      atomicAdd(&s_counts[d], blocks);              // (LDS; integer sums do not depend on the order)
      atomicAdd(&s_counts[n + d], __popcll(m));
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * n) p.rows[(size_t)blockIdx.x * (2 * n) + threadIdx.x] = s_counts[threadIdx.x];
}

// ---- host side ------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kWgTableBytes = (size_t)kSurveyGrid * sizeof(int);
constexpr size_t kMapTableBytes = (size_t)DSLAM_MAX_RENDER_MAPS * sizeof(SurveyMap);
constexpr size_t kPairTableBytes = (size_t)DSLAM_MAX_RENDER_MAPS * DSLAM_MAX_RENDER_MAPS * sizeof(SurveyPair);
static_assert(kWgTableBytes % 16 == 0 && sizeof(SurveyMap) % 8 == 0 && sizeof(SurveyPair) == 64, "table layout");

int ensure_overlap_scratch(dslam_engine *e) {
  if (e->overlap.tables) return DSLAM_OK;
  OverlapScratch s;   // (the engine gets the three together or none)
  DSLAM_TRY(s.rows.alloc((size_t)kSurveyGrid * 2 * DSLAM_MAX_RENDER_MAPS, hipHostMallocMapped));
  DSLAM_TRY(s.tables_host.alloc(kWgTableBytes + kMapTableBytes + kPairTableBytes));
  DSLAM_TRY(s.tables.alloc(kWgTableBytes + kMapTableBytes + kPairTableBytes));
  e->overlap = std::move(s);
  return DSLAM_OK;
}

}  // namespace

// everything already checked by dslam_survey_overlaps
int launch_survey_overlaps(dslam_engine *e, const dslam_scene *const *scenes, const float *T_in, int num_maps, int32_t *live_out,
                           int32_t *blocks_out, int32_t *octants_out) {
  const int n = num_maps;
  // ---- the live lists of all maps ----
  std::vector<int> all(n), list_offset, live, first_wg(n, 0), num_wg(n, 0);
  std::iota(all.begin(), all.end(), 0);
  DSLAM_TRY(fill_live_lists(e, scenes, n, all, list_offset, live));
  DSLAM_TRY(ensure_overlap_scratch(e));
  OverlapScratch &sc = e->overlap;
  split_workgroups(kSurveyGrid, all, live, first_wg, num_wg);

  // ---- the tables ----
  char *host = static_cast<char *>(sc.tables_host.get());
  int *wg_map = reinterpret_cast<int *>(host);
  SurveyMap *maps = reinterpret_cast<SurveyMap *>(host + kWgTableBytes);
  SurveyPair *pairs = reinterpret_cast<SurveyPair *>(host + kWgTableBytes + kMapTableBytes);
  const double vs = (double)scenes[0]->p.voxel_size;
  std::vector<double> T((size_t)n * 12);
  for (int i = 0; i < n; i++) {
    const dslam_scene *s = scenes[i];
    SurveyMap &m = maps[i];
    memset(&m, 0, sizeof m);
    m.hash = s->hash;
    m.num_buckets = s->p.num_buckets; m.n_entries = s->n_entries;
    m.mask = (unsigned)(s->p.num_buckets - 1);
    m.list_offset = list_offset[i];
    m.live = live[i];
    m.first_wg = first_wg[i]; m.num_wg = num_wg[i];
    for (int w = 0; w < num_wg[i]; w++) wg_map[first_wg[i] + w] = i;
    voxel_pose(T_in + 16 * i, vs, &T[(size_t)i * 12]);
  }
  memset(pairs, 0, (size_t)n * n * sizeof(SurveyPair));
  for (int s = 0; s < n; s++)
    for (int d = 0; d < n; d++) {
      if (s == d) continue;
      double X[12];
      SurveyPair &sp = pairs[s * n + d];
      sp.identity = pair_transform(&T[(size_t)s * 12], &T[(size_t)d * 12], X, sp.T) ? 1 : 0;
    }
  const size_t table_bytes = kWgTableBytes + kMapTableBytes + (size_t)n * n * sizeof(SurveyPair);
  DSLAM_HIP(hipMemcpyAsync(sc.tables.get(), host, table_bytes, hipMemcpyHostToDevice, e->stream));
  const char *dev = static_cast<const char *>(sc.tables.get());
  SurveyParams kp;
  memset(&kp, 0, sizeof kp);
  kp.wg_map = reinterpret_cast<const int *>(dev);
  kp.maps = reinterpret_cast<const SurveyMap *>(dev + kWgTableBytes);
  kp.pairs = reinterpret_cast<const SurveyPair *>(dev + kWgTableBytes + kMapTableBytes);
  kp.live_list = e->live_lists.live_list;
  kp.num_maps = n;
  kp.rows = sc.rows.device();
  hipLaunchKernelGGL(k_survey_overlaps, dim3(kSurveyGrid), dim3(kSurveyThreads), 0, e->stream, kp);
  DSLAM_HIP(hipGetLastError());
  DSLAM_HIP(hipStreamSynchronize(e->stream));   // (which also lets the next call rewrite the page-locked tables)
  DSLAM_TRY(device_errors(e));

  // ---- each source's rows, added in index order ----
  std::vector<long long> sums((size_t)2 * n);
  for (int s = 0; s < n; s++) {
    std::fill(sums.begin(), sums.end(), 0LL);
    for (int w = first_wg[s]; w < first_wg[s] + num_wg[s]; w++)
      for (int k = 0; k < 2 * n; k++) sums[k] += sc.rows[(size_t)w * (2 * n) + k];
    for (int d = 0; d < n; d++) {
      // the diagonal: every resident block and octant of a map, by definition
      const long long blocks = s == d ? (long long)live[s] : sums[d], octants = s == d ? 8LL * live[s] : sums[n + d];
      if (blocks_out) blocks_out[s * n + d] = (int32_t)blocks;
      octants_out[s * n + d] = (int32_t)octants;
    }
    live_out[s] = live[s];
  }
  return DSLAM_OK;
}

// ---- the selection (host only) --------------------------------------------------------------------------------
void select_register_pairs(const int32_t *live, const int32_t *shared, int n, const dslam_pair_select_params &sp, int32_t *pairs_out,
                           int32_t *component_out, dslam_pair_select_result *result) {
  struct Pair { int s, d, shared; };
  auto qualifies = [&](int s, int d) { return s != d && shared[s * n + d] >= sp.min_shared_octants; };
  // 1. / 2. the kept pairs, and 3. the components of the qualifying pairs (undirected)
  std::vector<Pair> kept;
  std::vector<int> comp(n);
  std::iota(comp.begin(), comp.end(), 0);
  auto find = [](std::vector<int> &set, int i) {
    while (set[i] != i) i = set[i] = set[set[i]];
    return i;
  };
  // (the smaller root wins, so a set's root is its smallest member)
  auto join = [&](std::vector<int> &set, int a, int b) {
    a = find(set, a); b = find(set, b);
    if (a == b) return false;
    set[std::max(a, b)] = std::min(a, b);
    return true;
  };
  for (int s = 0; s < n; s++)
    for (int d = 0; d < n; d++) {
      if (!qualifies(s, d)) continue;
      join(comp, s, d);
      if (sp.one_direction && qualifies(d, s)) {
        // the direction whose source is covered more: shared[a][b] / (8 live[a]) against shared[b][a] / (8 live[b]), a < b
        const int a = std::min(s, d), b = std::max(s, d);
        const long long ab = (long long)shared[a * n + b] * (long long)live[b], ba = (long long)shared[b * n + a] * (long long)live[a];
        const bool keep_ab = ab >= ba;
        if ((s == a) != keep_ab) continue;
      }
      kept.push_back({s, d, shared[s * n + d]});
    }
  int components = 0;
  for (int i = 0; i < n; i++) {
    component_out[i] = find(comp, i);
    components += component_out[i] == i;
  }
  // 4. the cap: spanning pairs first, then the rest by rank
  std::vector<int> order(kept.size());
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    const Pair &a = kept[x], &b = kept[y];
    if (a.shared != b.shared) return a.shared > b.shared;
    return a.s != b.s ? a.s < b.s : a.d < b.d;
  });
  std::vector<char> taken(kept.size(), 0);
  std::vector<int> tree(n);
  std::iota(tree.begin(), tree.end(), 0);
  int selected = 0;
  for (int k : order)
    if (selected < sp.max_pairs && join(tree, kept[k].s, kept[k].d)) { taken[k] = 1; selected++; }
  for (int k : order)
    if (selected < sp.max_pairs && !taken[k]) { taken[k] = 1; selected++; }
  // 5. by (s, d) ascending: the order `kept` was made in
  int at = 0;
  for (size_t k = 0; k < kept.size(); k++)
    if (taken[k]) { pairs_out[2 * at] = kept[k].s; pairs_out[2 * at + 1] = kept[k].d; at++; }
  result->qualifying = (int32_t)kept.size();
  result->selected = selected;
  result->num_components = components;
  result->pad = 0;
}

}  // namespace dslam
