// view_survey.hip -- which local maps a camera view reaches (dslam_view_frustum_planes, dslam_survey_views,
// dslam_select_view_maps; ITMMainEngine::SurveyLocalMapsInView / TrackVisibleLocalMaps / GetImageVisibleLocalMaps in the
// mirror).
//
// Reference: none.  The law is this project's own (include/dslam_fusion.h states it in full): the
// centre c = 8 B + 4 of every resident block B of map i is taken to the world by Y~_i = inv(T~_i) and tested against the six
// planes of every view, loosened by the radius of the block's sphere and a margin; a block that passes all six reaches the
// view.  Only hash entries are read, never a voxel; all maps are only read; counts, nearest and farthest depth are
// integers, so the result is exact and the same on every run however the work is split.
//
// Device work per call: one memset of the result arrays, one copy of the call's tables to the device, and k_survey_views,
// once, whatever N and V: a fixed grid of kViewGrid workgroups over the bitmap tiles (kViewTileEntries entries of a
// scene's alloc_bits) of all maps laid end to end -- workgroup w takes the tiles [w T / G, (w + 1) T / G), a range the host
// and the kernel know from the table sizes alone, so no live list is built and nothing is read back before the launch.
// A workgroup walks its range map by map; the map of a tile is uniform, so its descriptor and Y~_i are read with scalar
// indices, as are the 28 floats of each view.  The set bits of a tile are expanded into an LDS list (expand_bits,
// dslam_bits.h) and tested densely, one candidate per lane and round.  Per view a ballot gives the round's count, which
// lane 0 adds to the workgroup's LDS counter; reaching lanes fold their depth into LDS with integer atomicMax.  When the
// workgroup leaves a map it issues at most one global atomicAdd / atomicMax per (map, view) and array.  Integer atomics
// only: no float is accumulated, no workgroup waits for another, no scratch memory.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "dslam_bits.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {

constexpr int kViewGrid = 512;        // workgroups: two per CU of an MI355X
constexpr int kViewThreads = 256;
constexpr int kViewTileWords = kViewThreads;              // one bitmap word per thread
constexpr int kViewTileEntries = kViewTileWords * 32;     // 8192: a tile-relative entry index fits the LDS list's shorts
static_assert(kBitTileWords % kViewTileWords == 0, "a view-survey tile never straddles the bitmap's padding unit");

// one map of a view survey, as the kernel reads it
struct ViewSurveyMap {
  const HashEntry *hash;
  const unsigned *bits;      // alloc_bits
  int n_entries;
  int identity;              // T_i is exactly the identity: p = c
  float Y[12];               // Y~_i rounded, 3 x 4 row-major
  int pad[2];
};

struct ViewSurveyParams {
  const int *tile_start;     // [N + 1] first tile of each map in the sequence of all tiles; [N] = their number
  const ViewSurveyMap *maps; // [N]
  const float *views;        // [V][28]
  int num_maps, num_views, total_tiles;
  float rho;
  int *live;                 // [N]
  int *reach;                // [V][N]
  unsigned *nearest;         // [V][N] the maximum of ~(zi ^ 0x80000000): the minimum of zi, in an array that starts as zeros
  unsigned *farthest;        // [V][N] the maximum of zi ^ 0x80000000
};

__global__ __launch_bounds__(kViewThreads) void k_survey_views(ViewSurveyParams p) {
  __shared__ int s_red[kViewThreads / 64];
  __shared__ unsigned short s_list[kViewTileEntries];
  __shared__ int s_live;
  __shared__ int s_reach[DSLAM_MAX_SURVEY_VIEWS];
  __shared__ unsigned s_near[DSLAM_MAX_SURVEY_VIEWS], s_far[DSLAM_MAX_SURVEY_VIEWS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = p.num_maps, nv = p.num_views;
  int tile = (int)((long long)blockIdx.x * p.total_tiles / (int)gridDim.x);
  const int tile_end = (int)((long long)(blockIdx.x + 1) * p.total_tiles / (int)gridDim.x);
  if (tile >= tile_end) return;   // (fewer tiles than workgroups)
  // the map that holds the first tile: the last i with tile_start[i] <= tile (every map has at least one tile)
  int map = 0;
  for (int hi = n - 1; map < hi;) {
    const int mid = (map + hi + 1) >> 1;
    if (p.tile_start[mid] <= tile) map = mid; else hi = mid - 1;
  }
  map = __builtin_amdgcn_readfirstlane(map);
  if (tid < DSLAM_MAX_SURVEY_VIEWS) { s_reach[tid] = 0; s_near[tid] = 0u; s_far[tid] = 0u; }
  if (tid == 0) s_live = 0;
  __syncthreads();
  const float rho = p.rho;
  for (; tile < tile_end; map++) {   // (tile < tile_end <= tile_start[n], so map stays below n)
    map = __builtin_amdgcn_readfirstlane(map);
    const ViewSurveyMap &m = p.maps[map];
    const int first = p.tile_start[map];
    const int map_end = min(tile_end, p.tile_start[map + 1]);
    for (; tile < map_end; tile++) {
      const int rel = tile - first;
      // (alloc_bits is padded with zeros to whole units of kBitTileWords words, so the tile that ends the table is all there)
      const unsigned w = m.bits[(size_t)rel * kViewTileWords + tid];
      int tot;
      const int rank0 = block_excl_scan<kViewThreads / 64>(__popc(w), s_red, tot);
      if (tot == 0) continue;   // (most tiles of a sparse table)
      expand_bits(w, tid * 32, rank0, s_list);
      __syncthreads();
      const int t0 = rel * kViewTileEntries;
      for (int base = 0; base < tot; base += kViewThreads) {   // (uniform)
        const int j = base + tid;
        bool resident = false;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (j < tot) {
          const int t = t0 + (int)s_list[j];
          if (t < m.n_entries) {
            const HashEntry he = load_entry(m.hash, t);
            resident = he.ptr >= 0;
            // exact in float32: |8 B + 4| < 2^19
            const float cx = (float)(he.pos[0] * kBlock + 4), cy = (float)(he.pos[1] * kBlock + 4), cz = (float)(he.pos[2] * kBlock + 4);
            px = cx; py = cy; pz = cz;
            if (!m.identity) {
              px = ((m.Y[0] * cx + m.Y[1] * cy) + m.Y[2] * cz) + m.Y[3];
              py = ((m.Y[4] * cx + m.Y[5] * cy) + m.Y[6] * cz) + m.Y[7];
              pz = ((m.Y[8] * cx + m.Y[9] * cy) + m.Y[10] * cz) + m.Y[11];
            }
          }
        }
        const unsigned long long live_m = __ballot(resident);
        if (live_m == 0ull) continue;   // (uniform)
        if (lane == 0) atomicAdd(&s_live, __popcll(live_m));   // (LDS; integer sums do not depend on the order)
        for (int v = 0; v < nv; v++) {
          const float *pl = p.views + v * 28;   // (uniform: scalar loads)
          bool reach = resident;
#pragma unroll
          for (int k = 0; k < 6; k++) {
            const float s = ((pl[4 * k] * px + pl[4 * k + 1] * py) + pl[4 * k + 2] * pz) + pl[4 * k + 3];
            reach = reach && s >= -rho;   // (false for a NaN)
          }
          const unsigned long long reach_m = __ballot(reach);
          if (reach_m == 0ull) continue;
          if (lane == 0) atomicAdd(&s_reach[v], __popcll(reach_m));
          if (reach) {
            const float z = ((pl[24] * px + pl[25] * py) + pl[26] * pz) + pl[27];
            const float fz = fminf(fmaxf(floorf(z), -2147483648.0f), 2147483520.0f);
            const unsigned key = (unsigned)(int)fz ^ 0x80000000u;   // (unsigned order = the order of zi)
            atomicMax(&s_near[v], ~key);
            atomicMax(&s_far[v], key);
          }
        }
      }
      __syncthreads();   // (the next tile rewrites s_list)
    }
    // ---- the workgroup leaves the map: at most one global atomic per (map, view) and array ----
    __syncthreads();
    if (tid < nv && s_reach[tid] > 0) {
      atomicAdd(&p.reach[tid * n + map], s_reach[tid]);
      atomicMax(&p.nearest[tid * n + map], s_near[tid]);
      atomicMax(&p.farthest[tid * n + map], s_far[tid]);
    }
    if (tid == 0 && s_live > 0) atomicAdd(&p.live[map], s_live);
    __syncthreads();
    if (tid < DSLAM_MAX_SURVEY_VIEWS) { s_reach[tid] = 0; s_near[tid] = 0u; s_far[tid] = 0u; }
    if (tid == 0) s_live = 0;
    __syncthreads();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------

// the law of dslam_view_frustum_planes (include/dslam_fusion.h); the view has been checked
void view_frustum_planes(const dslam_survey_view &view, float voxel_size, float out[28]) {
  const double vs = (double)voxel_size;
  double R[3][3], tv[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = (double)view.M[4 * c + r];
    tv[r] = (double)view.M[12 + r] / vs;
  }
  const double fx = (double)view.intrinsics[0], fy = (double)view.intrinsics[1];
  const double cx = (double)view.intrinsics[2], cy = (double)view.intrinsics[3];
  double nc[6][3] = {{0}}, dc[6] = {0};
  auto side = [](double a, double b, double &ua, double &ub) {
    const double len = sqrt(a * a + b * b);
    ua = a / len; ub = b / len;
  };
  side(fx, cx + 1.0, nc[0][0], nc[0][2]);
  side(-fx, (double)view.width - cx, nc[1][0], nc[1][2]);
  side(fy, cy + 1.0, nc[2][1], nc[2][2]);
  side(-fy, (double)view.height - cy, nc[3][1], nc[3][2]);
  nc[4][2] = 1.0; dc[4] = -((double)view.near_m / vs);
  nc[5][2] = -1.0; dc[5] = (double)view.far_m / vs;
  for (int k = 0; k < 6; k++) {
    for (int j = 0; j < 3; j++) out[4 * k + j] = (float)((R[0][j] * nc[k][0] + R[1][j] * nc[k][1]) + R[2][j] * nc[k][2]);
    out[4 * k + 3] = (float)(((nc[k][0] * tv[0] + nc[k][1] * tv[1]) + nc[k][2] * tv[2]) + dc[k]);
  }
  if (view.far_m == 0.0f) {
    out[20] = out[21] = out[22] = 0.0f;
    out[23] = INFINITY;
  }
  for (int j = 0; j < 3; j++) out[24 + j] = (float)R[2][j];
  out[27] = (float)tv[2];
}

namespace {

constexpr size_t kStartTableBytes = (size_t)(DSLAM_MAX_SURVEY_MAPS + 4) * sizeof(int);
constexpr size_t kViewMapTableBytes = (size_t)DSLAM_MAX_SURVEY_MAPS * sizeof(ViewSurveyMap);
constexpr size_t kViewTableBytes = (size_t)DSLAM_MAX_SURVEY_VIEWS * 28 * sizeof(float);
constexpr size_t kViewResultInts = (size_t)DSLAM_MAX_SURVEY_MAPS * (1 + 3 * DSLAM_MAX_SURVEY_VIEWS);
static_assert(kStartTableBytes % 16 == 0 && sizeof(ViewSurveyMap) == 80, "table layout");

int ensure_view_survey_scratch(dslam_engine *e) {
  if (e->view_survey.tables) return DSLAM_OK;
  ViewSurveyScratch s;   // (the engine gets the four together or none)
  DSLAM_TRY(s.tables_host.alloc(kStartTableBytes + kViewMapTableBytes + kViewTableBytes));
  DSLAM_TRY(s.tables.alloc(kStartTableBytes + kViewMapTableBytes + kViewTableBytes));
  DSLAM_TRY(s.results.alloc(kViewResultInts));
  DSLAM_TRY(s.results_host.alloc(kViewResultInts));
  e->view_survey = std::move(s);
  return DSLAM_OK;
}

}  // namespace

// everything already checked by dslam_survey_views; planes: [V][28]; the outputs are written only when everything has succeeded
int launch_survey_views(dslam_engine *e, const dslam_scene *const *scenes, const float *T_in, int num_maps, const float *planes,
                        int num_views, float rho, int32_t *live_out, int32_t *reach_out, int32_t *nearest_out,
                        int32_t *farthest_out) {
  const int n = num_maps, nv = num_views;
  DSLAM_TRY(ensure_view_survey_scratch(e));
  ViewSurveyScratch &sc = e->view_survey;
  // ---- the tables ----
  char *host = static_cast<char *>(sc.tables_host.get());
  int *tile_start = reinterpret_cast<int *>(host);
  ViewSurveyMap *maps = reinterpret_cast<ViewSurveyMap *>(host + kStartTableBytes);
  float *views = reinterpret_cast<float *>(host + kStartTableBytes + kViewMapTableBytes);
  const double vs = (double)scenes[0]->p.voxel_size;
  long long tiles = 0;
  for (int i = 0; i < n; i++) {
    const dslam_scene *s = scenes[i];
    ViewSurveyMap &m = maps[i];
    memset(&m, 0, sizeof m);
    m.hash = s->hash;
    m.bits = s->alloc_bits;
    m.n_entries = s->n_entries;
    m.identity = is_identity16(T_in + 16 * i) ? 1 : 0;
    double T[12], Y[12];
    voxel_pose(T_in + 16 * i, vs, T);
    rigid_inverse(T, Y);
    for (int k = 0; k < 12; k++) m.Y[k] = (float)Y[k];
    tile_start[i] = (int)tiles;
    tiles += (s->n_entries + kViewTileEntries - 1) / kViewTileEntries;
    DSLAM_REQUIRE(tiles <= 0x7fffffffLL, "the maps' hash tables together exceed the view survey's 31-bit tile index");
  }
  tile_start[n] = (int)tiles;
  memcpy(views, planes, (size_t)nv * 28 * sizeof(float));
  // from the first copy on the page-locked tables are in flight: a failure waits for the stream before it returns, so the
  // next call never rewrites them under a copy
  const size_t result_ints = (size_t)n * (1 + 3 * nv);
  auto enqueue_and_wait = [&]() -> int {
    DSLAM_HIP(hipMemcpyAsync(sc.tables.get(), host, kStartTableBytes + kViewMapTableBytes + (size_t)nv * 28 * sizeof(float),
                             hipMemcpyHostToDevice, e->stream));
    DSLAM_HIP(hipMemsetAsync(sc.results.get(), 0, result_ints * sizeof(int), e->stream));
    const char *dev = static_cast<const char *>(sc.tables.get());
    ViewSurveyParams kp;
    memset(&kp, 0, sizeof kp);
    kp.tile_start = reinterpret_cast<const int *>(dev);
    kp.maps = reinterpret_cast<const ViewSurveyMap *>(dev + kStartTableBytes);
    kp.views = reinterpret_cast<const float *>(dev + kStartTableBytes + kViewMapTableBytes);
    kp.num_maps = n; kp.num_views = nv; kp.total_tiles = (int)tiles;
    kp.rho = rho;
    kp.live = sc.results.get();
    kp.reach = kp.live + n;
    kp.nearest = reinterpret_cast<unsigned *>(kp.reach + (size_t)nv * n);
    kp.farthest = kp.nearest + (size_t)nv * n;
    hipLaunchKernelGGL(k_survey_views, dim3(kViewGrid), dim3(kViewThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    e->view_survey_launches++;
    DSLAM_HIP(hipMemcpyAsync(sc.results_host.get(), sc.results.get(), result_ints * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));   // (which also lets the next call rewrite the page-locked tables)
    return DSLAM_OK;
  };
  if (const int rc = enqueue_and_wait()) {
    (void)hipStreamSynchronize(e->stream);
    return rc;
  }
  DSLAM_TRY(device_errors(e));

  const int *res = sc.results_host.get();
  const int *reach = res + n;
  const unsigned *nearest = reinterpret_cast<const unsigned *>(reach + (size_t)nv * n), *farthest = nearest + (size_t)nv * n;
  for (int i = 0; i < n; i++) live_out[i] = res[i];
  for (int k = 0; k < nv * n; k++) {
    reach_out[k] = reach[k];
    if (nearest_out) nearest_out[k] = reach[k] > 0 ? (int32_t)(~nearest[k] ^ 0x80000000u) : INT32_MAX;
    if (farthest_out) farthest_out[k] = reach[k] > 0 ? (int32_t)(farthest[k] ^ 0x80000000u) : INT32_MIN;
  }
  return DSLAM_OK;
}

// ---- the selection (host only) --------------------------------------------------------------------------------
void select_view_maps(const int32_t *reach, const int32_t *nearest, int num_views, int n, const dslam_view_select_params &sp,
                      int32_t *maps_out, dslam_view_select_result *result) {
  struct Cand { int index, nearest; long long sum; };
  std::vector<Cand> cands;
  for (int i = 0; i < n; i++) {
    int most = INT32_MIN, near = INT32_MAX;
    long long sum = 0;
    for (int v = 0; v < num_views; v++) {
      most = std::max(most, reach[v * n + i]);
      near = std::min(near, nearest[v * n + i]);
      sum += reach[v * n + i];
    }
    if (most >= sp.min_blocks || i == sp.always_keep) cands.push_back({i, near, sum});
  }
  std::vector<int> taken;
  if ((int)cands.size() <= sp.max_maps) {
    for (const Cand &c : cands) taken.push_back(c.index);
  } else {
    std::vector<Cand> order;
    for (const Cand &c : cands)
      if (c.index == sp.always_keep) taken.push_back(c.index); else order.push_back(c);
    std::sort(order.begin(), order.end(), [](const Cand &a, const Cand &b) {
      if (a.nearest != b.nearest) return a.nearest < b.nearest;
      if (a.sum != b.sum) return a.sum > b.sum;
      return a.index < b.index;
    });
    for (const Cand &c : order)
      if ((int)taken.size() < sp.max_maps) taken.push_back(c.index);
    std::sort(taken.begin(), taken.end());
  }
  for (size_t k = 0; k < taken.size(); k++) maps_out[k] = taken[k];
  result->reaching = (int32_t)cands.size();
  result->selected = (int32_t)taken.size();
}

}  // namespace dslam
