// distance_field.hip -- occupancy and exact distance grids over all local maps (dslam_mark_occupancy,
// dslam_distance_transform, dslam_distance_field; include/dslam_fusion.h states both laws in full).
//
// Reference: none.  The laws are this project's own and all-integer behind one float32 transform per voxel, so every
// result is held bit for bit against tests/ref_distance_field.py.
//
// k_df_mark     one launch for all listed maps: the launch grid runs over the concatenated live lists (fill_live_lists),
//               one workgroup of 512 lanes per resident block, one voxel per lane; a map's first workgroup is in its
//               descriptor, so a workgroup finds (map, entry) with a scan of at most 64 scalar reads.  A block whose
//               transformed bounding box misses the grid returns before it loads a voxel; a lane whose voxel lands
//               outside the grid does not load it either.  Only the low voxel word is read.  The states are packed 2
//               bits per cell, 16 cells along x per 32-bit word, zeroed per call and written with atomicOr of non-zero
//               contributions -- and only where the word does not hold the bits yet (bits are only ever set during the
//               launch, so a stale read costs an atomic and never a bit).  The OR makes the result independent of any order.
// k_df_pass_x   packed states -> int32 squared line distances along x: per line a bitmask of its seed cells in LDS (at
//               most 16 x 64 bits), per cell the nearest set bit on either side by count-leading / count-trailing zeros.
// k_df_pass_line  the y and the z pass: out[j] = min_i f[i] + (i - j)^2 along the axis.  A workgroup takes 32 columns
//               along x and the whole line along the axis into LDS (32 x n x 4 bytes: 128 KiB at n = 1024; instantiated
//               for n <= 64, 256, 1024 so a small grid leaves room for more workgroups per CU); lanes run along x, so
//               every global access is a row of 32 consecutive ints.  Per cell the search walks outwards from j and stops
//               where d^2 reaches the best so far, and at max_cells.  A column without a finite value is not searched.
//               The passes work in place (a workgroup has read its whole tile before it writes).  The last pass applies
//               max_cells, converts to the output format and, where asked, expands the packed states to bytes.
// k_df_pack / k_df_expand  state bytes <-> packed states, for the transform alone and the marking alone.
// No kernel uses scratch memory; no workgroup waits for another.
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "dslam_internal.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {

constexpr int kDfInf = 0x40000000;          // no seed on the line; kDfInf + 1023^2 stays below 2^31
constexpr float kDfMaxCoord = 1048576.0f;   // 2^20 voxels
constexpr int kDfTileX = 32;                // columns of a line-pass tile
constexpr int kDfTileRows = 256 / kDfTileX;

struct DfGrid {
  int ox, oy, oz, cell;
  int d0, d1, d2;
  int wx;                    // words of packed states per x line: ceil(d0 / 16)
};

// one map of a marking call
struct DfMap {
  const HashEntry *hash;
  const uint2 *voxels;
  float B[12];               // map voxels -> world voxels: float32(rigid_inverse(voxel_pose(T)))
  int list_offset;           // its resident entries: live_list[list_offset .. )
  int first_block;           // the first workgroup that walks it
  int num_local_blocks;
  int pad;
};
static_assert(sizeof(DfMap) == 80, "table layout");

struct DfMarkParams {
  const DfMap *maps;
  const int *live_list;
  int num_maps, min_weight, thr;
  DfGrid g;
  unsigned *packed;
};

__device__ __forceinline__ float df_row(const float *B, int r, float x, float y, float z) {
  return ((B[4 * r] * x + B[4 * r + 1] * y) + B[4 * r + 2] * z) + B[4 * r + 3];
}

__device__ __forceinline__ int df_floor_div(int a, int b) {   // b > 0
  const int q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(512) void k_df_mark(DfMarkParams p) {
  // (map, entry) of this workgroup: the last map whose first workgroup is not behind it (a map without a block shares its
  // first workgroup with the next one)
  int mi = 0;
  for (int i = 1; i < p.num_maps; i++)
    if (p.maps[i].first_block <= (int)blockIdx.x) mi = i;
  const DfMap &m = p.maps[mi];
  const HashEntry he = load_entry(m.hash, p.live_list[m.list_offset + ((int)blockIdx.x - m.first_block)]);
  // (a live entry holds a block; a table that was uploaded may say anything)
  if (he.ptr < 0 || he.ptr >= m.num_local_blocks) return;
  const DfGrid &g = p.g;
  const float bx = (float)(he.pos[0] * kBlock), by = (float)(he.pos[1] * kBlock), bz = (float)(he.pos[2] * kBlock);
  // The block's bounding box in the world: its 8 corners, as float32 gives them.  Every voxel of the block lies within
  // the corners' exact box, and a float32 row is less than 0.25 off the exact one while |w| <= 2^21 (three products of
  // at most 2^18 and three sums), so 2 voxels of margin hold every lane's w.  Corners beyond 2^21, or not finite, decide nothing.
  {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool sane = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const float cx = bx + ((k & 1) ? 7.0f : 0.0f), cy = by + ((k & 2) ? 7.0f : 0.0f), cz = bz + ((k & 4) ? 7.0f : 0.0f);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float w = df_row(m.B, r, cx, cy, cz);
        sane = sane && fabsf(w) <= 2.0f * kDfMaxCoord;
        lo[r] = fminf(lo[r], w);
        hi[r] = fmaxf(hi[r], w);
      }
    }
    if (sane) {
      const int o[3] = {g.ox, g.oy, g.oz}, d[3] = {g.d0, g.d1, g.d2};
      bool miss = false;
#pragma unroll
      for (int r = 0; r < 3; r++)
        miss = miss || (int)floorf(hi[r]) + 2 < o[r] || (int)floorf(lo[r]) - 2 >= o[r] + g.cell * d[r];
      if (miss) return;
    }
  }
  const int t = threadIdx.x;
  const float px = bx + (float)(t & 7), py = by + (float)((t >> 3) & 7), pz = bz + (float)(t >> 6);
  const float wx = df_row(m.B, 0, px, py, pz), wy = df_row(m.B, 1, px, py, pz), wz = df_row(m.B, 2, px, py, pz);
  // (false for a NaN)
  if (!(fabsf(wx) <= kDfMaxCoord && fabsf(wy) <= kDfMaxCoord && fabsf(wz) <= kDfMaxCoord)) return;
  const int cx = df_floor_div((int)floorf(wx) - g.ox, g.cell), cy = df_floor_div((int)floorf(wy) - g.oy, g.cell),
            cz = df_floor_div((int)floorf(wz) - g.oz, g.cell);
  if ((unsigned)cx >= (unsigned)g.d0 || (unsigned)cy >= (unsigned)g.d1 || (unsigned)cz >= (unsigned)g.d2) return;
  const unsigned low = m.voxels[(size_t)he.ptr * kBlock3 + t].x;
  if ((int)((low >> 16) & 0xffu) < p.min_weight) return;
  const unsigned state = (int)(short)(low & 0xffffu) <= p.thr ? 3u : 1u;
  const unsigned bits = state << (2 * (cx & 15));
  unsigned *word = p.packed + ((size_t)(cx >> 4) + (size_t)g.wx * ((size_t)cy + (size_t)g.d1 * (size_t)cz));
  if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(word, bits);
}

// ---- state bytes <-> packed states ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_df_pack(DfGrid g, const unsigned char *__restrict__ states, unsigned *__restrict__ packed,
                                                 size_t words) {
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= words) return;
  const size_t line = w / (size_t)g.wx;
  const int x0 = (int)(w - line * (size_t)g.wx) * 16;
  const unsigned char *src = states + line * (size_t)g.d0;
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 16; k++)
    if (x0 + k < g.d0) v |= ((unsigned)src[x0 + k] & 3u) << (2 * k);
  packed[w] = v;
}

__device__ __forceinline__ unsigned df_state_of(const DfGrid &g, const unsigned *packed, int x, size_t line) {
  return (packed[line * (size_t)g.wx + (size_t)(x >> 4)] >> (2 * (x & 15))) & 3u;
}

__global__ __launch_bounds__(256) void k_df_expand(DfGrid g, const unsigned *__restrict__ packed, unsigned char *__restrict__ states,
                                                   size_t cells) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const size_t line = c / (size_t)g.d0;
  states[c] = (unsigned char)df_state_of(g, packed, (int)(c - line * (size_t)g.d0), line);
}

// ---- the x pass -----------------------------------------------------------------------------------------------------
// the seed cells of one packed word as 16 bits
__device__ __forceinline__ unsigned df_seed16(unsigned v, int seeds) {
  unsigned s = 0;
  if (seeds & DSLAM_SEED_OCCUPIED) s |= (v >> 1) & 0x55555555u;
  if (seeds & DSLAM_SEED_UNKNOWN) s |= ~(v | (v >> 1)) & 0x55555555u;
  s = (s | (s >> 1)) & 0x33333333u;
  s = (s | (s >> 2)) & 0x0f0f0f0fu;
  s = (s | (s >> 4)) & 0x00ff00ffu;
  return (s | (s >> 8)) & 0xffffu;
}

// blockDim = (lx, 256 / lx), lx = min(256, d0 rounded up to 64): 256 / lx lines per workgroup
__global__ __launch_bounds__(256) void k_df_pass_x(DfGrid g, const unsigned *__restrict__ packed, int *__restrict__ lines, int seeds,
                                                   size_t num_lines) {
  __shared__ unsigned long long s_mask[4][16];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const size_t line = (size_t)blockIdx.x * blockDim.y + ty;
  const bool live = line < num_lines;
  if (tx < 16) {
    unsigned long long mk = 0ull;
    if (live)
      for (int q = 0; q < 4; q++) {
        const int wi = tx * 4 + q;
        if (wi >= g.wx) break;
        unsigned s = df_seed16(packed[line * (size_t)g.wx + wi], seeds);
        const int left = g.d0 - wi * 16;   // cells of this word inside the line (the rest of the word is not a cell)
        if (left < 16) s &= (1u << left) - 1u;
        mk |= (unsigned long long)s << (16 * q);
      }
    s_mask[ty][tx] = mk;
  }
  __syncthreads();
  if (!live) return;
  const unsigned long long *mk = s_mask[ty];
  const int nwords = (g.d0 + 63) >> 6;
  for (int x = tx; x < g.d0; x += blockDim.x) {
    const int wi = x >> 6, b = x & 63;
    int best = 1 << 20;
    const unsigned long long r = mk[wi] >> b;
    if (r) {
      best = __builtin_ctzll(r);
    } else {
      for (int k = wi + 1; k < nwords; k++)
        if (mk[k]) { best = (k << 6) + __builtin_ctzll(mk[k]) - x; break; }
    }
    const unsigned long long l = mk[wi] << (63 - b);
    if (l) {
      best = min(best, __builtin_clzll(l));
    } else {
      for (int k = wi - 1; k >= 0; k--)
        if (mk[k]) { best = min(best, x - ((k << 6) + 63 - __builtin_clzll(mk[k]))); break; }
    }
    lines[line * (size_t)g.d0 + x] = best >= (1 << 20) ? kDfInf : best * best;
  }
}

// ---- the y and the z pass -------------------------------------------------------------------------------------------
struct DfLineParams {
  DfGrid g;
  int *lines;
  int n;                     // cells along the axis
  size_t stride;             // elements between neighbours along the axis
  size_t other_stride;       // ... and between the lines of blockIdx.y
  int rmax;                  // the walk's bound: max_cells, or 2^30
  // the last pass only
  int r2;                    // max_cells^2, 0: no bound
  int format;
  float scale;               // (float)cell * voxel_size
  const unsigned *packed;
  unsigned char *states_out; // or null
  void *dist_out;
};

template <int NMAX, bool LAST>
__global__ __launch_bounds__(256) void k_df_pass_line(DfLineParams p) {
  __shared__ int s_f[NMAX * kDfTileX];
  __shared__ int s_colmin[kDfTileX];
  const int tx = threadIdx.x & (kDfTileX - 1), ty = threadIdx.x / kDfTileX;
  const int x = blockIdx.x * kDfTileX + tx;
  const bool in = x < p.g.d0;
  const size_t base = (size_t)blockIdx.y * p.other_stride + (size_t)x;
  const int n = p.n;
  if (threadIdx.x < kDfTileX) s_colmin[threadIdx.x] = kDfInf;
  __syncthreads();
  int mn = kDfInf;
  for (int i = ty; i < n; i += kDfTileRows) {
    const int v = in ? p.lines[base + (size_t)i * p.stride] : kDfInf;
    s_f[i * kDfTileX + tx] = v;
    mn = min(mn, v);
  }
  if (mn < kDfInf) atomicMin(&s_colmin[tx], mn);
  __syncthreads();
  if (!in) return;
  const bool any = s_colmin[tx] < kDfInf;
  for (int j = ty; j < n; j += kDfTileRows) {
    int best = s_f[j * kDfTileX + tx];
    if (any) {
      // outwards from j: a cell d away adds d^2, so nothing beyond d^2 >= best can win, and nothing beyond max_cells counts
      for (int d = 1; d <= p.rmax; d++) {
        const int dd = d * d, a = j - d, b = j + d;
        if (dd >= best || (a < 0 && b >= n)) break;
        if (a >= 0) best = min(best, s_f[a * kDfTileX + tx] + dd);
        if (b < n) best = min(best, s_f[b * kDfTileX + tx] + dd);
      }
      best = min(best, kDfInf);
    }
    const size_t at = base + (size_t)j * p.stride;
    if (!LAST) {
      p.lines[at] = best;
    } else {
      const bool far = best >= kDfInf || (p.r2 > 0 && best > p.r2);
      if (p.dist_out) {
        if (p.format == DSLAM_DIST_METRES)
          static_cast<float *>(p.dist_out)[at] = far ? INFINITY : sqrtf((float)best) * p.scale;
        else
          static_cast<int *>(p.dist_out)[at] = far ? DSLAM_DIST_FAR : best;
      }
      // (the last pass runs along z: blockIdx.y is y)
      if (p.states_out)
        p.states_out[at] = (unsigned char)df_state_of(p.g, p.packed, x, (size_t)blockIdx.y + (size_t)p.g.d1 * (size_t)j);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
bool grid_ok(const dslam_grid &g) {
  if (g.pad != 0 || g.cell < 1 || g.cell > DSLAM_GRID_MAX_CELL) return false;
  long long cells = 1;
  for (int a = 0; a < 3; a++) {
    if (g.dims[a] < 1 || g.dims[a] > DSLAM_GRID_MAX_DIM) return false;
    if (g.origin[a] < -(1 << 20) || (long long)g.origin[a] + (long long)g.cell * g.dims[a] > (1 << 20)) return false;
    cells *= g.dims[a];
  }
  return cells <= DSLAM_GRID_MAX_CELLS;
}

namespace {

template <bool LAST>
void launch_line_pass(hipStream_t stream, dim3 grid, const DfLineParams &lp) {
  if (lp.n <= 64) hipLaunchKernelGGL((k_df_pass_line<64, LAST>), grid, dim3(256), 0, stream, lp);
  else if (lp.n <= 256) hipLaunchKernelGGL((k_df_pass_line<256, LAST>), grid, dim3(256), 0, stream, lp);
  else hipLaunchKernelGGL((k_df_pass_line<1024, LAST>), grid, dim3(256), 0, stream, lp);
}

// a phase boundary of the bench hook (dslam_debug_distance_field_phases)
int mark_phase(dslam_engine *e, int k) {
  DistanceFieldScratch &s = e->distance_field;
  if (!s.timing) return DSLAM_OK;
  if (!s.events[k]) DSLAM_TRY(s.events[k].create(hipEventDefault));
  DSLAM_HIP(hipEventRecord(s.events[k], e->stream));
  s.recorded |= 1 << k;
  return DSLAM_OK;
}

}  // namespace

int launch_distance_field(dslam_engine *e, const DistanceFieldCall &c) {
  DistanceFieldScratch &s = e->distance_field;
  DfGrid g;
  g.ox = c.grid.origin[0]; g.oy = c.grid.origin[1]; g.oz = c.grid.origin[2]; g.cell = c.grid.cell;
  g.d0 = c.grid.dims[0]; g.d1 = c.grid.dims[1]; g.d2 = c.grid.dims[2];
  g.wx = (g.d0 + 15) / 16;
  const size_t num_lines = (size_t)g.d1 * g.d2, cells = num_lines * g.d0, words = num_lines * g.wx;
  const bool want_dist = c.transform && c.dist_out;

  // ---- the buffers (a buffer that grows is freed first, which waits for the device) ----
  if (s.packed_words < words) {
    DSLAM_TRY(s.packed.alloc(words));
    s.packed_words = words;
  }
  if (want_dist && s.lines_cells < cells) {
    DSLAM_TRY(s.lines.alloc(cells));
    s.lines_cells = cells;
  }
  if (c.host && (c.states_out || c.states_in) && s.bytes_cells < cells) {
    DSLAM_TRY(s.bytes.alloc(cells));
    s.bytes_cells = cells;
  }
  s.recorded = 0;

  // ---- the packed states: marked from the maps, or packed from the caller's bytes ----
  if (c.scenes) {
    const int n = c.num_maps;
    std::vector<int> all(n), list_offset, live;
    std::iota(all.begin(), all.end(), 0);
    DSLAM_TRY(fill_live_lists(e, c.scenes, n, all, list_offset, live));
    if (!s.maps) DSLAM_TRY(s.maps.alloc((size_t)DSLAM_MAX_RENDER_MAPS * sizeof(DfMap)));
    DfMap maps[DSLAM_MAX_RENDER_MAPS];
    const double vs = (double)c.scenes[0]->p.voxel_size;
    long long total = 0;
    for (int i = 0; i < n; i++) {
      const dslam_scene *sc = c.scenes[i];
      DfMap &m = maps[i];
      memset(&m, 0, sizeof m);
      m.hash = sc->hash; m.voxels = sc->voxels;
      double Tv[12], Bv[12];
      voxel_pose(c.T + 16 * i, vs, Tv);
      rigid_inverse(Tv, Bv);
      for (int k = 0; k < 12; k++) m.B[k] = (float)Bv[k];
      m.list_offset = list_offset[i];
      m.first_block = (int)total;
      m.num_local_blocks = sc->p.num_local_blocks;
      total += live[i];
    }
    DSLAM_REQUIRE(total <= 0x7fffffffLL, "the maps' resident blocks together exceed the marking launch's grid");
    DSLAM_TRY(mark_phase(e, 0));
    DSLAM_HIP(hipMemsetAsync(s.packed.get(), 0, words * sizeof(unsigned), e->stream));
    if (total > 0) {
      DSLAM_HIP(hipMemcpyAsync(s.maps.get(), maps, (size_t)n * sizeof(DfMap), hipMemcpyHostToDevice, e->stream));
      DfMarkParams mp;
      mp.maps = static_cast<const DfMap *>(s.maps.get());
      mp.live_list = e->live_lists.live_list;
      mp.num_maps = n; mp.min_weight = c.min_weight; mp.thr = c.thr;
      mp.g = g;
      mp.packed = s.packed.get();
      hipLaunchKernelGGL(k_df_mark, dim3((unsigned)total), dim3(512), 0, e->stream, mp);
      DSLAM_HIP(hipGetLastError());
    }
  } else {
    const unsigned char *src = static_cast<const unsigned char *>(c.states_in);
    DSLAM_TRY(mark_phase(e, 0));
    if (c.host) {
      DSLAM_HIP(hipMemcpyAsync(s.bytes.get(), c.states_in, cells, hipMemcpyHostToDevice, e->stream));
      src = s.bytes.get();
    }
    hipLaunchKernelGGL(k_df_pack, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, e->stream, g, src, s.packed.get(), words);
    DSLAM_HIP(hipGetLastError());
  }
  DSLAM_TRY(mark_phase(e, 1));

  unsigned char *states_dev = c.states_out ? (c.host ? s.bytes.get() : static_cast<unsigned char *>(c.states_out)) : nullptr;
  if (!want_dist) {
    // the states alone
    hipLaunchKernelGGL(k_df_expand, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, g, s.packed.get(), states_dev, cells);
    DSLAM_HIP(hipGetLastError());
  } else {
    const int lx = std::min(256, (g.d0 + 63) / 64 * 64), ly = 256 / lx;
    hipLaunchKernelGGL(k_df_pass_x, dim3((unsigned)((num_lines + ly - 1) / ly)), dim3(lx, ly), 0, e->stream, g, s.packed.get(),
                       s.lines.get(), c.seeds, num_lines);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(mark_phase(e, 2));
    DfLineParams lp;
    memset(&lp, 0, sizeof lp);
    lp.g = g;
    lp.lines = s.lines.get();
    lp.rmax = c.max_cells > 0 ? c.max_cells : (1 << 30);
    const unsigned tiles = (unsigned)((g.d0 + kDfTileX - 1) / kDfTileX);
    // y: one workgroup per (x tile, z)
    lp.n = g.d1; lp.stride = (size_t)g.d0; lp.other_stride = (size_t)g.d0 * g.d1;
    launch_line_pass<false>(e->stream, dim3(tiles, (unsigned)g.d2), lp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(mark_phase(e, 3));
    // z, the last: one workgroup per (x tile, y)
    lp.n = g.d2; lp.stride = (size_t)g.d0 * g.d1; lp.other_stride = (size_t)g.d0;
    lp.r2 = c.max_cells * c.max_cells;
    lp.format = c.format;
    lp.scale = (float)g.cell * c.voxel_size;
    lp.packed = s.packed.get();
    lp.states_out = states_dev;
    lp.dist_out = c.host ? static_cast<void *>(s.lines.get()) : c.dist_out;
    launch_line_pass<true>(e->stream, dim3(tiles, (unsigned)g.d1), lp);
    DSLAM_HIP(hipGetLastError());
  }
  DSLAM_TRY(mark_phase(e, 4));
  if (c.host) {
    if (c.states_out) DSLAM_HIP(hipMemcpyAsync(c.states_out, s.bytes.get(), cells, hipMemcpyDeviceToHost, e->stream));
    if (want_dist) DSLAM_HIP(hipMemcpyAsync(c.dist_out, s.lines.get(), cells * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  }
  return DSLAM_OK;
}

// bench hook: enable >= 0 switches the phase events on or off; ms_out [4] (or NULL): the last call's phases -- the states
// (memset and marking, or packing), the x pass, the y pass, the last pass (or the expansion); -1 where a phase did not run
int distance_field_phases(dslam_engine *e, int enable, float *ms_out) {
  DistanceFieldScratch &s = e->distance_field;
  if (ms_out) {
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    // the boundaries recorded, in order: 0, 1, [2, 3,] 4
    for (int k = 0; k < 4; k++) ms_out[k] = -1.0f;
    auto span = [&](int a, int b, float *out) {
      if ((s.recorded >> a & 1) && (s.recorded >> b & 1)) return hipEventElapsedTime(out, s.events[a], s.events[b]);
      return hipSuccess;
    };
    DSLAM_HIP(span(0, 1, &ms_out[0]));
    if (s.recorded >> 2 & 1) {
      DSLAM_HIP(span(1, 2, &ms_out[1]));
      DSLAM_HIP(span(2, 3, &ms_out[2]));
      DSLAM_HIP(span(3, 4, &ms_out[3]));
    } else {
      DSLAM_HIP(span(1, 4, &ms_out[3]));
    }
  }
  if (enable >= 0) s.timing = enable != 0;
  return DSLAM_OK;
}

}  // namespace dslam
