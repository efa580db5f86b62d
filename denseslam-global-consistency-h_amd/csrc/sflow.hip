// sflow.hip -- sparse stereo scene-flow matching on the device (dslam_sflow_*; include/dslam_fusion.h
// states the law in full).
//
// Reference: libviso2's Matcher (first matching pass: getRawMatches()).  The law is all-integer, so every result is held bit
// for bit against tests/ref_sflow.py and against that library's own output in tests/golden/sflow_*.npz.
//
// A push (both images of the frame in every launch):
// k_sf_filter       one workgroup per 64 x 16 tile of the matching image: the grey tile and a halo of 2 staged once in LDS
//                   (the 2 x 2 mean of half_resolution and the grey of RGBA formed in the load), ONE column pass into five
//                   LDS planes, then the row passes: du, dv, f1, f2 from that one staging.
// k_sf_nms          one lane per cell, both sets: the four extrema of the cell, their neighbourhood checks, the threshold.
// k_sf_scan         one workgroup per list: the exclusive scan that makes the compaction ORDERED (cell order, then class).
// k_sf_emit         one lane per cell: the whole 48-byte record of each accepted extremum, descriptor gather included,
//                   and one atomic add on the record's bin.
// k_sf_scan         the bin starts.
// k_sf_bin_scatter  one lane per feature into its bin.  The order inside a bin is whatever the atomics give: an entry
//                   carries (u_bin VB + v_bin) << 32 | index, and that, below the cost, IS the reference's traversal
//                   order, so the winner does not depend on the order in which candidates are met.
// A match:
// k_sf_match<M>     one wave64 per driving feature (grid-stride).  The legs run in sequence and are wave-uniform; the
//                   query's record is read through a uniform index (scalar loads).  Per bin row the bins u_min .. u_max are
//                   one contiguous run of the list; the lanes stride over it, 8 v_sad_u8 per candidate, each lane keeps
//                   the minimum of cost << 46 | entry, one butterfly gives the winner.
// k_sf_pixel        methods 0 and 1: of the kept features on one pixel the first stays.  Features on one pixel come from
//                   one cell, so they are at most 3 apart in index: a look at three predecessors.
// k_sf_scan, k_sf_compact   the kept records in driving order, the count.
// No kernel uses scratch memory; no workgroup waits for another; no float anywhere.
#include <cstring>

#include "dslam_internal.h"

#pragma clang fp contract(off)

namespace dslam {

namespace {

constexpr int kTileW = 64, kTileH = 16, kHalo = 2;
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;
constexpr int kScanThreads = 1024;
constexpr int kMatchBlocks = 2048;                       // x 4 waves, grid-stride over the driving features
constexpr unsigned long long kNoKey = ~0ull;
// a key is cost << 46 | (u_bin VB + v_bin) << 32 | index: the index is the low word, the bin's place in the walk 14 bits
static_assert(DSLAM_SFLOW_MAX_BINS / 4 <= (1 << 14) && DSLAM_SFLOW_MAX_COST < (1 << 13), "bin ordinal in 14 bits, cost in 13");

struct FilterParams {
  const unsigned char *img[2];
  unsigned char *sobel;      // [side][du, dv][mh mw]
  short *corner;             // [side][f1, f2][mh mw]
  int W, channels, half, mw, mh;
};

struct NmsParams {
  const short *corner;
  const unsigned char *sobel;
  int4 *cell_feat;
  int *cell_count;
  const int *cell_offset;
  int4 *feats[4];            // [side * 2 + set]
  int *bin_fill[4];
  int mw, mh, tau, s, binsize, ub, vb, stride;   // stride: cells of the dense set
  int n[2], cx[2], cy[2];
};

struct ScanList {
  const int *in;
  int *out;
  const int *n_dev;          // NULL: n as given; otherwise min(*n_dev, n)
  int *total;                // or NULL
  int n, tail;               // tail: out[n] = total as well
};
struct ScanParams { ScanList l[8]; };

struct BinParams {
  const int4 *feats[4];
  const int *count[4];
  int *bin_fill[4];
  const int *bin_start[4];
  unsigned long long *bin_list[4];
  int cap[4];
  int binsize, ub, vb;
};

struct MatchParams {
  const int4 *feat[4];       // by DSLAM_SFLOW_IMAGE_*
  const int *count[4], *dense_count[4];
  const int *bin_start[4];
  const unsigned long long *bin_list[4];
  int4 *stage;
  int *flags;
  int cap, binsize, ub, vb, radius, vtol;
};

__device__ __forceinline__ int sf_grey(const unsigned char *img, int channels, size_t pix) {
  if (channels == 1) return img[pix];
  const uchar4 c = reinterpret_cast<const uchar4 *>(img)[pix];
  return (c.x + 2 * c.y + c.z) >> 2;
}

__device__ __forceinline__ int sf_sat8(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void k_sf_filter(FilterParams p) {
  __shared__ short g[kLdsH][kLdsW];
  __shared__ short col[5][kTileH][kLdsW];   // (1,4,6,4,1) (1,2,0,-2,-1) (1,1,1,1,1) (0,1,1,1,0) (1,1,0,-1,-1) down the column
  const int side = blockIdx.z, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const unsigned char *img = p.img[side];
  for (int k = threadIdx.x; k < kLdsW * kLdsH; k += 256) {
    const int lx = k % kLdsW, ly = k / kLdsW, x = x0 - kHalo + lx, y = y0 - kHalo + ly;
    int v = 0;
    if (x >= 0 && x < p.mw && y >= 0 && y < p.mh) {
      if (p.half) {
        const size_t at = (size_t)(2 * y) * p.W + 2 * x;   // (2 x + 1 < W, 2 y + 1 < H: mw = W / 2, mh = H / 2)
        v = (sf_grey(img, p.channels, at) + sf_grey(img, p.channels, at + 1) + sf_grey(img, p.channels, at + p.W) +
             sf_grey(img, p.channels, at + p.W + 1)) >> 2;
      } else {
        v = sf_grey(img, p.channels, (size_t)y * p.W + x);
      }
    }
    g[ly][lx] = (short)v;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kLdsW * kTileH; k += 256) {
    const int lx = k % kLdsW, r = k / kLdsW;
    const int a = g[r][lx], b = g[r + 1][lx], c = g[r + 2][lx], d = g[r + 3][lx], e = g[r + 4][lx];
    col[0][r][lx] = (short)(a + 4 * b + 6 * c + 4 * d + e);
    col[1][r][lx] = (short)(a + 2 * b - 2 * d - e);
    col[2][r][lx] = (short)(a + b + c + d + e);
    col[3][r][lx] = (short)(b + c + d);
    col[4][r][lx] = (short)(a + b - d - e);
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, x = x0 + lx;
  const size_t mn = (size_t)p.mw * p.mh;
  unsigned char *du = p.sobel + (size_t)side * 2 * mn, *dv = du + mn;
  short *f1 = p.corner + (size_t)side * 2 * mn, *f2 = f1 + mn;
  for (int r = threadIdx.x >> 6; r < kTileH; r += 4) {
    const int y = y0 + r;
    if (x >= p.mw || y >= p.mh) continue;
    int o_du = 0, o_dv = 0, o_f1 = 0, o_f2 = 0;
    if (x >= 2 && x <= p.mw - 3 && y >= 2 && y <= p.mh - 3) {
      const short *s = col[0][r] + lx, *d = col[1][r] + lx, *b5 = col[2][r] + lx, *b3 = col[3][r] + lx, *c = col[4][r] + lx;
      o_du = sf_sat8(((s[0] + 2 * s[1] - 2 * s[3] - s[4]) >> 7) + 128);
      o_dv = sf_sat8(((d[0] + 4 * d[1] + 6 * d[2] + 4 * d[3] + d[4]) >> 7) + 128);
      o_f1 = -(b5[0] + b5[1] + b5[2] + b5[3] + b5[4]) + 2 * (b3[1] + b3[2] + b3[3]) + 7 * g[r + 2][lx + 2];
      o_f2 = c[0] + c[1] - c[3] - c[4];
    }
    const size_t at = (size_t)y * p.mw + x;
    du[at] = (unsigned char)o_du; dv[at] = (unsigned char)o_dv;
    f1[at] = (short)o_f1; f2[at] = (short)o_f2;
  }
}

// is the extremum at (u, v) beaten inside its neighbourhood?  sign = -1 for a minimum
__device__ __forceinline__ bool sf_beaten(const short *F, int mw, int mh, int n, int u, int v, int val, int sign) {
  const int x1 = min(u + n, mw - 1 - DSLAM_SFLOW_MARGIN), y1 = min(v + n, mh - 1 - DSLAM_SFLOW_MARGIN);
  bool beaten = false;
  for (int y = v - n; y <= y1; y++)
    for (int x = u - n; x <= x1; x++) beaten |= sign * F[(size_t)y * mw + x] > val;
  return beaten;
}

__global__ __launch_bounds__(256) void k_sf_nms(NmsParams p) {
  const int side = blockIdx.y >> 1, set = blockIdx.y & 1, cell = blockIdx.x * 256 + threadIdx.x;
  const int n = p.n[set], cy = p.cy[set];
  if (cell >= p.cx[set] * cy) return;
  const int i = n + DSLAM_SFLOW_MARGIN + (cell / cy) * (n + 1), j = n + DSLAM_SFLOW_MARGIN + (cell % cy) * (n + 1);
  const size_t mn = (size_t)p.mw * p.mh;
  int feat[4], count = 0;
  for (int f = 0; f < 2; f++) {
    const short *F = p.corner + ((size_t)side * 2 + f) * mn;
    int lo = F[(size_t)j * p.mw + i], hi = lo, lo_at = i | j << 16, hi_at = lo_at;
    for (int x = i; x <= i + n; x++)
      for (int y = j; y <= j + n; y++) {
        const int v = F[(size_t)y * p.mw + x];
        if (v < lo) { lo = v; lo_at = x | y << 16; }
        if (v > hi) { hi = v; hi_at = x | y << 16; }
      }
    const bool lo_ok = lo <= -p.tau && !sf_beaten(F, p.mw, p.mh, n, lo_at & 0xffff, lo_at >> 16, -lo, -1);
    const bool hi_ok = hi >= p.tau && !sf_beaten(F, p.mw, p.mh, n, hi_at & 0xffff, hi_at >> 16, hi, 1);
    feat[2 * f] = lo_ok ? lo_at : -1;
    feat[2 * f + 1] = hi_ok ? hi_at : -1;
    count += (int)lo_ok + (int)hi_ok;
  }
  const size_t at = (size_t)blockIdx.y * p.stride + cell;
  p.cell_feat[at] = make_int4(feat[0], feat[1], feat[2], feat[3]);
  p.cell_count[at] = count;
}

// exclusive scan of one list per workgroup: every thread sums a contiguous chunk, the chunk sums are scanned across the
// workgroup, every thread writes its chunk
__global__ __launch_bounds__(kScanThreads) void k_sf_scan(ScanParams p) {
  __shared__ int wave_sum[kScanThreads / 64];
  const ScanList L = p.l[blockIdx.x];
  int n = L.n;
  if (L.n_dev) n = min(max(*L.n_dev, 0), n);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int chunk = (n + kScanThreads - 1) / kScanThreads, first = min(t * chunk, n), last = min(first + chunk, n);
  int sum = 0;
  for (int k = first; k < last; k++) sum += L.in[k];
  int incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < kScanThreads / 64; w++) {
    const int s = wave_sum[w];
    if (w < wave) base += s;
    total += s;
  }
  int run = base + incl - sum;
  for (int k = first; k < last; k++) {
    const int v = L.in[k];
    L.out[k] = run;
    run += v;
  }
  if (t == 0) {
    if (L.tail) L.out[L.n] = total;
    if (L.total) *L.total = total;
  }
}

__device__ __forceinline__ int sf_bin_key(int u, int v, int c, int binsize, int ub, int vb, unsigned long long *entry_bins) {
  const int bu = min(u / binsize, ub - 1), bv = min(v / binsize, vb - 1);
  *entry_bins = (unsigned long long)(unsigned)(bu * vb + bv) << 32;
  return (c * vb + bv) * ub + bu;
}

__global__ __launch_bounds__(256) void k_sf_emit(NmsParams p) {
  const int side = blockIdx.y >> 1, set = blockIdx.y & 1, cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= p.cx[set] * p.cy[set]) return;
  const size_t at = (size_t)blockIdx.y * p.stride + cell, mn = (size_t)p.mw * p.mh;
  if (p.cell_count[at] == 0) return;
  const int4 f4 = p.cell_feat[at];
  const int feat[4] = {f4.x, f4.y, f4.z, f4.w};
  const unsigned char *du = p.sobel + (size_t)side * 2 * mn, *dv = du + mn;
  int4 *out = p.feats[blockIdx.y] + 3 * (size_t)p.cell_offset[at];   // (below the list's capacity: at most 4 per cell)
  for (int c = 0; c < 4; c++) {
    if (feat[c] < 0) continue;
    const int u = feat[c] & 0xffff, v = feat[c] >> 16;
    // the 16 taps (dx, dy), du then dv at each: four per dword pair
    constexpr int tx[16] = {-3, -3, -1, -1, 3, 3, 1, 1, -1, -1, 1, 1, -5, -5, 5, 5};
    constexpr int ty[16] = {-1, 1, -1, 1, -1, 1, -1, 1, -5, 5, -5, 5, -3, 3, -3, 3};
    unsigned d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const size_t a = (size_t)(v + ty[2 * k]) * p.mw + (u + tx[2 * k]), b = (size_t)(v + ty[2 * k + 1]) * p.mw + (u + tx[2 * k + 1]);
      d[k] = (unsigned)du[a] | (unsigned)dv[a] << 8 | (unsigned)du[b] << 16 | (unsigned)dv[b] << 24;
    }
    out[0] = make_int4(u * p.s, v * p.s, 0, c);
    out[1] = make_int4((int)d[0], (int)d[1], (int)d[2], (int)d[3]);
    out[2] = make_int4((int)d[4], (int)d[5], (int)d[6], (int)d[7]);
    out += 3;
    unsigned long long bins;
    atomicAdd(p.bin_fill[blockIdx.y] + sf_bin_key(u * p.s, v * p.s, c, p.binsize, p.ub, p.vb, &bins), 1);
  }
}

__global__ __launch_bounds__(256) void k_sf_bin_scatter(BinParams p) {
  const int l = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(*p.count[l], p.cap[l])) return;
  const int4 head = p.feats[l][3 * (size_t)i];
  unsigned long long bins;
  const int key = sf_bin_key(head.x, head.y, head.w, p.binsize, p.ub, p.vb, &bins);
  // (bin_fill[key] counts this bin's features, so the slots start[key] .. start[key + 1] - 1 are handed out once each)
  const int slot = p.bin_start[l][key] + atomicSub(p.bin_fill[l] + key, 1) - 1;
  p.bin_list[l][slot] = bins | (unsigned)i;
}

__device__ __forceinline__ int sf_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

__device__ __forceinline__ unsigned long long sf_wave_min(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned lo = __shfl_xor((int)(unsigned)v, d, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), d, 64);
    const unsigned long long o = (unsigned long long)hi << 32 | lo;
    v = o < v ? o : v;
  }
  return v;
}

// The partner in image `t` of feature `qi` (wave-uniform) of image `q`; every lane returns the same index.
__device__ __forceinline__ int sf_find(const MatchParams &p, int q, int qi, int t, bool flow, int lane) {
  const int4 *rec = p.feat[q] + 3 * (size_t)qi;
  const int4 head = rec[0], qa = rec[1], qb = rec[2];
  const int rv = flow ? p.radius : p.vtol;
  const int u0 = head.x - p.radius, u1 = head.x + p.radius, v0 = head.y - rv, v1 = head.y + rv;
  const int bu0 = min(max(sf_floor_div(u0, p.binsize), 0), p.ub - 1), bu1 = min(max(sf_floor_div(u1, p.binsize), 0), p.ub - 1);
  const int bv0 = min(max(sf_floor_div(v0, p.binsize), 0), p.vb - 1), bv1 = min(max(sf_floor_div(v1, p.binsize), 0), p.vb - 1);
  const int4 *feat = p.feat[t];
  const int *start = p.bin_start[t];
  const unsigned long long *list = p.bin_list[t];
  unsigned long long best = kNoKey;
  for (int bv = bv0; bv <= bv1; bv++) {
    const int row = (head.w * p.vb + bv) * p.ub;
    const int first = start[row + bu0], last = start[row + bu1 + 1];   // the bins of one row are one run of the list
    for (int k = first + lane; k < last; k += 64) {
      const unsigned long long entry = list[k];
      const int4 *c = feat + 3 * (size_t)(unsigned)entry;
      const int4 ch = c[0];
      if (ch.x < u0 || ch.x > u1 || ch.y < v0 || ch.y > v1) continue;
      const int4 ca = c[1], cb = c[2];
      unsigned cost = __builtin_amdgcn_sad_u8(qa.x, ca.x, 0u);
      cost = __builtin_amdgcn_sad_u8(qa.y, ca.y, cost);
      cost = __builtin_amdgcn_sad_u8(qa.z, ca.z, cost);
      cost = __builtin_amdgcn_sad_u8(qa.w, ca.w, cost);
      cost = __builtin_amdgcn_sad_u8(qb.x, cb.x, cost);
      cost = __builtin_amdgcn_sad_u8(qb.y, cb.y, cost);
      cost = __builtin_amdgcn_sad_u8(qb.z, cb.z, cost);
      cost = __builtin_amdgcn_sad_u8(qb.w, cb.w, cost);
      const unsigned long long key = (unsigned long long)cost << 46 | entry;
      best = key < best ? key : best;
    }
  }
  best = sf_wave_min(best);
  return __builtin_amdgcn_readfirstlane(best == kNoKey ? 0 : (int)(unsigned)best);
}

template <int M>
__global__ __launch_bounds__(256) void k_sf_match(MatchParams p) {
  constexpr int C1 = DSLAM_SFLOW_IMAGE_1C, C2 = DSLAM_SFLOW_IMAGE_2C, P1 = DSLAM_SFLOW_IMAGE_1P, P2 = DSLAM_SFLOW_IMAGE_2P;
  constexpr int drive = M == 2 ? P1 : C1;
  const int lane = threadIdx.x & 63;
  const int n = min(max(*p.count[drive], 0), p.cap);
  bool empty = false;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool need = M == 2 || i == C1 || (M == 1 && i == C2) || (M == 0 && i == P1);
    if (need) empty |= *p.count[i] <= 0 || *p.dense_count[i] <= 0;
  }
  const int waves = gridDim.x * 4;
  for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n; w += waves) {
    const int i = __builtin_amdgcn_readfirstlane(w);
    if (empty) {
      if (lane == 0) p.flags[i] = 0;
      continue;
    }
    int4 r0, r1, r2;
    bool ok;
    if (M == 2) {
      const int i2p = sf_find(p, P1, i, P2, false, lane);
      const int i2c = sf_find(p, P2, i2p, C2, true, lane);
      const int i1c = sf_find(p, C2, i2c, C1, false, lane);
      const int back = sf_find(p, C1, i1c, P1, true, lane);
      const int4 a = p.feat[P1][3 * (size_t)i], b = p.feat[P2][3 * (size_t)i2p], c = p.feat[C1][3 * (size_t)i1c],
                 d = p.feat[C2][3 * (size_t)i2c];
      ok = back == i && a.x >= b.x && c.x >= d.x;
      r0 = make_int4(a.x, a.y, i, b.x); r1 = make_int4(b.y, i2p, c.x, c.y); r2 = make_int4(i1c, d.x, d.y, i2c);
    } else {
      constexpr int other = M == 1 ? C2 : P1;
      const int io = sf_find(p, C1, i, other, M == 0, lane);
      const int back = sf_find(p, other, io, C1, M == 0, lane);
      const int4 c = p.feat[C1][3 * (size_t)i], o = p.feat[other][3 * (size_t)io];
      ok = back == i && (M == 0 || c.x >= o.x);
      if (M == 0) { r0 = make_int4(o.x, o.y, io, -1); r1 = make_int4(-1, -1, c.x, c.y); r2 = make_int4(i, -1, -1, -1); }
      else { r0 = make_int4(-1, -1, -1, -1); r1 = make_int4(-1, -1, c.x, c.y); r2 = make_int4(i, o.x, o.y, io); }
    }
    if (lane == 0) {
      p.flags[i] = ok ? 1 : 0;
      int4 *out = p.stage + 3 * (size_t)i;
      out[0] = r0; out[1] = r1; out[2] = r2;
    }
  }
}

__global__ __launch_bounds__(256) void k_sf_pixel(const int4 *feat, const int *count, int cap, const int *flags, int *keep) {
  const int n = min(max(*count, 0), cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    int k = flags[i];
    if (k) {
      const int4 me = feat[3 * (size_t)i];
      for (int d = 1; d <= 3 && d <= i; d++) {
        const int4 o = feat[3 * (size_t)(i - d)];
        if (o.x == me.x && o.y == me.y && flags[i - d]) k = 0;
      }
    }
    keep[i] = k;
  }
}

__global__ __launch_bounds__(256) void k_sf_compact(const int4 *stage, const int *count, int cap, const int *keep, const int *offset,
                                                    int4 *out, int capacity) {
  const int n = min(max(*count, 0), cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if (!keep[i]) continue;
    const int o = offset[i];
    if (o >= capacity) continue;
    const int4 *src = stage + 3 * (size_t)i;
    int4 *dst = out + 3 * (size_t)o;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  }
}

int cells_along(int size, int n) {
  const int span = size - 2 * n - 2 * DSLAM_SFLOW_MARGIN;
  return span <= 0 ? 0 : (span + n) / (n + 1);
}

int mark_phase(dslam_engine *e, dslam_sflow *sf, int k) {
  if (!sf->timing) return DSLAM_OK;
  if (!sf->events[k]) DSLAM_TRY(sf->events[k].create(hipEventDefault));
  DSLAM_HIP(hipEventRecord(sf->events[k], e->stream));
  sf->recorded |= 1 << k;
  return DSLAM_OK;
}

// where list l = (slot * 2 + side) * 2 + set lives in feats (records) and bin_list (entries)
size_t list_base(const dslam_sflow *sf, int l) { return (size_t)(l >> 1) * ((size_t)sf->cap[0] + sf->cap[1]) + ((l & 1) ? sf->cap[0] : 0); }
int bins_of(const dslam_sflow *sf) { return 4 * sf->ub * sf->vb; }

}  // namespace

int sflow_resolve_params(const dslam_sflow_params *params, int width, int height, dslam_sflow *sf) {
  dslam_sflow_params p;
  memset(&p, 0, sizeof p);
  if (params) p = *params;
  DSLAM_REQUIRE(p.pad == 0, "dslam_sflow_params: pad must be 0");
  if (p.nms_n == 0) p.nms_n = 3;
  if (p.nms_tau == 0) p.nms_tau = 50;
  if (p.match_binsize == 0) p.match_binsize = 50;
  if (p.match_radius == 0) p.match_radius = 200;
  if (p.match_disp_tolerance == 0) p.match_disp_tolerance = 2;
  if (p.half_resolution == 0) p.half_resolution = 1;
  if (p.channels == 0) p.channels = 1;
  DSLAM_REQUIRE(p.nms_n >= 1 && p.nms_n <= DSLAM_SFLOW_MAX_NMS_N, "nms_n must be 1 .. DSLAM_SFLOW_MAX_NMS_N");
  DSLAM_REQUIRE(p.nms_tau >= 1 && p.match_binsize >= 1 && p.match_radius >= 1 && p.match_disp_tolerance >= 1,
                "nms_tau, match_binsize, match_radius and match_disp_tolerance must be positive");
  DSLAM_REQUIRE(p.half_resolution == 1 || p.half_resolution == -1, "half_resolution must be 1 (on) or -1 (off)");
  DSLAM_REQUIRE(p.channels == 1 || p.channels == 4, "channels must be 1 or 4");
  const int s = p.half_resolution == 1 ? 2 : 1;
  DSLAM_REQUIRE(width >= s && width <= DSLAM_SFLOW_MAX_SIZE && height >= s && height <= DSLAM_SFLOW_MAX_SIZE,
                "width and height must be 1 (2 with half_resolution) .. DSLAM_SFLOW_MAX_SIZE");
  sf->p = p;
  sf->w = width; sf->h = height; sf->s = s; sf->mw = width / s; sf->mh = height / s;
  sf->n[0] = 3 * p.nms_n > 10 ? (p.nms_n > 10 ? p.nms_n : 10) : 3 * p.nms_n;
  sf->n[1] = p.nms_n;
  for (int k = 0; k < 2; k++) {
    sf->cx[k] = cells_along(sf->mw, sf->n[k]); sf->cy[k] = cells_along(sf->mh, sf->n[k]);
    sf->cap[k] = 4 * sf->cx[k] * sf->cy[k];
  }
  sf->tau = p.nms_tau; sf->binsize = p.match_binsize; sf->vtol = p.match_disp_tolerance; sf->channels = p.channels;
  sf->radius = s == 2 ? p.match_radius / 2 : p.match_radius;
  sf->ub = (width + p.match_binsize - 1) / p.match_binsize; sf->vb = (height + p.match_binsize - 1) / p.match_binsize;
  DSLAM_REQUIRE((long long)4 * sf->ub * sf->vb <= DSLAM_SFLOW_MAX_BINS, "more than DSLAM_SFLOW_MAX_BINS bin lists: raise match_binsize");
  DSLAM_REQUIRE(sf->cap[1] <= DSLAM_SFLOW_MAX_FEATURES && sf->cap[0] <= sf->cap[1], "more than DSLAM_SFLOW_MAX_FEATURES possible features");
  return DSLAM_OK;
}

int sflow_allocate(dslam_engine *e, dslam_sflow *sf) {
  DSLAM_HIP(hipSetDevice(e->device));
  const size_t mn = (size_t)sf->mw * sf->mh, cells = (size_t)sf->cx[1] * sf->cy[1] + 1, cap = (size_t)sf->cap[1] + 1;
  const size_t per_image = (size_t)sf->cap[0] + sf->cap[1] + 1, bins = bins_of(sf);
  SflowBuffers b;   // built aside: a failure leaves no partial handle
  DSLAM_TRY(b.images.alloc(2 * (size_t)sf->w * sf->h * sf->channels));
  DSLAM_TRY(b.sobel.alloc(4 * mn));
  DSLAM_TRY(b.corner.alloc(4 * mn));
  DSLAM_TRY(b.cell_feat.alloc(4 * cells));
  DSLAM_TRY(b.cell_count.alloc(4 * cells));
  DSLAM_TRY(b.cell_offset.alloc(4 * cells));
  DSLAM_TRY(b.feats.alloc(3 * 4 * per_image));
  DSLAM_TRY(b.counts.alloc(8));
  DSLAM_TRY(b.bin_fill.alloc(8 * bins));
  DSLAM_TRY(b.bin_start.alloc(8 * (bins + 1)));
  DSLAM_TRY(b.bin_list.alloc(4 * per_image));
  DSLAM_TRY(b.stage.alloc(3 * cap));
  DSLAM_TRY(b.packed.alloc(3 * cap));
  DSLAM_TRY(b.flags.alloc(cap));
  DSLAM_TRY(b.keep.alloc(cap));
  DSLAM_TRY(b.match_offset.alloc(cap));
  DSLAM_TRY(b.match_count.alloc(4));
  // no frame yet: every list is empty, and its bins with it
  DSLAM_HIP(hipMemsetAsync(b.counts.get(), 0, 8 * sizeof(int), e->stream));
  DSLAM_HIP(hipMemsetAsync(b.bin_start.get(), 0, 8 * (bins + 1) * sizeof(int), e->stream));
  DSLAM_HIP(hipMemsetAsync(b.match_count.get(), 0, 4 * sizeof(int), e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  static_cast<SflowBuffers &>(*sf) = std::move(b);
  return DSLAM_OK;
}

int launch_sflow_push(dslam_engine *e, dslam_sflow *sf, const SflowPush &c) {
  DSLAM_HIP(hipSetDevice(e->device));
  const size_t image_bytes = (size_t)sf->w * sf->h * sf->channels, mn = (size_t)sf->mw * sf->mh;
  const int sides = c.right ? 2 : 1, bins = bins_of(sf);
  const unsigned char *left = static_cast<const unsigned char *>(c.left), *right = static_cast<const unsigned char *>(c.right);
  sf->recorded &= ~0x1f;
  if (c.host) {
    DSLAM_HIP(hipMemcpyAsync(sf->images.get(), c.left, image_bytes, hipMemcpyHostToDevice, e->stream));
    left = sf->images.get();
    if (c.right) {
      DSLAM_HIP(hipMemcpyAsync(sf->images.get() + image_bytes, c.right, image_bytes, hipMemcpyHostToDevice, e->stream));
      right = left + image_bytes;
    }
  }
  if (!c.replace && sf->pushes > 0) sf->cur ^= 1;
  sf->pushes++;
  const int l0 = sf->cur * 4;   // the first list of the current frame
  if (!c.right) DSLAM_HIP(hipMemsetAsync(sf->counts.get() + l0 + 2, 0, 2 * sizeof(int), e->stream));

  DSLAM_TRY(mark_phase(e, sf, 0));
  FilterParams fp;
  fp.img[0] = left; fp.img[1] = right;
  fp.sobel = sf->sobel.get(); fp.corner = sf->corner.get();
  fp.W = sf->w; fp.channels = sf->channels; fp.half = sf->s == 2; fp.mw = sf->mw; fp.mh = sf->mh;
  hipLaunchKernelGGL(k_sf_filter, dim3((sf->mw + kTileW - 1) / kTileW, (sf->mh + kTileH - 1) / kTileH, sides), dim3(256), 0, e->stream, fp);
  DSLAM_HIP(hipGetLastError());
  DSLAM_TRY(mark_phase(e, sf, 1));

  const int cells = sf->cx[1] * sf->cy[1], stride = cells + 1;
  NmsParams np;
  memset(&np, 0, sizeof np);
  np.corner = sf->corner.get(); np.sobel = sf->sobel.get();
  np.cell_feat = sf->cell_feat.get(); np.cell_count = sf->cell_count.get(); np.cell_offset = sf->cell_offset.get();
  for (int k = 0; k < 4; k++) {
    np.feats[k] = sf->feats.get() + 3 * list_base(sf, l0 + k);
    np.bin_fill[k] = sf->bin_fill.get() + (size_t)(l0 + k) * bins;
  }
  np.mw = sf->mw; np.mh = sf->mh; np.tau = sf->tau; np.s = sf->s; np.binsize = sf->binsize; np.ub = sf->ub; np.vb = sf->vb;
  np.stride = stride;
  for (int k = 0; k < 2; k++) { np.n[k] = sf->n[k]; np.cx[k] = sf->cx[k]; np.cy[k] = sf->cy[k]; }
  ScanParams cells_scan, bins_scan;
  memset(&cells_scan, 0, sizeof cells_scan);
  memset(&bins_scan, 0, sizeof bins_scan);
  for (int k = 0; k < 2 * sides; k++) {
    cells_scan.l[k] = ScanList{sf->cell_count.get() + (size_t)k * stride, sf->cell_offset.get() + (size_t)k * stride, nullptr,
                               sf->counts.get() + l0 + k, sf->cx[k & 1] * sf->cy[k & 1], 0};
    bins_scan.l[k] = ScanList{sf->bin_fill.get() + (size_t)(l0 + k) * bins, sf->bin_start.get() + (size_t)(l0 + k) * (bins + 1), nullptr,
                              nullptr, bins, 1};
  }
  const dim3 cell_grid((cells + 255) / 256, 2 * sides);
  if (cells > 0) {
    hipLaunchKernelGGL(k_sf_nms, cell_grid, dim3(256), 0, e->stream, np);
    DSLAM_HIP(hipGetLastError());
  }
  DSLAM_TRY(mark_phase(e, sf, 2));
  hipLaunchKernelGGL(k_sf_scan, dim3(2 * sides), dim3(kScanThreads), 0, e->stream, cells_scan);
  DSLAM_HIP(hipGetLastError());
  DSLAM_HIP(hipMemsetAsync(sf->bin_fill.get() + (size_t)l0 * bins, 0, (size_t)4 * bins * sizeof(int), e->stream));
  if (cells > 0) {
    hipLaunchKernelGGL(k_sf_emit, cell_grid, dim3(256), 0, e->stream, np);
    DSLAM_HIP(hipGetLastError());
  }
  DSLAM_TRY(mark_phase(e, sf, 3));
  // (a frame without a right image: its right lists are empty and their bin starts all zero)
  if (!c.right) DSLAM_HIP(hipMemsetAsync(sf->bin_start.get() + (size_t)(l0 + 2) * (bins + 1), 0, (size_t)2 * (bins + 1) * sizeof(int), e->stream));
  hipLaunchKernelGGL(k_sf_scan, dim3(2 * sides), dim3(kScanThreads), 0, e->stream, bins_scan);
  DSLAM_HIP(hipGetLastError());
  if (sf->cap[1] > 0) {
    BinParams bp;
    memset(&bp, 0, sizeof bp);
    for (int k = 0; k < 2 * sides; k++) {
      bp.feats[k] = np.feats[k]; bp.count[k] = sf->counts.get() + l0 + k; bp.bin_fill[k] = np.bin_fill[k];
      bp.bin_start[k] = sf->bin_start.get() + (size_t)(l0 + k) * (bins + 1);
      bp.bin_list[k] = sf->bin_list.get() + list_base(sf, l0 + k);
      bp.cap[k] = sf->cap[k & 1];
    }
    bp.binsize = sf->binsize; bp.ub = sf->ub; bp.vb = sf->vb;
    hipLaunchKernelGGL(k_sf_bin_scatter, dim3((sf->cap[1] + 255) / 256, 2 * sides), dim3(256), 0, e->stream, bp);
    DSLAM_HIP(hipGetLastError());
  }
  DSLAM_TRY(mark_phase(e, sf, 4));
  (void)mn;
  return DSLAM_OK;
}

int launch_sflow_match(dslam_engine *e, dslam_sflow *sf, const SflowMatch &c) {
  DSLAM_HIP(hipSetDevice(e->device));
  const int bins = bins_of(sf), cap = sf->cap[c.set];
  sf->recorded &= 0x1f;
  int4 *out = c.host ? sf->packed.get() : static_cast<int4 *>(c.out);
  int *count = c.host ? sf->match_count.get() : static_cast<int *>(c.count);
  MatchParams mp;
  memset(&mp, 0, sizeof mp);
  for (int image = 0; image < 4; image++) {
    const int slot = image >= DSLAM_SFLOW_IMAGE_1P ? sf->cur ^ 1 : sf->cur;
    const int l = (slot * 2 + (image & 1)) * 2 + c.set;
    mp.feat[image] = sf->feats.get() + 3 * list_base(sf, l);
    mp.count[image] = sf->counts.get() + l;
    mp.dense_count[image] = sf->counts.get() + (l | 1);
    mp.bin_start[image] = sf->bin_start.get() + (size_t)l * (bins + 1);
    mp.bin_list[image] = sf->bin_list.get() + list_base(sf, l);
  }
  mp.stage = sf->stage.get(); mp.flags = sf->flags.get();
  mp.cap = cap; mp.binsize = sf->binsize; mp.ub = sf->ub; mp.vb = sf->vb; mp.radius = sf->radius; mp.vtol = sf->vtol;
  const int drive = c.method == 2 ? DSLAM_SFLOW_IMAGE_1P : DSLAM_SFLOW_IMAGE_1C;
  DSLAM_TRY(mark_phase(e, sf, 5));
  const int waves = cap < 4 * kMatchBlocks ? cap : 4 * kMatchBlocks;
  const dim3 grid((waves + 3) / 4 > 0 ? (waves + 3) / 4 : 1);
  if (c.method == 2) hipLaunchKernelGGL(k_sf_match<2>, grid, dim3(256), 0, e->stream, mp);
  else if (c.method == 1) hipLaunchKernelGGL(k_sf_match<1>, grid, dim3(256), 0, e->stream, mp);
  else hipLaunchKernelGGL(k_sf_match<0>, grid, dim3(256), 0, e->stream, mp);
  DSLAM_HIP(hipGetLastError());
  DSLAM_TRY(mark_phase(e, sf, 6));
  const int *keep = sf->flags.get();
  const dim3 lanes_grid((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  if (c.method != 2) {
    hipLaunchKernelGGL(k_sf_pixel, lanes_grid, dim3(256), 0, e->stream, mp.feat[drive], mp.count[drive], cap, sf->flags.get(), sf->keep.get());
    DSLAM_HIP(hipGetLastError());
    keep = sf->keep.get();
  }
  ScanParams sp;
  memset(&sp, 0, sizeof sp);
  sp.l[0] = ScanList{keep, sf->match_offset.get(), mp.count[drive], count, cap, 0};
  hipLaunchKernelGGL(k_sf_scan, dim3(1), dim3(kScanThreads), 0, e->stream, sp);
  DSLAM_HIP(hipGetLastError());
  if (c.capacity > 0) {
    hipLaunchKernelGGL(k_sf_compact, lanes_grid, dim3(256), 0, e->stream, sf->stage.get(), mp.count[drive], cap, keep, sf->match_offset.get(),
                       out, c.capacity);
    DSLAM_HIP(hipGetLastError());
  }
  DSLAM_TRY(mark_phase(e, sf, 7));
  if (c.host) {
    // the number of records to copy is a device result: wait for it, then copy no more than the caller has room for
    int n = 0;
    DSLAM_HIP(hipMemcpyAsync(&n, count, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    const int copy = n < c.capacity ? n : c.capacity;
    if (copy > 0) {
      DSLAM_HIP(hipMemcpyAsync(c.out, out, (size_t)copy * DSLAM_SFLOW_MATCH_WORDS * sizeof(int), hipMemcpyDeviceToHost, e->stream));
      DSLAM_HIP(hipStreamSynchronize(e->stream));
    }
    *static_cast<int32_t *>(c.count) = n;
  }
  return DSLAM_OK;
}

int sflow_features(dslam_engine *e, dslam_sflow *sf, int image, int set, void *out_host, int capacity, int32_t *count_out) {
  DSLAM_HIP(hipSetDevice(e->device));
  const int slot = image >= DSLAM_SFLOW_IMAGE_1P ? sf->cur ^ 1 : sf->cur;
  const int l = (slot * 2 + (image & 1)) * 2 + set;
  int n = 0;
  DSLAM_HIP(hipMemcpyAsync(&n, sf->counts.get() + l, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  const int copy = n < capacity ? n : capacity;
  if (copy > 0) {
    DSLAM_HIP(hipMemcpyAsync(out_host, sf->feats.get() + 3 * list_base(sf, l), (size_t)copy * DSLAM_SFLOW_FEATURE_BYTES, hipMemcpyDeviceToHost,
                             e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
  }
  *count_out = n;
  return DSLAM_OK;
}

int sflow_download(dslam_engine *e, dslam_sflow *sf, int side, int filter, void *out_host) {
  DSLAM_HIP(hipSetDevice(e->device));
  const size_t mn = (size_t)sf->mw * sf->mh;
  if (filter <= DSLAM_SFLOW_FILTER_DV)
    DSLAM_HIP(hipMemcpyAsync(out_host, sf->sobel.get() + ((size_t)side * 2 + filter) * mn, mn, hipMemcpyDeviceToHost, e->stream));
  else
    DSLAM_HIP(hipMemcpyAsync(out_host, sf->corner.get() + ((size_t)side * 2 + (filter - DSLAM_SFLOW_FILTER_F1)) * mn, mn * sizeof(short),
                             hipMemcpyDeviceToHost, e->stream));
  return DSLAM_OK;
}

// bench hook: the boundaries recorded are 0 filters 1 suppression 2 compaction 3 bins 4 | 5 matching 6 match compaction 7
int sflow_phases(dslam_engine *e, dslam_sflow *sf, int enable, float *ms_out) {
  if (ms_out) {
    DSLAM_HIP(hipSetDevice(e->device));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    const int first[6] = {0, 1, 2, 3, 5, 6};
    for (int k = 0; k < 6; k++) {
      ms_out[k] = -1.0f;
      const int a = first[k];
      if ((sf->recorded >> a & 1) && (sf->recorded >> (a + 1) & 1)) DSLAM_HIP(hipEventElapsedTime(&ms_out[k], sf->events[a], sf->events[a + 1]));
    }
  }
  if (enable >= 0) sf->timing = enable != 0;
  return DSLAM_OK;
}

}  // namespace dslam
