// stereo.hip -- semi-global stereo matching on the device (dslam_stereo_*, dslam_disparity_to_depth; DESIGN.md section 33;
// include/dslam_fusion.h states the law in full).
//
// Reference: the law is this project's own and all-integer up to the depth conversion, so every result is held bit for bit
// against tests/ref_stereo.py.  The conversion follows DepthProvider::DepthFromDisparityMap's order of float32 operations.
//
// k_st_census     one lane per pixel, both images in one launch (blockIdx.y): 62 clamped neighbour reads against the
//                 centre, the grey of an RGBA pixel formed as it is read.
// k_st_aggregate  one wave64 per path line, all eight directions in ONE launch (2 H + 2 W + 4 (W + H - 1) independent
//                 workgroups of one wave; the horizontal lines, the longest dependent chains, come first).  Lane l holds
//                 disparity l (and l + 64 at D = 128) in named registers.  Per step: the left code is wave-uniform, the
//                 right codes are one contiguous reversed row segment (both loaded one step ahead), the d +- 1 neighbours come by lane shifts, the
//                 minimum by a butterfly.  Every L_r is added to S with one 32-bit atomic add per PAIR of disparities (the
//                 even lane takes its neighbour's value into the high half; a half never carries: S <= 2040), so a wave's
//                 adds are 128 contiguous bytes per 64 disparities and the sum does not depend on any order.
// k_st_select     one wave per pixel over its row of S (D innermost: one contiguous 128 / 256 byte read): d*, s0, s2, the
//                 sub-pixel step and the uniqueness filter; every lane also offers S(y, x, d) << 8 | d to pixel x - d of the
//                 right image with an atomic min, which is the right disparity with the smallest d on ties.
// k_st_finish     one lane per pixel: x - d* >= 0, the left-right check, the disparity and, where asked, the depth.
// k_st_depth      the conversion alone.
// No kernel uses scratch memory or LDS; no workgroup waits for another.
#include <cmath>
#include <cstring>

#include "dslam_internal.h"

#pragma clang fp contract(off)

namespace dslam {

namespace {

constexpr unsigned kStBig = 0xFFFFu;   // an absent neighbour of the recurrence: beyond every L_r + p1

struct StCensusParams {
  const unsigned char *img[2];
  unsigned long long *out;   // [2][H W]
  int W, H, channels;
};

struct StAggParams {
  const unsigned long long *cl, *cr;
  unsigned *S32;             // S as pairs of disparities
  int W, H, p1, p2;
};

struct StSelectParams {
  const unsigned short *S;
  unsigned *rkey, *cand;
  int W, n, uniq;
};

struct StDepth {
  float fb, ks;              // focal_length_px * baseline_m, 1000 * scale
  int min_mm, max_mm;
};

struct StFinishParams {
  const unsigned *rkey, *cand;
  unsigned short *disp;
  short *depth;              // NULL: no conversion
  StDepth dc;
  int W, n, lr_max;
};

__device__ __forceinline__ unsigned st_wave_min(unsigned v) {
  for (int d = 32; d > 0; d >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, d, 64));
  return v;
}

__device__ __forceinline__ int st_grey(const unsigned char *img, int channels, size_t pix) {
  if (channels == 1) return img[pix];
  const uchar4 c = reinterpret_cast<const uchar4 *>(img)[pix];
  return (c.x + 2 * c.y + c.z) >> 2;
}

__device__ __forceinline__ short st_depth_mm(unsigned d16, const StDepth &c) {
  if (d16 == DSLAM_STEREO_INVALID || d16 == 0) return 0;
  const float disp = (float)d16 * 0.0625f;
  const float z = c.fb / disp;
  const float mm_f = c.ks * z;
  if (!(mm_f < 2147483648.0f)) return 0;
  const int mm = (int)mm_f;
  if (mm > c.max_mm || mm < c.min_mm) return 0;
  return (short)mm;
}

__global__ __launch_bounds__(256) void k_st_census(StCensusParams p) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.z * 4 + (threadIdx.x >> 6);
  if (x >= p.W || y >= p.H) return;
  const unsigned char *img = p.img[blockIdx.y];
  const int centre = st_grey(img, p.channels, (size_t)y * p.W + x);
  unsigned long long code = 0;
#pragma unroll
  for (int dy = -3; dy <= 3; dy++) {
    const size_t row = (size_t)min(max(y + dy, 0), p.H - 1) * p.W;
#pragma unroll
    for (int dx = -4; dx <= 4; dx++) {
      if (dy == 0 && dx == 0) continue;
      const int v = st_grey(img, p.channels, row + min(max(x + dx, 0), p.W - 1));
      code = (code << 1) | (unsigned long long)(v < centre);
    }
  }
  p.out[(size_t)blockIdx.y * p.W * p.H + (size_t)y * p.W + x] = code;
}

// K = D / 64 disparities per lane
template <int K>
__global__ __launch_bounds__(64) void k_st_aggregate(StAggParams p) {
  constexpr int D = 64 * K;
  const int lane = threadIdx.x, W = p.W, H = p.H;
  // the line of this wave: direction (dy, dx) and its first pixel, the one whose predecessor is outside the image
  int line = blockIdx.x, dy, dx, y, x;
  if (line < 2 * H) {
    dy = 0; dx = line < H ? 1 : -1;
    y = line < H ? line : line - H; x = dx > 0 ? 0 : W - 1;
  } else if ((line -= 2 * H) < 2 * W) {
    dx = 0; dy = line < W ? 1 : -1;
    x = line < W ? line : line - W; y = dy > 0 ? 0 : H - 1;
  } else {
    line -= 2 * W;
    const int n = W + H - 1, q = line / n, k = line - q * n;
    dy = (q & 2) ? -1 : 1; dx = (q & 1) ? -1 : 1;
    const int ys = k < W ? 0 : k - W + 1;   // the first W start on the first row, the others on the first column
    y = dy > 0 ? ys : H - 1 - ys;
    x = k < W ? k : (dx > 0 ? 0 : W - 1);
  }
  unsigned prev0 = 0, prev1 = 0;
  bool first = true;
  // the codes of a step are loaded one step ahead, so their latency hides behind the dependent chain of the step before
  unsigned long long cl = 0, r0 = 0, r1 = 0;
  auto load = [&](int xx, int yy) {
    const size_t at = (size_t)yy * W + xx;
    cl = p.cl[at];
    if (xx - lane >= 0) r0 = p.cr[at - lane];
    if (K == 2 && xx - lane - 64 >= 0) r1 = p.cr[at - lane - 64];
  };
  load(x, y);   // (W, H >= 1: every line has a first pixel)
  while (true) {
    const size_t pix = (size_t)y * W + x;
    unsigned c0 = DSLAM_STEREO_COST_OUT, c1 = DSLAM_STEREO_COST_OUT;
    if (x - lane >= 0) c0 = __popcll(cl ^ r0);
    if (K == 2 && x - lane - 64 >= 0) c1 = __popcll(cl ^ r1);
    const int xn = x + dx, yn = y + dy;
    const bool more = xn >= 0 && xn < W && yn >= 0 && yn < H;
    if (more) load(xn, yn);
    unsigned l0 = c0, l1 = c1;
    if (!first) {
      const unsigned m = st_wave_min(K == 2 ? min(prev0, prev1) : prev0);
      unsigned up0 = __shfl_up((int)prev0, 1, 64), dn0 = __shfl_down((int)prev0, 1, 64);
      if (lane == 0) up0 = kStBig;
      if (K == 2) {
        unsigned up1 = __shfl_up((int)prev1, 1, 64), dn1 = __shfl_down((int)prev1, 1, 64);
        const unsigned last0 = __shfl((int)prev0, 63, 64), first1 = __shfl((int)prev1, 0, 64);
        if (lane == 63) { dn0 = first1; dn1 = kStBig; }
        if (lane == 0) up1 = last0;
        l1 = c1 + min(min(prev1, min(up1, dn1) + p.p1), m + p.p2) - m;
      } else if (lane == 63) {
        dn0 = kStBig;
      }
      l0 = c0 + min(min(prev0, min(up0, dn0) + p.p1), m + p.p2) - m;
    }
    // S += L_r: the even lane adds its own value and its neighbour's
    unsigned *dst = p.S32 + ((pix * D + lane) >> 1);
    const unsigned hi0 = __shfl_down((int)l0, 1, 64);
    if (!(lane & 1)) __hip_atomic_fetch_add(dst, l0 | hi0 << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (K == 2) {
      const unsigned hi1 = __shfl_down((int)l1, 1, 64);
      if (!(lane & 1)) __hip_atomic_fetch_add(dst + 32, l1 | hi1 << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!more) break;
    prev0 = l0; prev1 = l1;
    first = false;
    x = xn; y = yn;
  }
}

template <int K>
__global__ __launch_bounds__(256) void k_st_select(StSelectParams p) {
  constexpr int D = 64 * K;
  const int lane = threadIdx.x & 63;
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= p.n) return;
  const int x = pix % p.W;
  const unsigned short *row = p.S + (size_t)pix * D;
  const unsigned s_0 = row[lane], s_1 = K == 2 ? row[lane + 64] : 0;
  unsigned key = s_0 << 8 | lane;
  if (K == 2) key = min(key, s_1 << 8 | (lane + 64));
  key = st_wave_min(key);
  const int ds = key & 0xff;
  const int s0 = key >> 8;
  unsigned t = 0xFFFFFFu;
  if (abs(lane - ds) > 1) t = s_0;
  if (K == 2 && abs(lane + 64 - ds) > 1) t = min(t, s_1);
  const int s2 = st_wave_min(t);
  // S(d* - 1), S(d* + 1): out of range where d* is at an end, and not used there
  const int dm = (ds - 1) & (D - 1), dp = (ds + 1) & (D - 1);
  int sm = __shfl((int)s_0, dm & 63, 64), sp = __shfl((int)s_0, dp & 63, 64);
  if (K == 2) {
    const int sm1 = __shfl((int)s_1, dm & 63, 64), sp1 = __shfl((int)s_1, dp & 63, 64);
    if (dm >= 64) sm = sm1;
    if (dp >= 64) sp = sp1;
  }
  int delta = 0;
  const int den = sm + sp - 2 * s0;
  if (ds > 0 && ds < D - 1 && den > 0) {
    const int num = 16 * (sm - sp) + den, den2 = 2 * den;
    delta = num / den2;
    if (num % den2 != 0 && num < 0) delta--;   // floor, not C's truncation
  }
  // the right image's view of this pixel's row of S
  if (x - lane >= 0) atomicMin(p.rkey + pix - lane, s_0 << 8 | lane);
  if (K == 2 && x - lane - 64 >= 0) atomicMin(p.rkey + pix - lane - 64, s_1 << 8 | (lane + 64));
  if (lane == 0) {
    const bool reject = s2 * (100 - p.uniq) < s0 * 100 || x - ds < 0;
    p.cand[pix] = reject ? 0xFFFFFFFFu : (unsigned)ds << 16 | (unsigned)(16 * ds + delta);
  }
}

__global__ __launch_bounds__(256) void k_st_finish(StFinishParams p) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= p.n) return;
  const unsigned c = p.cand[pix];
  unsigned d16 = DSLAM_STEREO_INVALID;
  if (c != 0xFFFFFFFFu) {
    const int ds = c >> 16;
    bool ok = true;
    if (p.lr_max >= 0) {
      const int dr = p.rkey[pix - ds] & 0xff;   // (x - d* >= 0: k_st_select rejected the others)
      ok = abs(dr - ds) <= p.lr_max;
    }
    if (ok) d16 = c & 0xffffu;
  }
  p.disp[pix] = (unsigned short)d16;
  if (p.depth) p.depth[pix] = st_depth_mm(d16, p.dc);
}

__global__ __launch_bounds__(256) void k_st_depth(const unsigned short *disp, short *depth, StDepth dc, int n) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix < n) depth[pix] = st_depth_mm(disp[pix], dc);
}

// a phase boundary of the bench hook (dslam_debug_stereo_phases)
int mark_phase(dslam_engine *e, dslam_stereo *st, int k) {
  if (!st->timing) return DSLAM_OK;
  if (!st->events[k]) DSLAM_TRY(st->events[k].create(hipEventDefault));
  DSLAM_HIP(hipEventRecord(st->events[k], e->stream));
  st->recorded |= 1 << k;
  return DSLAM_OK;
}

StDepth depth_constants(const dslam_stereo_calib &c) {
  StDepth d;
  d.fb = c.focal_length_px * c.baseline_m;
  d.ks = 1000.0f * c.scale;
  d.min_mm = (int)(c.min_depth_m * 1000.0f);
  d.max_mm = (int)(c.max_depth_m * 1000.0f);
  return d;
}

}  // namespace

int stereo_resolve_params(const dslam_stereo_params *params, dslam_stereo *st) {
  dslam_stereo_params p;
  memset(&p, 0, sizeof p);
  if (params) p = *params;
  DSLAM_REQUIRE(p.pad[0] == 0 && p.pad[1] == 0, "dslam_stereo_params: pad must be 0");
  if (p.max_disparity == 0) p.max_disparity = 128;
  if (p.p1 == 0) p.p1 = 10;
  if (p.p2 == 0) p.p2 = 120;
  if (p.uniqueness == 0) p.uniqueness = 5;
  if (p.lr_max == 0) p.lr_max = 1;
  if (p.channels == 0) p.channels = 1;
  DSLAM_REQUIRE(p.max_disparity == 64 || p.max_disparity == 128, "max_disparity must be 64 or 128");
  DSLAM_REQUIRE(p.p1 >= 1 && p.p1 <= p.p2 && p.p2 <= DSLAM_STEREO_MAX_P2, "need 1 <= p1 <= p2 <= DSLAM_STEREO_MAX_P2");
  DSLAM_REQUIRE(p.uniqueness >= -1 && p.uniqueness <= 99, "uniqueness must be -1 (off) or 1 .. 99");
  DSLAM_REQUIRE(p.lr_max >= -2 && p.lr_max <= p.max_disparity, "lr_max must be -2 (exact), -1 (off) or 1 .. max_disparity");
  DSLAM_REQUIRE(p.channels == 1 || p.channels == 4, "channels must be 1 or 4");
  st->p = p;
  st->D = p.max_disparity; st->p1 = p.p1; st->p2 = p.p2;
  st->uniq = p.uniqueness < 0 ? 0 : p.uniqueness;
  st->lr_max = p.lr_max == -2 ? 0 : p.lr_max;
  st->channels = p.channels;
  return DSLAM_OK;
}

int stereo_allocate(dslam_engine *e, dslam_stereo *st) {
  DSLAM_HIP(hipSetDevice(e->device));
  const size_t n = (size_t)st->w * st->h;
  StereoBuffers b;   // built aside: a failure leaves no partial handle
  DSLAM_TRY(b.S.alloc(n * st->D));
  DSLAM_TRY(b.census.alloc(2 * n));
  DSLAM_TRY(b.rkey.alloc(n));
  DSLAM_TRY(b.cand.alloc(n));
  DSLAM_TRY(b.images.alloc(2 * n * st->channels));
  DSLAM_TRY(b.disp.alloc(n));
  DSLAM_TRY(b.depth.alloc(n));
  static_cast<StereoBuffers &>(*st) = std::move(b);
  return DSLAM_OK;
}

int launch_stereo(dslam_engine *e, dslam_stereo *st, const StereoCall &c) {
  DSLAM_HIP(hipSetDevice(e->device));
  const int W = st->w, H = st->h, D = st->D;
  const size_t n = (size_t)W * H, image_bytes = n * st->channels;
  st->recorded = 0;
  unsigned short *disp_dev = c.host || !c.disp_out ? st->disp.get() : static_cast<unsigned short *>(c.disp_out);
  short *depth_dev = !c.calib ? nullptr : c.host ? st->depth.get() : static_cast<short *>(c.depth_out);
  const bool select = c.left || c.S_host;

  if (c.left) {
    const unsigned char *left = static_cast<const unsigned char *>(c.left), *right = static_cast<const unsigned char *>(c.right);
    if (c.host) {
      DSLAM_HIP(hipMemcpyAsync(st->images.get(), c.left, image_bytes, hipMemcpyHostToDevice, e->stream));
      DSLAM_HIP(hipMemcpyAsync(st->images.get() + image_bytes, c.right, image_bytes, hipMemcpyHostToDevice, e->stream));
      left = st->images.get(); right = left + image_bytes;
    }
    st->matched = true;
    DSLAM_TRY(mark_phase(e, st, 0));
    StCensusParams cp;
    cp.img[0] = left; cp.img[1] = right;
    cp.out = st->census.get();
    cp.W = W; cp.H = H; cp.channels = st->channels;
    hipLaunchKernelGGL(k_st_census, dim3((W + 63) / 64, 2, (H + 3) / 4), dim3(256), 0, e->stream, cp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(mark_phase(e, st, 1));
    DSLAM_HIP(hipMemsetAsync(st->S.get(), 0, n * D * sizeof(unsigned short), e->stream));
    StAggParams ap;
    ap.cl = st->census.get(); ap.cr = st->census.get() + n;
    ap.S32 = reinterpret_cast<unsigned *>(st->S.get());
    ap.W = W; ap.H = H; ap.p1 = st->p1; ap.p2 = st->p2;
    const unsigned lines = 2u * H + 2u * W + 4u * (W + H - 1);
    if (D == 64) hipLaunchKernelGGL(k_st_aggregate<1>, dim3(lines), dim3(64), 0, e->stream, ap);
    else hipLaunchKernelGGL(k_st_aggregate<2>, dim3(lines), dim3(64), 0, e->stream, ap);
    DSLAM_HIP(hipGetLastError());
  } else if (c.S_host) {
    DSLAM_HIP(hipMemcpyAsync(st->S.get(), c.S_host, n * D * sizeof(unsigned short), hipMemcpyHostToDevice, e->stream));
  }
  if (select) {
    DSLAM_TRY(mark_phase(e, st, 2));
    DSLAM_HIP(hipMemsetAsync(st->rkey.get(), 0xFF, n * sizeof(unsigned), e->stream));
    StSelectParams sp;
    sp.S = st->S.get(); sp.rkey = st->rkey.get(); sp.cand = st->cand.get();
    sp.W = W; sp.n = (int)n; sp.uniq = st->uniq;
    const unsigned blocks = (unsigned)((n + 3) / 4);
    if (D == 64) hipLaunchKernelGGL(k_st_select<1>, dim3(blocks), dim3(256), 0, e->stream, sp);
    else hipLaunchKernelGGL(k_st_select<2>, dim3(blocks), dim3(256), 0, e->stream, sp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(mark_phase(e, st, 3));
    StFinishParams fp;
    memset(&fp, 0, sizeof fp);
    fp.rkey = st->rkey.get(); fp.cand = st->cand.get();
    fp.disp = disp_dev; fp.depth = depth_dev;
    if (c.calib) fp.dc = depth_constants(*c.calib);
    fp.W = W; fp.n = (int)n; fp.lr_max = st->lr_max;
    hipLaunchKernelGGL(k_st_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, fp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(mark_phase(e, st, 4));
  } else {
    // the conversion alone
    const unsigned short *src = static_cast<const unsigned short *>(c.disp_in);
    if (c.host) {
      DSLAM_HIP(hipMemcpyAsync(st->disp.get(), c.disp_in, n * sizeof(unsigned short), hipMemcpyHostToDevice, e->stream));
      src = st->disp.get();
    }
    DSLAM_TRY(mark_phase(e, st, 4));
    hipLaunchKernelGGL(k_st_depth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, src, depth_dev, depth_constants(*c.calib), (int)n);
    DSLAM_HIP(hipGetLastError());
    DSLAM_TRY(mark_phase(e, st, 5));
  }
  if (c.host) {
    if (select && c.disp_out) DSLAM_HIP(hipMemcpyAsync(c.disp_out, st->disp.get(), n * sizeof(unsigned short), hipMemcpyDeviceToHost, e->stream));
    if (c.calib) DSLAM_HIP(hipMemcpyAsync(c.depth_out, st->depth.get(), n * sizeof(short), hipMemcpyDeviceToHost, e->stream));
  }
  return DSLAM_OK;
}

int stereo_download(dslam_engine *e, dslam_stereo *st, int what, void *out_host) {
  DSLAM_HIP(hipSetDevice(e->device));
  const size_t n = (size_t)st->w * st->h;
  const void *src = what == DSLAM_STEREO_S ? static_cast<const void *>(st->S.get())
                                           : static_cast<const void *>(st->census.get() + (what == DSLAM_STEREO_CENSUS_RIGHT ? n : 0));
  const size_t bytes = what == DSLAM_STEREO_S ? n * st->D * sizeof(unsigned short) : n * sizeof(unsigned long long);
  DSLAM_HIP(hipMemcpyAsync(out_host, src, bytes, hipMemcpyDeviceToHost, e->stream));
  return DSLAM_OK;
}

// bench hook: the boundaries recorded are 0 census 1 aggregation 2 selection 3 finish 4 [conversion alone 5]
int stereo_phases(dslam_engine *e, dslam_stereo *st, int enable, float *ms_out) {
  if (ms_out) {
    DSLAM_HIP(hipSetDevice(e->device));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    for (int k = 0; k < 5; k++) {
      ms_out[k] = -1.0f;
      if ((st->recorded >> k & 1) && (st->recorded >> (k + 1) & 1)) DSLAM_HIP(hipEventElapsedTime(&ms_out[k], st->events[k], st->events[k + 1]));
    }
  }
  if (enable >= 0) st->timing = enable != 0;
  return DSLAM_OK;
}

}  // namespace dslam
