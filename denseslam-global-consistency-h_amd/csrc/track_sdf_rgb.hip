// track_sdf_rgb.hip -- the depth-to-SDF camera tracker with a photometric term (dslam_track_camera_sdf_rgb).
//
// Reference: none (ITMColorTracker has the purpose; the law is this project's own, DESIGN.md section 30, stated in full in
// include/dslam_fusion.h).  Every map is only read; no render state, no raycast, no visible list, no image gradients.
//
// One evaluation is track_sdf.hip's (items 1 - 6 of its law, b = -d, A = [r x g, g]) and, on a level that carries the term,
// per pixel besides:
//   image     I = G_l[x, y], the grey pyramid of the view's RGBA image (k_grey_level0, k_grey_subsample below);
//   per map   that passed its 8-tap gate: colour-ok iff all 8 taps have w_color > 0; the tap grey
//             y_k = ((0.299f R + 0.587f G) + 0.114f B) * (float)(1.0 / 255.0) of the tap's clr bytes; C_i, h_i by the
//             expressions of d_i, g_i on y; w^c_i the three lerp stages on the taps' w_color; h_i^w = R_i^T h_i;
//   combine   Blend / Blend3 over the colour-ok maps in list order;
//   gate      e = C - I; a colour miss for a depth miss, no colour-ok map or |e| > colour_gate;
//   rows      b_c = -(k e), A_c = k [r x h, h], k = colour_weight; they go into the same 27 H / N accumulators, after the
//             pixel's depth products;
//   sums      35: the 33 of track_sdf.hip, [33] sum e^2 over the colour-valid pixels, [34] colour-valid.
//
// Device work per evaluation: k_track_sdf_rgb, with k_track_sdf's grid, pixel order (8 x 8 tiles or rows), partition of
// the pixels over the workgroups and reduction order, over 35 sums: per-lane doubles of float32 products, wave shuffle tree,
// the four wave partials through LDS in index order, one row of 35 per workgroup in mapped page-locked memory (a workgroup
// without a pixel writes zeros), rows added by the host in index order.  No atomics; the same bytes on every run.  The
// colour half comes out of the uint2 taps gather_cell has already loaded: the term adds no voxel load, and one 4-byte
// image read per colour-valid candidate.  The kernel's text is its own and not track_sdf_device.h's, so that the device
// code of k_track_sdf and k_track_sdf_starts stays what it was (profiles/device_code_diff.sh); the depth statements below
// are that header's, expression for expression, so that sums [0..32] of a level without the term, or of maps without
// colour, are dslam_track_camera_sdf's byte for byte (tests/test_gpu_track_sdf_rgb.py).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "register_device.h"
#include "register_host.h"
#include "track_sdf_host.h"

#pragma clang fp contract(off)

namespace dslam {

struct TrackSdfRgbParams {
  const float *depth;        // level l of the depth pyramid, lw x lh
  int lw, lh;
  float fx, fy, cx, cy;      // the intrinsics of the level
  float inv_vs;              // (float)(1.0 / (double)voxel_size)
  float P[12];               // P~
  const MultiMap *maps;      // [num_maps], device
  int num_maps;
  float residual_gate;
  const float *grey;         // level l of the grey pyramid, lw x lh; nullptr: the level carries no photometric term
  float colour_weight, colour_gate;
  double *partials;          // [gridDim.x][kTrackSdfRgbSums]
};

// grey of three colour bytes: the one expression of the image side (k_grey_level0) and of the map side (a tap's clr)
__device__ __forceinline__ float grey_of(unsigned r, unsigned g, unsigned b) {
  return ((0.299f * (float)r + 0.587f * (float)g) + 0.114f * (float)b) * (float)(1.0 / 255.0);
}

// G_0 of the view's RGBA image (alpha ignored)
__global__ __launch_bounds__(256) void k_grey_level0(const uchar4 *rgba, float *out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uchar4 c = rgba[i];
  out[i] = grey_of(c.x, c.y, c.z);
}

// G_k: the plain 2 x 2 mean of level k - 1 (iw wide); an odd last row or column of it is dropped
__global__ __launch_bounds__(256) void k_grey_subsample(const float *in, int iw, float *out, int ow, int oh) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= ow || y >= oh) return;
  const float *row0 = in + (size_t)(2 * y) * iw + 2 * x, *row1 = row0 + iw;
  out[x + (size_t)y * ow] = ((row0[0] + row0[1]) + (row1[0] + row1[1])) * 0.25f;
}

// One lane per pixel in a grid-stride loop (TILES: which pixel takes which lane, as k_track_sdf).
template <bool TILES>
__global__ __launch_bounds__(kTrackSdfThreads) void k_track_sdf_rgb(TrackSdfRgbParams p) {
  double sH[21], sN[6], sF = 0.0, sQx = 0.0, sQy = 0.0, sQz = 0.0, sE = 0.0;
  int valid = 0, cand = 0, cvalid = 0;
#pragma unroll
  for (int i = 0; i < 21; i++) sH[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) sN[i] = 0.0;
  const bool colour = p.grey != nullptr;
  const int tw = (p.lw + 7) >> 3, th = (p.lh + 7) >> 3;
  const int jobs = TILES ? tw * th * 64 : p.lw * p.lh;
  for (int job = blockIdx.x * kTrackSdfThreads + threadIdx.x; job < jobs; job += gridDim.x * kTrackSdfThreads) {
    int x, y;
    if (TILES) {
      const int tile = job >> 6, ty = tile / tw;
      x = (tile - ty * tw) * 8 + (job & 7);
      y = ty * 8 + ((job >> 3) & 7);
      if (x >= p.lw || y >= p.lh) continue;
    } else {
      y = job / p.lw;
      x = job - y * p.lw;
    }
    const float D = p.depth[x + (size_t)y * p.lw];
    if (!(D > 1e-8f)) continue;
    cand++;
    Vec3 c;
    c.x = (D * (((float)x - p.cx) / p.fx)) * p.inv_vs;
    c.y = (D * (((float)y - p.cy) / p.fy)) * p.inv_vs;
    c.z = D * p.inv_vs;
    // R c, the point relative to the camera centre t, and p = R c + t (track_sdf_device.h)
    Vec3 rc, pw;
    rc.x = (p.P[0] * c.x + p.P[1] * c.y) + p.P[2] * c.z;
    rc.y = (p.P[4] * c.x + p.P[5] * c.y) + p.P[6] * c.z;
    rc.z = (p.P[8] * c.x + p.P[9] * c.y) + p.P[10] * c.z;
    pw.x = rc.x + p.P[3];
    pw.y = rc.y + p.P[7];
    pw.z = rc.z + p.P[11];
    Blend bd = {0, 0.0f, 0.0f, 0.0f}, bc = {0, 0.0f, 0.0f, 0.0f};
    Blend3 bg = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}}, bh = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    for (int i = 0; i < p.num_maps; i++) {   // (i is the same in every lane: the descriptor is read by scalar loads)
      const MultiMap &m = p.maps[i];
      const Vec3 q = to_map(m, pw);
      // a block coordinate outside the short range is never resident (and this keeps the casts below defined)
      if (!(fabsf(q.x) < 262144.0f && fabsf(q.y) < 262144.0f && fabsf(q.z) < 262144.0f)) continue;
      const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
      const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
      const VolumeRef vol = volume_of(m);
      // tap 0 lies in the block of the cell's base corner: without that block the map cannot pass the gate below
      IndexCache none = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
      if (lookup_block(vol, ix >> 3, iy >> 3, iz >> 3, none) < 0) continue;
      uint2 t[8];
      if (!gather_cell(vol, ix, iy, iz, t)) continue;
      bool ok = true;
      float s[8], w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int raw = (int)(short)(t[k].x & 0xffffu);
        const unsigned wd = (t[k].x >> 16) & 0xffu;
        ok = ok && wd != 0u && raw != 32767 && raw != -32767;
        s[k] = sdf_to_float((short)raw);
        w[k] = (float)wd;
      }
      if (!ok) continue;
      const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
      const float ux = 1.0f - cx, uy = 1.0f - cy, uz = 1.0f - cz;
      {
        const float x00 = ux * s[0] + cx * s[1], x10 = ux * s[2] + cx * s[3];
        const float x01 = ux * s[4] + cx * s[5], x11 = ux * s[6] + cx * s[7];
        const float y0 = uy * x00 + cy * x10, y1 = uy * x01 + cy * x11;
        const float d = uz * y0 + cz * y1;
        Vec3 g;
        g.x = uz * (uy * (s[1] - s[0]) + cy * (s[3] - s[2])) + cz * (uy * (s[5] - s[4]) + cy * (s[7] - s[6]));
        g.y = uz * (x10 - x00) + cz * (x11 - x01);
        g.z = y1 - y0;
        const float w00 = ux * w[0] + cx * w[1], w10 = ux * w[2] + cx * w[3];
        const float w01 = ux * w[4] + cx * w[5], w11 = ux * w[6] + cx * w[7];
        const float om = uz * (uy * w00 + cy * w10) + cz * (uy * w01 + cy * w11);
        if (!m.identity) {   // the gradient in the world frame: R^T g
          const Vec3 gm = g;
          g.x = (m.T[0] * gm.x + m.T[4] * gm.y) + m.T[8] * gm.z;
          g.y = (m.T[1] * gm.x + m.T[5] * gm.y) + m.T[9] * gm.z;
          g.z = (m.T[2] * gm.x + m.T[6] * gm.y) + m.T[10] * gm.z;
        }
        bd.add(d, om);
        bg.add(g, om);
      }
      if (!colour) continue;
      // the colour half of the same 16 words: the arrays above are reused for the taps' greys and colour weights
      bool cok = true;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const unsigned hi = t[k].y, wc = (hi >> 16) & 0xffu;
        cok = cok && wc != 0u;
        s[k] = grey_of(t[k].x >> 24, hi & 0xffu, (hi >> 8) & 0xffu);
        w[k] = (float)wc;
      }
      if (!cok) continue;
      const float x00 = ux * s[0] + cx * s[1], x10 = ux * s[2] + cx * s[3];
      const float x01 = ux * s[4] + cx * s[5], x11 = ux * s[6] + cx * s[7];
      const float y0 = uy * x00 + cy * x10, y1 = uy * x01 + cy * x11;
      const float C = uz * y0 + cz * y1;
      Vec3 h;
      h.x = uz * (uy * (s[1] - s[0]) + cy * (s[3] - s[2])) + cz * (uy * (s[5] - s[4]) + cy * (s[7] - s[6]));
      h.y = uz * (x10 - x00) + cz * (x11 - x01);
      h.z = y1 - y0;
      const float w00 = ux * w[0] + cx * w[1], w10 = ux * w[2] + cx * w[3];
      const float w01 = ux * w[4] + cx * w[5], w11 = ux * w[6] + cx * w[7];
      const float omc = uz * (uy * w00 + cy * w10) + cz * (uy * w01 + cy * w11);
      if (!m.identity) {   // R^T h
        const Vec3 hm = h;
        h.x = (m.T[0] * hm.x + m.T[4] * hm.y) + m.T[8] * hm.z;
        h.y = (m.T[1] * hm.x + m.T[5] * hm.y) + m.T[9] * hm.z;
        h.z = (m.T[2] * hm.x + m.T[6] * hm.y) + m.T[10] * hm.z;
      }
      bc.add(C, omc);
      bh.add(h, omc);
    }
    if (bd.n == 0) continue;
    const float d = bd.value(0.0f);
    const Vec3 g = bg.value();
    if (fabsf(d) > p.residual_gate) continue;
    const float r = -d;
    float A[6];
    A[0] = rc.y * g.z - rc.z * g.y;
    A[1] = rc.z * g.x - rc.x * g.z;
    A[2] = rc.x * g.y - rc.y * g.x;
    A[3] = g.x; A[4] = g.y; A[5] = g.z;
    valid++;
    sF += (double)(r * r);
    sQx += (double)rc.x; sQy += (double)rc.y; sQz += (double)rc.z;
#pragma unroll
    for (int k = 0, c2 = 0; k < 6; k++) {
      sN[k] += (double)(r * A[k]);
#pragma unroll
      for (int j = 0; j <= k; j++, c2++) sH[c2] += (double)(A[k] * A[j]);
    }
    if (bc.n == 0) continue;   // (no colour-ok map; always so on a level without the term)
    const float e = bc.value(0.0f) - p.grey[x + (size_t)y * p.lw];
    if (fabsf(e) > p.colour_gate) continue;
    const Vec3 h = bh.value();
    const float kw = p.colour_weight, rcol = -(kw * e);
    A[0] = kw * (rc.y * h.z - rc.z * h.y);
    A[1] = kw * (rc.z * h.x - rc.x * h.z);
    A[2] = kw * (rc.x * h.y - rc.y * h.x);
    A[3] = kw * h.x; A[4] = kw * h.y; A[5] = kw * h.z;
    cvalid++;
    sE += (double)(e * e);
#pragma unroll
    for (int k = 0, c2 = 0; k < 6; k++) {
      sN[k] += (double)(rcol * A[k]);
#pragma unroll
      for (int j = 0; j <= k; j++, c2++) sH[c2] += (double)(A[k] * A[j]);
    }
  }
  // workgroup reduction in a fixed order: wave shuffle tree, then the four wave partials through LDS.  A workgroup
  // without a pixel arrives here with zeros and writes them.
  __shared__ double red[kRegWaves][kTrackSdfRgbSums];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double vals[kTrackSdfRgbSums];
#pragma unroll
  for (int i = 0; i < 21; i++) vals[i] = sH[i];
#pragma unroll
  for (int i = 0; i < 6; i++) vals[21 + i] = sN[i];
  vals[27] = sF;
  vals[28] = (double)valid;
  vals[29] = sQx; vals[30] = sQy; vals[31] = sQz;
  vals[32] = (double)cand;
  vals[33] = sE;
  vals[34] = (double)cvalid;
#pragma unroll
  for (int i = 0; i < kTrackSdfRgbSums; i++) {
    double v = vals[i];
    for (int dlt = 32; dlt > 0; dlt >>= 1) v += __shfl_down(v, dlt, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kTrackSdfRgbSums) {
    const int i = threadIdx.x;
    double v = red[0][i];
#pragma unroll
    for (int w = 1; w < kRegWaves; w++) v += red[w][i];
    p.partials[(size_t)blockIdx.x * kTrackSdfRgbSums + i] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
namespace {

// the totals of one evaluation and its costs
struct Evaluation35 {
  double sums[kTrackSdfRgbSums];
  int valid, candidates, colour_valid;
  bool term;   // the level carries the photometric term
  void take(const double *totals, bool with_term) {
    memcpy(sums, totals, sizeof sums);
    valid = (int)sums[28]; candidates = (int)sums[32]; colour_valid = (int)sums[34];
    term = with_term;
  }
  double cost_depth(double gate2) const {
    return candidates > 0 ? (sums[27] + (double)(candidates - valid) * gate2) / (double)candidates : gate2;
  }
  double cost_colour(double cgate2) const {
    if (!term) return 0.0;
    return candidates > 0 ? (sums[33] + (double)(candidates - colour_valid) * cgate2) / (double)candidates : cgate2;
  }
};

// the grey pyramid of the view's RGBA image, `levels` levels in one buffer of the view; level pointers to lgrey
int build_grey_pyramid(dslam_engine *e, const dslam_view *v, int levels, const int *lw, const int *lh, const float **lgrey) {
  const size_t n0 = (size_t)v->w_rgb * v->h_rgb;
  if (!v->grey) DSLAM_TRY(v->grey.alloc(n0 + n0 / 2));   // sum of levels 1.. < 1/3 of level 0
  v->grey_levels = 0;
  float *next = v->grey;
  hipLaunchKernelGGL(k_grey_level0, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, e->stream, v->rgba_src, next, (int)n0);
  lgrey[0] = next;
  next += n0;
  for (int i = 1; i < levels; i++) {
    hipLaunchKernelGGL(k_grey_subsample, dim3((lw[i] + 31) / 32, (lh[i] + 7) / 8), dim3(256), 0, e->stream, lgrey[i - 1],
                       lw[i - 1], next, lw[i], lh[i]);
    lgrey[i] = next;
    next += (size_t)lw[i] * lh[i];
  }
  DSLAM_HIP(hipGetLastError());
  v->grey_levels = levels;
  return DSLAM_OK;
}

}  // namespace

int download_track_sdf_rgb_grey(dslam_engine *e, const dslam_view *v, int level, float *out_host) {
  DSLAM_REQUIRE(level >= 0 && level < v->grey_levels, "the most recent dslam_track_camera_sdf_rgb on this view built no such level");
  const float *src = v->grey;
  int w = v->w_rgb, h = v->h_rgb;
  for (int i = 0; i < level; i++) { src += (size_t)w * h; w /= 2; h /= 2; }
  DSLAM_HIP(hipMemcpyAsync(out_host, src, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return DSLAM_OK;
}

// everything already checked (and params defaulted) by dslam_track_camera_sdf_rgb
int launch_track_camera_sdf_rgb(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T, int n,
                                float *pose_M, const float *intr, const dslam_track_sdf_rgb_params *rp,
                                dslam_track_sdf_rgb_result *res) {
  const dslam_track_sdf_params *tp = &rp->base;
  const int levels = tp->no_hierarchy_levels;
  TrackSdfPyramid pyr;
  DSLAM_TRY(pyr.prepare(e, v, intr, levels));
  const float *lgrey[DSLAM_TRACKER_MAX_LEVELS];
  DSLAM_TRY(build_grey_pyramid(e, v, levels, pyr.lw, pyr.lh, lgrey));
  DSLAM_TRY(e->track_sdf_rgb_sums.ensure(kTrackSdfGrid));

  const double vs = (double)scenes[0]->p.voxel_size;
  DSLAM_TRY(upload_posed_maps(e, scenes, T, n, vs));

  TrackSdfRgbParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.inv_vs = (float)(1.0 / vs);
  kp.maps = static_cast<const MultiMap *>(e->map_table.get());
  kp.num_maps = n;
  kp.residual_gate = tp->residual_gate;
  kp.colour_weight = rp->colour_weight;
  kp.colour_gate = rp->colour_gate;
  kp.partials = e->track_sdf_rgb_sums.partials.device();
  const double gate2 = (double)tp->residual_gate * (double)tp->residual_gate;
  const double cgate2 = (double)rp->colour_gate * (double)rp->colour_gate;
  const double k2 = (double)rp->colour_weight * (double)rp->colour_weight;
  const bool tiles = track_sdf_pixels_in_tiles();
  auto cost = [&](const Evaluation35 &ev) { return ev.cost_depth(gate2) + k2 * ev.cost_colour(cgate2); };

  auto evaluate = [&](int level, const double P[12], Evaluation35 &ev) -> int {
    const bool term = level - tp->run_till_level < rp->colour_levels;
    pyr.set_level(kp, level);
    kp.grey = term ? lgrey[level] : nullptr;
    for (int k = 0; k < 12; k++) kp.P[k] = (float)P[k];
    if (tiles) hipLaunchKernelGGL(k_track_sdf_rgb<true>, dim3(kTrackSdfGrid), dim3(kTrackSdfThreads), 0, e->stream, kp);
    else hipLaunchKernelGGL(k_track_sdf_rgb<false>, dim3(kTrackSdfGrid), dim3(kTrackSdfThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    e->track_sdf_rgb_sums.collect(kTrackSdfGrid);
    ev.take(e->track_sdf_rgb_sums.last_sums, term);
    return DSLAM_OK;
  };

  double Mv[12], P[12], c[3];
  voxel_pose(pose_M, vs, Mv);
  rigid_inverse(Mv, P);
  bool accepted_any = false;
  int total_evaluations = 0, levels_stepped = 0;
  // the last level's outcome is the call's
  LmOutcome lm = {0, 3, false, 0.0};
  Evaluation35 good;
  memset(&good, 0, sizeof good);
  double cost_first = 0.0;
  for (int level = levels - 1; level >= tp->run_till_level; level--) {
    DSLAM_TRY(evaluate(level, P, good));
    cost_first = cost(good);
    DSLAM_TRY(lm_iterate(
        6, good.valid >= tp->min_valid, tp->max_evaluations, (double)tp->term_rotation, (double)tp->term_translation_voxels,
        [&](double *H, double *g) { pivot_sums_at_camera(good.sums, P, c, H, g); },   // (the first 33 of the 35)
        [&](const double *y) -> int {
          double trial[12];
          Evaluation35 ev;
          apply_increment(y, c, P, trial);
          DSLAM_TRY(evaluate(level, trial, ev));
          if (!(ev.valid >= tp->min_valid && cost(ev) < cost(good))) return 0;
          memcpy(P, trial, sizeof trial);
          good = ev;
          return 1;
        },
        lm));
    total_evaluations += lm.evaluations;
    if (lm.accepted_any) { accepted_any = true; levels_stepped |= 1 << level; }
  }
  if (accepted_any) {
    rigid_inverse(P, Mv);
    pose_from_voxels(Mv, vs, pose_M);
  }
  res->base.evaluations = total_evaluations;
  res->base.levels_stepped = levels_stepped;
  res->base.stop_reason = lm.stop;
  res->base.candidates = good.candidates;
  res->base.valid_last = good.valid;
  res->base.cost_first = (float)cost_first;
  res->base.cost_last = (float)cost(good);
  res->base.conditioning = (float)lm.conditioning;
  res->colour_valid_last = good.colour_valid;
  res->colour_rms_last = good.colour_valid > 0 ? (float)sqrt(good.sums[33] / (double)good.colour_valid) : 0.0f;
  res->cost_depth_last = (float)good.cost_depth(gate2);
  res->cost_colour_last = (float)good.cost_colour(cgate2);
  return device_errors(e);
}

}  // namespace dslam
