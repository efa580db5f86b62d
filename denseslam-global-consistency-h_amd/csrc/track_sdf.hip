// track_sdf.hip -- the depth-to-SDF camera tracker over all local maps (dslam_track_camera_sdf;
// ITMMainEngine::TrackAllLocalMaps in the mirror).
//
// Reference: none.  The reference tracks by ICP against the points and normals raycast from ONE local map
// (DenseSlam.cpp:198-206; track.hip); the law below is this project's own (stated in full in
// include/dslam_fusion.h).  Every map is only read; no render state, no raycast, no visible list.
//
// One evaluation at P~ (camera -> world, the first three rows, row-major, translation in voxels, float32) on level l of
// the view's depth pyramid: every pixel (x, y) with depth D > 1e-8 (a candidate, counted in N),
//   camera point     c = (D ((x - cx) / fx), D ((y - cy) / fy), D), each component times (float)(1 / voxel_size);
//   world point      p = P~ c (to_map's row order);
//   per map i        q = T~_i p (to_map), a miss for a coordinate of magnitude >= 262144; cell floor(q); the 8-tap gate,
//                    value d_i and gradient g_i of register_body.h; weight w_i: the same three lerp stages on the taps'
//                    w_depth; g_i^w = R_i^T g_i, each component (r0 gx + r1 gy) + r2 gz;
//   combine          Blend / Blend3 of multimap_device.h in list order (one map: its values unchanged);
//   gate             |d| > residual_gate is a miss; else valid with b = -d and the row A = [p x g, g];
//   sums             the 33 doubles of register_body.h with p in place of q.
//
// Device work per evaluation: k_track_sdf, a fixed grid of kTrackSdfGrid workgroups, one lane per pixel in a grid-stride
// loop.  The map descriptors live in an engine-owned device table (64 of them do not fit in kernel arguments); the loop
// over maps has a wave-uniform index, so a descriptor's 80 bytes arrive by scalar loads.  A map whose block at the cell's
// base corner is not resident cannot pass the 8-tap gate: one table probe rules it out before the 16-load gather, so a
// pixel pays for the maps that hold its point and not for num_maps.  Accumulation and reduction are register_body.h's:
// per-lane doubles of float32 products, wave shuffle tree, the four wave partials through LDS in index order, one row of
// 33 per workgroup in mapped page-locked memory (a workgroup without a pixel writes zeros), rows added by the host in
// index order.  No atomics; the same bytes on every run.  The iteration is lm_iterate of register_host.h, on the host in
// double, once per pyramid level; this file's own are the kernel, the level loop and levels_stepped.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "register_device.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {

constexpr int kTrackSdfGrid = 512;      // workgroups: two per CU of an MI355X.  512 x 256 = 131072 lanes, so a level of
                                        // more than 131072 pixels (640 x 480 has 307200) takes further trips of the loop
constexpr int kTrackSdfThreads = kRegThreads;

struct TrackSdfParams {
  const float *depth;        // level l of the pyramid, lw x lh
  int lw, lh;
  float fx, fy, cx, cy;      // the intrinsics of the level
  float inv_vs;              // (float)(1.0 / (double)voxel_size)
  float P[12];               // P~
  const MultiMap *maps;      // [num_maps], device
  int num_maps;
  float residual_gate;
  double *partials;          // [gridDim.x][kRegSums]
};

// TILES: lane t of a wave takes pixel (t & 7, t >> 3) of an 8 x 8 tile (tiles in row-major order, those on the right
// and bottom edges partly outside the image); otherwise consecutive lanes take consecutive pixels of a row.
template <bool TILES>
__global__ __launch_bounds__(kTrackSdfThreads) void k_track_sdf(TrackSdfParams p) {
  double sH[21], sN[6], sF = 0.0, sQx = 0.0, sQy = 0.0, sQz = 0.0;
  int valid = 0, cand = 0;
#pragma unroll
  for (int i = 0; i < 21; i++) sH[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) sN[i] = 0.0;
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
    Vec3 pw;
    pw.x = ((p.P[0] * c.x + p.P[1] * c.y) + p.P[2] * c.z) + p.P[3];
    pw.y = ((p.P[4] * c.x + p.P[5] * c.y) + p.P[6] * c.z) + p.P[7];
    pw.z = ((p.P[8] * c.x + p.P[9] * c.y) + p.P[10] * c.z) + p.P[11];
    Blend bd = {0, 0.0f, 0.0f, 0.0f};
    Blend3 bg = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
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
    if (bd.n == 0) continue;
    const float d = bd.value(0.0f);
    const Vec3 g = bg.value();
    if (fabsf(d) > p.residual_gate) continue;
    const float r = -d;
    float A[6];
    A[0] = pw.y * g.z - pw.z * g.y;
    A[1] = pw.z * g.x - pw.x * g.z;
    A[2] = pw.x * g.y - pw.y * g.x;
    A[3] = g.x; A[4] = g.y; A[5] = g.z;
    valid++;
    sF += (double)(r * r);
    sQx += (double)pw.x; sQy += (double)pw.y; sQz += (double)pw.z;
#pragma unroll
    for (int k = 0, c2 = 0; k < 6; k++) {
      sN[k] += (double)(r * A[k]);
#pragma unroll
      for (int j = 0; j <= k; j++, c2++) sH[c2] += (double)(A[k] * A[j]);
    }
  }
  // workgroup reduction in a fixed order: wave shuffle tree, then the four wave partials through LDS.  A workgroup
  // without a pixel arrives here with zeros and writes them.
  __shared__ double red[kRegWaves][kRegSums];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double vals[kRegSums];
#pragma unroll
  for (int i = 0; i < 21; i++) vals[i] = sH[i];
#pragma unroll
  for (int i = 0; i < 6; i++) vals[21 + i] = sN[i];
  vals[27] = sF;
  vals[28] = (double)valid;
  vals[29] = sQx; vals[30] = sQy; vals[31] = sQz;
  vals[32] = (double)cand;
#pragma unroll
  for (int i = 0; i < kRegSums; i++) {
    double v = vals[i];
    for (int dlt = 32; dlt > 0; dlt >>= 1) v += __shfl_down(v, dlt, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kRegSums) {
    const int i = threadIdx.x;
    double v = red[0][i];
#pragma unroll
    for (int w = 1; w < kRegWaves; w++) v += red[w][i];
    p.partials[(size_t)blockIdx.x * kRegSums + i] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
namespace {

// Which pixel takes which lane.  Measured on the MI355X (harness/track_sdf_bench.py); the
// environment variable DSLAM_TRACK_SDF_PIXELS=rows|tiles is that measurement's switch and nothing else reads it.
bool pixels_in_tiles() {
  static const bool tiles = [] {
    const char *v = getenv("DSLAM_TRACK_SDF_PIXELS");
    return v ? strcmp(v, "rows") != 0 : true;
  }();
  return tiles;
}

}  // namespace

// everything already checked (and params defaulted) by dslam_track_camera_sdf
int launch_track_camera_sdf(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T, int n,
                            float *pose_M, const float *intr, const dslam_track_sdf_params *tp, dslam_track_sdf_result *res) {
  DSLAM_TRY(ensure_view_depth(e, v));
  const int levels = tp->no_hierarchy_levels;
  const float *ldepth[DSLAM_TRACKER_MAX_LEVELS];
  int lw[DSLAM_TRACKER_MAX_LEVELS], lh[DSLAM_TRACKER_MAX_LEVELS];
  float lintr[DSLAM_TRACKER_MAX_LEVELS][4];
  DSLAM_TRY(build_depth_pyramid(e, v, levels, ldepth, lw, lh));
  for (int k = 0; k < 4; k++) lintr[0][k] = intr[k];
  for (int i = 1; i < levels; i++)
    for (int k = 0; k < 4; k++) lintr[i][k] = lintr[i - 1][k] * 0.5f;
  DSLAM_TRY(e->track_sdf_sums.ensure(kTrackSdfGrid));

  const double vs = (double)scenes[0]->p.voxel_size;
  MultiMap maps[DSLAM_MAX_RENDER_MAPS];
  for (int i = 0; i < n; i++) maps[i] = posed_map(scenes[i], T + 16 * i, vs);
  DSLAM_HIP(hipMemcpyAsync(e->map_table, maps, (size_t)n * sizeof(MultiMap), hipMemcpyHostToDevice, e->stream));

  TrackSdfParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.inv_vs = (float)(1.0 / vs);
  kp.maps = static_cast<const MultiMap *>(e->map_table.get());
  kp.num_maps = n;
  kp.residual_gate = tp->residual_gate;
  kp.partials = e->track_sdf_sums.partials.device();
  const double gate2 = (double)tp->residual_gate * (double)tp->residual_gate;
  const bool tiles = pixels_in_tiles();

  auto evaluate = [&](int level, const double P[12], Evaluation33 &ev) -> int {
    kp.depth = ldepth[level]; kp.lw = lw[level]; kp.lh = lh[level];
    kp.fx = lintr[level][0]; kp.fy = lintr[level][1]; kp.cx = lintr[level][2]; kp.cy = lintr[level][3];
    for (int k = 0; k < 12; k++) kp.P[k] = (float)P[k];
    if (tiles) hipLaunchKernelGGL(k_track_sdf<true>, dim3(kTrackSdfGrid), dim3(kTrackSdfThreads), 0, e->stream, kp);
    else hipLaunchKernelGGL(k_track_sdf<false>, dim3(kTrackSdfGrid), dim3(kTrackSdfThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    e->track_sdf_sums.collect(kTrackSdfGrid, ev);
    return DSLAM_OK;
  };

  double Mv[12], P[12], c[3];
  voxel_pose(pose_M, vs, Mv);
  rigid_inverse(Mv, P);
  bool accepted_any = false;
  int total_evaluations = 0, levels_stepped = 0;
  // the last level's outcome is the call's (no level at all: stop reason 3, everything else zero)
  LmOutcome lm = {0, 3, false, 0.0};
  Evaluation33 good;
  memset(&good, 0, sizeof good);
  double cost_first = 0.0, cost_last = 0.0;
  for (int level = levels - 1; level >= tp->run_till_level; level--) {
    DSLAM_TRY(evaluate(level, P, good));
    cost_first = good.gated_cost(gate2);
    DSLAM_TRY(lm_iterate(
        6, good.valid >= tp->min_valid, tp->max_evaluations, (double)tp->term_rotation, (double)tp->term_translation_voxels,
        [&](double *H, double *g) { pivot_sums(good.sums, c, H, g); },
        [&](const double *y) -> int {
          double trial[12];
          Evaluation33 ev;
          apply_increment(y, c, P, trial);
          DSLAM_TRY(evaluate(level, trial, ev));
          if (!(ev.valid >= tp->min_valid && ev.gated_cost(gate2) < good.gated_cost(gate2))) return 0;
          memcpy(P, trial, sizeof trial);
          good = ev;
          return 1;
        },
        lm));
    total_evaluations += lm.evaluations;
    if (lm.accepted_any) { accepted_any = true; levels_stepped |= 1 << level; }
    cost_last = good.gated_cost(gate2);
  }
  if (accepted_any) {
    rigid_inverse(P, Mv);
    pose_from_voxels(Mv, vs, pose_M);
  }
  res->evaluations = total_evaluations;
  res->levels_stepped = levels_stepped;
  res->stop_reason = lm.stop;
  res->candidates = good.candidates;
  res->valid_last = good.valid;
  res->cost_first = (float)cost_first;
  res->cost_last = (float)cost_last;
  res->conditioning = (float)lm.conditioning;
  return device_errors(e);
}

}  // namespace dslam
