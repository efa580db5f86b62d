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
//   world point      p = P~ c (to_map's row order); r = R c, the three-term sum before the translation t is added, is kept;
//   per map i        q = T~_i p (to_map), a miss for a coordinate of magnitude >= 262144; cell floor(q); the 8-tap gate,
//                    value d_i and gradient g_i of register_body.h; weight w_i: the same three lerp stages on the taps'
//                    w_depth; g_i^w = R_i^T g_i, each component (r0 gx + r1 gy) + r2 gz;
//   combine          Blend / Blend3 of multimap_device.h in list order (one map: its values unchanged);
//   gate             |d| > residual_gate is a miss; else valid with b = -d and the row A = [r x g, g]: pivoted at the camera
//                    centre, so that no float32 product has an operand of the size of the camera's position (DESIGN.md
//                    section 28: with p x g the conditioning is wrong from block 8000 on and the track is lost at the
//                    table's ends);
//   sums             the 33 doubles of register_body.h with r in place of q; the host adds t back (pivot_sums_at_camera).
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
#include "track_sdf_host.h"

#pragma clang fp contract(off)

namespace dslam {

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

// One lane per pixel in a grid-stride loop; the body is track_sdf_device.h's (TILES: which pixel takes which lane).
template <bool TILES>
__global__ __launch_bounds__(kTrackSdfThreads) void k_track_sdf(TrackSdfParams p) {
#define DSLAM_TRACK_SDF_POSE(k) p.P[k]
#define DSLAM_TRACK_SDF_FIRST (blockIdx.x * kTrackSdfThreads + threadIdx.x)
#define DSLAM_TRACK_SDF_STRIDE (gridDim.x * kTrackSdfThreads)
#define DSLAM_TRACK_SDF_ROW blockIdx.x
#include "track_sdf_device.h"
#undef DSLAM_TRACK_SDF_POSE
#undef DSLAM_TRACK_SDF_FIRST
#undef DSLAM_TRACK_SDF_STRIDE
#undef DSLAM_TRACK_SDF_ROW
}

// ---- host side ------------------------------------------------------------------------------------------------
// Which pixel takes which lane (also track_sdf_starts.hip's).  Measured on the MI355X (harness/track_sdf_bench.py, DESIGN.md
// section 18); the environment variable DSLAM_TRACK_SDF_PIXELS=rows|tiles is that measurement's switch and nothing else
// reads it.
bool track_sdf_pixels_in_tiles() {
  static const bool tiles = [] {
    const char *v = getenv("DSLAM_TRACK_SDF_PIXELS");
    return v ? strcmp(v, "rows") != 0 : true;
  }();
  return tiles;
}

// everything already checked (and params defaulted) by dslam_track_camera_sdf
int launch_track_camera_sdf(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T, int n,
                            float *pose_M, const float *intr, const dslam_track_sdf_params *tp, dslam_track_sdf_result *res) {
  const int levels = tp->no_hierarchy_levels;
  TrackSdfPyramid pyr;
  DSLAM_TRY(pyr.prepare(e, v, intr, levels));
  DSLAM_TRY(e->track_sdf_sums.ensure(kTrackSdfGrid));

  const double vs = (double)scenes[0]->p.voxel_size;
  DSLAM_TRY(upload_posed_maps(e, scenes, T, n, vs));

  TrackSdfParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.inv_vs = (float)(1.0 / vs);
  kp.maps = static_cast<const MultiMap *>(e->map_table.get());
  kp.num_maps = n;
  kp.residual_gate = tp->residual_gate;
  kp.partials = e->track_sdf_sums.partials.device();
  const double gate2 = (double)tp->residual_gate * (double)tp->residual_gate;
  const bool tiles = track_sdf_pixels_in_tiles();

  auto evaluate = [&](int level, const double P[12], Evaluation33 &ev) -> int {
    pyr.set_level(kp, level);
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
        [&](double *H, double *g) { pivot_sums_at_camera(good.sums, P, c, H, g); },
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
  fill_track_sdf_result(res, total_evaluations, levels_stepped, lm, good, cost_first, cost_last);
  return device_errors(e);
}

}  // namespace dslam
