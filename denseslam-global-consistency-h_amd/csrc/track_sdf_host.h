// track_sdf_host.h -- what the two depth-to-SDF trackers set up alike on the host, stated once for track_sdf.hip
// (dslam_track_camera_sdf) and track_sdf_starts.hip (dslam_score_camera_poses, dslam_track_camera_sdf_starts): the depth
// pyramid with its per-level intrinsics, the level's part of the kernel arguments, and the result of one tracked pose.
// Host only: nothing here is device code, and both kernels' parameter structs stay where they are.
#pragma once
#include "dslam_internal.h"
#include "register_host.h"

namespace dslam {

// the view's depth in metres as a pyramid of `levels` levels; level i has the intrinsics of level i - 1 halved
struct TrackSdfPyramid {
  const float *ldepth[DSLAM_TRACKER_MAX_LEVELS];
  int lw[DSLAM_TRACKER_MAX_LEVELS], lh[DSLAM_TRACKER_MAX_LEVELS];
  float lintr[DSLAM_TRACKER_MAX_LEVELS][4];

  int prepare(dslam_engine *e, const dslam_view *v, const float *intr, int levels) {
    DSLAM_TRY(ensure_view_depth(e, v));
    DSLAM_TRY(build_depth_pyramid(e, v, levels, ldepth, lw, lh));
    for (int k = 0; k < 4; k++) lintr[0][k] = intr[k];
    for (int i = 1; i < levels; i++)
      for (int k = 0; k < 4; k++) lintr[i][k] = lintr[i - 1][k] * 0.5f;
    return DSLAM_OK;
  }

  // depth, size and intrinsics of `level` in the arguments of either kernel (TrackSdfParams, TrackSdfStartsParams)
  template <class Params>
  void set_level(Params &kp, int level) const {
    kp.depth = ldepth[level]; kp.lw = lw[level]; kp.lh = lh[level];
    kp.fx = lintr[level][0]; kp.fy = lintr[level][1]; kp.cx = lintr[level][2]; kp.cy = lintr[level][3];
  }
};

// The system of an evaluation's sums at its centroid.  The kernels form the rotation part of a row and sums 29..31 from
// R c = p - t, the point relative to the camera centre t (the float32 translation of the P~ that was evaluated; P is the
// double it was rounded from): pivot_sums' centroid is therefore relative to t, and H_c, g_c are what they would be had the
// rows been formed at the world origin in exact arithmetic.  c: the centroid in the world (voxels, double), the pivot
// apply_increment turns about.
inline void pivot_sums_at_camera(const double sums[kRegSums], const double P[12], double c[3], double Hc[36], double gc[6]) {
  pivot_sums(sums, c, Hc, gc);
  for (int i = 0; i < 3; i++) c[i] += (double)(float)P[i * 4 + 3];
}

// the result of one tracked pose: evaluations over all levels, the levels that took a step; of the last level its outcome,
// its accepted evaluation, the cost it started with and the cost it ended with
inline void fill_track_sdf_result(dslam_track_sdf_result *res, int evaluations, int levels_stepped, const LmOutcome &lm,
                                  const Evaluation33 &good, double cost_first, double cost_last) {
  res->evaluations = evaluations;
  res->levels_stepped = levels_stepped;
  res->stop_reason = lm.stop;
  res->candidates = good.candidates;
  res->valid_last = good.valid;
  res->cost_first = (float)cost_first;
  res->cost_last = (float)cost_last;
  res->conditioning = (float)lm.conditioning;
}

}  // namespace dslam
