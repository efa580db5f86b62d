// track_sdf_starts.hip -- the depth-to-SDF tracker from many poses at once (dslam_score_camera_poses,
// dslam_track_camera_sdf_starts; ITMMainEngine::RelocaliseAllLocalMaps in the mirror), and the two host functions that make
// a relocaliser of them (dslam_select_start_poses, dslam_camera_pose_lattice).
//
// Reference: none.  The law of one evaluation is dslam_track_camera_sdf's (track_sdf.hip; stated in full in
// include/dslam_fusion.h), and what these calls promise is that call's bytes.
//
// Device work per round of evaluations: k_track_sdf_starts on a grid (G, poses of the round).  blockIdx.y selects the pose
// -- its 12 floats come from an engine-owned device table by scalar loads --, blockIdx.x is the workgroup within the pose.
// The body is track_sdf_device.h's, the single call's, on the single call's partition: the same job -> lane mapping, a
// fixed stride of kTrackSdfGrid x kTrackSdfThreads jobs per trip whatever grid was launched, the same shuffle tree and LDS
// order, one row of 33 doubles per workgroup.  Of the single call's 512 workgroups those without a job write rows of +0.0,
// and x + (+0.0) == x for every x a sum from +0.0 can reach (-0.0 is not among them); so only
// G = min(512, ceil(jobs / 256)) are launched.  The rows stay in device memory; k_track_sdf_row_sum adds each pose's rows in
// index order from +0.0, one lane per (pose, sum), plain IEEE double adds, and writes [poses][33] to mapped page-locked
// memory.  No atomics; the same bytes on every run.
// Host: the iteration is LmStepper of register_host.h -- the rules lm_iterate runs for the single call -- once per start,
// advanced in lock-step: per pyramid level a round evaluates the trial poses of the starts that have not stopped at that
// level, as a compacted list.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "register_device.h"
#include "register_host.h"
#include "track_sdf_host.h"

#pragma clang fp contract(off)

namespace dslam {

struct TrackSdfStartsParams {
  const float *depth;        // level l of the pyramid, lw x lh
  int lw, lh;
  float fx, fy, cx, cy;      // the intrinsics of the level
  float inv_vs;              // (float)(1.0 / (double)voxel_size)
  const float *poses;        // [gridDim.y][12]: the P~ of the round, device
  const MultiMap *maps;      // [num_maps], device
  int num_maps;
  float residual_gate;
  double *partials;          // [gridDim.y][gridDim.x][kRegSums], device
};

template <bool TILES>
__global__ __launch_bounds__(kTrackSdfThreads) void k_track_sdf_starts(TrackSdfStartsParams p) {
  const float *P = p.poses + 12 * blockIdx.y;   // (the same in every lane, read before any store: scalar loads)
#define DSLAM_TRACK_SDF_POSE(k) P[k]
#define DSLAM_TRACK_SDF_FIRST (blockIdx.x * kTrackSdfThreads + threadIdx.x)
#define DSLAM_TRACK_SDF_STRIDE (kTrackSdfGrid * kTrackSdfThreads)
#define DSLAM_TRACK_SDF_ROW (blockIdx.y * gridDim.x + blockIdx.x)
#include "track_sdf_device.h"
#undef DSLAM_TRACK_SDF_POSE
#undef DSLAM_TRACK_SDF_FIRST
#undef DSLAM_TRACK_SDF_STRIDE
#undef DSLAM_TRACK_SDF_ROW
}

// totals[k][i] = ((+0.0 + rows[k][0][i]) + rows[k][1][i]) + ...: lane per (pose, sum).  The adds are one chain in index
// order; the loads do not depend on it and go out kRowSumBatch at a time (one at a time the 512 rows of a level-0 pose cost
// 512 memory latencies: 150 us measured, against 36 us for the kernel that wrote them).
constexpr int kRowSumBatch = 32;
__global__ __launch_bounds__(256) void k_track_sdf_row_sum(const double *__restrict__ rows, int rows_per_pose, int poses,
                                                           double *__restrict__ totals) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= poses * kRegSums) return;
  const int k = idx / kRegSums, i = idx - k * kRegSums;
  const double *r = rows + (size_t)k * rows_per_pose * kRegSums + i;
  double v = 0.0;
  int g = 0;
  for (; g + kRowSumBatch <= rows_per_pose; g += kRowSumBatch) {
    double t[kRowSumBatch];
#pragma unroll
    for (int u = 0; u < kRowSumBatch; u++) t[u] = r[(size_t)(g + u) * kRegSums];
#pragma unroll
    for (int u = 0; u < kRowSumBatch; u++) v += t[u];
  }
  for (; g < rows_per_pose; g++) v += r[(size_t)g * kRegSums];
  totals[idx] = v;
}

// ---- host side ------------------------------------------------------------------------------------------------
namespace {

// Where a pose's workgroup rows are added.  Measured on the MI355X (harness/track_starts_bench.py); the
// environment variable DSLAM_TRACK_STARTS_ROWS=host|device is that measurement's switch and nothing else reads it: with
// `host` the rows go to mapped page-locked memory and the host adds them in index order -- the same bytes, more PCIe.
bool rows_added_on_host() {
  static const bool host = [] {
    const char *v = getenv("DSLAM_TRACK_STARTS_ROWS");
    return v ? strcmp(v, "host") == 0 : false;
  }();
  return host;
}

// what a call evaluates on: the pyramid, the maps' table, the kernel's constant arguments
struct StartsCall {
  dslam_engine *e;
  TrackSdfPyramid pyr;
  TrackSdfStartsParams kp;
  bool tiles, rows_to_host;

  int prepare(dslam_engine *engine, const dslam_view *v, const dslam_scene *const *scenes, const float *T, int n, const float *intr,
              int levels, float residual_gate) {
    e = engine;
    DSLAM_TRY(pyr.prepare(e, v, intr, levels));
    TrackStartsScratch &sc = e->track_starts;
    if (!sc.sums) {
      TrackStartsScratch made;
      DSLAM_TRY(made.poses_host.alloc((size_t)DSLAM_MAX_TRACK_STARTS * 12));
      DSLAM_TRY(made.poses.alloc((size_t)DSLAM_MAX_TRACK_STARTS * 12));
      DSLAM_TRY(made.sums.alloc((size_t)DSLAM_MAX_TRACK_STARTS * kRegSums, hipHostMallocMapped));
      made.last_sums = std::move(sc.last_sums);
      sc = std::move(made);
    }
    const double vs = (double)scenes[0]->p.voxel_size;
    DSLAM_TRY(upload_posed_maps(e, scenes, T, n, vs));
    memset(&kp, 0, sizeof(kp));
    kp.inv_vs = (float)(1.0 / vs);
    kp.poses = sc.poses;
    kp.maps = static_cast<const MultiMap *>(e->map_table.get());
    kp.num_maps = n;
    kp.residual_gate = residual_gate;
    tiles = track_sdf_pixels_in_tiles();
    rows_to_host = rows_added_on_host();
    return DSLAM_OK;
  }

  // workgroups per pose on `level`: those of the single call's 512 that have a job
  int workgroups(int level) const {
    const int lw = pyr.lw[level], lh = pyr.lh[level];
    const long long jobs = tiles ? (long long)((lw + 7) >> 3) * ((lh + 7) >> 3) * 64 : (long long)lw * lh;
    return (int)std::max(1LL, std::min((long long)kTrackSdfGrid, (jobs + kTrackSdfThreads - 1) / kTrackSdfThreads));
  }

  // one round: pose k of the round is P[which[k]] (3 x 4 row-major double, rounded to float32 here); ev[k] its totals
  int evaluate(int level, const std::vector<const double *> &P, std::vector<Evaluation33> &ev) {
    const int poses = (int)P.size();
    TrackStartsScratch &sc = e->track_starts;
    const int G = workgroups(level);
    const size_t need = (size_t)poses * G * kRegSums;
    if (rows_to_host) {
      if (need > sc.rows_host_capacity) {
        DSLAM_TRY(sc.rows_host.alloc(need, hipHostMallocMapped));
        sc.rows_host_capacity = need;
      }
    } else if (need > sc.rows_capacity) {   // (nothing is in flight: every round ends with a wait for the stream)
      DSLAM_TRY(sc.rows.alloc(need));
      sc.rows_capacity = need;
    }
    float *ph = sc.poses_host;
    for (int k = 0; k < poses; k++)
      for (int i = 0; i < 12; i++) ph[12 * k + i] = (float)P[k][i];
    DSLAM_HIP(hipMemcpyAsync(sc.poses, ph, (size_t)poses * 12 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    pyr.set_level(kp, level);
    kp.partials = rows_to_host ? sc.rows_host.device() : sc.rows.get();
    if (tiles) hipLaunchKernelGGL(k_track_sdf_starts<true>, dim3(G, poses), dim3(kTrackSdfThreads), 0, e->stream, kp);
    else hipLaunchKernelGGL(k_track_sdf_starts<false>, dim3(G, poses), dim3(kTrackSdfThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    ev.resize(poses);
    if (rows_to_host) {   // the measurement's other side: the rows over PCIe, added here as the single call adds its 512
      DSLAM_HIP(hipStreamSynchronize(e->stream));
      for (int k = 0; k < poses; k++) ev[k].sum_rows(sc.rows_host, k * G, G);
      return DSLAM_OK;
    }
    hipLaunchKernelGGL(k_track_sdf_row_sum, dim3((poses * kRegSums + 255) / 256), dim3(256), 0, e->stream,
                       static_cast<const double *>(sc.rows.get()), G, poses, sc.sums.device());
    DSLAM_HIP(hipGetLastError());
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    const double *totals = sc.sums;
    for (int k = 0; k < poses; k++) ev[k].sum_rows(totals + (size_t)k * kRegSums, 0, 1);   // (+0.0 + x == x: the totals as they are)
    return DSLAM_OK;
  }
};

}  // namespace

int launch_score_camera_poses(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T, int n,
                              const float *poses_M, int num_poses, const float *intr, int level, float residual_gate,
                              dslam_pose_score *scores_out) {
  StartsCall call;
  DSLAM_TRY(call.prepare(e, v, scenes, T, n, intr, level + 1, residual_gate));
  const double vs = (double)scenes[0]->p.voxel_size;
  std::vector<double> P((size_t)num_poses * 12);
  std::vector<const double *> list(num_poses);
  for (int k = 0; k < num_poses; k++) {
    double Mv[12];
    voxel_pose(poses_M + 16 * k, vs, Mv);
    rigid_inverse(Mv, &P[(size_t)k * 12]);
    list[k] = &P[(size_t)k * 12];
  }
  std::vector<Evaluation33> ev;
  DSLAM_TRY(call.evaluate(level, list, ev));
  DSLAM_TRY(device_errors(e));
  const double gate2 = (double)residual_gate * (double)residual_gate;
  for (int k = 0; k < num_poses; k++) {
    scores_out[k].candidates = ev[k].candidates;
    scores_out[k].valid = ev[k].valid;
    scores_out[k].cost = (float)ev[k].gated_cost(gate2);
    scores_out[k].pad = 0;
  }
  return DSLAM_OK;
}

int launch_track_camera_sdf_starts(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T, int n,
                                   float *poses_M, int num_starts, const float *intr, const dslam_track_sdf_params *tp,
                                   dslam_track_sdf_result *results) {
  StartsCall call;
  DSLAM_TRY(call.prepare(e, v, scenes, T, n, intr, tp->no_hierarchy_levels, tp->residual_gate));
  const double vs = (double)scenes[0]->p.voxel_size;
  const double gate2 = (double)tp->residual_gate * (double)tp->residual_gate;
  // one start's state: what launch_track_camera_sdf keeps on its stack
  struct Start {
    double P[12], trial[12], c[3];
    Evaluation33 good;
    LmStepper lm;
    bool accepted_any = false;
    int total_evaluations = 0, levels_stepped = 0;
    double cost_first = 0.0, cost_last = 0.0;
  };
  std::vector<Start> starts(num_starts);
  std::vector<double> last((size_t)num_starts * kRegSums);
  for (int k = 0; k < num_starts; k++) {
    double Mv[12];
    voxel_pose(poses_M + 16 * k, vs, Mv);
    rigid_inverse(Mv, starts[k].P);
    memset(&starts[k].good, 0, sizeof(Evaluation33));
  }
  std::vector<int> active(num_starts);
  std::vector<const double *> list;
  std::vector<Evaluation33> ev;
  // evaluates the listed starts at P or at their trials, and keeps each one's sums as its most recent evaluation
  auto round = [&](int level, bool trials) -> int {
    list.clear();
    for (int k : active) list.push_back(trials ? starts[k].trial : starts[k].P);
    DSLAM_TRY(call.evaluate(level, list, ev));
    for (size_t a = 0; a < active.size(); a++) memcpy(&last[(size_t)active[a] * kRegSums], ev[a].sums, sizeof ev[a].sums);
    return DSLAM_OK;
  };
  for (int level = tp->no_hierarchy_levels - 1; level >= tp->run_till_level; level--) {
    active.resize(num_starts);
    std::iota(active.begin(), active.end(), 0);
    DSLAM_TRY(round(level, false));
    for (int k = 0; k < num_starts; k++) {
      Start &s = starts[k];
      s.good = ev[k];
      s.cost_first = s.good.gated_cost(gate2);
      s.lm.begin(6, s.good.valid >= tp->min_valid, tp->max_evaluations, (double)tp->term_rotation, (double)tp->term_translation_voxels);
    }
    for (;;) {
      active.clear();
      for (int k = 0; k < num_starts; k++) {
        Start &s = starts[k];
        if (!s.lm.propose([&](double *H, double *g) { pivot_sums_at_camera(s.good.sums, s.P, s.c, H, g); })) continue;
        apply_increment(s.lm.increment(), s.c, s.P, s.trial);
        active.push_back(k);
      }
      if (active.empty()) break;
      DSLAM_TRY(round(level, true));
      for (size_t a = 0; a < active.size(); a++) {
        Start &s = starts[active[a]];
        const bool adopted = ev[a].valid >= tp->min_valid && ev[a].gated_cost(gate2) < s.good.gated_cost(gate2);
        if (adopted) {
          memcpy(s.P, s.trial, sizeof s.trial);
          s.good = ev[a];
        }
        s.lm.verdict(adopted);
      }
    }
    for (int k = 0; k < num_starts; k++) {
      Start &s = starts[k];
      s.lm.finish([&](double *H, double *g) { pivot_sums_at_camera(s.good.sums, s.P, s.c, H, g); });
      s.total_evaluations += s.lm.out.evaluations;
      if (s.lm.out.accepted_any) { s.accepted_any = true; s.levels_stepped |= 1 << level; }
      s.cost_last = s.good.gated_cost(gate2);
    }
  }
  DSLAM_TRY(device_errors(e));
  for (int k = 0; k < num_starts; k++) {
    const Start &s = starts[k];
    if (s.accepted_any) {
      double Mv[12];
      rigid_inverse(s.P, Mv);
      pose_from_voxels(Mv, vs, poses_M + 16 * k);
    }
    fill_track_sdf_result(results + k, s.total_evaluations, s.levels_stepped, s.lm.out, s.good, s.cost_first, s.cost_last);
  }
  e->track_starts.last_sums = std::move(last);
  return DSLAM_OK;
}

// ---- the host functions ------------------------------------------------------------------------------------------------
// arguments already checked by dslam_select_start_poses
void select_start_poses(const dslam_pose_score *scores, int num, int min_valid, int max_keep, int32_t *kept_out, int32_t *num_kept_out) {
  std::vector<int> order;
  for (int k = 0; k < num; k++)
    if (scores[k].valid >= min_valid && !std::isnan(scores[k].cost)) order.push_back(k);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return scores[a].cost < scores[b].cost; });
  const int kept = std::min((int)order.size(), max_keep);
  for (int k = 0; k < kept; k++) kept_out[k] = order[k];
  *num_kept_out = kept;
}

// arguments already checked by dslam_camera_pose_lattice, which has also filled count_out
void camera_pose_lattice(const float pose_M[16], const dslam_pose_lattice &l, float *poses_out) {
  // world -> camera: rows of Rm, translation t; camera -> world: R = Rm^T, c = -R t
  double Rm[9], t[3], R[9], c[3];
  for (int r = 0; r < 3; r++) {
    for (int col = 0; col < 3; col++) Rm[r * 3 + col] = (double)pose_M[col * 4 + r];
    t[r] = (double)pose_M[12 + r];
  }
  for (int r = 0; r < 3; r++) {
    for (int col = 0; col < 3; col++) R[r * 3 + col] = Rm[col * 3 + r];
    c[r] = -((Rm[0 * 3 + r] * t[0] + Rm[1 * 3 + r] * t[1]) + Rm[2 * 3 + r] * t[2]);
  }
  double ax[3] = {0.0, 0.0, 0.0};
  if (l.nr > 0) {
    const double len = sqrt((double)l.axis[0] * l.axis[0] + (double)l.axis[1] * l.axis[1] + (double)l.axis[2] * l.axis[2]);
    for (int k = 0; k < 3; k++) ax[k] = (double)l.axis[k] / len;
  }
  float *out = poses_out;
  for (int ir = -l.nr; ir <= l.nr; ir++) {
    // Rot(a^, angle) = I + sin K + (1 - cos) K^2, K = [a^]x
    const double angle = (double)ir * (double)l.step_r, sn = sin(angle), cs = 1.0 - cos(angle);
    const double K[9] = {0.0, -ax[2], ax[1], ax[2], 0.0, -ax[0], -ax[1], ax[0], 0.0};
    double Rot[9], Rn[9];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double k2 = 0.0;
        for (int k = 0; k < 3; k++) k2 += K[i * 3 + k] * K[k * 3 + j];
        Rot[i * 3 + j] = (i == j ? 1.0 : 0.0) + sn * K[i * 3 + j] + cs * k2;
      }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double acc = 0.0;
        for (int k = 0; k < 3; k++) acc += Rot[i * 3 + k] * R[k * 3 + j];
        Rn[i * 3 + j] = acc;
      }
    for (int iz = -l.nt[2]; iz <= l.nt[2]; iz++)
      for (int iy = -l.nt[1]; iy <= l.nt[1]; iy++)
        for (int ix = -l.nt[0]; ix <= l.nt[0]; ix++, out += 16) {
          if (ir == 0 && iz == 0 && iy == 0 && ix == 0) { memcpy(out, pose_M, 16 * sizeof(float)); continue; }
          const double cn[3] = {c[0] + (double)l.step_t * ix, c[1] + (double)l.step_t * iy, c[2] + (double)l.step_t * iz};
          // world -> camera of the node: (Rn^T, -Rn^T cn), column-major
          for (int r = 0; r < 3; r++) {
            for (int col = 0; col < 3; col++) out[col * 4 + r] = (float)Rn[col * 3 + r];
            out[12 + r] = (float)-((Rn[0 * 3 + r] * cn[0] + Rn[1 * 3 + r] * cn[1]) + Rn[2 * 3 + r] * cn[2]);
            out[r * 4 + 3] = 0.0f;
          }
          out[15] = 1.0f;
        }
  }
}

}  // namespace dslam
