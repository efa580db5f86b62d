// register_graph.hip -- joint SDF-to-SDF alignment of N local maps from a list of overlapping pairs (dslam_register_graph;
// ITMMainEngine::AlignLocalMaps in the mirror).
//
// Reference: none.  The law is this project's own (include/dslam_fusion.h states it in full): one
// Levenberg-Marquardt problem over the poses of all maps but the anchor, every pair evaluated by dslam_register_maps' law
// (section 13, register_device.h) at X~_p = T~_d inv(T~_s).  All maps are only read.
//
// Device work per call: one ordered compaction of the resident entries of every distinct source map (fill_live_lists,
// live_list.hip) into the engine's live lists, one read-back of the counts; per evaluation k_register_graph, once: a fixed grid of
// kRegGrid workgroups, cut by the host into one contiguous range per pair in proportion to the sources' live blocks
// (split_workgroups).  Workgroup w of a pair's range of G takes the live blocks w - first, w - first + G, ... of that
// pair's source; lanes, gates, arithmetic and reduction are k_register's (register_body.h).  The pair's descriptor -- the
// destination as a MultiMap with T = X~_p, the source's table, voxels and range of the list -- comes from a table in
// mapped page-locked memory, indexed by a wave-uniform pair index, as k_render_multi reads its maps.  One row of 33 per
// workgroup in mapped page-locked memory (a workgroup whose share holds no block writes zeros); the host adds each pair's rows in
// index order.  No atomics, no workgroup waits for another; the same bytes on every run.  The joint system (pivots,
// Jacobians) is assembled on the host in double; the damped iteration is lm_iterate of register_host.h, the one the pairwise
// call runs.  This file's own are the kernel, the plan of the grid, the assembly, the active set and its connectivity.
#include <cmath>
#include <cstring>
#include <vector>

#include "dslam_internal.h"
#include "register_device.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {

// one pair of the graph, as the kernel reads it
struct RegisterGraphJob {
  MultiMap dst;              // the destination read from the source's voxel frame: T = X~_p
  const HashEntry *hash;     // the source
  const uint2 *voxels;
  int list_offset;           // its resident entries: live_list[list_offset .. list_offset + live)
  int live;
  int first_wg, num_wg;      // the pair's workgroups
};

struct RegisterGraphParams {
  const RegisterGraphJob *jobs;
  const int *wg_pair;        // [gridDim.x] the pair of each workgroup
  const int *live_list;
  int band_raw;              // (int)(band * 32767)
  float residual_gate;
  double *partials;          // [gridDim.x][kRegSums]
};


__global__ __launch_bounds__(kRegThreads) void k_register_graph(RegisterGraphParams gp) {
  // (split_workgroups hands out the whole grid, so every workgroup has a pair; one whose share holds no block writes zeros
  // through the body)
  const int pair = __builtin_amdgcn_readfirstlane(gp.wg_pair[blockIdx.x]);
  const RegisterGraphJob &pj = gp.jobs[pair];
  const unsigned first_wg = (unsigned)pj.first_wg, num_wg = (unsigned)pj.num_wg;
  RegisterParams p;
  p.hash = pj.hash; p.voxels = pj.voxels;
  p.live_list = gp.live_list + pj.list_offset; p.live_count = &pj.live;
  p.dst = pj.dst;
  p.band_raw = gp.band_raw; p.residual_gate = gp.residual_gate;
  p.partials = gp.partials;
#define DSLAM_REG_FIRST (blockIdx.x - first_wg)
#define DSLAM_REG_STRIDE num_wg
#include "register_body.h"
#undef DSLAM_REG_FIRST
#undef DSLAM_REG_STRIDE
}

// ---- host side ------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kJobTableBytes = (size_t)DSLAM_MAX_REGISTER_PAIRS * sizeof(RegisterGraphJob);

int ensure_graph_scratch(dslam_engine *e) {
  if (e->reg_graph.jobs) return DSLAM_OK;
  RegisterGraphScratch s;   // (the engine gets the two together or none)
  DSLAM_TRY(s.partials.alloc((size_t)kRegGrid * kRegSums, hipHostMallocMapped));
  DSLAM_TRY(s.jobs.alloc(kJobTableBytes + (size_t)kRegGrid * sizeof(int), hipHostMallocMapped));
  e->reg_graph = std::move(s);
  return DSLAM_OK;
}

// Ad(X)^T for twists ordered (rotation, translation): Ad = [[R, 0], [[t]x R, R]]
void adjoint_transposed(const double X[12], double out[36]) {
  const double t[3] = {X[3], X[7], X[11]};
  const double tx[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  double Ad[36];
  for (int i = 0; i < 36; i++) Ad[i] = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double r = X[i * 4 + j];
      double acc = 0.0;
      for (int k = 0; k < 3; k++) acc += tx[i * 3 + k] * X[k * 4 + j];
      Ad[i * 6 + j] = r;
      Ad[(3 + i) * 6 + 3 + j] = r;
      Ad[(3 + i) * 6 + j] = acc;
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) out[i * 6 + j] = Ad[j * 6 + i];
}

struct GraphEvaluation {
  std::vector<Evaluation33> pairs;   // (entries of pairs that are not evaluated keep what they held)
  double cost;
  // the gated cost of the pairs `use` together
  void cost_over(const std::vector<int> &use, double gate2) {
    double num = 0.0, den = 0.0;
    for (int p : use) {
      num += pairs[p].gated_sum(gate2);
      den += (double)pairs[p].candidates;
    }
    cost = den > 0.0 ? num / den : gate2;
  }
};

}  // namespace

// everything already checked and defaulted by dslam_register_graph
int launch_register_graph(dslam_engine *e, const dslam_scene *const *scenes, float *T_io, int num_maps, const int32_t *pairs,
                          int num_pairs, int anchor, const dslam_register_params *rp, dslam_register_graph_result *res,
                          dslam_register_pair_result *pair_res) {
  // ---- the live lists of the distinct sources, in the order the pairs name them ----
  std::vector<int> sources, list_offset, live;
  for (int p = 0; p < num_pairs; p++)
    if (std::find(sources.begin(), sources.end(), pairs[2 * p]) == sources.end()) sources.push_back(pairs[2 * p]);
  DSLAM_TRY(fill_live_lists(e, scenes, num_maps, sources, list_offset, live));
  DSLAM_TRY(ensure_graph_scratch(e));
  RegisterGraphScratch &sc = e->reg_graph;
  std::vector<int> live_of_pair(num_pairs);
  for (int p = 0; p < num_pairs; p++) live_of_pair[p] = live[pairs[2 * p]];

  RegisterGraphJob *jobs = static_cast<RegisterGraphJob *>(sc.jobs.get());
  int *wg_pair = reinterpret_cast<int *>(static_cast<char *>(sc.jobs.get()) + kJobTableBytes);
  RegisterGraphParams kp;
  memset(&kp, 0, sizeof kp);
  kp.jobs = static_cast<const RegisterGraphJob *>(sc.jobs.device());
  kp.wg_pair = reinterpret_cast<const int *>(static_cast<const char *>(sc.jobs.device()) + kJobTableBytes);
  kp.live_list = e->live_lists.live_list;
  kp.band_raw = (int)(rp->band * 32767.0f);
  kp.residual_gate = rp->residual_gate;
  kp.partials = sc.partials.device();

  const double vs = (double)scenes[0]->p.voxel_size;
  const double gate2 = (double)rp->residual_gate * (double)rp->residual_gate;
  e->reg_graph_sums.assign((size_t)num_pairs * kRegSums, 0.0);

  // the job table of the pairs `use`: everything but the transforms
  std::vector<int> first_wg(num_pairs, 0), num_wg(num_pairs, 0);
  auto plan = [&](const std::vector<int> &use) {
    split_workgroups(kRegGrid, use, live_of_pair, first_wg, num_wg);
    for (int p : use) {
      const dslam_scene *s = scenes[pairs[2 * p]], *d = scenes[pairs[2 * p + 1]];
      RegisterGraphJob &j = jobs[p];
      memset(&j, 0, sizeof j);
      j.dst = map_of(d);
      j.hash = s->hash; j.voxels = s->voxels;
      j.list_offset = list_offset[pairs[2 * p]];
      j.live = live_of_pair[p];
      j.first_wg = first_wg[p]; j.num_wg = num_wg[p];
      for (int w = 0; w < num_wg[p]; w++) wg_pair[first_wg[p] + w] = p;
    }
  };

  // X~_p of every pair at the poses T (double), and one joint evaluation of the pairs `use` there
  std::vector<double> Xp((size_t)num_pairs * 12);
  auto evaluate = [&](const std::vector<double> &T, const std::vector<int> &use, GraphEvaluation &ev) -> int {
    for (int p : use) {
      const bool identity = pair_transform(&T[(size_t)pairs[2 * p] * 12], &T[(size_t)pairs[2 * p + 1] * 12], &Xp[(size_t)p * 12],
                                           jobs[p].dst.T);
      jobs[p].dst.identity = identity ? 1 : 0;
    }
    hipLaunchKernelGGL(k_register_graph, dim3(kRegGrid), dim3(kRegThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    for (int p : use) {
      ev.pairs[p].sum_rows(sc.partials, first_wg[p], num_wg[p]);
      memcpy(&e->reg_graph_sums[(size_t)p * kRegSums], ev.pairs[p].sums, sizeof ev.pairs[p].sums);
    }
    ev.cost_over(use, gate2);
    return DSLAM_OK;
  };

  // ---- the start poses ----
  std::vector<double> T((size_t)num_maps * 12);
  for (int i = 0; i < num_maps; i++) voxel_pose(T_io + 16 * i, vs, &T[(size_t)i * 12]);
  std::vector<int> all(num_pairs), active;
  for (int p = 0; p < num_pairs; p++) all[p] = p;
  GraphEvaluation good;
  good.pairs.resize(num_pairs);
  plan(all);
  DSLAM_TRY(evaluate(T, all, good));
  const GraphEvaluation first = good;
  for (int p = 0; p < num_pairs; p++)
    if (good.pairs[p].valid >= rp->min_valid) active.push_back(p);
  if ((int)active.size() != num_pairs) {
    // the cost of the active pairs alone, and the grid to them
    good.cost_over(active, gate2);
    if (!active.empty()) plan(active);
  }
  const double cost_first = good.cost;

  // ---- do the active pairs connect every map to the anchor? ----
  std::vector<int> reached(num_maps, 0), stack(1, anchor);
  reached[anchor] = 1;
  while (!stack.empty()) {
    const int m = stack.back();
    stack.pop_back();
    for (int p : active) {
      const int s = pairs[2 * p], d = pairs[2 * p + 1];
      const int other = s == m ? d : (d == m ? s : -1);
      if (other >= 0 && !reached[other]) { reached[other] = 1; stack.push_back(other); }
    }
  }
  bool connected = true;
  for (int i = 0; i < num_maps; i++) connected = connected && reached[i];

  // unknown block of map i in the reduced system
  const int n_free = num_maps - 1, n = 6 * n_free;
  auto block_of = [&](int i) { return i == anchor ? -1 : (i < anchor ? i : i - 1); };
  std::vector<double> cpiv((size_t)num_maps * 3);
  // the joint system (H: n x n, g: n) at an evaluation and the poses it was made at (Xp holds their pair transforms)
  auto assemble = [&](const GraphEvaluation &ev, double *H, double *g) {
    std::fill_n(H, (size_t)n * n, 0.0);
    std::fill_n(g, n, 0.0);
    // pivots
    for (int i = 0; i < num_maps; i++) {
      double acc[3] = {0.0, 0.0, 0.0}, weight = 0.0;
      for (int p : active) {
        const Evaluation33 &pe = ev.pairs[p];
        const double valid = pe.sums[28];
        if (pairs[2 * p + 1] == i) {
          for (int k = 0; k < 3; k++) acc[k] += pe.sums[29 + k];
          weight += valid;
        } else if (pairs[2 * p] == i && valid > 0.0) {
          double inv[12];
          rigid_inverse(&Xp[(size_t)p * 12], inv);
          const double m[3] = {pe.sums[29] / valid, pe.sums[30] / valid, pe.sums[31] / valid};
          for (int k = 0; k < 3; k++)
            acc[k] += valid * (((inv[k * 4 + 0] * m[0] + inv[k * 4 + 1] * m[1]) + inv[k * 4 + 2] * m[2]) + inv[k * 4 + 3]);
          weight += valid;
        }
      }
      for (int k = 0; k < 3; k++) cpiv[(size_t)i * 3 + k] = weight > 0.0 ? acc[k] / weight : 0.0;
    }
    for (int p : active) {
      const Evaluation33 &pe = ev.pairs[p];
      const int maps_of[2] = {pairs[2 * p], pairs[2 * p + 1]};   // s, d
      double Hp[36], J[2][36], P[36], AdT[36];
      unpack_hessian(pe.sums, Hp);
      // J_s = -P(c_s) Ad(X~)^T
      pivot_matrix(&cpiv[(size_t)maps_of[0] * 3], P);
      adjoint_transposed(&Xp[(size_t)p * 12], AdT);
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
          double acc = 0.0;
          for (int k = 0; k < 6; k++) acc += P[i * 6 + k] * AdT[k * 6 + j];
          J[0][i * 6 + j] = -acc;
        }
      pivot_matrix(&cpiv[(size_t)maps_of[1] * 3], J[1]);   // J_d = P(c_d)
      for (int a = 0; a < 2; a++) {
        const int ba = block_of(maps_of[a]);
        if (ba < 0) continue;
        double ga[6];
        mat6_vec(J[a], pe.sums + 21, ga);
        for (int i = 0; i < 6; i++) g[ba * 6 + i] += ga[i];
        for (int b = 0; b < 2; b++) {
          const int bb = block_of(maps_of[b]);
          if (bb < 0) continue;
          double blk[36];
          sandwich6(J[a], Hp, J[b], blk);
          for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) H[(size_t)(ba * 6 + i) * n + bb * 6 + j] += blk[i * 6 + j];
        }
      }
    }
  };

  // a step: the poses the increment leads to, evaluated on the active pairs; adopted if every pair stays valid and the
  // joint cost falls, otherwise the pair transforms go back to those of the accepted poses (what the next system is made at)
  std::vector<double> trial((size_t)num_maps * 12), Xp_good;
  GraphEvaluation ev;
  ev.pairs.resize(num_pairs);
  auto step = [&](const double *y) -> int {
    Xp_good = Xp;
    trial = T;
    for (int i = 0; i < num_maps; i++) {
      const int b = block_of(i);
      if (b >= 0) apply_increment(y + (size_t)b * 6, &cpiv[(size_t)i * 3], &T[(size_t)i * 12], &trial[(size_t)i * 12]);
    }
    DSLAM_TRY(evaluate(trial, active, ev));
    bool all_valid = true;
    for (int p : active) all_valid = all_valid && ev.pairs[p].valid >= rp->min_valid;
    if (!(all_valid && ev.cost < good.cost)) { Xp = Xp_good; return 0; }
    T = trial;
    for (int p : active) good.pairs[p] = ev.pairs[p];
    good.cost = ev.cost;
    return 1;
  };
  LmOutcome lm;
  DSLAM_TRY(lm_iterate(
      n, connected, rp->max_evaluations, (double)rp->term_rotation, (double)rp->term_translation_voxels,
      [&](double *H, double *g) { assemble(good, H, g); }, step, lm));
  if (lm.accepted_any)
    for (int i = 0; i < num_maps; i++)
      if (i != anchor) pose_from_voxels(&T[(size_t)i * 12], vs, T_io + 16 * i);
  res->evaluations = lm.evaluations;
  res->stop_reason = lm.stop;
  res->active_pairs = (int)active.size();
  res->cost_first = (float)cost_first;
  res->cost_last = (float)good.cost;
  res->conditioning = (float)lm.conditioning;
  if (pair_res) {
    std::vector<char> is_active(num_pairs, 0);
    for (int p : active) is_active[p] = 1;
    for (int p = 0; p < num_pairs; p++) {
      dslam_register_pair_result &pr = pair_res[p];
      pr.candidates = first.pairs[p].candidates;
      pr.valid_first = first.pairs[p].valid;
      pr.valid_last = good.pairs[p].valid;
      pr.active = is_active[p];
      pr.cost_first = (float)first.pairs[p].gated_cost(gate2);
      pr.cost_last = (float)good.pairs[p].gated_cost(gate2);
    }
  }
  return device_errors(e);
}

}  // namespace dslam
