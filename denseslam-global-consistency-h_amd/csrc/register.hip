// register.hip -- SDF-to-SDF alignment of two local maps (dslam_register_maps; ITMMainEngine::AlignLocalMap in the mirror).
//
// Reference: none.  The reference gets its map-to-map constraints from frames tracked in two maps at once; the law below
// is this project's own definition.  Both maps are only read.
//
// One evaluation at X~ (source voxels -> destination voxels, the first three rows, row-major, float32): every voxel of
// every resident source block, at integer voxel position p with fields (sdf_s, w_s),
//   candidate gate    w_s > 0 and |sdf_s| < (int)(band * 32767); candidates are counted in N;
//   position          q = X~ p (to_map of multimap_device.h), cell floor(q), fractions c = q - floor(q);
//   destination gate  all 8 taps of the cell (gather_cell) have w_depth > 0 and a raw sdf other than +-32767 -- a tap in
//                     a block that is not resident reads the empty voxel (w_depth 0), so it fails here too; else a miss;
//   value, gradient   s[k] = raw[k] / 32767 (tap k = (k & 1, (k >> 1) & 1, k >> 2)), ux = 1 - cx, uy = 1 - cy, uz = 1 - cz,
//                       x00 = ux s0 + cx s1, x10 = ux s2 + cx s3, x01 = ux s4 + cx s5, x11 = ux s6 + cx s7
//                       y0 = uy x00 + cy x10, y1 = uy x01 + cy x11,           d = uz y0 + cz y1          (lerp8's order)
//                       gx = uz (uy (s1 - s0) + cy (s3 - s2)) + cz (uy (s5 - s4) + cy (s7 - s6))
//                       gy = uz (x10 - x00) + cz (x11 - x01),                  gz = y1 - y0;
//   residual          b = sdf_s / 32767 - d; |b| > residual_gate is a miss too; otherwise the voxel is valid with the
//                     row A = [q x g, g] (rotation about the destination's origin, then translation);
//   sums              33 doubles of float32 products: [0..20] lower triangle of sum A^T A row by row, [21..26] sum b A,
//                     [27] sum b^2, [28] valid, [29..31] sum q over valid voxels, [32] N.
//
// Device work per call: one ordered compaction of the source's resident entries (launch_live_list, live_list.hip) and, per
// evaluation, k_register: a fixed grid, workgroup i takes live blocks i, i + grid, ..., lane t voxels t and t + 256 of the
// block (coalesced 8-byte loads); the candidate gate comes first, so only the band's voxels gather.  The reduction is
// the tracker's: per-lane doubles, wave shuffle tree (32, 16, ..., 1), the four wave partials through LDS in index
// order, one row of 33 per workgroup in mapped page-locked memory, rows added by the host in index order.  No atomics;
// the same bytes on every run.  Bound: gather latency, as the mesh.  The Levenberg-Marquardt iteration (pivot at the
// centroid, damped 6 x 6 solve, acceptance, stop reasons, conditioning) is a few hundred flops per evaluation and runs
// on the host in double: lm_iterate of register_host.h, which the graph and the depth-to-SDF tracker drive too.  What is
// this file's own is the kernel, its launch and the conversion of X.
#include <cmath>
#include <cstring>

#include "dslam_internal.h"
#include "register_device.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {


__global__ __launch_bounds__(kRegThreads) void k_register(RegisterParams p) {
#define DSLAM_REG_FIRST blockIdx.x
#define DSLAM_REG_STRIDE gridDim.x
#include "register_body.h"
#undef DSLAM_REG_FIRST
#undef DSLAM_REG_STRIDE
}

// ---- host side ------------------------------------------------------------------------------------------------
// src / dst / X / params already checked and defaulted by dslam_register_maps
int launch_register_maps(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst, float *X_io,
                         const dslam_register_params *rp, dslam_register_result *res) {
  DSLAM_TRY(ensure_scratch(e, std::max(src->n_entries, dst->n_entries), std::max(src->p.num_local_blocks, dst->p.num_local_blocks)));
  DSLAM_TRY(e->reg_sums.ensure(kRegGrid));
  int *live_count = e->misc_counter + 8;
  DSLAM_TRY(launch_live_list(e, src, e->list_a, live_count));
  DSLAM_HIP(hipGetLastError());

  RegisterParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.hash = src->hash; kp.voxels = src->voxels; kp.live_list = e->list_a; kp.live_count = live_count;
  kp.dst = map_of(dst);
  kp.band_raw = (int)(rp->band * 32767.0f);
  kp.residual_gate = rp->residual_gate;
  kp.partials = e->reg_sums.partials.device();

  const double vs = (double)src->p.voxel_size;
  const double gate2 = (double)rp->residual_gate * (double)rp->residual_gate;

  // (only the start may be the identity to the kernel: a trial is read through its transform whatever it is)
  auto evaluate = [&](const double X[12], bool identity, Evaluation33 &ev) -> int {
    for (int k = 0; k < 12; k++) kp.dst.T[k] = (float)X[k];
    kp.dst.identity = identity ? 1 : 0;
    hipLaunchKernelGGL(k_register, dim3(kRegGrid), dim3(kRegThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    e->reg_sums.collect(kRegGrid, ev);
    return DSLAM_OK;
  };

  double X[12], c[3];
  voxel_pose(X_io, vs, X);
  Evaluation33 good;
  DSLAM_TRY(evaluate(X, is_identity16(X_io), good));
  const double cost_first = good.gated_cost(gate2);
  LmOutcome lm;
  DSLAM_TRY(lm_iterate(
      6, good.valid >= rp->min_valid, rp->max_evaluations, (double)rp->term_rotation, (double)rp->term_translation_voxels,
      [&](double *H, double *g) { pivot_sums(good.sums, c, H, g); },
      [&](const double *y) -> int {
        double trial[12];
        Evaluation33 ev;
        apply_increment(y, c, X, trial);
        DSLAM_TRY(evaluate(trial, false, ev));
        if (!(ev.valid >= rp->min_valid && ev.gated_cost(gate2) < good.gated_cost(gate2))) return 0;
        memcpy(X, trial, sizeof trial);
        good = ev;
        return 1;
      },
      lm));
  if (lm.accepted_any) pose_from_voxels(X, vs, X_io);
  res->evaluations = lm.evaluations;
  res->stop_reason = lm.stop;
  res->candidates = good.candidates;
  res->valid_last = good.valid;
  res->cost_first = (float)cost_first;
  res->cost_last = (float)good.gated_cost(gate2);
  res->conditioning = (float)lm.conditioning;
  res->pad = 0;
  return device_errors(e);
}

}  // namespace dslam
