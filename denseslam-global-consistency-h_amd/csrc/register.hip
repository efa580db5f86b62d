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
// Device work per call: one ordered compaction of the source's resident entries (launch_bits_select) and, per
// evaluation, k_register: a fixed grid, workgroup i takes live blocks i, i + grid, ..., lane t voxels t and t + 256 of the
// block (coalesced 8-byte loads); the candidate gate comes first, so only the band's voxels gather.  The reduction is
// the tracker's: per-lane doubles, wave shuffle tree (32, 16, ..., 1), the four wave partials through LDS in index
// order, one row of 33 per workgroup in mapped page-locked memory, rows added by the host in index order.  No atomics;
// the same bytes on every run.  Bound: gather latency, as the mesh.  The Levenberg-Marquardt iteration (pivot at the
// centroid, damped 6 x 6 solve, acceptance, stop reasons, conditioning) is a few hundred flops per evaluation and runs
// on the host in double, like the tracker's.
#include <cmath>
#include <cstring>

#include "dslam_bits.h"
#include "register_device.h"
#include "register_host.h"

#pragma clang fp contract(off)

namespace dslam {

// its own type: the selection kernel of this translation unit is not mesh.hip's
struct SelLiveRegister : SelLive {};

__global__ __launch_bounds__(kRegThreads) void k_register(RegisterParams p) {
#define DSLAM_REG_FIRST blockIdx.x
#define DSLAM_REG_STRIDE gridDim.x
#include "register_body.h"
#undef DSLAM_REG_FIRST
#undef DSLAM_REG_STRIDE
}

// ---- host side ------------------------------------------------------------------------------------------------
namespace {

struct Evaluation {
  double sums[kRegSums];
  double cost;
  int valid, candidates;
};

// the sums re-pivoted to the centroid c = sum q / valid: H_c = P H P^T, g_c = P g with P = [[I, -[c]x], [0, I]]
void pivot_sums(const double sums[kRegSums], double c[3], double Hc[36], double gc[6]) {
  double H[36], P[36];
  unpack_hessian(sums, H);
  const double valid = sums[28];
  for (int i = 0; i < 3; i++) c[i] = valid > 0.0 ? sums[29 + i] / valid : 0.0;
  pivot_matrix(c, P);
  sandwich6(P, H, P, Hc);
  mat6_vec(P, sums + 21, gc);
}

}  // namespace

// src / dst / X / params already checked and defaulted by dslam_register_maps
int launch_register_maps(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst, float *X_io,
                         const dslam_register_params *rp, dslam_register_result *res) {
  DSLAM_TRY(ensure_scratch(e, std::max(src->n_entries, dst->n_entries), std::max(src->p.num_local_blocks, dst->p.num_local_blocks)));
  if (!e->reg_partials) DSLAM_TRY(e->reg_partials.alloc((size_t)kRegGrid * kRegSums, hipHostMallocMapped));
  int *live_count = e->misc_counter + 8;
  const int N = src->n_entries;
  SelLiveRegister sel;
  sel.hash = src->hash;
  DSLAM_TRY(launch_bits_select(e, src->alloc_bits, N, sel, e->list_a, N, live_count, src->counters));
  DSLAM_HIP(hipGetLastError());

  RegisterParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.hash = src->hash; kp.voxels = src->voxels; kp.live_list = e->list_a; kp.live_count = live_count;
  kp.dst.hash = dst->hash; kp.dst.voxels = dst->voxels;
  kp.dst.mask = (unsigned)(dst->p.num_buckets - 1); kp.dst.num_buckets = dst->p.num_buckets;
  kp.band_raw = (int)(rp->band * 32767.0f);
  kp.residual_gate = rp->residual_gate;
  kp.partials = e->reg_partials.device();

  const double vs = (double)src->p.voxel_size;
  const double gate2 = (double)rp->residual_gate * (double)rp->residual_gate;
  bool start_is_identity = true;
  for (int i = 0; i < 16; i++) start_is_identity = start_is_identity && X_io[i] == ((i % 5) == 0 ? 1.0f : 0.0f);

  auto evaluate = [&](const double X[12], bool identity, Evaluation &ev) -> int {
    for (int k = 0; k < 12; k++) kp.dst.T[k] = (float)X[k];
    kp.dst.identity = identity ? 1 : 0;
    hipLaunchKernelGGL(k_register, dim3(kRegGrid), dim3(kRegThreads), 0, e->stream, kp);
    DSLAM_HIP(hipGetLastError());
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < kRegSums; i++) ev.sums[i] = 0.0;
    for (int g = 0; g < kRegGrid; g++)
      for (int i = 0; i < kRegSums; i++) ev.sums[i] += e->reg_partials[(size_t)g * kRegSums + i];
    memcpy(e->reg_last_sums, ev.sums, sizeof ev.sums);
    e->reg_have_sums = true;
    ev.valid = (int)ev.sums[28];
    ev.candidates = (int)ev.sums[32];
    ev.cost = ev.candidates > 0 ? (ev.sums[27] + (double)(ev.candidates - ev.valid) * gate2) / (double)ev.candidates : gate2;
    return DSLAM_OK;
  };

  double X[12];
  for (int row = 0; row < 3; row++) {
    for (int col = 0; col < 3; col++) X[row * 4 + col] = (double)X_io[col * 4 + row];
    X[row * 4 + 3] = (double)X_io[12 + row] / vs;
  }
  Evaluation good;
  DSLAM_TRY(evaluate(X, start_is_identity, good));
  int evaluations = 1, stop = -1;
  bool accepted_any = false;
  const double cost_first = good.cost;
  double lambda = 1.0, Hc[36], gc[6], c[3];
  if (good.valid < rp->min_valid) stop = 3;
  while (stop < 0) {
    if (evaluations >= rp->max_evaluations) { stop = 1; break; }
    pivot_sums(good.sums, c, Hc, gc);
    double M[36], y[6], trial[12];
    for (int i = 0; i < 36; i++) M[i] = Hc[i];
    for (int i = 0; i < 6; i++) M[i * 6 + i] += lambda * Hc[i * 6 + i];
    solve_damped(M, gc, 6, y);
    apply_increment(y, c, X, trial);
    Evaluation ev;
    DSLAM_TRY(evaluate(trial, false, ev));
    evaluations++;
    if (ev.valid >= rp->min_valid && ev.cost < good.cost) {
      const double used = lambda;
      memcpy(X, trial, sizeof trial);
      good = ev;
      accepted_any = true;
      lambda = std::max(lambda / 10.0, 1e-6);
      const double rot = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]), tr = sqrt(y[3] * y[3] + y[4] * y[4] + y[5] * y[5]);
      if (used <= 1.0 && rot < (double)rp->term_rotation && tr < (double)rp->term_translation_voxels) stop = 0;
    } else {
      lambda *= 10.0;
      if (lambda > 1e6) stop = 2;
    }
  }
  double conditioning = 0.0;
  if (stop != 3) {
    pivot_sums(good.sums, c, Hc, gc);
    conditioning = conditioning_of(Hc, 6);
  }
  if (accepted_any) {
    for (int row = 0; row < 3; row++) {
      for (int col = 0; col < 3; col++) X_io[col * 4 + row] = (float)X[row * 4 + col];
      X_io[12 + row] = (float)(X[row * 4 + 3] * vs);
      X_io[row * 4 + 3] = 0.0f;
    }
    X_io[15] = 1.0f;
  }
  res->evaluations = evaluations;
  res->stop_reason = stop;
  res->candidates = good.candidates;
  res->valid_last = good.valid;
  res->cost_first = (float)cost_first;
  res->cost_last = (float)good.cost;
  res->conditioning = (float)conditioning;
  res->pad = 0;
  return device_errors(e);
}

}  // namespace dslam
