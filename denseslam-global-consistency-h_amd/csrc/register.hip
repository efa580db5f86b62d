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
#include "mesh_device.h"
#include "multimap_device.h"

#pragma clang fp contract(off)

namespace dslam {

constexpr int kRegSums = 33;
constexpr int kRegGrid = 512;      // workgroups of k_register: two per CU of an MI355X
constexpr int kRegThreads = 256;   // lane t takes voxels t and t + 256 of a block
constexpr int kRegWaves = kRegThreads / 64;

struct RegisterParams {
  const HashEntry *hash;     // the source
  const uint2 *voxels;
  const int *live_list;      // its resident entries, ascending
  const int *live_count;
  MultiMap dst;              // the destination read from the source's voxel frame: T = X~
  int band_raw;              // (int)(band * 32767)
  float residual_gate;
  double *partials;          // [gridDim.x][kRegSums]
};

// its own type: the selection kernel of this translation unit is not mesh.hip's
struct SelLiveRegister : SelLive {};

__global__ __launch_bounds__(kRegThreads) void k_register(RegisterParams p) {
  double sH[21], sN[6], sF = 0.0, sQx = 0.0, sQy = 0.0, sQz = 0.0;
  int valid = 0, cand = 0;
#pragma unroll
  for (int i = 0; i < 21; i++) sH[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) sN[i] = 0.0;
  const int live = *p.live_count;
  const int x = threadIdx.x & 7, y = (threadIdx.x >> 3) & 7;
  const VolumeRef vol = volume_of(p.dst);
  for (int job = blockIdx.x * 2; job < live * 2; job += (job & 1) ? gridDim.x * 2 - 1 : 1) {
    const int b = job >> 1, z = (int)(threadIdx.x >> 6) + 4 * (job & 1);
    const HashEntry he = load_entry(p.hash, p.live_list[b]);
    if (he.ptr < 0) continue;  // (uniform; a live entry holds a block)
    const unsigned own = p.voxels[(size_t)he.ptr * kBlock3 + threadIdx.x + kRegThreads * (job & 1)].x;
    const int raw_s = (int)(short)(own & 0xffffu);
    if (((own >> 16) & 0xffu) == 0u || abs(raw_s) >= p.band_raw) continue;
    cand++;
    const Vec3 pt = {(float)(he.pos[0] * kBlock + x), (float)(he.pos[1] * kBlock + y), (float)(he.pos[2] * kBlock + z)};
    const Vec3 q = to_map(p.dst, pt);
    // a block coordinate outside the short range is never resident (and this keeps the casts below defined)
    if (!(fabsf(q.x) < 262144.0f && fabsf(q.y) < 262144.0f && fabsf(q.z) < 262144.0f)) continue;
    const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
    uint2 t[8];
    if (!gather_cell(vol, (int)fx, (int)fy, (int)fz, t)) continue;
    bool ok = true;
    float s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int raw = (int)(short)(t[k].x & 0xffffu);
      ok = ok && ((t[k].x >> 16) & 0xffu) != 0u && raw != 32767 && raw != -32767;
      s[k] = sdf_to_float((short)raw);
    }
    if (!ok) continue;
    const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
    const float ux = 1.0f - cx, uy = 1.0f - cy, uz = 1.0f - cz;
    const float x00 = ux * s[0] + cx * s[1], x10 = ux * s[2] + cx * s[3];
    const float x01 = ux * s[4] + cx * s[5], x11 = ux * s[6] + cx * s[7];
    const float y0 = uy * x00 + cy * x10, y1 = uy * x01 + cy * x11;
    const float d = uz * y0 + cz * y1;
    const float gx = uz * (uy * (s[1] - s[0]) + cy * (s[3] - s[2])) + cz * (uy * (s[5] - s[4]) + cy * (s[7] - s[6]));
    const float gy = uz * (x10 - x00) + cz * (x11 - x01);
    const float gz = y1 - y0;
    const float r = sdf_to_float((short)raw_s) - d;
    if (fabsf(r) > p.residual_gate) continue;
    float A[6];
    A[0] = q.y * gz - q.z * gy;
    A[1] = q.z * gx - q.x * gz;
    A[2] = q.x * gy - q.y * gx;
    A[3] = gx; A[4] = gy; A[5] = gz;
    valid++;
    sF += (double)(r * r);
    sQx += (double)q.x; sQy += (double)q.y; sQz += (double)q.z;
#pragma unroll
    for (int k = 0, c = 0; k < 6; k++) {
      sN[k] += (double)(r * A[k]);
#pragma unroll
      for (int j = 0; j <= k; j++, c++) sH[c] += (double)(A[k] * A[j]);
    }
  }
  // workgroup reduction in a fixed order: wave shuffle tree, then the four wave partials through LDS.  A workgroup
  // without a block arrives here with zeros and writes them.
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

struct Evaluation {
  double sums[kRegSums];
  double cost;
  int valid, candidates;
};

// solve M y = r (6 x 6, symmetric positive definite up to rounding) by Gaussian elimination with partial pivoting; a
// freedom whose diagonal entry is 0 is left out (y = 0)
void solve6(const double M[36], const double r[6], double y[6]) {
  int idx[6], n = 0;
  for (int i = 0; i < 6; i++) { y[i] = 0.0; if (M[i * 6 + i] > 0.0) idx[n++] = i; }
  double a[6][7];
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) a[i][j] = M[idx[i] * 6 + idx[j]];
    a[i][n] = r[idx[i]];
  }
  for (int c = 0; c < n; c++) {
    int piv = c;
    for (int i = c + 1; i < n; i++) if (fabs(a[i][c]) > fabs(a[piv][c])) piv = i;
    if (a[piv][c] == 0.0) return;
    if (piv != c) for (int j = 0; j <= n; j++) std::swap(a[piv][j], a[c][j]);
    for (int i = c + 1; i < n; i++) {
      const double f = a[i][c] / a[c][c];
      for (int j = c; j <= n; j++) a[i][j] -= f * a[c][j];
    }
  }
  for (int i = n - 1; i >= 0; i--) {
    double v = a[i][n];
    for (int j = i + 1; j < n; j++) v -= a[i][j] * y[idx[j]];
    y[idx[i]] = v / a[i][i];
  }
}

// smallest eigenvalue of a symmetric 6 x 6 matrix (cyclic Jacobi)
double smallest_eigenvalue6(double S[36]) {
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0.0;
    for (int i = 0; i < 6; i++) for (int j = 0; j < i; j++) off += S[i * 6 + j] * S[i * 6 + j];
    if (off < 1e-30) break;
    for (int pi = 0; pi < 5; pi++)
      for (int qi = pi + 1; qi < 6; qi++) {
        const double apq = S[pi * 6 + qi];
        if (apq == 0.0) continue;
        const double theta = (S[qi * 6 + qi] - S[pi * 6 + pi]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int k = 0; k < 6; k++) {
          const double akp = S[k * 6 + pi], akq = S[k * 6 + qi];
          S[k * 6 + pi] = cs * akp - sn * akq;
          S[k * 6 + qi] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 6; k++) {
          const double apk = S[pi * 6 + k], aqk = S[qi * 6 + k];
          S[pi * 6 + k] = cs * apk - sn * aqk;
          S[qi * 6 + k] = sn * apk + cs * aqk;
        }
      }
  }
  double lo = S[0];
  for (int i = 1; i < 6; i++) lo = std::min(lo, S[i * 6 + i]);
  return lo;
}

// the sums re-pivoted to the centroid c = sum q / valid: H_c = P H P^T, g_c = P g with P = [[I, -[c]x], [0, I]]
void pivot_sums(const double sums[kRegSums], double c[3], double Hc[36], double gc[6]) {
  double H[36], P[36], PH[36];
  for (int k = 0, n = 0; k < 6; k++)
    for (int j = 0; j <= k; j++, n++) H[k * 6 + j] = H[j * 6 + k] = sums[n];
  const double valid = sums[28];
  for (int i = 0; i < 3; i++) c[i] = valid > 0.0 ? sums[29 + i] / valid : 0.0;
  for (int i = 0; i < 36; i++) P[i] = (i % 7) == 0 ? 1.0 : 0.0;
  // -[c]x in the upper right block
  P[0 * 6 + 4] = c[2];  P[0 * 6 + 5] = -c[1];
  P[1 * 6 + 3] = -c[2]; P[1 * 6 + 5] = c[0];
  P[2 * 6 + 3] = c[1];  P[2 * 6 + 4] = -c[0];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double acc = 0.0;
      for (int k = 0; k < 6; k++) acc += P[i * 6 + k] * H[k * 6 + j];
      PH[i * 6 + j] = acc;
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double acc = 0.0;
      for (int k = 0; k < 6; k++) acc += PH[i * 6 + k] * P[j * 6 + k];
      Hc[i * 6 + j] = acc;
    }
  for (int i = 0; i < 6; i++) {
    double acc = 0.0;
    for (int k = 0; k < 6; k++) acc += P[i * 6 + k] * sums[21 + k];
    gc[i] = acc;
  }
}

double conditioning_of(const double Hc[36]) {
  double S[36];
  for (int i = 0; i < 6; i++) if (!(Hc[i * 6 + i] > 0.0)) return 0.0;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) S[i * 6 + j] = Hc[i * 6 + j] / sqrt(Hc[i * 6 + i] * Hc[j * 6 + j]);
  return smallest_eigenvalue6(S);
}

// X' = Inc X with Inc: q -> c + R(w)(q - c) + t (Rodrigues)
void apply_increment(const double y[6], const double c[3], const double X[12], double out[12]) {
  const double th = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
  double a, bq;   // R = I + a K + bq K^2, K = [w]x
  if (th < 1e-8) { a = 1.0 - th * th / 6.0; bq = 0.5 - th * th / 24.0; }
  else { a = sin(th) / th; bq = (1.0 - cos(th)) / (th * th); }
  const double K[9] = {0.0, -y[2], y[1], y[2], 0.0, -y[0], -y[1], y[0], 0.0};
  double K2[9], R[9], t[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double acc = 0.0;
      for (int k = 0; k < 3; k++) acc += K[i * 3 + k] * K[k * 3 + j];
      K2[i * 3 + j] = acc;
    }
  for (int i = 0; i < 9; i++) R[i] = ((i % 4) == 0 ? 1.0 : 0.0) + a * K[i] + bq * K2[i];
  for (int i = 0; i < 3; i++) t[i] = c[i] - (R[i * 3] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2]) + y[3 + i];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double acc = j == 3 ? t[i] : 0.0;
      for (int k = 0; k < 3; k++) acc += R[i * 3 + k] * X[k * 4 + j];
      out[i * 4 + j] = acc;
    }
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
    solve6(M, gc, y);
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
    conditioning = conditioning_of(Hc);
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
