// register_host.h -- the host arithmetic of the SDF optimisers (double): the 33 sums of an evaluation and their pivot, the
// damped iteration (lm_iterate), the damped solve, the conditioning, the twist matrices and the rigid compositions.
// register.hip (one pair, 6 unknowns), track_sdf.hip (the camera, 6 unknowns per pyramid level) and register_graph.hip (a
// pose graph, 6 (N - 1) unknowns) run the same functions, so a graph of one pair repeats the pairwise call operation for
// operation (DESIGN.md sections 13, 15, 18 and 19).  The pair transform and the split of a fixed grid are also what the
// overlap survey (overlap.hip) uses.  Plain C++: nothing here needs HIP (tests/stubs/lm_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace dslam {

// the sums of one evaluation (register_body.h): [0..20] lower triangle of sum A^T A row by row, [21..26] sum b A,
// [27] sum b^2, [28] valid, [29..31] sum q over valid points, [32] candidates
constexpr int kRegSums = 33;

// the totals of one evaluation
struct Evaluation33 {
  double sums[kRegSums];
  int valid, candidates;
  // rows first_row .. first_row + num_rows of the per-workgroup partials, added in index order
  void sum_rows(const double *partials, int first_row, int num_rows) {
    for (int i = 0; i < kRegSums; i++) sums[i] = 0.0;
    for (int g = first_row; g < first_row + num_rows; g++)
      for (int i = 0; i < kRegSums; i++) sums[i] += partials[(size_t)g * kRegSums + i];
    valid = (int)sums[28];
    candidates = (int)sums[32];
  }
  // sum b^2 with every candidate that is not valid counted at the gate ...
  double gated_sum(double gate2) const { return sums[27] + (double)(candidates - valid) * gate2; }
  // ... per candidate
  double gated_cost(double gate2) const { return candidates > 0 ? gated_sum(gate2) / (double)candidates : gate2; }
};

namespace {

// solve M y = r (n x n, symmetric positive definite up to rounding) by Gaussian elimination with partial pivoting; a
// freedom whose diagonal entry is not positive is left out (y = 0)
inline void solve_damped(const double *M, const double *r, int n_all, double *y) {
  std::vector<int> idx;
  for (int i = 0; i < n_all; i++) { y[i] = 0.0; if (M[(size_t)i * n_all + i] > 0.0) idx.push_back(i); }
  const int n = (int)idx.size();
  std::vector<double> a((size_t)n * (n + 1));
  const size_t w = (size_t)n + 1;
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) a[i * w + j] = M[(size_t)idx[i] * n_all + idx[j]];
    a[i * w + n] = r[idx[i]];
  }
  for (int c = 0; c < n; c++) {
    int piv = c;
    for (int i = c + 1; i < n; i++) if (fabs(a[i * w + c]) > fabs(a[piv * w + c])) piv = i;
    if (a[piv * w + c] == 0.0) return;
    if (piv != c) for (int j = 0; j <= n; j++) std::swap(a[piv * w + j], a[c * w + j]);
    for (int i = c + 1; i < n; i++) {
      const double f = a[i * w + c] / a[c * w + c];
      for (int j = c; j <= n; j++) a[i * w + j] -= f * a[c * w + j];
    }
  }
  for (int i = n - 1; i >= 0; i--) {
    double v = a[i * w + n];
    for (int j = i + 1; j < n; j++) v -= a[i * w + j] * y[idx[j]];
    y[idx[i]] = v / a[i * w + i];
  }
}

// smallest eigenvalue of a symmetric n x n matrix (cyclic Jacobi; S is overwritten)
inline double smallest_eigenvalue(double *S, int n) {
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0.0;
    for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) off += S[(size_t)i * n + j] * S[(size_t)i * n + j];
    if (off < 1e-30) break;
    for (int pi = 0; pi < n - 1; pi++)
      for (int qi = pi + 1; qi < n; qi++) {
        const double apq = S[(size_t)pi * n + qi];
        if (apq == 0.0) continue;
        const double theta = (S[(size_t)qi * n + qi] - S[(size_t)pi * n + pi]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int k = 0; k < n; k++) {
          const double akp = S[(size_t)k * n + pi], akq = S[(size_t)k * n + qi];
          S[(size_t)k * n + pi] = cs * akp - sn * akq;
          S[(size_t)k * n + qi] = sn * akp + cs * akq;
        }
        for (int k = 0; k < n; k++) {
          const double apk = S[(size_t)pi * n + k], aqk = S[(size_t)qi * n + k];
          S[(size_t)pi * n + k] = cs * apk - sn * aqk;
          S[(size_t)qi * n + k] = sn * apk + cs * aqk;
        }
      }
  }
  double lo = S[0];
  for (int i = 1; i < n; i++) lo = std::min(lo, S[(size_t)i * n + i]);
  return lo;
}

// smallest eigenvalue of D^-1/2 H D^-1/2, D = diag H; 0 if a diagonal entry is not positive
inline double conditioning_of(const double *H, int n) {
  for (int i = 0; i < n; i++) if (!(H[(size_t)i * n + i] > 0.0)) return 0.0;
  std::vector<double> S((size_t)n * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) S[(size_t)i * n + j] = H[(size_t)i * n + j] / sqrt(H[(size_t)i * n + i] * H[(size_t)j * n + j]);
  return smallest_eigenvalue(S.data(), n);
}

// the 6 x 6 matrix of sums [0 .. 20] (lower triangle, row by row)
inline void unpack_hessian(const double *sums, double H[36]) {
  for (int k = 0, n = 0; k < 6; k++)
    for (int j = 0; j <= k; j++, n++) H[k * 6 + j] = H[j * 6 + k] = sums[n];
}

// P(c) = [[I, -[c]x], [0, I]]
inline void pivot_matrix(const double c[3], double P[36]) {
  for (int i = 0; i < 36; i++) P[i] = (i % 7) == 0 ? 1.0 : 0.0;
  P[0 * 6 + 4] = c[2];  P[0 * 6 + 5] = -c[1];
  P[1 * 6 + 3] = -c[2]; P[1 * 6 + 5] = c[0];
  P[2 * 6 + 3] = c[1];  P[2 * 6 + 4] = -c[0];
}

// out = (A H) B^T, 6 x 6, every sum in index order
inline void sandwich6(const double A[36], const double H[36], const double B[36], double out[36]) {
  double AH[36];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double acc = 0.0;
      for (int k = 0; k < 6; k++) acc += A[i * 6 + k] * H[k * 6 + j];
      AH[i * 6 + j] = acc;
    }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double acc = 0.0;
      for (int k = 0; k < 6; k++) acc += AH[i * 6 + k] * B[j * 6 + k];
      out[i * 6 + j] = acc;
    }
}

inline void mat6_vec(const double A[36], const double *v, double out[6]) {
  for (int i = 0; i < 6; i++) {
    double acc = 0.0;
    for (int k = 0; k < 6; k++) acc += A[i * 6 + k] * v[k];
    out[i] = acc;
  }
}

// the sums re-pivoted to the centroid c = sum q / valid: H_c = P H P^T, g_c = P g with P = [[I, -[c]x], [0, I]]
inline void pivot_sums(const double sums[kRegSums], double c[3], double Hc[36], double gc[6]) {
  double H[36], P[36];
  unpack_hessian(sums, H);
  const double valid = sums[28];
  for (int i = 0; i < 3; i++) c[i] = valid > 0.0 ? sums[29 + i] / valid : 0.0;
  pivot_matrix(c, P);
  sandwich6(P, H, P, Hc);
  mat6_vec(P, sums + 21, gc);
}

// X' = Inc X with Inc: q -> c + R(w)(q - c) + t (Rodrigues); X, out: 3 x 4 row-major
inline void apply_increment(const double y[6], const double c[3], const double X[12], double out[12]) {
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

// the inverse (R^T, -(R^T t)) of a rigid 3 x 4, the sum evaluated left to right (the mirror's RigidInverse)
inline void rigid_inverse(const double X[12], double out[12]) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) out[r * 4 + c] = X[c * 4 + r];
    out[r * 4 + 3] = -((X[0 * 4 + r] * X[3] + X[1 * 4 + r] * X[7]) + X[2 * 4 + r] * X[11]);
  }
}

// C = A B of rigid 3 x 4 (fourth row 0 0 0 1), each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (the mirror's RigidProduct)
inline void rigid_product(const double A[12], const double B[12], double C[12]) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++)
      C[r * 4 + c] = ((A[r * 4 + 0] * B[0 * 4 + c] + A[r * 4 + 1] * B[1 * 4 + c]) + A[r * 4 + 2] * B[2 * 4 + c]) +
                     A[r * 4 + 3] * (c == 3 ? 1.0 : 0.0);
}

// T~: a column-major float32 4 x 4 in metres (world -> map) as 3 x 4 row-major double with its translation in voxels
inline void voxel_pose(const float T[16], double voxel_size, double out[12]) {
  for (int row = 0; row < 3; row++) {
    for (int col = 0; col < 3; col++) out[row * 4 + col] = (double)T[col * 4 + row];
    out[row * 4 + 3] = (double)T[12 + row] / voxel_size;
  }
}

// the pair transform X~ = T~_d inv(T~_s) in double (X) and rounded to float32 (Xf); returns whether Xf is the identity
inline bool pair_transform(const double Ts[12], const double Td[12], double X[12], float Xf[12]) {
  double inv[12];
  rigid_inverse(Ts, inv);
  rigid_product(Td, inv, X);
  bool identity = true;
  for (int k = 0; k < 12; k++) {
    Xf[k] = (float)X[k];
    identity = identity && Xf[k] == ((k % 5) == 0 ? 1.0f : 0.0f);
  }
  return identity;
}

// a column-major float32 4 x 4, exactly the identity?
inline bool is_identity16(const float *T) {
  for (int i = 0; i < 16; i++)
    if (T[i] != ((i % 5) == 0 ? 1.0f : 0.0f)) return false;
  return true;
}

// the estimate X (3 x 4 row-major double, translation in voxels) as a column-major float32 4 x 4 in metres
inline void pose_from_voxels(const double X[12], double voxel_size, float out[16]) {
  for (int row = 0; row < 3; row++) {
    for (int col = 0; col < 3; col++) out[col * 4 + row] = (float)X[row * 4 + col];
    out[12 + row] = (float)(X[row * 4 + 3] * voxel_size);
    out[row * 4 + 3] = 0.0f;
  }
  out[15] = 1.0f;
}

// The damped (Levenberg-Marquardt) iteration over n = 6 B unknowns, B blocks of (rotation, translation), from a state
// that has been evaluated once; start_ok: that evaluation allows a step at all.
//   system(H, g)   fills the n x n system at the accepted state;
//   step(y)        evaluates the state the increment y leads to and adopts it if it is valid and cheaper: 1 adopted,
//                  0 rejected (the accepted state is as before), negative: a failure, handed on.
// The driver damps (H + lambda diag H) y = g, lambda from 1: an adopted step divides it by 10 (not below 1e-6), a rejected
// one multiplies it by 10.  Stop reasons: 0 an adopted step taken with lambda <= 1 whose rotation and translation norms
// are below the thresholds in every block, 1 max_evaluations reached, 2 lambda above 1e6, 3 no step possible at the start.
struct LmOutcome {
  int evaluations;       // the start's included
  int stop;
  bool accepted_any;
  double conditioning;   // conditioning_of the system at the accepted state; 0 for stop reason 3
};
// The iteration as a resumable stepper, for a caller that has the trials of many problems evaluated together
// (track_sdf_starts.hip): begin(); then, while propose(system) returns true, have the state increment() leads to evaluated
// and hand its outcome to verdict(adopted); then finish(system).  lm_iterate below is that loop around one problem.
class LmStepper {
 public:
  LmOutcome out = {0, 3, false, 0.0};
  void begin(int n, bool start_ok, int max_evaluations, double term_rotation, double term_translation) {
    n_ = n; max_evaluations_ = max_evaluations; term_rotation_ = term_rotation; term_translation_ = term_translation;
    out.evaluations = 1;
    out.stop = start_ok ? -1 : 3;
    out.accepted_any = false;
    out.conditioning = 0.0;
    lambda_ = 1.0;
    H_.assign((size_t)n * n, 0.0);
    g_.assign(n, 0.0);
    y_.assign(n, 0.0);
  }
  // false: the iteration has stopped (out.stop says why); true: increment() is the step to try next
  template <class System>
  bool propose(System &&system) {
    if (out.stop >= 0) return false;
    if (out.evaluations >= max_evaluations_) { out.stop = 1; return false; }
    const int n = n_;
    system(H_.data(), g_.data());
    M_ = H_;
    for (int i = 0; i < n; i++) M_[(size_t)i * n + i] += lambda_ * H_[(size_t)i * n + i];
    solve_damped(M_.data(), g_.data(), n, y_.data());
    return true;
  }
  const double *increment() const { return y_.data(); }
  // the proposed step has been evaluated: adopted (the caller's accepted state is now the trial) or rejected
  void verdict(bool adopted) {
    const int n = n_;
    const std::vector<double> &y = y_;
    out.evaluations++;
    if (adopted) {
      const double used = lambda_;
      out.accepted_any = true;
      lambda_ = std::max(lambda_ / 10.0, 1e-6);
      // (the largest block norm is below a threshold exactly when every block's is)
      bool small = true;
      for (int b = 0; b < n; b += 6) {
        const double rot = sqrt(y[b] * y[b] + y[b + 1] * y[b + 1] + y[b + 2] * y[b + 2]);
        const double tr = sqrt(y[b + 3] * y[b + 3] + y[b + 4] * y[b + 4] + y[b + 5] * y[b + 5]);
        small = small && rot < term_rotation_ && tr < term_translation_;
      }
      if (used <= 1.0 && small) out.stop = 0;
    } else {
      lambda_ *= 10.0;
      if (lambda_ > 1e6) out.stop = 2;
    }
  }
  // after the stop: the conditioning at the accepted state
  template <class System>
  void finish(System &&system) {
    if (out.stop != 3) {
      system(H_.data(), g_.data());
      out.conditioning = conditioning_of(H_.data(), n_);
    }
  }
  double lambda() const { return lambda_; }

 private:
  int n_ = 0, max_evaluations_ = 0;
  double term_rotation_ = 0.0, term_translation_ = 0.0, lambda_ = 1.0;
  std::vector<double> H_, g_, M_, y_;
};
template <class System, class Step>
int lm_iterate(int n, bool start_ok, int max_evaluations, double term_rotation, double term_translation, System &&system,
               Step &&step, LmOutcome &out) {
  LmStepper lm;
  lm.begin(n, start_ok, max_evaluations, term_rotation, term_translation);
  while (lm.propose(system)) {
    const int adopted = step(lm.increment());
    if (adopted < 0) { out = lm.out; return adopted; }
    lm.verdict(adopted != 0);
  }
  lm.finish(system);
  out = lm.out;
  return 0;
}

// The workgroups of a grid over the jobs `use` (list order): G_p = 1 + floor((grid - n) L_p / sum L), the rest handed
// out one each in list order -- a function of the live counts alone, and all of the grid to a single job.
inline void split_workgroups(int grid, const std::vector<int> &use, const std::vector<int> &live_of, std::vector<int> &first,
                             std::vector<int> &count) {
  const int n = (int)use.size();
  long long total = 0;
  for (int p : use) total += live_of[p];
  int given = 0;
  for (int p : use) {
    count[p] = 1 + (total > 0 ? (int)((long long)(grid - n) * live_of[p] / total) : 0);
    given += count[p];
  }
  for (int k = 0; given < grid; k = (k + 1) % n, given++) count[use[k]]++;
  int at = 0;
  for (int p : use) { first[p] = at; at += count[p]; }
}

}  // namespace
}  // namespace dslam
