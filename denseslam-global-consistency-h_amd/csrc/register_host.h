// register_host.h -- the host arithmetic of the map registrations (double): the damped solve, the conditioning, the pivot
// and twist matrices and the rigid compositions.  register.hip (one pair, 6 unknowns) and register_graph.hip (a pose
// graph, 6 (N - 1) unknowns) run the same functions, so a graph of one pair repeats the pairwise call operation for
// operation (DESIGN.md sections 13 and 15).  The pair transform and the split of a fixed grid are also what the overlap
// survey (overlap.hip) uses.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace dslam {
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
