// lm_check.cpp -- lm_iterate of csrc/register_host.h on synthetic problems, without HIP (tests/test_register_host.py).
//
// A problem is a few hundred points p_i, each with a plane of its own: unit normal n_i through s_i = X* p_i.  The signed
// distance of q to that plane is linear, d(q) = n_i . (q - s_i), so an evaluation at X has q_i = X p_i, gradient n_i,
// residual b_i = -d(q_i) and the row A_i = [q_i x n_i, n_i] -- the law of register_body.h with an exact field -- and X* has
// zero residual.  The 33 sums are built here in double and driven the way register.hip drives them: pivot_sums for the
// system, apply_increment for a trial, "valid and cheaper" for acceptance.  Per case the program prints the accept / reject
// trail, the evaluation count, the stop code, the final transform(s) and what the case measures; the test asserts.
// It also checks that a float32 division equals the double division rounded to float32, bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "register_host.h"

using namespace dslam;

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
  double unit() { return (double)next() / 4294967296.0; }   // [0, 1)
};

// a rigid 3 x 4 from a rotation vector and a translation (apply_increment on the identity, pivot at the origin)
void rigid_from(const double w[3], const double t[3], double out[12]) {
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, zero[3] = {0, 0, 0}, y[6] = {w[0], w[1], w[2], t[0], t[1], t[2]};
  apply_increment(y, zero, I, out);
}
void transform(const double X[12], const double p[3], double q[3]) {
  for (int r = 0; r < 3; r++) q[r] = ((X[r * 4] * p[0] + X[r * 4 + 1] * p[1]) + X[r * 4 + 2] * p[2]) + X[r * 4 + 3];
}

struct Problem {
  std::vector<double> p, n, s;   // [points][3]
  double truth[12];
  int points() const { return (int)p.size() / 3; }
  Problem(uint64_t seed, int count, const double w[3], const double t[3]) {
    Rng rng{seed};
    rigid_from(w, t, truth);
    for (int i = 0; i < count; i++) {
      double pi[3], ni[3], si[3], len = 0.0;
      for (int k = 0; k < 3; k++) pi[k] = 40.0 * rng.unit() - 20.0;          // voxels
      do {
        len = 0.0;
        for (int k = 0; k < 3; k++) { ni[k] = 2.0 * rng.unit() - 1.0; len += ni[k] * ni[k]; }
      } while (len < 0.01);
      for (int k = 0; k < 3; k++) ni[k] /= sqrt(len);
      transform(truth, pi, si);
      for (int k = 0; k < 3; k++) { p.push_back(pi[k]); n.push_back(ni[k]); s.push_back(si[k]); }
    }
  }
  // the totals of one evaluation at X, one row of 33: every point is a candidate, |b| > gate is a miss
  void evaluate(const double X[12], double gate, Evaluation33 &ev) const {
    double row[kRegSums] = {0};
    for (int i = 0; i < points(); i++) {
      double q[3];
      transform(X, &p[3 * i], q);
      const double *g = &n[3 * i];
      const double b = -(g[0] * (q[0] - s[3 * i]) + g[1] * (q[1] - s[3 * i + 1]) + g[2] * (q[2] - s[3 * i + 2]));
      row[32] += 1.0;
      if (fabs(b) > gate) continue;
      const double A[6] = {q[1] * g[2] - q[2] * g[1], q[2] * g[0] - q[0] * g[2], q[0] * g[1] - q[1] * g[0], g[0], g[1], g[2]};
      for (int k = 0, c = 0; k < 6; k++) {
        row[21 + k] += b * A[k];
        for (int j = 0; j <= k; j++, c++) row[c] += A[k] * A[j];
      }
      row[27] += b * b;
      row[28] += 1.0;
      for (int k = 0; k < 3; k++) row[29 + k] += q[k];
    }
    ev.sum_rows(row, 0, 1);
  }
  // how far X is from the truth: the rotation angle of E = X inv(truth), and how far E moves the centroid of the targets
  void error(const double X[12], double &rot, double &tr) const {
    double inv[12], E[12], c[3] = {0, 0, 0}, Ec[3];
    rigid_inverse(truth, inv);
    rigid_product(X, inv, E);
    const double cosine = std::min(1.0, std::max(-1.0, (E[0] + E[5] + E[10] - 1.0) / 2.0));
    const double sine = 0.5 * sqrt((E[9] - E[6]) * (E[9] - E[6]) + (E[2] - E[8]) * (E[2] - E[8]) + (E[4] - E[1]) * (E[4] - E[1]));
    rot = atan2(sine, cosine);
    for (int i = 0; i < points(); i++)
      for (int k = 0; k < 3; k++) c[k] += s[3 * i + k] / points();
    transform(E, c, Ec);
    tr = sqrt((Ec[0] - c[0]) * (Ec[0] - c[0]) + (Ec[1] - c[1]) * (Ec[1] - c[1]) + (Ec[2] - c[2]) * (Ec[2] - c[2]));
  }
};

struct Settings {
  int max_evaluations = 30, min_valid = 50;
  double gate = 1e9, term_rotation = 1e-5, term_translation = 1e-3;
  bool trials_cost_more = false;   // every trial comes back with a larger sum of squares than the state it was tried from
};

void print_pose(const char *name, const double X[12]) {
  printf("%s", name);
  for (int k = 0; k < 12; k++) printf(" %.17g", X[k]);
  printf("\n");
}

// B blocks, block b: problem[b] from start[b].  The joint cost is the gated cost over all blocks' candidates.
void run_case(const char *name, const std::vector<const Problem *> &problems, std::vector<std::vector<double>> X, const Settings &st) {
  const int B = (int)problems.size();
  const double gate2 = st.gate * st.gate;
  const std::vector<std::vector<double>> start = X;
  std::vector<Evaluation33> good(B), ev(B);
  std::vector<double> c((size_t)3 * B);
  auto joint = [&](const std::vector<Evaluation33> &e) {
    double num = 0.0, den = 0.0;
    for (int b = 0; b < B; b++) { num += e[b].gated_sum(gate2); den += (double)e[b].candidates; }
    return den > 0.0 ? num / den : gate2;
  };
  bool start_ok = true;
  for (int b = 0; b < B; b++) {
    problems[b]->evaluate(X[b].data(), st.gate, good[b]);
    start_ok = start_ok && good[b].valid >= st.min_valid;
  }
  std::string trail, norms;
  LmOutcome lm;
  const int rc = lm_iterate(
      6 * B, start_ok, st.max_evaluations, st.term_rotation, st.term_translation,
      [&](double *H, double *g) {
        std::fill_n(H, (size_t)36 * B * B, 0.0);
        for (int b = 0; b < B; b++) {
          double Hc[36];
          pivot_sums(good[b].sums, &c[3 * b], Hc, g + 6 * b);
          for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) H[(size_t)(6 * b + i) * (6 * B) + 6 * b + j] = Hc[i * 6 + j];
        }
      },
      [&](const double *y) -> int {
        std::vector<std::vector<double>> trial = X;
        bool valid = true;
        for (int b = 0; b < B; b++) {
          apply_increment(y + 6 * b, &c[3 * b], X[b].data(), trial[b].data());
          problems[b]->evaluate(trial[b].data(), st.gate, ev[b]);
          if (st.trials_cost_more) ev[b].sums[27] = good[b].sums[27] + 1.0;
          valid = valid && ev[b].valid >= st.min_valid;
        }
        const bool adopted = valid && joint(ev) < joint(good);
        trail += adopted ? 'A' : 'R';
        if (adopted) {
          X = trial;
          good = ev;
          // the block norms of every adopted step: rotation and translation, block by block
          char buf[128];
          for (int b = 0; b < B; b++) {
            const double *yb = y + 6 * b;
            snprintf(buf, sizeof buf, " %.17g %.17g", sqrt(yb[0] * yb[0] + yb[1] * yb[1] + yb[2] * yb[2]),
                     sqrt(yb[3] * yb[3] + yb[4] * yb[4] + yb[5] * yb[5]));
            norms += buf;
          }
          norms += " ;";
        }
        return adopted ? 1 : 0;
      },
      lm);
  printf("case %s\n", name);
  printf("rc %d\n", rc);
  printf("trail %s\n", trail.empty() ? "-" : trail.c_str());
  printf("evaluations %d\n", lm.evaluations);
  printf("stop %d\n", lm.stop);
  printf("accepted_any %d\n", lm.accepted_any ? 1 : 0);
  printf("conditioning %.17g\n", lm.conditioning);
  printf("step_norms%s\n", norms.empty() ? " -" : norms.c_str());
  for (int b = 0; b < B; b++) {
    double rot, tr;
    problems[b]->error(X[b].data(), rot, tr);
    print_pose("X", X[b].data());
    printf("error %.17g %.17g\n", rot, tr);
    printf("untouched %d\n", memcmp(X[b].data(), start[b].data(), 12 * sizeof(double)) == 0 ? 1 : 0);
  }
}

// a / vs in float32 against the double quotient rounded to float32, on `pairs` pseudo-random pairs: a of either sign over
// forty binades, vs (a voxel size) over twelve
long long division_mismatches(long long pairs) {
  Rng rng{0x9e3779b97f4a7c15ull};
  long long bad = 0;
  for (long long i = 0; i < pairs; i++) {
    const uint32_t ua = (rng.next() & 0x807fffffu) | ((107u + rng.next() % 40u) << 23);
    const uint32_t uv = (rng.next() & 0x007fffffu) | ((115u + rng.next() % 12u) << 23);
    float a, vs;
    memcpy(&a, &ua, 4);
    memcpy(&vs, &uv, 4);
    const float in_float = a / vs, in_double = (float)((double)a / (double)vs);
    bad += memcmp(&in_float, &in_double, 4) != 0;
  }
  return bad;
}

}  // namespace

int main() {
  const double w[3] = {0.02, -0.03, 0.015}, t[3] = {0.8, -0.5, 0.3}, w2[3] = {-0.01, 0.02, 0.03}, t2[3] = {-0.4, 0.2, 0.6};
  const Problem one(1, 300, w, t), two(2, 200, w2, t2);
  // a start some way off the truth
  const double dw[3] = {0.03, 0.02, -0.025}, dt[3] = {0.5, -0.4, 0.3};
  double off[12];
  auto started = [&](const Problem &pr) {
    rigid_from(dw, dt, off);
    std::vector<double> X(12);
    rigid_product(off, pr.truth, X.data());
    return X;
  };
  const std::vector<double> truth_one(one.truth, one.truth + 12);

  Settings st;
  run_case("zero_residual", {&one}, {started(one)}, st);

  Settings few = st;
  few.max_evaluations = 3;
  few.term_rotation = few.term_translation = 0.0;   // (no step is below these)
  run_case("max_evaluations", {&one}, {started(one)}, few);

  Settings worse = st;
  worse.trials_cost_more = true;
  run_case("never_cheaper", {&one}, {started(one)}, worse);

  Settings starved = st;
  starved.min_valid = one.points() + 1;
  run_case("too_few_valid", {&one}, {started(one)}, starved);

  // two blocks: the first starts at its truth, the second does not
  run_case("two_blocks", {&one, &two}, {truth_one, started(two)}, st);

  printf("division_mismatches %lld of %lld\n", division_mismatches(1000000), 1000000LL);
  return 0;
}
