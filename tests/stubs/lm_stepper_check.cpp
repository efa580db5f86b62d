// lm_stepper_check.cpp -- LmStepper of csrc/register_host.h against lm_iterate, without HIP (tests/test_lm_stepper.py).
//
// The problems are lm_check.cpp's kind: points with a plane of their own through their true image, the 33 sums built here
// in double.  Every problem is run three ways -- by lm_iterate, by a stepper of its own driven alone, and by a stepper
// advanced round by round next to the other problems' steppers (each round proposes for every problem that has not
// stopped, evaluates the proposals as one list, then hands out the verdicts) -- and each run records, per evaluation, the
// damping it was proposed with, the verdict and the accepted state after it.  The program prints the three records of every
// problem as hexadecimal doubles; the test compares them as text, so equal means bit for bit.
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

void rigid_from(const double w[3], const double t[3], double out[12]) {
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, zero[3] = {0, 0, 0}, y[6] = {w[0], w[1], w[2], t[0], t[1], t[2]};
  apply_increment(y, zero, I, out);
}
void transform(const double X[12], const double p[3], double q[3]) {
  for (int r = 0; r < 3; r++) q[r] = ((X[r * 4] * p[0] + X[r * 4 + 1] * p[1]) + X[r * 4 + 2] * p[2]) + X[r * 4 + 3];
}

struct Settings {
  int max_evaluations = 30, min_valid = 50;
  double gate = 1e9, term_rotation = 1e-5, term_translation = 1e-3;
  bool trials_cost_more = false;   // every trial comes back with a larger sum of squares than the state it was tried from
  int worse_every = 0;             // ... every worse_every-th trial does
};

struct Problem {
  std::string name;
  std::vector<double> p, n, s;   // [points][3]
  double truth[12], start[12];
  Settings st;
  int points() const { return (int)p.size() / 3; }
  Problem(const char *nm, uint64_t seed, int count, const double w[3], const double t[3], const double dw[3], const double dt[3],
          const Settings &settings)
      : name(nm), st(settings) {
    Rng rng{seed};
    double off[12];
    rigid_from(w, t, truth);
    rigid_from(dw, dt, off);
    rigid_product(off, truth, start);
    for (int i = 0; i < count; i++) {
      double pi[3], ni[3], si[3], len = 0.0;
      for (int k = 0; k < 3; k++) pi[k] = 40.0 * rng.unit() - 20.0;
      do {
        len = 0.0;
        for (int k = 0; k < 3; k++) { ni[k] = 2.0 * rng.unit() - 1.0; len += ni[k] * ni[k]; }
      } while (len < 0.01);
      for (int k = 0; k < 3; k++) ni[k] /= sqrt(len);
      transform(truth, pi, si);
      for (int k = 0; k < 3; k++) { p.push_back(pi[k]); n.push_back(ni[k]); s.push_back(si[k]); }
    }
  }
  void evaluate(const double X[12], Evaluation33 &ev) const {
    double row[kRegSums] = {0};
    for (int i = 0; i < points(); i++) {
      double q[3];
      transform(X, &p[3 * i], q);
      const double *g = &n[3 * i];
      const double b = -(g[0] * (q[0] - s[3 * i]) + g[1] * (q[1] - s[3 * i + 1]) + g[2] * (q[2] - s[3 * i + 2]));
      row[32] += 1.0;
      if (fabs(b) > st.gate) continue;
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
};

// one problem's accepted state and the record of its run
struct Run {
  const Problem *pr;
  double X[12], trial[12], c[3];
  Evaluation33 good;
  std::string record;
  LmOutcome out;
  int trials = 0;
  explicit Run(const Problem *problem) : pr(problem) {
    memcpy(X, pr->start, sizeof X);
    pr->evaluate(X, good);
  }
  bool start_ok() const { return good.valid >= pr->st.min_valid; }
  double gate2() const { return pr->st.gate * pr->st.gate; }
  void system(double *H, double *g) { pivot_sums(good.sums, c, H, g); }
  void propose_trial(const double *y) { apply_increment(y, c, X, trial); }
  // the verdict on the evaluated trial; adopts it if it is valid and cheaper
  bool judge(Evaluation33 ev) {
    trials++;
    if (pr->st.trials_cost_more || (pr->st.worse_every > 0 && trials % pr->st.worse_every == 0)) ev.sums[27] = good.sums[27] + 1.0;
    const bool adopted = ev.valid >= pr->st.min_valid && ev.gated_cost(gate2()) < good.gated_cost(gate2());
    if (adopted) { memcpy(X, trial, sizeof X); good = ev; }
    return adopted;
  }
  void note(double lambda, bool adopted) {
    char buf[64];
    snprintf(buf, sizeof buf, " %a:%c", lambda, adopted ? 'A' : 'R');
    record += buf;
    for (int k = 0; k < 12; k++) { snprintf(buf, sizeof buf, ",%a", X[k]); record += buf; }
  }
  void print(const char *how) const {
    printf("%s %s evaluations %d stop %d accepted_any %d conditioning %a trail%s\n", pr->name.c_str(), how, out.evaluations, out.stop,
           out.accepted_any ? 1 : 0, out.conditioning, record.empty() ? " -" : record.c_str());
  }
};

// lm_iterate knows no damping to report: the record's lambda is reconstructed by the rules (1, / 10 not below 1e-6, x 10)
void run_iterate(Run &r) {
  double lambda = 1.0;
  const Settings &st = r.pr->st;
  lm_iterate(
      6, r.start_ok(), st.max_evaluations, st.term_rotation, st.term_translation, [&](double *H, double *g) { r.system(H, g); },
      [&](const double *y) -> int {
        Evaluation33 ev;
        r.propose_trial(y);
        r.pr->evaluate(r.trial, ev);
        const bool adopted = r.judge(ev);
        r.note(lambda, adopted);
        lambda = adopted ? std::max(lambda / 10.0, 1e-6) : lambda * 10.0;
        return adopted ? 1 : 0;
      },
      r.out);
}

void begin(LmStepper &lm, const Run &r) {
  const Settings &st = r.pr->st;
  lm.begin(6, r.start_ok(), st.max_evaluations, st.term_rotation, st.term_translation);
}

void run_alone(Run &r) {
  LmStepper lm;
  begin(lm, r);
  while (lm.propose([&](double *H, double *g) { r.system(H, g); })) {
    Evaluation33 ev;
    const double lambda = lm.lambda();
    r.propose_trial(lm.increment());
    r.pr->evaluate(r.trial, ev);
    const bool adopted = r.judge(ev);
    r.note(lambda, adopted);
    lm.verdict(adopted);
  }
  lm.finish([&](double *H, double *g) { r.system(H, g); });
  r.out = lm.out;
}

// all problems round by round: the proposals of a round are evaluated as one compacted list before any verdict is given
int run_interleaved(std::vector<Run> &runs) {
  std::vector<LmStepper> lm(runs.size());
  for (size_t k = 0; k < runs.size(); k++) begin(lm[k], runs[k]);
  int rounds = 0;
  for (;; rounds++) {
    std::vector<size_t> active;
    std::vector<double> lambdas;
    for (size_t k = 0; k < runs.size(); k++) {
      Run &r = runs[k];
      if (!lm[k].propose([&](double *H, double *g) { r.system(H, g); })) continue;
      lambdas.push_back(lm[k].lambda());
      r.propose_trial(lm[k].increment());
      active.push_back(k);
    }
    if (active.empty()) break;
    std::vector<Evaluation33> ev(active.size());
    for (size_t a = 0; a < active.size(); a++) runs[active[a]].pr->evaluate(runs[active[a]].trial, ev[a]);
    for (size_t a = 0; a < active.size(); a++) {
      Run &r = runs[active[a]];
      const bool adopted = r.judge(ev[a]);
      r.note(lambdas[a], adopted);
      lm[active[a]].verdict(adopted);
    }
  }
  for (size_t k = 0; k < runs.size(); k++) {
    Run &r = runs[k];
    lm[k].finish([&](double *H, double *g) { r.system(H, g); });
    r.out = lm[k].out;
  }
  return rounds;
}

}  // namespace

int main() {
  const double w[3] = {0.02, -0.03, 0.015}, t[3] = {0.8, -0.5, 0.3}, w2[3] = {-0.01, 0.02, 0.03}, t2[3] = {-0.4, 0.2, 0.6};
  const double dw[3] = {0.03, 0.02, -0.025}, dt[3] = {0.5, -0.4, 0.3}, none[3] = {0.0, 0.0, 0.0};
  const double far_w[3] = {1.5, 1.0, -1.2}, far_t[3] = {6.0, -4.0, 5.0};
  Settings st, few = st, worse = st, starved = st, gated = st;
  few.max_evaluations = 3;
  few.term_rotation = few.term_translation = 0.0;
  worse.trials_cost_more = true;
  starved.min_valid = 301;
  gated.gate = 6.0;   // a far start under a gate, every third trial made worse: rejected steps between adopted ones
  gated.worse_every = 3;
  const std::vector<Problem> problems = {
      Problem("zero_residual", 1, 300, w, t, dw, dt, st),       Problem("max_evaluations", 1, 300, w, t, dw, dt, few),
      Problem("never_cheaper", 1, 300, w, t, dw, dt, worse),    Problem("too_few_valid", 1, 300, w, t, dw, dt, starved),
      Problem("at_the_truth", 2, 200, w2, t2, none, none, st),  Problem("second", 2, 200, w2, t2, dw, dt, st),
      Problem("far_gated", 3, 400, w, t2, far_w, far_t, gated),
  };
  std::vector<Run> together;
  for (const Problem &pr : problems) {
    Run a(&pr), b(&pr);
    run_iterate(a);
    run_alone(b);
    a.print("iterate");
    b.print("alone");
    together.emplace_back(&pr);
  }
  const int rounds = run_interleaved(together);
  for (const Run &r : together) r.print("interleaved");
  printf("rounds %d\n", rounds);
  return 0;
}
