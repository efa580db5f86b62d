// Fixture driver for tests/golden/make_sflow_golden.py: runs libviso2's Matcher on two stereo pairs and dumps what it
// computed.  The include path of matcher.h comes from the compile line; nothing of libviso2 is part of this file.
//
// usage: driver IN OUT
//   IN   int32 header {W, H, method, half_resolution, multi_stage, refinement, nms_n, nms_tau, match_binsize, match_radius,
//        match_disp_tolerance, has_right}, then the grey images 1p, 2p, 1c, 2c as W H bytes each
//   OUT  int32 words: for each of m1p1 m2p1 m1c1 m2c1 m1p2 m2p2 m1c2 m2c2 the count n and n records of 12 words; then the
//        raw matches (count, 12 words each), then getMatches() alike; then the wall time of the two pushBack calls and of
//        matchFeatures in microseconds
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#define private public
#include "matcher.h"
#undef private

static void put_features(std::vector<int32_t> &out, const int32_t *m, int32_t n) {
  out.push_back(m ? n : 0);
  if (m) out.insert(out.end(), m, m + 12 * (size_t)n);
}

static void put_matches(std::vector<int32_t> &out, const std::vector<Matcher::p_match> &v) {
  out.push_back((int32_t)v.size());
  for (const Matcher::p_match &p : v) {
    const int32_t rec[12] = {(int32_t)p.u1p, (int32_t)p.v1p, p.i1p, (int32_t)p.u2p, (int32_t)p.v2p, p.i2p,
                             (int32_t)p.u1c, (int32_t)p.v1c, p.i1c, (int32_t)p.u2c, (int32_t)p.v2c, p.i2c};
    out.insert(out.end(), rec, rec + 12);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[12];
  if (fread(h, 4, 12, f) != 12) return 4;
  const int W = h[0], H = h[1], method = h[2];
  std::vector<uint8_t> img[4];
  for (auto &i : img) {
    i.resize((size_t)W * H);
    if (fread(i.data(), 1, i.size(), f) != i.size()) return 5;
  }
  fclose(f);

  Matcher::parameters p;
  p.half_resolution = h[3]; p.multi_stage = h[4]; p.refinement = h[5];
  p.nms_n = h[6]; p.nms_tau = h[7]; p.match_binsize = h[8]; p.match_radius = h[9]; p.match_disp_tolerance = h[10];
  Matcher m(p);
  int32_t dims[3] = {W, H, W};
  const auto t0 = std::chrono::steady_clock::now();
  m.pushBack(img[0].data(), h[11] ? img[1].data() : nullptr, dims, false);
  m.pushBack(img[2].data(), h[11] ? img[3].data() : nullptr, dims, false);
  const auto t1 = std::chrono::steady_clock::now();
  m.matchFeatures(method);
  const auto t2 = std::chrono::steady_clock::now();

  std::vector<int32_t> out;
  put_features(out, m.m1p1, m.n1p1); put_features(out, m.m2p1, m.n2p1);
  put_features(out, m.m1c1, m.n1c1); put_features(out, m.m2c1, m.n2c1);
  put_features(out, m.m1p2, m.n1p2); put_features(out, m.m2p2, m.n2p2);
  put_features(out, m.m1c2, m.n1c2); put_features(out, m.m2c2, m.n2c2);
  put_matches(out, m.getRawMatches());
  put_matches(out, m.getMatches());
  out.push_back((int32_t)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count());
  out.push_back((int32_t)std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count());
  FILE *g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 4, out.size(), g) != out.size()) return 6;
  fclose(g);
  return 0;
}
