// overlap_harness.cpp -- drives ITMMainEngine::SurveyLocalMapOverlaps and AlignAllLocalMaps through the ITMLib mirror: three
// local maps from the same keyframes, maps 1 and 2 anchored with known offsets D1, D2 that their estimatedGlobalPoses do not
// know (as register_graph_harness.cpp), and optionally a fourth map of the same keyframes whose estimatedGlobalPose puts it
// 3 m away.  The overlaps are surveyed and the pairs selected; AlignAllLocalMaps(anchor) runs; the poses are put back and
// AlignLocalMaps runs on the selected pairs, for comparison.
//
//   overlap_harness <frames.bin> <out.bin>
// frames.bin: as driver_harness.cpp, followed by float D1[16], D2[16] (column-major, metres), int32 anchor, with_far
// out.bin:    int32 n (3 or 4); float T_before[n][16], T_all[n][16] (after AlignAllLocalMaps), T_pairs[n][16] (after
//             AlignLocalMaps on the selected pairs), estimatedGlobalPose.GetM(), column-major;
//             float Mfused[n][N][16] (the pose_d each keyframe was fused with, map by map);
//             int32 live[n], shared_octants[n][n]; dslam_pair_select_result; int32 component[n]; int32 pairs[selected][2];
//             int32 AlignAllLocalMaps' return value, int32 the number of pairs it reported, dslam_register_graph_result,
//             dslam_register_pair_result[selected] (zeros when it made no registration call);
//             the same four items for AlignLocalMaps on the selected pairs (absent when nothing was selected or the maps
//             are not connected: int32 -1 in place of the return value, then nothing)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class OverlapHarness : public ITMMainEngine {
 public:
  OverlapHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~OverlapHarness() { delete rgb_itm_; delete raw_depth_itm_; }
  // InfiniTamDriver::UpdateView (InfiniTamDriver.cpp:280-288), as driver_harness.cpp
  void UpdateView(const uint8_t *rgba, const int16_t *depth, double timestamp) {
    memcpy(rgb_itm_->GetData(MEMORYDEVICE_CPU), rgba, rgb_itm_->dataSize * 4);
    memcpy(raw_depth_itm_->GetData(MEMORYDEVICE_CPU), depth, raw_depth_itm_->dataSize * 2);
    this->viewBuilder->UpdateView(&view, rgb_itm_, raw_depth_itm_, timestamp, settings->useBilateralFilter);
  }
  // InfiniTamDriver::IntegrateLocalMap (InfiniTamDriver.h:187-192)
  void IntegrateLocalMap(const ITMLocalMap *m) const {
    this->denseMapper->SetFusionWeightParams(fusion_weight_params_);
    this->denseMapper->ProcessFrame(this->view, m->trackingState, m->scene, m->renderState, false, false);
  }
  ITMVoxelMapGraphManager *GetMapManager() const { return this->mapManager; }

 private:
  ITMUChar4Image *rgb_itm_;
  ITMShortImage *raw_depth_itm_;
  WeightParams fusion_weight_params_;
};

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s frames.bin out.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror("frames"); return 2; }
  int32_t hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  const int W = hdr[0], H = hdr[1], N = hdr[2];
  if (N <= 0) return 2;
  std::vector<std::vector<uint8_t>> rgba(N, std::vector<uint8_t>((size_t)W * H * 4));
  std::vector<std::vector<int16_t>> depth(N, std::vector<int16_t>((size_t)W * H));
  std::vector<Matrix4f> poses(N);
  for (int i = 0; i < N; i++) {
    if (fread(rgba[i].data(), 1, rgba[i].size(), f) != rgba[i].size()) return 2;
    if (fread(depth[i].data(), 2, depth[i].size(), f) != depth[i].size()) return 2;
    if (fread(poses[i].m, 4, 16, f) != 16) return 2;
  }
  float intr[4], sp[4];
  int32_t ip[4];
  Matrix4f D[4];
  D[0].setIdentity();
  D[3].setIdentity();
  int32_t gp[2];
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4 || fread(D[1].m, 4, 16, f) != 16 ||
      fread(D[2].m, 4, 16, f) != 16 || fread(gp, 4, 2, f) != 2)
    return 2;
  fclose(f);
  const int anchor_map = gp[0], n_maps = gp[1] ? 4 : 3;

  try {
    ITMLibSettings *settings = new ITMLibSettings();
    settings->sceneParams = ITMSceneParams(sp[1], ip[0], sp[0], sp[2], sp[3], false);
    settings->numLocalBlocks = ip[1]; settings->numBuckets = ip[2]; settings->numExcess = ip[3];
    ITMRGBDCalib *calib = new ITMRGBDCalib;
    ITMIntrinsics intrinsics;
    intrinsics.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)W, (float)H);
    calib->intrinsics_rgb = intrinsics; calib->intrinsics_d = intrinsics;
    Matrix4f identity; identity.setIdentity();
    calib->trafo_rgb_to_depth.SetFrom(identity);
    calib->disparityCalib.SetFrom(1.0f / 1000.0f, 0.0f, ITMDisparityCalib::TRAFO_AFFINE);
    OverlapHarness drv(settings, calib, Vector2i(W, H));
    ITMVoxelMapGraphManager *maps = drv.GetMapManager();

    ITMPose anchor;
    anchor.SetM(poses[0]);
    std::vector<Matrix4f> fused((size_t)n_maps * N);
    for (int k = 0; k < n_maps; k++) {
      const int idx = maps->createNewLocalMap();
      ITMLocalMap *current = maps->getLocalMap(idx);
      // where the map really is: map k's frame is Dk times map 0's
      const Matrix4f Tmap_w = (k == 0 || k == 3) ? anchor.GetM() : D[k] * anchor.GetM();
      for (int i = 0; i < N; i++) {
        Matrix4f Twc;
        poses[i].inv(Twc);
        current->trackingState->pose_d->SetInvM(Tmap_w * Twc);   // SetPoseLocalMap
        fused[(size_t)k * N + i] = current->trackingState->pose_d->GetM();
        drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
        drv.IntegrateLocalMap(current);
      }
      // ... and where it is believed to be: the fourth map 3 m from where it is, along the first keyframe's viewing direction
      // (the maps are less than 3 m deep, so nothing of it then lies inside another map)
      ITMPose believed;
      Matrix4f far;
      far.setIdentity();
      far.m[14] = 3.0f;
      believed.SetM(k == 3 ? far * anchor.GetM() : anchor.GetM());
      maps->setEstimatedGlobalPose(idx, believed);
    }

    std::vector<Matrix4f> before(n_maps), after_all(n_maps), after_pairs(n_maps);
    for (int k = 0; k < n_maps; k++) before[k] = maps->getLocalMap(k)->estimatedGlobalPose.GetM();
    // the survey and the selection, as AlignAllLocalMaps makes them
    std::vector<int32_t> live, shared, component((size_t)n_maps), sel_pairs((size_t)DSLAM_MAX_REGISTER_PAIRS * 2);
    drv.SurveyLocalMapOverlaps(live, shared);
    dslam_pair_select_result sel;
    if (dslam_select_register_pairs(live.data(), shared.data(), n_maps, nullptr, sel_pairs.data(), component.data(), &sel) != DSLAM_OK)
      throw std::runtime_error(std::string("dslam_select_register_pairs: ") + dslam_last_error());
    sel_pairs.resize((size_t)sel.selected * 2);

    dslam_register_graph_result res_all, res_pairs;
    memset(&res_all, 0, sizeof res_all);
    memset(&res_pairs, 0, sizeof res_pairs);
    std::vector<int32_t> all_pairs;
    std::vector<dslam_register_pair_result> pres_all, pres_pairs((size_t)sel.selected);
    const int32_t aligned_all = drv.AlignAllLocalMaps(anchor_map, &res_all, &all_pairs, &pres_all) ? 1 : 0;
    for (int k = 0; k < n_maps; k++) after_all[k] = maps->getLocalMap(k)->estimatedGlobalPose.GetM();
    if (all_pairs != sel_pairs) throw std::runtime_error("AlignAllLocalMaps selected other pairs than the survey and the selection give");
    // the same pairs through AlignLocalMaps, from the same poses
    int32_t aligned_pairs = -1;
    if (sel.selected > 0 && sel.num_components == 1) {
      for (int k = 0; k < n_maps; k++) {
        ITMPose p;
        p.SetM(before[k]);
        maps->setEstimatedGlobalPose(k, p);
      }
      aligned_pairs = drv.AlignLocalMaps(reinterpret_cast<const int (*)[2]>(sel_pairs.data()), sel.selected, anchor_map, &res_pairs,
                                         pres_pairs.data()) ? 1 : 0;
    }
    for (int k = 0; k < n_maps; k++) after_pairs[k] = maps->getLocalMap(k)->estimatedGlobalPose.GetM();

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    const int32_t n32 = n_maps, reported = (int32_t)pres_all.size();
    fwrite(&n32, 4, 1, o);
    for (int k = 0; k < n_maps; k++) fwrite(before[k].m, 4, 16, o);
    for (int k = 0; k < n_maps; k++) fwrite(after_all[k].m, 4, 16, o);
    for (int k = 0; k < n_maps; k++) fwrite(after_pairs[k].m, 4, 16, o);
    for (size_t i = 0; i < fused.size(); i++) fwrite(fused[i].m, 4, 16, o);
    fwrite(live.data(), 4, live.size(), o);
    fwrite(shared.data(), 4, shared.size(), o);
    fwrite(&sel, sizeof(sel), 1, o);
    fwrite(component.data(), 4, component.size(), o);
    fwrite(sel_pairs.data(), 4, sel_pairs.size(), o);
    fwrite(&aligned_all, 4, 1, o);
    fwrite(&reported, 4, 1, o);
    fwrite(&res_all, sizeof(res_all), 1, o);
    fwrite(pres_all.data(), sizeof(dslam_register_pair_result), pres_all.size(), o);
    fwrite(&aligned_pairs, 4, 1, o);
    if (aligned_pairs >= 0) {
      fwrite(&reported, 4, 1, o);
      fwrite(&res_pairs, sizeof(res_pairs), 1, o);
      fwrite(pres_pairs.data(), sizeof(dslam_register_pair_result), pres_pairs.size(), o);
    }
    fclose(o);
    printf("overlap_harness ok: %d maps of %d keyframes, %d pairs selected of %d qualifying, %d component(s); AlignAllLocalMaps %d "
           "(stop reason %d after %d evaluations, cost %g -> %g)\n", n_maps, N, sel.selected, sel.qualifying, sel.num_components,
           aligned_all, res_all.stop_reason, res_all.evaluations, res_all.cost_first, res_all.cost_last);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "overlap_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
