// register_graph_harness.cpp -- drives ITMMainEngine::AlignLocalMaps through the ITMLib mirror: three local maps from the
// same keyframes, maps 1 and 2 anchored with known offsets D1, D2 that their estimatedGlobalPoses do not know (map k's frame
// is Dk times map 0's, all maps report map 0's anchor), then AlignLocalMaps(pairs, anchor).
//
//   register_graph_harness <frames.bin> <out.bin>
// frames.bin: as driver_harness.cpp, followed by float D1[16], D2[16] (column-major, metres), int32 num_pairs, anchor,
//             int32 pairs[num_pairs][2]
// out.bin:    float T_before[3][16], T_after[3][16] (estimatedGlobalPose.GetM(), column-major);
//             float Mfused[3][N][16] (the pose_d each keyframe was fused with, map by map);
//             dslam_register_graph_result; dslam_register_pair_result[num_pairs]; int32 AlignLocalMaps' return value
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class RegisterGraphHarness : public ITMMainEngine {
 public:
  RegisterGraphHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~RegisterGraphHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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
  Matrix4f D[3];
  D[0].setIdentity();
  int32_t gp[2];
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4 || fread(D[1].m, 4, 16, f) != 16 ||
      fread(D[2].m, 4, 16, f) != 16 || fread(gp, 4, 2, f) != 2)
    return 2;
  const int num_pairs = gp[0], anchor_map = gp[1];
  if (num_pairs <= 0 || num_pairs > DSLAM_MAX_REGISTER_PAIRS) return 2;
  std::vector<int32_t> pairs((size_t)num_pairs * 2);
  if (fread(pairs.data(), 4, pairs.size(), f) != pairs.size()) return 2;
  fclose(f);

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
    RegisterGraphHarness drv(settings, calib, Vector2i(W, H));
    ITMVoxelMapGraphManager *maps = drv.GetMapManager();

    ITMPose anchor;
    anchor.SetM(poses[0]);
    std::vector<Matrix4f> fused(3 * (size_t)N);
    for (int k = 0; k < 3; k++) {
      const int idx = maps->createNewLocalMap();
      ITMLocalMap *current = maps->getLocalMap(idx);
      // where the map really is: map k's frame is Dk times map 0's
      const Matrix4f Tmap_w = k == 0 ? anchor.GetM() : D[k] * anchor.GetM();
      for (int i = 0; i < N; i++) {
        Matrix4f Twc;
        poses[i].inv(Twc);
        current->trackingState->pose_d->SetInvM(Tmap_w * Twc);   // SetPoseLocalMap
        fused[(size_t)k * N + i] = current->trackingState->pose_d->GetM();
        drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
        drv.IntegrateLocalMap(current);
      }
      maps->setEstimatedGlobalPose(idx, anchor);   // ... and where it is believed to be
    }

    Matrix4f before[3];
    for (int k = 0; k < 3; k++) before[k] = maps->getLocalMap(k)->estimatedGlobalPose.GetM();
    dslam_register_graph_result res;
    std::vector<dslam_register_pair_result> pres((size_t)num_pairs);
    const int32_t aligned = drv.AlignLocalMaps(reinterpret_cast<const int (*)[2]>(pairs.data()), num_pairs, anchor_map, &res,
                                               pres.data()) ? 1 : 0;

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    for (int k = 0; k < 3; k++) fwrite(before[k].m, 4, 16, o);
    for (int k = 0; k < 3; k++) fwrite(maps->getLocalMap(k)->estimatedGlobalPose.GetM().m, 4, 16, o);
    for (size_t i = 0; i < fused.size(); i++) fwrite(fused[i].m, 4, 16, o);
    fwrite(&res, sizeof(res), 1, o);
    fwrite(pres.data(), sizeof(dslam_register_pair_result), pres.size(), o);
    fwrite(&aligned, 4, 1, o);
    fclose(o);
    printf("register_graph_harness ok: %d keyframes, %d pairs (%d active), stop reason %d after %d evaluations, cost %g -> %g\n", N,
           num_pairs, res.active_pairs, res.stop_reason, res.evaluations, res.cost_first, res.cost_last);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "register_graph_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
