// relocalise_harness.cpp -- drives ITMMainEngine::RelocaliseAllLocalMaps through the ITMLib mirror: two local maps fused
// from keyframes (map 1's frame is D times map 0's, and its estimatedGlobalPose says so), then a third local map that has
// just been created and holds nothing -- the current one -- whose pose_d is a start pose farther off the last frame's true
// pose than the truncation band; RelocaliseAllLocalMaps(current, lattice, level, keep) finds the frame again against all
// three maps.
//
//   relocalise_harness <frames.bin> <out.bin>
// frames.bin: as track_sdf_harness.cpp, followed by a dslam_pose_lattice and int32 score_level, keep
// out.bin:    as track_sdf_harness.cpp: float T[3][16]; float pose_d_before[16], pose_d_after[16] (the current map's);
//             float Mfused[2][N][16]; the winner's dslam_track_sdf_result; int32 RelocaliseAllLocalMaps' return value
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class RelocaliseHarness : public ITMMainEngine {
 public:
  RelocaliseHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~RelocaliseHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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
  const int W = hdr[0], H = hdr[1], N = hdr[2] - 1;
  if (N <= 0) return 2;
  std::vector<std::vector<uint8_t>> rgba(N + 1, std::vector<uint8_t>((size_t)W * H * 4));
  std::vector<std::vector<int16_t>> depth(N + 1, std::vector<int16_t>((size_t)W * H));
  std::vector<Matrix4f> poses(N + 1);
  for (int i = 0; i <= N; i++) {
    if (fread(rgba[i].data(), 1, rgba[i].size(), f) != rgba[i].size()) return 2;
    if (fread(depth[i].data(), 2, depth[i].size(), f) != depth[i].size()) return 2;
    if (fread(poses[i].m, 4, 16, f) != 16) return 2;
  }
  float intr[4], sp[4];
  int32_t ip[4];
  Matrix4f D, E;
  dslam_pose_lattice lattice;
  int32_t how[2];
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4 || fread(D.m, 4, 16, f) != 16 ||
      fread(E.m, 4, 16, f) != 16 || fread(&lattice, sizeof lattice, 1, f) != 1 || fread(how, 4, 2, f) != 2)
    return 2;
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
    RelocaliseHarness drv(settings, calib, Vector2i(W, H));
    ITMVoxelMapGraphManager *maps = drv.GetMapManager();

    ITMPose anchor;
    anchor.SetM(poses[0]);
    std::vector<Matrix4f> fused(2 * (size_t)N);
    for (int k = 0; k < 2; k++) {
      const int idx = maps->createNewLocalMap();
      ITMLocalMap *m = maps->getLocalMap(idx);
      ITMPose global;
      global.SetM(k == 0 ? anchor.GetM() : D * anchor.GetM());
      for (int i = 0; i < N; i++) {
        Matrix4f Twc;
        poses[i].inv(Twc);
        m->trackingState->pose_d->SetInvM(global.GetM() * Twc);   // SetPoseLocalMap
        fused[(size_t)k * N + i] = m->trackingState->pose_d->GetM();
        drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
        drv.IntegrateLocalMap(m);
      }
      maps->setEstimatedGlobalPose(idx, global);
    }
    // shouldStartNewLocalMap -> createNewLocalMap (DenseSlam.cpp:133-141, 260-261): the current map holds nothing
    const int cur = maps->createNewLocalMap();
    ITMLocalMap *current = maps->getLocalMap(cur);
    ITMPose global;
    global.SetM(E * anchor.GetM());
    maps->setEstimatedGlobalPose(cur, global);
    Matrix4f Tinv;
    global.GetM().inv(Tinv);
    current->trackingState->pose_d->SetM(poses[N] * Tinv);
    const Matrix4f before = current->trackingState->pose_d->GetM();
    drv.UpdateView(rgba[N].data(), depth[N].data(), (double)N);
    dslam_track_sdf_result res;
    const int32_t tracked = drv.RelocaliseAllLocalMaps(current, lattice, how[0], how[1], &res) ? 1 : 0;

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    for (int k = 0; k < 3; k++) fwrite(maps->getLocalMap(k)->estimatedGlobalPose.GetM().m, 4, 16, o);
    fwrite(before.m, 4, 16, o);
    fwrite(current->trackingState->pose_d->GetM().m, 4, 16, o);
    for (size_t i = 0; i < fused.size(); i++) fwrite(fused[i].m, 4, 16, o);
    fwrite(&res, sizeof(res), 1, o);
    fwrite(&tracked, 4, 1, o);
    fclose(o);
    printf("relocalise_harness ok: %d keyframes, winner: stop reason %d after %d evaluations, levels %d, %d of %d valid\n", N,
           res.stop_reason, res.evaluations, res.levels_stepped, res.valid_last, res.candidates);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "relocalise_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
