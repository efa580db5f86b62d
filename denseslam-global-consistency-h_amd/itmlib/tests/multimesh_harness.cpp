// multimesh_harness.cpp -- drives ITMMainEngine::SaveAllLocalMapsToMesh through the ITMLib mirror: local maps built as
// multimap_harness.cpp builds them (a new local map every K keyframes, anchored at that keyframe's pose, every keyframe
// fused into the newest map at its pose relative to that map), then one OBJ of all maps in the global frame.
//
//   multimesh_harness <frames.bin> <out.bin> <K> <mesh.obj>
// frames.bin: as driver_harness.cpp
// out.bin:    int32 nMaps; float T[nMaps][16] (estimatedGlobalPose.GetM(), column-major); float Mfused[N][16] (the
//             pose_d each keyframe was fused with)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class MultiMeshHarness : public ITMMainEngine {
 public:
  MultiMeshHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~MultiMeshHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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
  ITMIntrinsics DepthIntrinsics() const { return this->viewBuilder->GetCalib()->intrinsics_d; }

 private:
  ITMUChar4Image *rgb_itm_;
  ITMShortImage *raw_depth_itm_;
  WeightParams fusion_weight_params_;
};

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s frames.bin out.bin K mesh.obj\n", argv[0]); return 2; }
  const int K = atoi(argv[3]);
  if (K <= 0) { fprintf(stderr, "K must be positive\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror("frames"); return 2; }
  int32_t hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  const int W = hdr[0], H = hdr[1], N = hdr[2];
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
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4) return 2;
  fclose(f);
  if (N <= 0) return 2;

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
    MultiMeshHarness drv(settings, calib, Vector2i(W, H));
    ITMVoxelMapGraphManager *maps = drv.GetMapManager();

    std::vector<Matrix4f> fused(N);
    for (int i = 0; i < N; i++) {
      if (i % K == 0) {   // shouldStartNewLocalMap: a new map, anchored at this keyframe (DenseSlam.cpp:133-141)
        const int idx = maps->createNewLocalMap();
        ITMPose anchor;
        anchor.SetM(poses[i]);
        maps->setEstimatedGlobalPose(idx, anchor);
      }
      ITMLocalMap *current = maps->getLocalMap(maps->numLocalMaps() - 1);
      Matrix4f Twc, Tcurrmap_w = current->estimatedGlobalPose.GetM();
      poses[i].inv(Twc);
      current->trackingState->pose_d->SetInvM(Tcurrmap_w * Twc);   // SetPoseLocalMap
      fused[i] = current->trackingState->pose_d->GetM();
      drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
      drv.IntegrateLocalMap(current);
    }

    drv.SaveAllLocalMapsToMesh(argv[4]);

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    const int32_t n_maps = maps->numLocalMaps();
    fwrite(&n_maps, 4, 1, o);
    for (int i = 0; i < n_maps; i++) fwrite(maps->getLocalMap(i)->estimatedGlobalPose.GetM().m, 4, 16, o);
    for (int i = 0; i < N; i++) fwrite(fused[i].m, 4, 16, o);
    fclose(o);
    printf("multimesh_harness ok: %d keyframes, %d local maps\n", N, n_maps);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "multimesh_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
