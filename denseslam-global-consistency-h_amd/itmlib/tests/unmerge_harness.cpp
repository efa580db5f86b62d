// unmerge_harness.cpp -- drives ITMMainEngine::UnmergeLocalMap and RemergeLocalMap through the ITMLib mirror: two local
// maps from the same keyframes, the second anchored with a known offset D that its estimatedGlobalPose does not know (as
// merge_harness.cpp).  MergeLocalMap(1, 0) under the poses as they are believed (X_old = LocalMapTransform(1, 0)), then
// UnmergeLocalMap(1, 0, X_old); MergeLocalMap(1, 0) once more, the source's estimatedGlobalPose corrected to where the
// map really is, and RemergeLocalMap(1, 0, X_old).
//
//   unmerge_harness <frames.bin> <out.bin>
// frames.bin: as register_harness.cpp
// out.bin:    float X_old[16] (LocalMapTransform(1, 0) before the correction, column-major);
//             float Mfused[2][N][16] (the pose_d each keyframe was fused with, map 0 then map 1);
//             dslam_merge_result of the first merge; dslam_unmerge_result; int32 UnmergeLocalMap's return value;
//             map 0 after the unmerge;
//             float X_new[16] (LocalMapTransform(1, 0) after the correction);
//             dslam_unmerge_result and dslam_merge_result of the remerge; int32 RemergeLocalMap's return value;
//             map 0 after the remerge.
//             A map: int32 last_free, last_free_ex; its hash table, allocation list, excess list and voxel blocks as the
//             dslam_download_* calls return them
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class UnmergeHarness : public ITMMainEngine {
 public:
  UnmergeHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~UnmergeHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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
  Matrix4f D;
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4 || fread(D.m, 4, 16, f) != 16) return 2;
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
    UnmergeHarness drv(settings, calib, Vector2i(W, H));
    ITMVoxelMapGraphManager *maps = drv.GetMapManager();

    ITMPose anchor;
    anchor.SetM(poses[0]);
    std::vector<Matrix4f> fused(2 * (size_t)N);
    for (int k = 0; k < 2; k++) {
      const int idx = maps->createNewLocalMap();
      ITMLocalMap *current = maps->getLocalMap(idx);
      // where the map really is: map 1's frame is D times map 0's
      const Matrix4f Tmap_w = k == 0 ? anchor.GetM() : D * anchor.GetM();
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

    dslam_engine *e = drv.GetDslamEngine();
    const dslam_scene *s0 = maps->getLocalMap(0)->scene->handle;
    const size_t n_entries = (size_t)ip[2] + ip[3], n_local = (size_t)ip[1];
    std::vector<dslam_hash_entry> table(n_entries);
    std::vector<int32_t> alloc_list(n_local), excess_list((size_t)ip[3]);
    std::vector<dslam_voxel> voxels(n_local * 512);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    auto write_map0 = [&]() {
      dslam_stats st;
      if (dslam_download_hash_table(e, s0, table.data()) < 0 || dslam_download_allocation_list(e, s0, alloc_list.data()) < 0 ||
          dslam_download_excess_list(e, s0, excess_list.data()) < 0 ||
          dslam_download_voxel_blocks(e, s0, 0, (int)n_local, voxels.data()) < 0 || dslam_get_stats(e, s0, nullptr, &st) < 0)
        throw std::runtime_error(dslam_last_error());
      const int32_t tops[2] = {st.last_free_block_id, st.last_free_excess_id};
      fwrite(tops, 4, 2, o);
      fwrite(table.data(), sizeof(dslam_hash_entry), table.size(), o);
      fwrite(alloc_list.data(), 4, alloc_list.size(), o);
      fwrite(excess_list.data(), 4, excess_list.size(), o);
      fwrite(voxels.data(), sizeof(dslam_voxel), voxels.size(), o);
    };

    float X_old[16], X_new[16];
    drv.LocalMapTransform(1, 0, X_old);
    dslam_merge_result m1, again, m2;
    dslam_unmerge_result u1, u2;
    drv.MergeLocalMap(1, 0, &m1);
    const int32_t unmerged = drv.UnmergeLocalMap(1, 0, X_old, &u1) ? 1 : 0;
    fwrite(X_old, 4, 16, o);
    for (size_t i = 0; i < fused.size(); i++) fwrite(fused[i].m, 4, 16, o);
    fwrite(&m1, sizeof(m1), 1, o);
    fwrite(&u1, sizeof(u1), 1, o);
    fwrite(&unmerged, 4, 1, o);
    write_map0();
    // merged once more, then the correction: map 1's pose as it really is
    drv.MergeLocalMap(1, 0, &again);
    ITMPose truth;
    truth.SetM(D * anchor.GetM());
    maps->setEstimatedGlobalPose(1, truth);
    drv.LocalMapTransform(1, 0, X_new);
    const int32_t remerged = drv.RemergeLocalMap(1, 0, X_old, &u2, &m2) ? 1 : 0;
    fwrite(X_new, 4, 16, o);
    fwrite(&u2, sizeof(u2), 1, o);
    fwrite(&m2, sizeof(m2), 1, o);
    fwrite(&remerged, 4, 1, o);
    write_map0();
    fclose(o);
    printf("unmerge_harness ok: %d keyframes; merge: %d blocks touched, %lld voxels changed; unmerge: %d touched, %lld changed; "
           "remerge: %lld out, %lld in\n", N, m1.blocks_touched, (long long)m1.voxels_changed, u1.blocks_touched,
           (long long)u1.voxels_changed, (long long)u2.voxels_changed, (long long)m2.voxels_changed);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "unmerge_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
