// merge_harness.cpp -- drives ITMMainEngine::MergeLocalMap through the ITMLib mirror: two local maps from the same
// keyframes, the second anchored with a known offset D that its estimatedGlobalPose does not know (as register_harness.cpp),
// then AlignLocalMap(1, 0) and MergeLocalMap(1, 0).  The composite depth image of both maps before the merge and the depth
// image of the merged map alone, from the first keyframe's pose, go out as well.
//
//   merge_harness <frames.bin> <out.bin>
// frames.bin: as register_harness.cpp
// out.bin:    float T_dst[16], T_src_after[16] (estimatedGlobalPose.GetM(), column-major);
//             float Mfused[2][N][16] (the pose_d each keyframe was fused with, map 0 then map 1);
//             dslam_register_result; int32 AlignLocalMap's return value; dslam_merge_result; int32 MergeLocalMap's;
//             float depth_both[H][W], depth_merged[H][W];
//             map 0 after the merge: int32 last_free, last_free_ex; its hash table, allocation list, excess list and
//             voxel blocks as the dslam_download_* calls return them
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class MergeHarness : public ITMMainEngine {
 public:
  MergeHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~MergeHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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
    MergeHarness drv(settings, calib, Vector2i(W, H));
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

    dslam_register_result rres;
    const int32_t aligned = drv.AlignLocalMap(1, 0, &rres) ? 1 : 0;

    // both maps in one image from the first keyframe's pose, then the merge, then map 0 alone from the same camera
    ITMFloatImage depth_both(Vector2i(W, H), true, true), depth_merged(Vector2i(W, H), true, true);
    ITMPose camera;
    camera.SetM(poses[0]);
    ITMIntrinsics k = drv.DepthIntrinsics();
    drv.GetImageAllLocalMaps(nullptr, &depth_both, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &camera, &k);
    dslam_merge_result mres;
    const int32_t merged = drv.MergeLocalMap(1, 0, &mres) ? 1 : 0;
    Matrix4f Tinv;
    maps->getLocalMap(0)->estimatedGlobalPose.GetM().inv(Tinv);
    ITMPose in_map;
    in_map.SetM(poses[0] * Tinv);
    drv.GetImage(nullptr, &depth_merged, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &in_map, &k, maps->getLocalMap(0));

    dslam_engine *e = drv.GetDslamEngine();
    const dslam_scene *s0 = maps->getLocalMap(0)->scene->handle;
    const size_t n_entries = (size_t)ip[2] + ip[3], n_local = (size_t)ip[1];
    std::vector<dslam_hash_entry> table(n_entries);
    std::vector<int32_t> alloc_list(n_local), excess_list((size_t)ip[3]);
    std::vector<dslam_voxel> voxels(n_local * 512);
    dslam_stats st;
    if (dslam_download_hash_table(e, s0, table.data()) < 0 || dslam_download_allocation_list(e, s0, alloc_list.data()) < 0 ||
        dslam_download_excess_list(e, s0, excess_list.data()) < 0 ||
        dslam_download_voxel_blocks(e, s0, 0, (int)n_local, voxels.data()) < 0 || dslam_get_stats(e, s0, nullptr, &st) < 0)
      throw std::runtime_error(dslam_last_error());

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    fwrite(maps->getLocalMap(0)->estimatedGlobalPose.GetM().m, 4, 16, o);
    fwrite(maps->getLocalMap(1)->estimatedGlobalPose.GetM().m, 4, 16, o);
    for (size_t i = 0; i < fused.size(); i++) fwrite(fused[i].m, 4, 16, o);
    fwrite(&rres, sizeof(rres), 1, o);
    fwrite(&aligned, 4, 1, o);
    fwrite(&mres, sizeof(mres), 1, o);
    fwrite(&merged, 4, 1, o);
    fwrite(depth_both.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
    fwrite(depth_merged.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
    const int32_t tops[2] = {st.last_free_block_id, st.last_free_excess_id};
    fwrite(tops, 4, 2, o);
    fwrite(table.data(), sizeof(dslam_hash_entry), table.size(), o);
    fwrite(alloc_list.data(), 4, alloc_list.size(), o);
    fwrite(excess_list.data(), 4, excess_list.size(), o);
    fwrite(voxels.data(), sizeof(dslam_voxel), voxels.size(), o);
    fclose(o);
    printf("merge_harness ok: %d keyframes, registration stop reason %d; merge: %d passes, %d blocks allocated, %d touched, "
           "%lld voxels changed\n", N, rres.stop_reason, mres.passes, mres.blocks_allocated, mres.blocks_touched,
           (long long)mres.voxels_changed);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "merge_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
