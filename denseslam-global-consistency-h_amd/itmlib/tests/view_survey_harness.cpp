// view_survey_harness.cpp -- drives ITMMainEngine::SurveyLocalMapsInView, TrackVisibleLocalMaps and TrackAllLocalMaps through
// the ITMLib mirror: three local maps fused from the same keyframes (map 1's frame is D times map 0's, map 2's F times
// map 0's -- F puts it where the camera cannot reach it: map 2 is fused in map 0's frame and only believed to lie in F
// times that frame -- and their estimatedGlobalPoses say so), then a fourth local map
// that has just been created and holds nothing -- the current one -- whose pose_d is a start pose some way off the last
// frame's true pose.  The frame is tracked twice from that start: TrackAllLocalMaps(current), then, with pose_d put
// back, TrackVisibleLocalMaps(current).
//
//   view_survey_harness <frames.bin> <out.bin>
// frames.bin: as track_sdf_harness.cpp, followed by float F[16] and float near_m, far_m
// out.bin:    float T[4][16] (estimatedGlobalPose.GetM(), column-major); float pose_d_before[16], pose_d_after_all[16],
//             pose_d_after_visible[16] (the current map's); float Mfused[3][N][16]; float W0[16] (the start, world ->
//             camera, as both calls form it); int32 reach[4], nearest[4] (SurveyLocalMapsInView at W0); int32 kept_count,
//             kept[4] (TrackVisibleLocalMaps' list, padded with -1); dslam_track_sdf_result of TrackAllLocalMaps, then of
//             TrackVisibleLocalMaps; int32 their return values; int32 count, kept[4] of GetImageVisibleLocalMaps from W0, then
//             of the same call from a camera 1000 m further back; float depth[3][H][W]: GetImageAllLocalMaps from W0 and the
//             two GetImageVisibleLocalMaps images
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class ViewSurveyHarness : public ITMMainEngine {
 public:
  ViewSurveyHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~ViewSurveyHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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
  Matrix4f D, E, F;
  float range[2];
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4 || fread(D.m, 4, 16, f) != 16 ||
      fread(E.m, 4, 16, f) != 16 || fread(F.m, 4, 16, f) != 16 || fread(range, 4, 2, f) != 2)
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
    ViewSurveyHarness drv(settings, calib, Vector2i(W, H));
    ITMVoxelMapGraphManager *maps = drv.GetMapManager();

    ITMPose anchor;
    anchor.SetM(poses[0]);
    std::vector<Matrix4f> fused(3 * (size_t)N);
    for (int k = 0; k < 3; k++) {
      const int idx = maps->createNewLocalMap();
      ITMLocalMap *m = maps->getLocalMap(idx);
      ITMPose global;
      // (map 2 is fused in map 0's frame and then believed to lie in F times that frame: its content sits where F^-1 takes it)
      global.SetM(k == 1 ? D * anchor.GetM() : anchor.GetM());
      for (int i = 0; i < N; i++) {
        Matrix4f Twc;
        poses[i].inv(Twc);
        m->trackingState->pose_d->SetInvM(global.GetM() * Twc);   // SetPoseLocalMap
        fused[(size_t)k * N + i] = m->trackingState->pose_d->GetM();
        drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
        drv.IntegrateLocalMap(m);
      }
      if (k == 2) global.SetM(F * anchor.GetM());
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
    // the start as both tracking calls form it, and the survey there
    double Md[16], Tc[16], Wd[16];
    for (int i = 0; i < 16; i++) { Md[i] = (double)before.m[i]; Tc[i] = (double)global.GetM().m[i]; }
    ITMMainEngine::RigidProduct(Md, Tc, Wd);
    float W0[16];
    for (int i = 0; i < 16; i++) W0[i] = (float)Wd[i];
    std::vector<int32_t> reach, nearest, kept;
    drv.SurveyLocalMapsInView(W0, intr, Vector2i(W, H), range[0], range[1], reach, nearest);
    dslam_track_sdf_result res_all, res_vis;
    const int32_t tracked_all = drv.TrackAllLocalMaps(current, &res_all) ? 1 : 0;
    const Matrix4f after_all = current->trackingState->pose_d->GetM();
    current->trackingState->pose_d->SetM(before);
    const int32_t tracked_vis = drv.TrackVisibleLocalMaps(current, range[0], range[1], &res_vis, &kept) ? 1 : 0;

    // the free camera at the start: all maps, the maps in view, and -- 1000 m further back -- a camera none of them reaches
    // within the far plane, where map 0 is drawn
    Matrix4f W0m, Wfar;
    for (int i = 0; i < 16; i++) W0m.m[i] = Wfar.m[i] = W0[i];
    Wfar.m[14] += 1000.0f;
    ITMPose cam, cam_far;
    cam.SetM(W0m);
    cam_far.SetM(Wfar);
    ITMFloatImage img_all(Vector2i(W, H), true, true), img_vis(Vector2i(W, H), true, true), img_none(Vector2i(W, H), true, true);
    std::vector<int32_t> kept_img, kept_none;
    drv.GetImageAllLocalMaps(nullptr, &img_all, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &cam, &intrinsics);
    drv.GetImageVisibleLocalMaps(nullptr, &img_vis, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &cam, &intrinsics, range[0], range[1],
                                 &kept_img);
    drv.GetImageVisibleLocalMaps(nullptr, &img_none, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &cam_far, &intrinsics, range[0],
                                 range[1], &kept_none);

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    for (int k = 0; k < 4; k++) fwrite(maps->getLocalMap(k)->estimatedGlobalPose.GetM().m, 4, 16, o);
    fwrite(before.m, 4, 16, o);
    fwrite(after_all.m, 4, 16, o);
    fwrite(current->trackingState->pose_d->GetM().m, 4, 16, o);
    for (size_t i = 0; i < fused.size(); i++) fwrite(fused[i].m, 4, 16, o);
    fwrite(W0, 4, 16, o);
    fwrite(reach.data(), 4, 4, o);
    fwrite(nearest.data(), 4, 4, o);
    const int32_t kept_count = (int32_t)kept.size();
    kept.resize(4, -1);
    fwrite(&kept_count, 4, 1, o);
    fwrite(kept.data(), 4, 4, o);
    fwrite(&res_all, sizeof(res_all), 1, o);
    fwrite(&res_vis, sizeof(res_vis), 1, o);
    fwrite(&tracked_all, 4, 1, o);
    fwrite(&tracked_vis, 4, 1, o);
    const int32_t img_count = (int32_t)kept_img.size(), none_count = (int32_t)kept_none.size();
    kept_img.resize(4, -1);
    kept_none.resize(4, -1);
    fwrite(&img_count, 4, 1, o);
    fwrite(kept_img.data(), 4, 4, o);
    fwrite(&none_count, 4, 1, o);
    fwrite(kept_none.data(), 4, 4, o);
    fwrite(img_all.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
    fwrite(img_vis.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
    fwrite(img_none.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
    fclose(o);
    printf("view_survey_harness ok: %d keyframes, reach %d %d %d %d, %d maps kept, stop reason %d / %d after %d / %d evaluations\n", N,
           reach[0], reach[1], reach[2], reach[3], kept_count, res_all.stop_reason, res_vis.stop_reason, res_all.evaluations,
           res_vis.evaluations);
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "view_survey_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
