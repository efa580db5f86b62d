// ITMMainEngine.h -- the ITMLib engine classes InfiniTamDriver derives from and calls (reference include at
// InfiniTamDriver.h:11), implemented as thin host wrappers over the C ABI of libdslam_fusion.so.
//
//   ITMMainEngine(settings, calib, imgSize_rgb, imgSize_d)            InfiniTamDriver.h:102
//   members view, settings, denseMapper, trackingController, viewBuilder, visualisationEngine, mapManager,
//           mActiveDataManger                                         InfiniTamDriver.h:133-157,189-241,276-308,363
//   GetPrimaryLocalMap(), GetImage(out, outFloat, type, pose, intrinsics, localMap), SaveCurrSceneToMesh
//                                                                      InfiniTamDriver.h:146,169; InfiniTamDriver.cpp:242-275
//
// How calls complete.  The reference's driver treats every ITMLib call as done when it returns, but it only ever LOOKS at
// results in a few places: the image GetImage filled (InfiniTamDriver.cpp:242-250,269-277), the host mirrors view->rgb /
// view->depth (InfiniTamDriver.h:217-218), the counters lastFreeBlockId / noVisibleEntries / GetDecayedBlockCount
// (InfiniTamDriver.h:210,345,368), the tracked pose (:157-161), the mesh file (DenseSlam.cpp:641).  Between UpdateView,
// IntegrateLocalMap, SlideWindow* and Decay (DenseSlam.cpp:210-232) it looks at nothing.  So the mirror runs the engine
// asynchronously (dslam_engine_set_async): ProcessFrame, DeProcessFrame, Decay*, SlideWindow*, ResetScene, Prepare, the
// swapping calls and the visualisation steps ENQUEUE their kernels and return; UpdateView waits only for its own upload
// (which runs on the copy stream under the kernels enqueued before it; the caller may rewrite its images as soon as
// it returns); everything that hands data to the host WAITS: GetImage, a counter read, GetData on a stale host mirror,
// Track (per ICP iteration), MeshScene, CountVisibleBlocks.  What the device can only report late (dslam_fusion.h,
// "conditions only the device can detect") is thrown by the first of those waiting calls.  A caller that observes
// nothing between two waiting calls cannot tell the difference from the synchronous engine: same kernels, same order,
// same stream.  DSLAM_MIRROR_SYNC=1 in the environment gives the synchronous engine back (every call waits), for A/B
// measurements and debugging.
// Header-only; link with -ldslam_fusion.
#pragma once
#include <cstdio>
#include <vector>

#include "../Objects/ITMObjects.h"

namespace ITMLib {
namespace Engine {
using namespace Objects;

/// ITMLib::Engine::WeightParams (SystemEntry.cpp:183-187; InfiniTamDriver.h:101,391)
struct WeightParams {
  bool depthWeighting;
  int maxNewW;
  float maxDistance;
  WeightParams() : depthWeighting(false), maxNewW(1), maxDistance(1.0f) {}
};

/// ITMSwappingEngine<TVoxel,TIndex>: SaveToGlobalMemory(scene) is Hansry's one-argument form (DenseSlam.h:250)
template <class TVoxel, class TIndex> class ITMSwappingEngine {
  dslam_engine *eng_;
 public:
  explicit ITMSwappingEngine(dslam_engine *e) : eng_(e) {}
  void IntegrateGlobalIntoLocal(ITMScene<TVoxel, TIndex> *scene, ITMRenderState *rs) {
    dslam_check(dslam_swap_in(eng_, scene->handle, rs ? rs->handle : nullptr), "dslam_swap_in");
    scene->MarkCountersStale(rs);
  }
  void SaveToGlobalMemory(ITMScene<TVoxel, TIndex> *scene, ITMRenderState *rs) {
    dslam_check(dslam_swap_out(eng_, scene->handle, rs->handle), "dslam_swap_out");
    scene->MarkCountersStale(rs);
  }
  void SaveToGlobalMemory(ITMScene<TVoxel, TIndex> *scene) {
    dslam_check(dslam_save_to_global_memory(eng_, scene->handle), "dslam_save_to_global_memory");
    scene->MarkCountersStale();
  }
};

/// ITMDenseMapper: the fusion entry points (InfiniTamDriver.h:187-199,241,274-310,354-370)
class ITMDenseMapper {
  dslam_engine *eng_;
  const ITMRGBDCalib *calib_;
  ITMSwappingEngine<ITMVoxel, ITMVoxelIndex> *swappingEngine_;
  // the scenes this mapper has worked on (GetDecayedBlockCount sums their device-resident counters when asked; scenes
  // belong to the map manager, which lives as long as the engine that owns this mapper)
  std::vector<const ITMScene<ITMVoxel, ITMVoxelIndex> *> scenes_;
  void note(const ITMScene<ITMVoxel, ITMVoxelIndex> *scene) {
    for (size_t i = 0; i < scenes_.size(); i++) if (scenes_[i] == scene) return;
    scenes_.push_back(scene);
  }

  void poseArgs(const ITMView *view, const ITMTrackingState *ts, Matrix4f &M_d, Matrix4f &M_rgb, Vector4f &kd, Vector4f &kr) const {
    M_d = ts->pose_d->GetM();
    M_rgb = view->calib->trafo_rgb_to_depth.calib_inv * M_d;
    kd = view->calib->intrinsics_d.projectionParamsSimple.all;
    kr = view->calib->intrinsics_rgb.projectionParamsSimple.all;
  }

 public:
  ITMDenseMapper(dslam_engine *e, const ITMRGBDCalib *calib)
      : eng_(e), calib_(calib), swappingEngine_(new ITMSwappingEngine<ITMVoxel, ITMVoxelIndex>(e)) {}
  ~ITMDenseMapper() { delete swappingEngine_; }

  void SetFusionWeightParams(const WeightParams &p) {
    dslam_weight_params w = {p.depthWeighting ? 1 : 0, p.maxNewW, p.maxDistance};
    dslam_check(dslam_set_fusion_weight_params(eng_, &w), "dslam_set_fusion_weight_params");
  }
  void ResetScene(ITMScene<ITMVoxel, ITMVoxelIndex> *scene) {
    dslam_check(dslam_scene_reset(eng_, scene->handle), "dslam_scene_reset");
    scene->MarkCountersStale();
    note(scene);
  }
  void ProcessFrame(const ITMView *view, const ITMTrackingState *ts, ITMScene<ITMVoxel, ITMVoxelIndex> *scene,
                    ITMRenderState *rs, bool onlyUpdateVisibleList = false, bool isDefusion = false) {
    Matrix4f M_d, M_rgb; Vector4f kd, kr;
    poseArgs(view, ts, M_d, M_rgb, kd, kr);
    dslam_check(dslam_process_frame(eng_, scene->handle, view->handle, rs->handle, M_d.m, kd.v, M_rgb.m, kr.v,
                                    onlyUpdateVisibleList, isDefusion), "dslam_process_frame");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  void DeProcessFrame(const ITMView *view, const ITMTrackingState *ts, ITMScene<ITMVoxel, ITMVoxelIndex> *scene,
                      ITMRenderState *rs) {
    Matrix4f M_d, M_rgb; Vector4f kd, kr;
    poseArgs(view, ts, M_d, M_rgb, kd, kr);
    dslam_check(dslam_deprocess_frame(eng_, scene->handle, view->handle, rs->handle, M_d.m, kd.v, M_rgb.m, kr.v),
                "dslam_deprocess_frame");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  /// (extension of this engine, not in upstream) keep the visible list of the fusion that has just run with the keyframe's
  /// images in the device-resident store: what ReProcessFrames de-integrates from (dslam_frame_store_put_visible_list)
  void KeepVisibleList(dslam_frame_store *store, int slot, ITMScene<ITMVoxel, ITMVoxelIndex> *scene, ITMRenderState *rs) {
    dslam_check(dslam_frame_store_put_visible_list(eng_, store, slot, scene->handle, rs->handle), "dslam_frame_store_put_visible_list");
  }
  /// (extension) the re-fusion loop of DenseSlam::OnlineCorrection [REF DenseSlam.cpp:389-403] -- per keyframe DeProcessFrame at
  /// the old pose, ProcessFrame(isDefusion) at the new one -- as ONE call, run block-major on the device (dslam_reintegrate_batch;
  /// one camera).  De-integration visits the blocks of the keyframe's own stored list, not what an allocation pass at the old
  /// pose finds today: not the reference's call sequence.
  void ReProcessFrames(const ITMView *view, ITMScene<ITMVoxel, ITMVoxelIndex> *scene, ITMRenderState *rs, dslam_frame_store *store,
                       int n, const int *slots, const Matrix4f *oldM_d, const Matrix4f *newM_d) {
    const Vector4f kd = view->calib->intrinsics_d.projectionParamsSimple.all;
    const Vector2f ab = calib_->disparityCalib.params;
    static_assert(sizeof(Matrix4f) == 16 * sizeof(float), "poses are handed over as n x 16 floats");
    dslam_check(dslam_reintegrate_batch(eng_, scene->handle, view->handle, rs->handle, store, n, slots, n ? oldM_d[0].m : nullptr,
                                        n ? newM_d[0].m : nullptr, kd.v, ab.x, ab.y), "dslam_reintegrate_batch");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  void Decay(ITMScene<ITMVoxel, ITMVoxelIndex> *scene, ITMRenderState *rs, int maxWeight, int minAge, bool forceAllVoxels) {
    dslam_check(dslam_decay(eng_, scene->handle, rs ? rs->handle : nullptr, maxWeight, minAge, forceAllVoxels), "dslam_decay");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  void DecayDefusionPart(ITMScene<ITMVoxel, ITMVoxelIndex> *scene, ITMRenderState *rs, int maxWeight, int minAge, bool forceAllVoxels) {
    dslam_check(dslam_decay_defusion_part(eng_, scene->handle, rs ? rs->handle : nullptr, maxWeight, minAge, forceAllVoxels),
                "dslam_decay_defusion_part");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  void SlideWindow(ITMScene<ITMVoxel, ITMVoxelIndex> *scene, ITMRenderState *rs, int maxAge) {
    dslam_check(dslam_slide_window(eng_, scene->handle, rs ? rs->handle : nullptr, maxAge), "dslam_slide_window");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  void SlideWindowDefusionPart(ITMScene<ITMVoxel, ITMVoxelIndex> *scene, ITMRenderState *rs, int maxAge, int maxSize) {
    dslam_check(dslam_slide_window_defusion_part(eng_, scene->handle, rs ? rs->handle : nullptr, maxAge, maxSize),
                "dslam_slide_window_defusion_part");
    scene->MarkCountersStale(rs);
    note(scene);
  }
  /// InfiniTamDriver.h:366-370 (the GUI's "saved memory" figure): read from the device when asked, not after every call
  size_t GetDecayedBlockCount() const {
    long long n = 0;
    for (size_t i = 0; i < scenes_.size(); i++) n += scenes_[i]->Counters().decayed_block_count;
    return (size_t)n;
  }
  ITMSwappingEngine<ITMVoxel, ITMVoxelIndex> *GetSwappingEngine() { return swappingEngine_; }
};

/// ITMViewBuilder::UpdateView(&view, rgb, rawDepth, timestamp, useBilateralFilter) (InfiniTamDriver.cpp:286)
class ITMViewBuilder {
  dslam_engine *eng_;
  const ITMRGBDCalib *calib_;
 public:
  ITMViewBuilder(dslam_engine *e, const ITMRGBDCalib *c) : eng_(e), calib_(c) {}
  const ITMRGBDCalib *GetCalib() const { return calib_; }  ///< InfiniTamDriver.cpp:241
  void UpdateView(ITMView **view, ITMUChar4Image *rgb, ITMShortImage *rawDepth, double timestamp, bool useBilateralFilter) {
    if (*view == nullptr) *view = new ITMView(calib_, rgb->noDims, rawDepth->noDims, eng_);
    ITMView *v = *view;
    const Vector2f ab = calib_->disparityCalib.params;
    dslam_check(dslam_view_update(eng_, v->handle, &rgb->GetData(MEMORYDEVICE_CPU)->x, rawDepth->GetData(MEMORYDEVICE_CPU),
                                  ab.x, ab.y, timestamp, useBilateralFilter), "dslam_view_update");
    v->timestamp = timestamp;
    // host mirrors: view->rgb / view->depth are read back by the driver (InfiniTamDriver.h:217-218) -- on demand
    v->MarkHostStale();
  }
  /// UpdateView for a keyframe that already sits in the device-resident keyframe store (the UpdateView calls of
  /// DenseSlam::OnlineCorrection, DenseSlam.cpp:392,421): no upload; the host mirrors view->rgb / view->depth are
  /// refreshed only if somebody reads them (nothing on that path does).
  void UpdateViewFromStore(ITMView **view, const dslam_frame_store *store, int slot, double timestamp, bool useBilateralFilter) {
    if (*view == nullptr) throw std::runtime_error("UpdateViewFromStore: the view must have been created by UpdateView first");
    const Vector2f ab = calib_->disparityCalib.params;
    dslam_check(dslam_view_update_from_store(eng_, (*view)->handle, store, slot, ab.x, ab.y, timestamp, useBilateralFilter),
                "dslam_view_update_from_store");
    (*view)->timestamp = timestamp;
    (*view)->MarkHostStale();
  }
};

/// ITMTrackingController: Prepare = raycast into ICP maps (InfiniTamDriver.h:212-215); Track = ITMDepthTracker's
/// point-to-plane ICP of the view against those maps (InfiniTamDriver.h:151-163), both on the device.
class ITMTrackingController {
  dslam_engine *eng_;
  dslam_tracker_params params_;
 public:
  explicit ITMTrackingController(dslam_engine *e, const ITMLibSettings *settings = nullptr) : eng_(e) {
    ITMLibSettings defaults;
    if (settings == nullptr) settings = &defaults;
    params_.no_hierarchy_levels = settings->noHierarchyLevels;
    params_.no_icp_run_till_level = settings->noICPRunTillLevel;
    params_.dist_thresh = settings->depthTrackerICPThreshold;
    params_.termination_threshold = settings->depthTrackerTerminationThreshold;
    for (int i = 0; i < DSLAM_TRACKER_MAX_LEVELS; i++) params_.regime[i] = (int)settings->trackingRegime[i];
  }
  void Prepare(ITMTrackingState *ts, const ITMScene<ITMVoxel, ITMVoxelIndex> *scene, const ITMView *view, ITMRenderState *rs) {
    const Matrix4f M = ts->pose_d->GetM();
    const Vector4f k = view->calib->intrinsics_d.projectionParamsSimple.all;
    // the maps stay on the device (Track reads them there); trackingState->pointsMap / normalsMap are host mirrors
    // filled when somebody asks for them
    dslam_check(dslam_create_icp_maps(eng_, scene->handle, rs->handle, M.m, k.v, nullptr, nullptr), "dslam_create_icp_maps");
    dslam_engine *eng = eng_;
    dslam_render_state *h = rs->handle;
    ts->pointsMap->SetHostPull([eng, h](Vector4f *dst) { dslam_check(dslam_download_icp_maps(eng, h, &dst->x, nullptr), "dslam_download_icp_maps"); });
    ts->normalsMap->SetHostPull([eng, h](Vector4f *dst) { dslam_check(dslam_download_icp_maps(eng, h, nullptr, &dst->x), "dslam_download_icp_maps"); });
    ts->pointsMap->MarkHostStale();
    ts->normalsMap->MarkHostStale();
    // renderState->raycastImage: the grey rendering CreateICPMaps draws next to the maps (InfiniTAM_IMAGE_SCENERAYCAST)
    rs->raycastImage->SetHostPull([eng, h](Vector4u *dst) { dslam_check(dslam_download_raycast_image(eng, h, &dst->x), "dslam_download_raycast_image"); });
    rs->raycastImage->MarkHostStale();
    ts->pose_pointCloud->SetM(M);
    ts->preparedWith = rs;
    ts->age_pointCloud = 0;
  }
  void Track(ITMTrackingState *ts, const ITMView *view) {
    if (ts->preparedWith == nullptr) throw std::runtime_error("ITMTrackingController::Track: Prepare has not been called");
    const Vector4f k = view->calib->intrinsics_d.projectionParamsSimple.all;
    Matrix4f M = ts->pose_d->GetM();
    dslam_tracker_result res;
    dslam_check(dslam_track_camera(eng_, view->handle, ts->preparedWith->handle, ts->pose_pointCloud->GetM().m, M.m, k.v,
                                   &params_, &res), "dslam_track_camera");
    ts->pose_d->SetM(M);
    ts->age_pointCloud++;
  }
};

/// ITMVisualisationEngine (InfiniTamDriver.h:362-364)
template <class TVoxel, class TIndex> class ITMVisualisationEngine {
  dslam_engine *eng_;
 public:
  explicit ITMVisualisationEngine(dslam_engine *e) : eng_(e) {}
  ITMRenderState *CreateRenderState(const ITMScene<TVoxel, TIndex> *scene, Vector2i sz) const { return new ITMRenderState_VH(eng_, scene->handle, sz); }
  void FindVisibleBlocks(const ITMScene<TVoxel, TIndex> *scene, const ITMPose *pose, const ITMIntrinsics *intr, ITMRenderState *rs) const {
    dslam_check(dslam_find_visible_blocks(eng_, scene->handle, rs->handle, pose->GetM().m, intr->projectionParamsSimple.all.v), "dslam_find_visible_blocks");
    rs->MarkCountersStale();
  }
  int CountVisibleBlocks(const ITMScene<TVoxel, TIndex> *scene, const ITMRenderState *rs, int minBlockId, int maxBlockId) const {
    int n = 0;
    dslam_check(dslam_count_visible_blocks(eng_, scene->handle, rs->handle, minBlockId, maxBlockId, &n), "dslam_count_visible_blocks");
    return n;
  }
  void CreateExpectedDepths(const ITMScene<TVoxel, TIndex> *scene, const ITMPose *pose, const ITMIntrinsics *intr, ITMRenderState *rs) const {
    dslam_check(dslam_create_expected_depths(eng_, scene->handle, rs->handle, pose->GetM().m, intr->projectionParamsSimple.all.v), "dslam_create_expected_depths");
  }
};

/// ITMVoxelMapGraphManager (DenseSlam.cpp:135-152,555-556; InfiniTamDriver.h:136,269): host container of local maps
class ITMVoxelMapGraphManager {
  const ITMLibSettings *settings_;
  dslam_engine *eng_;
  Vector2i trackedImageSize_;
  const ITMVisualisationEngine<ITMVoxel, ITMVoxelIndex> *vis_;
  std::vector<ITMLocalMap *> maps_;
 public:
  ITMVoxelMapGraphManager(const ITMLibSettings *s, dslam_engine *e, const ITMVisualisationEngine<ITMVoxel, ITMVoxelIndex> *vis, Vector2i sz)
      : settings_(s), eng_(e), trackedImageSize_(sz), vis_(vis) {}
  ~ITMVoxelMapGraphManager() { for (auto *m : maps_) delete m; }
  int createNewLocalMap() { maps_.push_back(new ITMLocalMap(settings_, eng_, trackedImageSize_)); return (int)maps_.size() - 1; }
  int numLocalMaps() const { return (int)maps_.size(); }
  ITMLocalMap *getLocalMap(int i) const { return (i < 0 || i >= (int)maps_.size()) ? nullptr : maps_[i]; }
  void setEstimatedGlobalPose(int i, const ITMPose &pose) { maps_[i]->estimatedGlobalPose = pose; }
  int getLocalMapSize(int i) const {
    dslam_stats st;
    dslam_check(dslam_get_stats(eng_, maps_[i]->scene->handle, nullptr, &st), "dslam_get_stats");
    return st.num_allocated_blocks - st.last_free_block_id - 1;
  }
  int countVisibleBlocks(int i, int minBlockId, int maxBlockId, bool /*invertIDs*/) const {
    return vis_->CountVisibleBlocks(maps_[i]->scene, maps_[i]->renderState, minBlockId, maxBlockId);
  }
};

/// ITMActiveMapManager: only numActiveLocalMaps() is reached (InfiniTamDriver.h:264)
class ITMActiveMapManager {
  ITMVoxelMapGraphManager *maps_;
 public:
  explicit ITMActiveMapManager(ITMVoxelMapGraphManager *m) : maps_(m) {}
  int numActiveLocalMaps() const { return maps_->numLocalMaps() > 0 ? 1 : 0; }
};

class ITMMainEngine {
 public:
  enum GetImageType {
    InfiniTAM_IMAGE_ORIGINAL_RGB,
    InfiniTAM_IMAGE_ORIGINAL_DEPTH,
    InfiniTAM_IMAGE_SCENERAYCAST,
    InfiniTAM_IMAGE_FREECAMERA_SHADED,
    InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME,
    InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL,
    InfiniTAM_IMAGE_FREECAMERA_DEPTH,
    InfiniTAM_IMAGE_UNKNOWN
  };

  ITMMainEngine(const ITMLibSettings *settings_, const ITMRGBDCalib *calib, Vector2i imgSize_rgb, Vector2i imgSize_d = Vector2i(-1, -1))
      : settings(settings_), view(nullptr), engine_(nullptr), freeviewScene_(nullptr), renderState_freeview_(nullptr),
        renderState_allmaps_(nullptr), allmapsBlocks_(0), allmapsScene_(nullptr) {
    if (imgSize_d.x == -1 || imgSize_d.y == -1) imgSize_d = imgSize_rgb;
    dslam_check(dslam_engine_create(settings->hipDeviceIndex, &engine_), "dslam_engine_create");
    // calls enqueue; the calls that hand data to the host wait (see the head of this file)
    const char *sync_env = getenv("DSLAM_MIRROR_SYNC");
    deferred_ = !(sync_env && atoi(sync_env) != 0);
    dslam_check(dslam_engine_set_async(engine_, deferred_ ? 1 : 0), "dslam_engine_set_async");
    denseMapper = new ITMDenseMapper(engine_, calib);
    viewBuilder = new ITMViewBuilder(engine_, calib);
    trackingController = new ITMTrackingController(engine_, settings);
    visualisationEngine = new ITMVisualisationEngine<ITMVoxel, ITMVoxelIndex>(engine_);
    mapManager = new ITMVoxelMapGraphManager(settings, engine_, visualisationEngine, imgSize_d);
    mActiveDataManger = new ITMActiveMapManager(mapManager);
  }
  virtual ~ITMMainEngine() {
    delete renderState_freeview_;
    delete renderState_allmaps_;
    delete mActiveDataManger; delete mapManager; delete visualisationEngine; delete trackingController;
    delete viewBuilder; delete denseMapper; delete view;
    dslam_engine_destroy(engine_);
  }

  ITMLocalMap *GetPrimaryLocalMap() const { return mapManager->getLocalMap(0); }

  /// FREECAMERA_* render the given local map (primary when null; nothing before the first keyframe, B.1);
  /// SCENERAYCAST copies renderState->raycastImage, the grey tracking raycast trackingController->Prepare draws
  /// (zero until the first Prepare, as upstream); ORIGINAL_* copy the view.
  void GetImage(ITMUChar4Image *out, ITMFloatImage *outFloat, GetImageType type, ITMPose *pose = nullptr,
                ITMIntrinsics *intrinsics = nullptr, const ITMLocalMap *localMap = nullptr) {
    if (view == nullptr) return;
    if (localMap == nullptr) localMap = GetPrimaryLocalMap();
    switch (type) {
      case InfiniTAM_IMAGE_ORIGINAL_RGB:
        if (out) { out->ChangeDims(view->rgb->noDims); memcpy(out->GetData(MEMORYDEVICE_CPU), view->rgb->GetData(MEMORYDEVICE_CPU), out->dataSize * 4); }
        return;
      case InfiniTAM_IMAGE_ORIGINAL_DEPTH:
        if (outFloat) { outFloat->ChangeDims(view->depth->noDims); memcpy(outFloat->GetData(MEMORYDEVICE_CPU), view->depth->GetData(MEMORYDEVICE_CPU), outFloat->dataSize * 4); }
        return;
      case InfiniTAM_IMAGE_SCENERAYCAST:
        if (out && localMap && localMap->renderState->raycastImage) {
          out->ChangeDims(localMap->renderState->raycastImage->noDims);
          memcpy(out->GetData(MEMORYDEVICE_CPU), localMap->renderState->raycastImage->GetData(MEMORYDEVICE_CPU), out->dataSize * 4);
        }
        return;
      default: break;
    }
    if (localMap == nullptr || pose == nullptr || intrinsics == nullptr) return;
    int t;
    switch (type) {
      case InfiniTAM_IMAGE_FREECAMERA_SHADED: t = DSLAM_IMAGE_SHADED; break;
      case InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME: t = DSLAM_IMAGE_COLOUR_FROM_VOLUME; break;
      case InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL: t = DSLAM_IMAGE_COLOUR_FROM_NORMAL; break;
      case InfiniTAM_IMAGE_FREECAMERA_DEPTH: t = DSLAM_IMAGE_DEPTH; break;
      default: return;
    }
    const Vector2i sz = (t == DSLAM_IMAGE_DEPTH) ? (outFloat ? outFloat->noDims : Vector2i(0, 0)) : (out ? out->noDims : Vector2i(0, 0));
    if (sz.x <= 0) return;
    if (renderState_freeview_ == nullptr || freeviewScene_ != localMap->scene || freeviewSize_.x != sz.x || freeviewSize_.y != sz.y) {
      delete renderState_freeview_;
      renderState_freeview_ = visualisationEngine->CreateRenderState(localMap->scene, sz);
      freeviewScene_ = localMap->scene; freeviewSize_ = sz;
    }
    dslam_check(dslam_get_image(engine_, localMap->scene->handle, renderState_freeview_->handle, pose->GetM().m,
                                intrinsics->projectionParamsSimple.all.v, t,
                                t == DSLAM_IMAGE_DEPTH ? nullptr : &out->GetData(MEMORYDEVICE_CPU)->x,
                                t == DSLAM_IMAGE_DEPTH ? outFloat->GetData(MEMORYDEVICE_CPU) : nullptr), "dslam_get_image");
    // the caller reads the image next (ItmToCv / ItmDepthToCv, InfiniTamDriver.cpp:249,276): a page-locked image is filled
    // by the render kernel itself, so this is where the mirror waits for the stream -- and hears what the device reported
    if (deferred_) dslam_check(dslam_engine_synchronize(engine_), "dslam_engine_synchronize");
  }

  /// (extension) The whole reconstruction in one image: every local map of mapManager drawn through its
  /// estimatedGlobalPose.GetM() (Tdw, DenseSlam.cpp:190,577-579) from `pose` in the global frame -- the reference's
  /// previews draw currentLocalMap only (DenseSlam.h:146-164).  FREECAMERA_* types as GetImage; other types and a call
  /// before the first local map do nothing.  dslam_get_image_multi, combination law in DESIGN.md section 10.
  void GetImageAllLocalMaps(ITMUChar4Image *out, ITMFloatImage *outFloat, GetImageType type, ITMPose *pose,
                            ITMIntrinsics *intrinsics) {
    const int n = mapManager->numLocalMaps();
    if (n == 0 || pose == nullptr || intrinsics == nullptr) return;
    if (n > DSLAM_MAX_RENDER_MAPS)
      throw std::runtime_error("GetImageAllLocalMaps: " + std::to_string(n) + " local maps, at most " +
                               std::to_string(DSLAM_MAX_RENDER_MAPS) + " can be drawn in one image");
    int t;
    Vector2i sz;
    if (!FreeCameraImage(type, out, outFloat, t, sz)) return;
    std::vector<const dslam_scene *> scenes;
    std::vector<float> T;
    ListLocalMaps(scenes, T);
    DrawLocalMaps(scenes, T, t, sz, out, outFloat, pose, intrinsics);
  }

  /// SaveCurrSceneToMesh(objFileName, scene) (DenseSlam.cpp:641): meshingEngine->MeshScene(mesh, scene), then
  /// mesh->WriteOBJ(objFileName).  The marching cubes run on the device; the triangle list comes back in the order
  /// of upstream's CPU engine, so the file is the same from run to run.
  void SaveCurrSceneToMesh(const char *objFileName, const ITMScene<ITMVoxel, ITMVoxelIndex> *scene) {
    ITMMesh mesh((unsigned)settings->numLocalBlocks * 32u);
    MeshScene(&mesh, scene);
    mesh.WriteOBJ(objFileName);
  }

  /// (extension) Align local map `src` to local map `dst` from their voxels alone (dslam_register_maps, law in DESIGN.md
  /// section 13): the start is X = T_dst T_src^-1 from the two estimatedGlobalPoses; when the registration converges
  /// (stop reason 0) the source's estimatedGlobalPose becomes X^-1 T_dst and the call returns true, otherwise the pose is
  /// left alone.  Both compositions are made in double by RigidInverse / RigidProduct below, so a caller of the C ABI can
  /// reproduce them bit for bit.  Call it before GetImageAllLocalMaps / SaveAllLocalMapsToMesh, whose blend needs the
  /// maps' relative poses right to a fraction of a voxel.
  bool AlignLocalMap(int src, int dst, dslam_register_result *out = nullptr) {
    ITMLocalMap *ms = mapManager->getLocalMap(src);
    const ITMLocalMap *md = mapManager->getLocalMap(dst);
    double Ts[16], Td[16], inv[16], X[16];
    for (int i = 0; i < 16; i++) { Ts[i] = (double)ms->estimatedGlobalPose.GetM().m[i]; Td[i] = (double)md->estimatedGlobalPose.GetM().m[i]; }
    RigidInverse(Ts, inv);
    RigidProduct(Td, inv, X);
    float Xf[16];
    for (int i = 0; i < 16; i++) Xf[i] = (float)X[i];
    dslam_register_result res;
    dslam_check(dslam_register_maps(engine_, ms->scene->handle, md->scene->handle, Xf, nullptr, &res), "dslam_register_maps");
    if (out) *out = res;
    if (res.stop_reason != 0) return false;
    for (int i = 0; i < 16; i++) X[i] = (double)Xf[i];
    RigidInverse(X, inv);
    RigidProduct(inv, Td, X);
    Matrix4f M;
    for (int i = 0; i < 16; i++) M.m[i] = (float)X[i];
    ms->estimatedGlobalPose.SetM(M);
    return true;
  }
  /// (extension) Align all local maps jointly from their voxels (dslam_register_graph, law in DESIGN.md section 15): `pairs`
  /// lists the overlapping maps as (src, dst) indices, `anchor` is the map whose pose is held.  The starts are the maps'
  /// estimatedGlobalPoses; when the registration converges (stop reason 0) every other map's estimatedGlobalPose is set to
  /// its estimate and the call returns true, otherwise all poses are left alone, as AlignLocalMap leaves its one.  One
  /// kernel launch per evaluation however many pairs, and every overlap constrains the result -- where a chain of
  /// AlignLocalMap calls would add up its errors.  pair_out: one entry per pair.
  bool AlignLocalMaps(const int (*pairs)[2], int num_pairs, int anchor, dslam_register_graph_result *out = nullptr,
                      dslam_register_pair_result *pair_out = nullptr) {
    const int n = mapManager->numLocalMaps();
    std::vector<const dslam_scene *> scenes(n);
    std::vector<float> T((size_t)n * 16);
    for (int i = 0; i < n; i++) {
      const ITMLocalMap *m = mapManager->getLocalMap(i);
      scenes[i] = m->scene->handle;
      memcpy(&T[(size_t)i * 16], m->estimatedGlobalPose.GetM().m, 16 * sizeof(float));
    }
    std::vector<int32_t> flat((size_t)(num_pairs > 0 ? num_pairs : 0) * 2);
    for (size_t i = 0; i < flat.size(); i++) flat[i] = pairs[i / 2][i % 2];
    dslam_register_graph_result res;
    dslam_check(dslam_register_graph(engine_, scenes.data(), T.data(), n, flat.data(), num_pairs, anchor, nullptr, &res, pair_out),
                "dslam_register_graph");
    if (out) *out = res;
    if (res.stop_reason != 0) return false;
    for (int i = 0; i < n; i++) {
      if (i == anchor) continue;
      Matrix4f M;
      memcpy(M.m, &T[(size_t)i * 16], 16 * sizeof(float));
      mapManager->getLocalMap(i)->estimatedGlobalPose.SetM(M);
    }
    return true;
  }
  /// (extension) Which local maps overlap (dslam_survey_overlaps, law in DESIGN.md section 16): under the maps'
  /// estimatedGlobalPoses, `live[i]` becomes map i's resident blocks and `sharedOctants[s * n + d]` the octants of map
  /// s's blocks that fall into a resident block of map d (n = numLocalMaps(); the diagonal is 8 live[s]).  Only the hash
  /// tables are read.
  void SurveyLocalMapOverlaps(std::vector<int32_t> &live, std::vector<int32_t> &sharedOctants) {
    const int n = mapManager->numLocalMaps();
    std::vector<const dslam_scene *> scenes(n);
    std::vector<float> T((size_t)n * 16);
    for (int i = 0; i < n; i++) {
      const ITMLocalMap *m = mapManager->getLocalMap(i);
      scenes[i] = m->scene->handle;
      memcpy(&T[(size_t)i * 16], m->estimatedGlobalPose.GetM().m, 16 * sizeof(float));
    }
    std::vector<int32_t> l((size_t)n), o((size_t)n * n);
    dslam_check(dslam_survey_overlaps(engine_, scenes.data(), T.data(), n, l.data(), nullptr, o.data()), "dslam_survey_overlaps");
    live.swap(l);
    sharedOctants.swap(o);
  }
  /// (extension) AlignLocalMaps without a pair list from the caller: the overlaps are surveyed under the maps'
  /// estimatedGlobalPoses (SurveyLocalMapOverlaps), the pairs selected by dslam_select_register_pairs with its defaults
  /// (both directions of a pair), and AlignLocalMaps runs on them.  When the qualifying pairs do not join all maps
  /// (num_components > 1) no registration is attempted: the call returns false and every pose is left alone.
  /// pairs_out (optional): the selected pairs as (src, dst), by (src, dst) ascending.
  bool AlignAllLocalMaps(int anchor, dslam_register_graph_result *out = nullptr, std::vector<int32_t> *pairs_out = nullptr,
                         std::vector<dslam_register_pair_result> *pair_out = nullptr) {
    const int n = mapManager->numLocalMaps();
    std::vector<int32_t> live, shared, component((size_t)(n > 0 ? n : 1)), pairs((size_t)DSLAM_MAX_REGISTER_PAIRS * 2);
    SurveyLocalMapOverlaps(live, shared);
    dslam_pair_select_result sel;
    dslam_check(dslam_select_register_pairs(live.data(), shared.data(), n, nullptr, pairs.data(), component.data(), &sel),
                "dslam_select_register_pairs");
    pairs.resize((size_t)sel.selected * 2);
    if (pairs_out) *pairs_out = pairs;
    if (pair_out) pair_out->assign((size_t)sel.selected, dslam_register_pair_result());
    if (sel.num_components > 1) return false;
    return AlignLocalMaps(reinterpret_cast<const int (*)[2]>(pairs.data()), sel.selected, anchor, out,
                          pair_out ? pair_out->data() : nullptr);
  }
  /// (extension) Fuse local map `src` into local map `dst` on the device (dslam_merge_maps, law in DESIGN.md section 14)
  /// under X = T_dst T_src^-1 from the two estimatedGlobalPoses, composed as AlignLocalMap composes it -- call that first.
  /// `src` is only read and stays in the graph: dropping it is the caller's decision.  Returns false when the pools of
  /// `dst` ran dry (what could be allocated is fused all the same).
  bool MergeLocalMap(int src, int dst, dslam_merge_result *out = nullptr) {
    const ITMLocalMap *ms = mapManager->getLocalMap(src);
    ITMLocalMap *md = mapManager->getLocalMap(dst);
    double Ts[16], Td[16], inv[16], X[16];
    for (int i = 0; i < 16; i++) { Ts[i] = (double)ms->estimatedGlobalPose.GetM().m[i]; Td[i] = (double)md->estimatedGlobalPose.GetM().m[i]; }
    RigidInverse(Ts, inv);
    RigidProduct(Td, inv, X);
    float Xf[16];
    for (int i = 0; i < 16; i++) Xf[i] = (float)X[i];
    dslam_merge_result res;
    dslam_check(dslam_merge_maps(engine_, ms->scene->handle, md->scene->handle, Xf, nullptr, &res), "dslam_merge_maps");
    if (out) *out = res;
    return res.exhausted == 0;
  }
  /// (extension) X = T_dst T_src^-1 from the two estimatedGlobalPoses, composed exactly as MergeLocalMap composes it
  /// (double, RigidInverse / RigidProduct, rounded to float32): what a caller records when it merges, in order to undo the
  /// merge later -- the poses may have moved by then.
  void LocalMapTransform(int src, int dst, float X[16]) {
    const ITMLocalMap *ms = mapManager->getLocalMap(src);
    const ITMLocalMap *md = mapManager->getLocalMap(dst);
    double Ts[16], Td[16], inv[16], Xd[16];
    for (int i = 0; i < 16; i++) { Ts[i] = (double)ms->estimatedGlobalPose.GetM().m[i]; Td[i] = (double)md->estimatedGlobalPose.GetM().m[i]; }
    RigidInverse(Ts, inv);
    RigidProduct(Td, inv, Xd);
    for (int i = 0; i < 16; i++) X[i] = (float)Xd[i];
  }
  /// (extension) Take local map `src` out of local map `dst` again (dslam_unmerge_maps, law in DESIGN.md section 17):
  /// X_merged is the transform the merge was made under (LocalMapTransform at that time).  Exact only while nothing
  /// clamped at max_w during the merge and neither map has changed since.  Returns false when a voxel of `dst` held less
  /// than was to be taken out of it (such voxels are left alone).
  bool UnmergeLocalMap(int src, int dst, const float X_merged[16], dslam_unmerge_result *out = nullptr) {
    const ITMLocalMap *ms = mapManager->getLocalMap(src);
    ITMLocalMap *md = mapManager->getLocalMap(dst);
    dslam_unmerge_result res;
    dslam_check(dslam_unmerge_maps(engine_, ms->scene->handle, md->scene->handle, X_merged, nullptr, &res), "dslam_unmerge_maps");
    if (out) *out = res;
    return res.depth_underweight == 0 && res.colour_underweight == 0;
  }
  /// (extension) Correct a merge after the poses have moved (dslam_remerge_maps): `src` is taken out of `dst` under
  /// X_merged and merged again under X = T_dst T_src^-1 from the current estimatedGlobalPoses.  Nothing happens when the
  /// two are bit-identical.  Returns MergeLocalMap's verdict.
  bool RemergeLocalMap(int src, int dst, const float X_merged[16], dslam_unmerge_result *un = nullptr,
                       dslam_merge_result *re = nullptr) {
    const ITMLocalMap *ms = mapManager->getLocalMap(src);
    ITMLocalMap *md = mapManager->getLocalMap(dst);
    float X_new[16];
    LocalMapTransform(src, dst, X_new);
    dslam_unmerge_result ures;
    dslam_merge_result mres;
    dslam_check(dslam_remerge_maps(engine_, ms->scene->handle, md->scene->handle, X_merged, X_new, nullptr, &ures, &mres),
                "dslam_remerge_maps");
    if (un) *un = ures;
    if (re) *re = mres;
    return mres.exhausted == 0;
  }
  /// (extension) Shrink a finished local map's voxel pool to what the map holds plus `headroomBlocks` (dslam_pack_scene,
  /// dslam_unpack_scene; law in DESIGN.md section 21): the map is packed into device memory, its scene is replaced by
  /// one of n + headroomBlocks blocks with the same table geometry, and the image is unpacked into it.  Entries keep
  /// their hash indices, the free excess stack its order; blocks move to new slots.  The map's render state is sized by
  /// the old pool and is made anew (its visible list starts empty, as a new map's); the free-view and all-maps render
  /// states go if they were made from the old scene and are made again by the next image (DrawLocalMaps sizes the
  /// all-maps one by the largest pool among the maps it draws, so maps of different pools draw together).  Tracking
  /// state and estimatedGlobalPose stay.  Not for maps that use swapping.  Everything new -- image, scene, render state --
  /// is complete before anything old is let go: on failure the map is left as it was and the call throws.
  void CompactLocalMap(int mapIdx, int headroomBlocks, dslam_pack_info *out = nullptr) {
    ITMLocalMap *m = mapManager->getLocalMap(mapIdx);
    if (headroomBlocks < 0) throw std::runtime_error("CompactLocalMap: negative headroom");
    dslam_pack_info info;
    dslam_check(dslam_pack_scene(engine_, m->scene->handle, nullptr, 0, &info), "dslam_pack_scene (size query)");
    void *buf = nullptr;
    dslam_check(dslam_device_alloc(engine_, (size_t)info.total_bytes, &buf), "dslam_device_alloc");
    ITMScene<ITMVoxel, ITMVoxelIndex> *compact = nullptr;
    ITMRenderState *renderState = nullptr;
    try {
      dslam_check(dslam_pack_scene(engine_, m->scene->handle, buf, info.total_bytes, &info), "dslam_pack_scene");
      const long long blocks = std::max(1LL, (long long)info.blocks + headroomBlocks);
      if (blocks > 0x7fffffffLL) throw std::runtime_error("CompactLocalMap: headroom too large");
      compact = new ITMScene<ITMVoxel, ITMVoxelIndex>(settings, engine_, (int)blocks);
      dslam_check(dslam_unpack_scene(engine_, compact->handle, buf, info.total_bytes, nullptr), "dslam_unpack_scene");
      renderState = new ITMRenderState_VH(engine_, compact->handle, m->renderState->raycastImage->noDims);
      void *image = buf;
      buf = nullptr;
      dslam_check(dslam_device_free(engine_, image), "dslam_device_free");
    } catch (...) {
      delete renderState;
      delete compact;
      if (buf) dslam_device_free(engine_, buf);
      throw;
    }
    // nothing below throws: the old objects go, the new ones take their place
    if (freeviewScene_ == m->scene) { delete renderState_freeview_; renderState_freeview_ = nullptr; freeviewScene_ = nullptr; }
    if (allmapsScene_ == m->scene->handle) { delete renderState_allmaps_; renderState_allmaps_ = nullptr; allmapsScene_ = nullptr; }
    delete m->renderState;
    delete m->scene;
    m->scene = compact;
    m->renderState = renderState;
    if (out) *out = info;
  }
  /// (extension) Track the camera of the current view against ALL local maps under their estimatedGlobalPoses
  /// (dslam_track_camera_sdf, law in DESIGN.md section 18) -- where the reference's internal odometry prepares and tracks
  /// currentLocalMap alone (DenseSlam.cpp:198-206), which holds nothing just after createNewLocalMap.  The start is
  /// world -> camera = pose_d->GetM() T_current from `current`'s tracking state and estimatedGlobalPose; when a step was
  /// accepted pose_d is written back in the current map's frame, pose_d = (world -> camera) T_current^-1, and the call
  /// returns true, otherwise pose_d is left alone.  Both compositions are made in double by RigidProduct / RigidInverse,
  /// so a caller of the C ABI can reproduce them bit for bit.  No Prepare, no render state: call it in place of
  /// Prepare + Track, after AlignLocalMaps has made the neighbours' poses good.
  bool TrackAllLocalMaps(ITMLocalMap *current, dslam_track_sdf_result *out = nullptr) {
    if (view == nullptr) throw std::runtime_error("TrackAllLocalMaps: no view yet (call UpdateView first)");
    std::vector<const dslam_scene *> scenes;
    std::vector<float> T;
    ListLocalMaps(scenes, T);
    float Wf[16];
    WorldPoseOf(current, Wf);
    return TrackListedMaps(current, scenes, T, Wf, out);
  }
  /// (extension) Find the camera again from a pose that may be farther off than the truncation band -- after a tracking
  /// loss, at a loop closure, against maps AlignLocalMaps has just moved -- where TrackAllLocalMaps finds no valid pixel
  /// (DESIGN.md section 24).  The start is TrackAllLocalMaps' world -> camera pose of `current`.  In this order:
  /// dslam_camera_pose_lattice builds `lattice` around it (world axes); dslam_score_camera_poses evaluates every node on
  /// pyramid level scoreLevel in one launch; dslam_select_start_poses keeps the `keep` cheapest nodes with at least the
  /// default parameters' min_valid (500) valid pixels; dslam_track_camera_sdf_starts tracks them in lock-step with the
  /// default parameters.  The winner is the start with the lowest cost_last among those that end with valid_last >= 500
  /// and a stop reason other than 3, ties to the lower index; pose_d = (its world -> camera) T_current^-1 is written back as
  /// TrackAllLocalMaps writes it, `out` receives its result and the call returns true.  Without a winner pose_d is left
  /// alone, `out` is zeroed and the call returns false.  Throws on a lattice of more than DSLAM_MAX_TRACK_STARTS nodes.
  bool RelocaliseAllLocalMaps(ITMLocalMap *current, const dslam_pose_lattice &lattice, int scoreLevel, int keep,
                              dslam_track_sdf_result *out = nullptr) {
    if (view == nullptr) throw std::runtime_error("RelocaliseAllLocalMaps: no view yet (call UpdateView first)");
    if (keep < 1 || keep > DSLAM_MAX_TRACK_STARTS) throw std::runtime_error("RelocaliseAllLocalMaps: keep must be 1 .. DSLAM_MAX_TRACK_STARTS");
    std::vector<const dslam_scene *> scenes;
    std::vector<float> T;
    ListLocalMaps(scenes, T);
    float Wf[16];
    WorldPoseOf(current, Wf);
    const int minValid = 500;   // dslam_track_sdf_params' default
    const Vector4f k = view->calib->intrinsics_d.projectionParamsSimple.all;
    std::vector<float> nodes((size_t)DSLAM_MAX_TRACK_STARTS * 16);
    int32_t count = 0;
    if (dslam_camera_pose_lattice(Wf, &lattice, nodes.data(), DSLAM_MAX_TRACK_STARTS, &count) != DSLAM_OK) {
      if (count > DSLAM_MAX_TRACK_STARTS) throw std::runtime_error("RelocaliseAllLocalMaps: the lattice has more than DSLAM_MAX_TRACK_STARTS nodes");
      dslam_check(DSLAM_ERR_INVALID, "dslam_camera_pose_lattice");
    }
    std::vector<dslam_pose_score> scores((size_t)count);
    dslam_check(dslam_score_camera_poses(engine_, view->handle, scenes.data(), T.data(), (int)scenes.size(), nodes.data(), count, k.v,
                                         scoreLevel, 0.0f, scores.data()), "dslam_score_camera_poses");
    std::vector<int32_t> kept((size_t)keep);
    int32_t numKept = 0;
    dslam_check(dslam_select_start_poses(scores.data(), count, minValid, keep, kept.data(), &numKept), "dslam_select_start_poses");
    if (out) memset(out, 0, sizeof *out);
    if (numKept == 0) return false;
    std::vector<float> starts((size_t)numKept * 16);
    for (int s = 0; s < numKept; s++) memcpy(&starts[(size_t)s * 16], &nodes[(size_t)kept[(size_t)s] * 16], 16 * sizeof(float));
    std::vector<dslam_track_sdf_result> results((size_t)numKept);
    dslam_check(dslam_track_camera_sdf_starts(engine_, view->handle, scenes.data(), T.data(), (int)scenes.size(), starts.data(), numKept,
                                              k.v, nullptr, results.data()), "dslam_track_camera_sdf_starts");
    int winner = -1;
    for (int s = 0; s < numKept; s++) {
      const dslam_track_sdf_result &r = results[(size_t)s];
      if (r.valid_last < minValid || r.stop_reason == 3) continue;
      if (winner < 0 || r.cost_last < results[(size_t)winner].cost_last) winner = s;
    }
    if (winner < 0) return false;
    if (out) *out = results[(size_t)winner];
    WritePoseBack(current, &starts[(size_t)winner * 16]);
    return true;
  }
  /// (extension) Which local maps a camera view reaches (dslam_survey_views, law in DESIGN.md section 20): under the
  /// maps' estimatedGlobalPoses, `reach[i]` becomes the resident blocks of map i whose loosened sphere meets the frustum of
  /// the camera `M` (world -> camera, metres, column-major) with the image `size`, between nearM and farM metres (farM 0:
  /// no far plane), and `nearest[i]` the smallest depth, in voxels, among them (INT32_MAX for none).  Up to
  /// DSLAM_MAX_SURVEY_MAPS local maps; only the hash tables are read.
  void SurveyLocalMapsInView(const float M[16], const float intrinsics[4], Vector2i size, float nearM, float farM,
                             std::vector<int32_t> &reach, std::vector<int32_t> &nearest) {
    std::vector<const dslam_scene *> scenes;
    std::vector<float> T;
    ListLocalMaps(scenes, T);
    SurveyListedMaps(M, intrinsics, size, nearM, farM, scenes, T, reach, nearest);
  }
  /// (extension) TrackAllLocalMaps against the local maps the camera can reach: the maps are surveyed at the start pose
  /// (SurveyLocalMapsInView with the depth image's size, nearM and farM), dslam_select_view_maps keeps at most
  /// DSLAM_MAX_RENDER_MAPS of them -- `current` always, so the map being fused into stays listed while it is empty -- and
  /// dslam_track_camera_sdf runs on that sub-list, in list order.  With nearM < D <= farM for every depth pixel a map the
  /// survey drops holds no block at any pixel, and the result is TrackAllLocalMaps' bit for bit;
  /// the defaults, no near and no far plane, cover every depth.  Unlike TrackAllLocalMaps it takes more than
  /// DSLAM_MAX_RENDER_MAPS local maps.  kept (optional): the indices of the listed maps, ascending.
  bool TrackVisibleLocalMaps(ITMLocalMap *current, float nearM = 0.0f, float farM = 0.0f, dslam_track_sdf_result *out = nullptr,
                             std::vector<int32_t> *kept = nullptr) {
    if (view == nullptr) throw std::runtime_error("TrackVisibleLocalMaps: no view yet (call UpdateView first)");
    std::vector<const dslam_scene *> scenes;
    std::vector<float> T;
    const int cur = ListLocalMaps(scenes, T, current);
    if (cur < 0) throw std::runtime_error("TrackVisibleLocalMaps: `current` is not one of the local maps");
    float Wf[16];
    WorldPoseOf(current, Wf);
    std::vector<int32_t> keep;
    SelectLocalMapsInView(Wf, view->calib->intrinsics_d.projectionParamsSimple.all.v, view->depth->noDims, nearM, farM, cur, scenes, T, keep);
    if (kept) *kept = keep;
    return TrackListedMaps(current, scenes, T, Wf, out);
  }
  /// (extension) GetImageAllLocalMaps of the local maps the free camera can reach: the maps are surveyed at `pose`
  /// (the image's size, nearM, farM), at most DSLAM_MAX_RENDER_MAPS are kept -- the nearest first -- and
  /// dslam_get_image_multi draws that sub-list.  Every ray sample in a block of a dropped map lies outside the view, but
  /// the renderer's range image is bounded by projected block corners and the renderer draws whatever its rays meet, so
  /// the image is GetImageAllLocalMaps' only where no dropped block's bounding box touches the image and nothing lies
  /// beyond farM.  When no map reaches, map 0 is drawn.  kept (optional): the listed maps.
  void GetImageVisibleLocalMaps(ITMUChar4Image *out, ITMFloatImage *outFloat, GetImageType type, ITMPose *pose,
                                ITMIntrinsics *intrinsics, float nearM = 0.0f, float farM = 0.0f, std::vector<int32_t> *kept = nullptr) {
    if (mapManager->numLocalMaps() == 0 || pose == nullptr || intrinsics == nullptr) return;
    int t;
    Vector2i sz;
    if (!FreeCameraImage(type, out, outFloat, t, sz)) return;
    std::vector<const dslam_scene *> scenes;
    std::vector<float> T;
    ListLocalMaps(scenes, T);
    std::vector<int32_t> keep;
    SelectLocalMapsInView(pose->GetM().m, intrinsics->projectionParamsSimple.all.v, sz, nearM, farM, -1, scenes, T, keep);
    if (kept) *kept = keep;
    DrawLocalMaps(scenes, T, t, sz, out, outFloat, pose, intrinsics);
  }
  /// inverse of a rigid transform (column-major): [R^T | -(R^T t)], each sum evaluated left to right
  static void RigidInverse(const double M[16], double out[16]) {
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) out[c * 4 + r] = M[r * 4 + c];
      out[12 + r] = -((M[r * 4 + 0] * M[12] + M[r * 4 + 1] * M[13]) + M[r * 4 + 2] * M[14]);
      out[r * 4 + 3] = 0.0;
    }
    out[15] = 1.0;
  }
  /// C = A B (column-major), each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
  static void RigidProduct(const double A[16], const double B[16], double C[16]) {
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++)
        C[c * 4 + r] = ((A[0 * 4 + r] * B[c * 4 + 0] + A[1 * 4 + r] * B[c * 4 + 1]) + A[2 * 4 + r] * B[c * 4 + 2]) + A[3 * 4 + r] * B[c * 4 + 3];
  }
  /// ITMMeshingEngine::MeshScene(mesh, scene)
  void MeshScene(ITMMesh *mesh, const ITMScene<ITMVoxel, ITMVoxelIndex> *scene) {
    int n = 0;
    dslam_check(dslam_mesh_scene(engine_, scene->handle, (int)mesh->noMaxTriangles, settings->meshWithColour, &n), "dslam_mesh_scene");
    mesh->noTotalTriangles = (unsigned)n;
    mesh->triangles.resize((size_t)n + 1);  // never a null data()
    mesh->colours.resize(settings->meshWithColour ? (size_t)n + 1 : 0);
    dslam_check(dslam_mesh_download(engine_, &mesh->triangles[0].p0.x, settings->meshWithColour ? &mesh->colours[0].p0.x : nullptr, n),
                "dslam_mesh_download");
    mesh->triangles.resize((size_t)n);
    if (settings->meshWithColour) mesh->colours.resize((size_t)n);
  }

  /// (extension) The whole reconstruction as one mesh in the global frame: every local map of mapManager under its
  /// estimatedGlobalPose.GetM(), one surface where maps overlap -- the reference writes one mesh per local map, each in its
  /// own coordinates (SystemEntry.cpp:364-370).  dslam_mesh_scene_multi, law in DESIGN.md section 12.  Does nothing
  /// before the first local map; honours settings->meshWithColour.
  void MeshAllLocalMaps(ITMMesh *mesh) {
    const int n = mapManager->numLocalMaps();
    if (n == 0) return;
    if (n > DSLAM_MAX_RENDER_MAPS)
      throw std::runtime_error("MeshAllLocalMaps: " + std::to_string(n) + " local maps, at most " +
                               std::to_string(DSLAM_MAX_RENDER_MAPS) + " can be meshed in one call");
    std::vector<const dslam_scene *> scenes(n);
    std::vector<float> T((size_t)n * 16);
    for (int i = 0; i < n; i++) {
      const ITMLocalMap *m = mapManager->getLocalMap(i);
      scenes[i] = m->scene->handle;
      memcpy(&T[(size_t)i * 16], m->estimatedGlobalPose.GetM().m, 16 * sizeof(float));
    }
    int total = 0;
    dslam_check(dslam_mesh_scene_multi(engine_, scenes.data(), T.data(), n, (int)mesh->noMaxTriangles, settings->meshWithColour,
                                       &total, nullptr), "dslam_mesh_scene_multi");
    mesh->noTotalTriangles = (unsigned)total;
    mesh->triangles.resize((size_t)total + 1);  // never a null data()
    mesh->colours.resize(settings->meshWithColour ? (size_t)total + 1 : 0);
    dslam_check(dslam_mesh_download(engine_, &mesh->triangles[0].p0.x, settings->meshWithColour ? &mesh->colours[0].p0.x : nullptr, total),
                "dslam_mesh_download");
    mesh->triangles.resize((size_t)total);
    if (settings->meshWithColour) mesh->colours.resize((size_t)total);
  }
  /// (extension) MeshAllLocalMaps into one OBJ file: replaces the export loop over the local maps.
  void SaveAllLocalMapsToMesh(const char *objFileName) {
    const int n = mapManager->numLocalMaps();
    if (n == 0) return;
    const unsigned long long cap = (unsigned long long)settings->numLocalBlocks * 32ull * (unsigned long long)n;
    ITMMesh mesh((unsigned)(cap > 0x7fffffffull ? 0x7fffffffull : cap));
    MeshAllLocalMaps(&mesh);
    mesh.WriteOBJ(objFileName);
  }

  dslam_engine *GetDslamEngine() const { return engine_; }

 protected:
  const ITMLibSettings *settings;
  ITMView *view;
  ITMDenseMapper *denseMapper;
  ITMViewBuilder *viewBuilder;
  ITMTrackingController *trackingController;
  ITMVisualisationEngine<ITMVoxel, ITMVoxelIndex> *visualisationEngine;
  ITMVoxelMapGraphManager *mapManager;
  ITMActiveMapManager *mActiveDataManger;

 private:
  /// every local map's scene handle and estimatedGlobalPose.GetM(), in mapManager's order; returns the index of `which`
  /// (-1: not among them)
  int ListLocalMaps(std::vector<const dslam_scene *> &scenes, std::vector<float> &T, const ITMLocalMap *which = nullptr) const {
    const int n = mapManager->numLocalMaps();
    int at = -1;
    scenes.resize((size_t)n);
    T.resize((size_t)n * 16);
    for (int i = 0; i < n; i++) {
      const ITMLocalMap *m = mapManager->getLocalMap(i);
      if (m == which) at = i;
      scenes[(size_t)i] = m->scene->handle;
      memcpy(&T[(size_t)i * 16], m->estimatedGlobalPose.GetM().m, 16 * sizeof(float));
    }
    return at;
  }
  /// the dslam image type and the size of a FREECAMERA_* request; false: nothing to draw (another type, no image)
  static bool FreeCameraImage(GetImageType type, const ITMUChar4Image *out, const ITMFloatImage *outFloat, int &t, Vector2i &sz) {
    switch (type) {
      case InfiniTAM_IMAGE_FREECAMERA_SHADED: t = DSLAM_IMAGE_SHADED; break;
      case InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME: t = DSLAM_IMAGE_COLOUR_FROM_VOLUME; break;
      case InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL: t = DSLAM_IMAGE_COLOUR_FROM_NORMAL; break;
      case InfiniTAM_IMAGE_FREECAMERA_DEPTH: t = DSLAM_IMAGE_DEPTH; break;
      default: return false;
    }
    sz = (t == DSLAM_IMAGE_DEPTH) ? (outFloat ? outFloat->noDims : Vector2i(0, 0)) : (out ? out->noDims : Vector2i(0, 0));
    return sz.x > 0;
  }
  /// dslam_get_image_multi of the listed maps into the caller's image, through the all-maps render state
  void DrawLocalMaps(const std::vector<const dslam_scene *> &scenes, const std::vector<float> &T, int t, Vector2i sz,
                     ITMUChar4Image *out, ITMFloatImage *outFloat, ITMPose *pose, ITMIntrinsics *intrinsics) {
    // The render state's visible list has to hold the largest pool among the listed maps (dslam_get_image_multi rejects
    // a list otherwise), and pools differ once maps have been compacted: it is made from the listed scene with the
    // largest pool (the first of them), and made again when the image size changes or a listed pool exceeds it.
    const dslam_scene *largest = nullptr;
    int largestBlocks = 0;
    for (size_t i = 0; i < scenes.size(); i++) {
      dslam_scene_params p;
      dslam_check(dslam_scene_get_params(scenes[i], &p), "dslam_scene_get_params");
      if (p.num_local_blocks > largestBlocks) { largestBlocks = p.num_local_blocks; largest = scenes[i]; }
    }
    if (largest == nullptr) return;
    if (renderState_allmaps_ == nullptr || allmapsSize_.x != sz.x || allmapsSize_.y != sz.y || largestBlocks > allmapsBlocks_) {
      delete renderState_allmaps_;
      renderState_allmaps_ = nullptr; allmapsScene_ = nullptr;
      renderState_allmaps_ = new ITMRenderState_VH(engine_, largest, sz);
      allmapsSize_ = sz; allmapsBlocks_ = largestBlocks; allmapsScene_ = largest;
    }
    dslam_check(dslam_get_image_multi(engine_, scenes.data(), T.data(), (int)scenes.size(), renderState_allmaps_->handle,
                                      pose->GetM().m, intrinsics->projectionParamsSimple.all.v, t,
                                      t == DSLAM_IMAGE_DEPTH ? nullptr : &out->GetData(MEMORYDEVICE_CPU)->x,
                                      t == DSLAM_IMAGE_DEPTH ? outFloat->GetData(MEMORYDEVICE_CPU) : nullptr), "dslam_get_image_multi");
    if (deferred_) dslam_check(dslam_engine_synchronize(engine_), "dslam_engine_synchronize");
  }
  /// world -> camera = pose_d->GetM() T_current of `current`, composed in double (RigidProduct) and rounded to float32
  static void WorldPoseOf(const ITMLocalMap *current, float Wf[16]) {
    double Md[16], Tc[16], Wd[16];
    for (int i = 0; i < 16; i++) {
      Md[i] = (double)current->trackingState->pose_d->GetM().m[i];
      Tc[i] = (double)current->estimatedGlobalPose.GetM().m[i];
    }
    RigidProduct(Md, Tc, Wd);
    for (int i = 0; i < 16; i++) Wf[i] = (float)Wd[i];
  }
  /// dslam_track_camera_sdf of the current view against the listed maps from the start Wf (world -> camera); when a step
  /// was accepted, pose_d = (world -> camera) T_current^-1 is written back and the call returns true
  bool TrackListedMaps(ITMLocalMap *current, const std::vector<const dslam_scene *> &scenes, const std::vector<float> &T,
                       float Wf[16], dslam_track_sdf_result *out) {
    const Vector4f k = view->calib->intrinsics_d.projectionParamsSimple.all;
    dslam_track_sdf_result res;
    dslam_check(dslam_track_camera_sdf(engine_, view->handle, scenes.data(), T.data(), (int)scenes.size(), Wf, k.v, nullptr, &res),
                "dslam_track_camera_sdf");
    if (out) *out = res;
    if (res.levels_stepped == 0) return false;
    WritePoseBack(current, Wf);
    return true;
  }
  /// pose_d = (world -> camera) T_current^-1 of `current`, composed in double (RigidInverse, RigidProduct), rounded to float32
  static void WritePoseBack(ITMLocalMap *current, const float Wf[16]) {
    double Md[16], Tc[16], Wd[16], inv[16];
    for (int i = 0; i < 16; i++) {
      Wd[i] = (double)Wf[i];
      Tc[i] = (double)current->estimatedGlobalPose.GetM().m[i];
    }
    RigidInverse(Tc, inv);
    RigidProduct(Wd, inv, Md);
    Matrix4f M;
    for (int i = 0; i < 16; i++) M.m[i] = (float)Md[i];
    current->trackingState->pose_d->SetM(M);
  }
  /// dslam_survey_views of the listed maps from one camera: reach and nearest per map
  void SurveyListedMaps(const float M[16], const float intrinsics[4], Vector2i size, float nearM, float farM,
                        const std::vector<const dslam_scene *> &scenes, const std::vector<float> &T, std::vector<int32_t> &reach,
                        std::vector<int32_t> &nearest) {
    const int n = (int)scenes.size();
    dslam_survey_view v;
    memcpy(v.M, M, sizeof v.M);
    memcpy(v.intrinsics, intrinsics, sizeof v.intrinsics);
    v.width = size.x; v.height = size.y;
    v.near_m = nearM; v.far_m = farM;
    std::vector<int32_t> live((size_t)n), r((size_t)n), z((size_t)n);
    dslam_check(dslam_survey_views(engine_, scenes.data(), T.data(), n, &v, 1, nullptr, live.data(), r.data(), z.data(), nullptr),
                "dslam_survey_views");
    reach.swap(r);
    nearest.swap(z);
  }
  /// survey (scenes, T) from the camera M and cut both down to the maps dslam_select_view_maps keeps (`keep`, ascending;
  /// alwaysKeep: an index or -1); when none is kept, map 0 stays
  void SelectLocalMapsInView(const float M[16], const float intrinsics[4], Vector2i size, float nearM, float farM, int alwaysKeep,
                             std::vector<const dslam_scene *> &scenes, std::vector<float> &T, std::vector<int32_t> &keep) {
    std::vector<int32_t> reach, nearest;
    SurveyListedMaps(M, intrinsics, size, nearM, farM, scenes, T, reach, nearest);
    dslam_view_select_params sp = {0, 0, alwaysKeep, 0};
    dslam_view_select_result res;
    keep.assign(DSLAM_MAX_RENDER_MAPS, 0);
    dslam_check(dslam_select_view_maps(reach.data(), nearest.data(), 1, (int)scenes.size(), &sp, keep.data(), &res), "dslam_select_view_maps");
    keep.resize((size_t)res.selected);
    if (keep.empty()) keep.push_back(0);
    for (size_t k = 0; k < keep.size(); k++) {   // (ascending, so an entry is never overwritten before it is read)
      scenes[k] = scenes[(size_t)keep[k]];
      memmove(&T[k * 16], &T[(size_t)keep[k] * 16], 16 * sizeof(float));
    }
    scenes.resize(keep.size());
    T.resize(keep.size() * 16);
  }

  dslam_engine *engine_;
  bool deferred_;   ///< the engine runs asynchronously (default; DSLAM_MIRROR_SYNC=1 turns it off)
  const ITMScene<ITMVoxel, ITMVoxelIndex> *freeviewScene_;
  ITMRenderState *renderState_freeview_;
  Vector2i freeviewSize_;
  ITMRenderState *renderState_allmaps_;   ///< GetImageAllLocalMaps' own render state
  Vector2i allmapsSize_;
  int allmapsBlocks_;                     ///< ... the pool size its visible list holds
  const dslam_scene *allmapsScene_;       ///< ... the scene it was made from (its counters read that scene: gone with it)
};

}  // namespace Engine
}  // namespace ITMLib

// global names the reference uses unqualified (InfiniTamDriver.h:132-137,362; DenseSlam.h:511)
using ITMLib::Engine::ITMActiveMapManager;
using ITMLib::Engine::ITMLocalMap;
using ITMLib::Engine::ITMVisualisationEngine;
using ITMLib::Engine::ITMVoxelMapGraphManager;
using ITMLib::Objects::ITMRenderState_VH;
