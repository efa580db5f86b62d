// pack_harness.cpp -- drives ITMMainEngine::CompactLocalMap through the ITMLib mirror: two local maps fused from the
// keyframes (map 0 from all but the last, map 1 from all but the first), map 0's depth image and the composite image of
// both maps (GetImageAllLocalMaps) from the first keyframe's pose, CompactLocalMap(0, headroom), both images again -- the
// composite now draws a compacted map next to one with the settings' pool --, CompactLocalMap(1, headroom), the composite
// a third time, and one more keyframe fused into the compacted map 0 (its new render state at work).
//
//   pack_harness <frames.bin> <out.bin>
// frames.bin: int32 W, H, N; N x (rgba[H][W][4], int16 depth[H][W], float M[16] column-major); float intr[4];
//             float voxel_size, mu, frustum_min, frustum_max; int32 max_w, num_local_blocks, num_buckets, num_excess;
//             int32 headroom
// out.bin:    dslam_pack_info of the compaction; int32 new pool size;
//             float depth_before[H][W], depth_after[H][W];
//             float all_before[H][W], all_after[H][W], all_after_both[H][W] (the composite of both maps);
//             the map before the compaction, then after it (pool sizes differ): int32 last_free, last_free_ex; hash table,
//             allocation list, excess list, voxel blocks as the dslam_download_* calls return them; after it also
//             int32 last_seen[pool];
//             int32 no_visible, last_free after the keyframe fused into the compacted map
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib/Engine/ITMMainEngine.h"

using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

class PackHarness : public ITMMainEngine {
 public:
  PackHarness(const ITMLibSettings *settings, const ITMRGBDCalib *calib, const Vector2i &sz)
      : ITMMainEngine(settings, calib, sz, sz), rgb_itm_(new ITMUChar4Image(sz, true, true)),
        raw_depth_itm_(new ITMShortImage(sz, true, true)) {}
  ~PackHarness() { delete rgb_itm_; delete raw_depth_itm_; }
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

// the map's state as the download calls return it
static void dump_map(FILE *o, dslam_engine *e, const dslam_scene *s, size_t n_entries, size_t n_local, size_t n_excess, bool with_last_seen) {
  std::vector<dslam_hash_entry> table(n_entries);
  std::vector<int32_t> alloc_list(n_local), excess_list(n_excess), last_seen(n_local);
  std::vector<dslam_voxel> voxels(n_local * 512);
  dslam_stats st;
  if (dslam_download_hash_table(e, s, table.data()) < 0 || dslam_download_allocation_list(e, s, alloc_list.data()) < 0 ||
      dslam_download_excess_list(e, s, excess_list.data()) < 0 || dslam_download_last_seen(e, s, last_seen.data()) < 0 ||
      dslam_download_voxel_blocks(e, s, 0, (int)n_local, voxels.data()) < 0 || dslam_get_stats(e, s, nullptr, &st) < 0)
    throw std::runtime_error(dslam_last_error());
  const int32_t tops[2] = {st.last_free_block_id, st.last_free_excess_id};
  fwrite(tops, 4, 2, o);
  fwrite(table.data(), sizeof(dslam_hash_entry), table.size(), o);
  fwrite(alloc_list.data(), 4, alloc_list.size(), o);
  fwrite(excess_list.data(), 4, excess_list.size(), o);
  fwrite(voxels.data(), sizeof(dslam_voxel), voxels.size(), o);
  if (with_last_seen) fwrite(last_seen.data(), 4, last_seen.size(), o);
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s frames.bin out.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror("frames"); return 2; }
  int32_t hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  const int W = hdr[0], H = hdr[1], N = hdr[2];
  if (N <= 1) return 2;
  std::vector<std::vector<uint8_t>> rgba(N, std::vector<uint8_t>((size_t)W * H * 4));
  std::vector<std::vector<int16_t>> depth(N, std::vector<int16_t>((size_t)W * H));
  std::vector<Matrix4f> poses(N);
  for (int i = 0; i < N; i++) {
    if (fread(rgba[i].data(), 1, rgba[i].size(), f) != rgba[i].size()) return 2;
    if (fread(depth[i].data(), 2, depth[i].size(), f) != depth[i].size()) return 2;
    if (fread(poses[i].m, 4, 16, f) != 16) return 2;
  }
  float intr[4], sp[4];
  int32_t ip[4], headroom;
  if (fread(intr, 4, 4, f) != 4 || fread(sp, 4, 4, f) != 4 || fread(ip, 4, 4, f) != 4 || fread(&headroom, 4, 1, f) != 1) return 2;
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
    {
      PackHarness drv(settings, calib, Vector2i(W, H));
      ITMVoxelMapGraphManager *maps = drv.GetMapManager();
      const int idx = maps->createNewLocalMap();
      ITMLocalMap *map = maps->getLocalMap(idx);
      // all keyframes but the last go into the map before the compaction
      for (int i = 0; i < N - 1; i++) {
        map->trackingState->pose_d->SetM(poses[i]);
        drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
        drv.IntegrateLocalMap(map);
      }
      // a second map in the same frame, from all keyframes but the first: it keeps the settings' pool until its turn
      const int idx1 = maps->createNewLocalMap();
      ITMLocalMap *map1 = maps->getLocalMap(idx1);
      for (int i = 1; i < N; i++) {
        map1->trackingState->pose_d->SetM(poses[i]);
        drv.UpdateView(rgba[i].data(), depth[i].data(), (double)i);
        drv.IntegrateLocalMap(map1);
      }
      ITMFloatImage depth_before(Vector2i(W, H), true, true), depth_after(Vector2i(W, H), true, true);
      ITMFloatImage all_before(Vector2i(W, H), true, true), all_after(Vector2i(W, H), true, true), all_after_both(Vector2i(W, H), true, true);
      ITMPose camera;
      camera.SetM(poses[0]);
      ITMIntrinsics k = drv.DepthIntrinsics();
      drv.GetImage(nullptr, &depth_before, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &camera, &k, map);
      drv.GetImageAllLocalMaps(nullptr, &all_before, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &camera, &k);

      FILE *o = fopen(argv[2], "wb");
      if (!o) { perror("out"); return 2; }
      dslam_engine *e = drv.GetDslamEngine();
      const size_t n_entries = (size_t)ip[2] + ip[3];
      std::vector<char> before_dump;
      dslam_pack_info info;
      // (the header and the images come first in the file: the map before the compaction is dumped to memory)
      FILE *mem = tmpfile();
      if (!mem) { perror("tmpfile"); return 2; }
      dump_map(mem, e, map->scene->handle, n_entries, (size_t)ip[1], (size_t)ip[3], false);
      drv.CompactLocalMap(idx, headroom, &info);
      drv.GetImage(nullptr, &depth_after, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &camera, &k, map);
      drv.GetImageAllLocalMaps(nullptr, &all_after, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &camera, &k);
      // the other map's turn (map 0 is not touched by it): both pools now differ from the settings' and from each other
      dslam_pack_info info1;
      drv.CompactLocalMap(idx1, headroom, &info1);
      drv.GetImageAllLocalMaps(nullptr, &all_after_both, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_DEPTH, &camera, &k);
      const int32_t pool = map->scene->index.getNumAllocatedVoxelBlocks();
      fwrite(&info, sizeof info, 1, o);
      fwrite(&pool, 4, 1, o);
      fwrite(depth_before.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
      fwrite(depth_after.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
      fwrite(all_before.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
      fwrite(all_after.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
      fwrite(all_after_both.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, o);
      before_dump.resize((size_t)ftell(mem));
      rewind(mem);
      if (fread(before_dump.data(), 1, before_dump.size(), mem) != before_dump.size()) return 2;
      fclose(mem);
      fwrite(before_dump.data(), 1, before_dump.size(), o);
      dump_map(o, e, map->scene->handle, n_entries, (size_t)pool, (size_t)ip[3], true);
      // the compacted map lives on: the last keyframe through its new render state
      map->trackingState->pose_d->SetM(poses[N - 1]);
      drv.UpdateView(rgba[N - 1].data(), depth[N - 1].data(), (double)(N - 1));
      drv.IntegrateLocalMap(map);
      const int32_t tail[2] = {(int32_t)((ITMRenderState_VH *)map->renderState)->noVisibleEntries, (int32_t)map->scene->localVBA.lastFreeBlockId};
      fwrite(tail, 4, 2, o);
      fclose(o);
      printf("pack_harness ok: %d keyframes, %d blocks in %lld bytes, pool %d -> %d; map 1: %d blocks\n", N, info.blocks,
             (long long)info.total_bytes, ip[1], pool, info1.blocks);
    }
    delete calib;
    delete settings;
  } catch (const std::exception &ex) {
    fprintf(stderr, "pack_harness failed: %s\n", ex.what());
    return 1;
  }
  return 0;
}
