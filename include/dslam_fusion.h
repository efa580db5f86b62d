/*
 * dslam_fusion.h -- C ABI of libdslam_fusion.so, the MI355X (gfx950) TSDF fusion + raycast engine.
 *
 * This is the drop-in boundary for the voxel-block-hashing hot path of
 * Hansry/DenseSLAM-Global-Consistency-h.  Every entry point names the ITMLib engine method it stands in
 * for and the reference call site that reaches it (file:line under /root/reference/src/DenseSLAM).  The
 * ITMLib-compatible C++ classes in denseslam-global-consistency-h_amd/itmlib/ (ITMDenseMapper,
 * ITMSceneReconstructionEngine, ITMVisualisationEngine, ITMSwappingEngine, ...) are thin wrappers over
 * these functions, so InfiniTamDriver / DenseSlam / DenseSLAMGUI compile and run unchanged on top.
 *
 * Conventions
 *  - plain C, no exceptions across the boundary; every function returns a dslam_status (0 = ok).
 *  - 4x4 matrices are float[16], COLUMN-major, exactly ORUtils::Matrix4f::m[] (InfiniTamDriver.cpp:208-226).
 *  - intrinsics are float[4] = (fx, fy, cx, cy) = ITMIntrinsics::projectionParamsSimple.all
 *    (InfiniTamDriver.cpp:60-67).
 *  - "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory on the engine's device.
 *  - the engine is used from one thread (DenseSlam's main thread); it owns one HIP stream.
 *    In the default synchronous mode every call has completed (including D2H copies) when it returns,
 *    which is what the reference callers assume (DenseSlam.h:151-152,162-163).  dslam_engine_set_async
 *    lets a caller pipeline frames and synchronise explicitly (the ITMLib mirror in itmlib/ runs the engine this way
 *    and synchronises where data is handed to the host).
 *  - conditions only the device can detect (an allocation ray longer than the order key encodes: DSLAM_ERR_UNSUPPORTED;
 *    a tile count of an ordered compaction that never arrived, after which the map state is undefined: DSLAM_ERR_HIP)
 *    are returned by the first call that waits for the stream after the kernel in question: the call itself on a
 *    synchronous engine; on an asynchronous one the next dslam_engine_synchronize, dslam_fence_wait, dslam_get_stats,
 *    read-back (dslam_download_*, an image into ordinary host memory, dslam_mesh_download ...).  Told once per
 *    occurrence; dslam_get_stats keeps reporting them for the scene they happened in until dslam_scene_reset.
 */
#ifndef DSLAM_FUSION_H
#define DSLAM_FUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSLAM_BLOCK_SIZE 8    /* SDF_BLOCK_SIZE  */
#define DSLAM_BLOCK_SIZE3 512 /* SDF_BLOCK_SIZE3, used at InfiniTamDriver.h:346 */

/* upstream ITMLibDefines.h defaults (corroborated by the reference's memory logs) */
#define DSLAM_DEFAULT_LOCAL_BLOCK_NUM 0x40000 /* SDF_LOCAL_BLOCK_NUM   */
#define DSLAM_DEFAULT_BUCKET_NUM 0x100000     /* SDF_BUCKET_NUM        */
#define DSLAM_DEFAULT_EXCESS_LIST_SIZE 0x20000 /* SDF_EXCESS_LIST_SIZE */
/* Largest voxel pool of one scene: 4 GiB of voxels.  The ray march and its straddling-cell gather address a voxel by a
 * 32-bit byte offset from the pool's base (4096 * slot + at most 4092, below 2^32 up to slot 0xfffff); dslam_scene_create
 * refuses a larger num_local_blocks, for a pool of its own and for a caller's buffer alike. */
#define DSLAM_MAX_LOCAL_BLOCKS 0x100000
#define DSLAM_TRANSFER_BLOCK_NUM 0x1000       /* SDF_TRANSFER_BLOCK_NUM */
#define DSLAM_MAX_RENDERING_BLOCKS (65536 * 4)
/* local maps one dslam_get_image_multi call can draw (a bit each in a 64-bit mask per 8x8 pixel tile) */
#define DSLAM_MAX_RENDER_MAPS 64

typedef enum {
  DSLAM_OK = 0,
  DSLAM_ERR_INVALID = -1,     /* bad argument (null handle, size mismatch, ...) */
  DSLAM_ERR_HIP = -2,         /* a HIP runtime call failed; see dslam_last_error() */
  DSLAM_ERR_UNSUPPORTED = -3, /* parameter combination outside what the kernels are built for */
  DSLAM_ERR_NO_DEVICE = -4
} dslam_status;

/* ITMHashEntry {Vector3s pos; int offset; int ptr;}  -- 16 bytes.
 * ptr >= 0: slot in the voxel block array; ptr == -1: swapped out; ptr < -1: unused entry.
 * offset >= 1: next entry of the bucket lives at num_buckets + offset - 1. */
typedef struct {
  int16_t pos[3];
  int16_t _pad;
  int32_t offset;
  int32_t ptr;
} dslam_hash_entry;

/* ITMVoxel = ITMVoxel_s_rgb {short sdf; uchar w_depth; Vector3u clr; uchar w_color;} -- 8 bytes
 * (sizeof(ITMVoxel) at InfiniTamDriver.h:333-335).  Empty voxel: sdf 32767, everything else 0. */
typedef struct {
  int16_t sdf;
  uint8_t w_depth;
  uint8_t clr[3];
  uint8_t w_color;
  uint8_t _pad;
} dslam_voxel;

/* ITMSceneParams + the compile-time pool sizes of ITMLibDefines.h made runtime fields. */
typedef struct {
  float voxel_size;   /* metres                     (upstream default 0.005) */
  float mu;           /* truncation band, metres    (0.02) */
  int32_t max_w;      /* weight clamp, <= 255       (100)  */
  float frustum_min;  /* viewFrustum_min, metres    (0.2)  */
  float frustum_max;  /* viewFrustum_max, metres    (3.0)  */
  int32_t stop_integrating_at_max_w;
  int32_t num_local_blocks; /* SDF_LOCAL_BLOCK_NUM; 0 -> default; at most DSLAM_MAX_LOCAL_BLOCKS */
  int32_t num_buckets;      /* SDF_BUCKET_NUM, power of two; 0 -> default */
  int32_t num_excess;       /* SDF_EXCESS_LIST_SIZE; 0 -> default */
  int32_t use_swapping;     /* ITMLibSettings::useSwapping: allocate the host-side global cache */
  int32_t history_words;    /* 64-bit words per visible-list ring per block (ring holds 64*words lists,
                               bounds max_age / defusion maxSize); 0 -> 4 */
} dslam_scene_params;

/* ITMLib::Engine::WeightParams {depthWeighting, maxNewW, maxDistance} (SystemEntry.cpp:183-187,
 * InfiniTamDriver.h:189,196). */
typedef struct {
  int32_t depth_weighting;
  int32_t max_new_w;   /* 1..255 (a voxel weight is one byte; the kernels tabulate 1/(w_depth + newW)) */
  float max_distance;
} dslam_weight_params;

/* What InfiniTamDriver reads back after every call (InfiniTamDriver.h:209-210,344-351,366-370). */
typedef struct {
  int32_t num_allocated_blocks; /* scene->index.getNumAllocatedVoxelBlocks() == num_local_blocks */
  int32_t last_free_block_id;   /* scene->localVBA.lastFreeBlockId */
  int32_t last_free_excess_id;  /* scene->index.lastFreeExcessListId */
  int32_t no_visible_entries;   /* ITMRenderState_VH::noVisibleEntries of the render state passed */
  int64_t decayed_block_count;  /* ITMDenseMapper::GetDecayedBlockCount() */
  int64_t slid_block_count;     /* blocks released (or swapped out) by SlideWindow* so far */
  int32_t frame_counter;        /* number of visible lists queued so far (fusion + defusion) */
  int32_t fusion_fifo_len;
  int32_t defusion_fifo_len;
  int32_t alloc_failures;       /* blocks the last allocation wanted but could not get (pool exhausted) */
  int32_t last_swapped_in;      /* blocks moved by the last IntegrateGlobalIntoLocal */
  int32_t last_swapped_out;     /* blocks moved by the last SaveToGlobalMemory */
} dslam_stats;

/* ITMMainEngine::GetImageType values used by the reference (InfiniTamDriver.cpp:16-38). */
typedef enum {
  DSLAM_IMAGE_SHADED = 0,             /* InfiniTAM_IMAGE_FREECAMERA_SHADED */
  DSLAM_IMAGE_COLOUR_FROM_VOLUME = 1, /* InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME */
  DSLAM_IMAGE_COLOUR_FROM_NORMAL = 2, /* InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL */
  DSLAM_IMAGE_DEPTH = 3               /* InfiniTAM_IMAGE_FREECAMERA_DEPTH (float metres) */
} dslam_image_type;

typedef struct dslam_engine dslam_engine;             /* device + stream + scratch: the *_HIP engines */
typedef struct dslam_scene dslam_scene;               /* ITMScene<ITMVoxel,ITMVoxelBlockHash> (+ITMGlobalCache) */
typedef struct dslam_render_state dslam_render_state; /* ITMRenderState_VH */
typedef struct dslam_view dslam_view;                 /* ITMView (rgb, depth) */
typedef struct dslam_fence dslam_fence;               /* a marker in the engine's stream (async mode) */

/* ---- engine ------------------------------------------------------------------------------------ */
const char *dslam_last_error(void);
const char *dslam_version(void);
/* ITMSceneReconstructionEngineFactory / ITMVisualisationEngineFactory / ITMSwappingEngineFactory for
 * the HIP device type (ITMMainEngine ctor, InfiniTamDriver.h:102). */
int dslam_engine_create(int device_index, dslam_engine **out);
/* The NUMA node of the host the device hangs off (-1 if the platform does not say; read from sysfs by PCI bus id).  A caller
 * that fills page-locked images every frame (CvToItm, InfiniTamDriver.cpp:17-75) should run on that node: the 1.8 MB fill of a
 * 640x480 frame takes ~60 us there and ~160 us from the other socket of a two-socket host.  May be
 * called before any engine exists. */
int dslam_device_numa_node(int device_index, int *node_out);
/* Waits for both streams of the engine and ends its life for the caller.  Handles may be destroyed in any order: the
 * scenes, render states, views and frame stores made from the engine may still exist, and each of them is destroyed by
 * its own destroy call as before, whether that comes before or after this one -- the engine's object and streams are
 * kept until the last of them has gone, and freed by that call.  Fences the caller still holds are detached as before
 * (dslam_fence_wait / _query / _destroy on them stay valid).  No other call may be given a destroyed engine, nor a
 * handle of one for anything but its destroy call.  The threading rule above holds unchanged: the engine and its
 * handles, their destroy calls included, are used from one thread. */
int dslam_engine_destroy(dslam_engine *e);
/* Test hook: engine objects of this process that have not been freed yet -- created and not destroyed, or destroyed
 * while handles made from them are left (see dslam_engine_destroy).  Needs no engine. */
int dslam_debug_live_engines(int *out);
int dslam_engine_set_async(dslam_engine *e, int async_mode);
/* waits for everything enqueued so far; returns what kernels reported since the last synchronising call (above) */
int dslam_engine_synchronize(dslam_engine *e);
/* native hipStream_t of the engine, for callers that enqueue their own work (RCCL, torch). */
void *dslam_engine_stream(dslam_engine *e);
/* Pipelining across PCIe (async mode only; the reference's own driver is synchronous and needs none of this).
 * With dslam_engine_set_async(e, 1) and caller images in dslam_host_alloc memory:
 *  - dslam_view_update copies on a second (copy) stream into one of two landing buffers of the view while the kernels
 *    of the previous frame, enqueued earlier, keep the GPU busy; it returns when the frame has landed (the calling
 *    thread sits out the copy, the GPU does not).  A frame whose depth image directly follows its RGBA image in
 *    memory goes up as one copy.
 *  - dslam_get_image into a page-locked image returns at once; the render kernel stores the pixels there itself.
 *  - a fence marks "everything enqueued on the engine so far": record it after a frame's last call, wait for it
 *    before reading that frame's output image or rewriting its input images. */
int dslam_fence_create(dslam_engine *e, dslam_fence **out);
int dslam_fence_destroy(dslam_fence *f);
int dslam_fence_record(dslam_engine *e, dslam_fence *f);
int dslam_fence_wait(dslam_fence *f);               /* blocks the calling thread; a fence never recorded has passed */
int dslam_fence_query(dslam_fence *f, int *done);   /* non-blocking */
/* Page-locked host memory for the caller's image buffers: what ORUtils::MemoryBlock's host side is whenever the
 * block also has a device side (upstream ORUtils/MemoryBlock.h Allocate: cudaMallocHost), i.e. the rgb / raw-depth
 * images DenseSlam::ProcessFrame fills each frame (DenseSlam.cpp:66-74).  Zero-filled.  In the default synchronous
 * mode dslam_view_update* DMA straight from such buffers; any other host pointer is staged through the engine's
 * own pinned buffer first.  Needs no engine (the images are created before it). */
int dslam_host_alloc(size_t bytes, void **out);
int dslam_host_free(void *p);
/* Self-test: the integration kernel divides with a 2-wide, scaling-free form of the hardware's IEEE division sequence
 * (csrc/integrate.hip div_ieee2).  Compares it with the native float division on `samples` random operand pairs
 * drawn from the kernel's operand ranges, on the device; *mismatches_out must come back 0. */
int dslam_selftest_division(dslam_engine *e, long long samples, long long *mismatches_out);
/* Test hook: CreateExpectedDepths' render-tile budget (MAX_RENDERING_BLOCKS, default DSLAM_MAX_RENDERING_BLOCKS).
 * Upstream drops, in visible-list order, every block whose tiles would reach the budget; real scenes never get
 * there (it takes > 262144 tiles), so the parity test of that rule lowers the budget instead. */
int dslam_debug_set_render_tile_budget(dslam_engine *e, int budget);
/* Test hook: ProcessFrame queues the frame's visible list on the ring either from the fusion kernel's block waves or -- from
 * this many visible blocks on (default 65536: maps whose visible voxels no longer fit the Infinity Cache) -- from extra
 * workgroups at the end of the same launch (csrc/integrate.hip, kPushJobMin).  From the same size on the fusion and
 * de-integration launches over a render state's list read and write their voxel blocks with the non-temporal cache policy
 * (chosen by the host from the visible count the last allocation pass reported).  Same bits either way; the parity test of
 * the second forms lowers the threshold instead of building a quarter-million-block scene for the oracle. */
int dslam_debug_set_push_job_min(dslam_engine *e, int min_visible_blocks);
/* Test hook: how many fusion / de-integration launches of this engine took the streaming (non-temporal) instantiation. */
int dslam_debug_stream_launches(dslam_engine *e, long long *count_out);
/* Test hook: how many fusion launches of this engine also computed GetImage's front end for their pose (ProcessFrame,
 * unless DSLAM_SPECULATIVE_FRONT_END=0), and how many GetImage calls took such a result instead of computing it. */
int dslam_debug_front_end_counts(dslam_engine *e, long long *computed_out, long long *adopted_out);
/* Test hook: of this engine's allocation passes so far, how many ran their marking kernel beside the previous
 * dslam_get_image's ray march on the engine's auxiliary stream, and how many ran it in the engine's stream.  A pass takes
 * the first way only on an asynchronous engine, for a scene without swapping, when the last call before it that enqueued
 * anything was a dslam_get_image that computed a range image (not one answered from its memo) and returned without
 * waiting for the image (no output buffer, or a page-locked one), when no call has waited for the engine's stream since
 * (dslam_engine_synchronize, a read-back; a dslam_fence_wait does not count), and dslam_engine_stream was never asked
 * for; DSLAM_OVERLAP_MARK=0 in the environment of dslam_engine_create selects the second way always.  Both ways
 * compute the same bytes. */
int dslam_debug_mark_overlap_counts(dslam_engine *e, long long *overlapped_out, long long *in_stream_out);
/* Test hook: allocation passes so far whose sweep (k_alloc_sweep) ran behind that k_mark on the auxiliary stream, its
 * hash-table writes put on a list that a small kernel publishes behind the previous dslam_get_image's march, and passes
 * whose sweep ran in the engine's stream.  The first way is taken by a pass whose k_mark overlaps (above) and that writes
 * the render state's own visible list (no list_out / count_out, no re-integration batch being planned);
 * DSLAM_OVERLAP_SWEEP=0 in the environment of dslam_engine_create selects the second way always, and so does
 * DSLAM_OVERLAP_MARK=0.  A dslam_process_frame that takes the first way returns once the two kernels are launched; the
 * rest of it, and a dslam_get_image / dslam_fence_record behind it that would only enqueue, are handed to the GPU by
 * the next dslam_view_update (while its copy is in flight) or by whatever other call touches the engine next.  Both ways
 * compute the same bytes. */
int dslam_debug_sweep_overlap_counts(dslam_engine *e, long long *overlapped_out, long long *in_stream_out);
/* Test hook: of the front ends dslam_debug_front_end_counts reports as computed, how many ran on the engine's auxiliary stream
 * behind such a sweep -- the selection and the range pass both, beside the fusion launch, so that a dslam_get_image that takes
 * the result runs the ray march alone -- and how many ran inside the fusion launch.  The first way is taken by a
 * dslam_process_frame whose sweep took the auxiliary stream (above) and that computes a front end at all;
 * DSLAM_OVERLAP_FRONT=0 in the environment of dslam_engine_create selects the second way always, and so do
 * DSLAM_OVERLAP_SWEEP=0 and DSLAM_OVERLAP_MARK=0.  Both ways compute the same bytes. */
int dslam_debug_front_overlap_counts(dslam_engine *e, long long *on_aux_out, long long *in_launch_out);
/* Test hook: a one-thread kernel reports the given device-side error bits for the scene (1: allocation ray longer than the
 * order key encodes, 2: a tile count never arrived) exactly as a failing pass would (report_error, csrc/dslam_device.h), so
 * that the way such an error reaches the caller can be tested: returned by this very call on a synchronous engine, by the
 * next call that waits for the stream on an asynchronous one -- once --, and by dslam_get_stats of that scene until it is
 * reset. */
int dslam_debug_inject_device_error(dslam_engine *e, dslam_scene *s, int bits);

/* ---- scene ------------------------------------------------------------------------------------- */
/* new ITMScene(sceneParams, useSwapping, memoryType) + ResetScene.  ext_voxel_blocks_dev may be NULL
 * (library allocates) or a caller-owned device buffer of num_local_blocks*512*8 bytes (e.g. a torch
 * tensor used as the RCCL all-gather buffer).  DSLAM_ERR_INVALID, before anything is allocated: num_local_blocks above
 * DSLAM_MAX_LOCAL_BLOCKS (with either kind of pool), or the parameters the error message names. */
int dslam_scene_create(dslam_engine *e, const dslam_scene_params *p, void *ext_voxel_blocks_dev,
                       dslam_scene **out);
int dslam_scene_destroy(dslam_scene *s);
/* denseMapper->ResetScene(scene)  (InfiniTamDriver.h:354-360). */
int dslam_scene_reset(dslam_engine *e, dslam_scene *s);
int dslam_scene_get_params(const dslam_scene *s, dslam_scene_params *out);

/* ---- render state / view ----------------------------------------------------------------------- */
/* visualisationEngine->CreateRenderState(imgSize) */
int dslam_render_state_create(dslam_engine *e, const dslam_scene *s, int width, int height,
                              dslam_render_state **out);
int dslam_render_state_destroy(dslam_render_state *r);
int dslam_view_create(dslam_engine *e, int width_rgb, int height_rgb, int width_d, int height_d,
                      dslam_view **out);
int dslam_view_destroy(dslam_view *v);

/* viewBuilder->UpdateView(&view, rgb, rawDepth, timestamp, useBilateralFilter)
 * (InfiniTamDriver.cpp:280-288).  rgba: Vector4u per pixel as written by CvToItm (:84-103);
 * depth_mm: int16 millimetres (:106-110); depth_m = d<=0 ? -1 : d*affine_a + affine_b with
 * (a,b) = (1/1000, 0) from CreateItmCalib (:58,79).
 * use_bilateral_filter: ITMViewBuilder's five passes of the 5x5 bilateral depth filter (upstream InfiniTAM v2
 * filterDepth); the filtered image keeps upstream's 2-pixel border of 0 (= no measurement).  A depth image below
 * 5 x 5 has no pixel the filter could write: with the filter on, every update entry point refuses such a view
 * with an error (the next update without the filter is served as usual). */
int dslam_view_update(dslam_engine *e, dslam_view *v, const uint8_t *rgba_host, const int16_t *depth_mm_host,
                      float affine_a, float affine_b, double timestamp, int use_bilateral_filter);
/* same, inputs already resident in HBM (frame database kept on device). */
int dslam_view_update_device(dslam_engine *e, dslam_view *v, const void *rgba_dev, const void *depth_mm_dev,
                             float affine_a, float affine_b, double timestamp, int use_bilateral_filter);

/* CvToItm(const cv::Mat3b&, ITMUChar4Image*) fused into UpdateView (InfiniTamDriver.cpp:84-103, 280-288): the
 * colour image arrives as OpenCV packed BGR (3 bytes per pixel, rows contiguous) and is converted to RGBA with
 * a = 255 on the device.  The _device variant needs a 4-byte aligned image. */
int dslam_view_update_bgr(dslam_engine *e, dslam_view *v, const uint8_t *bgr_host, const int16_t *depth_mm_host,
                          float affine_a, float affine_b, double timestamp, int use_bilateral_filter);
int dslam_view_update_bgr_device(dslam_engine *e, dslam_view *v, const void *bgr_dev, const void *depth_mm_dev,
                                 float affine_a, float affine_b, double timestamp, int use_bilateral_filter);
/* Dataset wire formats either side of the path, converted on the device.
 * Input: the per-pixel loop of PrecomputedDepthProvider::ReadPrecomputed on the 16-bit depth image as stored by the
 * datasets (PrecomputedDepthProvider.cpp:30-64): KITTI-style maps hold depth * 256 (values above max_depth_m * 256
 * are dropped, then int16 mm = (int16)((float)v * (1000 / 256))), TUM / ICL-NUIM maps are divided by 5.0 and
 * dropped above (int16)round(max_depth_m * 1000).  The converted millimetre image then takes UpdateView's path.
 * colour_channels: 4 = RGBA as dslam_view_update, 3 = OpenCV BGR as dslam_view_update_bgr.  (A float -> int16
 * conversion that overflows is undefined in C; here it wraps like the x86 code the reference compiles to.) */
enum { DSLAM_DEPTH_MM = 0, DSLAM_DEPTH_KITTI_X256 = 1, DSLAM_DEPTH_RGBD_X5 = 2 };
int dslam_view_update_dataset(dslam_engine *e, dslam_view *v, const uint8_t *colour_host, int colour_channels,
                              const int16_t *depth_raw_host, int depth_format, float max_depth_m, float affine_a,
                              float affine_b, double timestamp, int use_bilateral_filter);
/* read-back of the view's raw millimetre image as the kernels see it (after the dataset conversion) */
int dslam_download_view_raw_depth(dslam_engine *e, const dslam_view *v, int16_t *out_mm);
/* Output: GetImage(FREECAMERA_DEPTH) followed by FloatDepthmapToShort (scale 1000, InfiniTamDriver.cpp:167-180) or
 * FloatDepthmapToInt16 (scale 256, the raycast-depth PNGs of DenseSlam::SaveRaycastDepth, InfiniTamDriver.cpp:188-
 * 200, DenseSlam.cpp:573-592): int16 = (int16)(depth_m * scale) per pixel, converted on the device, so half the
 * bytes cross PCIe and the host loop disappears. */
int dslam_get_depth_image_int16(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                                const float intrinsics[4], int scale, int16_t *out_host);
/* test / debug read-back of the view's RGBA image (what IntegrateIntoScene will read). */
int dslam_download_view_rgba(dslam_engine *e, const dslam_view *v, uint8_t *out_rgba);

/* ---- keyframe store --------------------------------------------------------------------------- */
/* The image payload of DenseSlam's mfusionFrameDataBase (fusionFrameInfo::rgbinfo / depthinfo, DenseSlam.h:431-433)
 * kept resident in HBM: `capacity` slots of one RGBA + one int16-millimetre depth image.  The
 * reference re-uploads every keyframe through UpdateView for each de-/re-integration (DenseSlam.cpp:389-403,
 * 420-422); with the store OnlineCorrection's UpdateView becomes dslam_view_update_from_store -- no copy at all.
 * Slot bookkeeping (timestamp -> slot) stays with the caller's std::map.  640x480: 1.8 MB per keyframe. */
typedef struct dslam_frame_store dslam_frame_store;
int dslam_frame_store_create(dslam_engine *e, int width_rgb, int height_rgb, int width_d, int height_d, int capacity,
                             dslam_frame_store **out);
int dslam_frame_store_destroy(dslam_frame_store *fs);
/* host images in (the same layouts as dslam_view_update / dslam_view_update_bgr) */
int dslam_frame_store_put(dslam_engine *e, dslam_frame_store *fs, int slot, const uint8_t *rgba_host,
                          const int16_t *depth_mm_host);
int dslam_frame_store_put_bgr(dslam_engine *e, dslam_frame_store *fs, int slot, const uint8_t *bgr_host,
                              const int16_t *depth_mm_host);
/* device-to-device from the view that was just fused (mfusionFrameDataBase insert, DenseSlam.cpp:196-208):
 * the keyframe never crosses PCIe a second time */
int dslam_frame_store_put_view(dslam_engine *e, dslam_frame_store *fs, int slot, const dslam_view *v);
int dslam_frame_store_get(dslam_engine *e, const dslam_frame_store *fs, int slot, uint8_t *rgba_out,
                          int16_t *depth_mm_out);
int dslam_frame_store_device_ptrs(const dslam_frame_store *fs, int slot, void **rgba_dev, void **depth_mm_dev);
/* static_scene_->UpdateView(currRGBInfo, currDepthInfo, timestamp) for a stored keyframe (DenseSlam.cpp:392,421):
 * the view reads the slot in place until its next update; overwriting the slot before that changes what it sees */
int dslam_view_update_from_store(dslam_engine *e, dslam_view *v, const dslam_frame_store *fs, int slot,
                                 float affine_a, float affine_b, double timestamp, int use_bilateral_filter);

/* The blocks a keyframe was fused into, kept with it (optional).  DeProcessFrame as the reference calls it has only the
 * frame and its old pose, so it first has to find the blocks again: a visible-list-only allocation pass at that pose (two
 * kernel launches over the depth image and the table) -- which in a re-integration batch is work every GPU repeats.  With
 * the list stored at fusion time, de-integration goes straight to the integration kernel:
 *   dslam_frame_store_enable_lists(e, fs, scene)            room for one list of num_local_blocks entries per slot; the
 *                                                           lists hold entry ids of THIS scene's table size, and every
 *                                                           call that reads one refuses a scene of another size
 *   dslam_frame_store_put_visible_list(e, fs, slot, s, r)   after ProcessFrame of that keyframe (fusion or re-fusion): the
 *                                                           render state's visible list with each entry's block position
 *   dslam_deprocess_frame_stored(e, s, v, fs, slot, M_d, ...)   the inverse update of DeProcessFrame on exactly those
 *                                                           blocks: an entry that no longer holds the same block (released
 *                                                           by decay / the window since, or re-used) is skipped
 * Semantics differ from dslam_deprocess_frame in WHICH blocks are visited (the keyframe's own, instead of whatever an
 * allocation pass at the old pose finds today, previous-list carry-over included), and the render state is left alone.
 * The view must hold the keyframe's images (dslam_view_update_from_store). */
int dslam_frame_store_enable_lists(dslam_engine *e, dslam_frame_store *fs, const dslam_scene *s);
int dslam_frame_store_put_visible_list(dslam_engine *e, dslam_frame_store *fs, int slot, const dslam_scene *s,
                                       const dslam_render_state *r);
int dslam_deprocess_frame_stored(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_frame_store *fs, int slot,
                                 const float M_d[16], const float intrinsics_d[4], const float M_rgb[16],
                                 const float intrinsics_rgb[4]);

/* The re-integration batch of DenseSlam::OnlineCorrection (DenseSlam.cpp:389-403: for every corrected keyframe
 * DeProcessFrame at its old pose, ProcessFrame at the new one), as ONE call.  Equal -- map, rings, free lists, render state,
 * stored lists: bit for bit -- to
 *   for k in 0 .. n-1:  dslam_view_update_from_store(v, fs, slots[k]);  dslam_deprocess_frame_stored(s, v, fs, slots[k], old_M[k]);
 *                       dslam_process_frame(s, v, r, new_M[k], is_defusion = 1);  dslam_frame_store_put_visible_list(fs, slots[k], s, r)
 * but run block-major: the n allocation passes first, then every voxel block the batch touches is loaded once, takes the
 * de- and re-updates of every keyframe that names it in keyframe order, and is stored once (csrc/integrate.hip).  The
 * keyframes' images and fusion-time visible lists must be in the store; poses are n x 16 floats (column-major world ->
 * camera), one camera (depth = colour).  Scenes with host swapping or stopIntegratingAtMaxW return DSLAM_ERR_UNSUPPORTED:
 * use the per-keyframe calls.  On a sharded scene (dslam_scene_set_shard) every rank runs the allocation passes and
 * updates its own blocks; the exchange is dslam_shard_dirty_plan / _pack / _unpack as for the per-keyframe calls.
 * n = 0 changes nothing and allocates the call's scratch buffers (a second copy of 32 stored lists, per-block operation
 * masks): a set-up call keeps those allocations out of the first batch.
 * Errors: every argument -- slots, stored lists, table sizes, invertible new poses, the order key's range -- is checked
 * before anything is changed, so DSLAM_ERR_INVALID / DSLAM_ERR_UNSUPPORTED leave scene, render state and store as they
 * were.  A HIP failure in mid-batch (DSLAM_ERR_HIP) does not: allocation passes may have run whose blocks were never de-
 * or re-integrated, i.e. the scene is UNDEFINED (neither the old nor the new map) and must be reset or restored; the
 * render state's visible list is re-derived by its next pass, and the keyframes of the interrupted chunk lose their
 * stored lists (dslam_frame_store_put_visible_list again after re-fusing them). */
int dslam_reintegrate_batch(dslam_engine *e, dslam_scene *s, dslam_view *v, dslam_render_state *r, dslam_frame_store *fs,
                            int n, const int32_t *slots, const float *old_M, const float *new_M, const float intr[4],
                            float affine_a, float affine_b);

/* what the last dslam_reintegrate_batch (its last chunk of <= 32 keyframes) worked on: the distinct voxel blocks it loaded, and
 * its block-operations -- (block, keyframe) pairs de-integrated or re-fused, the unit the block kernel's cost is quoted in */
int dslam_reintegrate_batch_stats(dslam_engine *e, const dslam_scene *s, int32_t *blocks_out, int32_t *block_operations_out);

/* DenseSlam::depthPostProcessing's pixel loop (DenseSlam.cpp:488-529): blanks (sets to 0) every pixel of the
 * current keyframe's depth whose reprojection into the previous keyframe disagrees with that keyframe's depth by
 * more than `filter_threshold` (relative) and which lies below row `filter_area * rows`
 * (PostPocessParams, VoxelDecayParams.h:38-46).  Tpc = prev_pose.inv() * curr_pose (DenseSlam.cpp:507), column-major
 * like every matrix of this ABI; intrinsics = (fx, fy, cx, cy) of projection_left_rgb_ (:436-439).  The reference
 * pairs `row` with cx/fx and `col` with cy/fy (:500-513); that pairing is reproduced.  curr is updated in place;
 * *count_out (optional) receives the reference's `count` (pixels compared).  Host variant: cv::Mat1s buffers;
 * device variant: frames resident in HBM (frame database on device). */
int dslam_depth_post_processing(dslam_engine *e, int16_t *curr_depth_mm_host, const int16_t *prev_depth_mm_host,
                                int width, int height, const float Tpc[16], const float intrinsics[4],
                                float filter_threshold, float filter_area, int *count_out);
int dslam_depth_post_processing_device(dslam_engine *e, void *curr_depth_mm_dev, const void *prev_depth_mm_dev,
                                       int width, int height, const float Tpc[16], const float intrinsics[4],
                                       float filter_threshold, float filter_area, int *count_out);

/* ---- fusion ------------------------------------------------------------------------------------ */
/* denseMapper->SetFusionWeightParams(...)  (InfiniTamDriver.h:189,196) */
int dslam_set_fusion_weight_params(dslam_engine *e, const dslam_weight_params *w);

/* sceneRecoEngine->AllocateSceneFromDepth(scene, view, trackingState, renderState, onlyUpdateVisibleList)
 * M_d = trackingState->pose_d->GetM() (world -> camera), InfiniTamDriver.h:173-178. */
int dslam_allocate_scene_from_depth(dslam_engine *e, dslam_scene *s, const dslam_view *v,
                                    dslam_render_state *r, const float M_d[16], const float intrinsics_d[4],
                                    int only_update_visible_list);
/* sceneRecoEngine->IntegrateIntoScene(scene, view, trackingState, renderState).
 * M_rgb = calib.trafo_rgb_to_depth.calib_inv * M_d (identity calib in the reference,
 * InfiniTamDriver.cpp:74-75); pass M_rgb = NULL for "same as M_d". */
int dslam_integrate_into_scene(dslam_engine *e, dslam_scene *s, const dslam_view *v,
                               const dslam_render_state *r, const float M_d[16],
                               const float intrinsics_d[4], const float M_rgb[16],
                               const float intrinsics_rgb[4]);
/* denseMapper->ProcessFrame(view, trackingState, scene, renderState, onlyUpdateVisibleList, isDefusion)
 * (InfiniTamDriver.h:187-192; DenseSlam.cpp:213,236,403): allocate + integrate, queue the frame's
 * visible list (fusion or defusion FIFO), then swap in/out when the scene was created with swapping. */
int dslam_process_frame(dslam_engine *e, dslam_scene *s, const dslam_view *v, dslam_render_state *r,
                        const float M_d[16], const float intrinsics_d[4], const float M_rgb[16],
                        const float intrinsics_rgb[4], int only_update_visible_list, int is_defusion);
/* denseMapper->DeProcessFrame(view, trackingState, scene, renderState)
 * (InfiniTamDriver.h:194-199; DenseSlam.cpp:393,425): visible-list-only pass at the old pose, then the
 * inverse running average. */
int dslam_deprocess_frame(dslam_engine *e, dslam_scene *s, const dslam_view *v, dslam_render_state *r,
                          const float M_d[16], const float intrinsics_d[4], const float M_rgb[16],
                          const float intrinsics_rgb[4]);

/* ---- map regularisation / sliding window (the "global consistency" memory path) ------------------ */
/* denseMapper->Decay(scene, renderState, maxWeight, minAge, forceAllVoxels) (InfiniTamDriver.h:274-282,
 * 315-331) and DecayDefusionPart (:284-292). */
int dslam_decay(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_weight, int min_age,
                int force_all_voxels);
int dslam_decay_defusion_part(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_weight,
                              int min_age, int force_all_voxels);
/* denseMapper->SlideWindow(scene, renderState, maxAge) (InfiniTamDriver.h:294-300) and
 * SlideWindowDefusionPart(scene, renderState, maxAge, maxSize) (:302-310). */
int dslam_slide_window(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_age);
int dslam_slide_window_defusion_part(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_age,
                                     int max_size);

/* ---- swapping ---------------------------------------------------------------------------------- */
/* ITMSwappingEngine::IntegrateGlobalIntoLocal(scene, renderState) */
int dslam_swap_in(dslam_engine *e, dslam_scene *s, dslam_render_state *r);
/* ITMSwappingEngine::SaveToGlobalMemory(scene, renderState): swap out blocks that left the view */
int dslam_swap_out(dslam_engine *e, dslam_scene *s, dslam_render_state *r);
/* Hansry's one-argument SaveToGlobalMemory(scene) (DenseSlam.h:248-251): flush every resident block */
int dslam_save_to_global_memory(dslam_engine *e, dslam_scene *s);

/* ---- visualisation / raycast ------------------------------------------------------------------- */
/* visualisationEngine->FindVisibleBlocks(scene, pose, intrinsics, renderState) */
int dslam_find_visible_blocks(dslam_engine *e, const dslam_scene *s, dslam_render_state *r,
                              const float M[16], const float intrinsics[4]);
/* visualisationEngine->CountVisibleBlocks(scene, renderState, minBlockId, maxBlockId)
 * (mapManager->countVisibleBlocks, DenseSlam.cpp:555-556) */
int dslam_count_visible_blocks(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r,
                               int min_block_id, int max_block_id, int *out_count);
/* visualisationEngine->CreateExpectedDepths(scene, pose, intrinsics, renderState) */
int dslam_create_expected_depths(dslam_engine *e, const dslam_scene *s, dslam_render_state *r,
                                 const float M[16], const float intrinsics[4]);
/* visualisationEngine->RenderImage(scene, pose, intrinsics, renderState, outputImage, type): raycast
 * with the render state's range image, then shade.  Exactly one of out_rgba_host (Vector4u per pixel)
 * / out_float_host (float per pixel, DSLAM_IMAGE_DEPTH only) may be non-NULL; both NULL leaves the
 * result on the device (dslam_render_state_image_dev). */
int dslam_render_image(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                       const float intrinsics[4], int image_type, uint8_t *out_rgba_host,
                       float *out_float_host);
/* ITMMainEngine::GetImage(out, outFloat, type, pose, intrinsics, localMap) for the FREECAMERA_* types
 * (InfiniTamDriver.cpp:229-277): FindVisibleBlocks + CreateExpectedDepths + RenderImage.
 * Two things the caller gets for free: (1) the render state remembers the view (map version, pose, intrinsics) its
 * raycast result belongs to, so a second image type of the same view -- the GUI's depth + colour pair per tick,
 * DenseSlam.h:146-164 -- is only shaded; any call that can change the map or the render state drops that memo (maps
 * over caller-owned voxel memory are never memoised); (2) an output image inside a dslam_host_alloc buffer is written
 * by the render kernel itself instead of by a copy queued behind it. */
int dslam_get_image(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                    const float intrinsics[4], int image_type, uint8_t *out_rgba_host,
                    float *out_float_host);
/* A view of the whole reconstruction: every local map of the map graph in one raycast, each read through its
 * estimatedGlobalPose.  The reference creates local maps (createNewLocalMap, DenseSlam.cpp:133-141; shouldStartNewLocalMap,
 * :260-261, :554-565) and counts them in the GUI (DenseSLAMGUI.cpp:290), but every preview draws currentLocalMap only
 * (DenseSlam.h:146-164, InfiniTamDriver.cpp:229-277) and the export writes one mesh per map (SystemEntry.cpp:365-369).
 * scenes[i] is seen through T_map_from_world[16 i .. 16 i + 15] (column-major, metres: the Tdw = estimatedGlobalPose.GetM()
 * of DenseSlam.cpp:190, 577-579), i.e. from the camera M T_i^-1.  Every read of the march at a world point p goes to each
 * map whose blocks project into p's 8x8 tile, at T_i p; the maps that hold the voxel are combined: one -> its value
 * unchanged, several -> sum(w_i v_i) / sum(w_i) in list order, w = w_depth (sdf, normal) or w_color (colour), trilinear
 * where the read is.  A list of one map at the identity draws exactly what dslam_get_image draws.
 * Same image types, outputs (host, dslam_host_alloc, both NULL: the device image) and async behaviour as dslam_get_image;
 * the render-tile budget (MAX_RENDERING_BLOCKS) is not applied.  The render state's visible list is not touched; its
 * GetImage memo is dropped.  DSLAM_ERR_INVALID: num_maps outside 1 .. DSLAM_MAX_RENDER_MAPS, a NULL scene, a scene of
 * another engine or with another voxel_size / mu than scenes[0], a singular M or T_i, or a scene whose num_local_blocks
 * exceeds the render state's visible-list capacity. */
int dslam_get_image_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world,
                          int num_maps, dslam_render_state *r, const float M[16], const float intrinsics[4],
                          int image_type, uint8_t *out_rgba_host, float *out_float_host);
/* trackingController->Prepare(trackingState, scene, view, renderState) (InfiniTamDriver.h:208-220):
 * CreateExpectedDepths + CreateICPMaps from the render state's own visible list.  Outputs are
 * Vector4f per pixel (points: metres, world frame, w = 1 or -1; normals: w = 0 or -1); may be NULL. */
int dslam_create_icp_maps(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float M[16],
                          const float intrinsics[4], float *out_points_host, float *out_normals_host);
/* ITMMainEngine::GetImage(out, NULL, InfiniTAM_IMAGE_SCENERAYCAST, ...) = PreviewType::kRaycastImage
 * (InfiniTamDriver.cpp:28-29), the GUI's default rgb preview (DenseSLAMGUI.h:240): a copy of renderState->raycastImage,
 * the grey rendering upstream's CreateICPMaps draws with the ICP maps (processPixelICP -> drawPixelGrey: all four
 * channels (uchar)((0.8 angle + 0.2) 255) with the image-space normal, 0 where the ray found nothing), i.e. what
 * dslam_create_icp_maps (PrepareNextStepLocalMap, InfiniTamDriver.h:208-220) last left in this render state.
 * Vector4u per pixel.  DSLAM_ERR_INVALID before the first dslam_create_icp_maps (upstream: a zero image -- the
 * mirror's GetImage returns that). */
int dslam_download_raycast_image(dslam_engine *e, const dslam_render_state *r, uint8_t *out_rgba_host);

/* ---- meshing export ---------------------------------------------------------------------------- */
/* ITMMainEngine::SaveCurrSceneToMesh(objFileName, scene) -> ITMMeshingEngine::MeshScene(mesh, scene) (DenseSlam.cpp:
 * 638-643): marching cubes over every allocated voxel block, in upstream's CPU-engine order (hash
 * entries ascending, voxels z/y/x, triangles in case-table order), so the output is deterministic.  A cube is
 * skipped when one of its 8 corner voxels is missing or has sdf == 1 (findPointNeighbors).  max_triangles <= 0
 * selects ITMMesh's noMaxTriangles = num_local_blocks * 32; like upstream the list saturates at max_triangles - 1.
 * The mesh stays on the device until dslam_mesh_download: per triangle 3 vertices x (x, y, z) floats in metres
 * (world frame), and with with_colour the voxel colours interpolated to the same crossings, as (r, g, b) floats
 * in [0, 1] (the coloured-OBJ form of the DynSLAM lineage; upstream v2 writes positions only). */
int dslam_mesh_scene(dslam_engine *e, const dslam_scene *s, int max_triangles, int with_colour,
                     int *out_num_triangles);
int dslam_mesh_download(dslam_engine *e, float *out_positions_host, float *out_colours_host,
                        int capacity_triangles);

/* One mesh of the whole reconstruction: every local map of the map graph, each under its estimatedGlobalPose, in one
 * triangle list in the world frame (metres).  The reference writes one mesh-<n>-frames.obj per local map, each in its
 * own coordinates (SystemEntry.cpp:364-370, DenseSlam.cpp:638-643); loaded together they lie on top of each other at the
 * origin, and posed by hand they show two or three surfaces wherever maps overlap.  scenes / T_map_from_world are exactly as
 * in dslam_get_image_multi (column-major, metres, world -> map).  The law is this project's own.
 * With T~_i = T_i with its translation in voxel units, A_ij = T~_j T~_i^-1 (voxels of map i -> voxels of map j) and
 * B_i = T~_i^-1, both computed on the host in double from the float inputs and rounded to float32 (A_ij is exactly the
 * identity when T_i and T_j are bit-identical): for every allocated block of map i and every cube of it with corner 0 at
 * the integer voxel g of map i
 *   1. own gate: the cube is skipped when one of its 8 corner voxels of map i is missing or has sdf == 1 (as
 *      dslam_mesh_scene);
 *   2. coverage gate: ... or when an earlier map j < i holds a valid voxel (resident block, w_depth > 0, raw sdf != 32767)
 *      at iround(A_ij (g + 1/2)): earlier maps own overlapped space, later maps fill only what is left;
 *   3. corner values, one per lattice point of map i (every cube sharing the point sees the same value, so the mesh of one
 *      map stays watertight): the contributors are combined in list order, map i at its own position.  Own map: the
 *      voxel's sdf with weight w_depth (colour: the voxel's colour with weight w_color).  Every other map j: the
 *      trilinear read at A_ij (g + corner) exactly as dslam_get_image_multi's (found = any of the 8 taps in a resident
 *      block, weight = trilinear w_depth; colour: the trilinear colour on the 0 .. 255 scale with the trilinear w_color).
 *      Only the own map found -> its value unchanged, bit for bit; several -> sum(w v) / sum(w), accumulated in float32
 *      in list order; sum(w) == 0 -> the own map's value;
 *   4. triangles: case index from the combined values (< 0), zero crossings and case table as dslam_mesh_scene in map-i
 *      voxel coordinates; each vertex v leaves as (B_i v) * voxel_size, rows evaluated as ((a x + b y) + c z) + d (a T_i
 *      that is exactly the identity skips the transform).
 * So a list of one identity map is dslam_mesh_scene bit for bit, maps that do not reach each other give the concatenation
 * of their posed meshes, and where maps overlap there is one surface at the weighted consensus.  Seams between maps are
 * NOT stitched: along the edge of a later map's contribution a crack of up to about one voxel is accepted, and within a
 * voxel of a map's block edge, where another map's read finds only part of its taps (the missing ones read as sdf 1),
 * the surface is drawn up to 0.21 mu behind its place.
 * Triangle order: the triangles of map 0, then map 1, ...; inside a map dslam_mesh_scene's order.  out_map_triangles
 * ([num_maps] or NULL): the triangles map i contributed after saturation; they sum to *out_num_triangles.
 * max_triangles <= 0 selects the sum of num_local_blocks * 32 over the list (clamped to INT_MAX); the list saturates at
 * max_triangles - 1.  The mesh stays on the device until dslam_mesh_download; a later dslam_mesh_scene replaces it.  The
 * maps are only read.  Waits for the stream as dslam_mesh_scene does, on synchronous and asynchronous engines.
 * DSLAM_ERR_INVALID (the engine's previous mesh stays as it was): num_maps outside 1 .. DSLAM_MAX_RENDER_MAPS, a NULL
 * scene, a scene of another engine or with another voxel_size / mu than scenes[0], a singular T_i, NULL
 * out_num_triangles. */
int dslam_mesh_scene_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world,
                           int num_maps, int max_triangles, int with_colour, int *out_num_triangles,
                           int32_t *out_map_triangles);

/* ---- map registration ------------------------------------------------------------------------- */
/* SDF-to-SDF alignment of two overlapping local maps (no counterpart in the reference, whose map-to-map constraints come
 * from frames tracked in two maps at once; the law is this project's own).  X is the rigid transform
 * from the source map's frame to the destination map's (metres, column-major; for maps with world -> map transforms T_src,
 * T_dst it is T_dst T_src^-1); X~ is X with its translation in voxel units, kept in double on the host and rounded to
 * float32 (first three rows) for each evaluation.  One evaluation at X~: every voxel of every resident block of the
 * source, at integer voxel position p with fields (sdf_s, w_s),
 *   1. candidate gate: w_s > 0 and |sdf_s| < (int)(band * 32767); candidates are counted in N;
 *   2. q = X~ p, rows evaluated as ((a x + b y) + c z) + d in float32 (an X that is exactly the identity reads at p
 *      itself); cell floor(q), fractions c = q - floor(q);
 *   3. destination gate: all 8 taps of the cell lie in resident blocks of the destination, each with w_depth > 0 and a
 *      raw sdf other than +-32767; otherwise the voxel is a miss;
 *   4. value and gradient from those 8 taps, float32, s[k] = raw[k] / 32767 with tap k = (k & 1, (k >> 1) & 1, k >> 2),
 *      u = 1 - c per axis:
 *        x00 = ux s0 + cx s1, x10 = ux s2 + cx s3, x01 = ux s4 + cx s5, x11 = ux s6 + cx s7,
 *        y0 = uy x00 + cy x10, y1 = uy x01 + cy x11, d = uz y0 + cz y1,
 *        gx = uz (uy (s1 - s0) + cy (s3 - s2)) + cz (uy (s5 - s4) + cy (s7 - s6)),
 *        gy = uz (x10 - x00) + cz (x11 - x01), gz = y1 - y0;
 *   5. b = sdf_s / 32767 - d; |b| > residual_gate is a miss too; otherwise the voxel is valid with the row
 *      A = [q x g, g] (rotation about the destination's origin, then translation);
 *   6. 33 sums, accumulated in double from float32 products: [0..20] the lower triangle of sum A^T A row by row,
 *      [21..26] sum b A, [27] sum b^2, [28] the valid count, [29..31] sum q over the valid voxels, [32] N.
 * cost = (sum b^2 + (N - valid) residual_gate^2) / N: every miss pays the gate, so the cost cannot fall by shedding
 * overlap.  Iteration (host, double): the sums are re-pivoted to the centroid c = sum q / valid (H_c = P H P^T, g_c = P g,
 * P = [[I, -[c]x], [0, I]]); the step solves (H_c + lambda diag H_c) y = g_c and is applied on the left of X~ as
 * q' = c + R(y0..2)(q - c) + y3..5; it is accepted when the new evaluation has valid >= min_valid and a lower cost.
 * lambda starts at 1, is divided by 10 (not below 1e-6) on acceptance and multiplied by 10 on rejection.
 * stop_reason: 0 an accepted step taken with lambda <= 1 had |rotation| < term_rotation and |translation| <
 * term_translation_voxels; 1 max_evaluations reached (max_evaluations = 1: the start pose is evaluated once and returned);
 * 2 lambda > 1e6; 3 fewer than min_valid valid voxels at the start pose.  On every stop reason X returns the last
 * accepted pose (untouched if no step was accepted).  conditioning: the smallest eigenvalue of D^-1/2 H_c D^-1/2,
 * D = diag H_c, at the last accepted evaluation (0 if a diagonal entry is 0 or stop_reason is 3): small when the geometry
 * does not fix all six freedoms; the call never refuses on it.
 * Both maps are only read (blocks that are swapped out are simply not resident); no render state is involved.  Waits for
 * the stream on synchronous and asynchronous engines, as dslam_track_camera does.  DSLAM_ERR_INVALID with X untouched: a
 * NULL argument other than params, a scene of another engine, different voxel_size / mu, a non-finite or singular X, a
 * negative parameter. */
typedef struct {
  float band;                      /* 0 -> 0.5 */
  float residual_gate;             /* 0 -> 0.75 */
  int32_t max_evaluations;         /* 0 -> 30 */
  int32_t min_valid;               /* 0 -> 500 */
  float term_rotation;             /* radians; 0 -> 1e-5 */
  float term_translation_voxels;   /* 0 -> 1e-3 */
} dslam_register_params;
typedef struct {
  int32_t evaluations;
  int32_t stop_reason;
  int32_t candidates;              /* N */
  int32_t valid_last;              /* valid voxels at the returned pose */
  float cost_first;                /* cost at the start pose */
  float cost_last;                 /* cost at the returned pose */
  float conditioning;
  int32_t pad;
} dslam_register_result;
int dslam_register_maps(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst,
                        float X_dst_from_src[16] /* in: start, out: estimate */,
                        const dslam_register_params *params /* NULL: defaults */, dslam_register_result *result);
/* Test hook: the 33 raw sums (pivot at the origin) of the engine's most recent evaluation.  Error if none has run. */
int dslam_debug_register_sums(dslam_engine *e, double out[33]);

/* Joint alignment of N local maps from a list of overlapping pairs (no counterpart in the reference; the law is this
 * project's own).  T_i: world -> map i, metres, column-major (estimatedGlobalPose.GetM()); pairs:
 * (src, dst) indices into the map list, map src read as dslam_register_maps' source against map dst; `anchor`: the map
 * whose T is held fixed.  T~_i is T_i in double with its translation in voxels (3 x 4, kept by the host through the run).
 *   pair transform  X~_p = T~_d inv(T~_s) in double, inv = (R^T, -(R^T t)) and the product both with every sum evaluated
 *                   left to right (the mirror's RigidInverse / RigidProduct); its 12 entries are rounded to float32;
 *   one evaluation  every pair gets items 1 - 6 of dslam_register_maps at its X~_p, unchanged: 33 sums per pair.  One
 *                   kernel launch and one wait for the stream, however many pairs;
 *   active pairs    valid >= min_valid at the start poses; the others are reported and then left out of everything;
 *   cost            sum over active pairs of (sum b^2 + (N_p - valid_p) gate^2), divided by the sum of their N_p;
 *   linearisation   map i moves by a left increment about a pivot c_i in its own voxel frame, T~_i' = Inc(y_i, c_i) T~_i
 *                   (Inc: dslam_register_maps' step), so X~' = Inc_d X~ Inc_s^-1.  With H_p, g_p the pair's 6 x 6 and
 *                   6-vector at the origin, P(c) = [[I, -[c]x], [0, I]] and Ad(X) = [[R, 0], [[t]x R, R]] (X~ in double,
 *                   before rounding): J_d = P(c_d), J_s = -P(c_s) Ad(X~)^T; the pair adds J_a H_p J_b^T to block (a, b)
 *                   and J_a g_p to block a, for a, b in {s, d};
 *   pivots          c_i = (sum over active pairs with d = i of sum q + sum over active pairs with s = i of
 *                   valid_p X~_p^-1 (sum q / valid_p)) / (the sum of valid_p over those pairs); 0 if there is none;
 *   step            the anchor's rows and columns are removed; (H + lambda diag H) y = g over the 6 (N - 1) unknowns,
 *                   an unknown whose diagonal entry is not positive left out; applied to every free map;
 *   acceptance      the new evaluation has a lower cost and every active pair still has valid >= min_valid;
 *   lambda, stop reasons 0 - 2: dslam_register_maps', the termination test on the largest |rotation| and the largest
 *                   |translation| over the free maps;  stop reason 3: the active pairs do not connect every map to the
 *                   anchor -- no step is attempted;
 *   conditioning    the smallest eigenvalue of D^-1/2 H D^-1/2 of the reduced matrix at the last accepted evaluation (0
 *                   if a diagonal entry is not positive, or on stop reason 3).
 * On every stop reason the T_i return the last accepted poses (rotation rounded to float32, translation times voxel_size,
 * then rounded); untouched, byte for byte, if no step was accepted; the anchor's T is never written.  Two maps, the pair
 * (0, 1), anchor 0 and T_0 the identity is dslam_register_maps(src 0, dst 1, X = T_1), step for step.
 * All maps are only read (blocks that are swapped out are simply not resident).  Waits for the stream on synchronous and
 * asynchronous engines.  DSLAM_ERR_INVALID with every T untouched: a NULL argument other than params or pair_results,
 * num_maps outside 2 .. DSLAM_MAX_RENDER_MAPS, num_pairs outside 1 .. DSLAM_MAX_REGISTER_PAIRS, an index out of range,
 * src == dst, an ordered pair given twice, a scene listed twice, a scene of another engine, voxel_size or mu that differ
 * bitwise between two maps, a non-finite T or one whose rotation block is not orthonormal to 1e-4, a negative parameter. */
#define DSLAM_MAX_REGISTER_PAIRS 128
typedef struct {
  int32_t evaluations;
  int32_t stop_reason;
  int32_t active_pairs;
  float cost_first;                /* cost at the start poses */
  float cost_last;                 /* cost at the returned poses */
  float conditioning;
} dslam_register_graph_result;
typedef struct {
  int32_t candidates;              /* N_p */
  int32_t valid_first;             /* valid voxels at the start poses */
  int32_t valid_last;              /* ... at the returned poses (an inactive pair: valid_first) */
  int32_t active;
  float cost_first;                /* the pair's own (sum b^2 + misses gate^2) / N_p at the start poses */
  float cost_last;                 /* ... at the returned poses */
} dslam_register_pair_result;
int dslam_register_graph(dslam_engine *e, const dslam_scene *const *scenes,
                         float *T_map_from_world /* [num_maps][16]; in: start, out: estimate */, int num_maps,
                         const int32_t *pairs /* [num_pairs][2] = (src, dst) */, int num_pairs, int anchor,
                         const dslam_register_params *params /* NULL: defaults */, dslam_register_graph_result *result,
                         dslam_register_pair_result *pair_results /* [num_pairs], may be NULL */);
/* Test hook: the 33 raw sums (pivot at the origin) of pair `pair` at the engine's most recent joint evaluation (a pair
 * that was not active: at the first).  Error if no dslam_register_graph has run or the index is out of range. */
int dslam_debug_register_graph_sums(dslam_engine *e, int pair, double out[33]);

/* Which local maps overlap: a survey of all N (N - 1) ordered pairs at block granularity (no counterpart in the
 * reference; the law is this project's own).  It reads only the hash tables, never a voxel, and
 * produces what dslam_register_graph cannot: the evidence for its list of overlapping pairs.  T_i: world -> map i, metres,
 * column-major, exactly as dslam_register_graph takes them.
 *   pair transform  for every ordered pair (s, d), s != d: X~_sd = T~_d inv(T~_s), dslam_register_graph's pair transform
 *                   (double, translation in voxel units, the sums of inverse and product evaluated left to right, the
 *                   12 entries rounded to float32);
 *   live blocks     live[s] = the hash entries of map s with ptr >= 0: resident blocks (a swapped-out block is not);
 *   octant centres  a resident block of s at block position B (the entry's three shorts) has 8 octants o = (ox, oy, oz)
 *                   in {0, 1}^3 with centres c = 8 B + (1.5 + 4 ox, 1.5 + 4 oy, 1.5 + 4 oz), exact in float32;
 *   transform       q = X~_sd c, each row evaluated as ((a x + b y) + c z) + d in float32 without contraction; an X~_sd
 *                   that rounds to the identity reads at c itself;
 *   destination     cell = (int)floorf(q) per axis, D = cell >> 3 (floor division, not truncation);
 *   shared octant   every component of D lies in [-32768, 32767] and map d holds a resident entry (ptr >= 0) at D, found
 *                   by the ordinary lookup: the bucket of D's hash, then its excess chain.  A q too large for an int, or
 *                   not a number, is not shared;
 *   shared_octants[s][d]  the shared octants over all resident blocks of s;
 *   shared_blocks[s][d]   the resident blocks of s with at least one shared octant;
 *   the diagonal    shared_octants[s][s] = 8 live[s], shared_blocks[s][s] = live[s], by definition (nothing is probed).
 * All outputs are integers: exact, and the same on every run.  Both matrices are [N][N] with the source as the row.
 * Every map is only read; no render state is involved.  Waits for the stream on synchronous and asynchronous engines.
 * DSLAM_ERR_INVALID with the outputs untouched: a NULL argument other than shared_blocks_out, num_maps outside
 * 2 .. DSLAM_MAX_RENDER_MAPS, a scene listed twice, a scene of another engine, voxel_size or mu that differ bitwise
 * between two maps, a non-finite T or one whose rotation block is not orthonormal to 1e-4. */
int dslam_survey_overlaps(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                          int32_t *live_blocks_out /* [N] */,
                          int32_t *shared_blocks_out /* [N][N], row = source; may be NULL */,
                          int32_t *shared_octants_out /* [N][N], row = source */);

/* From a survey to a pair list dslam_register_graph accepts.  A pure host function: no engine, no device.
 *   1. qualifying   the ordered pairs (s, d), s != d, with shared_octants[s][d] >= min_shared_octants;
 *   2. one_direction != 0: of an unordered pair {a < b} whose two directions both qualify only one is kept, the one
 *      whose source is covered more -- shared[s][d] / (8 live[s]), compared exactly as shared[a][b] live[b] against
 *      shared[b][a] live[a] in 64-bit integers; a tie keeps (a, b).  A pair with one qualifying direction keeps it;
 *   3. components   the maps joined by the qualifying pairs, undirected: component_out[i] is the smallest index in map
 *      i's component, num_components their number;
 *   4. the cap      the kept pairs ordered by shared_octants descending, ties by (s, d) ascending.  Pass 1 takes, in that
 *      order, every pair that joins two sets of a union-find over the maps; pass 2 takes the others in that order until
 *      max_pairs pairs are taken.  So the cap never disconnects what step 3 connected;
 *   5. pairs_out    the selected pairs by (s, d) ascending (entries past `selected` are not written); qualifying = the
 *      pairs kept after step 2, before the cap; selected = the pairs in pairs_out.
 * min_shared_octants is a coarse prefilter in units of octants (64 octants = 8 blocks' worth), not a measurement:
 * dslam_register_graph's own min_valid remains the gate on what a pair contributes.
 * DSLAM_ERR_INVALID with the outputs untouched: a NULL argument other than params, num_maps outside
 * 2 .. DSLAM_MAX_RENDER_MAPS, a negative parameter, max_pairs above DSLAM_MAX_REGISTER_PAIRS or below num_maps - 1. */
typedef struct {
  int32_t min_shared_octants;      /* 0 -> 64 */
  int32_t one_direction;
  int32_t max_pairs;               /* 0 -> DSLAM_MAX_REGISTER_PAIRS */
  int32_t pad;
} dslam_pair_select_params;
typedef struct {
  int32_t qualifying;
  int32_t selected;
  int32_t num_components;
  int32_t pad;
} dslam_pair_select_result;
int dslam_select_register_pairs(const int32_t *live_blocks /* [N] */, const int32_t *shared_octants /* [N][N] */,
                                int num_maps, const dslam_pair_select_params *params /* NULL: defaults */,
                                int32_t *pairs_out /* [max_pairs][2] */, int32_t *component_out /* [N] */,
                                dslam_pair_select_result *result);

/* ---- which local maps a camera view reaches (no counterpart in the reference) ---------------- */
#define DSLAM_MAX_SURVEY_MAPS 256
#define DSLAM_MAX_SURVEY_VIEWS 16
typedef struct {
  float M[16];                     /* world -> camera, metres, column-major (as pose_M of dslam_track_camera_sdf) */
  float intrinsics[4];             /* fx, fy, cx, cy */
  int32_t width, height;
  float near_m, far_m;             /* far_m == 0: no far plane */
} dslam_survey_view;
/* The frustum of a view as seven rows of four float32 in the world frame, in voxel units: rows 0..5 the inward unit-normal
 * planes left, right, top, bottom, near, far (a point p is inside when n . p + d >= 0), row 6 the camera's z row.  A pure
 * host function: no engine, no device.  Everything below is double; each of the 28 numbers is rounded to float32 once, at
 * the end.  R[r][c] = M[4 c + r], t[r] = M[12 + r], vs = voxel_size, each converted to double first.
 *   t~[r] = t[r] / vs;
 *   the image bounds are one pixel wider than the image, x from -1 to width, y from -1 to height, so the integer pixel
 *   coordinates of the tracker and the renderer lie strictly inside;
 *   camera-frame normals before scaling: left (fx, 0, cx + 1), right (-fx, 0, width - cx), top (0, fy, cy + 1),
 *   bottom (0, -fy, height - cy), where cx + 1, width - cx, cy + 1 and height - cy are formed in double; for each, with
 *   (a, b) its two non-zero entries in that order, len = sqrt(a a + b b) and the unit normal is (a / len, 0, b / len)
 *   (respectively (0, a / len, b / len)); their d_c is 0.  near: n_c = (0, 0, 1), d_c = -(near_m / vs).  far:
 *   n_c = (0, 0, -1), d_c = far_m / vs;
 *   world frame, for each of the six: n_w[j] = (R[0][j] n_c[0] + R[1][j] n_c[1]) + R[2][j] n_c[2] for j = 0, 1, 2 (all
 *   three products are formed, the zero ones included) and d_w = ((n_c[0] t~[0] + n_c[1] t~[1]) + n_c[2] t~[2]) + d_c;
 *   with far_m == 0 row 5 is (0, 0, 0, +INFINITY): it always passes;
 *   row 6 = (R[2][0], R[2][1], R[2][2], t~[2]).
 * DSLAM_ERR_INVALID with `out` untouched: a NULL argument, a non-finite entry of the view or voxel_size, a rotation block of
 * M that is not orthonormal to 1e-4, fx or fy <= 0, width or height < 1, near_m < 0, far_m < 0, 0 < far_m <= near_m,
 * voxel_size <= 0. */
int dslam_view_frustum_planes(const dslam_survey_view *view, float voxel_size, float out[28]);

/* Which of N local maps reach V camera views, at block granularity, from the hash tables alone (never a voxel).
 * T_i: world -> map i, metres, column-major, as the other multi-map calls take it.
 *   inverse pose    T~_i is T_i with its translation in voxel units; Y~_i = (R^T, -(R^T t)) is its rigid inverse, formed
 *                   in double (each translation entry -((r0 t0 + r1 t1) + r2 t2) with (r0, r1, r2) a column of R), its 12
 *                   entries rounded to float32 -- as dslam_merge_maps forms its Y~;
 *   resident block  a hash entry of map i with ptr >= 0; its block position B is the entry's three shorts, its centre
 *                   c = 8 B + 4, exact in float32;
 *   world point     p = Y~_i c, rows evaluated as ((a x + b y) + c z) + d in float32 without contraction; a T_i that is
 *                   exactly the identity reads at c itself;
 *   planes          the 28 floats of dslam_view_frustum_planes(view v, the maps' voxel_size); for rows k = 0..5
 *                   s_k = ((n_x p_x + n_y p_y) + n_z p_z) + d in float32;
 *   reach           the block reaches view v when s_k >= -rho for all six rows, rho = (float)(6.92820323027550917 +
 *                   (double)margin_voxels): 4 sqrt(3), the radius of the sphere around the block's cube
 *                   [8 B, 8 B + 8]^3, plus the margin.  A NaN s_k does not reach;
 *   depth           z = ((r20 p_x + r21 p_y) + r22 p_z) + t~_z from row 6, zi = (int)floorf(z) with floorf(z) first
 *                   clamped to [-2147483648, 2147483520] (both exact in float32), so the cast is always defined;
 *   live_blocks[i]      the resident entries of map i;
 *   reach_blocks[v][i]  its reaching blocks;
 *   nearest[v][i], farthest[v][i]  the minimum and the maximum of zi over the reaching blocks; INT32_MAX and INT32_MIN
 *                   when no block reaches.
 * All outputs are integers: exact, the same bytes on every run, and independent of how the work is split.
 * The six half-spaces, loosened by the block's radius, are conservative: a point inside the frustum lies in no block the
 * test rejects (DESIGN.md section 20 gives the float32 rounding bound the margin has to cover).  So a map with
 * reach_blocks[v][i] == 0 holds no resident block at any depth pixel of view v with near_m < D <= far_m, fails the
 * base-corner probe of dslam_track_camera_sdf at every such pixel, and can be dropped from that call's list without
 * changing a bit of its sums.  Nothing is promised about the images of dslam_get_image_multi: its range image lists
 * blocks by the bounding box of their projected corners, which can touch the image for a block that misses the frustum.
 * Every map is only read (a block that is swapped out is not resident); no render state is involved; no map's version,
 * GetImage memo or front-end record changes.  One kernel launch whatever N and V.  Waits for the stream on synchronous
 * and asynchronous engines.
 * DSLAM_ERR_INVALID with all outputs untouched: a NULL argument other than params, nearest_out or farthest_out, num_maps
 * outside 1 .. DSLAM_MAX_SURVEY_MAPS, num_views outside 1 .. DSLAM_MAX_SURVEY_VIEWS, a scene listed twice, a scene of
 * another engine, voxel_size or mu that differ between maps, a non-finite T_i or one whose rotation block is not
 * orthonormal to 1e-4, a view dslam_view_frustum_planes rejects, a negative or non-finite margin. */
typedef struct {
  float margin_voxels;             /* 0 -> 2.0 */
  int32_t pad[3];
} dslam_view_survey_params;
int dslam_survey_views(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                       const dslam_survey_view *views, int num_views, const dslam_view_survey_params *params /* NULL: defaults */,
                       int32_t *live_blocks_out /* [N] */, int32_t *reach_blocks_out /* [V][N] */,
                       int32_t *nearest_out /* [V][N]; may be NULL */, int32_t *farthest_out /* [V][N]; may be NULL */);
/* Test hook: the kernel launches all dslam_survey_views calls of this engine have enqueued so far (one per call). */
int dslam_debug_survey_views_launches(dslam_engine *e, long long *count_out);

/* From a view survey to a list of at most max_maps maps the multi-map calls accept.  A pure host function.
 *   candidates  the maps with max_v reach_blocks[v][i] >= min_blocks; always_keep, if >= 0, is a candidate regardless
 *               (the map being fused into stays listed even while it is empty); reaching = their number;
 *   the cap     with more than max_maps candidates: always_keep is taken first, then the candidates in the order of the
 *               smaller min_v nearest[v][i], ties to the larger sum_v reach_blocks[v][i] (64-bit), then to the smaller
 *               index, until max_maps are taken;
 *   maps_out    the taken indices ascending (entries past `selected` are not written), so a sub-list built from them
 *               keeps the list order the blend laws depend on; selected = their number.
 * DSLAM_ERR_INVALID with the outputs untouched: a NULL argument other than params, num_views outside
 * 1 .. DSLAM_MAX_SURVEY_VIEWS, num_maps outside 1 .. DSLAM_MAX_SURVEY_MAPS, a negative parameter other than
 * always_keep == -1 (pad counts as a parameter: it must not be negative), always_keep >= num_maps, max_maps above
 * DSLAM_MAX_RENDER_MAPS. */
typedef struct {
  int32_t min_blocks;              /* 0 -> 1 */
  int32_t max_maps;                /* 0 -> DSLAM_MAX_RENDER_MAPS */
  int32_t always_keep;             /* index, or -1 */
  int32_t pad;
} dslam_view_select_params;
typedef struct {
  int32_t reaching;
  int32_t selected;
} dslam_view_select_result;
int dslam_select_view_maps(const int32_t *reach_blocks /* [V][N] */, const int32_t *nearest /* [V][N] */, int num_views,
                           int num_maps, const dslam_view_select_params *params /* NULL: defaults */,
                           int32_t *maps_out /* [max_maps] */, dslam_view_select_result *result);

/* ---- the maps at any point or along any ray (no counterpart in the reference) ---------------
 * The posed, weighted cross-map reads of dslam_get_image_multi (the law of DESIGN.md section 10) without a camera: at
 * arbitrary world points, and along arbitrary rays.  scenes / T_map_from_world / num_maps as dslam_track_camera_sdf (1 ..
 * DSLAM_MAX_RENDER_MAPS scenes of one engine, none twice, one voxel_size and mu, rigid transforms).  Every listed map is
 * visited for every element, in list order; narrow the list with dslam_survey_views / dslam_select_view_maps.  The
 * scenes are only read, no render state is taken and no GetImage memo is touched.
 *
 * dslam_query_points: per world point p (metres) the combined trilinear sdf (1.0 where no map holds a tap of the cell),
 * `weight` = the law's sum of the weights of that read (the trilinear w_depth of every map that reported found, float32,
 * list order; 0 where none did), the combined un-normalised gradient in the world frame, the combined colour in 0 .. 1,
 * and in found_lo / found_hi bit i set when map i holds a tap of the cell.  status DSLAM_QUERY_OUTSIDE: a coordinate is
 * not finite or lies beyond +-2^20 voxels; no map is read, sdf is 1 and every other field 0.  `what`: DSLAM_QUERY_SDF,
 * optionally | DSLAM_QUERY_GRADIENT | DSLAM_QUERY_COLOUR; a field not asked for is written as 0, a field asked for carries
 * the same bits whatever else was asked.
 *
 * dslam_cast_rays: per ray (origin o, direction d of any length > 0, t_min, t_max; metres along the normalised
 * direction) the march of dslam_get_image_multi from o + t_min d^ to min(t_max, t_min + max_range).  max_range: metres,
 * 0 -> the limit DSLAM_QUERY_MAX_RAY_VOXELS x voxel_size, above the limit an error: a ray takes at most
 * DSLAM_QUERY_MAX_RAY_VOXELS iterations whatever its t_max.  status 0: a miss (t_min >= t_max: with steps 0); 1: a hit;
 * 2: a hit at the first read -- the ray began at or behind a surface, and `point` is where the march's two refinement
 * steps led from there; -1: an invalid ray (a component not finite, a direction of length 0 or not finite, t_min < 0,
 * the start beyond +-2^20 voxels), never marched, everything else 0.  At a hit: t = (point - o) . d^, point in world
 * metres, normal = the combined gradient at the hit point, normalised ((0, 0, 0) when its float32 length is exactly 0),
 * colour as dslam_query_points gives it there -- both are read at `point` taken back to voxel units as
 * dslam_query_points takes its points, so a later dslam_query_points at `point` returns the bits the ray carries.  `what`: DSLAM_QUERY_GRADIENT (normal) and DSLAM_QUERY_COLOUR select the shading;
 * DSLAM_QUERY_SDF is accepted and means nothing more.
 *
 * The host forms stage through buffers of the engine in chunks of 2^20 elements and return when the results are in
 * out_host.  The device forms (points_dev / rays_dev 4-byte aligned, out_dev 16-byte aligned, device memory) enqueue on the
 * engine's stream and return as every enqueue-only call does (dslam_engine_set_async).  n == 0 is DSLAM_OK.
 * DSLAM_ERR_INVALID: the map-list errors, n outside 0 .. DSLAM_QUERY_MAX_ELEMENTS, unknown bits in `what` (or no
 * DSLAM_QUERY_SDF for points), max_range negative, not finite or above the limit, a NULL array with n > 0. */
#define DSLAM_QUERY_MAX_ELEMENTS (1 << 24)
#define DSLAM_QUERY_MAX_RAY_VOXELS 16384
#define DSLAM_QUERY_SDF 1
#define DSLAM_QUERY_GRADIENT 2
#define DSLAM_QUERY_COLOUR 4
#define DSLAM_QUERY_OUTSIDE 1
typedef struct {
  float sdf, weight, grad[3], colour[3];
  uint32_t found_lo, found_hi;
  int32_t status, pad;
} dslam_point_sample; /* 48 bytes */
typedef struct {
  float t, point[3], normal[3], colour[3];
  int32_t status, steps;
} dslam_ray_hit; /* 48 bytes */
int dslam_query_points(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                       const float *points_host /* [n][3] */, int n, int what, dslam_point_sample *out_host);
int dslam_query_points_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                              const void *points_dev /* [n][3] float */, int n, int what, void *out_dev /* [n] dslam_point_sample */);
int dslam_cast_rays(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                    const float *rays_host /* [n][8]: o, d, t_min, t_max */, int n, float max_range, int what,
                    dslam_ray_hit *out_host);
int dslam_cast_rays_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                           const void *rays_dev /* [n][8] float */, int n, float max_range, int what,
                           void *out_dev /* [n] dslam_ray_hit */);

/* ---- occupancy and exact distance grids (no counterpart in the reference) --------------------
 * What a planner reads next to the truncated distances of dslam_query_points: over a world-aligned box of cells, which
 * cells the listed maps have observed, which hold a surface, and the exact Euclidean distance of every cell to the
 * nearest occupied (or never observed) cell.  Everything behind one float32 transform per voxel is integer arithmetic, so
 * the results are the same bits on every run and equal tests/ref_distance_field.py bit for bit.
 *
 * dslam_grid: the box in world VOXEL units.  origin: the world voxel coordinate of the low corner of cell (0, 0, 0); cell:
 * the edge of a cell in voxels, 1 .. DSLAM_GRID_MAX_CELL; dims: cells per axis, each 1 .. DSLAM_GRID_MAX_DIM, their
 * product at most DSLAM_GRID_MAX_CELLS; origin[a] >= -2^20 and origin[a] + cell * dims[a] <= 2^20; pad 0.  Every per-cell
 * array is x-fastest: cell (x, y, z) at index x + dims[0] * (y + dims[1] * z).  dslam_grid_from_box (host only) makes the
 * grid of cell edge `cell` that covers the metric box lo_m .. hi_m: origin = floor((double)lo / (double)voxel_size), dims =
 * max(1, ceil((hi / voxel_size - origin) / cell)); DSLAM_ERR_INVALID (and *out untouched) where a limit is exceeded, hi <
 * lo, or an input is not finite.
 *
 * dslam_mark_occupancy (law 1).  scenes / T_map_from_world / num_maps as dslam_query_points.  For every listed map i,
 * every hash entry with ptr >= 0 and each of its 512 voxels at integer position p of the map's own frame:
 *   1. w_depth >= min_weight (0 -> 1, else 1 .. 255), or the voxel is ignored;
 *   2. w = B_i p, B_i = float32(rigid_inverse(voxel_pose(T_i, (double)voxel_size))) (csrc/register_host.h, in double, the
 *      12 entries then rounded), p as float32, each row ((a x + b y) + c z) + d in float32 without contraction; a voxel
 *      with a coordinate of w not finite or |w| > 2^20 is ignored;
 *   3. g = (int)floorf(w) per axis, c = floor_div(g - origin, cell); a voxel whose c lies outside dims is ignored;
 *   4. the cell's byte gets DSLAM_CELL_OBSERVED, and DSLAM_CELL_OCCUPIED as well when (int16)sdf <= thr, thr =
 *      (int)floor((double)occupied_below / (double)mu * 32767.0); occupied_below: metres, |occupied_below| < mu, 0 = the
 *      shell behind the surface.
 * A cell's byte is the OR over all voxels of all maps that land in it: 0 unknown, 1 observed and free, 3 occupied -- so
 * the order of the list, and of anything else, does not matter.  Two consequences: with cell = 1 under a rotation not
 * every world cell of the shell receives a lattice point of the map (the shell is mu deep, so it stays closed; a caller
 * who needs every cell of it filled uses cell >= 2), and blocks that are swapped out (ptr == -1) are not resident and
 * mark nothing.
 *
 * dslam_distance_transform (law 2).  states: one byte per cell, of which bits 0 and 1 are read.  seeds:
 * DSLAM_SEED_OCCUPIED (byte & 2), DSLAM_SEED_UNKNOWN ((byte & 3) == 0), or both (either).  d2[c] = the smallest |c - s|^2
 * over the seed cells s, an exact integer.  max_cells R: 0 no bound; 1 .. DSLAM_DIST_MAX_CELLS: a cell with d2 > R^2 is
 * far (d2 == R^2 is kept).  A grid without a seed is far everywhere.  format DSLAM_DIST_SQUARED_CELLS: int32 d2, far =
 * DSLAM_DIST_FAR; DSLAM_DIST_METRES: float32 sqrtf((float)d2) * ((float)cell * voxel_size) (one correctly rounded root,
 * the cell size computed first), far = +inf; voxel_size is read for this format only (finite, > 0).
 *
 * dslam_distance_field: law 1, then law 2 on its states, without leaving the device; states_out and dist_out are each
 * optional, not both NULL.
 *
 * The host forms stage through buffers of the engine (grown on demand, released with it) and return when the results
 * are in the caller's arrays.  The device forms (states: bytes; distances: 4 bytes per cell; both 16-byte aligned device
 * memory) enqueue on the engine's stream and return as every enqueue-only call does (dslam_engine_set_async).  The scenes
 * are only read, no render state is taken and no GetImage memo is touched.  DSLAM_ERR_INVALID, with nothing written: the
 * map-list errors, a grid outside the limits or with pad != 0, min_weight outside 0 .. 255, occupied_below not finite or
 * |occupied_below| >= mu, seeds outside 1 .. 3, max_cells outside 0 .. DSLAM_DIST_MAX_CELLS, an unknown format, a NULL
 * array that is needed, a misaligned device pointer. */
#define DSLAM_GRID_MAX_CELL 64
#define DSLAM_GRID_MAX_DIM 1024
#define DSLAM_GRID_MAX_CELLS (1 << 26)
#define DSLAM_CELL_OBSERVED 1
#define DSLAM_CELL_OCCUPIED 2
#define DSLAM_SEED_OCCUPIED 1
#define DSLAM_SEED_UNKNOWN 2
#define DSLAM_DIST_SQUARED_CELLS 0
#define DSLAM_DIST_METRES 1
#define DSLAM_DIST_MAX_CELLS 1774
#define DSLAM_DIST_FAR 0x7fffffff
typedef struct { int32_t origin[3]; int32_t cell; int32_t dims[3]; int32_t pad; } dslam_grid; /* 32 bytes */
int dslam_grid_from_box(const float *lo_m /* [3] */, const float *hi_m /* [3] */, float voxel_size, int cell, dslam_grid *out);
int dslam_mark_occupancy(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                         const dslam_grid *grid, int min_weight, float occupied_below, uint8_t *states_out_host);
int dslam_mark_occupancy_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                                const dslam_grid *grid, int min_weight, float occupied_below, void *states_out_dev);
int dslam_distance_transform(dslam_engine *e, const dslam_grid *grid, const uint8_t *states_host, int seeds, int max_cells,
                             int format, float voxel_size, void *dist_out_host /* [cells] int32 or float */);
int dslam_distance_transform_device(dslam_engine *e, const dslam_grid *grid, const void *states_dev, int seeds, int max_cells,
                                    int format, float voxel_size, void *dist_out_dev);
int dslam_distance_field(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                         const dslam_grid *grid, int min_weight, float occupied_below, int seeds, int max_cells, int format,
                         uint8_t *states_out_host /* or NULL */, void *dist_out_host /* or NULL */);
int dslam_distance_field_device(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                                const dslam_grid *grid, int min_weight, float occupied_below, int seeds, int max_cells,
                                int format, void *states_out_dev /* or NULL */, void *dist_out_dev /* or NULL */);
/* bench hook: enable 1 / 0 switches events at the phase boundaries of the calls above on or off (-1: leaves it as it is);
 * out_ms (or NULL): waits for the stream, then the device time of the most recent call's phases -- [0] the packed states
 * (memset and k_df_mark, or the packing of the caller's bytes), [1] the x pass, [2] the y pass, [3] the last pass (or the
 * expansion of the states when no distance was asked for); -1 for a phase that did not run or was not timed */
int dslam_debug_distance_field_phases(dslam_engine *e, int enable, float out_ms[4]);

/* ---- semi-global stereo matching: a depth image from a rectified pair ------------------------
 * A handle is made for one image size W x H (1 .. 4096 each) and one parameter block and owns all working memory.  The law
 * is all-integer up to the depth conversion, so the device gives the same bytes as tests/ref_stereo.py.  D = max_disparity.
 *   grey         channels == 1: the byte as it is; channels == 4 (RGBA): (r + 2 g + b) >> 2.
 *   census       window 9 wide, 7 high, coordinates clamped to the image; 62 bits in a uint64: over the neighbours in
 *                row-major order (dy = -3 .. 3 outer, dx = -4 .. 4 inner, centre skipped) code = code << 1 | (neighbour <
 *                centre).
 *   cost         C(y, x, d) = popcount(censusL(y, x) ^ censusR(y, x - d)) for 0 <= d < D and x - d >= 0, otherwise
 *                DSLAM_STEREO_COST_OUT.
 *   aggregation  eight directions r = (dy, dx) in {(0, +-1), (+-1, 0), (+-1, +-1)}, q = p - r.  q outside the image:
 *                L_r(p, d) = C(p, d).  Otherwise with m = min_k L_r(q, k):  L_r(p, d) = C(p, d) + min(L_r(q, d),
 *                L_r(q, d - 1) + p1, L_r(q, d + 1) + p1, m + p2) - m, the d +- 1 terms absent at the ends of the range.
 *                S = the sum of the eight L_r (every L_r <= 63 + 192, S <= 2040).
 *   selection    d* = argmin_d S(y, x, d), the smallest d on ties; s0 = S(d*); s2 = min S(d) over |d - d*| > 1; with
 *                uniqueness u (percent) the pixel is rejected iff s2 (100 - u) < 100 s0.
 *   left-right   dR(y, xr) = argmin_d S(y, xr + d, d) over the d with xr + d < W, the smallest d on ties.  Rejected if
 *                x - d* < 0, and, unless the check is off, if |dR(y, x - d*) - d*| > lr_max.
 *   sub-pixel    sm = S(d* - 1), sp = S(d* + 1), den = sm + sp - 2 s0.  If 0 < d* < D - 1 and den > 0: delta =
 *                floor((16 (sm - sp) + den) / (2 den)), else 0.  d16 = 16 d* + delta (1/16 pixel), DSLAM_STEREO_INVALID
 *                where rejected.
 *   depth        float32, in this order: disp = d16 * 0.0625f; z = (focal_length_px * baseline_m) / disp; mm_f =
 *                (1000.0f * scale) * z; mm = (int32)mm_f.  0 where d16 is DSLAM_STEREO_INVALID or 0, !(mm_f <
 *                2147483648.0f), mm > (int32)(max_depth_m * 1000.0f) or mm < (int32)(min_depth_m * 1000.0f).
 * Parameter encoding (dslam_stereo_params, all int32): a field left at 0 selects its default.  Two fields have a meaningful
 * value 0, which therefore has a code of its own: uniqueness -1 means 0 (the filter is off); lr_max -1 switches the
 * left-right check off and lr_max -2 means 0 (dR must equal d*).  dslam_stereo_get_params returns the block in the same
 * encoding with no field left at 0, so it recreates the same matcher.  pad must be 0.
 * Images are dense rows: left / right uint8 [H][W][channels], disparity uint16 [H][W], depth int16 [H][W] millimetres --
 * what dslam_view_update_device takes as depth_mm_dev.  The host forms stage through buffers of the handle and wait for the
 * stream; the _device forms take device addresses (16-byte aligned), enqueue on the engine's stream and return as every
 * call of a synchronous or asynchronous engine does.  A handle may be destroyed before or after dslam_engine_destroy
 * (DESIGN.md section 21).  None of the calls touches a scene, a view or a render state.
 * DSLAM_ERR_INVALID with nothing enqueued and nothing written: a NULL argument other than params / disp_out; a handle of
 * another engine; width or height outside 1 .. 4096; max_disparity other than 64 or 128; p1 > p2, p2 > 192 or a negative
 * penalty; uniqueness above 99 or below -1; lr_max above D or below -2; channels other than 1 or 4; a non-zero pad; a
 * calibration that is not finite and positive in focal_length_px, baseline_m and scale, with min_depth_m < 0, max_depth_m
 * < min_depth_m or max_depth_m * 1000 >= 32767; a misaligned device address; an unknown `what`; a debug download before
 * the first match.  DSLAM_ERR_HIP from dslam_stereo_create when the volumes cannot be allocated: no handle is made. */
#define DSLAM_STEREO_INVALID 0xFFFF
#define DSLAM_STEREO_COST_OUT 63
#define DSLAM_STEREO_MAX_SIZE 4096
#define DSLAM_STEREO_MAX_P2 192
#define DSLAM_STEREO_CENSUS_LEFT 0
#define DSLAM_STEREO_CENSUS_RIGHT 1
#define DSLAM_STEREO_S 2
typedef struct dslam_stereo dslam_stereo;
typedef struct {
  int32_t max_disparity;           /* 0 -> 128; 64 or 128 */
  int32_t p1;                      /* 0 -> 10; 1 <= p1 <= p2 */
  int32_t p2;                      /* 0 -> 120; p1 <= p2 <= 192 */
  int32_t uniqueness;              /* 0 -> 5; percent, 1 .. 99; -1 = off */
  int32_t lr_max;                  /* 0 -> 1; 1 .. D; -1 = check off; -2 = exact (tolerance 0) */
  int32_t channels;                /* 0 -> 1; 1 = grey bytes, 4 = RGBA */
  int32_t pad[2];
} dslam_stereo_params; /* 32 bytes */
typedef struct {
  float focal_length_px;
  float baseline_m;
  float scale;
  float min_depth_m;
  float max_depth_m;
} dslam_stereo_calib; /* 20 bytes */
int dslam_stereo_create(dslam_engine *e, int width, int height, const dslam_stereo_params *params /* NULL: defaults */,
                        dslam_stereo **out);
int dslam_stereo_destroy(dslam_stereo *st);
int dslam_stereo_get_params(const dslam_stereo *st, dslam_stereo_params *params_out);
/* The disparity of the LEFT image in 1/16 pixel.  Four launches and two memsets: the census of both images, the aggregation of
 * all eight directions, the selection, the left-right check. */
int dslam_stereo_match(dslam_engine *e, dslam_stereo *st, const uint8_t *left_host, const uint8_t *right_host, uint16_t *disp_out_host);
int dslam_stereo_match_device(dslam_engine *e, dslam_stereo *st, const void *left_dev, const void *right_dev, void *disp_out_dev);
int dslam_disparity_to_depth(dslam_engine *e, dslam_stereo *st, const uint16_t *disp_host, const dslam_stereo_calib *calib,
                             int16_t *depth_mm_out_host);
int dslam_disparity_to_depth_device(dslam_engine *e, dslam_stereo *st, const void *disp_dev, const dslam_stereo_calib *calib,
                                    void *depth_mm_out_dev);
/* The match and the conversion without leaving the device (the conversion runs inside the last launch of the match). */
int dslam_stereo_depth(dslam_engine *e, dslam_stereo *st, const uint8_t *left_host, const uint8_t *right_host,
                       const dslam_stereo_calib *calib, int16_t *depth_mm_out_host, uint16_t *disp_out_host /* or NULL */);
int dslam_stereo_depth_device(dslam_engine *e, dslam_stereo *st, const void *left_dev, const void *right_dev,
                              const dslam_stereo_calib *calib, void *depth_mm_out_dev, void *disp_out_dev /* or NULL */);
/* Test hooks.  download: one intermediate result of the most recent match to the host -- DSLAM_STEREO_CENSUS_LEFT / _RIGHT
 * uint64 [H][W], DSLAM_STEREO_S uint16 [H][W][D].  select: selection, left-right check and sub-pixel step on the caller's
 * S (uint16 [H][W][D]; it replaces the handle's).  phases (bench hook): enable >= 0 switches the handle's phase events on
 * or off; out_ms [5] (or NULL): census, aggregation (with its memset), selection, left-right check (with the conversion),
 * stand-alone conversion of the most recent call in ms, -1 where a phase did not run. */
int dslam_debug_stereo_download(dslam_engine *e, dslam_stereo *st, int what, void *out_host);
int dslam_debug_stereo_select(dslam_engine *e, dslam_stereo *st, const uint16_t *S_host, uint16_t *disp_out_host);
int dslam_debug_stereo_phases(dslam_engine *e, dslam_stereo *st, int enable, float out_ms[5]);

/* ---- sparse stereo scene flow: feature matches over a stereo pair and over time -------------
 * What libviso2's Matcher returns from getRawMatches() after two pushBack calls and matchFeatures(method) without a motion
 * prior: the first matching pass, with no prior, refinement or outlier removal.  The law is all-integer, so the device gives
 * the same bytes as tests/ref_sflow.py, and both are held to that library's own output (tests/golden/sflow_*.npz).
 * A handle is made for one image size W x H and one parameter block and keeps two frames: the current one (1c left, 2c
 * right) and the previous one (1p, 2p).  s = 2 and (w, h) = (W / 2, H / 2) with half_resolution, else s = 1, (w, h) = (W, H).
 *   grey        channels == 1: the byte as it is; channels == 4 (RGBA): (r + 2 g + b) >> 2.  With half_resolution the
 *               matching image is m(y, x) = (g(2y, 2x) + g(2y, 2x + 1) + g(2y + 1, 2x) + g(2y + 1, 2x + 1)) >> 2.
 *   filters     four images of m, stated on the interior 2 <= x <= w - 3, 2 <= y <= h - 3 and 0 outside it.  (The
 *               reference pads rows to 16 and lets its row passes run across row ends, which only reaches pixels outside
 *               this interior, and nothing below reads those: the cells and their neighbourhoods stay inside 9 .. w - 10,
 *               and a descriptor tap is at most 5 from its feature, so every read is inside 4 .. w - 5, rows alike.)
 *               With column sums over dy = -2 .. 2 and row sums over dx = -2 .. 2 of the weights given:
 *                 du = sat8(((rows (1, 2, 0, -2, -1) of cols (1, 4, 6, 4, 1)) >> 7) + 128)      left minus right
 *                 dv = sat8(((rows (1, 4, 6, 4, 1) of cols (1, 2, 0, -2, -1)) >> 7) + 128)      top minus bottom
 *                 f1 = - (sum of the 5 x 5 window) + 2 (sum of the 3 x 3 window) + 7 m(y, x)     the blob
 *                 f2 = rows (1, 1, 0, -1, -1) of cols (1, 1, 0, -1, -1)                          the checkerboard
 *               >> is arithmetic, sat8 clamps to 0 .. 255; du, dv are uint8, f1, f2 int16.  (The reference forms f1 from
 *               an integral image of inclusive sums; read that way, what it stores at (y, x) is the window y - 2 .. y + 2,
 *               x - 2 .. x + 2: centred, with no displacement, and the golden files confirm it.)  No intermediate leaves int16, so the reference's wrapping 16-bit
 *               adds never wrap: a (1, 4, 6, 4, 1) sum is at most 16 * 255 = 4080 and the (1, 2, 0, -2, -1) row of it at
 *               most 3 * 4080 = 12240 in magnitude (DSLAM_SFLOW_SOBEL_BOUND); a (1, 2, 0, -2, -1) sum is at most 765 and
 *               its (1, 4, 6, 4, 1) row 16 * 765 = 12240; |f1| <= 16 * 255 = 4080; a (1, 1, 0, -1, -1) sum is at most 510
 *               and f2 at most 4 * 510 = 2040 (DSLAM_SFLOW_CHECKER_BOUND).
 *   features    non-maximum suppression with distance n over cells of (n + 1)^2 pixels.  Cell (a, b) starts at
 *               (i, j) = (n + 9 + a (n + 1), n + 9 + b (n + 1)) and exists while i < w - n - 9 and j < h - n - 9; cells
 *               are taken with the COLUMN index a outermost.  In a cell the minimum and the maximum of f1 and of f2 are
 *               found scanning x outer, y inner, with strict comparisons: of equal values the first met wins.  An
 *               extremum at (u, v) with value e fails if any pixel of u - n .. min(u + n, w - 10), v - n .. min(v + n,
 *               h - 10) is strictly better (the lower bounds are not clamped and need not be: u - n >= 9); it is
 *               accepted if e <= -nms_tau (minimum) or e >= nms_tau (maximum).  A cell gives up to four features, in
 *               class order 0 f1 minimum, 1 f1 maximum, 2 f2 minimum, 3 f2 maximum.  Every image has two sets: set 0
 *               (sparse) with n = 3 nms_n, replaced by max(nms_n, 10) where that exceeds 10; set 1 (dense) with n = nms_n.
 *   record      a feature is 48 bytes: int32 u s, v s, 0, class, then 32 descriptor bytes: for the 16 taps (dx, dy) =
 *               (-3,-1) (-3,1) (-1,-1) (-1,1) (3,-1) (3,1) (1,-1) (1,1) (-1,-5) (-1,5) (1,-5) (1,5) (-5,-3) (-5,3) (5,-3)
 *               (5,3) in this order du(v + dy, u + dx) then dv(v + dy, u + dx).
 *   bins        coordinates of records are full-resolution.  UB = ceil(W / match_binsize), VB = ceil(H / match_binsize);
 *               a feature lies in bin (min(u / match_binsize, UB - 1), min(v / match_binsize, VB - 1)) of its class, with
 *               integer division.  (The reference takes floor of a float quotient.  The quotient of an integer below 2^24
 *               by match_binsize is an integer or at least 1 / match_binsize away from one, and the float rounding error
 *               is below that, so both floors agree.)
 *   find        the partner of a feature q in another set T: the candidates are the features of T of q's class with
 *               |u - uq| <= R and |v - vq| <= R (a flow leg) or <= match_disp_tolerance (a stereo leg), R = match_radius,
 *               halved by integer division with half_resolution.  The cost is the sum of absolute differences of the 32
 *               descriptor bytes (at most DSLAM_SFLOW_MAX_COST = 8160).  The smallest cost wins; of equal costs the
 *               candidate met first when the bins that the window touches (clamped to the grid) are visited bin column
 *               outermost, then bin row, then ascending feature index.  NO candidate gives feature 0 of T: a circle can
 *               close through feature 0, and does so here as in the reference.
 *   methods     2 (quad): for every i1p in order 1p -> 2p (stereo) -> 2c (flow) -> 1c (stereo) -> 1p (flow); kept if the
 *               last leg returns i1p, u1p >= u2p and u1c >= u2c.  1 (stereo): 1c -> 2c -> 1c, kept if it returns and
 *               u1c >= u2c.  0 (flow): 1c -> 1p -> 1c.  For methods 0 and 1 only the first kept feature, in index order,
 *               of those on one current-left pixel stays.  If a set the method needs is empty there are no matches; set 0
 *               also needs the dense sets of the same images non-empty, as the reference checks them before its first
 *               pass.  A match is int32[12]: u1p, v1p, i1p, u2p, v2p, i2p, u1c, v1c, i1c, u2c, v2c, i2c; the fields a
 *               method does not fill hold -1.  Matches are in ascending order of the driving feature's index.
 * Parameter encoding (dslam_sflow_params, all int32): a field left at 0 selects its default; half_resolution has a
 * meaningful 0, so -1 means off.  dslam_sflow_get_params returns the block with no field left at 0.  pad must be 0.
 * Images are dense rows, uint8 [H][W][channels].  push is Matcher::pushBack: the current frame becomes the previous one
 * (or, with replace != 0, is overwritten) and the features and bin lists of the new one are built at once; right may be NULL
 * (monocular flow: the right sets of that frame are empty).  The host forms stage through buffers of the handle and wait
 * for the stream; the _device forms take device addresses (16-byte aligned) and enqueue on the engine's stream: match_device
 * writes min(count, capacity) records to out_dev and the full count to count_dev (one int32) without a host round trip.
 * count is the full number also where capacity is smaller.  A handle may be destroyed before or after its engine.
 * DSLAM_ERR_INVALID with nothing enqueued and nothing written: a NULL argument other than params / right; a handle of another
 * engine; W or H outside s .. DSLAM_SFLOW_MAX_SIZE; nms_n outside 1 .. DSLAM_SFLOW_MAX_NMS_N; nms_tau, match_binsize,
 * match_radius or match_disp_tolerance below 1 (after defaults); more than DSLAM_SFLOW_MAX_BINS bin lists or
 * DSLAM_SFLOW_MAX_FEATURES possible dense features; half_resolution other than 0, 1, -1; channels other than 1 or 4; a
 * non-zero pad; a method, set, image or filter id that does not exist; a negative capacity; a misaligned device address; a
 * debug download before the first push. */
#define DSLAM_SFLOW_MAX_SIZE 4096
#define DSLAM_SFLOW_MAX_NMS_N 32
#define DSLAM_SFLOW_MAX_BINS 65536
#define DSLAM_SFLOW_MAX_FEATURES 4194304
#define DSLAM_SFLOW_MARGIN 9
#define DSLAM_SFLOW_MAX_COST 8160
#define DSLAM_SFLOW_SOBEL_BOUND 12240
#define DSLAM_SFLOW_CHECKER_BOUND 2040
#define DSLAM_SFLOW_FEATURE_BYTES 48
#define DSLAM_SFLOW_MATCH_WORDS 12
#define DSLAM_SFLOW_IMAGE_1C 0
#define DSLAM_SFLOW_IMAGE_2C 1
#define DSLAM_SFLOW_IMAGE_1P 2
#define DSLAM_SFLOW_IMAGE_2P 3
#define DSLAM_SFLOW_FILTER_DU 0
#define DSLAM_SFLOW_FILTER_DV 1
#define DSLAM_SFLOW_FILTER_F1 2
#define DSLAM_SFLOW_FILTER_F2 3
typedef struct dslam_sflow dslam_sflow;
typedef struct {
  int32_t nms_n;                   /* 0 -> 3; 1 .. 32 */
  int32_t nms_tau;                 /* 0 -> 50; >= 1 */
  int32_t match_binsize;           /* 0 -> 50; >= 1 */
  int32_t match_radius;            /* 0 -> 200; >= 1 */
  int32_t match_disp_tolerance;    /* 0 -> 2; >= 1 */
  int32_t half_resolution;         /* 0 -> 1; 1 = on, -1 = off */
  int32_t channels;                /* 0 -> 1; 1 = grey bytes, 4 = RGBA */
  int32_t pad;
} dslam_sflow_params; /* 32 bytes */
int dslam_sflow_create(dslam_engine *e, int width, int height, const dslam_sflow_params *params /* NULL: defaults */,
                       dslam_sflow **out);
int dslam_sflow_destroy(dslam_sflow *sf);
int dslam_sflow_get_params(const dslam_sflow *sf, dslam_sflow_params *params_out);
int dslam_sflow_push(dslam_engine *e, dslam_sflow *sf, const uint8_t *left_host, const uint8_t *right_host /* or NULL */, int replace);
int dslam_sflow_push_device(dslam_engine *e, dslam_sflow *sf, const void *left_dev, const void *right_dev /* or NULL */, int replace);
/* method 0 flow, 1 stereo, 2 quad; set 0 sparse (getRawMatches), 1 dense matched the same way.  out: int32 [capacity][12]. */
int dslam_sflow_match(dslam_engine *e, dslam_sflow *sf, int method, int set, int32_t *out_host, int capacity, int32_t *count_out);
int dslam_sflow_match_device(dslam_engine *e, dslam_sflow *sf, int method, int set, void *out_dev, int capacity, void *count_dev);
/* the feature records of one image (DSLAM_SFLOW_IMAGE_*) and set: [capacity][48] bytes */
int dslam_sflow_features(dslam_engine *e, dslam_sflow *sf, int image, int set, void *out_host, int capacity, int32_t *count_out);
/* Test hooks.  download: one filter image (DSLAM_SFLOW_FILTER_*: du, dv uint8 [h][w]; f1, f2 int16 [h][w]) of the current
 * frame's left (side 0) or right (side 1) image.  phases (bench hook): enable >= 0 switches the handle's phase events on or
 * off; out_ms [6] (or NULL): filters, suppression, feature compaction, bin lists of the most recent push and matching, match
 * compaction of the most recent match in ms, -1 where a phase did not run. */
int dslam_debug_sflow_download(dslam_engine *e, dslam_sflow *sf, int side, int filter, void *out_host);
int dslam_debug_sflow_phases(dslam_engine *e, dslam_sflow *sf, int enable, float out_ms[6]);

/* ---- fern keyframe index: which stored keyframe does this frame look like? ------------------
 * Upstream's relocaliser (FernRelocLib: randomised ferns over a thumbnail of the frame, Glocker et al.) with the codes of
 * all keyframes in HBM.  The reference ships the submodule empty, so the law is this project's own; it is all-integer, so
 * the device gives the same bytes as any other statement of it.
 *   parameters   dslam_fern_params below (every field int32 except seed; 0 selects the default).  F = num_ferns, c = cell.
 *   thumbnail    the index is created for one depth image size W x H.  TW = W / c, TH = H / c (floor); the columns
 *                x >= TW c and the rows y >= TH c are never read.  For cell (tx, ty), over its c x c pixels of the raw
 *                int16 millimetre image as the kernels see it (what dslam_download_view_raw_depth returns) and of the
 *                view's RGBA:  n = the pixels with mm > 0 (a negative value is invalid like 0), S = the int32 sum of
 *                those mm, D = S / n (floor) if 2 n >= c c, else 0 -- a hole;  G = (sum over all c c pixels of
 *                r + 2 g + b) / (4 c c), in 0 .. 255.
 *   fern table   F ferns x 4 decisions, drawn in the order f, then j, from splitmix64 whose state starts at
 *                (uint64_t)seed: next() is  state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) *
 *                0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31.  A decision draws
 *                cell = next() % (TW TH);  channel = next() & 1 (drawn only when channels == 2, otherwise 0);  threshold =
 *                depth_min_mm + next() % (depth_max_mm - depth_min_mm + 1) for channel 0, next() % 255 for channel 1.
 *                dslam_fern_index_table gives it as int32 [F][4][3] = (cell, channel, threshold), cell = ty TW + tx.
 *   code         decision bit = value(cell, channel) > threshold, the value being D for channel 0 (a hole is 0 and never
 *                passes) and G for channel 1;  nibble of fern f = sum_j bit_j << j.  A code is 64 uint32 (256 bytes): fern f
 *                sits in dword f / 8 at bits 4 (f % 8) .. 4 (f % 8) + 3; the dwords of ferns >= F are zero.
 *   dissimilarity of two codes: the ferns f < F whose nibbles differ, 0 .. F.
 *   index        `capacity` codes in HBM with ids 0, 1, ... in the order of insertion; count = how many are stored.  What
 *                else belongs to a keyframe (pose, timestamp, map) stays in the caller's containers keyed by id, as slot
 *                bookkeeping does for the frame store.
 *   query        the candidates are the ids in [first_id, last_id) n [0, count), ordered by (dissimilarity ascending, id
 *                ascending); the first k (k <= DSLAM_FERN_MAX_MATCHES) go to matches_out, their number -- possibly 0 --
 *                to num_out.  Entries of matches_out past that number are not written.
 * With channels == 2 the grey channel is read at the depth image's pixel positions, so a view or frame store whose RGB
 * size differs from its depth size counts as one of another size.  An index may be destroyed before or after its engine's
 * other handles, and before or after dslam_engine_destroy (the lifetime rule of DESIGN.md section 21).  Every call below
 * that takes the engine waits for the stream on synchronous and asynchronous engines, as dslam_survey_views does; none
 * touches a scene, a render state, a view's images, a GetImage memo or a map version.
 * DSLAM_ERR_INVALID with all outputs untouched (and the index unchanged): a NULL argument other than params; a view, store
 * or index of another engine; a view never updated, or a view or store of another size than the index; k outside
 * 1 .. DSLAM_FERN_MAX_MATCHES; first_id > last_id or a negative id; a query id outside [0, count); num_queries outside
 * 1 .. DSLAM_FERN_MAX_QUERIES; a negative harvest threshold; parameters outside their ranges. */
#define DSLAM_FERN_MAX_MATCHES 64
#define DSLAM_FERN_MAX_QUERIES 64
#define DSLAM_FERN_CODE_DWORDS 64
typedef struct dslam_fern_index dslam_fern_index;
typedef struct {
  int32_t num_ferns;               /* 0 -> 512; a multiple of 8 in 8 .. 512 */
  int32_t cell;                    /* 0 -> 8; 1 .. 32 */
  int32_t channels;                /* 0 -> 1; 1 = depth, 2 = depth + grey */
  int32_t depth_min_mm;            /* 0 -> 300 */
  int32_t depth_max_mm;            /* 0 -> 10000; depth_min_mm <= depth_max_mm <= 32767 */
  uint32_t seed;
} dslam_fern_params;
typedef struct {
  int32_t id;
  int32_t dissimilarity;
} dslam_fern_match;
/* capacity: 1 .. 4194304 codes (256 bytes each).  TW TH >= 1, i.e. cell <= min(W, H). */
int dslam_fern_index_create(dslam_engine *e, int width_d, int height_d, const dslam_fern_params *params /* NULL: defaults */,
                            int capacity, dslam_fern_index **out);
int dslam_fern_index_destroy(dslam_fern_index *idx);
int dslam_fern_index_count(const dslam_fern_index *idx, int32_t *count_out);
/* the parameters with their defaults filled in (params_out may be NULL) and the table, int32 [F][4][3] (table_out may be NULL) */
int dslam_fern_index_table(const dslam_fern_index *idx, dslam_fern_params *params_out, int32_t *table_out);
/* count = 0; the ids start again at 0 */
int dslam_fern_index_reset(dslam_engine *e, dslam_fern_index *idx);
/* The view's code, to the host.  Two launches: the thumbnails (the view's images read once), the ferns. */
int dslam_fern_encode(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, uint32_t code_out[DSLAM_FERN_CODE_DWORDS]);
/* The query of the view's code; the index is only read. */
int dslam_fern_query(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, int first_id, int last_id, int k,
                     dslam_fern_match *matches_out /* [k] */, int32_t *num_out);
/* Upstream's ProcessFrame in one device round trip: the query's result, and the view's code is appended (its id to
 * added_id_out, -1 when nothing was added) when the index is empty or the smallest dissimilarity over ALL stored ids --
 * whatever the window -- is >= harvest_min_dissimilarity; 0 always appends.  The decision is taken on the device.  A full
 * index that should append returns DSLAM_ERR_UNSUPPORTED: the matches and their number are still delivered, added_id_out
 * is -1 and the index is unchanged. */
int dslam_fern_process(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, int harvest_min_dissimilarity, int first_id,
                       int last_id, int k, dslam_fern_match *matches_out /* [k] */, int32_t *num_out, int32_t *added_id_out);
/* Encodes and appends the stored keyframes of the slots first_slot .. first_slot + num_slots - 1 straight from the store's
 * device images: ids in slot order, the first to first_id_out; the same codes as dslam_view_update_from_store +
 * dslam_fern_process(..., 0, ...) per slot.  Two launches per batch of slots whose thumbnails fit the index's scratch
 * (64 MiB: 3495 keyframes of 640 x 480 at cell 8), never one per slot.  DSLAM_ERR_INVALID with nothing written: num_slots
 * < 1, a range that does not fit the store or the remaining capacity, a store of another size. */
int dslam_fern_add_from_store(dslam_engine *e, dslam_fern_index *idx, const dslam_frame_store *fs, int first_slot, int num_slots,
                              int32_t *first_id_out);
/* The queries are stored codes (num_queries in 1 .. DSLAM_FERN_MAX_QUERIES); the stored codes of the window are read once
 * for all of them.  Row q of matches_out / num_out is what dslam_fern_query gives for a view with the code of
 * query_ids[q]; a query id inside the window is a candidate like any other and matches itself at 0.  Rows are num_queries
 * x k: entry j of row q is matches_out[q k + j]. */
int dslam_fern_query_stored(dslam_engine *e, dslam_fern_index *idx, const int32_t *query_ids, int num_queries, int first_id,
                            int last_id, int k, dslam_fern_match *matches_out /* [num_queries][k] */,
                            int32_t *num_out /* [num_queries] */);

/* Fuse one local map into another on the device (no counterpart in the reference; the law is this project's own,
 * DESIGN.md section 14).  X is what dslam_register_maps takes and returns: source frame -> destination frame, metres,
 * column-major.  X~ is X with its translation in voxel units, Y~ its inverse (R^T, -R^T t); both are formed on the host
 * in double and rounded to float32 (12 entries each); an X that is exactly the identity reads at p itself both ways.
 *   1. targets (push): source voxels in order -- resident entries ascending by hash index (rank r), then the voxel's
 *      linear index l (x fastest) -- with key r * 512 + l + 1; a candidate has w_depth > 0 (no band gate: observed free
 *      space merges too); q = X~ p, rows evaluated as ((a x + b y) + c z) + d in float32; target voxel floor(q + 0.5f)
 *      per axis, target block B = t >> 3; a B outside int16 is skipped and counted in out_of_range;
 *   2. allocation passes: every candidate's B is looked up in dst; a hit marks the entry touched, a miss requests the
 *      slot the allocation pass would use for that bucket (empty bucket head: type 1, otherwise the chain end: type 2)
 *      and a slot keeps the largest key that asked.  Requested slots are served in ascending hash-index order exactly
 *      as AllocateSceneFromDepth deals pool slots (the successful request that has v voxel-block slots taken in front
 *      of it gets voxelAllocationList[lastFree - v]; type 2 also takes the next excess slot; a request that finds a
 *      pool empty fails and takes nothing); the entry gets the winner's B and is touched, its block holds empty
 *      voxels.  Blocks that lost a slot ask again in the next pass.  Passes stop when a pass has no miss; or serves
 *      nothing while misses remain (exhausted = 1, requests_unserved = the slots asked for in that pass); or when
 *      max_passes have run (exhausted = 1, requests_unserved = the requests of the last pass that were not served);
 *   3. fusion (pull): every voxel p' of every touched destination block: q' = Y~ p', cell floor(q'), fractions c; all 8
 *      taps of the cell must lie in resident blocks of the source with w_depth > 0, else the voxel is left alone;
 *      d = the trilinear blend of raw / 32767 in dslam_register_maps' order; the resampled voxel is packed:
 *      sdf = (short)(d * 32767), w_depth = min of the 8 taps'; its colour half is live only with with_colour and all 8
 *      w_color > 0: each channel (unsigned char)(blend((float)c_k) + 0.5f), w_color = min of the taps'; otherwise
 *      w_color = 0.  With the identity the resampled voxel is the source's voxel at p' as stored (an absent block reads
 *      as the empty voxel).  It is then merged into the resident voxel exactly as a swapped-out block's host copy is
 *      (CombineVoxelInformation, dst's max_w); a voxel is stored only if it changed (voxels_changed).
 * Under a non-identity X the outermost one-voxel layer of what src saw is therefore not transferred.
 * src is only read.  dst's render states are not touched (their visible lists stay as they were); GetImage memos and
 * front-end records of dst are invalidated as by dslam_upload_scene_state.  Waits for the stream on synchronous and
 * asynchronous engines.  DSLAM_ERR_INVALID with nothing changed: a NULL argument other than params, a scene of another
 * engine, src == dst, voxel_size or mu that differ bitwise, a scene that uses swapping or is sharded, a non-finite X or
 * one whose rotation block is not orthonormal to 1e-4, a negative max_passes. */
typedef struct {
  int32_t max_passes;              /* 0 -> 16 */
  int32_t with_colour;             /* default 1 */
} dslam_merge_params;
typedef struct {
  int32_t passes, exhausted;       /* allocation passes run; 1 if the pools ran dry (or max_passes was reached) */
  int32_t src_blocks, blocks_allocated, blocks_touched, requests_unserved;
  int64_t src_candidates, out_of_range, voxels_changed;
} dslam_merge_result;
int dslam_merge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float X_dst_from_src[16],
                     const dslam_merge_params *params /* NULL: defaults */, dslam_merge_result *result);
/* Bench hook: out_ms (may be NULL) receives the wall clock of the engine's last merge by phase -- [0] the source's live
 * list, [1] mark kernels, [2] ordered selections (ranks, serve, touched list), [3] block kernel, [4] read-backs -- measured
 * only while the hook is on, when every phase ends with a wait for the stream (the bytes do not change); then `enable`
 * turns the hook on or off for the merges that follow. */
int dslam_debug_merge_phases(dslam_engine *e, int enable, double out_ms[5]);

/* Undo a map merge on the device (no counterpart in the reference; the law is this project's own):
 * dslam_unmerge_maps(src, dst, X) removes from dst what dslam_merge_maps(src, dst, X) added.  X, X~, Y~ and the identity
 * flag are formed exactly as dslam_merge_maps forms them.
 *   1. targets (push): step 1 of the merge, unchanged -- the source's resident entries ascending by hash index, candidates
 *      have w_depth > 0, q = X~ p with rows evaluated as ((a x + b y) + c z) + d in float32, target voxel floor(q + 0.5f)
 *      per axis, target block B = t >> 3; a B outside int16 is skipped and counted in out_of_range;
 *   2. lookup: every candidate's B is looked up in dst.  A hit marks the entry touched; a miss counts the candidate voxel
 *      in candidates_without_block (one count per source voxel).  Nothing is allocated: the table, both free lists, the
 *      counters, alloc_bits and the born stamps of dst are not written;
 *   3. removal (pull): every voxel p' of every touched destination block.  The resampled voxel is step 3 of the merge,
 *      unchanged: q' = Y~ p', cell floor(q'), all 8 taps in resident blocks of the source with w_depth > 0 (else the voxel
 *      is left alone), sdf = (short)(blend * 32767), w_depth = min of the 8 taps'; the colour half live only with
 *      with_colour and all 8 w_color > 0, each channel (unsigned char)(blend((float)c_k) + 0.5f), w_color = min of the
 *      taps'; under the identity the source's voxel at p' as stored (its w_color read as 0 without with_colour).  It is
 *      then taken out of the resident voxel by the inverse of CombineVoxelInformation, the two halves independent, in
 *      float32 with no contraction and IEEE division:
 *      depth half, ws the resampled w_depth and W the resident one: ws == 0 idles; W < ws idles and is counted in
 *      depth_underweight (dst does not hold that much: it was decayed, or never merged); otherwise rem = W - ws;
 *      rem == 0: sdf = 32767, w_depth = 0 (the colour byte that shares the word stays), as removing the last observation
 *      leaves a voxel; rem > 0: F = ((float)W * (sdf / 32767.0f) - (float)ws * (sdf_s / 32767.0f)) / (float)rem, clamped
 *      to [-1, 1], sdf = (short)(F * 32767.0f), w_depth = rem;
 *      colour half, wcs and Wc the w_colors: wcs == 0 idles; Wc < wcs idles and is counted in colour_underweight;
 *      rem == 0: the three channels and w_color become 0; otherwise per channel
 *      v = (((float)dc / 255.0f) * (float)Wc - ((float)sc / 255.0f) * (float)wcs) / (float)rem, clamped to [0, 1], the
 *      channel (unsigned char)(v * 255.0f), w_color = rem.
 *      A voxel is stored only if it changed (voxels_changed).
 * What the law does not promise: the removal is the exact inverse of the merge's weights, and of its values to within
 * (W0 + ws) / W0 + 1 raw sdf units for a voxel of weight W0 before the merge, only while nothing
 * clamped at max_w during the merge and src and the affected part of dst have not changed since; the call cannot check
 * any of this.  Blocks the merge allocated stay allocated and hold empty voxels: releasing them is dslam_decay's job.
 * src is only read.  dst's render states are not touched; GetImage memos and front-end records of dst are invalidated as
 * by dslam_merge_maps.  Waits for the stream on synchronous and asynchronous engines.  DSLAM_ERR_INVALID with nothing
 * changed: a NULL argument other than params, a scene of another engine, src == dst, voxel_size or mu that differ bitwise,
 * a scene that uses swapping or is sharded, a non-finite X or one whose rotation block is not orthonormal to 1e-4. */
typedef struct {
  int32_t with_colour;             /* default 1 */
  int32_t reserved;                /* 0 */
} dslam_unmerge_params;
typedef struct {
  int32_t src_blocks, blocks_touched;
  int64_t src_candidates, out_of_range, candidates_without_block, voxels_changed, depth_underweight, colour_underweight;
} dslam_unmerge_result;
int dslam_unmerge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float X_dst_from_src[16],
                       const dslam_unmerge_params *params /* NULL: defaults */, dslam_unmerge_result *result);
/* Correct a merge: dslam_unmerge_maps(src, dst, X_old) with params->with_colour, then dslam_merge_maps(src, dst, X_new,
 * params), in one call -- dst ends byte-identical to the two calls made one after the other, and the two results are what
 * they return.  All arguments of both halves are checked before anything is changed (the rejections of both calls).
 * X_old and X_new bit-identical: nothing is done, both results are zeroed, DSLAM_OK.  The one call validates once,
 * compacts the source's live list once and saves one wait for the stream. */
int dslam_remerge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float X_old[16],
                       const float X_new[16], const dslam_merge_params *params /* NULL: defaults */,
                       dslam_unmerge_result *unmerged, dslam_merge_result *merged);

/* ---- packed maps: the layout and its host half ---------------------------------------------------- */
/* A compact, self-describing, deterministic image of a map (DESIGN.md section 21 states the law in full: which entries are
 * packed, what an unpack into a pool of any size leaves, what is checked before its first write).  The host half -- the
 * two layout functions, callable without a device, as dslam_view_frustum_planes is -- comes first; the device calls that
 * write and read such an image, dslam_pack_scene and dslam_unpack_scene, follow.
 * Layout, little-endian; every byte up to total_bytes is defined.  n: the resident entries (ptr >= 0), in ascending hash
 * index (rank order); f = last_free_excess_id + 1:
 *   offset 0                64-byte header: dslam_pack_info as it lies in memory
 *   offset 64               n records of 16 bytes, rank order: a dslam_hash_entry with pos and offset as stored,
 *                           _pad = 0, and ptr = THE ENTRY'S HASH INDEX
 *   offset 64 + 16 n        f values of int32: excess_list[0 .. f-1] verbatim (the order of the free stack decides
 *                           future allocations, so it is carried)
 *   up to blocks_offset     zeros; blocks_offset = 64 + 16 n + 4 f rounded up to a multiple of 4096
 *   offset blocks_offset    n voxel blocks of 4096 bytes, rank order, as stored
 *   total_bytes = blocks_offset + 4096 n.
 * bbox_min / bbox_max: componentwise minimum and maximum of pos over the packed entries (n = 0: 32767 and -32768), so a
 * host can test a parked map against dslam_view_frustum_planes without a table on the device. */
typedef struct {
  char magic[4];                   /* "DSPK" */
  uint32_t version;                /* 1 */
  int32_t num_buckets, num_excess; /* the geometry of the table the indices refer to */
  int32_t blocks;                  /* n */
  int32_t free_excess;             /* f */
  uint32_t voxel_size_bits, mu_bits;  /* the bit patterns of the scene's float32 voxel_size and mu */
  int64_t blocks_offset, total_bytes;
  int16_t bbox_min[3], bbox_max[3];
  uint32_t reserved;               /* 0 */
} dslam_pack_info;
/* Host only: the two layout functions of (n, f) above, in 64 bits.  DSLAM_ERR_INVALID, with both outputs untouched, for a
 * negative n or f or a NULL output. */
int dslam_pack_layout(int32_t blocks, int32_t free_excess, int64_t *blocks_offset_out, int64_t *total_bytes_out);
/* Host only: reads the header of a packed map from its first 64 bytes (host memory, any alignment).  Validates magic,
 * version, the reserved word, that num_buckets, num_excess, n and f are not negative, f <= num_excess, and that
 * blocks_offset and total_bytes are the functions of n and f above; DSLAM_ERR_INVALID leaves *out untouched.  voxel_size,
 * mu and the bounding box pass through unjudged: comparing them with a scene is the caller's. */
int dslam_pack_header_read(const void *first_64_bytes, dslam_pack_info *out);
/* Device memory of the engine's device for a packed map, for callers without a HIP runtime of their own (the ITMLib
 * mirror's CompactLocalMap): hipMalloc / hipFree, 256-byte aligned at least; the free waits for the engine's stream. */
int dslam_device_alloc(dslam_engine *e, size_t bytes, void **out);
int dslam_device_free(dslam_engine *e, void *p);
/* The device half (csrc/pack.hip).  `buf` is device memory of the engine's device or page-locked host memory
 * (dslam_host_alloc, hipHostMalloc, hipHostRegister), 16-byte aligned: the kernels write and read it directly.  The
 * library asks hipPointerGetAttributes about its first and its last byte and rejects, before anything is launched, a
 * pointer the device cannot address (ordinary pageable memory).  Both calls reject (DSLAM_ERR_INVALID, nothing written)
 * a scene that uses swapping, a sharded scene (num_shards > 1 or a shard range), a scene whose re-integration batch is
 * being planned, and a scene of another engine.
 *
 * dslam_pack_scene writes the image of `s` to buf[0 .. total_bytes): every byte of that range and none outside, the same
 * bytes on every run.  It runs on the engine's stream, so it sees everything enqueued before it, and it returns with the
 * buffer complete on synchronous and asynchronous engines alike.  `s` is only read: version, front-end record and GetImage
 * memos stay.  buf == NULL is the size query: *info_out is filled (it is the header a pack would write) and nothing is
 * written; capacity is ignored.  capacity < total_bytes: DSLAM_ERR_INVALID, nothing written, *info_out still filled.
 *
 * dslam_unpack_scene reads the image in buf[0 .. bytes) into `s`, a scene of N = num_local_blocks blocks, and leaves
 * what DESIGN.md section 21 states: record k at the entry its index names with ptr = N-1-k, block k in slot N-1-k,
 * every other slot empty, every other entry the reset entry, the free excess stack as packed, everything else as
 * dslam_scene_reset leaves it; the version is advanced, front-end record and memos are dropped.  Before the first write
 * to `s` the host validates the header (dslam_pack_header_read) and compares it with the scene -- num_buckets and
 * num_excess equal, voxel_size and mu equal bitwise, 0 <= n <= N, bytes >= total_bytes -- and a read-only device pass
 * checks that the record indices lie in the table and ascend strictly, every offset in [0, num_excess], every free
 * value in [0, num_excess); its verdict is read back first.  A failure of any of these leaves `s` as it was
 * (DSLAM_ERR_INVALID).  The kernels that write judge every record index, offset and free value again as they read it,
 * so even if the buffer changes under the call no address depends on an unchecked value and no value outside these
 * ranges reaches the table or the free list (a record or free value that fails then is skipped: the reset's stays).
 * If anything fails after the first write -- a HIP call, or a device report heard by the wait -- `s` is left as
 * dslam_scene_reset leaves it and the failure's code is returned.  Returns with the scene complete; buf may be released
 * then.  info_out (may be NULL for unpack): the header read, filled only on success. */
int dslam_pack_scene(dslam_engine *e, const dslam_scene *s, void *buf, int64_t capacity, dslam_pack_info *info_out);
int dslam_unpack_scene(dslam_engine *e, dslam_scene *s, const void *buf, int64_t bytes, dslam_pack_info *info_out);

/* ---- depth tracker (ICP) ---------------------------------------------------------------------- */
/* trackingController->Track(trackingState, view) (InfiniTamDriver.h:151-163, reached through
 * DenseSlam.cpp:200-206 when the reference runs without ORB-SLAM2 odometry): upstream InfiniTAM v2's
 * ITMDepthTracker::TrackCamera -- point-to-plane ICP of the view's depth image against the points / normals maps
 * that dslam_create_icp_maps left in the render state, coarse to fine over a depth-image pyramid
 * (FilterSubsampleWithHoles), Levenberg-Marquardt damping, 3x3 / 6x6 Cholesky steps.
 * iteration types as upstream's TrackerIterationType. */
enum { DSLAM_TRACKER_ITERATION_ROTATION = 1, DSLAM_TRACKER_ITERATION_TRANSLATION = 2,
       DSLAM_TRACKER_ITERATION_BOTH = 3, DSLAM_TRACKER_ITERATION_NONE = 4 };
#define DSLAM_TRACKER_MAX_LEVELS 8
typedef struct {
  int32_t no_hierarchy_levels;     /* ITMLibSettings::noHierarchyLevels (upstream default 5) */
  int32_t no_icp_run_till_level;   /* ITMLibSettings::noICPRunTillLevel (0) */
  float dist_thresh;               /* depthTrackerICPThreshold (0.1 * 0.1) */
  float termination_threshold;     /* depthTrackerTerminationThreshold (1e-3) */
  int32_t regime[DSLAM_TRACKER_MAX_LEVELS]; /* trackingRegime per level, level 0 = full resolution
                                     * (upstream default: BOTH, BOTH, ROTATION, ROTATION, ROTATION) */
} dslam_tracker_params;
typedef struct {
  int32_t iterations;              /* ComputeGandH evaluations */
  int32_t valid_points_last;       /* noValidPoints of the last evaluation */
  float f_last;                    /* its error value */
  int32_t pad;
} dslam_tracker_result;
/* scene_pose_M = trackingState->pose_pointCloud->GetM() (the pose the ICP maps were rendered from); pose_M is
 * trackingState->pose_d->GetM() on entry and the tracked pose on return.  The view must have been updated. */
int dslam_track_camera(dslam_engine *e, const dslam_view *v, dslam_render_state *r, const float scene_pose_M[16],
                       float pose_M[16], const float intrinsics_d[4], const dslam_tracker_params *params,
                       dslam_tracker_result *result);
/* Test hook: the sums of the most recent ComputeGandH evaluation of this engine's tracker, as accumulated in double and
 * before anything is rounded to float: out[0..20] the Hessian's lower triangle row by row (k, j <= k; the 3-parameter
 * iteration types fill the first 6), out[21..26] the gradient, out[27] the sum of b^2, out[28] the valid-point count.
 * A tracked pose mixes all of them through damped solves; a test of the per-pixel function reads them here (one
 * evaluation is isolated with no_hierarchy_levels = k + 1, no_icp_run_till_level = k and a termination threshold no
 * step stays below).  Error if no evaluation has run. */
int dslam_debug_icp_sums(dslam_engine *e, double out[29]);

/* ---- depth-to-SDF tracker over all local maps --------------------------------------------------- */
/* Tracks the camera of a view directly against the signed distance fields of N posed local maps (no counterpart in the
 * reference, which tracks by ICP against the raycast of the current local map alone, DenseSlam.cpp:198-206; the law is
 * this project's own).  It back-projects the depth pixels under the pose estimate, reads the
 * blended SDF and its gradient where the points land and drives the SDF there to zero: no raycast, no render state, no
 * visible list, and a local map that is still empty is tracked through its neighbours.
 * T_i: world -> map i in metres, column-major (estimatedGlobalPose.GetM()), as dslam_get_image_multi and
 * dslam_register_graph take it; T~_i is T_i with its translation in voxel units.  pose_M: world -> camera, metres,
 * column-major.  P~ is camera -> world: the rigid inverse of pose_M with its translation in voxel units; the host keeps
 * it in double for the whole call and rounds its 12 entries to float32 for each evaluation.
 * One evaluation at level l of the depth pyramid (level 0 is the view's float depth, level k FilterSubsampleWithHoles of
 * level k - 1, the intrinsics halved per level, as dslam_track_camera).  For every pixel (x, y):
 *   1. candidate: D = depth_l[x, y] > 1e-8f; candidates are counted in N;
 *   2. camera point in voxel units: c = (D ((x - cx) / fx), D ((y - cy) / fy), D) in float32, each component then
 *      multiplied by (float)(1.0 / (double)voxel_size);
 *   3. world point p = P~ c, rows evaluated as ((a x + b y) + c z) + d in float32; the three-term sum before d is added,
 *      r = R c, is kept: it is p relative to the camera centre t (the translation of P~), free of t's rounding;
 *   4. per map i, in list order: q_i = T~_i p in the same row order (a T_i that is exactly the identity reads at p
 *      itself); a q_i with a coordinate of magnitude >= 262144 is a miss for that map; cell floor(q_i), fractions
 *      c = q_i - floor(q_i); items 3 and 4 of dslam_register_maps apply unchanged: all 8 taps resident, each with
 *      w_depth > 0 and a raw sdf other than +-32767, else a miss for that map; the value d_i and the gradient g_i from
 *      those taps in the float32 expressions stated there; the weight w_i is the same three lerp stages applied to the
 *      taps' w_depth as floats (x00 = ux w0 + cx w1, ..., w_i = uz (uy x00 + cy x10) + cz (uy x01 + cy x11)); the gradient
 *      in the world frame is g_i^w = R_i^T g_i, each component (r0 gx + r1 gy) + r2 gz with (r0, r1, r2) a column of
 *      R_i (an identity map leaves g_i as it is);
 *   5. combine, by the law of dslam_get_image_multi: no map passed: the pixel is a miss; one map passed: d and g are its
 *      values unchanged; several: d = sum w_i d_i / sum w_i and g = sum w_i g_i^w / sum w_i, component by component, in
 *      float32, in list order (sum w > 0 always: every tap weighs at least 1) -- the camera is tracked against the
 *      field the composite raycast draws;
 *   6. gate: |d| > residual_gate is a miss;
 *   7. a valid pixel has b = -d and the row A = [r x g, g] (rotation about the camera centre t, then translation): no
 *      operand of the row has the size of the camera's position, so the products, which are float32, keep their
 *      relative precision however far from the world origin the camera is;
 *   8. the 33 sums of dslam_register_maps' item 6 with r in place of q: [29..31] sum r over the valid pixels, [32] N;
 *   9. cost = (sum b^2 + (N - valid) residual_gate^2) / N (residual_gate^2 for N = 0).
 * Iteration: the levels run from no_hierarchy_levels - 1 down to run_till_level.  Each level runs dslam_register_maps'
 * iteration word for word on P~: pivot at the centroid -- sum r / valid is the centroid relative to t, H_c and g_c are the
 * sums re-pivoted by it, and c = t + sum r / valid in double, t the float32 translation that was evaluated, is the centroid
 * in the world --, (H_c + lambda diag H_c) y = g_c, the step
 * applied on the left of P~ as p' = c + R(y0..2)(p - c) + y3..5, accepted on valid >= min_valid and a lower cost, the
 * lambda rules and stop reasons 0 - 3 unchanged.  Each level starts at lambda = 1 from the pose the level above returned;
 * max_evaluations is per level; a level that stops with reason 3 changes nothing and the next level starts from the same
 * pose.  pose_M returns the rigid inverse of the last accepted P~ (rotation rounded to float32, translation multiplied
 * by voxel_size, then rounded); if no step was accepted on any level it is untouched, byte for byte.
 * Every map is only read (blocks that are swapped out are simply not resident); no render state is involved; no map's
 * version, GetImage memo or front-end record changes.  Waits for the stream on synchronous and asynchronous engines.
 * DSLAM_ERR_INVALID with pose_M untouched: a NULL argument other than params, num_maps outside
 * 1 .. DSLAM_MAX_RENDER_MAPS, a scene listed twice, a scene (or the view) of another engine, voxel_size or mu that differ
 * bitwise between maps, a non-finite T_i or pose_M or one whose rotation block is not orthonormal to 1e-4, levels outside
 * 1 .. DSLAM_TRACKER_MAX_LEVELS or too many for the image, run_till_level outside the levels, a negative parameter, a
 * view that was never updated.
 * Not promised: convergence from farther away than the truncation band -- a tap at +-32767 is a miss, so a pixel whose
 * point lies more than mu from every surface contributes nothing and the start pose has to come from the previous frame
 * or a motion model; anything about dslam_track_camera, which is not touched. */
typedef struct {
  int32_t no_hierarchy_levels;     /* 0 -> 3 */
  int32_t run_till_level;          /* finest level run (0: full resolution) */
  int32_t max_evaluations;         /* per level; 0 -> 10 */
  int32_t min_valid;               /* 0 -> 500 */
  float residual_gate;             /* 0 -> 0.75 */
  float term_rotation;             /* radians; 0 -> 1e-5 */
  float term_translation_voxels;   /* 0 -> 1e-3 */
  int32_t pad;
} dslam_track_sdf_params;
typedef struct {
  int32_t evaluations;             /* of all levels together */
  int32_t levels_stepped;          /* bit l: level l accepted a step */
  int32_t stop_reason;             /* this and the fields below: of the finest level run */
  int32_t candidates;              /* N */
  int32_t valid_last;              /* valid pixels at the returned pose */
  float cost_first;                /* cost at the level's start pose */
  float cost_last;                 /* cost at the returned pose */
  float conditioning;
} dslam_track_sdf_result;
int dslam_track_camera_sdf(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes,
                           const float *T_map_from_world /* [num_maps][16] */, int num_maps,
                           float pose_M[16] /* world -> camera; in: start, out: estimate */, const float intrinsics_d[4],
                           const dslam_track_sdf_params *params /* NULL: defaults */, dslam_track_sdf_result *result);
/* Test hook: the 33 raw sums of the engine's most recent evaluation.  The rows are pivoted at the camera centre of the P~
 * that was evaluated: [0..20] and [21..23] hold r x g where they held p x g with p in world voxels, and [29..31] sum r where
 * they held sum p (items 7 and 8 above); [24..28] and [32] do not depend on the pivot.  Error if none has run. */
int dslam_debug_track_sdf_sums(dslam_engine *e, double out[33]);

/* ---- depth-to-SDF tracker with a photometric term ------------------------------------------------ */
/* dslam_track_camera_sdf fixes only what the surface's shape fixes: on a road, a facade or a corridor wall it slides
 * along the plane.  dslam_track_camera_sdf_rgb adds a photometric residual between the maps' colour field at the
 * back-projected point and the view's own pixel (ITMColorTracker's purpose in the reference).  The
 * colour comes out of the 8 taps the depth term has already loaded (a voxel's second word), the Jacobian goes through the
 * maps' trilinear colour field as the SDF's does: no image gradients, no raycast, one 4-byte image read per pixel.
 * The view's colour and depth images must have the same size (pixel (x, y) of the one is pixel (x, y) of the other).
 *
 * One evaluation at level l.  Items 1 - 6 of dslam_track_camera_sdf stand word for word (candidate, camera point, world
 * point p and r = R c, the per-map read, the blend, the residual gate), and so do b = -d and A = [r x g, g].  Added:
 *   where     level l carries the photometric term iff l - run_till_level < colour_levels; on the other levels an
 *             evaluation is dslam_track_camera_sdf's, with sums [33] and [34] zero;
 *   image     G_0[x, y] = ((0.299f R + 0.587f G) + 0.114f B) * (float)(1.0 / 255.0) of the view's RGBA pixel, alpha
 *             ignored; G_k[x, y] = ((a + b) + (c + d)) * 0.25f of level k - 1's pixels (2x, 2y), (2x + 1, 2y),
 *             (2x, 2y + 1), (2x + 1, 2y + 1); level k has the size of level k of the depth pyramid (H / 2, W / 2, an odd
 *             last row or column dropped).  The pixel's intensity is I = G_l[x, y]: integer pixel, no interpolation;
 *   map       per map i that passed its 8-tap gate for this pixel, on the same cell and the same 16 words: the map is
 *             colour-ok iff all 8 taps have w_color > 0; the tap grey y_k is the expression of G_0 on the tap's clr bytes;
 *             C_i and h_i are the trilinear value and the analytic gradient by the expressions of d_i and g_i with y in
 *             place of s; w^c_i is the three lerp stages on the taps' w_color; h_i^w = R_i^T h_i as g_i^w; the colour-ok
 *             maps are combined by item 5's law in list order (one: unchanged; several: C = sum w^c C / sum w^c, h alike):
 *             dslam_get_image_multi's colour law;
 *   gate      e = C - I; the pixel is a colour miss if it is a depth miss (item 6), if no map is colour-ok, or if
 *             |e| > colour_gate;
 *   rows      with k = colour_weight: b_c = -(k e) and A_c = k [r x h, h] (each of the six entries of [r x h, h] times k),
 *             pivoted at the camera centre as A;
 *   sums      35 doubles of float32 products: [0..20] the lower triangle of sum A A^T + sum A_c A_c^T (a pixel adds its
 *             depth product, then its colour product), [21..26] sum b A + sum b_c A_c, [27] sum b^2, [28] valid,
 *             [29..31] sum r over the valid pixels, [32] N, [33] sum e^2 over the colour-valid pixels, [34] colour-valid;
 *   cost      cost = cost_depth + k^2 cost_colour; cost_depth is item 9; cost_colour = (sum e^2 + (N - colour_valid)
 *             colour_gate^2) / N, colour_gate^2 for N = 0, and absent (0) on a level without the term.
 * Iteration: dslam_track_camera_sdf's, on the combined sums: the pivot at sum r / valid (the colour rows are pivoted at t
 * too), a trial accepted on valid >= min_valid and a lower cost; lambda rules, stop reasons and "pose_M untouched byte for
 * byte if nothing was accepted" unchanged.
 * colour_weight's default of 1 is a convention and not a tuned value: d is a fraction of mu and e a fraction of 255, so
 * both residuals are dimensionless on their full scale.
 * Every map is only read; no render state, version, memo or front-end record changes.  Waits for the stream on synchronous
 * and asynchronous engines.  dslam_track_camera_sdf is not touched.
 * DSLAM_ERR_INVALID with pose_M and result untouched: every rejection of dslam_track_camera_sdf; a view whose colour and
 * depth images differ in size; a negative or NaN colour_weight or colour_gate; colour_levels negative or above the levels
 * run (no_hierarchy_levels - run_till_level).
 * Not promised: convergence from farther than the truncation band or a quarter of the texture's period; anything about
 * exposure changes. */
typedef struct {
  dslam_track_sdf_params base;
  float colour_weight;             /* k; 0 -> 1.0 */
  float colour_gate;               /* fraction of full scale; 0 -> 0.25 */
  int32_t colour_levels;           /* finest levels that carry the term; 0 -> 1 */
  int32_t pad;
} dslam_track_sdf_rgb_params;
typedef struct {
  dslam_track_sdf_result base;     /* cost_first, cost_last: the combined cost */
  int32_t colour_valid_last;       /* this and the fields below: of the finest level run, at the returned pose */
  float colour_rms_last;           /* sqrt(sum e^2 / colour_valid), 0 for colour_valid = 0 */
  float cost_depth_last;
  float cost_colour_last;          /* before k^2; 0 on a level without the term */
} dslam_track_sdf_rgb_result;
int dslam_track_camera_sdf_rgb(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes,
                               const float *T_map_from_world /* [num_maps][16] */, int num_maps,
                               float pose_M[16] /* world -> camera; in: start, out: estimate */, const float intrinsics_d[4],
                               const dslam_track_sdf_rgb_params *params /* NULL: defaults */,
                               dslam_track_sdf_rgb_result *result);
/* Test hooks: the 35 raw sums of the engine's most recent evaluation of dslam_track_camera_sdf_rgb (error if none has
 * run), and level `level` of the grey pyramid G as the most recent call on this view built it, (W >> level) x (H >> level)
 * floats to host memory (error if that call built no such level). */
int dslam_debug_track_sdf_rgb_sums(dslam_engine *e, double out[35]);
int dslam_debug_track_sdf_rgb_grey(dslam_engine *e, const dslam_view *v, int level, float *out_host);

/* ---- depth-to-SDF tracking from many start poses at once ---------------------------------------- */
/* dslam_track_camera_sdf promises nothing from farther away than the truncation band.  After a tracking loss, at a loop
 * closure or against maps dslam_register_graph has just moved, a caller has a region of poses and not a pose; these calls
 * try many of them for the price of a few: one kernel launch per round of evaluations, however
 * many poses take part in it.  No counterpart in the reference.
 *
 * dslam_score_camera_poses: element k of scores_out is one evaluation (items 1 - 9 above) of poses_M[k] on `level` of the
 * view's pyramid: candidates = N, valid, cost.  They are exactly the candidates, valid_last and cost_first
 * dslam_track_camera_sdf returns for that pose with no_hierarchy_levels = level + 1, run_till_level = level,
 * max_evaluations = 1 and the same residual_gate (0 -> 0.75): the kernel keeps the single call's partition of the pixels
 * over 512 workgroups, its reduction order inside a workgroup, and adds a pose's workgroup rows in index order from +0.0.
 * An element depends on its own pose alone: permuting the list permutes the outputs and changes nothing else.
 *
 * dslam_track_camera_sdf_starts: poses_M[k] and results[k] are, byte for byte, what dslam_track_camera_sdf returns when
 * called alone from start k with the same arguments; a start whose single call would leave its pose untouched is left
 * untouched.  Per pyramid level, coarse to fine, the iterations of all starts advance in lock-step, one launch per round
 * over the starts that have not stopped at that level; a start that has stopped idles until the level ends (the
 * trajectories do not depend on each other, so idling changes no outcome).
 *
 * Both are read-only on every map, touch no render state, version, memo or front-end record, and wait for the stream on
 * synchronous and asynchronous engines.  DSLAM_ERR_INVALID with poses_M, results and scores_out untouched: every rejection
 * of dslam_track_camera_sdf (a pose of the list in place of pose_M); num_poses / num_starts outside
 * 1 .. DSLAM_MAX_TRACK_STARTS; level outside 0 .. DSLAM_TRACKER_MAX_LEVELS - 1 or with no pixel at this image size; a
 * negative (or NaN) residual_gate. */
#define DSLAM_MAX_TRACK_STARTS 256
typedef struct {
  int32_t candidates, valid;       /* N and the valid pixels of the evaluation */
  float cost;                      /* item 9 */
  int32_t pad;
} dslam_pose_score;
int dslam_score_camera_poses(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes,
                             const float *T_map_from_world /* [num_maps][16] */, int num_maps,
                             const float *poses_M /* [num_poses][16], world -> camera */, int num_poses,
                             const float intrinsics_d[4], int level, float residual_gate /* 0 -> 0.75 */,
                             dslam_pose_score *scores_out /* [num_poses] */);
int dslam_track_camera_sdf_starts(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes,
                                  const float *T_map_from_world /* [num_maps][16] */, int num_maps,
                                  float *poses_M /* [num_starts][16]; in: starts, out: estimates */, int num_starts,
                                  const float intrinsics_d[4], const dslam_track_sdf_params *params /* NULL: defaults */,
                                  dslam_track_sdf_result *results /* [num_starts] */);
/* Test hook: the 33 raw sums of the last evaluation of start `start` in the engine's most recent
 * dslam_track_camera_sdf_starts -- what dslam_debug_track_sdf_sums gives after the single call from that start, its
 * entries pivoted at that evaluation's camera centre as stated there.  Error if
 * no such call has run or `start` is not one of its starts. */
int dslam_debug_track_sdf_start_sums(dslam_engine *e, int start, double out[33]);

/* Host only, callable without a device (as dslam_select_view_maps is).
 * dslam_select_start_poses: of scores[0 .. num), the poses with valid >= min_valid and a cost that is not NaN, ordered by
 * cost ascending (ties: the lower index first); the first max_keep of them go to kept_out, their number to num_kept_out.
 * DSLAM_ERR_INVALID: a NULL argument, num < 1, min_valid or max_keep negative. */
int dslam_select_start_poses(const dslam_pose_score *scores, int num, int min_valid, int max_keep,
                             int32_t *kept_out /* [max_keep] */, int32_t *num_kept_out);
/* dslam_camera_pose_lattice: poses on a lattice of camera centres and of rotations about one axis around pose_M (world ->
 * camera).  All arithmetic in double.  (R, c): the camera -> world rotation and the camera centre from the rigid inverse
 * of pose_M; a^ = axis / |axis|.  Node (ir, iz, iy, ix), ir in [-nr, nr], ia in [-nt[a], nt[a]] (nt[0] counts x), has the
 * centre c + step_t (ix, iy, iz) and the orientation Rot(a^, ir step_r) R (Rodrigues); its pose is the rigid inverse
 * (R'^T, -R'^T c'), rounded to float32.  Nodes are listed with ir slowest and ix fastest; the node with all indices 0 is
 * pose_M byte for byte.  count_out = (2 nr + 1)(2 nt[2] + 1)(2 nt[1] + 1)(2 nt[0] + 1) is always filled (0 when a count is
 * negative).  DSLAM_ERR_INVALID with poses_out untouched: a NULL argument, a count above capacity, a negative count or a
 * negative or non-finite step, a zero or non-finite axis with nr > 0, a non-finite pose_M or one whose rotation block is
 * not orthonormal to 1e-4. */
typedef struct {
  int32_t nt[3];                   /* translation nodes to each side, per axis x, y, z (world) */
  float step_t;                    /* metres */
  int32_t nr;                      /* rotation nodes to each side */
  float step_r;                    /* radians */
  float axis[3];                   /* world; need not be normalised */
  int32_t pad;
} dslam_pose_lattice;
int dslam_camera_pose_lattice(const float pose_M[16], const dslam_pose_lattice *l, float *poses_out /* [capacity][16] */,
                              int capacity, int32_t *count_out);

/* ---- state read-back (stats for the driver; bulk downloads for parity tests and checkpoints) ------ */
int dslam_get_stats(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, dslam_stats *out);
int dslam_download_hash_table(dslam_engine *e, const dslam_scene *s, dslam_hash_entry *out_host);
int dslam_download_voxel_blocks(dslam_engine *e, const dslam_scene *s, int first_block, int num_blocks,
                                dslam_voxel *out_host);
int dslam_download_allocation_list(dslam_engine *e, const dslam_scene *s, int32_t *out_host);
int dslam_download_excess_list(dslam_engine *e, const dslam_scene *s, int32_t *out_host);
int dslam_download_visible_ids(dslam_engine *e, const dslam_render_state *r, int32_t *out_host,
                               int capacity, int *out_count);
int dslam_download_visible_types(dslam_engine *e, const dslam_render_state *r, uint8_t *out_host);
int dslam_download_range_image(dslam_engine *e, const dslam_render_state *r, float *out_minmax_host);
int dslam_download_raycast_result(dslam_engine *e, const dslam_render_state *r, float *out_xyzw_host);
int dslam_download_view_depth(dslam_engine *e, const dslam_view *v, float *out_host);
/* the points / normals maps dslam_create_icp_maps left on the device (either pointer may be NULL) */
int dslam_download_icp_maps(dslam_engine *e, const dslam_render_state *r, float *out_points_host,
                            float *out_normals_host);
int dslam_download_swap_states(dslam_engine *e, const dslam_scene *s, uint8_t *out_host);
/* per voxel-block slot: newest global list index that holds the block (-1 never, <= -2 swept by Decay) */
int dslam_download_last_seen(dslam_engine *e, const dslam_scene *s, int32_t *out_host);
/* ITMGlobalCache::GetStoredVoxelBlock(entry): copies the host-stored block; returns 1 if the entry has
 * stored data, 0 if not */
int dslam_download_stored_block(dslam_engine *e, const dslam_scene *s, int entry, dslam_voxel *out_host);
/* scratch of the last allocation pass (entriesAllocType / blockCoords), for bit-exactness tests */
int dslam_download_alloc_scratch(dslam_engine *e, const dslam_scene *s, uint8_t *alloc_types_host,
                                 int16_t *block_coords_host);
/* upload a complete map state (hash table, pool free lists, voxel blocks): checkpoint restore and the
 * stress/roofline generator.  Any pointer may be NULL to keep that part. */
int dslam_upload_scene_state(dslam_engine *e, dslam_scene *s, const dslam_hash_entry *hash_host,
                             const int32_t *allocation_list_host, int last_free_block_id,
                             const int32_t *excess_list_host, int last_free_excess_id);
int dslam_upload_voxel_blocks(dslam_engine *e, dslam_scene *s, int first_block, int num_blocks,
                              const dslam_voxel *host);
int dslam_upload_visible_ids(dslam_engine *e, dslam_render_state *r, const int32_t *ids_host, int count);

/* raw device pointers (HBM layout is documented in DESIGN.md).
 * The hash table is READ-ONLY through this pointer: every pass that lists entries (visibility, decay, window, swapping,
 * meshing, FindVisibleBlocks) walks a bitmap that mirrors `ptr >= 0` of the table (alloc_bits) instead of the table, so an
 * entry written behind the engine's back exists but is never seen.  A caller that must patch or restore the table in
 * place calls dslam_scene_table_changed afterwards (the bitmap is rebuilt from the table: the one pass that reads all of
 * it); dslam_upload_scene_state does that by itself.  Voxel blocks may be written freely (they have no shadow). */
void *dslam_scene_voxel_blocks_dev(dslam_scene *s);
void *dslam_scene_hash_table_dev(dslam_scene *s);
int dslam_scene_table_changed(dslam_engine *e, dslam_scene *s);
void *dslam_render_state_image_dev(dslam_render_state *r, int want_float);

/* ---- sharded re-integration (multi-GPU) ------------------------------------------------ */
/* Restrict the voxel-writing kernels (integrate / de-integrate) of this scene to the voxel-block slots
 * whose chunk (slot / chunk_blocks) satisfies chunk % num_shards == shard; allocation stays global
 * (and bit-identical on every rank).  num_shards = 1 disables sharding.  A scene with host swapping cannot be sharded
 * (DSLAM_ERR_INVALID): every rank would swap its own, partly stale copies out to its own host store, which the block
 * exchange does not cover.  (The reference never turns swapping on: its ITMLibSettings is default-constructed.) */
int dslam_scene_set_shard(dslam_scene *s, int shard, int num_shards, int chunk_blocks);
/* Same, with a contiguous slot range [first_block, first_block + num_blocks): the layout an in-place RCCL
 * all-gather over the voxel-block array needs.  num_blocks < 0 disables. */
int dslam_scene_set_shard_range(dslam_scene *s, int first_block, int num_blocks);
/* The exchange for a batch whose blocks may sit ANYWHERE in the pool (after decay, the sliding window or swapping have
 * returned slots to the free list in arbitrary order, the used slots are no longer a top range): move exactly the blocks
 * the batch touched.  Allocation is replicated and bit-identical on every rank, and the (de-)integration kernels mark
 * every visible resident block they walk over BEFORE their shard test, so all ranks hold the same marks and derive the
 * same per-shard lists of dirty slots -- no ids travel, no counts are exchanged:
 *   dslam_scene_track_dirty(e, s, 1)            clear the marks, start marking         (before the batch)
 *   ... the batch: dslam_deprocess_frame / dslam_process_frame under dslam_scene_set_shard(rank, world, chunk) ...
 *   dslam_shard_dirty_plan(e, s, world, chunk, counts)   counts[r] = dirty blocks of shard r, identical on all ranks
 *   dslam_shard_dirty_pack(e, s, rank, send, cap)        this rank's dirty blocks, ascending in slot, 4096 B each
 *   ncclAllGather(send, recv, cap * 4096 bytes) with cap = max(counts)   (the one collective)
 *   dslam_shard_dirty_unpack(e, s, rank, recv, cap)      every other shard's blocks into place
 *   dslam_scene_track_dirty(e, s, 0)
 * num_local_blocks must be a multiple of world * chunk; world <= 64. */
int dslam_scene_track_dirty(dslam_engine *e, dslam_scene *s, int enable);
int dslam_shard_dirty_plan(dslam_engine *e, dslam_scene *s, int num_shards, int chunk_blocks, int32_t *counts_out);
int dslam_shard_dirty_pack(dslam_engine *e, const dslam_scene *s, int shard, void *send_dev, int capacity_blocks);
int dslam_shard_dirty_unpack(dslam_engine *e, dslam_scene *s, int skip_shard, const void *recv_dev, int stride_blocks);

/* ---- instrumentation ---------------------------------------------------------------------------- */
/* Time `iterations` back-to-back launches of the integrate kernel alone on the engine stream with HIP
 * events (state is restored afterwards is NOT guaranteed: use on a scratch scene).  Returns the mean
 * milliseconds per launch and the number of visible blocks processed per launch. */
int dslam_time_integrate(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_render_state *r,
                         const float M_d[16], const float intrinsics_d[4], int iterations,
                         float *out_ms_per_launch, int *out_visible_blocks);
/* accumulated HIP-event time of the integrate kernel launched by dslam_process_frame /
 * dslam_integrate_into_scene since the last reset (events are recorded only while enabled). */
int dslam_kernel_timer_enable(dslam_engine *e, int enable);
int dslam_kernel_timer_read(dslam_engine *e, double *out_integrate_ms, int64_t *out_launches,
                            int64_t *out_visible_blocks);

#ifdef __cplusplus
}
#endif
#endif /* DSLAM_FUSION_H */
