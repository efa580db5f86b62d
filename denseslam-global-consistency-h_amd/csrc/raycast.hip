// raycast.hip -- ITMVisualisationEngine for gfx950: FindVisibleBlocks, CountVisibleBlocks,
// CreateExpectedDepths, RenderImage (raycast + shading), CreateICPMaps.
//
// Reference call sites: ITMMainEngine::GetImage via InfiniTamDriver::GetImage / GetFloatImage
// (InfiniTamDriver.cpp:229-277, types :16-38), trackingController->Prepare (InfiniTamDriver.h:208-220),
// mapManager->countVisibleBlocks (DenseSlam.cpp:555-556).  Algorithm: SURVEY.md Appendix A.6, A.7.
//
// Mapping: the ray march is latency/gather bound (random 16-B hash probes + 8-B voxel reads).  One wavefront (= one
// workgroup) renders an 8x8 pixel tile, i.e. exactly one cell of the 1/8-resolution range image, so (zmin, zmax)
// and -- mostly -- the marched blocks are wave-uniform.
//
// The instantiations of k_render<SHADE, DIAG, REUSE> and the calls that reach them (launch_render unless said otherwise):
//   <false>               march, and the depth image if asked for: type < 0 or DSLAM_IMAGE_DEPTH; launch_icp_maps
//   <true>                march + one of the three shaded types
//   <false, false, true>  GetImage memo hit (reuse_raycast): depth image from the stored raycast result
//   <true, false, true>   GetImage memo hit: a shaded type from the stored raycast result
//   <false, true>         diagnostics: the one launch that DSLAM_DBG_WAVETIME dumps (march with per-wave cycle counts)
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "dslam_bits.h"
#include "raycast_device.h"

#pragma clang fp contract(off)

namespace dslam {


// ---------------------------------------------------------------------------------------------------------
// CountVisibleBlocks
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_count_visible(const int *__restrict__ ids, RenderCounters *rc,
                                                       const HashEntry *__restrict__ hash, int min_id, int max_id) {
  const int n = rc->no_visible;
  int c = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int ptr = hash[ids[i]].ptr;
    c += (ptr >= min_id && ptr <= max_id);
  }
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&rc->count_result, c);
}

int launch_count_visible(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, int min_id, int max_id,
                         int *out) {
  DSLAM_HIP(hipMemsetAsync(&r->counters->count_result, 0, sizeof(int), e->stream));
  hipLaunchKernelGGL(k_count_visible, dim3(128), dim3(256), 0, e->stream, r->visible_ids, r->counters, s->hash, min_id,
                     max_id);
  int *host = reinterpret_cast<int *>(e->pinned.get());
  DSLAM_HIP(hipMemcpyAsync(host, &r->counters->count_result, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  *out = *host;
  return DSLAM_OK;
}


int launch_find_visible(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                        const float *intr) {
  const int N = s->n_entries;
  DSLAM_REQUIRE(r->n_entries == N, "render state was created for a different scene size");
  int rc = ensure_scratch(e, N, s->p.num_local_blocks);
  if (rc) return rc;
  SelFrustum<false> sel{s->hash, make_frustum_params(s, r, M, intr), nullptr, nullptr, nullptr, nullptr, 0};
  launch_bits_select(e, s->alloc_bits, N, sel, r->visible_ids, r->n_local, &r->counters->no_visible, s->counters);
  DSLAM_HIP(hipGetLastError());
  return DSLAM_OK;
}

// ProjectSingleBlock for every visible block; records bbox / z-range / required render tiles
__global__ __launch_bounds__(256) void k_project_blocks(const int *__restrict__ ids, RenderCounters *rc,
                                                        const HashEntry *__restrict__ hash, ProjParams p,
                                                        int4 *__restrict__ boxes, float2 *__restrict__ zr_out,
                                                        int *req_out, float2 *range, int npix, int *wg_tiles) {
  __shared__ int s_tiles;
  if (threadIdx.x == 0) s_tiles = 0;
  __syncthreads();
  // (independent job in the same launch) reset the range image to (FAR_AWAY, VERY_CLOSE)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x)
    range[i] = make_float2(kFarAway, kVeryClose);
  const int n = rc->no_visible;
  int local_tiles = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const HashEntry e = load_entry(hash, ids[i]);
    int4 box;
    float2 zr;
    const int req = project_single_block(e, p, box, zr);
    if (req) { boxes[i] = box; zr_out[i] = zr; }
    req_out[i] = req;
    local_tiles += req;
  }
  for (int d = 32; d > 0; d >>= 1) local_tiles += __shfl_down(local_tiles, d, 64);
  if ((threadIdx.x & 63) == 0 && local_tiles) atomicAdd(&s_tiles, local_tiles);
  __syncthreads();
  // per-workgroup totals instead of one contended global counter; the range-image kernel sums them
  if (threadIdx.x == 0) wg_tiles[blockIdx.x] = s_tiles;
}

// Fill the range image.  The render tiles of a block partition its bbox, so min/max over the bbox is identical to
// upstream's tile list.  Values are positive floats, so integer min/max on the bit patterns order correctly.
//
// Corner pass (the ceil(W/8) x ceil(H/8) cells the raycaster reads): one workgroup = one 16x16-cell tile x one chunk
// slice of the visible list.  Overlapping blocks are accumulated with LDS atomics (ds_min/ds_max), then every touched cell
// is flushed with ONE global atomic pair -- instead of one contended global atomic pair per (block, cell).
constexpr int kRangeTile = 16;
constexpr int kRangeSlices = 32;   // workgroups per tile; each strides over the visible list
constexpr int kRangeBigBox = 32;   // cells of a tile above which a box is taken by the whole workgroup

__global__ __launch_bounds__(256) void k_fill_range_tiles(const RenderCounters *rc, const int4 *__restrict__ boxes,
                                                          const float2 *__restrict__ zr, const int *__restrict__ req,
                                                          float2 *range, int W, int tiles_x,
                                                          const int *__restrict__ wg_tiles, int n_wg_tiles, int budget,
                                                          int capacity, unsigned *start_stamp, unsigned stamp) {
  __shared__ int s_min[kRangeTile * kRangeTile], s_max[kRangeTile * kRangeTile];
  __shared__ int red[4];
  // GetImage's range pass tells the host that it has STARTED (one lane, one ordinary store to a page-locked word): the stream
  // runs its launches in order, so everything enqueued in front of this one is complete
  if (start_stamp && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    __hip_atomic_store(start_stamp, stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // The visible count, the per-workgroup tile totals and this lane's first list entry are all fetched before anything
  // waits: four dependent round trips become one (the entry is read speculatively -- the index is inside the
  // buffers whatever the count turns out to be).
  const int i0 = blockIdx.y * 256 + threadIdx.x;
  int r0 = 0;
  int4 b0 = make_int4(0, 0, 0, 0);
  float2 z0 = make_float2(0.0f, 0.0f);
  if (i0 < capacity) { r0 = req[i0]; b0 = boxes[i0]; z0 = zr[i0]; }
  const int n = __builtin_amdgcn_readfirstlane(rc->no_visible);   // (uniform, and the compiler should know: a loop with barriers hangs off it)
  // The render-tile budget (MAX_RENDERING_BLOCKS) is applied in visible-list order; only when the total (the sum of
  // the projection pass' per-workgroup counts) exceeds it does the order matter.  That case (> 262144 tiles) is
  // replayed below, by every workgroup for itself.
  const bool over_budget = block_sum_strided(wg_tiles, n_wg_tiles, 1, red) >= budget;
  if ((int)(blockIdx.y * 256) >= n && !over_budget) return;
  const int tx0 = (blockIdx.x % tiles_x) * kRangeTile, ty0 = (blockIdx.x / tiles_x) * kRangeTile;
  const int far_i = __float_as_int(kFarAway), close_i = __float_as_int(kVeryClose);
  s_min[threadIdx.x] = far_i;
  s_max[threadIdx.x] = close_i;
  __syncthreads();
  auto splat_box = [&](const int4 &b, const float2 &z) {
    const int x0 = b.x > tx0 ? b.x : tx0, x1 = b.z < tx0 + kRangeTile - 1 ? b.z : tx0 + kRangeTile - 1;
    const int y0 = b.y > ty0 ? b.y : ty0, y1 = b.w < ty0 + kRangeTile - 1 ? b.w : ty0 + kRangeTile - 1;
    if (x0 > x1 || y0 > y1) return;
    const int zmin_i = __float_as_int(z.x), zmax_i = __float_as_int(z.y);
    for (int y = y0; y <= y1; y++)
      for (int x = x0; x <= x1; x++) {
        const int c = (x - tx0) + (y - ty0) * kRangeTile;
        atomicMin(&s_min[c], zmin_i);
        atomicMax(&s_max[c], zmax_i);
      }
  };
  auto splat = [&](int i) { splat_box(boxes[i], zr[i]); };
  if (!over_budget) {
    // A box that covers many cells of this tile (a block next to the camera: up to all 256) is not walked by the lane that
    // holds it -- 2 x 256 LDS atomics one after the other while the lanes with distant blocks are done after a handful --
    // but queued, and taken by the whole workgroup: thread c looks at cell c of the tile, in registers.
    __shared__ int4 s_big[256];
    __shared__ int2 s_bigz[256];
    __shared__ int s_nbig;
    int mn_c = far_i, mx_c = close_i;
    const int cx = tx0 + (threadIdx.x % kRangeTile), cy = ty0 + (threadIdx.x / kRangeTile);
    auto take = [&](bool have, const int4 &b, const float2 &z) {
      if (threadIdx.x == 0) s_nbig = 0;
      __syncthreads();
      if (have) {
        const int x0 = b.x > tx0 ? b.x : tx0, x1 = b.z < tx0 + kRangeTile - 1 ? b.z : tx0 + kRangeTile - 1;
        const int y0 = b.y > ty0 ? b.y : ty0, y1 = b.w < ty0 + kRangeTile - 1 ? b.w : ty0 + kRangeTile - 1;
        if (x0 <= x1 && y0 <= y1) {
          if ((x1 - x0 + 1) * (y1 - y0 + 1) > kRangeBigBox) {
            const int k = atomicAdd(&s_nbig, 1);
            s_big[k] = make_int4(x0, y0, x1, y1);
            s_bigz[k] = make_int2(__float_as_int(z.x), __float_as_int(z.y));
          } else {
            splat_box(b, z);
          }
        }
      }
      __syncthreads();
      const int nb = s_nbig;
      for (int k = 0; k < nb; k++) {
        const int4 bb = s_big[k];
        const int2 zz = s_bigz[k];
        if (cx >= bb.x && cx <= bb.z && cy >= bb.y && cy <= bb.w) {
          mn_c = zz.x < mn_c ? zz.x : mn_c;
          mx_c = zz.y > mx_c ? zz.y : mx_c;
        }
      }
      __syncthreads();   // (the queue is refilled by the next round)
    };
    take(i0 < n && r0 != 0, b0, z0);
    for (int ib = blockIdx.y * 256 + gridDim.y * 256; ib < n; ib += gridDim.y * 256) {   // (uniform trip count: barriers inside)
      const int i = ib + threadIdx.x;
      const bool have = i < n && req[i] != 0;
      int4 b = make_int4(0, 0, -1, -1);
      float2 z = make_float2(0.0f, 0.0f);
      if (have) { b = boxes[i]; z = zr[i]; }
      take(have, b, z);
    }
    if (mn_c != far_i) atomicMin(&s_min[threadIdx.x], mn_c);
    if (mx_c != close_i) atomicMax(&s_max[threadIdx.x], mx_c);
  } else {
    // sequential rule of the reference's tile list: entry i is dropped when the tiles accepted so far plus its own
    // reach the budget (a dropped entry does not count).  Chunks of the request list are staged in LDS, lane 0
    // replays them in order, then the lanes splat the accepted entries of this workgroup's slice.
    __shared__ int s_req[1024];
    __shared__ unsigned char s_keep[1024];
    __shared__ int s_num;
    if (threadIdx.x == 0) s_num = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
      __syncthreads();
      for (int j = threadIdx.x; j < 1024; j += 256) s_req[j] = (c0 + j < n) ? req[c0 + j] : 0;
      __syncthreads();
      if (threadIdx.x == 0) {
        int num = s_num;
        for (int j = 0; j < 1024; j++) {
          const int r = s_req[j];
          bool keep = r != 0;
          if (keep) {
            if (num + r >= budget) keep = false;
            else num += r;
          }
          s_keep[j] = keep;
        }
        s_num = num;
      }
      __syncthreads();
      for (int j = threadIdx.x; j < 1024; j += 256) {
        const int i = c0 + j;
        // this workgroup's slice of the list, as in the common path: i = blockIdx.y * 256 + t (mod gridDim.y * 256)
        if (i < n && s_keep[j] && (i / 256) % (int)gridDim.y == (int)blockIdx.y) splat(i);
      }
    }
  }
  __syncthreads();
  const int mn = s_min[threadIdx.x], mx = s_max[threadIdx.x];
  if (mn != far_i || mx != close_i) {
    const int x = tx0 + (threadIdx.x % kRangeTile), y = ty0 + (threadIdx.x / kRangeTile);
    int *px = reinterpret_cast<int *>(&range[x + (size_t)y * W]);
    if (mn != far_i) atomicMin(&px[0], mn);
    if (mx != close_i) atomicMax(&px[1], mx);
  }
}

// Cells outside that corner: upstream clamps bboxes to the full image size although coordinates are 1/8 scale, so
// blocks near the camera spill thousands of cells past the corner.  Nothing ever reads them (castRay indexes
// floor(x/8) + floor(y/8) * W), so they are not filled here; tests compare the corner.

constexpr int kProjectGrid = 512;

// stamped: the pass is GetImage's, and an asynchronous engine that overlaps k_mark wants to hear of its start
static int launch_fill_range(dslam_engine *e, dslam_render_state *r, int n_wg_tiles, bool stamped = false) {
  // corner = the tiles covering ceil(W/8) x ceil(H/8) cells (clamped to the image); chunks sized for the pool
  const int cw = (r->w + 7) / 8, ch = (r->h + 7) / 8;
  const int tiles_x = (cw + kRangeTile - 1) / kRangeTile, tiles_y = (ch + kRangeTile - 1) / kRangeTile;
  unsigned *stamp_word = nullptr;
  if (stamped && e->overlap_mark && e->async_mode) {
    stamp_word = e->start_stamp;
    if (++e->stamp_seq == 0) e->stamp_seq = 1;   // (0 is the word's value before the first stamp)
    e->stamp_view_reads = e->view_reads;   // (every call that read a view so far has its kernels in front of this pass)
  }
  hipLaunchKernelGGL(k_fill_range_tiles, dim3(tiles_x * tiles_y, kRangeSlices), dim3(256), 0, e->stream, r->counters,
                     r->proj_boxes, r->proj_z, r->proj_req, r->range, r->w, tiles_x, r->proj_wg_tiles, n_wg_tiles,
                     e->render_tile_budget, r->n_local, stamp_word, e->stamp_seq);
  DSLAM_HIP(hipGetLastError());
  return DSLAM_OK;
}


int launch_expected_depths(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                           const float *intr) {
  const ProjParams pp = make_proj_params(s, r, M, intr);
  hipLaunchKernelGGL(k_project_blocks, dim3(kProjectGrid), dim3(256), 0, e->stream, r->visible_ids, r->counters, s->hash,
                     pp, r->proj_boxes, r->proj_z, r->proj_req, r->range, r->w * r->h, r->proj_wg_tiles);
  return launch_fill_range(e, r, kProjectGrid);
}

// FindVisibleBlocks + CreateExpectedDepths for the same pose (ITMMainEngine::GetImage's FREECAMERA path): three launches
// (round 1: five), none of which reads the table as a whole any more.
int launch_find_visible_and_depths(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                                   const float *intr) {
  const int N = s->n_entries;
  DSLAM_REQUIRE(r->n_entries == N, "render state was created for a different scene size");
  int rc = ensure_scratch(e, N, s->p.num_local_blocks);
  if (rc) return rc;
  // A front end still in flight on aux_stream is sat out first, adopted or not: the range image must be
  // complete before the march is enqueued, and a selection of this call's own would share the per-tile words with it.
  DSLAM_TRY(settle_front(e));
  // The last ProcessFrame computed this selection already (FrontEndRecord): same map, pose, intrinsics and image size.  The
  // render state takes its buffers -- the list, its count, the projections, the per-tile totals, the reset range image --
  // and gives its own in exchange (the same sizes), all on the engine's one stream.
  if (FrontEndRecord *f = s->front.get()) {
    if (f->valid && f->version == s->version && f->w == r->w && f->h == r->h && f->n_local == r->n_local &&
        f->n_entries == r->n_entries && memcmp(f->M, M, sizeof(f->M)) == 0 && memcmp(f->intr, intr, sizeof(f->intr)) == 0) {
      std::swap(r->visible_ids, f->visible_ids);
      std::swap(r->counters, f->counters);
      std::swap(r->proj_boxes, f->proj_boxes);
      std::swap(r->proj_z, f->proj_z);
      std::swap(r->proj_req, f->proj_req);
      std::swap(r->proj_wg_tiles, f->proj_wg_tiles);
      std::swap(r->range, f->range);
      f->valid = false;
      e->front_adoptions++;
      if (f->range_filled) {
        // A complete record: the range image the render state just took was filled on aux_stream.  The march
        // may only be enqueued once that stream has drained (settle_front above), and it carries the start stamp, as the
        // first kernel this call puts on the engine stream behind the fusion launch.
        f->range_filled = false;
        e->stamp_due = true;
        return DSLAM_OK;
      }
      return launch_fill_range(e, r, select_tiles(N), true);
    }
  }
  SelFrustum<true> sel{s->hash, make_frustum_params(s, r, M, intr), r->proj_boxes, r->proj_z, r->proj_req, r->range, r->w * r->h};
  DSLAM_TRY(launch_bits_select(e, s->alloc_bits, N, sel, r->visible_ids, r->n_local, &r->counters->no_visible, s->counters, r->proj_wg_tiles));
  return launch_fill_range(e, r, select_tiles(N), true);
}


// GetImage's front end for the pose of a ProcessFrame whose sweep ran on aux_stream: the same k_bits_select
// over alloc_bits as above (4 entries per lane) and the same range pass, into the scene's FrontEndRecord, on aux_stream behind
// that sweep -- beside k_publish_entries and the plain fusion launch, which the engine stream holds.  The selection reads the
// table but sees the entries the sweep created through hidden_pos (SelFrustum<true, true>); nothing here writes the table.
// Tickets come from the auxiliary stream's word (ticket + 2), errors go to a page-locked word of the selection's own
// (err_host[3]); the range pass carries no stamp.  The host waits for the stream in settle_front.
int launch_front_end_aux(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, const float *M, const float *intr,
                         FrontEndRecord *f) {
  const int N = s->n_entries;
  DSLAM_TRY(ensure_scratch(e, N, s->p.num_local_blocks));
  SelFrustum<true, true> sel{s->hash, make_frustum_params(s, r, M, intr), f->proj_boxes, f->proj_z, f->proj_req, f->range, r->w * r->h,
                             e->hidden_pos};
  const int n_tiles = select_tiles(N);
  TileChain ch;
  (void)tickets_ok(e);
  if (++e->epoch == 0) e->epoch = 1;
  ch.agg = e->agg + 2 * (size_t)e->agg_tiles;   // (the third channel: no launch of the engine stream publishes through it)
  ch.epoch = e->epoch;
  ch.ticket = e->ticket + 2; ch.ticket_base = e->ticket_base3;
  ch.n_tiles = n_tiles;
  ch.dbg = nullptr;
  ch.err_word = e->err_host ? e->err_host.get() + 3 : nullptr;
  ch.start_word = e->sweep_done_seq ? e->start_stamp.get() + 1 : nullptr;   // (the held tail waits for the sweep in front: alloc.hip)
  ch.start_value = e->sweep_done_seq;
  const int grid = n_tiles > 0 ? n_tiles : 1;
  e->ticket_base3 += (unsigned)grid;
  hipLaunchKernelGGL((k_bits_select<SelFrustum<true, true>>), dim3(grid), dim3(kSelThreads), 0, e->aux_stream, s->alloc_bits.get(), sel,
                     f->visible_ids.get(), r->n_local, &f->counters->no_visible, f->proj_wg_tiles.get(), ch, s->counters.get());
  DSLAM_HIP(hipGetLastError());
  const int cw = (r->w + 7) / 8, chh = (r->h + 7) / 8;
  const int tiles_x = (cw + kRangeTile - 1) / kRangeTile, tiles_y = (chh + kRangeTile - 1) / kRangeTile;
  hipLaunchKernelGGL(k_fill_range_tiles, dim3(tiles_x * tiles_y, kRangeSlices), dim3(256), 0, e->aux_stream, f->counters.get(),
                     f->proj_boxes.get(), f->proj_z.get(), f->proj_req.get(), f->range.get(), r->w, tiles_x, f->proj_wg_tiles.get(), n_tiles,
                     e->render_tile_budget, r->n_local, (unsigned *)nullptr, 0u);
  DSLAM_HIP(hipGetLastError());
  e->front_pending = true;
  f->range_filled = true;
  return DSLAM_OK;
}

int settle_front(dslam_engine *e) {
  if (!e->front_pending) return DSLAM_OK;
  e->front_pending = false;
  DSLAM_HIP(hipStreamSynchronize(e->aux_stream));
  return DSLAM_OK;
}

// ---------------------------------------------------------------------------------------------------------
// castRay + shading, one kernel
// ---------------------------------------------------------------------------------------------------------
struct RenderParams {
  VolumeRef vol;
  RayCamera cam;
  unsigned *start_stamp;   // non-null: the march of a GetImage that adopted a complete front-end record -- the
  unsigned stamp;          // first kernel of the call on the engine stream, so IT tells the host that it has started
  unsigned long long *dbg_waves;  // diagnostics only (env DSLAM_DBG_WAVETIME=<file>): per wave {cycles, max iterations, straddling iterations, their cycles, setup cycles, refinement cycles}
  float split_len;  // > 0: tiles with a longer depth range (voxels) are marched by two wavefronts; the grid is (W/8, 2 H/8)
};

constexpr float kSplitLen = 175.0f;  // voxels of depth range above which a tile is marched by two wavefronts (150-200 measure the same)

// DIAG instantiation only: wave-level split of the march (single-wave workgroups): iterations in which some lane took
// the straddling-cell path, and the cycles of those iterations
struct MarchDiag { int iters, wave_iters, slow_iters; unsigned long long slow_cycles, setup_cycles, tail_cycles; };

template <bool DIAG>
__device__ __forceinline__ bool cast_ray(Vec4 &out, int x, int y, const RenderParams &p, const float2 minmax,
                                         MarchDiag &diag) {
  const unsigned long long t_enter = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
  const RayCamera &c = p.cam;
  float sdf = 1.0f;
  const float step_scale = c.mu * c.one_over_vs;
  const RaySegment seg = ray_segment(c, x, y, minmax);
  const Vec3 dir = seg.dir;
  Vec3 res = seg.start;
  float total = seg.total, step;
  const float total_max = seg.total_max;
  IndexCache cache = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
  int iter = 0;
  unsigned long long t_iter = 0;
  int *slow_flag = nullptr;  // DIAG: some lane of the wave took the straddling-cell path in this iteration
  if constexpr (DIAG) {
    __shared__ int s_slow_flag;
    slow_flag = &s_slow_flag;
    diag.slow_iters = 0; diag.wave_iters = 0; diag.slow_cycles = 0;
    diag.setup_cycles = __builtin_amdgcn_s_memtime() - t_enter;
    *slow_flag = 0;
    t_iter = __builtin_amdgcn_s_memtime();
  }
  while (total < total_max) {
    ++iter;
    if (DIAG) {  // account the previous wave iteration
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      if (iter > 1) {
        diag.wave_iters++;
        if (*slow_flag) { diag.slow_iters++; diag.slow_cycles += now - t_iter; }
      }
      *slow_flag = 0;
      t_iter = now;
    }
    // Measured on MI355X (DSLAM_DBG_WAVETIME dump): the launch keeps only ~1.1 waves per SIMD resident on average
    // and ends when its longest wave ends, and a lone wave64 issues one VALU instruction per 4 cycles -- a step costs
    // its load round trips (~700 cycles each) PLUS 4 cycles for every instruction ANY lane of the wave executes.
    // Hence: (a) the common step is kept short -- one probe for the block of the nearest voxel ROUND(p), then the
    // 8 taps of the trilinear cell floor(p)..floor(p)+1 in one batch from THAT block (in-block offsets wrap, so the
    // loads are unconditional; all 8 taps lie in it at 67 % of the positions, ROUND(p) always does); (b) the
    // uncommon step -- near the surface with the cell straddling blocks -- resolves all its blocks in one further
    // round trip and re-reads the taps in a second (read_sdf_interp_batched), instead of readFromSDF_float_
    // interpolated's eight lookups one after the other.  Variants that add loads or instructions to the common
    // step (bitmap, prefetch, speculation, resolving the whole cell every step) all measured slower.
    const int vx = iround(res.x), vy = iround(res.y), vz = iround(res.z);
    const int bx = vx >> 3, by = vy >> 3, bz = vz >> 3;
    const int base = lookup_block(p.vol, bx, by, bz, cache);
    if (base < 0) {
      sdf = 1.0f;  // empty voxel: 32767 / 32767
      step = (float)kBlock;
    } else {
      const float f0x = floorf(res.x), f0y = floorf(res.y), f0z = floorf(res.z);
      const int x0 = (int)f0x, y0 = (int)f0y, z0 = (int)f0z;
      unsigned raw[8];
      // The 8 taps as 32-bit byte offsets from the (uniform) voxel array: one or3 + one shift-add per tap and the
      // load takes the scalar base.  A tap that belongs to a neighbouring block still reads a valid address inside
      // this block; its value is only used when all 8 taps are inside (all_in).
      const unsigned lx[2] = {(unsigned)x0 & 7u, (unsigned)(x0 + 1) & 7u};
      const unsigned ly[2] = {((unsigned)y0 & 7u) << 3, ((unsigned)(y0 + 1) & 7u) << 3};
      const unsigned lz[2] = {((unsigned)z0 & 7u) << 6, ((unsigned)(z0 + 1) & 7u) << 6};
      const char *vbytes = reinterpret_cast<const char *>(p.vol.voxels);
      const unsigned off0 = (unsigned)base * 8u;  // base < 2^29 voxels -> < 2^32 bytes (DSLAM_MAX_LOCAL_BLOCKS)
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const unsigned off = off0 + ((lx[k & 1] | ly[(k >> 1) & 1] | lz[k >> 2]) << 3);
        raw[k] = *reinterpret_cast<const unsigned *>(vbytes + off);  // unconditional, batched
      }
      // nearest voxel ROUND(p) = tap (vx - x0, vy - y0, vz - z0): a 3-level select tree
      const bool nx = vx != x0, ny = vy != y0, nz = vz != z0;
      const unsigned r01 = nx ? raw[1] : raw[0], r23 = nx ? raw[3] : raw[2];
      const unsigned r45 = nx ? raw[5] : raw[4], r67 = nx ? raw[7] : raw[6];
      const unsigned rn = nz ? (ny ? r67 : r45) : (ny ? r23 : r01);
      sdf = div_exact((float)(short)(rn & 0xffffu), 32767.0f, c.inv_32767);
      if ((sdf <= 0.1f) && (sdf >= -0.5f)) {
        const bool all_in = (x0 >> 3) == bx && ((x0 + 1) >> 3) == bx && (y0 >> 3) == by && ((y0 + 1) >> 3) == by &&
                            (z0 >> 3) == bz && ((z0 + 1) >> 3) == bz;
        if (!all_in) {  // the cell straddles blocks: fetch it properly
          if (DIAG) *slow_flag = 1;
          gather_taps_batched(p.vol, x0, y0, z0, raw);
        }
        sdf = trilinear_raw(raw, res.x - f0x, res.y - f0y, res.z - f0z);
      }
      if (sdf <= 0.0f) break;
      step = fmaxf(sdf * step_scale, 1.0f);
    }
    res.x += step * dir.x; res.y += step * dir.y; res.z += step * dir.z;
    total += step;
  }
  diag.iters = iter;
  const unsigned long long t_tail = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
  const bool pt_found = refine_hit(out, res, dir, sdf, step_scale,
                                   [&](const Vec3 &pt) { return read_sdf_interp_batched(p.vol, pt); });
  if (DIAG) diag.tail_cycles = __builtin_amdgcn_s_memtime() - t_tail;
  return pt_found;
}

// SHADE = false: raycast only / depth image -- the variant the fusion loop and the tracker use; it carries no
// shading code, which keeps it at <= 64 VGPRs = 8 waves per SIMD (the march is latency-bound, occupancy is what
// hides its load round trips).  SHADE = true adds the normal / colour modes.
// REUSE = true: raycastResult already holds this very view's march (GetImage memo) -- shade only.
template <bool SHADE, bool DIAG = false, bool REUSE = false>
__global__ __launch_bounds__(64, 5) void k_render(RenderParams rp) {
  const RayCamera &p = rp.cam;
  // (what the stamp proves is what it proved on the range pass, DESIGN.md 4g: everything enqueued in front of this launch is complete)
  if (rp.start_stamp && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    __hip_atomic_store(rp.start_stamp, rp.stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // one wavefront = one workgroup = an 8x8 pixel tile = exactly one cell of the 1/8-resolution range image.
  // Single-wave workgroups let the dispatcher backfill a SIMD the moment a short tile finishes (ray lengths vary
  // by 10x between tiles), instead of holding 4 waves until the slowest of a 16x16 tile is done.
  const int lane = threadIdx.x & 63;
  // (measured: dealing each XCD a contiguous band of tiles for L2 locality is slower, 104 vs 100 us -- the long
  // rays of one image region then pile up on one XCD; the march is bound by its longest dependent-load chain)
  const int x = blockIdx.x * 8 + (lane & 7);
  int y = blockIdx.y * 8 + (lane >> 3);
  if (rp.split_len > 0.0f) {
    // The launch ends when its longest wavefront ends, and a step of a wavefront costs the union of what its rays do
    // (measured: the first 32 steps of the longest tile, all 64 rays alive, take twice as long as its last 36).  So a
    // tile whose rays have far to go -- depth range of its cell of the range image, in voxels -- is marched by TWO
    // wavefronts of 32 rays (upper / lower four rows): 78 -> 70 us on the bench scene.  Splitting every tile loses
    // (throughput: 9600 half-empty waves), 16 rays per wave loses; the grid has two workgroups per tile and the second
    // one of an unsplit tile leaves at once.  Rays are independent: the images do not change.
    const int ty = blockIdx.y >> 1, sub = blockIdx.y & 1;
    const float2 mm = p.range[(int)blockIdx.x + ty * p.W];
    const bool split = (mm.y - mm.x) * p.one_over_vs > rp.split_len;
    if (split ? (lane >= 32) : (sub != 0)) return;
    y = ty * 8 + (split ? sub * 4 : 0) + (lane >> 3);
    // (the launch ends with these wavefronts: while short tiles share their SIMDs they issue first -- 138.2 -> 137.5 us per frame,
    // four alternations, every run of the one below every run of the other)
    if (split) __builtin_amdgcn_s_setprio(3);   // (a second level -- tiles half as long at priority 2 -- measures the same)
  }
  if (x >= p.W || y >= p.H) return;
  const int loc = x + y * p.W;
  const int loc2 = (int)floorf((float)x / 8.0f) + (int)floorf((float)y / 8.0f) * p.W;
  Vec4 pr;
  MarchDiag diag;
  const unsigned long long t_start = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
  if (REUSE) {
    const float4 q = p.raycast[loc];
    pr.x = q.x; pr.y = q.y; pr.z = q.z; pr.w = q.w;
  } else {
    cast_ray<DIAG>(pr, x, y, rp, p.range[loc2], diag);
  }
  if (DIAG) {  // diagnostic instantiation (DSLAM_DBG_WAVETIME): per-wave cycles and march length
    const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_start;
    // the lane with the longest march saw every wave iteration
    int mx = diag.iters;
    for (int d = 32; d > 0; d >>= 1) { const int o = __shfl_xor(mx, d, 64); mx = mx > o ? mx : o; }
    if (diag.iters == mx) {  // (several lanes may tie; they write the same values)
      const int wid = blockIdx.y * gridDim.x + blockIdx.x;
      rp.dbg_waves[6 * wid] = dt;
      rp.dbg_waves[6 * wid + 1] = (unsigned long long)mx;
      rp.dbg_waves[6 * wid + 2] = (unsigned long long)diag.slow_iters;
      rp.dbg_waves[6 * wid + 3] = diag.slow_cycles;
      rp.dbg_waves[6 * wid + 4] = diag.setup_cycles;
      rp.dbg_waves[6 * wid + 5] = diag.tail_cycles;
    }
  }
  if (!REUSE) p.raycast[loc] = make_float4(pr.x, pr.y, pr.z, pr.w);
  if (p.type < 0) return;

  IndexCache c = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};  // (the colour read starts from the normal's last block)
  store_pixel<SHADE>(p, loc, pr, [&](const Vec3 &pt) { return normal_from_sdf(rp.vol, pt, c); },
                     [&](const Vec3 &pt) { return read_colour_interp(rp.vol, pt, c); });
}

int fill_ray_camera(RayCamera &c, const dslam_scene *s, const dslam_render_state *r, const float *M, const float *intr,
                    int type, void *image_out_override) {
  memcpy(c.M.m, M, 64);
  if (!invert_matrix(M, c.invM.m)) { set_last_error("pose matrix is singular"); return DSLAM_ERR_INVALID; }
  c.inv_fx = 1.0f / intr[0]; c.inv_fy = 1.0f / intr[1]; c.cx = intr[2]; c.cy = intr[3];
  c.voxel_size = s->p.voxel_size; c.one_over_vs = 1.0f / s->p.voxel_size; c.mu = s->p.mu;
  c.inv_32767 = 1.0f / 32767.0f;
  c.W = r->w; c.H = r->h;
  c.range = r->range; c.raycast = r->raycast; c.out_rgba = r->image_rgba; c.out_float = r->image_float;
  c.type = type;
  if (image_out_override) {
    if (type == DSLAM_IMAGE_DEPTH) c.out_float = static_cast<float *>(image_out_override);
    else c.out_rgba = static_cast<uchar4 *>(image_out_override);
  }
  return DSLAM_OK;
}

static int fill_render_params(RenderParams &rp, const dslam_scene *s, dslam_render_state *r, const float *M,
                              const float *intr, int type, void *image_out_override = nullptr) {
  rp.vol.hash = s->hash; rp.vol.voxels = s->voxels; rp.vol.mask = (unsigned)(s->p.num_buckets - 1);
  rp.vol.num_buckets = s->p.num_buckets;
  DSLAM_TRY(fill_ray_camera(rp.cam, s, r, M, intr, type, image_out_override));
  rp.dbg_waves = nullptr; rp.split_len = 0.0f;
  rp.start_stamp = nullptr; rp.stamp = 0;
  return DSLAM_OK;
}

// grid of the single-wave march kernels; `split`: long tiles get two wavefronts (see k_render)
static dim3 march_grid(RenderParams &rp, const dslam_render_state *r, bool split) {
  rp.split_len = split ? kSplitLen : 0.0f;
  return dim3((r->w + 7) / 8, ((r->h + 7) / 8) * (split ? 2 : 1));
}

int launch_render(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M, const float *intr,
                  int type, bool reuse_raycast, void *image_out_override) {
  RenderParams rp;
  DSLAM_TRY(fill_render_params(rp, s, r, M, intr, type, image_out_override));
  static DiagDump dump("DSLAM_DBG_WAVETIME", 30);
  rp.dbg_waves = dump.arm((size_t)((r->w + 7) / 8) * ((r->h + 7) / 8) * 2, 48);   // (6 words per wavefront of the split grid)
  const dim3 grid1 = march_grid(rp, r, !reuse_raycast);
  if (e->stamp_due) {   // (set by the adoption of a complete record in this very GetImage: launch_find_visible_and_depths)
    e->stamp_due = false;
    if (e->overlap_mark && e->async_mode) {
      rp.start_stamp = e->start_stamp;
      if (++e->stamp_seq == 0) e->stamp_seq = 1;
      rp.stamp = e->stamp_seq;
      e->stamp_view_reads = e->view_reads;   // (as launch_fill_range: every call that read a view so far has its kernels in front)
    }
  }
  if (reuse_raycast) {
    if (type == DSLAM_IMAGE_DEPTH || type < 0) hipLaunchKernelGGL((k_render<false, false, true>), grid1, dim3(64), 0, e->stream, rp);
    else hipLaunchKernelGGL((k_render<true, false, true>), grid1, dim3(64), 0, e->stream, rp);
  } else if (rp.dbg_waves)
    hipLaunchKernelGGL((k_render<false, true>), grid1, dim3(64), 0, e->stream, rp);
  else if (type == DSLAM_IMAGE_DEPTH || type < 0)
    hipLaunchKernelGGL((k_render<false>), grid1, dim3(64), 0, e->stream, rp);
  else
    hipLaunchKernelGGL((k_render<true>), grid1, dim3(64), 0, e->stream, rp);
  DSLAM_HIP(hipGetLastError());
  return dump.write(e);
}

// ---------------------------------------------------------------------------------------------------------
// CreateICPMaps: processPixelICP<useSmoothing = true, flipNormals = false>
// ---------------------------------------------------------------------------------------------------------
// Also drawPixelGrey into renderState->raycastImage: the picture ITMMainEngine::GetImage(InfiniTAM_IMAGE_SCENERAYCAST)
// copies out (PreviewType::kRaycastImage, InfiniTamDriver.cpp:28-29) -- (0.8 angle + 0.2) 255 on all four channels, 0
// where the ray found nothing.
__global__ __launch_bounds__(256) void k_icp_maps(const float4 *__restrict__ pr, int W, int H, float vs, float lx,
                                                  float ly, float lz, float4 *points, float4 *normals,
                                                  uchar4 *grey) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const int loc = x + y * W;
  const float4 point = pr[loc];
  bool found = point.w > 0.0f;
  float nx = 0, ny = 0, nz = 0, angle = 0.0f;
  if (found && (y <= 2 || y >= H - 3 || x <= 2 || x >= W - 3)) found = false;
  if (found) {
    float4 xp = pr[(x + 2) + y * W], yp = pr[x + (y + 2) * W], xm = pr[(x - 2) + y * W], ym = pr[x + (y - 2) * W];
    float4 dx = make_float4(0, 0, 0, 0), dy = make_float4(0, 0, 0, 0);
    bool plus1 = false;
    if (xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0) plus1 = true;
    if (!plus1) {
      dx = make_float4(xp.x - xm.x, xp.y - xm.y, xp.z - xm.z, xp.w - xm.w);
      dy = make_float4(yp.x - ym.x, yp.y - ym.y, yp.z - ym.z, yp.w - ym.w);
      const float ld = fmaxf(dx.x * dx.x + dx.y * dx.y + dx.z * dx.z, dy.x * dy.x + dy.y * dy.y + dy.z * dy.z);
      if (ld * vs * vs > (0.15f * 0.15f)) plus1 = true;
    }
    if (plus1) {
      xp = pr[(x + 1) + y * W]; yp = pr[x + (y + 1) * W]; xm = pr[(x - 1) + y * W]; ym = pr[x + (y - 1) * W];
      dx = make_float4(xp.x - xm.x, xp.y - xm.y, xp.z - xm.z, xp.w - xm.w);
      dy = make_float4(yp.x - ym.x, yp.y - ym.y, yp.z - ym.z, yp.w - ym.w);
      if (xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0) found = false;
    }
    if (found) {
      nx = -(dx.y * dy.z - dx.z * dy.y);
      ny = -(dx.z * dy.x - dx.x * dy.z);
      nz = -(dx.x * dy.y - dx.y * dy.x);
      const float ns = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
      nx *= ns; ny *= ns; nz *= ns;
      angle = nx * lx + ny * ly + nz * lz;
      if (!(angle > 0.0f)) found = false;
    }
  }
  if (found) {
    const unsigned char g = (unsigned char)((0.8f * angle + 0.2f) * 255.0f);
    grey[loc] = make_uchar4(g, g, g, g);
    points[loc] = make_float4(point.x * vs, point.y * vs, point.z * vs, 1.0f);
    normals[loc] = make_float4(nx, ny, nz, 0.0f);
  } else {
    grey[loc] = make_uchar4(0, 0, 0, 0);
    points[loc] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    normals[loc] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  }
}

int launch_icp_maps(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M, const float *intr) {
  if (!r->icp_points) {
    RenderIcpMaps n;   // (the render state gets the three together or none)
    DSLAM_TRY(n.icp_points.alloc((size_t)r->w * r->h)); DSLAM_TRY(n.icp_normals.alloc((size_t)r->w * r->h));
    DSLAM_TRY(n.raycast_image.alloc((size_t)r->w * r->h));
    static_cast<RenderIcpMaps &>(*r) = std::move(n);
  }
  RenderParams rp;
  DSLAM_TRY(fill_render_params(rp, s, r, M, intr, -1));
  const dim3 grid((r->w + 15) / 16, (r->h + 15) / 16);
  hipLaunchKernelGGL((k_render<false>), march_grid(rp, r, true), dim3(64), 0, e->stream, rp);
  hipLaunchKernelGGL(k_icp_maps, grid, dim3(256), 0, e->stream, r->raycast, r->w, r->h, s->p.voxel_size, -rp.cam.invM.m[8],
                     -rp.cam.invM.m[9], -rp.cam.invM.m[10], r->icp_points, r->icp_normals, r->raycast_image);
  DSLAM_HIP(hipGetLastError());
  return DSLAM_OK;
}

}  // namespace dslam
