// multimap.hip -- one raycast over several local maps, each read through its own world -> map transform
// (dslam_get_image_multi; ITMMainEngine::GetImageAllLocalMaps in the mirror).
//
// Reference: the static map is split into local maps (DenseSlam.cpp:133-141, 260-261, 554-565), each a voxel-hash scene
// with an estimatedGlobalPose (DenseSlam.cpp:190, 577-579); every preview draws currentLocalMap only
// (InfiniTamDriver.cpp:229-277).  The combination law below is this project's own definition.
//
// Front end, 2N + 1 launches for N maps: per map a frustum selection + projection over its alloc_bits (the compaction of
// FindVisibleBlocks with no list output: the render state's visible list is never written) and a splat of its boxes into
// the shared range image (per-cell min / max) and the per-cell map mask (bit i: a block of map i projects into the cell);
// the first selection also resets the range image and the mask.  Then one march launch.
//
// March: one wavefront = one 8x8 tile = one range cell, as k_render, so the cell's map mask is wave-uniform.  Every read
// of the march (nearest voxel, trilinear, 6-tap normal, trilinear colour) is a combined read over the maps of the mask,
// in ascending map order: a map reports (value v_i, found, confidence w_i); none found -> not found; exactly one ->
// its value unchanged; more -> sum(w_i v_i) / sum(w_i), accumulated in float32 in map order as
// num = ((w_0 v_0 + w_1 v_1) + w_2 v_2) + ..., den = ((w_0 + w_1) + w_2) + ..., value = num / den (den == 0: 1.0 for
// sdf, the first contributor's value for normal / colour).  A map whose transform is exactly the identity reads at
// the march position itself, so a tile that sees one such map marches and shades bit for bit like k_render.
#include <cmath>
#include <cstdio>

#include "dslam_bits.h"
#include "multimap_device.h"
#include "raycast_device.h"

#pragma clang fp contract(off)

namespace dslam {

// FindVisibleBlocks + ProjectSingleBlock of one map; the first map's launch also resets the range image and the mask
struct SelMulti : SelFrustum<true> {
  unsigned long long *cell_mask;
  int ncell;
  __device__ void prologue() const {
    SelFrustum<true>::prologue();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ncell; i += gridDim.x * blockDim.x) cell_mask[i] = 0ull;
  }
};

// every projected box of one map into the range image (min / max, as k_fill_range_tiles) and the map mask; cells outside
// the ceil(W/8) x ceil(H/8) corner the march reads are not touched.  A wavefront takes its 64 boxes one after the other,
// each with all 64 lanes over its cells: a block next to the camera covers thousands of cells, which one lane alone
// would walk through serially.
__global__ __launch_bounds__(256) void k_multi_splat(const int *__restrict__ count, const int4 *__restrict__ boxes,
                                                     const float2 *__restrict__ zr, const int *__restrict__ req,
                                                     float2 *range, unsigned long long *cell_mask, int W, int cw, int ch,
                                                     int bit) {
  const int n = *count;
  const int lane = threadIdx.x & 63;
  const unsigned long long b = 1ull << bit;
  for (int base = blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n; base += gridDim.x * blockDim.x) {   // (uniform)
    const int i = base + lane;
    int x0 = 0, y0 = 0, x1 = -1, y1 = -1, zmin_i = 0, zmax_i = 0;
    if (i < n && req[i] != 0) {
      const int4 box = boxes[i];
      const float2 z = zr[i];
      x0 = box.x; y0 = box.y;
      x1 = box.z < cw - 1 ? box.z : cw - 1;
      y1 = box.w < ch - 1 ? box.w : ch - 1;
      zmin_i = __float_as_int(z.x); zmax_i = __float_as_int(z.y);
    }
    for (int j = 0; j < 64; j++) {
      const int bx0 = __shfl(x0, j, 64), by0 = __shfl(y0, j, 64), bx1 = __shfl(x1, j, 64), by1 = __shfl(y1, j, 64);
      const int zmin = __shfl(zmin_i, j, 64), zmax = __shfl(zmax_i, j, 64);
      if (bx0 > bx1 || by0 > by1) continue;
      const int w = bx1 - bx0 + 1, cells = w * (by1 - by0 + 1);
      for (int c = lane; c < cells; c += 64) {
        const int x = bx0 + c % w, y = by0 + c / w;
        int *px = reinterpret_cast<int *>(&range[x + (size_t)y * W]);
        atomicMin(&px[0], zmin);
        atomicMax(&px[1], zmax);
        atomicOr(&cell_mask[x + y * cw], b);
      }
    }
  }
}

struct MultiRenderParams {
  const MultiMap *maps;
  const unsigned long long *cell_mask;
  int cw;
  RayCamera cam;
};

// a gradient of the map frame back into the world frame: R^T g
__device__ __forceinline__ Vec3 to_world_dir(const MultiMap &m, const Vec3 &g) {
  if (m.identity) return g;
  Vec3 r;
  r.x = (m.T[0] * g.x + m.T[4] * g.y) + m.T[8] * g.z;
  r.y = (m.T[1] * g.x + m.T[5] * g.y) + m.T[9] * g.z;
  r.z = (m.T[2] * g.x + m.T[6] * g.y) + m.T[10] * g.z;
  return r;
}

// combined trilinear sdf read at world position p; `first_any`: the first candidate's read (all of its taps empty when
// no map reports found -- what a single-map read returns there)
__device__ float multi_trilinear(const MultiRenderParams &p, unsigned long long mk, const Vec3 &pt) {
  Blend b = {0, 0.0f, 0.0f, 0.0f};
  float first_any = 1.0f;
  bool have_any = false;
  while (mk) {
    const int i = first_map(mk);
    mk &= mk - 1;
    const MultiMap &m = p.maps[i];
    const Vec3 q = to_map(m, pt);
    const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
    uint2 t[8];
    const bool found = gather_cell(volume_of(m), (int)fx, (int)fy, (int)fz, t);
    unsigned raw[8];
    float wt[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { raw[k] = t[k].x; wt[k] = (float)((t[k].x >> 16) & 0xffu); }
    const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
    const float v = trilinear_raw(raw, cx, cy, cz);
    if (!have_any) { first_any = v; have_any = true; }
    if (found) b.add(v, lerp8(wt, cx, cy, cz));
  }
  return b.n == 0 ? first_any : b.value(1.0f);
}

// castRay (cast_ray<false> in raycast.hip) with every read combined over the maps of the cell's mask
__device__ __forceinline__ bool cast_ray_multi(Vec4 &out, int x, int y, const MultiRenderParams &p, const float2 minmax,
                                               const unsigned long long cell_mk) {
  const RayCamera &c = p.cam;
  float sdf = 1.0f;
  const float step_scale = c.mu * c.one_over_vs;
  const RaySegment seg = ray_segment(c, x, y, minmax);
  const Vec3 dir = seg.dir;
  Vec3 res = seg.start;
  float total = seg.total, step;
  const float total_max = seg.total_max;
  // per-lane block cache: one entry, tagged with its map
  IndexCache cache = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
  int cache_map = -1;
  while (total < total_max) {
    // nearest-voxel read of every map of the cell
    Blend b = {0, 0.0f, 0.0f, 0.0f};
    unsigned long long mk = cell_mk;
    while (mk) {
      const int i = first_map(mk);
      mk &= mk - 1;
      const MultiMap &m = p.maps[i];
      const Vec3 qm = to_map(m, res);
      const int vx = iround(qm.x), vy = iround(qm.y), vz = iround(qm.z);
      if (cache_map != i) { cache.bx = 0x7fffffff; cache_map = i; }
      const int base = lookup_block(volume_of(m), vx >> 3, vy >> 3, vz >> 3, cache);
      if (base >= 0) {
        const unsigned raw = m.voxels[(size_t)base + (unsigned)((vx & 7) | ((vy & 7) << 3) | ((vz & 7) << 6))].x;
        b.add(div_exact((float)(short)(raw & 0xffffu), 32767.0f, c.inv_32767), (float)((raw >> 16) & 0xffu));
      }
    }
    if (b.n == 0) {
      sdf = 1.0f;  // empty voxel: 32767 / 32767
      step = (float)kBlock;
    } else {
      sdf = b.value(1.0f);
      if ((sdf <= 0.1f) && (sdf >= -0.5f)) sdf = multi_trilinear(p, cell_mk, res);
      if (sdf <= 0.0f) break;
      step = fmaxf(sdf * step_scale, 1.0f);
    }
    res.x += step * dir.x; res.y += step * dir.y; res.z += step * dir.z;
    total += step;
  }
  return refine_hit(out, res, dir, sdf, step_scale, [&](const Vec3 &pt) { return multi_trilinear(p, cell_mk, pt); });
}

// k_render<SHADE> over several maps: march, depth, and the three shaded types
template <bool SHADE>
__global__ __launch_bounds__(64) void k_render_multi(MultiRenderParams mp) {
  const RayCamera &p = mp.cam;
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 8 + (lane & 7), y = blockIdx.y * 8 + (lane >> 3);
  const unsigned long long m0 = mp.cell_mask[blockIdx.x + blockIdx.y * mp.cw];
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m0), hi = __builtin_amdgcn_readfirstlane((unsigned)(m0 >> 32));
  const unsigned long long cell_mk = ((unsigned long long)hi << 32) | lo;
  if (x >= p.W || y >= p.H) return;
  const int loc = x + y * p.W;
  const int loc2 = (int)floorf((float)x / 8.0f) + (int)floorf((float)y / 8.0f) * p.W;
  Vec4 pr;
  cast_ray_multi(pr, x, y, mp, p.range[loc2], cell_mk);
  p.raycast[loc] = make_float4(pr.x, pr.y, pr.z, pr.w);
  if (p.type < 0) return;

  // combined 6-tap normal: each map's gradient in the world frame, confidence = trilinear w_depth at the point
  auto normal = [&](const Vec3 &pt) {
    Blend3 b = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    Vec3 first_any = {0.0f, 0.0f, 0.0f};
    bool have_any = false;
    unsigned long long mk = cell_mk;
    while (mk) {
      const int i = first_map(mk);
      mk &= mk - 1;
      const MultiMap &m = mp.maps[i];
      const VolumeRef vol = volume_of(m);
      const Vec3 q = to_map(m, pt);
      IndexCache c = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
      const Vec3 g = to_world_dir(m, normal_from_sdf(vol, q, c));
      if (!have_any) { first_any = g; have_any = true; }
      const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
      uint2 t[8];
      if (gather_cell(vol, (int)fx, (int)fy, (int)fz, t)) {
        float wt[8];
#pragma unroll
        for (int k = 0; k < 8; k++) wt[k] = (float)((t[k].x >> 16) & 0xffu);
        b.add(g, lerp8(wt, q.x - fx, q.y - fy, q.z - fz));
      }
    }
    return b.n == 0 ? first_any : b.value();
  };
  // combined colour: confidence = trilinear w_color
  auto colour = [&](const Vec3 &pt) {
    Blend3 b = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    Vec3 first_any = {0.0f, 0.0f, 0.0f};
    bool have_any = false;
    unsigned long long mk = cell_mk;
    while (mk) {
      const int i = first_map(mk);
      mk &= mk - 1;
      const MultiMap &m = mp.maps[i];
      const Vec3 q = to_map(m, pt);
      const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
      uint2 t[8];
      const bool hit = gather_cell(volume_of(m), (int)fx, (int)fy, (int)fz, t);
      const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
      const Vec4 c4 = colour_from_taps(t, cx, cy, cz);
      const Vec3 c3 = {c4.x, c4.y, c4.z};
      if (!have_any) { first_any = c3; have_any = true; }
      if (hit) {
        float wt[8];
#pragma unroll
        for (int k = 0; k < 8; k++) wt[k] = (float)((t[k].y >> 16) & 0xffu);
        b.add(c3, lerp8(wt, cx, cy, cz));
      }
    }
    return b.n == 0 ? first_any : b.value();
  };
  store_pixel<SHADE>(p, loc, pr, normal, colour);
}

static int ensure_multi_buffers(dslam_render_state *r) {
  if (r->multi_mask) return DSLAM_OK;
  const size_t ncell = (size_t)((r->w + 7) / 8) * ((r->h + 7) / 8);
  RenderMulti n;   // (the render state gets the two together or none)
  DSLAM_TRY(n.multi_mask.alloc(ncell));
  DSLAM_TRY(n.multi_counts.alloc(DSLAM_MAX_RENDER_MAPS));
  static_cast<RenderMulti &>(*r) = std::move(n);
  return DSLAM_OK;
}

// scenes / T_map_from_world (column-major, metres) are checked by the caller (dslam_get_image_multi)
int launch_render_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T, int n, dslam_render_state *r,
                        const float *M, const float *intr, int type, void *image_out_override) {
  int rc = ensure_multi_buffers(r);
  if (rc) return rc;
  const int cw = (r->w + 7) / 8, ch = (r->h + 7) / 8;
  // (posed_map divides the translation in double and rounds; the float32 division this call used to do gives the same bits)
  DSLAM_TRY(upload_posed_maps(e, scenes, T, n, (double)scenes[0]->p.voxel_size));
  // front end: map i seen from M is a camera at M T_i^-1 (the identity keeps M bit for bit)
  for (int i = 0; i < n; i++) {
    const dslam_scene *s = scenes[i];
    const float *Ti = T + 16 * i;
    float Mi[16];
    if (is_identity16(Ti)) {
      memcpy(Mi, M, sizeof(Mi));
    } else {
      float Tinv[16];
      if (!invert_matrix(Ti, Tinv)) { set_last_error("map transform is singular"); return DSLAM_ERR_INVALID; }
      for (int col = 0; col < 4; col++)
        for (int row = 0; row < 4; row++) {
          double acc = 0.0;
          for (int k = 0; k < 4; k++) acc += (double)M[k * 4 + row] * (double)Tinv[col * 4 + k];
          Mi[col * 4 + row] = (float)acc;
        }
    }
    if ((rc = ensure_scratch(e, s->n_entries, s->p.num_local_blocks))) return rc;
    SelMulti sel;
    sel.hash = s->hash;
    sel.fp = make_frustum_params(s, r, Mi, intr);
    sel.boxes = r->proj_boxes; sel.zr_out = r->proj_z; sel.req_out = r->proj_req; sel.range = r->range;
    sel.npix = i == 0 ? r->w * r->h : 0;
    sel.cell_mask = r->multi_mask;
    sel.ncell = i == 0 ? cw * ch : 0;
    launch_bits_select(e, s->alloc_bits, s->n_entries, sel, nullptr, r->n_local, r->multi_counts + i, s->counters);
    hipLaunchKernelGGL(k_multi_splat, dim3(256), dim3(256), 0, e->stream, r->multi_counts + i, r->proj_boxes, r->proj_z,
                       r->proj_req, r->range, r->multi_mask, r->w, cw, ch, i);
    DSLAM_HIP(hipGetLastError());
  }
  MultiRenderParams rp;
  rp.maps = static_cast<const MultiMap *>(e->map_table.get());
  rp.cell_mask = r->multi_mask;
  rp.cw = cw;
  DSLAM_TRY(fill_ray_camera(rp.cam, scenes[0], r, M, intr, type, image_out_override));
  if (type == DSLAM_IMAGE_DEPTH || type < 0)
    hipLaunchKernelGGL(k_render_multi<false>, dim3(cw, ch), dim3(64), 0, e->stream, rp);
  else
    hipLaunchKernelGGL(k_render_multi<true>, dim3(cw, ch), dim3(64), 0, e->stream, rp);
  DSLAM_HIP(hipGetLastError());
  return DSLAM_OK;
}

}  // namespace dslam
