// frustum_device.h -- block frustum test and projection (FindVisibleBlocks / CreateExpectedDepths): the selection that
// GetImage runs (raycast.hip, multimap.hip) and that ProcessFrame runs for its own pose in the fusion launch (integrate.hip).
// Moved here unchanged from raycast_device.h.
#pragma once
#include <cstring>

#include "dslam_bits.h"

#pragma clang fp contract(off)

namespace dslam {
// ---------------------------------------------------------------------------------------------------------
// FindVisibleBlocks: ordered compaction of entries with ptr >= 0 that pass the 8-corner frustum test
// ---------------------------------------------------------------------------------------------------------
// An ordered selection over the scene's alloc_bits (dslam_bits.h): only entries that hold a block are read and tested
// (round 2: a frustum-flag sweep over all 1.18 M entries and a compaction sweep over 1.18 M byte flags).
struct FrustumParams {
  Mat4 M;
  float fx, fy, cx, cy, voxel_size;
  int W, H;
};

// ---------------------------------------------------------------------------------------------------------
// CreateExpectedDepths
// ---------------------------------------------------------------------------------------------------------
struct ProjParams {
  Mat4 M;
  float fx, fy, cx, cy, voxel_size;
  int W, H;
};

// ProjectSingleBlock: bbox (in 1/8-resolution cells) and z-range of one block; returns the number of 16x16 render
// tiles it needs (0 = nothing to render)
__device__ __forceinline__ int project_single_block(const HashEntry &e, const ProjParams &p, int4 &box, float2 &zr) {
  if (e.ptr < 0) return 0;
  int ulx = p.W / 8, uly = p.H / 8, lrx = -1, lry = -1;
  float zmin = kFarAway, zmax = kVeryClose;
#pragma unroll
  for (int corner = 0; corner < 8; corner++) {
    short tx = e.pos[0], ty = e.pos[1], tz = e.pos[2];
    tx += (corner & 1) ? 1 : 0; ty += (corner & 2) ? 1 : 0; tz += (corner & 4) ? 1 : 0;
    Vec4 q;
    q.x = (float)tx * (float)kBlock * p.voxel_size;
    q.y = (float)ty * (float)kBlock * p.voxel_size;
    q.z = (float)tz * (float)kBlock * p.voxel_size;
    q.w = 1.0f;
    q = mul(p.M, q);
    if (q.z < 1e-6f) continue;
    const float px = (p.fx * q.x / q.z + p.cx) / 8.0f;
    const float py = (p.fy * q.y / q.z + p.cy) / 8.0f;
    if ((float)ulx > floorf(px)) ulx = (int)floorf(px);
    if ((float)lrx < ceilf(px)) lrx = (int)ceilf(px);
    if ((float)uly > floorf(py)) uly = (int)floorf(py);
    if ((float)lry < ceilf(py)) lry = (int)ceilf(py);
    if (zmin > q.z) zmin = q.z;
    if (zmax < q.z) zmax = q.z;
  }
  if (ulx < 0) ulx = 0;
  if (uly < 0) uly = 0;
  if (lrx >= p.W) lrx = p.W - 1;
  if (lry >= p.H) lry = p.H - 1;
  bool valid = !(ulx > lrx) && !(uly > lry);
  if (zmin < kVeryClose) zmin = kVeryClose;
  if (zmax < kVeryClose) valid = false;
  if (!valid) return 0;
  const int rx = (int)ceilf((float)(lrx - ulx + 1) / 16.0f), ry = (int)ceilf((float)(lry - uly + 1) / 16.0f);
  box = make_int4(ulx, uly, lrx, lry);
  zr = make_float2(zmin, zmax);
  return rx * ry;
}

// PROJECT: the lane that lists visible entry number r also projects it (CreateExpectedDepths' ProjectSingleBlock; GetImage
// runs both with one pose), the compaction launch resets the range image, and every compaction tile leaves its
// render-tile total for k_fill_range_tiles.
// HIDDEN: the selection runs on the auxiliary stream behind a deferring allocation sweep whose table stores k_publish_entries
// has not scattered yet.  The sweep has set alloc_bits for the entries it created and left their positions in
// hidden_pos.  A selection only loads entries whose bit is set, and without swapping a set bit over a table entry that is
// still empty (ptr < 0) can only mean "created by this pass": every other path that sets the bit stores the entry in the same
// launch, and every path that empties an entry clears the bit.  Such an entry is taken as resident at its hidden position; the
// slot is not known yet and nothing here reads it (test and project_single_block look at the sign of ptr alone).  An entry
// the publish kernel has already stored carries the same position in the table.  Scenes with swapping never take this path.
template <bool PROJECT, bool HIDDEN = false>
struct SelFrustum {
  const HashEntry *hash;
  FrustumParams fp;
  int4 *boxes;
  float2 *zr_out;
  int *req_out;
  float2 *range;
  int npix;
  const short4 *hidden_pos = nullptr;   // (HIDDEN only)
  __device__ void prologue() const {
    if (PROJECT)   // (independent job) reset the range image to (FAR_AWAY, VERY_CLOSE)
      for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) range[i] = make_float2(kFarAway, kVeryClose);
  }
  typedef HashEntry Payload;
  __device__ HashEntry load(int t) const {
    HashEntry e = load_entry(hash, t);
    if constexpr (HIDDEN) {
      if (e.ptr < 0) {
        const short4 p = hidden_pos[t];
        e.pos[0] = p.x; e.pos[1] = p.y; e.pos[2] = p.z;
        e.ptr = 0;
      }
    }
    return e;
  }
  __device__ bool test(int, const HashEntry &e) const {
    if (e.ptr < 0) return false;
    bool vis, vis_enl;
    check_block_vis<false>(vis, vis_enl, e.pos[0], e.pos[1], e.pos[2], fp.M, fp.fx, fp.fy, fp.cx, fp.cy, fp.voxel_size, fp.W, fp.H);
    return vis;
  }
  struct Staged { int4 box; float2 zr; int req; };
  __device__ Staged stage(int, const HashEntry &e) const {
    Staged s;
    s.req = 0;
    if (!PROJECT) return s;
    ProjParams pp;
    pp.M = fp.M; pp.fx = fp.fx; pp.fy = fp.fy; pp.cx = fp.cx; pp.cy = fp.cy; pp.voxel_size = fp.voxel_size; pp.W = fp.W; pp.H = fp.H;
    s.req = project_single_block(e, pp, s.box, s.zr);
    return s;
  }
  __device__ int emit(int, int r, bool listed, const Staged &s) const {
    if (!PROJECT || !listed) return 0;
    if (s.req) { boxes[r] = s.box; zr_out[r] = s.zr; }
    req_out[r] = s.req;
    return s.req;
  }
  __device__ void finish(int) const {}
};

static FrustumParams make_frustum_params(const dslam_scene *s, const dslam_render_state *r, const float *M, const float *intr) {
  FrustumParams fp;
  memcpy(fp.M.m, M, 64);
  fp.fx = intr[0]; fp.fy = intr[1]; fp.cx = intr[2]; fp.cy = intr[3]; fp.voxel_size = s->p.voxel_size;
  fp.W = r->w; fp.H = r->h;
  return fp;
}

static ProjParams make_proj_params(const dslam_scene *s, const dslam_render_state *r, const float *M, const float *intr) {
  ProjParams pp;
  memcpy(pp.M.m, M, 64);
  pp.fx = intr[0]; pp.fy = intr[1]; pp.cx = intr[2]; pp.cy = intr[3]; pp.voxel_size = s->p.voxel_size;
  pp.W = r->w; pp.H = r->h;
  return pp;
}

}  // namespace dslam
