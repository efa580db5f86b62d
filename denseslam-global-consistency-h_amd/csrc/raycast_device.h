// raycast_device.h -- the device side of the ray march shared by raycast.hip (one map) and multimap.hip (several
// maps): the camera of a render launch, the ray segment of a pixel, the voxel reads of castRay, the refinement behind the
// march and the pixel epilogue (the frustum test and projection are in frustum_device.h).  The march loops themselves are
// the renderers' own.
#pragma once
#include <cstring>

#include "dslam_bits.h"
#include "frustum_device.h"

#pragma clang fp contract(off)

namespace dslam {

// ---------------------------------------------------------------------------------------------------------
// voxel access
// ---------------------------------------------------------------------------------------------------------
struct VolumeRef {
  const HashEntry *hash;
  const uint2 *voxels;
  unsigned mask;
  int num_buckets;
};

struct IndexCache {
  int bx, by, bz, block_ptr;
};

__device__ __forceinline__ uint2 read_voxel(const VolumeRef &vol, int px, int py, int pz, bool &found, IndexCache &c) {
  const int bx = ((px < 0) ? px - kBlock + 1 : px) / kBlock;
  const int by = ((py < 0) ? py - kBlock + 1 : py) / kBlock;
  const int bz = ((pz < 0) ? pz - kBlock + 1 : pz) / kBlock;
  const int lin = (px - bx * kBlock) + (py - by * kBlock) * kBlock + (pz - bz * kBlock) * kBlock * kBlock;
  if (bx == c.bx && by == c.by && bz == c.bz) {
    found = true;
    return vol.voxels[(size_t)c.block_ptr + lin];
  }
  int h = hash_index(bx, by, bz, vol.mask);
  while (true) {
    const HashEntry e = load_entry(vol.hash, h);
    if (e.pos[0] == bx && e.pos[1] == by && e.pos[2] == bz && e.ptr >= 0) {
      found = true;
      c.bx = bx; c.by = by; c.bz = bz;
      c.block_ptr = e.ptr * kBlock3;
      return vol.voxels[(size_t)c.block_ptr + lin];
    }
    if (e.offset < 1) break;
    h = vol.num_buckets + e.offset - 1;
  }
  found = false;
  return make_uint2(kEmptyVoxelLo, kEmptyVoxelHi);
}

__device__ __forceinline__ float rd_sdf(const VolumeRef &vol, int x, int y, int z, bool &found, IndexCache &c) {
  return (float)(short)(read_voxel(vol, x, y, z, found, c).x & 0xffffu);
}

// (int)(x < 0 ? x - 0.5f : x + 0.5f); copysign folds the compare + select into one bit-field insert (-0.0 gives 0
// either way)
__device__ __forceinline__ int iround(float x) { return (int)(x + __builtin_copysignf(0.5f, x)); }

// block base pointer (voxel index of the block's first voxel) or -1; refreshes the per-lane cache on a hit
__device__ __forceinline__ int lookup_block(const VolumeRef &vol, int bx, int by, int bz, IndexCache &c) {
  if (bx == c.bx && by == c.by && bz == c.bz) return c.block_ptr;
  int h = hash_index(bx, by, bz, vol.mask);
  while (true) {
    const HashEntry e = load_entry(vol.hash, h);
    if (e.pos[0] == bx && e.pos[1] == by && e.pos[2] == bz && e.ptr >= 0) {
      c.bx = bx; c.by = by; c.bz = bz;
      c.block_ptr = e.ptr * kBlock3;
      return c.block_ptr;
    }
    if (e.offset < 1) return -1;
    h = vol.num_buckets + e.offset - 1;
  }
}

// Block base pointers (voxel index of the block's first voxel, or -1) of the 8 corners of a trilinear cell whose
// per-axis block coordinates are bxa/bya/bza[0..1]; corner k = (k & 1, (k >> 1) & 1, k >> 2).  All eight bucket heads
// are loaded in ONE round trip (equal blocks hit the same address); corners whose head holds another block follow
// their excess chains together, one round trip per link.
__device__ __forceinline__ void resolve_cell_blocks(const VolumeRef &vol, const int bxa[2], const int bya[2],
                                                    const int bza[2], int base[8]) {
  const unsigned hx[2] = {(unsigned)bxa[0] * 73856093u, (unsigned)bxa[1] * 73856093u};
  const unsigned hy[2] = {(unsigned)bya[0] * 19349669u, (unsigned)bya[1] * 19349669u};
  const unsigned hz[2] = {(unsigned)bza[0] * 83492791u, (unsigned)bza[1] * 83492791u};
  // packed position words of an entry: x = pos0 | pos1 << 16, y = pos2 (| pad); a block coordinate outside the
  // short range can never be stored, so it never matches
  const unsigned tx[2] = {(unsigned)bxa[0] & 0xffffu, (unsigned)bxa[1] & 0xffffu};
  const unsigned ty[2] = {(unsigned)bya[0] << 16, (unsigned)bya[1] << 16};
  const unsigned tz[2] = {(unsigned)bza[0] & 0xffffu, (unsigned)bza[1] & 0xffffu};
  const bool okx[2] = {bxa[0] == (short)bxa[0], bxa[1] == (short)bxa[1]};
  const bool oky[2] = {bya[0] == (short)bya[0], bya[1] == (short)bya[1]};
  const bool okz[2] = {bza[0] == (short)bza[0], bza[1] == (short)bza[1]};
  int h[8];
  u32x4 e[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    h[k] = (int)((hx[k & 1] ^ hy[(k >> 1) & 1] ^ hz[k >> 2]) & vol.mask);
    e[k] = *reinterpret_cast<const u32x4 *>(vol.hash + h[k]);
  }
  unsigned pending = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const bool ok = okx[k & 1] && oky[(k >> 1) & 1] && okz[k >> 2];
    const bool match = ok && e[k].x == (tx[k & 1] | ty[(k >> 1) & 1]) && (e[k].y & 0xffffu) == tz[k >> 2] && (int)e[k].w >= 0;
    base[k] = match ? (int)e[k].w * kBlock3 : -1;
    if (!match && (int)e[k].z >= 1) { pending |= 1u << k; h[k] = vol.num_buckets + (int)e[k].z - 1; }
  }
  // excess chains: all unresolved corners advance one link per round trip.  Branch-free on purpose -- a wave64
  // executes every instruction any of its lanes needs, and eight predicated blocks with a branch each cost five
  // times the instructions of selects (resolved corners just re-read their last entry and ignore it).
  while (pending) {
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = *reinterpret_cast<const u32x4 *>(vol.hash + h[k]);
    unsigned still = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const bool pk = (pending & (1u << k)) != 0;
      const bool ok = okx[k & 1] && oky[(k >> 1) & 1] && okz[k >> 2];
      const bool match = ok && e[k].x == (tx[k & 1] | ty[(k >> 1) & 1]) && (e[k].y & 0xffffu) == tz[k >> 2] && (int)e[k].w >= 0;
      const bool cont = pk && !match && (int)e[k].z >= 1;
      base[k] = (pk && match) ? (int)e[k].w * kBlock3 : base[k];
      h[k] = cont ? vol.num_buckets + (int)e[k].z - 1 : h[k];
      still |= cont ? (1u << k) : 0u;
    }
    pending = still;
  }
}

// The 8 taps of a trilinear read.  Tap k = (dx, dy, dz) = (k & 1, (k >> 1) & 1, k >> 2) relative to (x, y, z).  The
// kernel is bound by the NUMBER of scattered load instructions (measured: prefetching or speculative variants that
// add loads are slower), so the <= 8 (usually 1 or 2) distinct voxel blocks are resolved with as few probes as
// possible -- de-duplicated per axis, per-lane block cache first -- and then the 8 voxel loads are issued together.
// A tap whose block is not allocated reads the empty voxel, exactly like readVoxel.
__device__ __forceinline__ void gather_taps(const VolumeRef &vol, int x, int y, int z, IndexCache &c, uint2 t[8]) {
  const int bx0 = x >> 3, by0 = y >> 3, bz0 = z >> 3;  // arithmetic shift = floor division, as pointToVoxelBlockPos
  const int bx1 = (x + 1) >> 3, by1 = (y + 1) >> 3, bz1 = (z + 1) >> 3;
  const bool sx = bx1 == bx0, sy = by1 == by0, sz = bz1 == bz0;
  int p[8];
  p[0] = lookup_block(vol, bx0, by0, bz0, c);
  p[1] = sx ? p[0] : lookup_block(vol, bx1, by0, bz0, c);
  p[2] = sy ? p[0] : lookup_block(vol, bx0, by1, bz0, c);
  p[3] = sx ? p[2] : (sy ? p[1] : lookup_block(vol, bx1, by1, bz0, c));
  p[4] = sz ? p[0] : lookup_block(vol, bx0, by0, bz1, c);
  p[5] = sz ? p[1] : (sx ? p[4] : lookup_block(vol, bx1, by0, bz1, c));
  p[6] = sz ? p[2] : (sy ? p[4] : lookup_block(vol, bx0, by1, bz1, c));
  p[7] = sz ? p[3] : (sx ? p[6] : (sy ? p[5] : lookup_block(vol, bx1, by1, bz1, c)));
  const int lx0 = x & 7, lx1 = (x + 1) & 7, ly0 = (y & 7) * kBlock, ly1 = ((y + 1) & 7) * kBlock;
  const int lz0 = (z & 7) * kBlock * kBlock, lz1 = ((z + 1) & 7) * kBlock * kBlock;
  const int lin[8] = {lx0 + ly0 + lz0, lx1 + ly0 + lz0, lx0 + ly1 + lz0, lx1 + ly1 + lz0,
                      lx0 + ly0 + lz1, lx1 + ly0 + lz1, lx0 + ly1 + lz1, lx1 + ly1 + lz1};
#pragma unroll
  for (int k = 0; k < 8; k++) {
    // clamp the address so the load is unconditional (and therefore batched); select afterwards
    const uint2 v = vol.voxels[(size_t)(p[k] >= 0 ? p[k] : 0) + lin[k]];
    t[k] = (p[k] >= 0) ? v : make_uint2(kEmptyVoxelLo, kEmptyVoxelHi);
  }
}

// a / b via the correctly rounded reciprocal y = RN(1/b): exactly RN(a/b) for b = 32767 (0 mismatches over every
// finite float a, tests/tools/verify_exact_div.cpp); 3 instructions instead of the ~10 of an IEEE division
__device__ __forceinline__ float div_exact(float a, float b, float y) {
  const float q = a * y;
  const float r = __fmaf_rn(-b, q, a);
  return __fmaf_rn(r, y, q);
}

// trilinear blend of 8 tap values: x, then y, then z
__device__ __forceinline__ float lerp8(const float s[8], float cx, float cy, float cz) {
  float res1 = (1.0f - cx) * s[0] + cx * s[1];
  res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * s[2] + cx * s[3]);
  float res2 = (1.0f - cx) * s[4] + cx * s[5];
  res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * s[6] + cx * s[7]);
  return (1.0f - cz) * res1 + cz * res2;
}

__device__ __forceinline__ float trilinear_sdf(const uint2 t[8], float cx, float cy, float cz) {
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = (float)(short)(t[k].x & 0xffffu);
  return div_exact(lerp8(s, cx, cy, cz), 32767.0f, 1.0f / 32767.0f);
}

// The 8 taps (low voxel words) of the trilinear cell at (x0, y0, z0) in two load round trips: every block of the
// cell resolved together, then the 8 taps together; a tap whose block is not allocated reads the empty voxel.
// (multimap.hip's gather_cell is the same with 8-byte tap loads: merged, k_render's march would load both words too.)
__device__ __forceinline__ void gather_taps_batched(const VolumeRef &vol, int x0, int y0, int z0, unsigned raw[8]) {
  const int bxa[2] = {x0 >> 3, (x0 + 1) >> 3}, bya[2] = {y0 >> 3, (y0 + 1) >> 3}, bza[2] = {z0 >> 3, (z0 + 1) >> 3};
  int base[8];
  resolve_cell_blocks(vol, bxa, bya, bza, base);
  const unsigned lx[2] = {(unsigned)x0 & 7u, (unsigned)(x0 + 1) & 7u};
  const unsigned ly[2] = {((unsigned)y0 & 7u) << 3, ((unsigned)(y0 + 1) & 7u) << 3};
  const unsigned lz[2] = {((unsigned)z0 & 7u) << 6, ((unsigned)(z0 + 1) & 7u) << 6};
  const char *vbytes = reinterpret_cast<const char *>(vol.voxels);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const unsigned lin = lx[k & 1] | ly[(k >> 1) & 1] | lz[k >> 2];
    const unsigned off = (base[k] < 0) ? 0u : ((unsigned)base[k] + lin) * 8u;
    raw[k] = *reinterpret_cast<const unsigned *>(vbytes + off);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) raw[k] = (base[k] < 0) ? kEmptyVoxelLo : raw[k];
}

__device__ __forceinline__ float trilinear_raw(const unsigned raw[8], float cx, float cy, float cz) {
  uint2 t[8];
#pragma unroll
  for (int k = 0; k < 8; k++) t[k] = make_uint2(raw[k], 0u);
  return trilinear_sdf(t, cx, cy, cz);
}

// readFromSDF_float_interpolated in two round trips instead of up to nine
__device__ __forceinline__ float read_sdf_interp_batched(const VolumeRef &vol, const Vec3 &pt) {
  const float fx = floorf(pt.x), fy = floorf(pt.y), fz = floorf(pt.z);
  unsigned raw[8];
  gather_taps_batched(vol, (int)fx, (int)fy, (int)fz, raw);
  return trilinear_raw(raw, pt.x - fx, pt.y - fy, pt.z - fz);
}

// trilinear colour of 8 gathered taps (readFromSDF_color4u_interpolated's arithmetic)
__device__ __forceinline__ Vec4 colour_from_taps(const uint2 t[8], float cx, float cy, float cz) {
  float rx = 0.0f, ry = 0.0f, rz = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int ox = k & 1, oy = (k >> 1) & 1, oz = (k >> 2) & 1;
    const uint2 v = t[k];
    const float wx = ox ? cx : (1.0f - cx), wy = oy ? cy : (1.0f - cy), wz = oz ? cz : (1.0f - cz);
    const float w = wx * wy * wz;
    rx += w * (float)(v.x >> 24);
    ry += w * (float)(v.y & 0xffu);
    rz += w * (float)((v.y >> 8) & 0xffu);
  }
  Vec4 r = {rx / 255.0f, ry / 255.0f, rz / 255.0f, 255.0f / 255.0f};
  return r;
}

__device__ __forceinline__ Vec4 read_colour_interp(const VolumeRef &vol, const Vec3 &pt, IndexCache &c) {
  const float fx = floorf(pt.x), fy = floorf(pt.y), fz = floorf(pt.z);
  uint2 t[8];
  gather_taps(vol, (int)fx, (int)fy, (int)fz, c, t);
  return colour_from_taps(t, pt.x - fx, pt.y - fy, pt.z - fz);
}

// computeSingleNormalFromSDF (un-normalised gradient)
__device__ __forceinline__ Vec3 normal_from_sdf(const VolumeRef &vol, const Vec3 &pt, IndexCache &c) {
  bool f;
  Vec3 ret;
  const float flx = floorf(pt.x), fly = floorf(pt.y), flz = floorf(pt.z);
  const int x = (int)flx, y = (int)fly, z = (int)flz;
  const float cx = pt.x - flx, cy = pt.y - fly, cz = pt.z - flz;
  const float nx = 1.0f - cx, ny = 1.0f - cy, nz = 1.0f - cz;
  Vec4 front, back, tmp;
  front.x = rd_sdf(vol, x, y, z, f, c); front.y = rd_sdf(vol, x + 1, y, z, f, c);
  front.z = rd_sdf(vol, x, y + 1, z, f, c); front.w = rd_sdf(vol, x + 1, y + 1, z, f, c);
  back.x = rd_sdf(vol, x, y, z + 1, f, c); back.y = rd_sdf(vol, x + 1, y, z + 1, f, c);
  back.z = rd_sdf(vol, x, y + 1, z + 1, f, c); back.w = rd_sdf(vol, x + 1, y + 1, z + 1, f, c);
  float p1, p2, v1;
  // gradient x
  p1 = front.x * ny * nz + front.z * cy * nz + back.x * ny * cz + back.z * cy * cz;
  tmp.x = rd_sdf(vol, x - 1, y, z, f, c); tmp.y = rd_sdf(vol, x - 1, y + 1, z, f, c);
  tmp.z = rd_sdf(vol, x - 1, y, z + 1, f, c); tmp.w = rd_sdf(vol, x - 1, y + 1, z + 1, f, c);
  p2 = tmp.x * ny * nz + tmp.y * cy * nz + tmp.z * ny * cz + tmp.w * cy * cz;
  v1 = p1 * cx + p2 * nx;
  p1 = front.y * ny * nz + front.w * cy * nz + back.y * ny * cz + back.w * cy * cz;
  tmp.x = rd_sdf(vol, x + 2, y, z, f, c); tmp.y = rd_sdf(vol, x + 2, y + 1, z, f, c);
  tmp.z = rd_sdf(vol, x + 2, y, z + 1, f, c); tmp.w = rd_sdf(vol, x + 2, y + 1, z + 1, f, c);
  p2 = tmp.x * ny * nz + tmp.y * cy * nz + tmp.z * ny * cz + tmp.w * cy * cz;
  ret.x = (p1 * nx + p2 * cx - v1) / 32767.0f;
  // gradient y
  p1 = front.x * nx * nz + front.y * cx * nz + back.x * nx * cz + back.y * cx * cz;
  tmp.x = rd_sdf(vol, x, y - 1, z, f, c); tmp.y = rd_sdf(vol, x + 1, y - 1, z, f, c);
  tmp.z = rd_sdf(vol, x, y - 1, z + 1, f, c); tmp.w = rd_sdf(vol, x + 1, y - 1, z + 1, f, c);
  p2 = tmp.x * nx * nz + tmp.y * cx * nz + tmp.z * nx * cz + tmp.w * cx * cz;
  v1 = p1 * cy + p2 * ny;
  p1 = front.z * nx * nz + front.w * cx * nz + back.z * nx * cz + back.w * cx * cz;
  tmp.x = rd_sdf(vol, x, y + 2, z, f, c); tmp.y = rd_sdf(vol, x + 1, y + 2, z, f, c);
  tmp.z = rd_sdf(vol, x, y + 2, z + 1, f, c); tmp.w = rd_sdf(vol, x + 1, y + 2, z + 1, f, c);
  p2 = tmp.x * nx * nz + tmp.y * cx * nz + tmp.z * nx * cz + tmp.w * cx * cz;
  ret.y = (p1 * ny + p2 * cy - v1) / 32767.0f;
  // gradient z
  p1 = front.x * nx * ny + front.y * cx * ny + front.z * nx * cy + front.w * cx * cy;
  tmp.x = rd_sdf(vol, x, y, z - 1, f, c); tmp.y = rd_sdf(vol, x + 1, y, z - 1, f, c);
  tmp.z = rd_sdf(vol, x, y + 1, z - 1, f, c); tmp.w = rd_sdf(vol, x + 1, y + 1, z - 1, f, c);
  p2 = tmp.x * nx * ny + tmp.y * cx * ny + tmp.z * nx * cy + tmp.w * cx * cy;
  v1 = p1 * cz + p2 * nz;
  p1 = back.x * nx * ny + back.y * cx * ny + back.z * nx * cy + back.w * cx * cy;
  tmp.x = rd_sdf(vol, x, y, z + 2, f, c); tmp.y = rd_sdf(vol, x + 1, y, z + 2, f, c);
  tmp.z = rd_sdf(vol, x, y + 1, z + 2, f, c); tmp.w = rd_sdf(vol, x + 1, y + 1, z + 2, f, c);
  p2 = tmp.x * nx * ny + tmp.y * cx * ny + tmp.z * nx * cy + tmp.w * cx * cy;
  ret.z = (p1 * nz + p2 * cz - v1) / 32767.0f;
  return ret;
}

// ---------------------------------------------------------------------------------------------------------
// what the one-map and the several-map renderer share around their march loops
// ---------------------------------------------------------------------------------------------------------
// the camera and the images of one render launch (filled by fill_ray_camera, raycast.hip)
struct RayCamera {
  Mat4 M, invM;
  float inv_fx, inv_fy, cx, cy;
  float one_over_vs, voxel_size, mu, inv_32767;
  int W, H;
  const float2 *range;
  float4 *raycast;
  uchar4 *out_rgba;
  float *out_float;
  int type;  // dslam_image_type, or -1: raycast only
};

// s: the scene (of several: the first, they agree) whose voxel_size and mu the march uses.  image_out_override: a page-locked
// caller image the kernel stores the pixels of `type` into itself (over PCIe) instead of the render state's image.
int fill_ray_camera(RayCamera &c, const dslam_scene *s, const dslam_render_state *r, const float *M, const float *intr,
                    int type, void *image_out_override = nullptr);

// castRay's set-up: the ray of pixel (x, y) between the depths (zmin, zmax) of its range cell, in voxel units
struct RaySegment {
  Vec3 start, dir;         // dir: unit length
  float total, total_max;  // distance from the camera at the start / at the end
};

__device__ __forceinline__ RaySegment ray_segment(const RayCamera &p, int x, int y, const float2 minmax) {
  RaySegment s;
  Vec4 pc;
  Vec3 pe;
  pc.z = minmax.x;
  pc.x = pc.z * (((float)x - p.cx) * p.inv_fx);
  pc.y = pc.z * (((float)y - p.cy) * p.inv_fy);
  pc.w = 1.0f;
  s.total = sqrtf(pc.x * pc.x + pc.y * pc.y + pc.z * pc.z) * p.one_over_vs;
  Vec4 q = mul(p.invM, pc);
  s.start.x = q.x * p.one_over_vs; s.start.y = q.y * p.one_over_vs; s.start.z = q.z * p.one_over_vs;

  pc.z = minmax.y;
  pc.x = pc.z * (((float)x - p.cx) * p.inv_fx);
  pc.y = pc.z * (((float)y - p.cy) * p.inv_fy);
  pc.w = 1.0f;
  s.total_max = sqrtf(pc.x * pc.x + pc.y * pc.y + pc.z * pc.z) * p.one_over_vs;
  q = mul(p.invM, pc);
  pe.x = q.x * p.one_over_vs; pe.y = q.y * p.one_over_vs; pe.z = q.z * p.one_over_vs;

  s.dir.x = pe.x - s.start.x; s.dir.y = pe.y - s.start.y; s.dir.z = pe.z - s.start.z;
  const float dn = 1.0f / sqrtf(s.dir.x * s.dir.x + s.dir.y * s.dir.y + s.dir.z * s.dir.z);
  s.dir.x *= dn; s.dir.y *= dn; s.dir.z *= dn;
  return s;
}

// castRay behind its loop: a march that ended at sdf <= 0 is refined by two steps of sdf * step_scale, the second with
// the trilinear read at the point the first one reached (trilinear(pt): that read); out = (point, found ? 1 : 0)
template <class Trilinear>
__device__ __forceinline__ bool refine_hit(Vec4 &out, Vec3 res, const Vec3 &dir, float sdf, float step_scale,
                                           Trilinear trilinear) {
  const bool pt_found = sdf <= 0.0f;
  if (pt_found) {
    float step = sdf * step_scale;
    res.x += step * dir.x; res.y += step * dir.y; res.z += step * dir.z;
    sdf = trilinear(res);
    step = sdf * step_scale;
    res.x += step * dir.x; res.y += step * dir.y; res.z += step * dir.z;
  }
  out.x = res.x; out.y = res.y; out.z = res.z; out.w = pt_found ? 1.0f : 0.0f;
  return pt_found;
}

// The pixel `loc` of an image of p.type (>= 0) from its raycast result pr: the depth image, or -- SHADE instantiations --
// the three shaded types (SHADE = false compiles the shading, and with it both callables, away).  normal(pt): the
// un-normalised gradient at the point, colour(pt): the volume's colour there (.x .y .z in 0 .. 1).
template <bool SHADE, class Normal, class Colour>
__device__ __forceinline__ void store_pixel(const RayCamera &p, int loc, const Vec4 &pr, Normal normal, Colour colour) {
  const Vec3 pt = {pr.x, pr.y, pr.z};
  bool found = pr.w > 0;
  if (p.type == DSLAM_IMAGE_DEPTH) {
    float d = 0.0f;
    if (found) {
      Vec4 pw = {pt.x * p.voxel_size, pt.y * p.voxel_size, pt.z * p.voxel_size, 1.0f};
      d = mul(p.M, pw).z;
    }
    p.out_float[loc] = d;
    return;
  }
  if (!SHADE) return;
  Vec3 n = {0, 0, 0};
  float angle = 0.0f;
  if (found) {
    const Vec3 light = {-p.invM.m[8], -p.invM.m[9], -p.invM.m[10]};
    n = normal(pt);
    const float ns = 1.0f / sqrtf(n.x * n.x + n.y * n.y + n.z * n.z);
    n.x *= ns; n.y *= ns; n.z *= ns;
    angle = n.x * light.x + n.y * light.y + n.z * light.z;
    if (!(angle > 0.0f)) found = false;
  }
  uchar4 o = make_uchar4(0, 0, 0, 0);
  if (found) {
    if (p.type == DSLAM_IMAGE_COLOUR_FROM_VOLUME) {
      const auto clr = colour(pt);
      o = make_uchar4((unsigned char)(clr.x * 255.0f), (unsigned char)(clr.y * 255.0f), (unsigned char)(clr.z * 255.0f),
                      255);
    } else if (p.type == DSLAM_IMAGE_COLOUR_FROM_NORMAL) {
      o = make_uchar4((unsigned char)((0.3f + (-n.x + 1.0f) * 0.35f) * 255.0f),
                      (unsigned char)((0.3f + (-n.y + 1.0f) * 0.35f) * 255.0f),
                      (unsigned char)((0.3f + (-n.z + 1.0f) * 0.35f) * 255.0f), 255);
    } else {
      const unsigned char g = (unsigned char)((0.8f * angle + 0.2f) * 255.0f);
      o = make_uchar4(g, g, g, g);
    }
  }
  p.out_rgba[loc] = o;
}

}  // namespace dslam
