// merge_device.h -- the resampled voxel of the map merge, stated once for merge.hip (dslam_merge_maps) and unmerge.hip
// (dslam_unmerge_maps, dslam_remerge_maps): where a source voxel falls in the destination (merge_target), the source read
// back at a destination voxel and packed as a voxel (merge_resample), and X~ / Y~ as both calls form them on the host.
#pragma once
#include <cstring>

#include "mesh_device.h"
#include "multimap_device.h"

#pragma clang fp contract(off)

namespace dslam {

constexpr int kMergeGrid = 512;      // workgroups of the mark and block kernels: two per CU of an MI355X
constexpr int kMergeThreads = 256;

// the destination block a source voxel falls into; false: outside the table's short range
__device__ __forceinline__ bool merge_target(const MultiMap &fwd, const HashEntry &he, int l, int B[3]) {
  const Vec3 p = {(float)(he.pos[0] * kBlock + (l & 7)), (float)(he.pos[1] * kBlock + ((l >> 3) & 7)), (float)(he.pos[2] * kBlock + (l >> 6))};
  const Vec3 q = to_map(fwd, p);
  const float tx = floorf(q.x + 0.5f), ty = floorf(q.y + 0.5f), tz = floorf(q.z + 0.5f);
  const bool ok = tx >= -262144.0f && tx < 262144.0f && ty >= -262144.0f && ty < 262144.0f && tz >= -262144.0f && tz < 262144.0f;
  B[0] = ok ? (int)tx >> 3 : 0;
  B[1] = ok ? (int)ty >> 3 : 0;
  B[2] = ok ? (int)tz >> 3 : 0;
  return ok;
}

struct MergeBlockParams {
  const HashEntry *dst_hash;
  uint4 *dst_voxels;         // two voxels per element
  const int *touched_list;
  const MergeCounters *mc;
  MultiMap src;              // the source read from the destination's voxel frame: T = Y~
  int max_w, with_colour;
  unsigned long long *changed;   // [gridDim.x]
};

// the source resampled at the destination voxel (px, py, pz), packed as a voxel; the empty voxel where the source has
// nothing to give
__device__ __forceinline__ uint2 merge_resample(const MergeBlockParams &p, const VolumeRef &vol, int px, int py, int pz) {
  const uint2 empty = make_uint2(kEmptyVoxelLo, kEmptyVoxelHi);
  if (p.src.identity) {
    const int ptr = find_block_ptr(vol.hash, vol.num_buckets, vol.mask, px >> 3, py >> 3, pz >> 3);
    if (ptr < 0) return empty;
    uint2 v = vol.voxels[(size_t)ptr * kBlock3 + ((px & 7) | ((py & 7) << 3) | ((pz & 7) << 6))];
    if (!p.with_colour) v.y &= 0xff00ffffu;
    return v;
  }
  const Vec3 pt = {(float)px, (float)py, (float)pz};
  const Vec3 q = to_map(p.src, pt);
  // a block coordinate outside the short range is never resident (and this keeps the casts below defined)
  if (!(fabsf(q.x) < 262144.0f && fabsf(q.y) < 262144.0f && fabsf(q.z) < 262144.0f)) return empty;
  const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
  uint2 t[8];
  if (!gather_cell(vol, (int)fx, (int)fy, (int)fz, t)) return empty;
  unsigned wd = 255u, wc = 255u;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const unsigned a = (t[k].x >> 16) & 0xffu, c = (t[k].y >> 16) & 0xffu;
    wd = a < wd ? a : wd;
    wc = c < wc ? c : wc;
    s[k] = sdf_to_float((short)(t[k].x & 0xffffu));
  }
  if (wd == 0u) return empty;
  const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
  uint2 out;
  out.x = (unsigned)(unsigned short)float_to_sdf(lerp8(s, cx, cy, cz)) | (wd << 16);
  out.y = 0u;
  if (p.with_colour && wc != 0u) {
    float c0[8], c1[8], c2[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { c0[k] = (float)(t[k].x >> 24); c1[k] = (float)(t[k].y & 0xffu); c2[k] = (float)((t[k].y >> 8) & 0xffu); }
    out.x |= (unsigned)(unsigned char)(lerp8(c0, cx, cy, cz) + 0.5f) << 24;
    out.y = (unsigned)(unsigned char)(lerp8(c1, cx, cy, cz) + 0.5f) | ((unsigned)(unsigned char)(lerp8(c2, cx, cy, cz) + 0.5f) << 8) | (wc << 16);
  }
  return out;
}

// X~ (into fwd) and Y~ = (R^T, -R^T t~) (into inv): formed in double from the float32 X (column-major, metres) and the
// voxel size, rounded to float32; an X that is exactly the identity sets the flag in both.  inv reads the source's volume.
inline void merge_transforms(const dslam_scene *src, const float *X_in, MultiMap &fwd, MultiMap &inv) {
  memset(&fwd, 0, sizeof fwd);
  memset(&inv, 0, sizeof inv);
  const double vs = (double)src->p.voxel_size;
  double R[3][3], t[3];
  bool identity = true;
  for (int i = 0; i < 16; i++) identity = identity && X_in[i] == ((i % 5) == 0 ? 1.0f : 0.0f);
  for (int row = 0; row < 3; row++) {
    for (int col = 0; col < 3; col++) R[row][col] = (double)X_in[col * 4 + row];
    t[row] = (double)X_in[12 + row] / vs;
  }
  for (int row = 0; row < 3; row++) {
    for (int col = 0; col < 3; col++) {
      fwd.T[row * 4 + col] = (float)R[row][col];
      inv.T[row * 4 + col] = (float)R[col][row];
    }
    fwd.T[row * 4 + 3] = (float)t[row];
    inv.T[row * 4 + 3] = (float)-((R[0][row] * t[0] + R[1][row] * t[1]) + R[2][row] * t[2]);
  }
  fwd.identity = inv.identity = identity ? 1 : 0;
  inv.hash = src->hash; inv.voxels = src->voxels;
  inv.mask = (unsigned)(src->p.num_buckets - 1); inv.num_buckets = src->p.num_buckets;
}

}  // namespace dslam
