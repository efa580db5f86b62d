// mesh_device.h -- what mesh.hip (one scene) and multimesh.hip (several posed scenes) share of the marching-cubes export:
// findVoxel's block search and sdfInterp's zero crossing.  (The live list both walk comes from launch_live_list, live_list.hip.)
#pragma once
#include <hip/hip_runtime.h>

#include "dslam_internal.h"

#pragma clang fp contract(off)

namespace dslam {

// findVoxel's block search: walk the bucket's chain for a resident block at (bx, by, bz); -1 when there is none
__device__ __forceinline__ int find_block_ptr(const HashEntry *hash, int num_buckets, unsigned mask, int bx, int by, int bz) {
  int idx = hash_index(bx, by, bz, mask);
  while (true) {
    const HashEntry he = load_entry(hash, idx);
    if (he.pos[0] == bx && he.pos[1] == by && he.pos[2] == bz && he.ptr >= 0) return he.ptr;
    if (he.offset < 1) return -1;
    idx = num_buckets + he.offset - 1;
  }
}

// sdfInterp: the zero crossing between two corners (positions in voxel units); t is shared with the colour
struct Crossing { float t; int take; };  // take: 1 = first corner, 2 = second corner, 0 = interpolate with t
__device__ __forceinline__ Crossing crossing(float v1, float v2) {
  Crossing r{0.0f, 0};
  if (fabsf(0.0f - v1) < 0.00001f) r.take = 1;
  else if (fabsf(0.0f - v2) < 0.00001f) r.take = 2;
  else if (fabsf(v1 - v2) < 0.00001f) r.take = 1;
  else r.t = (0.0f - v1) / (v2 - v1);
  return r;
}
__device__ __forceinline__ float lerp_value(const Crossing &k, float a, float b) {
  if (k.take == 1) return a;
  if (k.take == 2) return b;
  return a + k.t * (b - a);
}

}  // namespace dslam
