// multimap_device.h -- the posed, weighted cross-map reads shared by multimap.hip (the composite raycast) and multimesh.hip
// (the composite mesh): a map's descriptor, the transform into its frame, the 8-tap cell gather and the running state of
// a combined read (DESIGN.md sections 10 and 12); and, for the host, how every launcher fills a descriptor (section 19).
#pragma once
#include "raycast_device.h"

#pragma clang fp contract(off)

namespace dslam {

// one map of a composite render; T: the first three rows of world -> map, row-major, translation in voxel units
struct MultiMap {
  const HashEntry *hash;
  const uint2 *voxels;
  unsigned mask;
  int num_buckets;
  float T[12];
  int identity;
  int pad;
};
static_assert(sizeof(MultiMap) == kMapDescriptorBytes, "dslam_engine::map_table is sized for this");

// ---- host: a scene's descriptor ----
// the table and the voxels of a scene; T and identity zero, for the caller to fill
inline MultiMap map_of(const dslam_scene *s) {
  MultiMap m;
  memset(&m, 0, sizeof(m));
  m.hash = s->hash; m.voxels = s->voxels; m.mask = (unsigned)(s->p.num_buckets - 1); m.num_buckets = s->p.num_buckets;
  return m;
}
// ... under T16 (world -> map, column-major, metres): T is voxel_pose rounded to float32.  (The translation is divided in
// double and then rounded; a float32 division of the same two float32 values gives the same bits, because a quotient of
// two 24-bit significands rounded to 53 >= 2 * 24 + 2 bits rounds on to 24 bits as the exact quotient does.)
inline MultiMap posed_map(const dslam_scene *s, const float *T16, double voxel_size) {
  MultiMap m = map_of(s);
  double Tv[12];
  voxel_pose(T16, voxel_size, Tv);
  for (int k = 0; k < 12; k++) m.T[k] = (float)Tv[k];
  m.identity = is_identity16(T16) ? 1 : 0;
  return m;
}
// the posed descriptors of a call's n maps, in list order, to dslam_engine::map_table (enqueued on the engine's stream)
inline int upload_posed_maps(dslam_engine *e, const dslam_scene *const *scenes, const float *T, int n, double voxel_size) {
  MultiMap maps[DSLAM_MAX_RENDER_MAPS];
  for (int i = 0; i < n; i++) maps[i] = posed_map(scenes[i], T + 16 * i, voxel_size);
  DSLAM_HIP(hipMemcpyAsync(e->map_table, maps, (size_t)n * sizeof(MultiMap), hipMemcpyHostToDevice, e->stream));
  return DSLAM_OK;
}

// lowest set bit of a wave-uniform mask, as a scalar
__device__ __forceinline__ int first_map(unsigned long long mk) {
  return __builtin_amdgcn_readfirstlane(__builtin_ctzll(mk));
}

__device__ __forceinline__ VolumeRef volume_of(const MultiMap &m) {
  VolumeRef v;
  v.hash = m.hash; v.voxels = m.voxels; v.mask = m.mask; v.num_buckets = m.num_buckets;
  return v;
}

// q = T p: ((t0 x + t1 y) + t2 z) + t3 per row; the identity reads at p itself
__device__ __forceinline__ Vec3 to_map(const MultiMap &m, const Vec3 &p) {
  if (m.identity) return p;
  Vec3 q;
  q.x = ((m.T[0] * p.x + m.T[1] * p.y) + m.T[2] * p.z) + m.T[3];
  q.y = ((m.T[4] * p.x + m.T[5] * p.y) + m.T[6] * p.z) + m.T[7];
  q.z = ((m.T[8] * p.x + m.T[9] * p.y) + m.T[10] * p.z) + m.T[11];
  return q;
}

// the 8 taps (both voxel words) of the trilinear cell at (x0, y0, z0), as gather_taps_batched (which loads the low words only); returns whether
// any tap lies in an allocated block
__device__ __forceinline__ bool gather_cell(const VolumeRef &vol, int x0, int y0, int z0, uint2 t[8]) {
  const int bxa[2] = {x0 >> 3, (x0 + 1) >> 3}, bya[2] = {y0 >> 3, (y0 + 1) >> 3}, bza[2] = {z0 >> 3, (z0 + 1) >> 3};
  int base[8];
  resolve_cell_blocks(vol, bxa, bya, bza, base);
  const unsigned lx[2] = {(unsigned)x0 & 7u, (unsigned)(x0 + 1) & 7u};
  const unsigned ly[2] = {((unsigned)y0 & 7u) << 3, ((unsigned)(y0 + 1) & 7u) << 3};
  const unsigned lz[2] = {((unsigned)z0 & 7u) << 6, ((unsigned)(z0 + 1) & 7u) << 6};
  bool any = false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const unsigned lin = lx[k & 1] | ly[(k >> 1) & 1] | lz[k >> 2];
    const uint2 v = vol.voxels[(size_t)(base[k] < 0 ? 0 : base[k]) + lin];
    t[k] = base[k] < 0 ? make_uint2(kEmptyVoxelLo, kEmptyVoxelHi) : v;
    any |= base[k] >= 0;
  }
  return any;
}

// running state of one combined read
struct Blend {
  int n;            // maps that reported found
  float num, den;   // sum w v, sum w (float32, map order)
  float first;      // value of the first map that reported found
  __device__ void add(float v, float w) {
    if (n == 0) first = v;
    num += w * v;
    den += w;
    n++;
  }
  // two or more found: num / den, or `fallback` for den == 0
  __device__ float value(float fallback) const { return n == 1 ? first : (den > 0.0f ? num / den : fallback); }
};

// one running sum per component (the same law, component by component)
struct Blend3 {
  int n;
  float nx, ny, nz, den;
  Vec3 first;
  __device__ void add(const Vec3 &v, float w) {
    if (n == 0) first = v;
    nx += w * v.x; ny += w * v.y; nz += w * v.z;
    den += w;
    n++;
  }
  __device__ Vec3 value() const {
    if (n == 1 || !(den > 0.0f)) return first;
    Vec3 r = {nx / den, ny / den, nz / den};
    return r;
  }
};

}  // namespace dslam
