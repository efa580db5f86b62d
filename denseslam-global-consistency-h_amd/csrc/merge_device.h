// merge_device.h -- what merge.hip (dslam_merge_maps) and unmerge.hip (dslam_unmerge_maps, dslam_remerge_maps) share, stated
// once.  Device: where a source voxel falls in the destination (merge_target), the look-up of a block in the destination's
// table (merge_probe), the walk over the source's voxels that both mark kernels are (merge_walk), the source read back at a
// destination voxel and packed as a voxel (merge_resample), the pass over the touched blocks that both block kernels are
// (merge_pull).  Host: X~ / Y~ (merge_transforms), the head and the tail of both calls (merge_begin, merge_pull_touched).
#pragma once
#include <cstring>

#include "combine_device.h"

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

// what both mark kernels read: the source, its live list, X~ and the destination's table
struct MergeWalkParams {
  const HashEntry *src_hash;
  const uint2 *src_voxels;
  const int *live_list;
  MultiMap fwd;              // T = X~ (its map pointers are not used)
  const HashEntry *dst_hash;
  unsigned mask;
  int num_buckets;
};

// The look-up of block B in a table, one 16-byte load per chain step.  found: an entry with ptr >= -1 holds B, at index h;
// otherwise h is where the walk stopped -- the slot AllocateSceneFromDepth would use: the bucket head if it is free
// (in_use false), else the end of its chain.
struct MergeProbe { bool found, in_use; int h; };
__device__ __forceinline__ MergeProbe merge_probe(const HashEntry *hash, unsigned mask, int num_buckets, const int B[3]) {
  int h = hash_index(B[0], B[1], B[2], mask);
  HashEntry e = load_entry(hash, h);
  bool found = e.pos[0] == B[0] && e.pos[1] == B[1] && e.pos[2] == B[2] && e.ptr >= -1;
  if (!found && e.ptr >= -1) {
    while (e.offset >= 1) {
      h = num_buckets + e.offset - 1;
      e = load_entry(hash, h);
      if (e.pos[0] == B[0] && e.pos[1] == B[1] && e.pos[2] == B[2] && e.ptr >= -1) { found = true; break; }
    }
  }
  return {found, e.ptr >= -1, h};
}

// a hit: the entry's bit in `touched` (read first: most probes find it set)
__device__ __forceinline__ void merge_touch(unsigned *touched, int h) {
  const unsigned bit = 1u << (h & 31);
  if (!(touched[h >> 5] & bit)) atomicOr(&touched[h >> 5], bit);
}

// The walk of both mark kernels (kMergeGrid x kMergeThreads): every source voxel with w_depth > 0, in the order (rank r of
// its entry in the live list, linear index l), names its destination block B; B is looked up and the outcome handed to
// outcome(probe, r, l, run, n).  Job 2r + k is half k of block r; a workgroup takes the jobs 2b, 2b + 1, 2(b + grid), ...;
// the trip count is the same for every lane of a workgroup.
// Neighbouring lanes are neighbouring voxels of a row and mostly fall into the same block: a lane whose right neighbour
// asks for the same block leaves the probe to it (keys grow with the lane, so the prober's is the largest).  The prober
// answers for its whole run: the lanes between the nearest lane to its left that probes itself or asks for nothing, and
// itself.
// n[COUNTS] are this lane's counts: n[0] candidates and n[1] out of range are the walk's, n[2] (COUNTS == 3) is the
// outcome's, candidates without a block.  They are summed per wavefront and added to mc.
template <int COUNTS, class Outcome>
__device__ __forceinline__ void merge_walk(const MergeWalkParams &p, MergeCounters *mc, Outcome outcome) {
  const int live = mc->live;
  const int lane = threadIdx.x & 63;
  int n[COUNTS] = {};
  for (int job = blockIdx.x * 2; job < live * 2; job += (job & 1) ? gridDim.x * 2 - 1 : 1) {
    const int r = job >> 1, l = (int)threadIdx.x + kMergeThreads * (job & 1);
    const HashEntry he = load_entry(p.src_hash, p.live_list[r]);
    bool cand = false;
    int B[3] = {0, 0, 0};
    if (he.ptr >= 0) {  // (uniform; a live entry holds a block)
      const unsigned own = p.src_voxels[(size_t)he.ptr * kBlock3 + l].x;
      if (((own >> 16) & 0xffu) != 0u) {
        n[0]++;
        cand = merge_target(p.fwd, he, l, B);
        n[1] += cand ? 0 : 1;
      }
    }
    const int rc = __shfl_down((int)cand, 1, 64), rx = __shfl_down(B[0], 1, 64), ry = __shfl_down(B[1], 1, 64), rz = __shfl_down(B[2], 1, 64);
    const bool probes = cand && !(lane < 63 && rc && rx == B[0] && ry == B[1] && rz == B[2]);
    const unsigned long long ends = __ballot(probes || !cand);
    if (!probes) continue;
    const unsigned long long below = ends & ((1ull << lane) - 1ull);
    const int run = lane - (below ? 64 - __clzll((long long)below) : 0) + 1;
    outcome(merge_probe(p.dst_hash, p.mask, p.num_buckets, B), r, l, run, n);
  }
  // integer counts: the order of the additions does not matter
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < COUNTS; k++) n[k] += __shfl_xor(n[k], d, 64);
  }
  unsigned long long *const to[3] = {&mc->candidates, &mc->out_of_range, &mc->without_block};
  if (lane == 0 && n[0]) {
    atomicAdd(to[0], (unsigned long long)n[0]);
#pragma unroll
    for (int k = 1; k < COUNTS; k++)
      if (n[k]) atomicAdd(to[k], (unsigned long long)n[k]);
  }
}

struct MergeBlockParams {
  const HashEntry *dst_hash;
  uint4 *dst_voxels;         // two voxels per element
  const int *touched_list;
  const MergeCounters *mc;
  MultiMap src;              // the source read from the destination's voxel frame: T = Y~
  int max_w, with_colour;
  unsigned long long *changed;   // [gridDim.x][COUNTS of merge_pull]
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

// The pass of both block kernels (kMergeGrid x kMergeThreads): one workgroup per touched destination block at a time
// (grid-stride over the ordered list of touched entries), lane t the voxels 2t and 2t + 1 -- the block moves as 16-byte
// accesses.  Each voxel reads the source at Y~ p' (merge_resample) and hands it to fuse(slo, shi, dlo, dhi, n); a lane
// stores only if one of its voxels changed.  n[COUNTS] are this lane's counts: n[0] voxels changed is the pull's, the
// rest are the fuse's.  One row of COUNTS sums per workgroup goes to p.changed (a workgroup without a block writes zeros).
template <int COUNTS, class Fuse>
__device__ __forceinline__ void merge_pull(const MergeBlockParams &p, Fuse fuse) {
  const int touched = p.mc->touched;
  const VolumeRef vol = volume_of(p.src);
  const int tid = threadIdx.x;
  const int x = (tid & 3) * 2, y = (tid >> 2) & 7, z = tid >> 5;
  int n[COUNTS] = {};
  for (int i = blockIdx.x; i < touched; i += gridDim.x) {
    const HashEntry he = load_entry(p.dst_hash, p.touched_list[i]);
    if (he.ptr < 0) continue;  // (uniform; a touched entry holds a block)
    uint4 *blk = p.dst_voxels + (size_t)he.ptr * (kBlock3 / 2);
    const uint4 was = blk[tid];
    uint4 d = was;
    const int px = he.pos[0] * kBlock + x, py = he.pos[1] * kBlock + y, pz = he.pos[2] * kBlock + z;
    const uint2 s0 = merge_resample(p, vol, px, py, pz);
    const uint2 s1 = merge_resample(p, vol, px + 1, py, pz);
    fuse(s0.x, s0.y, d.x, d.y, n);
    fuse(s1.x, s1.y, d.z, d.w, n);
    const int c = (int)(d.x != was.x || d.y != was.y) + (int)(d.z != was.z || d.w != was.w);
    if (c) blk[tid] = d;
    n[0] += c;
  }
  __shared__ int red[kMergeThreads / 64][COUNTS];
  for (int dlt = 32; dlt > 0; dlt >>= 1) {
#pragma unroll
    for (int k = 0; k < COUNTS; k++) n[k] += __shfl_xor(n[k], dlt, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < COUNTS; k++) red[tid >> 6][k] = n[k];
  }
  __syncthreads();
  if (tid < COUNTS) {
    unsigned long long v = 0;
    for (int w = 0; w < kMergeThreads / 64; w++) v += (unsigned long long)red[w][tid];
    p.changed[(size_t)blockIdx.x * COUNTS + tid] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
// X~ (into fwd) and Y~ = (R^T, -R^T t~) (into inv): formed in double from the float32 X (column-major, metres) and the
// voxel size, rounded to float32; an X that is exactly the identity sets the flag in both.  inv reads the source's volume.
inline void merge_transforms(const dslam_scene *src, const float *X_in, MultiMap &fwd, MultiMap &inv) {
  memset(&fwd, 0, sizeof fwd);
  inv = map_of(src);
  double X[12], Y[12];
  voxel_pose(X_in, (double)src->p.voxel_size, X);
  rigid_inverse(X, Y);
  for (int k = 0; k < 12; k++) { fwd.T[k] = (float)X[k]; inv.T[k] = (float)Y[k]; }
  fwd.identity = inv.identity = is_identity16(X_in) ? 1 : 0;
}

// the head of both calls: the engine's and the merge's scratch, X~ and Y~
inline int merge_begin(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst, const float *X_in, MultiMap &fwd, MultiMap &inv) {
  DSLAM_TRY(ensure_scratch(e, std::max(src->n_entries, dst->n_entries), std::max(src->p.num_local_blocks, dst->p.num_local_blocks)));
  DSLAM_TRY(ensure_merge_scratch(e, src->n_entries, dst->n_entries));
  merge_transforms(src, X_in, fwd, inv);
  return DSLAM_OK;
}

// what both mark kernels are launched with, but for the bitmaps and the counters
template <class Params>
inline void merge_fill_walk(Params &kp, dslam_engine *e, const dslam_scene *src, const dslam_scene *dst, const MultiMap &fwd) {
  memset(&kp, 0, sizeof kp);
  kp.src_hash = src->hash; kp.src_voxels = src->voxels; kp.live_list = e->merge.live_list;
  kp.fwd = fwd;
  kp.dst_hash = dst->hash; kp.mask = (unsigned)(dst->p.num_buckets - 1); kp.num_buckets = dst->p.num_buckets;
}

// the tail of both calls: `touched` as an ordered list, then the block kernel over it with its rows at `changed`;
// between_the_two: what the caller does behind the list and in front of the kernel (the merge's phase clock)
template <class Between>
inline int merge_pull_touched(dslam_engine *e, dslam_scene *dst, const MultiMap &inv, int with_colour, void (*kernel)(MergeBlockParams),
                              const char *name, unsigned long long *changed, Between between_the_two) {
  MergeScratch &m = e->merge;
  DSLAM_TRY(launch_bits_list(e, m.bits + 3 * (size_t)m.words, dst->n_entries, m.touched_list, &m.counters->touched, dst->counters));
  MergeBlockParams bp;
  memset(&bp, 0, sizeof bp);
  bp.dst_hash = dst->hash; bp.dst_voxels = reinterpret_cast<uint4 *>(dst->voxels);
  bp.touched_list = m.touched_list; bp.mc = m.counters;
  bp.src = inv;
  bp.max_w = dst->p.max_w; bp.with_colour = with_colour;
  bp.changed = changed;
  DSLAM_TRY(between_the_two());
  hipLaunchKernelGGL(kernel, dim3(kMergeGrid), dim3(kMergeThreads), 0, e->stream, bp);
  dbg_sync(e, name);
  DSLAM_HIP(hipGetLastError());
  return DSLAM_OK;
}

}  // namespace dslam
