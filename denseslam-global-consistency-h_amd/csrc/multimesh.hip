// multimesh.hip -- one mesh of several local maps, each under its own world -> map transform (dslam_mesh_scene_multi;
// ITMMainEngine::MeshAllLocalMaps in the mirror).
//
// Reference: the export writes one mesh per local map, each in its own coordinates (SaveCurrSceneToMesh per entry of the
// todoList, SystemEntry.cpp:364-370; DenseSlam.cpp:638-643).  The law below is this project's own definition (DESIGN.md
// section 12): the maps are meshed one after the other in list order, map i on its own voxel lattice, with
//   own gate       a cube is skipped when one of its 8 corner voxels of map i is missing or has sdf == 1 (mesh.hip);
//   coverage gate  ... or when an earlier map j < i holds a valid voxel (resident block, w_depth > 0, sdf != 32767) at
//                  iround(A_ij (g + 1/2)): earlier maps own overlapped space, later maps fill what is left;
//   corner values  per lattice point of map i the section-10 combination, in list order, of the own voxel (sdf, w_depth;
//                  colour, w_color) and every other map's trilinear read at A_ij (g + corner);
//   triangles      case table and crossings as mesh.hip, in map-i voxel coordinates; each vertex leaves as (B_i v) * voxel_size.
// A_ij = T~_j T~_i^-1 and B_i = T~_i^-1 (T~: translation in voxel units) are computed on the host in double and rounded
// to float32; row i of the A table is uploaded per map pass.
//
// Order machinery as mesh.hip, per map: live list -> count (one 512-thread workgroup per live block) -> scan -> emit with an
// in-workgroup scan, so the output is map 0's triangles, then map 1's, ..., each in dslam_mesh_scene's order, the same
// bytes on every run.  The host learns each map's total before its emit pass (it sizes the output), so a call costs
// O(num_maps) launches and waits.
//
// A workgroup evaluates the 9 x 9 x 9 lattice points its block's cubes touch ONCE into LDS (combined sdf, colour, own-gate
// flag; the +1 planes come from the 7 neighbour blocks) and reads the cubes' corners from there: the cross-map gathers are
// done once per point, not once per cube corner.  Before that it finds the other maps that can reach the block at all
// (the block's lattice box under A_ij against map j's hash: at most 3 x 3 x 3 block positions, one thread each); a block no
// other map reaches pays for the own voxels only.  That mask is a pure optimisation -- the law defines the result.
// Bound: gather latency, as mesh.hip; an offline export -- no roofline claim.
#include <climits>
#include <cmath>
#include <cstring>

#include "dslam_internal.h"
#include "mc_tables.h"
#include "mesh_device.h"
#include "multimap_device.h"

#pragma clang fp contract(off)

namespace dslam {

// this translation unit's copy of the case table (constant memory is per code object)
__constant__ signed char d_mm_triangles[256][16];

constexpr int kLattice = 9 * 9 * 9;

struct MultiMeshParams {
  const HashEntry *hash;     // map i, the map being meshed
  const uint2 *voxels;
  int num_buckets;
  unsigned mask;
  const int *live_list;      // as MeshParams
  const int *live_count;
  int *block_counts;
  const int *block_offsets;
  const MultiMap *maps;      // [num_maps] map j as read from map i's voxel frame: T = A_ij (slot i: the identity, not read)
  int self, num_maps;
  float B[12];               // map-i voxels -> world voxels (first three rows, row-major)
  int b_identity;
  float *positions;          // [limit][3][3]: this map's part of the output
  float *colours;
  float factor;
  int limit;                 // triangles of this map with rank >= limit are dropped
};

__device__ __forceinline__ int mm_triangles_of_case(int cube) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < 15; i += 3) n += d_mm_triangles[cube][i] >= 0;
  return n;
}

__device__ __forceinline__ int lattice_offset(int corner) {
  return mc_corner_x(corner) + 9 * mc_corner_y(corner) + 81 * mc_corner_z(corner);
}

// Which other maps can hold a tap of the block's lattice points or a cube centre: map j's resident blocks under the
// axis-aligned bounds of A_ij [g0, g0 + 8]^3 (+ the tap at +1, + 1/16 voxel for the rounding of the transform).  One thread
// per (map, block position); bounds wider than 3 blocks (a transform that scales) make the map a candidate outright.
__device__ __forceinline__ void find_candidates(const MultiMeshParams &p, const HashEntry &he, unsigned *s_cand) {
  const float g0x = (float)(he.pos[0] * kBlock), g0y = (float)(he.pos[1] * kBlock), g0z = (float)(he.pos[2] * kBlock);
  for (int idx = threadIdx.x; idx < p.num_maps * 27; idx += blockDim.x) {
    const int j = idx / 27, k = idx - j * 27;
    if (j == p.self) continue;
    const MultiMap &m = p.maps[j];
    Vec3 lo = {3.0e38f, 3.0e38f, 3.0e38f}, hi = {-3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const Vec3 pt = {g0x + (float)((c & 1) * kBlock), g0y + (float)(((c >> 1) & 1) * kBlock), g0z + (float)((c >> 2) * kBlock)};
      const Vec3 q = to_map(m, pt);
      lo.x = fminf(lo.x, q.x); lo.y = fminf(lo.y, q.y); lo.z = fminf(lo.z, q.z);
      hi.x = fmaxf(hi.x, q.x); hi.y = fmaxf(hi.y, q.y); hi.z = fmaxf(hi.z, q.z);
    }
    const float eps = 0.0625f;
    const int bx0 = (int)floorf(lo.x - eps) >> 3, bx1 = ((int)floorf(hi.x + eps) + 1) >> 3;
    const int by0 = (int)floorf(lo.y - eps) >> 3, by1 = ((int)floorf(hi.y + eps) + 1) >> 3;
    const int bz0 = (int)floorf(lo.z - eps) >> 3, bz1 = ((int)floorf(hi.z + eps) + 1) >> 3;
    bool reach;
    if (bx1 - bx0 > 2 || by1 - by0 > 2 || bz1 - bz0 > 2) {
      reach = true;
    } else {
      const int bx = bx0 + k % 3, by = by0 + (k / 3) % 3, bz = bz0 + k / 9;
      reach = bx <= bx1 && by <= by1 && bz <= bz1 && find_block_ptr(m.hash, m.num_buckets, m.mask, bx, by, bz) >= 0;
    }
    if (reach) atomicOr(&s_cand[j >> 5], 1u << (j & 31));
  }
}

// count (EMIT = false): block_counts[b] = triangles of live block b.  emit: the same evaluation, every triangle to its slot.
template <bool EMIT, bool COLOUR>
__global__ __launch_bounds__(512) void k_multimesh(MultiMeshParams p) {
  __shared__ int nb_ptr[8];
  __shared__ int wave_sums[8];
  __shared__ unsigned s_cand[2];
  __shared__ float s_val[kLattice];                  // combined sdf per lattice point
  __shared__ float s_rgb[COLOUR ? 3 : 1][kLattice];  // combined colour, 0 .. 255
  __shared__ unsigned char s_bad[kLattice + 3];      // own voxel missing or sdf == 1
  const int live = *p.live_count;
  const int x = threadIdx.x & 7, y = (threadIdx.x >> 3) & 7, z = threadIdx.x >> 6;
  for (int b = blockIdx.x; b < live; b += gridDim.x) {
    if (EMIT && p.block_counts[b] == 0) continue;  // uniform over the workgroup
    const HashEntry he = load_entry(p.hash, p.live_list[b]);
    // the block's own slot and the 7 blocks at +x, +y, +z (resolve_neighbours of mesh.hip)
    if (threadIdx.x < 8) {
      const int ox = threadIdx.x & 1, oy = (threadIdx.x >> 1) & 1, oz = threadIdx.x >> 2;
      nb_ptr[threadIdx.x] = threadIdx.x == 0 ? he.ptr
                                             : find_block_ptr(p.hash, p.num_buckets, p.mask, he.pos[0] + ox, he.pos[1] + oy, he.pos[2] + oz);
    } else if (threadIdx.x < 10) {
      s_cand[threadIdx.x - 8] = 0u;
    }
    __syncthreads();
    if (p.num_maps > 1) {
      find_candidates(p, he, s_cand);
      __syncthreads();
    }
    const unsigned long long cand = ((unsigned long long)__builtin_amdgcn_readfirstlane(s_cand[1]) << 32) |
                                    __builtin_amdgcn_readfirstlane(s_cand[0]);

    // ---- the lattice: every point once ----
    for (int l = threadIdx.x; l < kLattice; l += blockDim.x) {
      const int lx = l % 9, ly = (l / 9) % 9, lz = l / 81;
      const int ptr = nb_ptr[(lx >> 3) | ((ly >> 3) << 1) | ((lz >> 3) << 2)];
      uint2 v = make_uint2(kEmptyVoxelLo, kEmptyVoxelHi);
      if (ptr >= 0) v = p.voxels[(size_t)ptr * kBlock3 + (lx & 7) + (ly & 7) * kBlock + (lz & 7) * kBlock * kBlock];
      const float s = sdf_to_float((short)(v.x & 0xffffu));
      const Vec3 own = {(float)(v.x >> 24), (float)(v.y & 0xffu), (float)((v.y >> 8) & 0xffu)};
      float val = s;
      Vec3 rgb = own;
      if (cand) {
        const Vec3 pt = {(float)(he.pos[0] * kBlock + lx), (float)(he.pos[1] * kBlock + ly), (float)(he.pos[2] * kBlock + lz)};
        Blend bs = {0, 0.0f, 0.0f, 0.0f};
        Blend3 bc = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
        unsigned long long mk = cand | (1ull << p.self);
        while (mk) {
          const int j = first_map(mk);
          mk &= mk - 1;
          if (j == p.self) {
            if (ptr >= 0) {
              bs.add(s, (float)((v.x >> 16) & 0xffu));
              if (COLOUR) bc.add(own, (float)((v.y >> 16) & 0xffu));
            }
            continue;
          }
          const MultiMap &m = p.maps[j];
          const Vec3 q = to_map(m, pt);
          const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
          uint2 t[8];
          if (!gather_cell(volume_of(m), (int)fx, (int)fy, (int)fz, t)) continue;
          const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
          float wt[8];
#pragma unroll
          for (int k = 0; k < 8; k++) wt[k] = (float)((t[k].x >> 16) & 0xffu);
          bs.add(trilinear_sdf(t, cx, cy, cz), lerp8(wt, cx, cy, cz));
          if (COLOUR) {
            const Vec4 c4 = colour_from_taps(t, cx, cy, cz);
            const Vec3 c3 = {c4.x * 255.0f, c4.y * 255.0f, c4.z * 255.0f};
#pragma unroll
            for (int k = 0; k < 8; k++) wt[k] = (float)((t[k].y >> 16) & 0xffu);
            bc.add(c3, lerp8(wt, cx, cy, cz));
          }
        }
        // only the own map found: its value as it is; sum w == 0: the own map's value
        if (bs.n > 1 && bs.den > 0.0f) val = bs.num / bs.den;
        if (COLOUR && bc.n > 1 && bc.den > 0.0f) { rgb.x = bc.nx / bc.den; rgb.y = bc.ny / bc.den; rgb.z = bc.nz / bc.den; }
      }
      s_val[l] = val;
      s_bad[l] = (ptr < 0 || s == 1.0f) ? 1 : 0;
      if (COLOUR) { s_rgb[0][l] = rgb.x; s_rgb[1][l] = rgb.y; s_rgb[2][l] = rgb.z; }
    }
    __syncthreads();

    // ---- the cube of this thread ----
    const int l0 = x + 9 * y + 81 * z;
    int cube = 0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int l = l0 + lattice_offset(k);
      if (s_bad[l]) ok = false;
      if (s_val[l] < 0.0f) cube |= 1 << k;
    }
    ok = ok && mc_edge_mask(cube) != 0;
    const int gxi = he.pos[0] * kBlock + x, gyi = he.pos[1] * kBlock + y, gzi = he.pos[2] * kBlock + z;
    unsigned long long earlier = cand & ((1ull << p.self) - 1ull);
    if (earlier) {
      const Vec3 centre = {(float)gxi + 0.5f, (float)gyi + 0.5f, (float)gzi + 0.5f};
      IndexCache cache = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
      while (earlier) {
        const int j = first_map(earlier);
        earlier &= earlier - 1;
        if (!ok) continue;
        const MultiMap &m = p.maps[j];
        const Vec3 c = to_map(m, centre);
        const int vx = iround(c.x), vy = iround(c.y), vz = iround(c.z);
        cache.bx = 0x7fffffff;  // (one entry, and the next map is another table)
        const int base = lookup_block(volume_of(m), vx >> 3, vy >> 3, vz >> 3, cache);
        if (base >= 0) {
          const unsigned raw = m.voxels[(size_t)base + (unsigned)((vx & 7) | ((vy & 7) << 3) | ((vz & 7) << 6))].x;
          if (((raw >> 16) & 0xffu) != 0u && (raw & 0xffffu) != 0x7fffu) ok = false;
        }
      }
    }
    const int n = ok ? mm_triangles_of_case(cube) : 0;
    int total;
    int rank = block_excl_scan<8>(n, wave_sums, total);
    if (!EMIT) {
      if (threadIdx.x == 0) p.block_counts[b] = total;
    } else if (n > 0) {
      rank += p.block_offsets[b];
      const float gx = (float)gxi, gy = (float)gyi, gz = (float)gzi;
      for (int i = 0; i < 3 * n; i += 3, rank++) {
        if (rank >= p.limit) break;
        float *out = p.positions + (size_t)rank * 9;
        float *col = COLOUR ? p.colours + (size_t)rank * 9 : nullptr;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const int e = d_mm_triangles[cube][i + k];
          const int a = mc_edge_first(e), bb = mc_edge_second(e);
          const int la = l0 + lattice_offset(a), lb = l0 + lattice_offset(bb);
          const Crossing cr = crossing(s_val[la], s_val[lb]);
          const float ax = gx + (float)mc_corner_x(a), ay = gy + (float)mc_corner_y(a), az = gz + (float)mc_corner_z(a);
          const float bx = gx + (float)mc_corner_x(bb), by = gy + (float)mc_corner_y(bb), bz = gz + (float)mc_corner_z(bb);
          float vx = lerp_value(cr, ax, bx), vy = lerp_value(cr, ay, by), vz = lerp_value(cr, az, bz);
          if (!p.b_identity) {
            const float wx = ((p.B[0] * vx + p.B[1] * vy) + p.B[2] * vz) + p.B[3];
            const float wy = ((p.B[4] * vx + p.B[5] * vy) + p.B[6] * vz) + p.B[7];
            const float wz = ((p.B[8] * vx + p.B[9] * vy) + p.B[10] * vz) + p.B[11];
            vx = wx; vy = wy; vz = wz;
          }
          out[3 * k + 0] = vx * p.factor;
          out[3 * k + 1] = vy * p.factor;
          out[3 * k + 2] = vz * p.factor;
          if (COLOUR) {
            col[3 * k + 0] = lerp_value(cr, s_rgb[0][la], s_rgb[0][lb]) / 255.0f;
            col[3 * k + 1] = lerp_value(cr, s_rgb[1][la], s_rgb[1][lb]) / 255.0f;
            col[3 * k + 2] = lerp_value(cr, s_rgb[2][la], s_rgb[2][lb]) / 255.0f;
          }
        }
      }
    }
    __syncthreads();  // nb_ptr / s_cand / the lattice are rewritten by the next block
  }
}

__global__ __launch_bounds__(1024) void k_multimesh_scan(const int *block_counts, int *block_offsets, const int *live_count,
                                                         int *total_out) {
  int totals[1];
  scan_tiles<1>(block_counts, block_offsets, *live_count, totals);
  if (threadIdx.x == 0) *total_out = totals[0];
}

// inverse of an affine transform [R | t] (R by its adjugate; the caller has checked that T is not singular)
static void invert_affine(const double a[12], double out[12]) {
  const double r00 = a[0], r01 = a[1], r02 = a[2], r10 = a[4], r11 = a[5], r12 = a[6], r20 = a[8], r21 = a[9], r22 = a[10];
  const double c00 = r11 * r22 - r12 * r21, c01 = r02 * r21 - r01 * r22, c02 = r01 * r12 - r02 * r11;
  const double c10 = r12 * r20 - r10 * r22, c11 = r00 * r22 - r02 * r20, c12 = r02 * r10 - r00 * r12;
  const double c20 = r10 * r21 - r11 * r20, c21 = r01 * r20 - r00 * r21, c22 = r00 * r11 - r01 * r10;
  const double det = r00 * c00 + r01 * c10 + r02 * c20;
  const double inv[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
  for (int row = 0; row < 3; row++) {
    for (int col = 0; col < 3; col++) out[row * 4 + col] = inv[row * 3 + col];
    out[row * 4 + 3] = -(inv[row * 3 + 0] * a[3] + inv[row * 3 + 1] * a[7] + inv[row * 3 + 2] * a[11]);
  }
}

// c = a b for affine transforms (first three rows)
static void compose_affine(const double a[12], const double b[12], double c[12]) {
  for (int row = 0; row < 3; row++)
    for (int col = 0; col < 4; col++) {
      double acc = col == 3 ? a[row * 4 + 3] : 0.0;
      for (int k = 0; k < 3; k++) acc += a[row * 4 + k] * b[k * 4 + col];
      c[row * 4 + col] = acc;
    }
}

static void set_identity(float T[12]) {
  for (int i = 0; i < 12; i++) T[i] = (i % 5) == 0 ? 1.0f : 0.0f;
}

// room for `triangles` in the engine's mesh buffers, the first `keep` triangles preserved (keep == 0: the old mesh goes
// first, as launch_mesh_scene; otherwise the buffers at least double, so a call copies O(its size)).  On failure the
// engine has no mesh buffers and mesh_bytes == 0.
static int reserve_mesh(dslam_engine *e, int triangles, int keep, int with_colour) {
  const size_t need = (size_t)(triangles > 0 ? triangles : 1) * 9 * sizeof(float);
  if (need <= e->mesh_bytes && (!with_colour || e->mesh_colours)) return DSLAM_OK;
  size_t bytes = need > e->mesh_bytes ? need : e->mesh_bytes;
  DeviceBuffer<float> positions, colours;
  int rc = DSLAM_OK;
  if (keep == 0) {
    e->mesh_positions.reset(); e->mesh_colours.reset();
    e->mesh_bytes = 0;
    rc = positions.alloc(bytes / sizeof(float));
    if (!rc && with_colour) rc = colours.alloc(bytes / sizeof(float));
  } else {
    if (bytes < 2 * e->mesh_bytes) bytes = 2 * e->mesh_bytes;
    const size_t kept = (size_t)keep * 9 * sizeof(float);
    rc = positions.alloc(bytes / sizeof(float));
    if (!rc && with_colour) rc = colours.alloc(bytes / sizeof(float));
    hipError_t err = hipSuccess;
    if (!rc) err = hipMemcpyAsync(positions, e->mesh_positions, kept, hipMemcpyDeviceToDevice, e->stream);
    if (!rc && err == hipSuccess && with_colour)
      err = hipMemcpyAsync(colours, e->mesh_colours, kept, hipMemcpyDeviceToDevice, e->stream);
    if (!rc && err == hipSuccess) err = hipStreamSynchronize(e->stream);   // (the old buffers go below)
    e->mesh_positions.reset(); e->mesh_colours.reset();
    e->mesh_bytes = 0;
    if (!rc) DSLAM_HIP(err);
  }
  if (rc) return rc;
  e->mesh_positions = std::move(positions); e->mesh_colours = std::move(colours); e->mesh_bytes = bytes;
  return DSLAM_OK;
}

// scenes / T (N x 16, world -> map, column-major, metres) already checked by dslam_mesh_scene_multi
int launch_mesh_scene_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T, int n, int max_triangles,
                            int with_colour, int *out_num, int32_t *out_map) {
  if (!e->multimesh_table_ready) {
    DSLAM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_mm_triangles), kMcTriangles, sizeof(kMcTriangles)));
    e->multimesh_table_ready = true;
  }
  int max_entries = 0, max_local = 0;
  for (int i = 0; i < n; i++) {
    max_entries = std::max(max_entries, scenes[i]->n_entries);
    max_local = std::max(max_local, scenes[i]->p.num_local_blocks);
  }
  DSLAM_TRY(ensure_scratch(e, max_entries, max_local));
  const double vs = (double)scenes[0]->p.voxel_size;
  std::vector<double> Tv((size_t)n * 12), Bv((size_t)n * 12);
  for (int i = 0; i < n; i++) {
    voxel_pose(T + 16 * i, vs, &Tv[(size_t)i * 12]);
    invert_affine(&Tv[(size_t)i * 12], &Bv[(size_t)i * 12]);
  }
  int *live_count = e->misc_counter + 8, *total = e->misc_counter + 9;
  int *host = reinterpret_cast<int *>(e->pinned.get());
  const int grid = e->sm_count * 4;
  const int limit = max_triangles > 1 ? max_triangles - 1 : 0;   // the list saturates at max_triangles - 1
  int acc = 0;
  e->mesh_triangles = 0;
  e->mesh_has_colour = with_colour != 0;
  MultiMap row[DSLAM_MAX_RENDER_MAPS];
  for (int i = 0; i < n; i++) {
    const dslam_scene *s = scenes[i];
    int n_i = 0;
    if (acc < limit) {
      // row i of the A table: map j read from map i's voxel frame
      for (int j = 0; j < n; j++) {
        MultiMap &m = row[j] = map_of(scenes[j]);
        if (memcmp(T + 16 * i, T + 16 * j, 16 * sizeof(float)) == 0) {
          m.identity = 1;
          set_identity(m.T);
        } else {
          double A[12];
          compose_affine(&Tv[(size_t)j * 12], &Bv[(size_t)i * 12], A);
          for (int k = 0; k < 12; k++) m.T[k] = (float)A[k];
        }
      }
      DSLAM_HIP(hipMemcpyAsync(e->map_table, row, (size_t)n * sizeof(MultiMap), hipMemcpyHostToDevice, e->stream));
      DSLAM_TRY(launch_live_list(e, s, e->list_a, live_count));
      MultiMeshParams p;
      p.hash = s->hash; p.voxels = s->voxels; p.num_buckets = s->p.num_buckets; p.mask = (unsigned)(s->p.num_buckets - 1);
      p.live_list = e->list_a; p.live_count = live_count; p.block_counts = e->list_b; p.block_offsets = e->list_c;
      p.maps = static_cast<const MultiMap *>(e->map_table.get());
      p.self = i; p.num_maps = n;
      p.b_identity = is_identity16(T + 16 * i) ? 1 : 0;
      for (int k = 0; k < 12; k++) p.B[k] = (float)Bv[(size_t)i * 12 + k];
      p.positions = nullptr; p.colours = nullptr; p.factor = s->p.voxel_size; p.limit = 0;
      // (the count pass needs no colours: the case index and both gates come from the sdf values alone)
      hipLaunchKernelGGL((k_multimesh<false, false>), dim3(grid), dim3(512), 0, e->stream, p);
      hipLaunchKernelGGL(k_multimesh_scan, dim3(1), dim3(1024), 0, e->stream, e->list_b, e->list_c, live_count, total);
      DSLAM_HIP(hipGetLastError());
      DSLAM_HIP(hipMemcpyAsync(host, total, sizeof(int), hipMemcpyDeviceToHost, e->stream));
      DSLAM_HIP(hipStreamSynchronize(e->stream));
      n_i = host[0] < limit - acc ? host[0] : limit - acc;
      if (n_i > 0) {
        DSLAM_TRY(reserve_mesh(e, acc + n_i, acc, with_colour));
        p.positions = e->mesh_positions.get() + (size_t)acc * 9;
        p.colours = with_colour ? e->mesh_colours.get() + (size_t)acc * 9 : nullptr;
        p.limit = n_i;
        if (with_colour) hipLaunchKernelGGL((k_multimesh<true, true>), dim3(grid), dim3(512), 0, e->stream, p);
        else hipLaunchKernelGGL((k_multimesh<true, false>), dim3(grid), dim3(512), 0, e->stream, p);
        DSLAM_HIP(hipGetLastError());
      }
    }
    if (out_map) out_map[i] = n_i;
    acc += n_i;
  }
  if (acc == 0) DSLAM_TRY(reserve_mesh(e, 0, 0, with_colour));   // an empty mesh still has its buffers, as dslam_mesh_scene's
  e->mesh_triangles = acc;
  *out_num = acc;
  return DSLAM_OK;
}

}  // namespace dslam
