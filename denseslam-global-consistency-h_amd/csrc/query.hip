// query.hip -- the maps at any point or along any ray (dslam_query_points, dslam_cast_rays): the posed,
// weighted cross-map reads of the composite raycast (multimap.hip; the law of DESIGN.md section 10) without a camera.
// One lane per element; every lane visits every map of the call, in list order, so the map mask is all ones over the
// list -- a kernel argument, wave-uniform, and the scalar find-first-set loop of k_render_multi is kept.
//
// The combined reads below (q_trilinear, q_nearest, q_normal, q_colour, q_world_dir) are COPIES of multimap.hip's
// multi_trilinear, the nearest read of cast_ray_multi's loop body, k_render_multi's normal and colour lambdas and
// to_world_dir, taking the map table and the mask instead of MultiRenderParams.  They are copies, not a move into
// multimap_device.h, on purpose: with the reads moved and multimap.hip calling them there, the gfx950 code of
// k_render_multi came out with another block order and scalar schedule (the same VGPRs, 117 / 155), and the composite
// raycast's code generation is not to change with this file.  Keep the two in step; every test of test_gpu_query.py that
// compares against float64 holds these to the law the composite raycast is held to.
#include <cmath>
#include <cstdio>

#include "dslam_bits.h"
#include "multimap_device.h"
#include "raycast_device.h"

#pragma clang fp contract(off)

namespace dslam {

// a gradient of the map frame back into the world frame: R^T g
__device__ __forceinline__ Vec3 q_world_dir(const MultiMap &m, const Vec3 &g) {
  if (m.identity) return g;
  Vec3 r;
  r.x = (m.T[0] * g.x + m.T[4] * g.y) + m.T[8] * g.z;
  r.y = (m.T[1] * g.x + m.T[5] * g.y) + m.T[9] * g.z;
  r.z = (m.T[2] * g.x + m.T[6] * g.y) + m.T[10] * g.z;
  return r;
}

// combined trilinear sdf read at world position pt (voxel units); `first_any`: the first map's read (all of its taps
// empty when no map reports found -- what a single-map read returns there).  den_out: the law's sum of the weights (the
// trilinear w_depth of every map that reported found, in list order); found_out: bit i = map i reported found
__device__ __forceinline__ float q_trilinear(const MultiMap *maps, unsigned long long mk, const Vec3 &pt, float &den_out,
                                             unsigned long long &found_out) {
  Blend b = {0, 0.0f, 0.0f, 0.0f};
  float first_any = 1.0f;
  bool have_any = false;
  unsigned long long found_mk = 0ull;
  while (mk) {
    const int i = first_map(mk);
    mk &= mk - 1;
    const MultiMap &m = maps[i];
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
    if (found) { b.add(v, lerp8(wt, cx, cy, cz)); found_mk |= 1ull << i; }
  }
  den_out = b.den;
  found_out = found_mk;
  return b.n == 0 ? first_any : b.value(1.0f);
}
__device__ __forceinline__ float q_trilinear(const MultiMap *maps, unsigned long long mk, const Vec3 &pt) {
  float den;
  unsigned long long found;
  return q_trilinear(maps, mk, pt, den, found);
}

// the combined nearest-voxel read of a march step (b.n == 0: no map holds the voxel); cache: the lane's one-entry block
// cache, tagged with its map
__device__ __forceinline__ Blend q_nearest(const MultiMap *maps, unsigned long long mk, const Vec3 &pt, float inv_32767,
                                           IndexCache &cache, int &cache_map) {
  Blend b = {0, 0.0f, 0.0f, 0.0f};
  while (mk) {
    const int i = first_map(mk);
    mk &= mk - 1;
    const MultiMap &m = maps[i];
    const Vec3 qm = to_map(m, pt);
    const int vx = iround(qm.x), vy = iround(qm.y), vz = iround(qm.z);
    if (cache_map != i) { cache.bx = 0x7fffffff; cache_map = i; }
    const int base = lookup_block(volume_of(m), vx >> 3, vy >> 3, vz >> 3, cache);
    if (base >= 0) {
      const unsigned raw = m.voxels[(size_t)base + (unsigned)((vx & 7) | ((vy & 7) << 3) | ((vz & 7) << 6))].x;
      b.add(div_exact((float)(short)(raw & 0xffffu), 32767.0f, inv_32767), (float)((raw >> 16) & 0xffu));
    }
  }
  return b;
}

// combined 6-tap gradient (un-normalised, world frame): confidence = trilinear w_depth at the point
__device__ __forceinline__ Vec3 q_normal(const MultiMap *maps, unsigned long long mk, const Vec3 &pt) {
  Blend3 b = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
  Vec3 first_any = {0.0f, 0.0f, 0.0f};
  bool have_any = false;
  while (mk) {
    const int i = first_map(mk);
    mk &= mk - 1;
    const MultiMap &m = maps[i];
    const VolumeRef vol = volume_of(m);
    const Vec3 q = to_map(m, pt);
    IndexCache c = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
    const Vec3 g = q_world_dir(m, normal_from_sdf(vol, q, c));
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
}

// combined colour (0 .. 1): confidence = trilinear w_color
__device__ __forceinline__ Vec3 q_colour(const MultiMap *maps, unsigned long long mk, const Vec3 &pt) {
  Blend3 b = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
  Vec3 first_any = {0.0f, 0.0f, 0.0f};
  bool have_any = false;
  while (mk) {
    const int i = first_map(mk);
    mk &= mk - 1;
    const MultiMap &m = maps[i];
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
}

// ---------------------------------------------------------------------------------------------------------------------
struct QueryParams {
  const MultiMap *maps;
  unsigned long long mask;   // bits 0 .. num_maps - 1
  int n, what;
  float one_over_vs, voxel_size, mu, inv_32767;
  float max_range;           // rays: metres, already defaulted and checked
};

constexpr float kQueryMaxCoord = 1048576.0f;   // 2^20 voxels

// a world point in metres -> voxel units, as ray_segment scales its points; false: a coordinate is not finite or lies
// beyond +-2^20 voxels (the comparison is false for a NaN)
__device__ __forceinline__ bool query_voxel_point(const QueryParams &p, float x, float y, float z, Vec3 &pv) {
  pv.x = x * p.one_over_vs; pv.y = y * p.one_over_vs; pv.z = z * p.one_over_vs;
  return fabsf(pv.x) <= kQueryMaxCoord && fabsf(pv.y) <= kQueryMaxCoord && fabsf(pv.z) <= kQueryMaxCoord;
}

// The gradient and the colour both kernels give for the world point (x, y, z) in metres: k_query_points for its points,
// k_cast_rays for its hit points -- one function, so a point query at a ray's `point` returns the ray's bits.  A field
// `what` does not ask for, and every field of a point outside the range, is 0.
__device__ __forceinline__ void query_shading(const QueryParams &p, float x, float y, float z, Vec3 &grad, Vec3 &colour) {
  grad.x = grad.y = grad.z = 0.0f;
  colour.x = colour.y = colour.z = 0.0f;
  Vec3 pv;
  if (!query_voxel_point(p, x, y, z, pv)) return;
  if (p.what & DSLAM_QUERY_GRADIENT) grad = q_normal(p.maps, p.mask, pv);
  if (p.what & DSLAM_QUERY_COLOUR) colour = q_colour(p.maps, p.mask, pv);
}

// one element's 48 bytes
__device__ __forceinline__ void store48(float4 *out, int i, const float4 &a, const float4 &b, const float4 &c) {
  float4 *o = out + 3 * (size_t)i;
  o[0] = a; o[1] = b; o[2] = c;
}

__global__ __launch_bounds__(64) void k_query_points(QueryParams p, const float *__restrict__ pts, float4 *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.n) return;
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  Vec3 pv;
  if (!query_voxel_point(p, x, y, z, pv)) {
    store48(out, i, make_float4(1.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f),
            make_float4(0.0f, 0.0f, __int_as_float(DSLAM_QUERY_OUTSIDE), 0.0f));
    return;
  }
  float den;
  unsigned long long found;
  const float sdf = q_trilinear(p.maps, p.mask, pv, den, found);
  Vec3 g, c;
  query_shading(p, x, y, z, g, c);
  store48(out, i, make_float4(sdf, den, g.x, g.y), make_float4(g.z, c.x, c.y, c.z),
          make_float4(__uint_as_float((unsigned)found), __uint_as_float((unsigned)(found >> 32)), 0.0f, 0.0f));
}

// cast_ray_multi (multimap.hip) for a ray given as origin, direction, t_min, t_max: the same loop body and refine_hit,
// the ray's set-up from the caller's numbers instead of a pixel's range cell, the iterations counted.  The iteration cap
// in the loop's condition cannot bind while `total` advances (the range is at most DSLAM_QUERY_MAX_RAY_VOXELS voxels and a
// step at least one); it ends the march where a t_min so large that total + step == total in float32 would not.
__global__ __launch_bounds__(64) void k_cast_rays(QueryParams p, const float4 *__restrict__ rays, float4 *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.n) return;
  const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
  const float ox = r0.x, oy = r0.y, oz = r0.z, t_min = r1.z, t_max = r1.w;
  Vec3 dir = {r0.w, r1.x, r1.y};
  const float len2 = dir.x * dir.x + dir.y * dir.y + dir.z * dir.z;
  const float dn = 1.0f / sqrtf(len2);
  dir.x *= dn; dir.y *= dn; dir.z *= dn;
  Vec3 res;
  res.x = (ox + t_min * dir.x) * p.one_over_vs;
  res.y = (oy + t_min * dir.y) * p.one_over_vs;
  res.z = (oz + t_min * dir.z) * p.one_over_vs;
  // (every comparison is false for a NaN; an infinite component makes len2, a start coordinate or t_max itself infinite)
  const bool valid = len2 > 0.0f && len2 < INFINITY && dn < INFINITY && t_min >= 0.0f && fabsf(t_max) < INFINITY &&
                     fabsf(res.x) <= kQueryMaxCoord && fabsf(res.y) <= kQueryMaxCoord && fabsf(res.z) <= kQueryMaxCoord;
  if (!valid) {
    store48(out, i, make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f),
            make_float4(0.0f, 0.0f, __int_as_float(-1), 0.0f));
    return;
  }
  float sdf = 1.0f;
  const float step_scale = p.mu * p.one_over_vs;
  float total = t_min * p.one_over_vs, step;
  const float total_max = fminf(t_max, t_min + p.max_range) * p.one_over_vs;
  int steps = 0;
  // per-lane block cache: one entry, tagged with its map
  IndexCache cache = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
  int cache_map = -1;
  while (total < total_max && steps < DSLAM_QUERY_MAX_RAY_VOXELS) {
    steps++;
    // nearest-voxel read of every map
    const Blend b = q_nearest(p.maps, p.mask, res, p.inv_32767, cache, cache_map);
    if (b.n == 0) {
      sdf = 1.0f;  // empty voxel: 32767 / 32767
      step = (float)kBlock;
    } else {
      sdf = b.value(1.0f);
      if ((sdf <= 0.1f) && (sdf >= -0.5f)) sdf = q_trilinear(p.maps, p.mask, res);
      if (sdf <= 0.0f) break;
      step = fmaxf(sdf * step_scale, 1.0f);
    }
    res.x += step * dir.x; res.y += step * dir.y; res.z += step * dir.z;
    total += step;
  }
  Vec4 hit;
  const bool found = refine_hit(hit, res, dir, sdf, step_scale, [&](const Vec3 &pt) { return q_trilinear(p.maps, p.mask, pt); });
  if (!found) {
    store48(out, i, make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f),
            make_float4(0.0f, 0.0f, __int_as_float(0), __int_as_float(steps)));
    return;
  }
  const float px = hit.x * p.voxel_size, py = hit.y * p.voxel_size, pz = hit.z * p.voxel_size;
  const float t = ((px - ox) * dir.x + (py - oy) * dir.y) + (pz - oz) * dir.z;
  Vec3 g, c;
  query_shading(p, px, py, pz, g, c);
  // the gradient normalised as store_pixel does; a length of exactly 0 (behind a surface without weight) gives 0
  const float gl = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
  if (gl == 0.0f) {
    g.x = g.y = g.z = 0.0f;
  } else {
    const float ns = 1.0f / gl;
    g.x *= ns; g.y *= ns; g.z *= ns;
  }
  store48(out, i, make_float4(t, px, py, pz), make_float4(g.x, g.y, g.z, c.x),
          make_float4(c.y, c.z, __int_as_float(steps == 1 ? 2 : 1), __int_as_float(steps)));
}

static_assert(sizeof(dslam_point_sample) == 48 && sizeof(dslam_ray_hit) == 48, "the kernels store 3 x 16 bytes per element");

// The call's kernels, everything already checked by the entry points (capi.hip).  rays: dslam_cast_rays, else
// dslam_query_points.  host: `in` and `out` are host arrays, staged through dslam_engine::query in chunks of
// kQueryChunk elements (the buffers grow on demand, to a chunk at the most); else device arrays, used in place.  Enqueues
// only: the caller waits (or not, dslam_engine_set_async).
constexpr int kQueryChunk = 1 << 20;

int launch_query(dslam_engine *e, const dslam_scene *const *scenes, const float *T, int num_maps, bool rays, const void *in, int n,
                 float max_range, int what, void *out, bool host) {
  const dslam_scene *s0 = scenes[0];
  DSLAM_TRY(upload_posed_maps(e, scenes, T, num_maps, (double)s0->p.voxel_size));
  QueryParams qp;
  qp.maps = static_cast<const MultiMap *>(e->map_table.get());
  qp.mask = num_maps >= 64 ? ~0ull : ((1ull << num_maps) - 1ull);
  qp.what = what;
  qp.voxel_size = s0->p.voxel_size; qp.one_over_vs = 1.0f / s0->p.voxel_size; qp.mu = s0->p.mu;
  qp.inv_32767 = 1.0f / 32767.0f;
  qp.max_range = max_range;
  const size_t in_stride = rays ? 32 : 12, out_stride = 48;
  if (host) {
    QueryScratch &q = e->query;
    const size_t chunk = (size_t)std::min(n, kQueryChunk);
    if (q.in_bytes < chunk * in_stride) {
      DSLAM_TRY(q.in.alloc(chunk * in_stride));
      q.in_bytes = chunk * in_stride;
    }
    if (q.out_bytes < chunk * out_stride) {
      DSLAM_TRY(q.out.alloc(chunk * out_stride));
      q.out_bytes = chunk * out_stride;
    }
  }
  for (int off = 0; off < n; off += kQueryChunk) {
    const int m = std::min(n - off, host ? kQueryChunk : n);
    const void *src = static_cast<const char *>(in) + (size_t)off * in_stride;
    void *dst = static_cast<char *>(out) + (size_t)off * out_stride;
    const void *in_dev = src;
    void *out_dev = dst;
    if (host) {
      in_dev = e->query.in.get();
      out_dev = e->query.out.get();
      DSLAM_HIP(hipMemcpyAsync(e->query.in.get(), src, (size_t)m * in_stride, hipMemcpyHostToDevice, e->stream));
    }
    qp.n = m;
    if (rays)
      hipLaunchKernelGGL(k_cast_rays, dim3((m + 63) / 64), dim3(64), 0, e->stream, qp, static_cast<const float4 *>(in_dev),
                         static_cast<float4 *>(out_dev));
    else
      hipLaunchKernelGGL(k_query_points, dim3((m + 63) / 64), dim3(64), 0, e->stream, qp, static_cast<const float *>(in_dev),
                         static_cast<float4 *>(out_dev));
    DSLAM_HIP(hipGetLastError());
    if (host) DSLAM_HIP(hipMemcpyAsync(dst, out_dev, (size_t)m * out_stride, hipMemcpyDeviceToHost, e->stream));
    if (!host) break;
  }
  return DSLAM_OK;
}

}  // namespace dslam
