// register_body.h -- the statements of one workgroup's evaluation of the registration law (stated in
// full at the head of register.hip), included INSIDE the body of k_register (register.hip) and of k_register_graph
// (register_graph.hip): no include guard, not a header of declarations.  It is text and not a function because the
// compiler does not give the inlined function the code it gives the statements in place: as a __forceinline__ function
// (by reference, by value, as a template -- all were built) k_register came out with 205 instead of 163 VGPRs and 2
// instead of 3 waves per SIMD, and this project asks that a refactor leaves the device code of its units identical
// (profiles/device_code_diff.sh).
// The including kernel provides: `p`, a RegisterParams (register_device.h); DSLAM_REG_FIRST and DSLAM_REG_STRIDE, unsigned
// expressions: the workgroup takes the live blocks DSLAM_REG_FIRST, + DSLAM_REG_STRIDE, ... of the source.  It writes row
// blockIdx.x of p.partials.
  double sH[21], sN[6], sF = 0.0, sQx = 0.0, sQy = 0.0, sQz = 0.0;
  int valid = 0, cand = 0;
#pragma unroll
  for (int i = 0; i < 21; i++) sH[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) sN[i] = 0.0;
  const int live = *p.live_count;
  const int x = threadIdx.x & 7, y = (threadIdx.x >> 3) & 7;
  const VolumeRef vol = volume_of(p.dst);
  for (int job = DSLAM_REG_FIRST * 2; job < live * 2; job += (job & 1) ? DSLAM_REG_STRIDE * 2 - 1 : 1) {
    const int b = job >> 1, z = (int)(threadIdx.x >> 6) + 4 * (job & 1);
    const HashEntry he = load_entry(p.hash, p.live_list[b]);
    if (he.ptr < 0) continue;  // (uniform; a live entry holds a block)
    const unsigned own = p.voxels[(size_t)he.ptr * kBlock3 + threadIdx.x + kRegThreads * (job & 1)].x;
    const int raw_s = (int)(short)(own & 0xffffu);
    if (((own >> 16) & 0xffu) == 0u || abs(raw_s) >= p.band_raw) continue;
    cand++;
    const Vec3 pt = {(float)(he.pos[0] * kBlock + x), (float)(he.pos[1] * kBlock + y), (float)(he.pos[2] * kBlock + z)};
    const Vec3 q = to_map(p.dst, pt);
    // a block coordinate outside the short range is never resident (and this keeps the casts below defined)
    if (!(fabsf(q.x) < 262144.0f && fabsf(q.y) < 262144.0f && fabsf(q.z) < 262144.0f)) continue;
    const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
    uint2 t[8];
    if (!gather_cell(vol, (int)fx, (int)fy, (int)fz, t)) continue;
    bool ok = true;
    float s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int raw = (int)(short)(t[k].x & 0xffffu);
      ok = ok && ((t[k].x >> 16) & 0xffu) != 0u && raw != 32767 && raw != -32767;
      s[k] = sdf_to_float((short)raw);
    }
    if (!ok) continue;
    const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
    const float ux = 1.0f - cx, uy = 1.0f - cy, uz = 1.0f - cz;
    const float x00 = ux * s[0] + cx * s[1], x10 = ux * s[2] + cx * s[3];
    const float x01 = ux * s[4] + cx * s[5], x11 = ux * s[6] + cx * s[7];
    const float y0 = uy * x00 + cy * x10, y1 = uy * x01 + cy * x11;
    const float d = uz * y0 + cz * y1;
    const float gx = uz * (uy * (s[1] - s[0]) + cy * (s[3] - s[2])) + cz * (uy * (s[5] - s[4]) + cy * (s[7] - s[6]));
    const float gy = uz * (x10 - x00) + cz * (x11 - x01);
    const float gz = y1 - y0;
    const float r = sdf_to_float((short)raw_s) - d;
    if (fabsf(r) > p.residual_gate) continue;
    float A[6];
    A[0] = q.y * gz - q.z * gy;
    A[1] = q.z * gx - q.x * gz;
    A[2] = q.x * gy - q.y * gx;
    A[3] = gx; A[4] = gy; A[5] = gz;
    valid++;
    sF += (double)(r * r);
    sQx += (double)q.x; sQy += (double)q.y; sQz += (double)q.z;
#pragma unroll
    for (int k = 0, c = 0; k < 6; k++) {
      sN[k] += (double)(r * A[k]);
#pragma unroll
      for (int j = 0; j <= k; j++, c++) sH[c] += (double)(A[k] * A[j]);
    }
  }
  // workgroup reduction in a fixed order: wave shuffle tree, then the four wave partials through LDS.  A workgroup
  // without a block arrives here with zeros and writes them.
  __shared__ double red[kRegWaves][kRegSums];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double vals[kRegSums];
#pragma unroll
  for (int i = 0; i < 21; i++) vals[i] = sH[i];
#pragma unroll
  for (int i = 0; i < 6; i++) vals[21 + i] = sN[i];
  vals[27] = sF;
  vals[28] = (double)valid;
  vals[29] = sQx; vals[30] = sQy; vals[31] = sQz;
  vals[32] = (double)cand;
#pragma unroll
  for (int i = 0; i < kRegSums; i++) {
    double v = vals[i];
    for (int dlt = 32; dlt > 0; dlt >>= 1) v += __shfl_down(v, dlt, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kRegSums) {
    const int i = threadIdx.x;
    double v = red[0][i];
#pragma unroll
    for (int w = 1; w < kRegWaves; w++) v += red[w][i];
    p.partials[(size_t)blockIdx.x * kRegSums + i] = v;
  }
