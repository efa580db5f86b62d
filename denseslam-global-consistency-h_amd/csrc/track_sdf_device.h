// track_sdf_device.h -- the statements of one workgroup's share of an evaluation of the depth-to-SDF tracking law (DESIGN.md
// section 18; stated in full in include/dslam_fusion.h and at the head of track_sdf.hip): back-projection, the loop over
// maps, blend, gate, the 33 per-lane accumulations and the workgroup reduction.  Included INSIDE the body of k_track_sdf
// (track_sdf.hip, one pose per launch) and of k_track_sdf_starts (track_sdf_starts.hip, many poses per launch): no include
// guard, not a header of declarations -- text and not a function for the reason register_body.h gives (as __forceinline__
// functions over a struct of the lane's sums k_track_sdf came out with other code, and a refactor here leaves the device
// code of its units identical, profiles/device_code_diff.sh).
// The including kernel provides: TILES (bool): lane t of a wave takes pixel (t & 7, t >> 3) of an 8 x 8 tile (tiles in
// row-major order, those on the right and bottom edges partly outside the image), otherwise consecutive lanes take
// consecutive pixels of a row; `p` with depth, lw, lh, fx, fy, cx, cy, inv_vs, maps, num_maps, residual_gate and partials;
// DSLAM_TRACK_SDF_POSE(k): entry k of P~; DSLAM_TRACK_SDF_FIRST and DSLAM_TRACK_SDF_STRIDE, int expressions: the lane takes
// the jobs FIRST, FIRST + STRIDE, ...; DSLAM_TRACK_SDF_ROW: the row of p.partials the workgroup writes.
  double sH[21], sN[6], sF = 0.0, sQx = 0.0, sQy = 0.0, sQz = 0.0;
  int valid = 0, cand = 0;
#pragma unroll
  for (int i = 0; i < 21; i++) sH[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) sN[i] = 0.0;
  const int tw = (p.lw + 7) >> 3, th = (p.lh + 7) >> 3;
  const int jobs = TILES ? tw * th * 64 : p.lw * p.lh;
  for (int job = DSLAM_TRACK_SDF_FIRST; job < jobs; job += DSLAM_TRACK_SDF_STRIDE) {
    int x, y;
    if (TILES) {
      const int tile = job >> 6, ty = tile / tw;
      x = (tile - ty * tw) * 8 + (job & 7);
      y = ty * 8 + ((job >> 3) & 7);
      if (x >= p.lw || y >= p.lh) continue;
    } else {
      y = job / p.lw;
      x = job - y * p.lw;
    }
    const float D = p.depth[x + (size_t)y * p.lw];
    if (!(D > 1e-8f)) continue;
    cand++;
    Vec3 c;
    c.x = (D * (((float)x - p.cx) / p.fx)) * p.inv_vs;
    c.y = (D * (((float)y - p.cy) / p.fy)) * p.inv_vs;
    c.z = D * p.inv_vs;
    // R c, the point relative to the camera centre t: what the rotation part of the row and sums 29..31 are formed from, so
    // that neither has an operand of the size of the camera's position; p = R c + t is what the maps are read at
    Vec3 rc, pw;
    rc.x = (DSLAM_TRACK_SDF_POSE(0) * c.x + DSLAM_TRACK_SDF_POSE(1) * c.y) + DSLAM_TRACK_SDF_POSE(2) * c.z;
    rc.y = (DSLAM_TRACK_SDF_POSE(4) * c.x + DSLAM_TRACK_SDF_POSE(5) * c.y) + DSLAM_TRACK_SDF_POSE(6) * c.z;
    rc.z = (DSLAM_TRACK_SDF_POSE(8) * c.x + DSLAM_TRACK_SDF_POSE(9) * c.y) + DSLAM_TRACK_SDF_POSE(10) * c.z;
    pw.x = rc.x + DSLAM_TRACK_SDF_POSE(3);
    pw.y = rc.y + DSLAM_TRACK_SDF_POSE(7);
    pw.z = rc.z + DSLAM_TRACK_SDF_POSE(11);
    Blend bd = {0, 0.0f, 0.0f, 0.0f};
    Blend3 bg = {0, 0.0f, 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    for (int i = 0; i < p.num_maps; i++) {   // (i is the same in every lane: the descriptor is read by scalar loads)
      const MultiMap &m = p.maps[i];
      const Vec3 q = to_map(m, pw);
      // a block coordinate outside the short range is never resident (and this keeps the casts below defined)
      if (!(fabsf(q.x) < 262144.0f && fabsf(q.y) < 262144.0f && fabsf(q.z) < 262144.0f)) continue;
      const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
      const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
      const VolumeRef vol = volume_of(m);
      // tap 0 lies in the block of the cell's base corner: without that block the map cannot pass the gate below
      IndexCache none = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
      if (lookup_block(vol, ix >> 3, iy >> 3, iz >> 3, none) < 0) continue;
      uint2 t[8];
      if (!gather_cell(vol, ix, iy, iz, t)) continue;
      bool ok = true;
      float s[8], w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int raw = (int)(short)(t[k].x & 0xffffu);
        const unsigned wd = (t[k].x >> 16) & 0xffu;
        ok = ok && wd != 0u && raw != 32767 && raw != -32767;
        s[k] = sdf_to_float((short)raw);
        w[k] = (float)wd;
      }
      if (!ok) continue;
      const float cx = q.x - fx, cy = q.y - fy, cz = q.z - fz;
      const float ux = 1.0f - cx, uy = 1.0f - cy, uz = 1.0f - cz;
      const float x00 = ux * s[0] + cx * s[1], x10 = ux * s[2] + cx * s[3];
      const float x01 = ux * s[4] + cx * s[5], x11 = ux * s[6] + cx * s[7];
      const float y0 = uy * x00 + cy * x10, y1 = uy * x01 + cy * x11;
      const float d = uz * y0 + cz * y1;
      Vec3 g;
      g.x = uz * (uy * (s[1] - s[0]) + cy * (s[3] - s[2])) + cz * (uy * (s[5] - s[4]) + cy * (s[7] - s[6]));
      g.y = uz * (x10 - x00) + cz * (x11 - x01);
      g.z = y1 - y0;
      const float w00 = ux * w[0] + cx * w[1], w10 = ux * w[2] + cx * w[3];
      const float w01 = ux * w[4] + cx * w[5], w11 = ux * w[6] + cx * w[7];
      const float om = uz * (uy * w00 + cy * w10) + cz * (uy * w01 + cy * w11);
      if (!m.identity) {   // the gradient in the world frame: R^T g
        const Vec3 gm = g;
        g.x = (m.T[0] * gm.x + m.T[4] * gm.y) + m.T[8] * gm.z;
        g.y = (m.T[1] * gm.x + m.T[5] * gm.y) + m.T[9] * gm.z;
        g.z = (m.T[2] * gm.x + m.T[6] * gm.y) + m.T[10] * gm.z;
      }
      bd.add(d, om);
      bg.add(g, om);
    }
    if (bd.n == 0) continue;
    const float d = bd.value(0.0f);
    const Vec3 g = bg.value();
    if (fabsf(d) > p.residual_gate) continue;
    const float r = -d;
    float A[6];
    A[0] = rc.y * g.z - rc.z * g.y;
    A[1] = rc.z * g.x - rc.x * g.z;
    A[2] = rc.x * g.y - rc.y * g.x;
    A[3] = g.x; A[4] = g.y; A[5] = g.z;
    valid++;
    sF += (double)(r * r);
    sQx += (double)rc.x; sQy += (double)rc.y; sQz += (double)rc.z;
#pragma unroll
    for (int k = 0, c2 = 0; k < 6; k++) {
      sN[k] += (double)(r * A[k]);
#pragma unroll
      for (int j = 0; j <= k; j++, c2++) sH[c2] += (double)(A[k] * A[j]);
    }
  }
  // workgroup reduction in a fixed order: wave shuffle tree, then the four wave partials through LDS.  A workgroup
  // without a pixel arrives here with zeros and writes them.
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
    p.partials[(size_t)DSLAM_TRACK_SDF_ROW * kRegSums + i] = v;
  }
