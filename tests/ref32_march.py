"""castRay restated in plain numpy float32, in the spec's operation order, for one purpose: to measure how
far float32 moves a ray's hit from the float64 march of ref64.cast_rays when the coordinates are large (DESIGN section
27).  No engine enters: the pose inverse (refmap.inv_f32, ORUtils' cofactor inverse), the ray's ends, its direction, the accumulated march
position, the two refinement steps and the depth image's mat-vec are float32 here; the voxel reads, whose weights come
from the position's exact fractional part, are ref64's on the float32 position.  numpy never fuses a multiply-add."""
import numpy as np

import ref64
import refmap

F = np.float32

def cast_rays(m, M, intr, W, H, max_steps=4000):
    """dict(p [H, W, 3] float32 hit position in voxel units, hit [H, W], depth [H, W] float32: IMAGE_DEPTH)."""
    vs, mu = F(m.vs), F(m.mu)
    one_over_vs = F(1) / vs
    rng = ref64.expected_depths(m, M, intr, W, H, z32=True).astype(F)
    fx, fy, cx, cy = (F(v) for v in intr)
    inv_fx, inv_fy = F(1) / fx, F(1) / fy
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F)
    r = rng[(ys // 8).astype(int), (xs // 8).astype(int)]
    invM = refmap.inv_f32(M)

    def at(z):
        pc = np.stack([z * ((xs - cx) * inv_fx), z * ((ys - cy) * inv_fy), z], -1)
        total = np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2]) * one_over_vs
        return total, ref64.mat_vec_f32(invM, pc) * one_over_vs

    total, ps = at(r[:, 0])
    total_max, pe = at(r[:, 1])
    d = pe - ps
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d * (F(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[:, None]
    step_scale = mu * one_over_vs
    n = len(xs)
    p = ps.copy()
    sdf = np.ones(n, F)
    hit = np.zeros(n, bool)
    active = total < total_max
    for _ in range(max_steps):
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        q = p[idx]
        s16, _, found = m.lookup(ref64._iround(q.astype(np.float64)))
        s = (s16.astype(F) / F(32767)).astype(F)
        step = np.full(len(idx), 8.0, F)
        win = found & (s <= F(0.1)) & (s >= F(-0.5))
        if win.any():
            s[win] = ref64.read_trilinear(m, q[win].astype(np.float64))[0].astype(F)
        stop = found & (s <= 0)
        step[found] = np.maximum(s[found] * step_scale, F(1))
        sdf[idx] = s
        hit[idx[stop]] = True
        go = idx[~stop]
        p[go] = p[go] + step[~stop, None] * d[go]
        total[go] = total[go] + step[~stop]
        active[idx[stop]] = False
        active[go] = total[go] < total_max[go]
    else:
        raise AssertionError("ray march did not terminate")
    h = np.nonzero(hit)[0]
    p[h] = p[h] + (sdf[h] * step_scale)[:, None] * d[h]
    s = ref64.read_trilinear(m, p[h].astype(np.float64))[0].astype(F)
    p[h] = p[h] + (s * step_scale)[:, None] * d[h]
    depth = np.zeros(n, F)
    depth[h] = ref64.mat_vec_f32(M, p[h] * vs)[:, 2]
    return dict(p=p.reshape(H, W, 3), hit=hit.reshape(H, W), depth=depth.reshape(H, W))
