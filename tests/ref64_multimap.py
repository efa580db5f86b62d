"""Float64 reference of the composite raycast over several local maps (dslam_get_image_multi), built on ref64.py.

Each map is an analytic map (analytic_maps.py) built in its own frame, plus T, its 4x4 world -> map transform
(metres).  The law: every read of the march at a world point p (voxel units) goes to every map
whose blocks project into p's 8x8 tile, in list order, at q_i = T~_i p (T~: translation in voxel units).  Maps that
report found are combined: none -> not found (the coarse step takes the 8-voxel block step; a trilinear read returns
the first candidate's read), one -> its value, several -> sum(w v) / sum(w) (sum(w) = 0: 1.0, or the first
contributor's normal / colour).  w: the voxel's w_depth (nearest read), the trilinear w_depth (trilinear read, normal),
the trilinear w_color (colour).  Predicates are evaluated in float64 with the tie flags of ref64.cast_rays, plus the
cell boundaries where a map's "any tap found" of a trilinear read flips.
"""
import numpy as np

import ref64

F = np.float32


class Posed:
    """Map `m` (analytic_maps.Map, built in the map's frame) seen through T (world -> map, metres)."""

    def __init__(self, m, T):
        self.m = m
        self.T = np.asarray(T, np.float64)
        self.identity = bool(np.array_equal(np.asarray(T, F), np.eye(4, dtype=F)))
        self.R = self.T[:3, :3]
        self.t_vox = self.T[:3, 3] / float(F(m.vs))
        found = m.voxels["w_depth"]
        self.w_depth = float(found.flat[0]) if found.size else 0.0
        self.w_color = float(m.voxels["w_color"].flat[0]) if found.size else 0.0
        assert (m.voxels["w_depth"] == self.w_depth).all() and (m.voxels["w_color"] == self.w_color).all()

    def to_map(self, p):
        return p if self.identity else p @ self.R.T + self.t_vox


def set_weights(m, w_depth, w_color=None):
    """Give every voxel of map `m` these weights (its uploaded pool `vba` too)."""
    m.voxels["w_depth"] = w_depth
    if w_color is not None:
        m.voxels["w_color"] = w_color
    m.vba[m.ptrs] = m.voxels
    return m


def camera_of(M, T):
    """The camera that sees map T from world camera M: M T^-1, float32 (the identity keeps M)."""
    if np.array_equal(np.asarray(T, F), np.eye(4, dtype=F)):
        return np.asarray(M, F)
    return (np.asarray(M, np.float64) @ np.linalg.inv(np.asarray(T, F).astype(np.float64))).astype(F)


def front_end(maps, M, intr, W, H):
    """Union range image [ceil(H/8), ceil(W/8), 2] and the per-cell map mask [.., .., n] (bool)."""
    tw, th = -(-W // 8), -(-H // 8)
    rng = np.empty((th, tw, 2))
    rng[..., 0], rng[..., 1] = ref64.FAR_AWAY, ref64.VERY_CLOSE
    mask = np.zeros((th, tw, len(maps)), bool)
    for i, pm in enumerate(maps):
        r = ref64.expected_depths(pm.m, camera_of(M, pm.T), intr, W, H)
        mask[..., i] = (r[..., 0] != ref64.FAR_AWAY) | (r[..., 1] != ref64.VERY_CLOSE)
        rng[..., 0] = np.minimum(rng[..., 0], r[..., 0])
        rng[..., 1] = np.maximum(rng[..., 1], r[..., 1])
    return rng, mask


def _trilinear(pm, q, colour=False):
    """(sdf value, trilinear w_depth, any tap found) -- or with colour=True (colour [n, 3], trilinear w_color, found)."""
    q0 = np.floor(q)
    c = q - q0
    q0 = q0.astype(np.int64)
    acc = np.zeros((len(q), 3)) if colour else np.zeros(len(q))
    wsum = np.zeros(len(q))
    anyf = np.zeros(len(q), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                s, clr, f = pm.m.lookup(q0 + np.array([dx, dy, dz]))
                w = (c[:, 0] if dx else 1 - c[:, 0]) * (c[:, 1] if dy else 1 - c[:, 1]) * (c[:, 2] if dz else 1 - c[:, 2])
                acc += (w[:, None] * clr) if colour else w * s
                wsum += w * f * (pm.w_color if colour else pm.w_depth)
                anyf |= f
    return (acc if colour else acc / 32767.0), wsum, anyf


def _combine(vals, ws, fs, first_any, fallback=None):
    """The law over candidate reads (lists in map order; vals [n] or [n, 3]; a candidate's f False where it is not one)."""
    n = len(first_any)
    nf = np.zeros(n, np.int64)
    num = np.zeros_like(first_any)
    den = np.zeros(n)
    first = first_any.copy()
    for v, w, f in zip(vals, ws, fs):
        take = f & (nf == 0)
        first[take] = v[take]
        ww = np.where(f, w, 0.0)
        num = num + (ww[:, None] * v if v.ndim == 2 else ww * v) * (f[:, None] if v.ndim == 2 else f)
        den += ww
        nf += f
    with np.errstate(invalid="ignore", divide="ignore"):
        blend = num / (den[:, None] if num.ndim == 2 else den)
    fb = first if fallback is None else np.full_like(first, fallback)
    many = np.where((den > 0)[:, None] if num.ndim == 2 else den > 0, blend, fb)
    one = (nf == 1)[:, None] if num.ndim == 2 else nf == 1
    none = (nf == 0)[:, None] if num.ndim == 2 else nf == 0
    return np.where(none, first_any, np.where(one, first, many)), nf


def _floor_tie(q, tol):
    return np.any(np.abs(q - np.round(q)) < tol, axis=1)


def multi_trilinear(maps, cand, p, tie, tie_tol):
    """Combined trilinear sdf read at world points p [n, 3]; cand [n, maps] bool."""
    vals, ws, fs = [], [], []
    first_any = np.full(len(p), np.nan)
    for i, pm in enumerate(maps):
        sel = cand[:, i]
        v, w, f = np.ones(len(p)), np.zeros(len(p)), np.zeros(len(p), bool)
        if sel.any():
            q = pm.to_map(p[sel])
            v[sel], w[sel], f[sel] = _trilinear(pm, q)
            if cand.sum(1).max() > 1:
                tie[sel] |= (cand[sel].sum(1) > 1) & _floor_tie(q, tie_tol)
        first_any = np.where(np.isnan(first_any) & sel, v, first_any)
        vals.append(v), ws.append(w), fs.append(f & sel)
    out, _ = _combine(vals, ws, fs, np.where(np.isnan(first_any), 1.0, first_any), fallback=1.0)
    return out


def cast_rays(maps, M, intr, W, H, tie_tol=1e-4, max_steps=4000):
    """ref64.cast_rays over the composite.  Returns the same dict plus `cand` [H, W, maps] (the pixel's cell mask)."""
    vs, mu = float(F(maps[0].m.vs)), float(F(maps[0].m.mu))
    rng, cmask = front_end(maps, M, intr, W, H)
    fx, fy, cx, cy = (float(F(v)) for v in intr)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
    r = rng[(ys // 8).astype(int), (xs // 8).astype(int)]
    cand_all = cmask[(ys // 8).astype(int), (xs // 8).astype(int)]
    invM = np.linalg.inv(np.asarray(M, np.float64))

    def at(z):
        pc = np.stack([z * ((xs - cx) / fx), z * ((ys - cy) / fy), z], -1)
        return np.linalg.norm(pc, axis=1) / vs, ref64.mat_vec_f64(invM, pc) / vs

    total, ps = at(r[:, 0])
    total_max, pe = at(r[:, 1])
    d = pe - ps
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
    step_scale = mu / vs
    n = len(xs)
    p = ps.copy()
    sdf = np.ones(n)
    hit = np.zeros(n, bool)
    tie = np.zeros(n, bool)
    active = total < total_max
    tie |= np.abs(total - total_max) < tie_tol
    for _ in range(max_steps):
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        cand = cand_all[idx]
        vals, ws, fs = [], [], []
        for i, pm in enumerate(maps):
            sel = cand[:, i]
            v, w, f = np.ones(len(idx)), np.zeros(len(idx)), np.zeros(len(idx), bool)
            if sel.any():
                q = pm.to_map(p[idx[sel]])
                frac = np.abs(q) - np.floor(np.abs(q))
                tie[idx[sel]] |= np.any(np.abs(frac - 0.5) < tie_tol, axis=1)
                s16, _, f[sel] = pm.m.lookup(ref64._iround(q))
                v[sel] = s16 / 32767.0
                w[sel] = pm.w_depth
            vals.append(v), ws.append(w), fs.append(f)
        s, nf = _combine(vals, ws, fs, np.ones(len(idx)), fallback=1.0)
        found = nf > 0
        step = np.full(len(idx), 8.0)
        win = found & (s <= 0.1) & (s >= -0.5)
        tie[idx] |= found & ((np.abs(s - 0.1) < tie_tol) | (np.abs(s + 0.5) < tie_tol))
        if win.any():
            t_sub = np.zeros(win.sum(), bool)
            s[win] = multi_trilinear(maps, cand[win], p[idx[win]], t_sub, tie_tol)
            tie[idx[win]] |= t_sub
        stop = found & (s <= 0.0)
        tie[idx] |= found & (np.abs(s) < tie_tol)
        step[found] = np.maximum(s[found] * step_scale, 1.0)
        sdf[idx] = s
        hit[idx[stop]] = True
        go = idx[~stop]
        p[go] += step[~stop, None] * d[go]
        total[go] += step[~stop]
        active[idx[stop]] = False
        active[go] = total[go] < total_max[go]
        tie[go] |= np.abs(total[go] - total_max[go]) < tie_tol
    else:
        raise AssertionError("ray march did not terminate")
    h = np.nonzero(hit)[0]
    p_stop = p.copy()
    t_sub = np.zeros(len(h), bool)
    p[h] += (sdf[h] * step_scale)[:, None] * d[h]
    s = multi_trilinear(maps, cand_all[h], p[h], t_sub, tie_tol)
    p[h] += (s * step_scale)[:, None] * d[h]
    tie[h] |= t_sub
    return dict(p=p.reshape(H, W, 3), hit=hit.reshape(H, W), tie=tie.reshape(H, W), dir=d.reshape(H, W, 3),
                p_stop=p_stop.reshape(H, W, 3), sdf_stop=sdf.reshape(H, W), cand=cand_all.reshape(H, W, len(maps)))


def _gradient(pm, q):
    """computeSingleNormalFromSDF's un-normalised gradient (trilinear one voxel ahead minus one behind), map frame."""
    g = np.zeros((len(q), 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        g[:, k] = ref64.read_trilinear(pm.m, q + e)[0] - ref64.read_trilinear(pm.m, q - e)[0]
    return g


def normals(maps, cand, p):
    """Combined unit normal (world frame) at world points p [n, 3] (voxel units); cand [n, maps]."""
    vals, ws, fs = [], [], []
    first_any = np.full((len(p), 3), np.nan)
    for i, pm in enumerate(maps):
        sel = cand[:, i]
        v, w, f = np.zeros((len(p), 3)), np.zeros(len(p)), np.zeros(len(p), bool)
        if sel.any():
            q = pm.to_map(p[sel])
            g = _gradient(pm, q)
            v[sel] = g if pm.identity else g @ pm.R
            _, w[sel], f[sel] = _trilinear(pm, q)
        take = np.isnan(first_any[:, 0]) & sel
        first_any[take] = v[take]
        vals.append(v), ws.append(w), fs.append(f)
    g, _ = _combine(vals, ws, fs, np.nan_to_num(first_any))
    with np.errstate(invalid="ignore", divide="ignore"):
        return g / np.linalg.norm(g, axis=1, keepdims=True)


def colours(maps, cand, p):
    """Combined trilinear colour (0 .. 255 scale) at world points p [n, 3]."""
    vals, ws, fs = [], [], []
    first_any = np.full((len(p), 3), np.nan)
    for i, pm in enumerate(maps):
        sel = cand[:, i]
        v, w, f = np.zeros((len(p), 3)), np.zeros(len(p)), np.zeros(len(p), bool)
        if sel.any():
            v[sel], w[sel], f[sel] = _trilinear(pm, pm.to_map(p[sel]), colour=True)
        take = np.isnan(first_any[:, 0]) & sel
        first_any[take] = v[take]
        vals.append(v), ws.append(w), fs.append(f)
    c, _ = _combine(vals, ws, fs, np.nan_to_num(first_any))
    return c
