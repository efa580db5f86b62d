"""Float64 reference of the composite raycast over several local maps (dslam_get_image_multi), built on ref64.py.

Each map is an analytic map (analytic_maps.py) built in its own frame, plus T, its 4x4 world -> map transform
(metres).  The law: every read of the march at a world point p (voxel units) goes to every map
whose blocks project into p's 8x8 tile, in list order, at q_i = T~_i p (T~: translation in voxel units).  Maps that
report found are combined: none -> not found (the coarse step takes the 8-voxel block step; a trilinear read returns
the first candidate's read), one -> its value, several -> sum(w v) / sum(w) (sum(w) = 0: 1.0, or the first
contributor's normal / colour).  w: the voxel's w_depth (nearest read), the trilinear w_depth (trilinear read, normal),
the trilinear w_color (colour) -- each voxel's own stored weights (a missing voxel weighs 0), so a fused map, whose
weights run from 0 to max_w from one voxel to the next, is read as it is.  Predicates are evaluated in float64 with the
tie flags of ref64.cast_rays, plus the cell boundaries where a map's "any tap found" of a trilinear read flips.
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
        # overrides, for the alternative laws the tests hold the kernel away from: a number makes every stored voxel of
        # the map weigh that much; weight_read = "nearest" gives a trilinear read the weight of its nearest tap;
        # colour_weight = "w_depth" gives the colour the confidence of the sdf
        self.w_depth = self.w_color = None
        self.weight_read = "trilinear"
        self.colour_weight = "w_color"

    def to_map(self, p):
        return p if self.identity else p @ self.R.T + self.t_vox

    def weights(self, p, found):
        """(w_depth, w_color) as float64 of integer voxel coordinates p, whose `found` the caller has from m.lookup."""
        wd, wc = self.m.lookup_weights(p)
        wd = wd.astype(np.float64) if self.w_depth is None else found * float(self.w_depth)
        wc = wc.astype(np.float64) if self.w_color is None else found * float(self.w_color)
        return wd, wc


def set_weights(m, w_depth, w_color=None):
    """Give every voxel of map `m` these weights (its uploaded pool `vba` and its lookup grid too)."""
    m.voxels["w_depth"] = w_depth
    if w_color is not None:
        m.voxels["w_color"] = w_color
    m.vba[m.ptrs] = m.voxels
    m._build_grid()
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
                tap = q0 + np.array([dx, dy, dz])
                s, clr, f = pm.m.lookup(tap)
                w = (c[:, 0] if dx else 1 - c[:, 0]) * (c[:, 1] if dy else 1 - c[:, 1]) * (c[:, 2] if dz else 1 - c[:, 2])
                acc += (w[:, None] * clr) if colour else w * s
                wt = pm.weights(tap, f)[1 if colour and pm.colour_weight == "w_color" else 0]
                if pm.weight_read == "nearest":
                    wsum += np.where(np.all((c >= 0.5) == np.array([dx, dy, dz], bool), axis=1), wt, 0.0)
                else:
                    wsum += w * wt
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


def _floor_flip(pm, q, tol):
    """_floor_tie, kept only where the boundary decides something.  A trilinear read and its trilinear weight are
    continuous across a cell boundary (the taps that enter or leave have the coefficient 0 there), so the law's result can
    jump only where one of its predicates flips: the map's `any tap found`, or its weight's `> 0` (with integer weights the
    sum over the maps is 0 only where every tap with a positive coefficient weighs 0, so `den > 0` can flip nowhere else)."""
    close = np.abs(q - np.round(q)) < tol
    tie = close.sum(axis=1) > 1          # near a boundary on two axes at once: flagged as the plain flag does
    for a in range(3):
        r = np.round(q[:, a])
        near = np.nonzero(close[:, a] & ~tie)[0]
        if len(near):
            lo, hi = q[near].copy(), q[near].copy()
            lo[:, a], hi[:, a] = r[near] - 0.25, r[near] + 0.25
            (_, w0, f0), (_, w1, f1) = _trilinear(pm, lo), _trilinear(pm, hi)
            tie[near] |= (f0 != f1) | ((w0 > 0) != (w1 > 0))
    return tie


def _round_flip(pm, q, tol):
    """A coordinate of q within tol of a half, kept only where the two voxels iround chooses between differ in what the
    nearest read takes from them (found, sdf, w_depth): between two missing voxels nothing is decided."""
    frac = np.abs(q) - np.floor(np.abs(q))
    close = np.abs(frac - 0.5) < tol
    tie = close.sum(axis=1) > 1          # near a half on two axes at once: flagged as the plain flag does
    for a in range(3):
        near = np.nonzero(close[:, a] & ~tie)[0]
        if len(near):
            lo, hi = q[near].copy(), q[near].copy()
            lo[:, a] -= 0.25
            hi[:, a] += 0.25
            v0, v1 = ref64._iround(lo), ref64._iround(hi)
            (s0, _, f0), (s1, _, f1) = pm.m.lookup(v0), pm.m.lookup(v1)
            tie[near] |= (f0 != f1) | (f0 & ((s0 != s1) | (pm.weights(v0, f0)[0] != pm.weights(v1, f1)[0])))
    return tie


def multi_trilinear(maps, cand, p, tie, tie_tol, sharp_ties=False):
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
                tie[sel] |= (cand[sel].sum(1) > 1) & (_floor_flip(pm, q, tie_tol) if sharp_ties else _floor_tie(q, tie_tol))
        first_any = np.where(np.isnan(first_any) & sel, v, first_any)
        vals.append(v), ws.append(w), fs.append(f & sel)
    out, _ = _combine(vals, ws, fs, np.where(np.isnan(first_any), 1.0, first_any), fallback=1.0)
    return out


def cast_rays(maps, M, intr, W, H, tie_tol=1e-4, max_steps=4000, sharp_ties=False):
    """ref64.cast_rays over the composite.  Returns the same dict plus `cand` [H, W, maps] (the pixel's cell mask).
    sharp_ties: flag a voxel or cell boundary only where it decides something (_round_flip, _floor_flip) -- fewer ties, so
    more pixels held to the bound."""
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
                if sharp_ties:
                    tie[idx[sel]] |= _round_flip(pm, q, tie_tol)
                else:
                    frac = np.abs(q) - np.floor(np.abs(q))
                    tie[idx[sel]] |= np.any(np.abs(frac - 0.5) < tie_tol, axis=1)
                near = ref64._iround(q)
                s16, _, f[sel] = pm.m.lookup(near)
                v[sel] = s16 / 32767.0
                w[sel] = pm.weights(near, f[sel])[0]
            vals.append(v), ws.append(w), fs.append(f)
        s, nf = _combine(vals, ws, fs, np.ones(len(idx)), fallback=1.0)
        found = nf > 0
        step = np.full(len(idx), 8.0)
        win = found & (s <= 0.1) & (s >= -0.5)
        tie[idx] |= found & ((np.abs(s - 0.1) < tie_tol) | (np.abs(s + 0.5) < tie_tol))
        if win.any():
            t_sub = np.zeros(win.sum(), bool)
            s[win] = multi_trilinear(maps, cand[win], p[idx[win]], t_sub, tie_tol, sharp_ties)
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
    s = multi_trilinear(maps, cand_all[h], p[h], t_sub, tie_tol, sharp_ties)
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


def normals(maps, cand, p, magnitude=False):
    """Combined unit normal (world frame) at world points p [n, 3] (voxel units); cand [n, maps].  magnitude=True: also the
    length of the combined gradient before it is normalised (sdf units per 2 voxels): where it is next to nothing -- inside
    the region whose sdf is clamped to -1 or 1 -- the direction is rounding noise."""
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
        n = g / np.linalg.norm(g, axis=1, keepdims=True)
    return (n, np.linalg.norm(g, axis=1)) if magnitude else n


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
