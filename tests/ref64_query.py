"""Float64 reference of dslam_query_points and dslam_cast_rays, built on ref64_multimap.py: the law of
DESIGN.md section 10 read at arbitrary world points and marched along arbitrary rays, with every listed map a candidate
everywhere (the queries have no range image and no cell mask).

maps: ref64_multimap.Posed objects.  Points and rays are in metres, as the calls take them; inputs are taken as the float32
values the device receives, everything behind that is float64.  Predicates carry tie flags as ref64_multimap's do: a result
is compared only where no predicate of its computation lay within tie_tol of flipping.
"""
import numpy as np

import ref64
import ref64_multimap as rm

F = np.float32
SDF, GRADIENT, COLOUR = 1, 2, 4
OUTSIDE = 1
MAX_RAY_VOXELS = 16384
MAX_COORD = float(1 << 20)


def _vs_mu(maps):
    return float(F(maps[0].m.vs)), float(F(maps[0].m.mu))


def shade(maps, p, what):
    """(combined un-normalised gradient [n, 3], its length [n], combined colour 0 .. 1 [n, 3]) at world points p (voxel
    units) -- what both calls report; a field `what` leaves out is 0."""
    n = len(p)
    cand = np.ones((n, len(maps)), bool)
    grad, length, colour = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3))
    if n and what & GRADIENT:
        unit, length = rm.normals(maps, cand, p, magnitude=True)
        grad = np.nan_to_num(unit) * length[:, None]
    if n and what & COLOUR:
        colour = rm.colours(maps, cand, p) / 255.0
    return grad, length, colour


def sample_points(maps, p_world_m, what=SDF | GRADIENT | COLOUR, tie_tol=1e-4):
    """dslam_query_points.  Returns a dict: sdf, weight [n], grad, colour [n, 3], found [n, maps] (bool), status [n], and
    tie [n]: a map-frame coordinate of the point lies within tie_tol of a cell boundary that decides something
    (ref64_multimap._floor_flip) -- there `found`, and with it every field, may differ by a predicate."""
    vs, _ = _vs_mu(maps)
    pm_in = np.asarray(p_world_m, F).astype(np.float64).reshape(-1, 3)
    n = len(pm_in)
    with np.errstate(invalid="ignore", over="ignore"):
        p_all = pm_in / vs
        inside = np.all(np.isfinite(p_all) & (np.abs(p_all) <= MAX_COORD), axis=1)
    out = dict(sdf=np.ones(n), weight=np.zeros(n), grad=np.zeros((n, 3)), colour=np.zeros((n, 3)),
               found=np.zeros((n, len(maps)), bool), status=np.where(inside, 0, OUTSIDE), tie=np.zeros(n, bool),
               grad_length=np.zeros(n))
    idx = np.nonzero(inside)[0]
    if len(idx) == 0:
        return out
    p = p_all[idx]
    cand = np.ones((len(p), len(maps)), bool)
    tie = np.zeros(len(p), bool)
    weight = np.zeros(len(p))
    for i, pm in enumerate(maps):
        q = pm.to_map(p)
        _, w, f = rm._trilinear(pm, q)
        out["found"][idx, i] = f
        weight += np.where(f, w, 0.0)
        tie |= rm._floor_flip(pm, q, tie_tol)
    unused = np.zeros(len(p), bool)
    out["sdf"][idx] = rm.multi_trilinear(maps, cand, p, unused, tie_tol, sharp_ties=True)
    out["weight"][idx] = weight
    out["grad"][idx], out["grad_length"][idx], out["colour"][idx] = shade(maps, p, what)
    out["tie"][idx] = tie
    return out


def sample_points_scalar(maps, p_world_m):
    """sample_points' sdf, weight and found by a scalar loop over points, maps and the 8 stored voxels of a cell, written out
    without the vectorised helpers (the check of the reference against itself)."""
    vs, _ = _vs_mu(maps)
    pts = np.asarray(p_world_m, F).astype(np.float64).reshape(-1, 3) / vs
    sdf, weight, found = np.ones(len(pts)), np.zeros(len(pts)), np.zeros((len(pts), len(maps)), bool)
    for j, p in enumerate(pts):
        n_found, num, den, first, first_any = 0, 0.0, 0.0, None, None
        for i, pm in enumerate(maps):
            q = p if pm.identity else pm.R @ p + pm.t_vox
            q0 = np.floor(q)
            c = q - q0
            v = w = 0.0
            any_found = False
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        tap = q0.astype(np.int64) + np.array([dx, dy, dz])
                        s, _, f = pm.m.lookup(tap)
                        wd, _ = pm.m.lookup_weights(tap)
                        k = (c[0] if dx else 1 - c[0]) * (c[1] if dy else 1 - c[1]) * (c[2] if dz else 1 - c[2])
                        v += k * float(s)
                        w += k * float(wd)
                        any_found |= bool(f)
            v /= 32767.0
            if first_any is None:
                first_any = v
            if any_found:
                found[j, i] = True
                if n_found == 0:
                    first = v
                num, den, n_found = num + w * v, den + w, n_found + 1
        sdf[j] = first_any if n_found == 0 else first if n_found == 1 else (num / den if den > 0 else 1.0)
        weight[j] = den
    return sdf, weight, found


def cast_rays(maps, o, d, t_min, t_max, max_range=0.0, sharp_ties=True, tie_tol=1e-4, what=SDF | GRADIENT | COLOUR):
    """dslam_cast_rays: ref64_multimap.cast_rays' march for rays given as origin o [n, 3], direction d [n, 3] (any length),
    t_min, t_max [n] or scalars (metres), every map a candidate.  Returns a dict: status (0 miss, 1 hit, 2 hit at the first
    read, -1 invalid), steps, hit, tie, p [n, 3] (hit point, voxel units), point (metres), t, dir, and -- at the hits --
    normal (unit, nan where the gradient is 0), grad_length, colour (0 .. 1)."""
    vs, mu = _vs_mu(maps)
    o = np.asarray(o, F).astype(np.float64).reshape(-1, 3)
    n = len(o)
    d = np.broadcast_to(np.asarray(d, F).astype(np.float64), (n, 3))
    t_min = np.broadcast_to(np.asarray(t_min, F).astype(np.float64), (n,))
    t_max = np.broadcast_to(np.asarray(t_max, F).astype(np.float64), (n,))
    max_range = float(F(max_range))
    limit = float(F(MAX_RAY_VOXELS) * F(maps[0].m.vs))
    assert 0.0 <= max_range <= limit
    if max_range == 0.0:
        max_range = limit
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.linalg.norm(d, axis=1)
        u = d / length[:, None]
        p0 = (o + t_min[:, None] * u) / vs
        valid = (np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(t_min) & np.isfinite(t_max) & (length > 0)
                 & np.isfinite(length) & (t_min >= 0) & np.isfinite(p0).all(1))
        valid &= np.all(np.abs(np.where(np.isfinite(p0), p0, 0.0)) <= MAX_COORD, axis=1)
    u = np.where(valid[:, None], u, 0.0)
    p = np.where(valid[:, None], p0, 0.0)
    total = np.where(valid, t_min / vs, 0.0)
    total_max = np.where(valid, np.minimum(t_max, t_min + max_range) / vs, 0.0)
    step_scale = mu / vs
    sdf = np.ones(n)
    hit = np.zeros(n, bool)
    tie = np.zeros(n, bool)
    steps = np.zeros(n, np.int64)
    active = valid & (total < total_max)
    tie |= valid & (np.abs(total - total_max) < tie_tol)
    for _ in range(MAX_RAY_VOXELS):
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        steps[idx] += 1
        vals, ws, fs = [], [], []
        for pm in maps:
            q = pm.to_map(p[idx])
            if sharp_ties:
                tie[idx] |= rm._round_flip(pm, q, tie_tol)
            else:
                frac = np.abs(q) - np.floor(np.abs(q))
                tie[idx] |= np.any(np.abs(frac - 0.5) < tie_tol, axis=1)
            near = ref64._iround(q)
            s16, _, f = pm.m.lookup(near)
            vals.append(s16 / 32767.0), ws.append(pm.weights(near, f)[0]), fs.append(f)
        s, nf = rm._combine(vals, ws, fs, np.ones(len(idx)), fallback=1.0)
        found = nf > 0
        step = np.full(len(idx), 8.0)
        win = found & (s <= 0.1) & (s >= -0.5)
        tie[idx] |= found & ((np.abs(s - 0.1) < tie_tol) | (np.abs(s + 0.5) < tie_tol))
        if win.any():
            t_sub = np.zeros(win.sum(), bool)
            s[win] = _trilinear_all(maps, p[idx[win]], t_sub, tie_tol, sharp_ties)
            tie[idx[win]] |= t_sub
        stop = found & (s <= 0.0)
        tie[idx] |= found & (np.abs(s) < tie_tol)
        step[found] = np.maximum(s[found] * step_scale, 1.0)
        sdf[idx] = s
        hit[idx[stop]] = True
        go = idx[~stop]
        p[go] += step[~stop, None] * u[go]
        total[go] += step[~stop]
        active[idx[stop]] = False
        active[go] = total[go] < total_max[go]
        tie[go] |= np.abs(total[go] - total_max[go]) < tie_tol
    h = np.nonzero(hit)[0]
    t_sub = np.zeros(len(h), bool)
    p[h] += (sdf[h] * step_scale)[:, None] * u[h]
    s = _trilinear_all(maps, p[h], t_sub, tie_tol, sharp_ties)
    p[h] += (s * step_scale)[:, None] * u[h]
    tie[h] |= t_sub
    status = np.where(~valid, -1, np.where(hit, np.where(steps == 1, 2, 1), 0))
    point = np.where(hit[:, None], p * vs, 0.0)
    out = dict(status=status, steps=steps, hit=hit, tie=tie, p=np.where(hit[:, None], p, 0.0), point=point, dir=u,
               t=np.where(hit, np.einsum("ij,ij->i", point - o, u), 0.0), normal=np.zeros((n, 3)), grad_length=np.zeros(n),
               colour=np.zeros((n, 3)))
    if len(h):
        g, out["grad_length"][h], out["colour"][h] = shade(maps, p[h], what)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["normal"][h] = g / np.linalg.norm(g, axis=1, keepdims=True)
    return out


def _trilinear_all(maps, p, tie, tie_tol, sharp_ties):
    """ref64_multimap.multi_trilinear with every map a candidate.  (With one map listed that function flags no tie: a cell
    boundary decides nothing between the reads of one map, whose trilinear value is continuous across it.)"""
    return rm.multi_trilinear(maps, np.ones((len(p), len(maps)), bool), p, tie, tie_tol, sharp_ties)
