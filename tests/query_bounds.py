"""How far a float32 evaluation of dslam_query_points may lie from ref64_query.sample_points, point by point (DESIGN.md
section 31).  Everything here is computed from the maps and the float64 reference, nothing from an engine's output.

Two terms, as DESIGN sections 18 and 27 derive theirs.

1. The transform's rounding.  P is the largest |coordinate| (voxel units) among the world points and their map-frame images,
   u = spacing(float32(2 P)) (a partial sum of the mat-vec may be twice a coordinate).  The device's map-frame coordinate
   differs from the reference's, per component, by at most

       DELTA_U * u,   DELTA_U = sqrt(3) + 3 + 1/2:

   the point is scaled to voxels by a rounded 1/vs and a rounded product (1 u on a world coordinate, sqrt(3) u behind a
   rotation), to_map rounds three products and three sums (u/2 each), and the translation in voxel units is itself rounded
   to float32 (u/2).  A read moves by at most its slope times that.  The slope is taken where the point is, from the stored
   voxels: a trilinear interpolant changes along an axis by no more than the largest difference between two taps of the
   cell, so over three axes a read of map i moves by at most 3 DELTA_U u (max - min of the cell's 8 taps).  For the sdf
   inside the band that range is the vs / mu per voxel of a distance field (plus its 1 / 32767 steps); at the rim of the
   allocated blocks, where a missing tap reads 1.0 beside a stored -1.0, it is up to 2, and a constant slope would either
   fail there or test nothing elsewhere.  The gradient's two reads per axis lie one voxel either side, so its range is taken
   over the 4 x 4 x 4 taps around the cell, twice.

2. The rounding of the float32 sums.  A trilinear read is three nested levels of (1 - c) a + c b: per level one rounding
   of 1 - c, two products, one sum, so 12 roundings of 2^-24 relative to the largest tap (EPS_TRI); the gradient's reads
   are sums of four products of three factors, differences and a division: 16 (EPS_GRAD, per unit of sdf), and the
   rotation back to the world adds 3.  The n-map blend num / den rounds n products and n - 1 sums above, n - 1 below and
   the quotient: (2 n + 1) 2^-24 of the largest value.

The blend itself: with found maps' values v_i and weights w_i, f = sum(w_i v_i) / W.  If every v_i is off by at most dv_i
and every w_i by at most dw_i, then, because sum(w_i (v_i - f)) = 0,

    f' - f = [ sum(w'_i (v'_i - v_i)) + sum((w'_i - w_i)(v_i - f)) ] / W'
    |f' - f| <= [ sum((w_i + dw_i) dv_i) + sum(dw_i |v_i - f|) ] / (W - sum(dw_i))

which is exact, not first order; where the denominator is not positive the bound is infinite (the weights there are so
small that the transform's rounding alone can move the blend anywhere between the maps' values).  One found map gives its
own value (dv_i), none gives the first map's read.
"""
import numpy as np

import ref64_multimap as rm

F = np.float32
EPS = 2.0 ** -24
DELTA_U = np.sqrt(3.0) + 3.5
EPS_TRI, EPS_GRAD = 12 * EPS, 19 * EPS


def delta(maps, p):
    """(DELTA_U * u, P) for world points p (voxel units)."""
    P = max([np.abs(p).max()] + [np.abs(pm.to_map(p)).max() for pm in maps])
    return DELTA_U * float(np.spacing(F(2.0 * P))), float(P)


def _cell_ranges(pm, q):
    """Per point: max - min over the cell's 8 taps of sdf / 32767, w_depth, colour / 255 [.., 3], w_color; the largest
    w_depth and w_color; and max - min of sdf / 32767 over the 4 x 4 x 4 taps around the cell."""
    q0 = np.floor(q).astype(np.int64)
    off = np.stack(np.meshgrid(*[np.arange(-1, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    taps = q0[:, None, :] + off[None]
    s, clr, _ = pm.m.lookup(taps)
    wd, wc = pm.m.lookup_weights(taps)
    s, clr, wd, wc = s / 32767.0, clr / 255.0, wd.astype(np.float64), wc.astype(np.float64)
    inner = np.all((off >= 0) & (off <= 1), axis=1)
    rng = lambda a: a.max(axis=1) - a.min(axis=1)
    return dict(sdf=rng(s[:, inner]), wd=rng(wd[:, inner]), clr=rng(clr[:, inner]), wc=rng(wc[:, inner]),
                wd_max=wd[:, inner].max(axis=1), wc_max=wc[:, inner].max(axis=1), sdf_wide=rng(s))


def _blend_bound(vals, ws, fs, dvs, dws, scale):
    """The bound of the module docstring; vals [N, k], ws / dws [N], fs [N] bool, dvs [N] per map (list order); scale: the
    largest |value| for the blend's own rounding."""
    n = len(fs[0])
    k = vals[0].shape[1]
    first_any = vals[0]
    f, nf = rm._combine(vals, ws, fs, first_any)
    W, Wd, num = np.zeros(n), np.zeros(n), np.zeros((n, k))
    first_dv = np.full(n, np.nan)
    for v, w, fo, dv, dw in zip(vals, ws, fs, dvs, dws):
        first_dv = np.where(np.isnan(first_dv) & fo, dv, first_dv)
        W += fo * w
        Wd += fo * dw
        num += fo[:, None] * ((w + dw) * dv)[:, None] + fo[:, None] * dw[:, None] * np.abs(v - f)
    den = W - Wd
    with np.errstate(invalid="ignore", divide="ignore"):
        many = np.where((den > 0)[:, None], num / den[:, None], np.inf)
    # no weight anywhere, and none within reach of the rounding: the fallback (sdf 1.0 / the first contributor's value)
    many = np.where(((W == 0) & (Wd == 0))[:, None], np.nan_to_num(first_dv)[:, None], many)
    out = np.where((nf == 0)[:, None], dvs[0][:, None], np.where((nf == 1)[:, None], np.nan_to_num(first_dv)[:, None], many))
    return out + (2 * np.maximum(nf, 1) + 1)[:, None] * EPS * scale


def point_bounds(maps, p_world_m):
    """Bounds of sdf [N], weight [N], grad [N, 3], colour [N, 3] (0 .. 1) for world points in metres, and `near_cell` [N]:
    a map-frame coordinate lies within DELTA_U u of a cell boundary -- there the device may read the neighbouring cell,
    whose slope this bound has not looked at (the read is continuous across the boundary, so nothing jumps; the point is
    left out of the value comparison).  Also delta and P."""
    vs = float(F(maps[0].m.vs))
    p = np.asarray(p_world_m, F).astype(np.float64).reshape(-1, 3) / vs
    d, P = delta(maps, p)
    n = len(p)
    v_s, w_s, f_s, dv_s, dw_s = [], [], [], [], []
    v_g, dv_g, v_c, w_c, f_c, dv_c, dw_c = [], [], [], [], [], [], []
    near = np.zeros(n, bool)
    d_weight = np.zeros(n)
    for pm in maps:
        q = pm.to_map(p)
        near |= rm._floor_tie(q, d)
        r = _cell_ranges(pm, q)
        v, w, f = rm._trilinear(pm, q)
        v_s.append(v[:, None]), w_s.append(w), f_s.append(f)
        dv_s.append(3 * d * r["sdf"] + EPS_TRI)
        dw = 3 * d * r["wd"] + EPS_TRI * r["wd_max"]
        dw_s.append(dw)
        d_weight += f * dw
        g = rm._gradient(pm, q)
        v_g.append(g if pm.identity else g @ pm.R)
        dv_g.append(np.sqrt(3.0) * (2 * 3 * d * r["sdf_wide"] + 2 * EPS_GRAD))
        c, wc, fc = rm._trilinear(pm, q, colour=True)
        v_c.append(c / 255.0), w_c.append(wc), f_c.append(fc)
        dv_c.append(3 * d * r["clr"].max(axis=1) + EPS_TRI)
        dw_c.append(3 * d * r["wc"] + EPS_TRI * r["wc_max"])
    weight = sum(f * w for f, w in zip(f_s, w_s))
    return dict(sdf=_blend_bound(v_s, w_s, f_s, dv_s, dw_s, 1.0)[:, 0],
                weight=d_weight + len(maps) * EPS * weight,
                grad=_blend_bound(v_g, w_s, f_s, dv_g, dw_s, 2.0),
                colour=_blend_bound(v_c, w_c, f_c, dv_c, dw_c, 1.0),
                near_cell=near, delta=d, P=P)
