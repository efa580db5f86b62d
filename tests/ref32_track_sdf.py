"""One evaluation of the depth-to-SDF tracking law (ref64_track_sdf.py states it in float64) restated in
plain numpy float32, in the order the law's text gives every operation, for one purpose: to measure what float32 does to
the 33 sums, and through them to the pivoted system, the step and the conditioning, when the coordinates are large (DESIGN
section 28).  No engine enters.  Every product and sum of the law is a float32 operation here; the float32 products are
accumulated in float64, as the law says.  numpy never fuses a multiply-add, and the sums are added pixel by pixel in one
order: contraction and the reduction order are what the factor 2 of the tests that use this file allows for.

`pivot` selects where the rotation part of a row and sums 29..31 are formed:
  "camera"  from r = R c, the point relative to the camera centre: the law;
  "world"   from p = R c + t, the point in world voxels: the law as it stood before section 28, kept to show what it loses.
`track` runs the reference's iteration on either one's sums.
"""
import numpy as np

import ref64_track_sdf as rt

F = np.float32
_OFFS = rt._OFFS


def _lerp3(v, c):
    """ref64_track_sdf._lerp3's expressions on float32 arrays (each operation rounds)."""
    one = F(1)
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    ux, uy, uz = one - cx, one - cy, one - cz
    x00, x10 = ux * v[:, 0] + cx * v[:, 1], ux * v[:, 2] + cx * v[:, 3]
    x01, x11 = ux * v[:, 4] + cx * v[:, 5], ux * v[:, 6] + cx * v[:, 7]
    y0, y1 = uy * x00 + cy * x10, uy * x01 + cy * x11
    val = uz * y0 + cz * y1
    gx = uz * (uy * (v[:, 1] - v[:, 0]) + cy * (v[:, 3] - v[:, 2])) + cz * (uy * (v[:, 5] - v[:, 4]) + cy * (v[:, 7] - v[:, 6]))
    gy = uz * (x10 - x00) + cz * (x11 - x01)
    gz = y1 - y0
    return val, np.stack([gx, gy, gz], 1)


def _rows(M, v):
    """(m0 x + m1 y) + m2 z per row of a float32 3 x 3, on float32 points [n, 3]."""
    return np.stack([(M[i, 0] * v[:, 0] + M[i, 1] * v[:, 1]) + M[i, 2] * v[:, 2] for i in range(3)], 1)


def evaluate(maps, depth, intr, Pt, gate=0.75, pivot="camera", pixels=None):
    """The 33 sums (float64 array) of one evaluation of one pyramid level at Pt [3, 4] (rounded to float32 here).  maps:
    ref64_track_sdf.PosedMap; pixels: a bool mask over the candidates (ref64's order) of those to keep, default all."""
    assert pivot in ("camera", "world")
    P = np.asarray(Pt, np.float64).astype(F)
    gate = F(gate)
    depth = np.asarray(depth, F)
    h, w = depth.shape
    fx, fy, cx, cy = (F(v) for v in np.asarray(intr, F))
    cand = np.flatnonzero(depth.reshape(-1) > F(1e-8))
    if pixels is not None:
        cand = cand[np.asarray(pixels, bool)]
    D = depth.reshape(-1)[cand]
    x, y = (cand % w).astype(F), (cand // w).astype(F)
    inv_vs = F(1.0 / float(maps[0].data.vs))
    c = np.stack([(D * ((x - cx) / fx)) * inv_vs, (D * ((y - cy) / fy)) * inv_vs, D * inv_vs], 1)
    r = _rows(P[:, :3], c)
    p = r + P[:, 3][None]
    n = len(cand)
    k = np.zeros(n, np.int64)
    num_d, den = np.zeros(n, F), np.zeros(n, F)
    num_g = np.zeros((n, 3), F)
    first_d, first_g = np.zeros(n, F), np.zeros((n, 3), F)
    for pm in maps:
        T = pm.Tt.astype(F)
        q = p if pm.identity else _rows(T[:, :3], p) + T[:, 3][None]
        fl = np.floor(q)
        inrange = np.all(np.abs(q) < F(262144.0), axis=1)
        cell = np.where(inrange[:, None], fl, 0).astype(np.int64)
        raw, wd, found = pm.data.voxels_at(cell[:, None, :] + _OFFS[None])
        ok = inrange & np.all(found & (wd > 0) & (np.abs(raw) != 32767), axis=1)
        s = raw.astype(F) / F(32767.0)
        fr = q - fl
        d, g = _lerp3(s, fr)
        om = _lerp3(wd.astype(F), fr)[0]
        if not pm.identity:
            g = _rows(T[:, :3].T.copy(), g)   # R^T g: (r0 gx + r1 gy) + r2 gz
        first = ok & (k == 0)
        first_d = np.where(first, d, first_d)
        first_g = np.where(first[:, None], g, first_g)
        num_d = np.where(ok, num_d + om * d, num_d)
        num_g = np.where(ok[:, None], num_g + om[:, None] * g, num_g)
        den = np.where(ok, den + om, den)
        k += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        blend = (k >= 2) & (den > 0)
        d = np.where(blend, num_d / den, np.where(k >= 2, F(0), first_d))
        g = np.where(blend[:, None], num_g / den[:, None], first_g)
    valid = (k > 0) & ~(np.abs(d) > gate)
    a = (r if pivot == "camera" else p)[valid]
    g, b = g[valid], -d[valid]
    A = np.stack([a[:, 1] * g[:, 2] - a[:, 2] * g[:, 1], a[:, 2] * g[:, 0] - a[:, 0] * g[:, 2],
                  a[:, 0] * g[:, 1] - a[:, 1] * g[:, 0], g[:, 0], g[:, 1], g[:, 2]], 1)
    assert A.dtype == F and b.dtype == F
    sums = np.zeros(rt.NSUMS)
    for col, (i, j) in enumerate(rt._TRI):
        sums[col] = (A[:, i] * A[:, j]).astype(np.float64).sum()
    for i in range(6):
        sums[21 + i] = (b * A[:, i]).astype(np.float64).sum()
    sums[27] = (b * b).astype(np.float64).sum()
    sums[28] = valid.sum()
    sums[29:32] = a.astype(np.float64).sum(0)
    sums[32] = n
    return sums


def track(maps, depth0, intr, pose_M, pivot="camera", **params):
    """ref64_track_sdf.track with every evaluation's sums replaced by this file's: the reference's iteration, in double, on
    float32 sums.  Returns (pose, result dict) as it does."""
    def ev32(maps_, depth, k, Pt, gate=0.75):
        ev = rt.evaluate(maps_, depth, k, Pt, gate)
        ev.sums = evaluate(maps_, depth, k, Pt, gate, pivot)
        if pivot == "world":
            ev.t = np.zeros(3)
        ev.valid = int(ev.sums[28])
        ev.cost = ev.cost_of(ev.sums, ev.gate)
        return ev

    return rt.track(maps, depth0, intr, pose_M, evaluator=ev32, **params)
