"""Float64 statement of dslam_track_camera_sdf: one evaluation of a depth image against N posed
maps, the cost, the pivot, the iteration per pyramid level, the stop reasons and the conditioning, in numpy, on maps given
as hash table + voxel array (ref64_register.MapData).  Shares no text with the engine.

One evaluation at P~ (camera -> world, 3 x 4, translation in voxels, entries rounded to float32) on one level of the depth
pyramid.  Every pixel (x, y) with depth D > 1e-8:
  c = (D (x - cx) / fx, D (y - cy) / fy, D) * float32(1 / vs);  p = P~ c;
  per map i (list order)  q = T~_i p, cell = floor(q); the 8 taps of the cell all resident, each with w_depth > 0 and raw sdf
                          not +-32767, else the map is a miss; d_i, g_i the trilinear interpolant of raw / 32767 and its
                          analytic gradient, w_i the trilinear interpolant of the taps' w_depth, g_i^w = R_i^T g_i;
  combine                 no map: a miss; one: its d, g; several: d = sum w_i d_i / sum w_i, g = sum w_i g_i^w / sum w_i;
  |d| > gate is a miss, else valid with b = -d and row A = [(p - t) x g, g], t the translation of P~ and p - t = R c the
                          three products of c with P~'s rotation, before t is added: the row is pivoted at the camera
                          centre and has no operand of the size of the camera's position;
  sums                    21 lower-triangle entries of sum A^T A, 6 of sum b A, sum b^2, valid, sum (p - t) (3), N.

What the engine may differ by: it evaluates the same expressions in float32 (u = 2^-24 per operation) and accumulates the
float32 products in double.  The first-order propagation of u, per valid pixel, extends ref64_register.py's over
  the camera point   dc = 4 u |c| (a difference, a quotient and two products on the longest path);
  the product with P~ dr = |R| dc + 3 u (|a x| + |b y| + |c z|) per row for r = p - t, and dp = dr + 3 u |d| for p;
  each map           dq = |T~| dp + 3 u (...) per row (dq = dp under the identity); fractions dc' = dq + 2 u; with M the
                     largest |s| of the taps, D the largest first difference along a cell edge, H2 the largest mixed second
                     difference over a face:  dd = sum_axis |g_axis| dc' + 10 u M,  dg = 16 u M + 8 u D + 2 H2 max dc';
                     the weight, with Mw, Dw the same of the taps' weights: dw = 3 Dw max dc' + 10 u Mw;
  the rotation back  dg^w = |R^T| dg + 3 u |R^T| |g| per component;
  the blend of k > 1 maps: numerators sum w_i v_i: sum (w_i dv_i + |v_i| dw_i + u |w_i v_i|) + (k - 1) u sum |w_i v_i|;
                     denominator: sum dw_i + (k - 1) u sum w_i; quotient: dnum / den + |num| dden / den^2 + u |v|;
  the row            rotation i: sum over its two products |r| dg + |g| dr + 2 u |r g|; translation: dg;
  products x y       |x| dy + |y| dx + u |x y|.
They are added over the pixels (no cancellation assumed).

Ties.  A pixel whose q has a coordinate within max(TIE_Q, dq) of an integer in any map -- dq the bound derived above for
that pixel, map and axis: 4e-5 at the origin, the spacing of float32 at q far from it -- may fall into the neighbouring cell
there in float32 (the value is continuous across the boundary, the gradient, the weight's slope and the 8-tap gate are not); a pixel
with | |d| - gate | < TIE_B may fall on the other side of the gate.  For those the alternatives are evaluated (the cell
moved on the tied axes, in all tied maps together and in each alone; valid or a miss) and each sum is compared as an
interval over them; counts are exact up to the number of tie pixels.
"""
import math

import numpy as np

from ref64_register import MapData, pose_distance, rigid, voxel_transform   # noqa: F401  (re-exported for the tests)
from ref64_tracker import subsample_with_holes

U = 2.0 ** -24
TIE_Q = 1e-4
TIE_B = 1e-5
NSUMS = 33
F = np.float32

DEFAULTS = dict(no_hierarchy_levels=3, run_till_level=0, max_evaluations=10, min_valid=500, residual_gate=0.75,
                term_rotation=1e-5, term_translation_voxels=1e-3)

_TRI = [(k, j) for k in range(6) for j in range(k + 1)]
_OFFS = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)], np.int64)
_EDGES = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
_FACES = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (2, 3, 6, 7), (0, 2, 4, 6), (1, 3, 5, 7)]


def _r32(a):
    return np.asarray(a, np.float64).astype(F).astype(np.float64)


class PosedMap:
    """A MapData under a world -> map transform T (4 x 4, metres; its entries are taken as float32, as the ABI's)."""

    def __init__(self, data, T):
        self.data = data
        self.T = np.asarray(T, F)
        self.identity = bool(np.array_equal(self.T, np.eye(4, dtype=F)))
        self.Tt = _r32(voxel_transform(self.T.astype(np.float64), data.vs))   # T~ as the engine holds it


def depth_level0(mm, a=0.001, b=0.0):
    """The view's float32 depth image of an int16 millimetre image (UpdateView: d * a + b, -1 for d <= 0 or d > 32000)."""
    mm = np.asarray(mm)
    d = (mm.astype(F) * F(a) + F(b)).astype(F)
    return np.where((mm <= 0) | (mm > 32000), F(-1.0), d).astype(F)


def pyramid(depth0, intr, levels):
    """Per level (float32 depth image, float32 intrinsics halved per level)."""
    out = [(np.asarray(depth0, F), np.asarray(intr, F))]
    for _ in range(1, levels):
        d, k = out[-1]
        out.append((subsample_with_holes(d)[1], (k * F(0.5)).astype(F)))
    return out


def camera_to_world(pose_M, vs):
    """P~ [3, 4] float64 of a world -> camera pose (4 x 4, metres): its rigid inverse with the translation in voxels."""
    Mv = voxel_transform(np.asarray(pose_M, F).astype(np.float64), vs)
    P = np.empty((3, 4))
    P[:, :3] = Mv[:, :3].T
    P[:, 3] = -(Mv[:, :3].T @ Mv[:, 3])
    return P


def pose_of(P, vs):
    """The world -> camera pose (4 x 4 float32, metres) of P~."""
    M = np.eye(4, dtype=F)
    M[:3, :3] = P[:, :3].T.astype(F)
    M[:3, 3] = (-(P[:, :3].T @ P[:, 3]) * vs).astype(F)
    return M


# ---------------------------------------------------------------------------------------------------------------------
# one map's read
# ---------------------------------------------------------------------------------------------------------------------
def _lerp3(v, c):
    """Trilinear interpolant of tap values v [n, 8] at fractions c [n, 3] and its analytic gradient [n, 3]."""
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    ux, uy, uz = 1 - cx, 1 - cy, 1 - cz
    x00, x10 = ux * v[:, 0] + cx * v[:, 1], ux * v[:, 2] + cx * v[:, 3]
    x01, x11 = ux * v[:, 4] + cx * v[:, 5], ux * v[:, 6] + cx * v[:, 7]
    y0, y1 = uy * x00 + cy * x10, uy * x01 + cy * x11
    val = uz * y0 + cz * y1
    gx = uz * (uy * (v[:, 1] - v[:, 0]) + cy * (v[:, 3] - v[:, 2])) + cz * (uy * (v[:, 5] - v[:, 4]) + cy * (v[:, 7] - v[:, 6]))
    gy = uz * (x10 - x00) + cz * (x11 - x01)
    gz = y1 - y0
    return val, np.stack([gx, gy, gz], 1)


def read_map(pm, q, cell, dq, weight_law="trilinear"):
    """One map's read of points q [n, 3] (its own frame, voxels) in `cell` [n, 3]: (ok, d, g (map frame), w, dd, dg, dw).
    weight_law: 'trilinear' is the law; 'tap0' is the wrong law the tests have to tell apart."""
    raw, w, found = pm.data.voxels_at(cell[:, None, :] + _OFFS[None])
    inrange = np.all(np.abs(q) < 262144.0, axis=1)
    ok = inrange & np.all(found & (w > 0) & (np.abs(raw) != 32767), axis=1)
    s = raw / 32767.0
    wf = w.astype(np.float64)
    c = q - cell
    d, g = _lerp3(s, c)
    om = wf[:, 0] if weight_law == "tap0" else _lerp3(wf, c)[0]
    dc = dq + 2 * U
    M = np.abs(s).max(1)
    D = np.max(np.stack([np.abs(s[:, j] - s[:, i]) for i, j in _EDGES], 1), 1)
    H2 = np.max(np.stack([np.abs((s[:, f[3]] - s[:, f[2]]) - (s[:, f[1]] - s[:, f[0]])) for f in _FACES], 1), 1)
    dd = (np.abs(g) * dc).sum(1) + 10 * U * M
    dg = 16 * U * M + 8 * U * D + 2 * H2 * dc.max(1)
    Dw = np.max(np.stack([np.abs(wf[:, j] - wf[:, i]) for i, j in _EDGES], 1), 1)
    dw = 3 * Dw * dc.max(1) + 10 * U * wf.max(1)
    return ok, d, g, om, dd, dg, dw


def _pixel_terms(maps, qs, dqs, cells, p, dp, gate, weight_law="trilinear"):
    """Pixels with camera-relative point p [n, 3] = R c (the rows' and sum 29..31's operand), per map the point qs[i], its bound dqs[i] and the cell to read it in:
    (valid [n], terms [n, 32], bounds [n, 32], d [n], holders [n]: the maps that passed their gate)."""
    n = len(p)
    k = np.zeros(n, np.int64)
    num_d, den, abs_d = np.zeros(n), np.zeros(n), np.zeros(n)
    num_g, abs_g = np.zeros((n, 3)), np.zeros((n, 3))
    e_num_d, e_den, e_num_g = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    first_d, first_dd = np.zeros(n), np.zeros(n)
    first_g, first_dg = np.zeros((n, 3)), np.zeros((n, 3))
    for pm, q, dq, cell in zip(maps, qs, dqs, cells):
        ok, d, g, om, dd, dg, dw = read_map(pm, q, cell, dq, weight_law)
        if pm.identity:
            gw, dgw = g, np.repeat(dg[:, None], 3, 1)
        else:
            R = pm.Tt[:, :3]
            gw = g @ R                                                  # R^T g
            dgw = dg[:, None] * np.abs(R).sum(0)[None] + 3 * U * (np.abs(g) @ np.abs(R))
        if weight_law == "unweighted":
            om, dw = np.ones(n), np.zeros(n)
        first = ok & (k == 0)
        first_d, first_dd = np.where(first, d, first_d), np.where(first, dd, first_dd)
        first_g, first_dg = np.where(first[:, None], gw, first_g), np.where(first[:, None], dgw, first_dg)
        o = ok.astype(np.float64)
        num_d += o * om * d
        abs_d += o * np.abs(om * d)
        e_num_d += o * (om * dd + np.abs(d) * dw + U * np.abs(om * d))
        den += o * om
        e_den += o * dw
        num_g += o[:, None] * om[:, None] * gw
        abs_g += o[:, None] * np.abs(om[:, None] * gw)
        e_num_g += o[:, None] * (om[:, None] * dgw + np.abs(gw) * dw[:, None] + U * np.abs(om[:, None] * gw))
        k += ok
    multi = k >= 2
    dn = np.where(multi, den, 1.0)
    km1 = np.maximum(k - 1, 0)
    e_dn = e_den + km1 * U * den
    d_bl = num_d / dn
    dd_bl = (e_num_d + km1 * U * abs_d) / dn + np.abs(num_d) * e_dn / dn ** 2 + U * np.abs(d_bl)
    g_bl = num_g / dn[:, None]
    dg_bl = ((e_num_g + km1[:, None] * U * abs_g) / dn[:, None] + np.abs(num_g) * (e_dn / dn ** 2)[:, None] + U * np.abs(g_bl))
    d, dd = np.where(multi, d_bl, first_d), np.where(multi, dd_bl, first_dd)
    g, dg = np.where(multi[:, None], g_bl, first_g), np.where(multi[:, None], dg_bl, first_dg)
    valid = (k > 0) & ~(np.abs(d) > gate)
    b, db = -d, dd
    A = np.concatenate([np.cross(p, g), g], 1)
    dA = np.empty((n, 6))
    for i, (j, l) in enumerate(((1, 2), (2, 0), (0, 1))):   # A_i = p_j g_l - p_l g_j
        dA[:, i] = (np.abs(p[:, j]) * dg[:, l] + np.abs(g[:, l]) * dp[:, j] + 2 * U * np.abs(p[:, j] * g[:, l])
                    + np.abs(p[:, l]) * dg[:, j] + np.abs(g[:, j]) * dp[:, l] + 2 * U * np.abs(p[:, l] * g[:, j]))
    dA[:, 3:] = dg
    terms, bounds = np.zeros((n, 32)), np.zeros((n, 32))
    for col, (r, c) in enumerate(_TRI):
        terms[:, col] = A[:, r] * A[:, c]
        bounds[:, col] = np.abs(A[:, r]) * dA[:, c] + np.abs(A[:, c]) * dA[:, r] + U * np.abs(terms[:, col])
    for r in range(6):
        terms[:, 21 + r] = b * A[:, r]
        bounds[:, 21 + r] = np.abs(b) * dA[:, r] + np.abs(A[:, r]) * db + U * np.abs(terms[:, 21 + r])
    terms[:, 27] = b * b
    bounds[:, 27] = 2 * np.abs(b) * db + U * terms[:, 27]
    terms[:, 28] = 1.0
    terms[:, 29:32] = p
    bounds[:, 29:32] = dp
    terms[~valid] = 0.0
    bounds[~valid] = 0.0
    return valid, terms, bounds, np.where(k > 0, d, np.inf), k


# ---------------------------------------------------------------------------------------------------------------------
# one evaluation
# ---------------------------------------------------------------------------------------------------------------------
class Evaluation:
    """sums [33]; lo / hi [33]: the interval a float32 evaluation of the same law may lie in; candidates, valid, ties."""

    def cost_of(self, sums, gate):
        n = sums[32]
        return (sums[27] + (n - sums[28]) * gate * gate) / n if n > 0 else gate * gate

    def cost_interval(self):
        n, g2 = self.sums[32], self.gate * self.gate
        if n <= 0:
            return g2, g2
        lo = (self.lo[27] + (n - self.hi[28]) * g2) / n
        hi = (self.hi[27] + (n - self.lo[28]) * g2) / n
        return lo * (1 - 2 * U), hi * (1 + 2 * U)   # (the result is handed out as a float32)

    def check_sums(self, got, what=""):
        """Assert the engine's 33 sums lie in the interval; returns the largest share of the bound they use."""
        got = np.asarray(got, np.float64)
        assert got[32] == self.sums[32], f"{what}: {got[32]:.0f} candidates, reference {self.sums[32]:.0f}"
        assert abs(got[28] - self.sums[28]) <= self.ties, f"{what}: valid {got[28]:.0f}, reference {self.sums[28]:.0f}, {self.ties} ties"
        slack = 1e-12 * np.maximum(np.abs(self.lo), np.abs(self.hi))   # the double accumulation itself
        bad = np.flatnonzero((got < self.lo - slack) | (got > self.hi + slack))
        assert len(bad) == 0, (f"{what}: sums {bad.tolist()} outside the bound: got {got[bad]}, reference {self.sums[bad]}, "
                               f"interval [{self.lo[bad]}, {self.hi[bad]}]")
        with np.errstate(divide="ignore", invalid="ignore"):
            used = np.nanmax(np.where(self.hi > self.lo, np.abs(got - self.sums) / (0.5 * (self.hi - self.lo)), 0.0))
        return float(used)


def camera_points(depth, intr, Pt, vs):
    """Of one pyramid level under P~ (rounded to float32 here): (pixel index [n] of the candidates, r [n, 3] = R c, dr, p = r + t,
    dp)."""
    P = _r32(Pt)
    depth = np.asarray(depth, F)
    h, w = depth.shape
    fx, fy, cx, cy = (float(v) for v in np.asarray(intr, F))
    cand = np.flatnonzero(depth.reshape(-1) > F(1e-8))
    D = depth.reshape(-1)[cand].astype(np.float64)
    x, y = (cand % w).astype(np.float64), (cand // w).astype(np.float64)
    inv_vs = float(F(1.0 / float(vs)))
    c = np.stack([D * ((x - cx) / fx), D * ((y - cy) / fy), D], 1) * inv_vs
    dc = 4 * U * np.abs(c)
    r = c @ P[:, :3].T
    dr = dc @ np.abs(P[:, :3]).T + 3 * U * (np.abs(c) @ np.abs(P[:, :3]).T)
    return cand, r, dr, r + P[:, 3], dr + 3 * U * np.abs(P[:, 3])


def world_points(depth, intr, Pt, vs):
    """Of one pyramid level: (pixel index [n] of the candidates, p [n, 3], dp [n, 3]) under P~ (rounded to float32 here)."""
    cand, _, _, p, dp = camera_points(depth, intr, Pt, vs)
    return cand, p, dp


def evaluate(maps, depth, intr, Pt, gate=0.75, weight_law="trilinear"):
    """One evaluation of one pyramid level (float32 depth image [h, w], its float32 intrinsics) at Pt [3, 4]."""
    gate = float(F(gate))
    vs = maps[0].data.vs
    cand, r, dr, p, dp = camera_points(depth, intr, Pt, vs)
    ev = Evaluation()
    ev.gate, ev.candidates = gate, len(cand)
    qs, dqs, cells, tie_axes, windows = [], [], [], [], []
    for pm in maps:
        if pm.identity:
            q, dq = p, dp
        else:
            T = pm.Tt
            q = p @ T[:, :3].T + T[:, 3]
            dq = dp @ np.abs(T[:, :3]).T + 3 * U * (np.abs(p) @ np.abs(T[:, :3]).T + np.abs(T[:, 3]))
        cell = np.floor(q)
        frac = q - cell
        qs.append(q); dqs.append(dq); cells.append(cell.astype(np.int64))
        windows.append(np.maximum(TIE_Q, dq))
        tie_axes.append(np.minimum(frac, 1 - frac) < windows[-1])
    valid, terms, bounds, d, holders = _pixel_terms(maps, qs, dqs, cells, r, dr, gate, weight_law)
    tie = np.any([t.any(1) for t in tie_axes], axis=0) | (np.abs(np.abs(d) - gate) < TIE_B) if len(cand) else np.zeros(0, bool)
    sums = np.zeros(NSUMS)
    sums[:32] = terms.sum(0)
    sums[32] = ev.candidates
    lo, hi = np.zeros(NSUMS), np.zeros(NSUMS)
    ev.tie_lo, ev.tie_hi, ev.sums_no_tie = np.zeros(NSUMS), np.zeros(NSUMS), np.zeros(NSUMS)
    nt = ~tie
    lo[:32] = terms[nt].sum(0) - bounds[nt].sum(0)
    hi[:32] = terms[nt].sum(0) + bounds[nt].sum(0)
    lo[32] = hi[32] = ev.candidates
    ti = np.flatnonzero(tie)
    if len(ti):
        alt_lo, alt_hi = terms[ti] - bounds[ti], terms[ti] + bounds[ti]
        sub_q, sub_dq = [q[ti] for q in qs], [dq[ti] for dq in dqs]
        sub_win = [w[ti] * a[ti] for w, a in zip(windows, tie_axes)]
        shifts = {(0, 0, 0)} | {tuple(s * (((combo >> a) & 1) * 2 - 1) for a in range(3)) for combo in range(8) for s in (1, -1)}
        movers = [list(range(len(maps)))] + ([[i] for i in range(len(maps))] if len(maps) > 1 else [])
        for moved in movers:
            for shift in sorted(shifts):
                c2 = [np.floor(sub_q[i] + (np.array(shift) * sub_win[i] if i in moved else 0.0)).astype(np.int64)
                      for i in range(len(maps))]
                _, t2, b2, d2, _ = _pixel_terms(maps, sub_q, sub_dq, c2, r[ti], dr[ti], gate, weight_law)
                alt_lo, alt_hi = np.minimum(alt_lo, t2 - b2), np.maximum(alt_hi, t2 + b2)
                on_gate = np.abs(np.abs(d2) - gate) < TIE_B   # either side of the gate: valid, or a miss
                if on_gate.any():
                    _, t3, b3, _, _ = _pixel_terms(maps, sub_q, sub_dq, c2, r[ti], dr[ti], 1e30, weight_law)
                    g_ = on_gate[:, None]
                    alt_lo = np.where(g_, np.minimum(alt_lo, np.minimum(t3 - b3, 0.0)), alt_lo)
                    alt_hi = np.where(g_, np.maximum(alt_hi, np.maximum(t3 + b3, 0.0)), alt_hi)
        lo[:32] += alt_lo.sum(0)
        hi[:32] += alt_hi.sum(0)
        ev.tie_lo[:32], ev.tie_hi[:32] = alt_lo.sum(0), alt_hi.sum(0)
    ev.sums, ev.lo, ev.hi = sums, lo, hi
    ev.sums_no_tie[:32] = terms[nt].sum(0)   # the pixels that are no tie, alone; the tie pixels' share lies in tie_lo .. tie_hi
    ev.sums_no_tie[32] = ev.candidates
    ev.tie, ev.t = tie, _r32(Pt)[:, 3]
    ev.valid, ev.ties = int(sums[28]), int(tie.sum())
    ev.tie_share = ev.ties / max(ev.candidates, 1)
    ev.cost = ev.cost_of(sums, gate)
    ev.maps_per_pixel = float(holders.mean()) if len(cand) else 0.0
    ev.d = d   # the blended value per candidate (inf: no map holds the point)
    ev.pixels = cand
    return ev


# ---------------------------------------------------------------------------------------------------------------------
# the iteration
# ---------------------------------------------------------------------------------------------------------------------
def pivot(sums, t):
    """(c, H_c, g_c): the sums, whose rows are pivoted at the camera centre t, re-pivoted to the centroid; c = t + sum (p - t)
    / valid is the centroid in the world."""
    H = np.zeros((6, 6))
    for col, (k, j) in enumerate(_TRI):
        H[k, j] = H[j, k] = sums[col]
    c = sums[29:32] / sums[28] if sums[28] > 0 else np.zeros(3)
    S = np.eye(6)
    S[:3, 3:] = np.array([[0, c[2], -c[1]], [-c[2], 0, c[0]], [c[1], -c[0], 0]])
    return np.asarray(t, np.float64) + c, S @ H @ S.T, S @ sums[21:27]


def conditioning(Hc):
    dg = np.diag(Hc)
    if not np.all(dg > 0):
        return 0.0
    s = 1.0 / np.sqrt(dg)
    return float(np.linalg.eigvalsh(Hc * np.outer(s, s))[0])


def damped_step(Hc, gc, lam):
    dg = np.diag(Hc)
    use = np.flatnonzero(dg > 0)
    y = np.zeros(6)
    if len(use):
        y[use] = np.linalg.solve(Hc[np.ix_(use, use)] + lam * np.diag(dg[use]), gc[use])
    return y


def moved(y, c, Pt):
    """Inc P~ with Inc: p -> c + R(y[:3]) (p - c) + y[3:]."""
    R = rigid(float(np.linalg.norm(y[:3])), y[:3], (0.0, 0.0, 0.0))[:3, :3] if np.linalg.norm(y[:3]) > 0 else np.eye(3)
    out = np.empty((3, 4))
    out[:, :3] = R @ Pt[:, :3]
    out[:, 3] = R @ Pt[:, 3] + (c - R @ c + y[3:])
    return out


def track(maps, depth0, intr, pose_M, evaluator=None, **params):
    """dslam_track_camera_sdf on PosedMaps.  depth0: the view's float32 depth image; pose_M: 4 x 4 world -> camera in metres
    (its entries are taken as float32).  Returns (pose 4 x 4 float32 -- pose_M's own bytes if no step was accepted --, result
    dict as dslam_track_sdf_result plus `per_level`: level -> dict(evaluations, stop_reason, trace) and `last`: the finest
    level's last accepted Evaluation; a trace holds one dict per evaluation with cost, valid, tie_share and, for trial
    evaluations, accepted, lam, margin and cost_slack as ref64_register.register's).  evaluator: what stands in for `evaluate`
    (ref32_track_sdf.py: the same iteration on float32 sums)."""
    evaluate_ = evaluator or evaluate
    pr = dict(DEFAULTS)
    pr.update({k: v for k, v in params.items() if v})
    pose_M = np.asarray(pose_M, F)
    vs = maps[0].data.vs
    gate = float(F(pr["residual_gate"]))
    levels = pyramid(depth0, intr, pr["no_hierarchy_levels"])
    Pt = camera_to_world(pose_M, vs)
    accepted_any, total, stepped, per_level = False, 0, 0, {}
    for level in range(pr["no_hierarchy_levels"] - 1, pr["run_till_level"] - 1, -1):
        depth, k = levels[level]
        good = evaluate_(maps, depth, k, Pt, gate)
        trace = [dict(cost=good.cost, valid=good.valid, tie_share=good.tie_share, ev=good)]
        evaluations, stop, lam, accepted_here = 1, -1, 1.0, False
        cost_first = good.cost
        if good.valid < pr["min_valid"]:
            stop = 3
        while stop < 0:
            if evaluations >= pr["max_evaluations"]:
                stop = 1
                break
            c, Hc, gc = pivot(good.sums, good.t)
            y = damped_step(Hc, gc, lam)
            trial = moved(y, c, Pt)
            ev = evaluate_(maps, depth, k, trial, gate)
            evaluations += 1
            accept = ev.valid >= pr["min_valid"] and ev.cost < good.cost
            (l1, h1), (l2, h2) = ev.cost_interval(), good.cost_interval()
            trace.append(dict(cost=ev.cost, valid=ev.valid, tie_share=ev.tie_share, ev=ev, accepted=accept, lam=lam,
                              margin=abs(ev.cost - good.cost), cost_slack=(h1 - l1) + (h2 - l2)))
            if accept:
                used = lam
                Pt, good, accepted_here = trial, ev, True
                lam = max(lam / 10.0, 1e-6)
                if (used <= 1.0 and np.linalg.norm(y[:3]) < float(F(pr["term_rotation"]))
                        and np.linalg.norm(y[3:]) < float(F(pr["term_translation_voxels"]))):
                    stop = 0
            else:
                lam *= 10.0
                if lam > 1e6:
                    stop = 2
        total += evaluations
        if accepted_here:
            accepted_any = True
            stepped |= 1 << level
        cond = 0.0 if stop == 3 else conditioning(pivot(good.sums, good.t)[1])
        per_level[level] = dict(evaluations=evaluations, stop_reason=stop, trace=trace)
        res = dict(stop_reason=stop, candidates=good.candidates, valid_last=good.valid, cost_first=cost_first,
                   cost_last=good.cost, conditioning=cond, last=good)
    res.update(evaluations=total, levels_stepped=stepped, per_level=per_level)
    return (pose_of(Pt, vs) if accepted_any else pose_M.copy()), res
