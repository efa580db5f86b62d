"""Float64 statement of dslam_register_maps: one evaluation, the cost, the pivot, the iteration,
the stop reasons and the conditioning, in numpy, on any map given as hash table + voxel array (an analytic_maps.Map or a
map downloaded from an engine).  Shares no text with the engine.

One evaluation at X~ (3 x 4, translation in voxels, entries rounded to float32).  Every voxel of every resident source
block (table entries with ptr >= 0, ascending), at integer position p with (sdf_s, w_s):
  candidate     w_s > 0 and |sdf_s| < int(float32(band) * 32767);
  q = X~ p, cell = floor(q), c = q - cell;
  destination   the 8 taps of the cell all in resident blocks, each with w_depth > 0 and raw sdf not +-32767;
  d, g          the trilinear interpolant of raw / 32767 over the taps and its analytic gradient;
  b = sdf_s / 32767 - d, a miss if |b| > gate, else valid with row A = [q x g, g];
  sums          21 lower-triangle entries of sum A^T A, 6 of sum b A, sum b^2, valid, sum q (3), N.

What the engine may differ by.  It evaluates the same expressions in float32 (u = 2^-24 per operation) and accumulates the
float32 products in double.  Per valid voxel the first-order propagation of u through the stated operations is
  dq   = 3 u (|a x| + |b y| + |c z| + |d|) per row of X~ (three roundings on the longest path), fractions dc = dq + 2 u;
  ds   = u |s| for every tap value raw / 32767, M = max |s|, D = max first difference along a cell edge, H2 = max mixed
         second difference over a cell face;
  dd   = sum_axis |g_axis| dc + 10 u M                (one division and three lerp stages of three operations);
  dg   = 16 u M + 8 u D + 2 H2 max(dc)                (the worst of the three components: gz subtracts two 7 u M lerps)
  db   = dd + u |s_s| + u |b|;
  dA   rotation i: sum over its two products |q| dg + |g| dq + 2 u |q g|; translation: dg;
  products x y: |x| dy + |y| dx + u |x y|.
They are added over the voxels (no cancellation assumed), exactly as the tracker's bound is (ref64_tracker.py).

Ties.  A voxel whose q has a coordinate within TIE_Q of an integer may fall into the neighbouring cell in float32 (the
value is continuous there, the gradient and the destination gate are not); a voxel with | |b| - gate | < TIE_B may fall on
the other side of the gate.  For those the alternatives are evaluated (every choice of cell on the tied axes, valid or
miss) and each sum is compared as an interval over them; counts are exact up to the number of tie voxels.  If every entry
of X~ is an integer (the identity, a shift by whole voxels) q is a small integer, exact in float32: no cell ties there.
"""
import math

import numpy as np

U = 2.0 ** -24
TIE_Q = 1e-4
TIE_B = 1e-5
NSUMS = 33

DEFAULTS = dict(band=0.5, residual_gate=0.75, max_evaluations=30, min_valid=500, term_rotation=1e-5,
                term_translation_voxels=1e-3)

_TRI = [(k, j) for k in range(6) for j in range(k + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------------------------------------------------
class Moved:
    """An analytic geometry seen in the frame y = X x (X rigid, 4 x 4, metres): sdf(y) = geom.sdf(X^-1 y)."""

    def __init__(self, geom, X):
        self.geom, self.X = geom, np.asarray(X, np.float64)
        self.Xinv = np.linalg.inv(self.X)

    def sdf(self, y):
        return self.geom.sdf(y @ self.Xinv[:3, :3].T + self.Xinv[:3, 3])


def rigid(angle, axis, t, centre=(0.0, 0.0, 0.0)):
    """Rotation by `angle` (rad) about `axis` through `centre`, then a translation t (metres); 4 x 4 float64."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    c = np.asarray(centre, np.float64)
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = c - R @ c + np.asarray(t, np.float64)
    return X


def pose_difference(Xa, Xb, centre, vs):
    """(rotation angle in rad between the two transforms, distance in voxels between the images of `centre`)."""
    Xa, Xb = np.asarray(Xa, np.float64), np.asarray(Xb, np.float64)
    R = Xa[:3, :3] @ Xb[:3, :3].T
    vee = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    ang = math.atan2(float(np.linalg.norm(vee)), (np.trace(R) - 1.0) / 2.0)
    c = np.append(np.asarray(centre, np.float64), 1.0)
    return ang, float(np.linalg.norm((Xa @ c - Xb @ c)[:3]) / vs)


def pose_distance(Xa, Xb, corners, vs):
    """One figure for two transforms: the largest distance, in voxels, between the images of `corners` [n, 3] (metres)."""
    P = np.concatenate([np.asarray(corners, np.float64), np.ones((len(corners), 1))], 1)
    d = (P @ np.asarray(Xa, np.float64).T - P @ np.asarray(Xb, np.float64).T)[:, :3]
    return float(np.linalg.norm(d, axis=1).max() / vs)


# ---------------------------------------------------------------------------------------------------------------------
# maps as data
# ---------------------------------------------------------------------------------------------------------------------
class MapData:
    """Hash table [entries] + voxel array [local blocks, 512]: the resident blocks in table order and a lookup."""

    def __init__(self, table, vba, vs):
        self.vs = float(np.float32(vs))   # (the scene parameter is a float32)
        live = np.flatnonzero(table["ptr"] >= 0)
        self.block_pos = table["pos"][live].astype(np.int64)
        self.ptr = table["ptr"][live].astype(np.int64)
        self.vba = vba
        keys = self._key(self.block_pos)
        order = np.argsort(keys)
        self._keys, self._ptr_sorted = keys[order], self.ptr[order]

    @classmethod
    def of_map(cls, m):
        return cls(m.hash, m.vba, m.vs)

    @classmethod
    def of_scene(cls, api, scene):
        return cls(api.download_hash_table(scene), api.download_voxel_blocks(scene), scene.params.voxel_size)

    @staticmethod
    def _key(b):
        return ((b[..., 0] + 32768) << 32) | ((b[..., 1] + 32768) << 16) | (b[..., 2] + 32768)

    def corners(self):
        """The 8 corners (metres) of the bounding box of the resident blocks."""
        lo, hi = self.block_pos.min(0) * 8 * self.vs, (self.block_pos.max(0) + 1) * 8 * self.vs
        return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])

    def centre(self):
        return self.corners().mean(0)

    def voxels_at(self, v):
        """(raw sdf int64, w_depth int64, resident bool) of integer voxel positions v [..., 3]."""
        v = np.asarray(v, np.int64)
        b = v >> 3
        inside = np.all((b >= -32768) & (b <= 32767), axis=-1)
        keys = self._key(np.where(inside[..., None], b, 0))
        if len(self._keys) == 0:
            found = np.zeros(keys.shape, bool)
            i = np.zeros(keys.shape, np.int64)
        else:
            i = np.minimum(np.searchsorted(self._keys, keys), len(self._keys) - 1)
            found = inside & (self._keys[i] == keys)
        ptr = np.where(found, self._ptr_sorted[i] if len(self._keys) else 0, 0)
        loc = (v[..., 0] & 7) | ((v[..., 1] & 7) << 3) | ((v[..., 2] & 7) << 6)
        vox = self.vba[ptr, loc]
        sdf = np.where(found, vox["sdf"].astype(np.int64), 32767)
        w = np.where(found, vox["w_depth"].astype(np.int64), 0)
        return sdf, w, found

    def source_voxels(self):
        """(p [n, 3] int64, raw sdf [n], w_depth [n]) of every voxel of every resident block, table order."""
        loc = np.arange(512)
        off = np.stack([loc & 7, (loc >> 3) & 7, loc >> 6], -1)
        p = (self.block_pos[:, None, :] * 8 + off[None]).reshape(-1, 3)
        vox = self.vba[self.ptr]
        return p, vox["sdf"].astype(np.int64).reshape(-1), vox["w_depth"].astype(np.int64).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# one evaluation
# ---------------------------------------------------------------------------------------------------------------------
def voxel_transform(X, vs):
    """X~ of a 4 x 4 transform in metres (entries as given): rows 0..2, translation / vs, in float64 [3, 4]."""
    X = np.asarray(X, np.float64)
    out = X[:3, :].copy()
    out[:, 3] = X[:3, 3] / float(vs)
    return out


def round32(Xt):
    return np.asarray(Xt, np.float64).astype(np.float32).astype(np.float64)


def _cell_terms(dst, q, cell, s_src, dq, gate):
    """For voxels with position q [n, 3] read in `cell` [n, 3]: (valid [n], terms [n, 32], bounds [n, 32], b [n]).  Terms
    and bounds are zero where the voxel is a miss; column k is the voxel's contribution to sum k (k < 32)."""
    n = len(q)
    taps = np.stack([cell + np.array([k & 1, (k >> 1) & 1, k >> 2]) for k in range(8)], 1)  # [n, 8, 3]
    raw, w, found = dst.voxels_at(taps)
    ok = np.all(found & (w > 0) & (np.abs(raw) != 32767), axis=1)
    s = raw / 32767.0
    c = q - cell
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    ux, uy, uz = 1 - cx, 1 - cy, 1 - cz
    x00, x10 = ux * s[:, 0] + cx * s[:, 1], ux * s[:, 2] + cx * s[:, 3]
    x01, x11 = ux * s[:, 4] + cx * s[:, 5], ux * s[:, 6] + cx * s[:, 7]
    y0, y1 = uy * x00 + cy * x10, uy * x01 + cy * x11
    d = uz * y0 + cz * y1
    gx = uz * (uy * (s[:, 1] - s[:, 0]) + cy * (s[:, 3] - s[:, 2])) + cz * (uy * (s[:, 5] - s[:, 4]) + cy * (s[:, 7] - s[:, 6]))
    gy = uz * (x10 - x00) + cz * (x11 - x01)
    gz = y1 - y0
    g = np.stack([gx, gy, gz], 1)
    ss = s_src / 32767.0
    b = ss - d
    valid = ok & ~(np.abs(b) > gate)
    A = np.concatenate([np.cross(q, g), g], 1)
    # ---- the rounding bound (module docstring) ----
    M = np.abs(s).max(1)
    edges = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
    D = np.max(np.stack([np.abs(s[:, j] - s[:, i]) for i, j in edges], 1), 1)
    faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (2, 3, 6, 7), (0, 2, 4, 6), (1, 3, 5, 7)]
    H2 = np.max(np.stack([np.abs((s[:, f[3]] - s[:, f[2]]) - (s[:, f[1]] - s[:, f[0]])) for f in faces], 1), 1)
    dc = dq + 2 * U
    dd = (np.abs(g) * dc).sum(1) + 10 * U * M
    dg = 16 * U * M + 8 * U * D + 2 * H2 * dc.max(1)
    db = dd + U * np.abs(ss) + U * np.abs(b)
    dA = np.empty((n, 6))
    for i, (j, k) in enumerate(((1, 2), (2, 0), (0, 1))):   # A_i = q_j g_k - q_k g_j
        dA[:, i] = (np.abs(q[:, j]) * dg + np.abs(g[:, k]) * dq[:, j] + 2 * U * np.abs(q[:, j] * g[:, k])
                    + np.abs(q[:, k]) * dg + np.abs(g[:, j]) * dq[:, k] + 2 * U * np.abs(q[:, k] * g[:, j]))
    dA[:, 3:] = dg[:, None]
    terms, bounds = np.zeros((n, 32)), np.zeros((n, 32))
    for col, (k, j) in enumerate(_TRI):
        terms[:, col] = A[:, k] * A[:, j]
        bounds[:, col] = np.abs(A[:, k]) * dA[:, j] + np.abs(A[:, j]) * dA[:, k] + U * np.abs(terms[:, col])
    for k in range(6):
        terms[:, 21 + k] = b * A[:, k]
        bounds[:, 21 + k] = np.abs(b) * dA[:, k] + np.abs(A[:, k]) * db + U * np.abs(terms[:, 21 + k])
    terms[:, 27] = b * b
    bounds[:, 27] = 2 * np.abs(b) * db + U * terms[:, 27]
    terms[:, 28] = 1.0
    terms[:, 29:32] = q
    bounds[:, 29:32] = dq
    terms[~valid] = 0.0
    bounds[~valid] = 0.0
    return valid, terms, bounds, b


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
        """Assert the engine's 33 sums lie in the interval."""
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


def evaluate(src, dst, Xt, band=0.5, gate=0.75):
    """One evaluation at Xt [3, 4] (rounded to float32 here).  `src`, `dst`: MapData."""
    X = round32(Xt)
    gate = float(np.float32(gate))
    band_raw = int(np.float32(band) * np.float32(32767.0))
    p, sdf, w = src.source_voxels()
    cand = (w > 0) & (np.abs(sdf) < band_raw)
    p, sdf = p[cand].astype(np.float64), sdf[cand].astype(np.float64)
    ev = Evaluation()
    ev.gate, ev.candidates = gate, int(cand.sum())
    q = p @ X[:, :3].T + X[:, 3]
    dq = 3 * U * (np.abs(p) @ np.abs(X[:, :3]).T + np.abs(X[:, 3]))
    exact = bool(np.all(X == np.rint(X)))   # the identity, whole-voxel shifts: q is a small integer, exact in float32
    if exact:
        dq = np.zeros_like(dq)
    cell = np.floor(q)
    valid, terms, bounds, b = _cell_terms(dst, q, cell.astype(np.int64), sdf, dq, gate)
    frac = q - cell
    tie_axis = (np.minimum(frac, 1 - frac) < TIE_Q) & (not exact)
    tie = tie_axis.any(1) | (np.abs(np.abs(b) - gate) < TIE_B)
    sums = np.zeros(NSUMS)
    sums[:32] = terms.sum(0)
    sums[32] = ev.candidates
    lo = np.zeros(NSUMS)
    hi = np.zeros(NSUMS)
    nt = ~tie
    lo[:32] = terms[nt].sum(0) - bounds[nt].sum(0)
    hi[:32] = terms[nt].sum(0) + bounds[nt].sum(0)
    lo[32] = hi[32] = ev.candidates
    ti = np.flatnonzero(tie)
    if len(ti):
        qt, dqt, st = q[ti], dq[ti], sdf[ti]
        alt_lo, alt_hi = terms[ti] - bounds[ti], terms[ti] + bounds[ti]
        shifts = {(0, 0, 0)} | {tuple(s * (((combo >> a) & 1) * 2 - 1) for a in range(3)) for combo in range(8) for s in (1, -1)}
        for shift in sorted(shifts):
            c2 = np.floor(qt + np.array(shift) * TIE_Q * tie_axis[ti]).astype(np.int64)
            _, t2, b2, bres = _cell_terms(dst, qt, c2, st, dqt, gate)
            alt_lo, alt_hi = np.minimum(alt_lo, t2 - b2), np.maximum(alt_hi, t2 + b2)
            on_gate = np.abs(np.abs(bres) - gate) < TIE_B   # either side of the gate: valid, or a miss
            if on_gate.any():
                _, t3, b3, _ = _cell_terms(dst, qt, c2, st, dqt, 1e30)
                g_ = on_gate[:, None]
                alt_lo = np.where(g_, np.minimum(alt_lo, np.minimum(t3 - b3, 0.0)), alt_lo)
                alt_hi = np.where(g_, np.maximum(alt_hi, np.maximum(t3 + b3, 0.0)), alt_hi)
        lo[:32] += alt_lo.sum(0)
        hi[:32] += alt_hi.sum(0)
    ev.sums, ev.lo, ev.hi = sums, lo, hi
    ev.valid, ev.ties = int(sums[28]), int(tie.sum())
    ev.tie_share = ev.ties / max(ev.candidates, 1)
    ev.cost = ev.cost_of(sums, gate)
    return ev


# ---------------------------------------------------------------------------------------------------------------------
# the iteration
# ---------------------------------------------------------------------------------------------------------------------
def pivot(sums):
    """(c, H_c, g_c): the sums re-pivoted to the centroid c = sum q / valid."""
    H = np.zeros((6, 6))
    for col, (k, j) in enumerate(_TRI):
        H[k, j] = H[j, k] = sums[col]
    g = sums[21:27].copy()
    c = sums[29:32] / sums[28] if sums[28] > 0 else np.zeros(3)
    P = np.eye(6)
    P[:3, 3:] = -np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])
    return c, P @ H @ P.T, P @ g


def conditioning(Hc):
    d = np.diag(Hc)
    if not np.all(d > 0):
        return 0.0
    s = 1.0 / np.sqrt(d)
    return float(np.linalg.eigvalsh(Hc * s[:, None] * s[None, :])[0])


def _solve(Hc, gc, lam):
    d = np.diag(Hc)
    use = np.flatnonzero(d > 0)
    y = np.zeros(6)
    if len(use):
        M = Hc[np.ix_(use, use)] + lam * np.diag(d[use])
        y[use] = np.linalg.solve(M, gc[use])
    return y


def _increment(y, c, Xt):
    w = y[:3]
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        a, bq = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, bq = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
    R = np.eye(3) + a * K + bq * (K @ K)
    out = np.empty((3, 4))
    out[:, :3] = R @ Xt[:, :3]
    out[:, 3] = R @ Xt[:, 3] + (c - R @ c + y[3:])
    return out


def register(src, dst, X0, **params):
    """dslam_register_maps on MapData.  X0: 4 x 4 in metres (its entries are taken as float32, as the ABI's).  Returns
    (X 4 x 4 float32 -- X0's own bytes if no step was accepted --, result dict as dslam_register_result plus `trace`:
    one dict per evaluation with cost, valid, tie_share, and for trial evaluations accepted, lam, margin = |cost - the cost
    it was compared with| and cost_slack = the width of the two cost intervals: a decision with margin < cost_slack is a
    tie)."""
    pr = dict(DEFAULTS)
    pr.update({k: v for k, v in params.items() if v})
    X0 = np.asarray(X0, np.float32)
    vs = src.vs
    Xt = voxel_transform(X0.astype(np.float64), vs)
    gate = float(np.float32(pr["residual_gate"]))

    def ev_at(X):
        return evaluate(src, dst, X, pr["band"], gate)

    good = ev_at(Xt)
    trace = [dict(cost=good.cost, valid=good.valid, tie_share=good.tie_share, ev=good)]
    evaluations, stop, accepted_any, lam = 1, -1, False, 1.0
    cost_first = good.cost
    if good.valid < pr["min_valid"]:
        stop = 3
    while stop < 0:
        if evaluations >= pr["max_evaluations"]:
            stop = 1
            break
        c, Hc, gc = pivot(good.sums)
        y = _solve(Hc, gc, lam)
        trial = _increment(y, c, Xt)
        ev = ev_at(trial)
        evaluations += 1
        accept = ev.valid >= pr["min_valid"] and ev.cost < good.cost
        (l1, h1), (l2, h2) = ev.cost_interval(), good.cost_interval()
        trace.append(dict(cost=ev.cost, valid=ev.valid, tie_share=ev.tie_share, ev=ev, accepted=accept, lam=lam,
                          margin=abs(ev.cost - good.cost), cost_slack=(h1 - l1) + (h2 - l2)))
        if accept:
            used = lam
            Xt, good, accepted_any = trial, ev, True
            lam = max(lam / 10.0, 1e-6)
            if (used <= 1.0 and np.linalg.norm(y[:3]) < float(np.float32(pr["term_rotation"]))
                    and np.linalg.norm(y[3:]) < float(np.float32(pr["term_translation_voxels"]))):
                stop = 0
        else:
            lam *= 10.0
            if lam > 1e6:
                stop = 2
    cond = 0.0 if stop == 3 else conditioning(pivot(good.sums)[1])
    X = X0.copy()
    if accepted_any:
        X = np.eye(4, dtype=np.float32)
        X[:3, :3] = Xt[:, :3].astype(np.float32)
        X[:3, 3] = (Xt[:, 3] * vs).astype(np.float32)
    res = dict(evaluations=evaluations, stop_reason=stop, candidates=good.candidates, valid_last=good.valid,
               cost_first=cost_first, cost_last=good.cost, conditioning=cond, trace=trace, last=good)
    return X, res
