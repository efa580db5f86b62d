"""Float64 statement of dslam_track_camera_sdf_rgb: dslam_track_camera_sdf's evaluation
(ref64_track_sdf.py, whose map read, camera points, pivot and iteration are imported and not restated) with the
photometric term, in numpy.  Shares no text with the engine.

On a level that carries the term, per pixel besides section 18's:
  image   I = G_l[x, y]; the greys G_l are taken in float32 exactly as the law states them, because they are inputs:
          G_0 = ((0.299f R + 0.587f G) + 0.114f B) * (float)(1 / 255), G_k the 2 x 2 mean ((a + b) + (c + d)) * 0.25f;
  map     per map that passed its 8-tap gate: colour-ok iff all 8 taps have w_color > 0; the tap grey y_k is G_0's expression
          on the tap's clr bytes (the four constants are their float32 values); C_i, h_i the trilinear interpolant of y and
          its analytic gradient; w^c_i the trilinear interpolant of the taps' w_color; h_i^w = R_i^T h_i;
  blend   no colour-ok map: a colour miss; one: its C, h; several: C = sum w^c C / sum w^c, h alike;
  gate    e = C - I; a colour miss for a depth miss or |e| > colour_gate;
  rows    b_c = -(k e), A_c = k [r x h, h]; sums [0..26] hold depth and colour rows together, [33] sum e^2 over the
          colour-valid pixels, [34] colour-valid;
  cost    cost_depth + k^2 cost_colour, cost_colour = (sum e^2 + (N - colour_valid) colour_gate^2) / N.

What the engine may differ by: everything from the taps on is float32 there (u = 2^-24 per operation).  The first-order
bound of ref64_track_sdf.py is extended over
  a tap grey         dy = 4 u y (a product, two additions and a product on the longest path; every term is positive);
  the colour lerp    with M, D, H2 of the greys as section 18's of the sdf taps: dC = sum_axis |h_axis| dc' + 10 u M + 4 u M
                     (the interpolant is a convex combination of the taps, so their own error enters once) and
                     dh = 16 u M + 8 u D + 2 H2 max dc' + 8 u M (every gradient term is a difference of two taps);
  the colour weight  dw as section 18's with the taps' w_color;
  the rotation back and the blend: section 18's expressions on h and w^c;
  the residual       de = dC + u |e| (I is exact);
  the scaling by k   d(k v) = k dv + u |k v| for b_c and each of the six entries of [r x h, h] (whose own bound is section
                     18's row bound with h in place of g);
  the products       |x| dy + |y| dx + u |x y|; e^2: 2 |e| de + u e^2.
They are added over the pixels and to the depth term's bounds (no cancellation assumed).

Ties.  Section 18's cell ties apply to the colour read as well (the alternatives are evaluated for both terms together);
| |d| - gate | < TIE_B may fall either side of the depth gate (a miss there is a colour miss too), | |e| - colour_gate | <
TIE_E either side of the colour gate.
"""
import numpy as np

import ref64_track_sdf as rt

U = rt.U
TIE_E = 1e-5
NSUMS = 35
F = np.float32
C_R, C_G, C_B, INV255 = float(F(0.299)), float(F(0.587)), float(F(0.114)), float(F(1.0 / 255.0))

DEFAULTS = dict(colour_weight=1.0, colour_gate=0.25, colour_levels=1)
LAWS = ("law", "w_depth", "tap0", "unrotated", "sign", "swap_br")   # the law, and the wrong laws the tests tell apart


# ---------------------------------------------------------------------------------------------------------------------
# image side (float32, as stated)
# ---------------------------------------------------------------------------------------------------------------------
def grey_level0(rgba):
    c = np.asarray(rgba, np.uint8).astype(F)
    return (((F(0.299) * c[..., 0] + F(0.587) * c[..., 1]) + F(0.114) * c[..., 2]) * F(1.0 / 255.0)).astype(F)


def grey_subsample(g):
    h, w = g.shape[0] // 2, g.shape[1] // 2
    g = np.asarray(g, F)[:2 * h, :2 * w]
    return (((g[0::2, 0::2] + g[0::2, 1::2]) + (g[1::2, 0::2] + g[1::2, 1::2])) * F(0.25)).astype(F)


def grey_pyramid(rgba, levels):
    out = [grey_level0(rgba)]
    for _ in range(1, levels):
        out.append(grey_subsample(out[-1]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# map side
# ---------------------------------------------------------------------------------------------------------------------
def colour_at(data, v):
    """(clr int64 [..., 3], w_color int64, w_depth int64) of integer voxel positions v [..., 3] of a MapData; zeros where the
    block is not resident."""
    v = np.asarray(v, np.int64)
    b = v >> 3
    inside = np.all((b >= -32768) & (b <= 32767), axis=-1)
    keys = data._key(np.where(inside[..., None], b, 0))
    if len(data._keys) == 0:
        z = np.zeros(keys.shape, np.int64)
        return np.zeros(keys.shape + (3,), np.int64), z, z
    i = np.minimum(np.searchsorted(data._keys, keys), len(data._keys) - 1)
    found = inside & (data._keys[i] == keys)
    ptr = np.where(found, data._ptr_sorted[i], 0)
    loc = (v[..., 0] & 7) | ((v[..., 1] & 7) << 3) | ((v[..., 2] & 7) << 6)
    vox = data.vba[ptr, loc]
    return (np.where(found[..., None], vox["clr"].astype(np.int64), 0), np.where(found, vox["w_color"].astype(np.int64), 0),
            np.where(found, vox["w_depth"].astype(np.int64), 0))


def _max_diffs(v):
    D = np.max(np.stack([np.abs(v[:, j] - v[:, i]) for i, j in rt._EDGES], 1), 1)
    H2 = np.max(np.stack([np.abs((v[:, f[3]] - v[:, f[2]]) - (v[:, f[1]] - v[:, f[0]])) for f in rt._FACES], 1), 1)
    return D, H2


def read_colour(pm, q, cell, dq, law="law"):
    """One map's colour read of points q [n, 3] in `cell`: (colour-ok, C, h (map frame), w^c, dC, dh, dw)."""
    clr, wc, wd = colour_at(pm.data, cell[:, None, :] + rt._OFFS[None])
    cok = np.all(wc > 0, axis=1)
    R, G, B = (clr[..., k].astype(np.float64) for k in ((2, 1, 0) if law == "swap_br" else (0, 1, 2)))
    y = ((C_R * R + C_G * G) + C_B * B) * INV255
    c = q - cell
    C, h = rt._lerp3(y, c)
    wf = (wd if law == "w_depth" else wc).astype(np.float64)
    om = wf[:, 0] if law == "tap0" else rt._lerp3(wf, c)[0]
    dc = dq + 2 * U
    M = np.abs(y).max(1)
    D, H2 = _max_diffs(y)
    dC = (np.abs(h) * dc).sum(1) + 14 * U * M
    dh = 24 * U * M + 8 * U * D + 2 * H2 * dc.max(1)
    Dw, _ = _max_diffs(wf)
    dw = 3 * Dw * dc.max(1) + 10 * U * wf.max(1)
    return cok, C, h, om, dC, dh, dw


def _blend(items, n):
    """Section 18's blend (value [n], vector [n, 3]) with its bound, over items (use, v, dv, vec, dvec, w, dw) in list order:
    (count, v, dv, vec, dvec)."""
    k = np.zeros(n, np.int64)
    num, den, absn, e_num, e_den = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    num3, abs3, e_num3 = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    f_v, f_dv, f_vec, f_dvec = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    for use, v, dv, vec, dvec, w, dw in items:
        first = use & (k == 0)
        f_v, f_dv = np.where(first, v, f_v), np.where(first, dv, f_dv)
        f_vec, f_dvec = np.where(first[:, None], vec, f_vec), np.where(first[:, None], dvec, f_dvec)
        o = use.astype(np.float64)
        num += o * w * v
        absn += o * np.abs(w * v)
        e_num += o * (w * dv + np.abs(v) * dw + U * np.abs(w * v))
        den += o * w
        e_den += o * dw
        num3 += o[:, None] * w[:, None] * vec
        abs3 += o[:, None] * np.abs(w[:, None] * vec)
        e_num3 += o[:, None] * (w[:, None] * dvec + np.abs(vec) * dw[:, None] + U * np.abs(w[:, None] * vec))
        k += use
    multi = k >= 2
    dn = np.where(multi, den, 1.0)
    km1 = np.maximum(k - 1, 0)
    e_dn = e_den + km1 * U * den
    v_bl = num / dn
    dv_bl = (e_num + km1 * U * absn) / dn + np.abs(num) * e_dn / dn ** 2 + U * np.abs(v_bl)
    vec_bl = num3 / dn[:, None]
    dvec_bl = (e_num3 + km1[:, None] * U * abs3) / dn[:, None] + np.abs(num3) * (e_dn / dn ** 2)[:, None] + U * np.abs(vec_bl)
    return (k, np.where(multi, v_bl, f_v), np.where(multi, dv_bl, f_dv), np.where(multi[:, None], vec_bl, f_vec),
            np.where(multi[:, None], dvec_bl, f_dvec))


def colour_field(maps, qs, dqs, cells, law="law"):
    """The blended colour field at the pixels' points: (colour-ok maps per pixel, C, dC, h (world), dh)."""
    n = len(qs[0])
    items = []
    for pm, q, dq, cell in zip(maps, qs, dqs, cells):
        ok = rt.read_map(pm, q, cell, dq)[0]
        cok, C, h, om, dC, dh, dw = read_colour(pm, q, cell, dq, law)
        if pm.identity or law == "unrotated":
            hw, dhw = h, np.repeat(dh[:, None], 3, 1)
        else:
            R = pm.Tt[:, :3]
            hw = h @ R                                                  # R^T h
            dhw = dh[:, None] * np.abs(R).sum(0)[None] + 3 * U * (np.abs(h) @ np.abs(R))
        items.append((ok & cok, C, dC, hw, dhw, om, dw))
    return _blend(items, n)


def _terms(maps, qs, dqs, cells, r, dr, I, gate, cgate, kw, law):
    """Per pixel: (valid, terms [n, 34], bounds [n, 34], d, e, colour-valid).  Columns 0..31 are section 18's with the colour
    rows added into 0..26; column 32 is e^2 and column 33 the colour-valid flag.  I None: a level without the term."""
    valid, t18, b18, d, _ = rt._pixel_terms(maps, qs, dqs, cells, r, dr, gate)
    n = len(r)
    terms, bounds = np.zeros((n, 34)), np.zeros((n, 34))
    terms[:, :32], bounds[:, :32] = t18, b18
    if I is None:
        return valid, terms, bounds, d, np.full(n, np.inf), np.zeros(n, bool)
    k, C, dC, h, dh = colour_field(maps, qs, dqs, cells, law)
    e = C - I
    de = dC + U * np.abs(e)
    cv = valid & (k > 0) & ~(np.abs(e) > cgate)
    b = (kw * e) if law == "sign" else -(kw * e)
    db = kw * de + U * np.abs(b)
    X = np.concatenate([np.cross(r, h), h], 1)
    dX = np.empty((n, 6))
    for i, (j, l) in enumerate(((1, 2), (2, 0), (0, 1))):   # X_i = r_j h_l - r_l h_j
        dX[:, i] = (np.abs(r[:, j]) * dh[:, l] + np.abs(h[:, l]) * dr[:, j] + 2 * U * np.abs(r[:, j] * h[:, l])
                    + np.abs(r[:, l]) * dh[:, j] + np.abs(h[:, j]) * dr[:, l] + 2 * U * np.abs(r[:, l] * h[:, j]))
    dX[:, 3:] = dh
    A = kw * X
    dA = kw * dX + U * np.abs(A)
    ct, cb = np.zeros((n, 34)), np.zeros((n, 34))
    for col, (rr, cc) in enumerate(rt._TRI):
        ct[:, col] = A[:, rr] * A[:, cc]
        cb[:, col] = np.abs(A[:, rr]) * dA[:, cc] + np.abs(A[:, cc]) * dA[:, rr] + U * np.abs(ct[:, col])
    for rr in range(6):
        ct[:, 21 + rr] = b * A[:, rr]
        cb[:, 21 + rr] = np.abs(b) * dA[:, rr] + np.abs(A[:, rr]) * db + U * np.abs(ct[:, 21 + rr])
    ct[:, 32] = e * e
    cb[:, 32] = 2 * np.abs(e) * de + U * ct[:, 32]
    ct[:, 33] = 1.0
    ct[~cv] = 0.0
    cb[~cv] = 0.0
    return valid, terms + ct, bounds + cb, d, np.where(valid & (k > 0), e, np.inf), cv


# ---------------------------------------------------------------------------------------------------------------------
# one evaluation
# ---------------------------------------------------------------------------------------------------------------------
class Evaluation(rt.Evaluation):
    """sums [35]; lo / hi [35]; candidates, valid, colour_valid, ties; term: whether the level carries the photometric term."""

    def costs_of(self, sums):
        """(cost_depth, cost_colour) of 35 sums."""
        n, g2, c2 = sums[32], self.gate * self.gate, self.cgate * self.cgate
        if n <= 0:
            return g2, (c2 if self.term else 0.0)
        return (sums[27] + (n - sums[28]) * g2) / n, ((sums[33] + (n - sums[34]) * c2) / n if self.term else 0.0)

    def cost_of(self, sums, gate=None):
        cd, cc = self.costs_of(sums)
        return cd + self.kw * self.kw * cc

    def cost_interval(self):
        n, g2, c2, k2 = self.sums[32], self.gate * self.gate, self.cgate * self.cgate, self.kw * self.kw
        if n <= 0:
            c = self.cost_of(self.sums)
            return c, c
        lo = (self.lo[27] + (n - self.hi[28]) * g2) / n
        hi = (self.hi[27] + (n - self.lo[28]) * g2) / n
        if self.term:
            lo += k2 * (self.lo[33] + (n - self.hi[34]) * c2) / n
            hi += k2 * (self.hi[33] + (n - self.lo[34]) * c2) / n
        return lo * (1 - 2 * U), hi * (1 + 2 * U)   # (the result is handed out as a float32)

    def check_sums(self, got, what=""):
        """Assert an engine's 35 sums lie in the interval; returns the largest share of the bound they use."""
        got = np.asarray(got, np.float64)
        assert got[32] == self.sums[32], f"{what}: {got[32]:.0f} candidates, reference {self.sums[32]:.0f}"
        assert abs(got[28] - self.sums[28]) <= self.ties, f"{what}: valid {got[28]:.0f}, reference {self.sums[28]:.0f}, {self.ties} ties"
        assert abs(got[34] - self.sums[34]) <= self.ties, (f"{what}: colour-valid {got[34]:.0f}, reference {self.sums[34]:.0f}, "
                                                           f"{self.ties} ties")
        return self.share_used(got, what)

    def outside(self, got):
        """The sums of `got` that lie outside the interval."""
        got = np.asarray(got, np.float64)
        slack = 1e-12 * np.maximum(np.abs(self.lo), np.abs(self.hi))   # the double accumulation itself
        return np.flatnonzero((got < self.lo - slack) | (got > self.hi + slack))

    def share_used(self, got, what=""):
        got = np.asarray(got, np.float64)
        bad = self.outside(got)
        assert len(bad) == 0, (f"{what}: sums {bad.tolist()} outside the bound: got {got[bad]}, reference {self.sums[bad]}, "
                               f"interval [{self.lo[bad]}, {self.hi[bad]}]")
        with np.errstate(divide="ignore", invalid="ignore"):
            used = np.nanmax(np.where(self.hi > self.lo, np.abs(got - self.sums) / (0.5 * (self.hi - self.lo)), 0.0))
        return float(used)


def _to_sums(cols, n_cand):
    s = np.zeros(NSUMS)
    s[:32], s[32], s[33], s[34] = cols[:32], n_cand, cols[32], cols[33]
    return s


def evaluate(maps, depth, grey, intr, Pt, gate=0.75, colour_weight=1.0, colour_gate=0.25, law="law"):
    """One evaluation of one pyramid level (float32 depth image [h, w], the float32 grey image of that level or None for a
    level without the term, the level's float32 intrinsics) at Pt [3, 4]."""
    gate, cgate, kw = float(F(gate)), float(F(colour_gate)), float(F(colour_weight))
    vs = maps[0].data.vs
    cand, r, dr, p, dp = rt.camera_points(depth, intr, Pt, vs)
    I = None if grey is None else np.asarray(grey, F).reshape(-1)[cand].astype(np.float64)
    assert grey is None or np.asarray(grey).shape == np.asarray(depth).shape
    ev = Evaluation()
    ev.gate, ev.cgate, ev.kw, ev.term, ev.candidates = gate, cgate, kw, grey is not None, len(cand)
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
        windows.append(np.maximum(rt.TIE_Q, dq))
        tie_axes.append(np.minimum(frac, 1 - frac) < windows[-1])
    valid, terms, bounds, d, e, cv = _terms(maps, qs, dqs, cells, r, dr, I, gate, cgate, kw, law)
    if len(cand):
        tie = (np.any([t.any(1) for t in tie_axes], axis=0) | (np.abs(np.abs(d) - gate) < rt.TIE_B)
               | (np.abs(np.abs(e) - cgate) < TIE_E))
    else:
        tie = np.zeros(0, bool)
    nt = ~tie
    c_lo, c_hi = terms[nt].sum(0) - bounds[nt].sum(0), terms[nt].sum(0) + bounds[nt].sum(0)
    ti = np.flatnonzero(tie)
    if len(ti):
        alt_lo, alt_hi = terms[ti] - bounds[ti], terms[ti] + bounds[ti]
        sub_q, sub_dq = [q[ti] for q in qs], [dq[ti] for dq in dqs]
        sub_win = [w[ti] * a[ti] for w, a in zip(windows, tie_axes)]
        sub_I = None if I is None else I[ti]
        shifts = {(0, 0, 0)} | {tuple(s * (((combo >> a) & 1) * 2 - 1) for a in range(3)) for combo in range(8) for s in (1, -1)}
        movers = [list(range(len(maps)))] + ([[i] for i in range(len(maps))] if len(maps) > 1 else [])
        for moved in movers:
            for shift in sorted(shifts):
                c2 = [np.floor(sub_q[i] + (np.array(shift) * sub_win[i] if i in moved else 0.0)).astype(np.int64)
                      for i in range(len(maps))]

                def alt(g_, cg_):
                    return _terms(maps, sub_q, sub_dq, c2, r[ti], dr[ti], sub_I, g_, cg_, kw, law)
                _, t2, b2, d2, _, _ = alt(gate, cgate)
                alt_lo, alt_hi = np.minimum(alt_lo, t2 - b2), np.maximum(alt_hi, t2 + b2)
                _, _, _, _, e2, _ = alt(1e30, cgate)   # (e wherever a map holds colour, whatever the depth gate says)
                on_d = np.abs(np.abs(d2) - gate) < rt.TIE_B
                on_e = np.abs(np.abs(e2) - cgate) < TIE_E
                # either side of either gate: depth valid or a miss (then a colour miss too), colour valid or a colour miss
                variants = []
                if on_d.any():
                    variants += [(on_d, 1e30, cgate, True)]
                if on_e.any():
                    variants += [(on_e, gate, 1e30, False), (on_e, gate, -1.0, False)]
                if (on_d & on_e).any():
                    variants += [(on_d & on_e, 1e30, 1e30, True), (on_d & on_e, 1e30, -1.0, True)]
                for mask, g_, cg_, or_miss in variants:
                    _, t3, b3, _, _, _ = alt(g_, cg_)
                    l3, h3 = t3 - b3, t3 + b3
                    if or_miss:
                        l3, h3 = np.minimum(l3, 0.0), np.maximum(h3, 0.0)
                    m_ = mask[:, None]
                    alt_lo = np.where(m_, np.minimum(alt_lo, l3), alt_lo)
                    alt_hi = np.where(m_, np.maximum(alt_hi, h3), alt_hi)
        c_lo, c_hi = c_lo + alt_lo.sum(0), c_hi + alt_hi.sum(0)
    ev.sums, ev.lo, ev.hi = _to_sums(terms.sum(0), len(cand)), _to_sums(c_lo, len(cand)), _to_sums(c_hi, len(cand))
    ev.tie, ev.t = tie, rt._r32(Pt)[:, 3]
    ev.valid, ev.colour_valid, ev.ties = int(ev.sums[28]), int(ev.sums[34]), int(tie.sum())
    ev.tie_share = ev.ties / max(ev.candidates, 1)
    ev.cost_depth, ev.cost_colour = ev.costs_of(ev.sums)
    ev.cost = ev.cost_of(ev.sums)
    ev.d, ev.e, ev.pixels = d, e, cand
    return ev


# ---------------------------------------------------------------------------------------------------------------------
# the iteration: ref64_track_sdf.track's, on this file's evaluation
# ---------------------------------------------------------------------------------------------------------------------
def track(maps, depth0, rgba, intr, pose_M, colour_weight=0.0, colour_gate=0.0, colour_levels=0, law="law", **params):
    """dslam_track_camera_sdf_rgb on PosedMaps: (pose 4 x 4 float32, result dict as ref64_track_sdf.track's with the
    dslam_track_sdf_rgb_result fields added).  rgba: the view's colour image [h, w, 4] uint8, of the depth image's size."""
    kw, cgate, clev = (colour_weight or DEFAULTS["colour_weight"], colour_gate or DEFAULTS["colour_gate"],
                       colour_levels or DEFAULTS["colour_levels"])
    levels = params.get("no_hierarchy_levels") or rt.DEFAULTS["no_hierarchy_levels"]
    till = params.get("run_till_level") or 0
    greys = grey_pyramid(rgba, levels)
    level_of = {g.shape: l for l, g in enumerate(greys)}

    def evaluator(maps_, depth, k, Pt, gate):
        level = level_of[np.asarray(depth).shape]
        return evaluate(maps_, depth, greys[level] if level - till < clev else None, k, Pt, gate, kw, cgate, law)

    M, res = rt.track(maps, depth0, intr, pose_M, evaluator=evaluator, **params)
    last = res["last"]
    res.update(colour_valid_last=last.colour_valid, cost_depth_last=last.cost_depth, cost_colour_last=last.cost_colour,
               colour_rms_last=float(np.sqrt(last.sums[33] / last.colour_valid)) if last.colour_valid else 0.0)
    return M, res
