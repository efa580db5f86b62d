"""Float64 reference of the depth tracker (ITMDepthTracker::TrackCamera), written from SURVEY.md A.12 -- not from
csrc/track.hip or the oracle.  Plain numpy, the convention of ref64.py: **branch predicates in float32** (the spec's
expression in the spec's operation order, element-wise np.float32), **values in float64**; every predicate also
reports the pixels that sit within a relative 1e-5 (absolute 1e-5 pixel for u, v) of its boundary ("ties").

`evaluate` also returns a first-order float32 rounding bound for each of the 29 sums.  It is derived, not tuned:
eps = 2^-24 is propagated through the operations of A.12 with the magnitudes of the float64 intermediates
(|fl(a op b) - (a op b)| <= eps |a op b|; an input error e_a reaches a product a b as |b| e_a, a quotient a / b as
e_a / |b| + |a| e_b / b^2), per valid pixel, and the per-pixel bounds are added.  The residual b = n . (cp - p) is a
difference of metre-sized numbers, so its bound is of order eps (|cp| + |p|), far above eps |b|.
"""
import math

import numpy as np

F = np.float32
EPS = 2.0 ** -24
TIE = 1e-5
ROTATION, TRANSLATION, BOTH, NONE = 1, 2, 3, 4
N_SUMS = 29


def hessian_slots(npara):
    """(k, j) of the lower-triangle slots, row by row: the layout of the first 21 sums."""
    return [(k, j) for k in range(npara) for j in range(k + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# A.12 FilterSubsampleWithHoles and the per-level parameters
# ---------------------------------------------------------------------------------------------------------------------
def subsample_with_holes(depth):
    """[H, W] -> [H // 2, W // 2]: mean of the pixels > 0 of each 2x2 group, 0 if there is none (an odd last row or
    column is dropped).  Returns (float64 values, float32 values): the float32 image is what the next level and the
    depth <= 1e-8 predicate see."""
    d = np.asarray(depth)
    H, W = d.shape
    nh, nw = H // 2, W // 2
    g = np.stack([d[0:2 * nh:2, 0:2 * nw:2], d[0:2 * nh:2, 1:2 * nw:2], d[1:2 * nh:2, 0:2 * nw:2], d[1:2 * nh:2, 1:2 * nw:2]])
    good = g > 0
    n = good.sum(0)
    s64 = np.where(good, g.astype(np.float64), 0.0).sum(0)
    out64 = np.where(n > 0, s64 / np.maximum(n, 1), 0.0)
    acc = np.zeros((nh, nw), F)
    for k in range(4):  # float32 in the spec's order: (0,0), (1,0), (0,1), (1,1)
        acc = np.where(good[k], acc + g[k].astype(F), acc)
    out32 = np.where(n > 0, acc / np.maximum(n, 1).astype(F), F(0)).astype(F)
    return out64, out32


def pyramid(depth, intr, levels):
    """Per level: (float32 depth image, float32 view intrinsics).  Intrinsics (fx, fy, cx, cy) are halved per level."""
    out = [(np.asarray(depth, F), np.asarray(intr, F))]
    for _ in range(1, levels):
        d, k = out[-1]
        out.append((subsample_with_holes(d)[1], (k * F(0.5)).astype(F)))
    return out


def level_schedule(levels, dist_thresh):
    """(iterations per level, squared-distance threshold per level), float32 as the settings are stored."""
    iters = [2 + 2 * i for i in range(levels)]
    step = F(dist_thresh) / F(levels)
    dist = [F(0)] * levels
    dist[levels - 1] = F(dist_thresh)
    for i in range(levels - 2, -1, -1):
        dist[i] = F(dist[i + 1] - step)
    return iters, dist


# ---------------------------------------------------------------------------------------------------------------------
# one ComputeGandH evaluation
# ---------------------------------------------------------------------------------------------------------------------
def _mul32(M, x, y, z):
    """Matrix4f * (x, y, z, 1) in float32, rows 0..2: ((m0 x + m1 y) + m2 z) + m3 * 1."""
    M = np.asarray(M, F)
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] * F(1) for r in range(3)]


def _corners(img, ix, iy):
    return img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]


def _bilinear32(img, ix, iy, dx, dy):
    a, b, c, d = (t.astype(F) for t in _corners(img, ix, iy))
    one = F(1)
    dx, dy = dx[:, None], dy[:, None]
    return a * (one - dx) * (one - dy) + b * dx * (one - dy) + c * (one - dx) * dy + d * dx * dy


def inverse_error(M):
    """Bound on |fl(inverse) - inverse| per entry when a rigid 4x4 is inverted as A.12 says poses are (Matrix4::inv:
    cofactor expansion, float).  Step by step:
      * a cofactor is six triple products, three added and three subtracted: 2 roundings per product and 5 for the
        sum, so its error is <= 7 eps S, S = the sum of the |triple products|.  With the bottom row (0, 0, 0, 1) only
        two of them are non-zero for a rotation entry, |r_ab r_cd| + |r_ad r_cb| <= 1 (Cauchy-Schwarz on unit rows):
        S <= 1.  For a translation entry each t_k multiplies such a pair: S <= |t|_1;
      * the determinant is sum_i m_i c_i over one row (three non-zero terms, sum |m_i| <= sqrt 3, value 1): the
        cofactors' errors enter as 7 sqrt(3) eps, the products and the sum add 4 eps: <= 16.2 eps, relative;
      * entry = cofactor * (1 / det): two more roundings.  |entry| <= 1 (rotation) or <= |t|_1 (translation), so
        7 eps S + |entry| (16.2 + 2) eps <= 25.2 eps S; 26 eps S is used."""
    M = np.asarray(M, np.float64)
    e = np.zeros((4, 4))
    e[:3, :3] = 26.0 * EPS
    e[:3, 3] = 26.0 * EPS * np.abs(M[:3, 3]).sum()
    return e


def _transform(M, p, e_p, e_M):
    """M p with its float32 rounding bound: a product and up to three additions per term, the input's error e_p and the
    matrix's entry-wise error e_M."""
    out = p @ M[:3, :3].T + M[:3, 3]
    mag = np.abs(p) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])
    e = 4.0 * EPS * mag + e_p @ np.abs(M[:3, :3]).T
    if e_M is not None:
        e = e + np.abs(p) @ e_M[:3, :3].T + e_M[:3, 3]
    return out, e


def _chain(d, x, y, k, Minv, S, si, e_inv):
    """The float64 chain from a pixel to its projection into the scene image, each value with its float32 rounding bound:
    (p, e_p, q, e_q, uv [2], e_uv [2])."""
    pc = np.stack([d * ((x - k[2]) / k[0]), d * ((y - k[3]) / k[1]), d], -1)
    e_pc = np.abs(pc) * np.array([3.0 * EPS, 3.0 * EPS, 0.0])  # subtract, divide, multiply; z is the input itself
    p, e_p = _transform(Minv, pc, e_pc, e_inv)
    q, e_q = _transform(S, p, e_p, None)
    uv, e_uv = [], []
    with np.errstate(all="ignore"):
        for a in (0, 1):
            r = si[a] * q[:, a] / q[:, 2]
            uv.append(r + si[2 + a])
            e_uv.append(EPS * (2.0 * np.abs(r) + np.abs(uv[-1]))
                        + abs(si[a]) * (e_q[:, a] / np.abs(q[:, 2]) + np.abs(q[:, a]) * e_q[:, 2] / q[:, 2] ** 2))
    return p, e_p, q, e_q, uv, e_uv


def _bilinear(img, ix, iy, dx, dy, e_u, e_v):
    """Bilinear interpolant of img's cell (ix, iy) at fractions dx, dy [n, 1] and its bound: 1 - dx, two products, up to
    three additions are 6 roundings on each weighted corner; the fractions' errors enter through the slopes."""
    a, b, c, dd = (t.astype(np.float64) for t in _corners(img, ix, iy))
    val = a * (1 - dx) * (1 - dy) + b * dx * (1 - dy) + c * (1 - dx) * dy + dd * dx * dy
    mag = (np.abs(a) * np.abs((1 - dx) * (1 - dy)) + np.abs(b) * np.abs(dx * (1 - dy)) + np.abs(c) * np.abs((1 - dx) * dy)
           + np.abs(dd) * np.abs(dx * dy))
    du = np.abs((b - a) * (1 - dy) + (dd - c) * dy)
    dv = np.abs((c - a) * (1 - dx) + (dd - b) * dx)
    return val, 6.0 * EPS * mag + du * e_u[:, None] + dv * e_v[:, None]


def evaluate(depth_level, view_intr_level, points, normals, scene_intr, approx_inv_pose, scene_pose, dist_thresh,
             type, inv_err=None, derived_ties=False):
    """One evaluation at one level.  depth_level [h, w] float32; points / normals [H, W, 4] float32 (w < 0: hole);
    approx_inv_pose (camera -> world) and scene_pose (world -> scene camera) 4x4; `inv_err`: entry-wise bound on the
    error of approx_inv_pose as the engine holds it (it inverts in float32).
    Returns dict: sums[29], bound[29], max_term[29], valid [h, w] bool, tie [h, w] bool, projected (pixels that
    reached the distance gate), gated (those it rejected), b / A / p / n / cp per valid pixel (float64), and the numbers
    of pixels that fell behind the scene camera, outside the projection bounds and onto a cell with a hole (one_hole:
    of those, per corner a / b / c / d, the pixels whose cell has that corner as its only hole).
    derived_ties: a predicate's tie window is the larger of the fixed one and the bound this function derives for the
    predicate's operand at that pixel (q.z, u, v, the squared distance) -- for poses far from the origin, where a float32
    projection moves by more than 1e-5 pixel; at the origin's cases the fixed windows stay as they are."""
    depth = np.asarray(depth_level, F)
    h, w = depth.shape
    H, W = points.shape[:2]
    npara = 6 if type == BOTH else 3
    ys, xs = np.mgrid[0:h, 0:w]
    Minv32, S32 = np.asarray(approx_inv_pose, F), np.asarray(scene_pose, F)
    Minv, S = np.asarray(approx_inv_pose, np.float64), np.asarray(scene_pose, np.float64)
    vfx, vfy, vcx, vcy = (F(v) for v in view_intr_level)
    sfx, sfy, scx, scy = (F(v) for v in scene_intr)
    tie = np.zeros((h, w), bool)
    k = [float(v) for v in (vfx, vfy, vcx, vcy)]
    si = [float(v) for v in (sfx, sfy, scx, scy)]
    e_inv = inverse_error(np.linalg.inv(Minv)) if inv_err is None else np.asarray(inv_err, np.float64)
    win = None
    if derived_ties:   # the chain's bounds on every pixel, as images
        _, e_p_all, _, e_q_all, _, e_uv_all = _chain(np.where(depth > F(1e-8), depth, F(1)).astype(np.float64).reshape(-1),
                                                     xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64), k, Minv, S, si, e_inv)
        win = dict(qz=e_q_all[:, 2].reshape(h, w), u=e_uv_all[0].reshape(h, w), v=e_uv_all[1].reshape(h, w), p=e_p_all.reshape(h, w, 3))

    ok = depth > F(1e-8)
    tie |= np.abs(depth.astype(np.float64) - 1e-8) <= TIE * 1e-8
    d32 = np.where(ok, depth, F(1))
    with np.errstate(all="ignore"):
        # ---- float32 chain: decides every branch ------------------------------------------------------------------
        cx32 = d32 * ((xs.astype(F) - vcx) / vfx)
        cy32 = d32 * ((ys.astype(F) - vcy) / vfy)
        p32 = _mul32(Minv32, cx32, cy32, d32)
        q32 = _mul32(S32, *p32)
        front = q32[2] > F(0)
        qscale = np.abs(S[2, :3]) @ np.abs(np.stack([t.astype(np.float64) for t in p32]).reshape(3, -1)) + abs(S[2, 3])
        tie |= ok & (np.abs(q32[2].astype(np.float64)) <= TIE * qscale.reshape(h, w))
        if win is not None:
            tie |= ok & (np.abs(q32[2].astype(np.float64)) <= win["qz"])
        n_behind = int((ok & ~front).sum())
        ok &= front
        qz = np.where(ok, q32[2], F(1))
        u32 = sfx * q32[0] / qz + scx
        v32 = sfy * q32[1] / qz + scy
        inside = (u32 >= F(0)) & (u32 <= F(W - 2)) & (v32 >= F(0)) & (v32 <= F(H - 2))
        for t, hi, axis in ((u32, W - 2, "u"), (v32, H - 2, "v")):
            t64 = t.astype(np.float64)
            e_t = TIE if win is None else np.maximum(TIE, win[axis])
            tie |= ok & ((np.abs(t64) <= e_t) | (np.abs(t64 - hi) <= e_t))
            tie |= ok & inside & (np.abs(t64 - np.round(t64)) <= e_t)  # the cell (and its hole test) could change
        n_outside = int((ok & ~inside).sum())
        # pixels only q.z <= 0 rejects: behind the scene camera, yet projecting inside the bounds onto a cell without holes
        bi = np.nonzero((depth > F(1e-8)) & ~front & (q32[2] < F(0)))
        ub, vb = sfx * q32[0][bi] / q32[2][bi] + scx, sfy * q32[1][bi] / q32[2][bi] + scy
        kb = (ub >= F(0)) & (ub <= F(W - 2)) & (vb >= F(0)) & (vb <= F(H - 2))
        ixb, iyb = np.floor(ub[kb]).astype(np.int64), np.floor(vb[kb]).astype(np.int64)
        pw = np.asarray(points)[..., 3]
        n_behind_inside = int(((pw[iyb, ixb] >= 0) & (pw[iyb, ixb + 1] >= 0) & (pw[iyb + 1, ixb] >= 0) & (pw[iyb + 1, ixb + 1] >= 0)).sum())
        ok &= inside
    idx = np.nonzero(ok)
    u32, v32 = u32[idx], v32[idx]
    ix, iy = np.floor(u32).astype(np.int64), np.floor(v32).astype(np.int64)
    pts, nrm = np.asarray(points), np.asarray(normals)
    hole = np.zeros(len(ix), bool)
    for c in _corners(pts[..., 3], ix, iy):
        hole |= c < 0
    wneg = np.stack([c < 0 for c in _corners(pts[..., 3], ix, iy)])
    # pixels inside the bounds whose cell has exactly one hole, per corner (a, b, c, d): where the four-corner rule decides
    one_hole = [int((wneg[k] & (wneg.sum(0) == 1)).sum()) for k in range(4)]
    keep = ~hole
    idx = tuple(t[keep] for t in idx)
    u32, v32, ix, iy = u32[keep], v32[keep], ix[keep], iy[keep]
    dx32, dy32 = u32 - ix.astype(F), v32 - iy.astype(F)
    cp32 = _bilinear32(pts[..., :3], ix, iy, dx32, dy32)
    pw32 = np.stack([t[idx] for t in p32], -1)
    dd32 = cp32 - pw32
    dist32 = dd32[:, 0] * dd32[:, 0] + dd32[:, 1] * dd32[:, 1] + dd32[:, 2] * dd32[:, 2]
    thr = F(dist_thresh)
    gate = dist32 > thr
    t_gate = np.abs(dist32.astype(np.float64) - float(thr)) <= TIE * float(thr)
    if win is not None:   # the squared distance's own bound: cp from the cell the float32 chain chose, p, their difference
        e_u, e_v = win["u"][idx], win["v"][idx]
        cp_g, e_cp_g = _bilinear(pts[..., :3], ix, iy, (u32.astype(np.float64) - ix)[:, None], (v32.astype(np.float64) - iy)[:, None], e_u, e_v)
        dd_g = cp32.astype(np.float64) - pw32.astype(np.float64)
        e_dd_g = e_cp_g + win["p"][idx] + EPS * np.abs(dd_g)
        e_dist = np.sum(2.0 * np.abs(dd_g) * e_dd_g, -1) + 5.0 * EPS * dist32.astype(np.float64)
        t_gate |= np.abs(dist32.astype(np.float64) - float(thr)) <= e_dist
    tie[tuple(t[t_gate] for t in idx)] = True
    projected = np.zeros((h, w), bool)
    projected[idx] = True
    gated = np.zeros((h, w), bool)
    gated[tuple(t[gate] for t in idx)] = True
    keep = ~gate
    idx = tuple(t[keep] for t in idx)
    ix, iy = ix[keep], iy[keep]
    valid = np.zeros((h, w), bool)
    valid[idx] = True

    # ---- float64 chain on the valid pixels, each value with its float32 rounding bound ----------------------------
    d = depth[idx].astype(np.float64)
    x, y = xs[idx].astype(np.float64), ys[idx].astype(np.float64)
    p, e_p, q, e_q, uv, e_uv = _chain(d, x, y, k, Minv, S, si, e_inv)
    dx, dy = (uv[0] - ix)[:, None], (uv[1] - iy)[:, None]

    def bilinear(img):
        return _bilinear(img, ix, iy, dx, dy, e_uv[0], e_uv[1])

    cp, e_cp = bilinear(pts[..., :3])
    n, e_n = bilinear(nrm[..., :3])
    dd = cp - p
    e_dd = e_cp + e_p + EPS * np.abs(dd)
    b = np.sum(n * dd, -1)
    e_b = np.sum(np.abs(n) * e_dd + np.abs(dd) * e_n, -1) + 3.0 * EPS * np.sum(np.abs(n * dd), -1)

    def rot_row(i, j):  # p_i n_j - p_j n_i: two products and a difference
        e = (np.abs(n[:, j]) * e_p[:, i] + np.abs(p[:, i]) * e_n[:, j] + np.abs(n[:, i]) * e_p[:, j] + np.abs(p[:, j]) * e_n[:, i]
             + 2.0 * EPS * (np.abs(p[:, i] * n[:, j]) + np.abs(p[:, j] * n[:, i])))
        return p[:, i] * n[:, j] - p[:, j] * n[:, i], e

    # r0 = +p.z n.y - p.y n.z;  r1 = -p.z n.x + p.x n.z;  r2 = +p.y n.x - p.x n.y
    rot = [rot_row(2, 1), rot_row(0, 2), rot_row(1, 0)]
    tra = [(n[:, c], e_n[:, c]) for c in range(3)]
    cols = rot if type == ROTATION else tra if type == TRANSLATION else rot + tra
    A = np.stack([c[0] for c in cols], -1)
    e_A = np.stack([c[1] for c in cols], -1)

    sums, bound, max_term = np.zeros(N_SUMS), np.zeros(N_SUMS), np.zeros(N_SUMS)

    def put(slot, term, e_term):
        sums[slot] = math.fsum(term)
        absum = math.fsum(np.abs(term))
        bound[slot] = math.fsum(e_term) + EPS * absum + 2.0 ** -50 * absum  # the product's rounding; double accumulation
        max_term[slot] = np.abs(term).max() if len(term) else 0.0

    for slot, (kk, jj) in enumerate(hessian_slots(npara)):
        put(slot, A[:, kk] * A[:, jj], np.abs(A[:, kk]) * e_A[:, jj] + np.abs(A[:, jj]) * e_A[:, kk])
    for kk in range(npara):
        put(21 + kk, b * A[:, kk], np.abs(A[:, kk]) * e_b + np.abs(b) * e_A[:, kk])
    put(27, b * b, 2.0 * np.abs(b) * e_b)
    sums[28] = float(len(b))
    max_term[28] = 1.0
    return dict(sums=sums, bound=bound, max_term=max_term, valid=valid, tie=tie, projected=projected, gated=gated,
                b=b, A=A, p=p, n=n, cp=cp, idx=idx, behind=n_behind, outside=n_outside, holes=int(hole.sum()),
                one_hole=one_hole, behind_inside=n_behind_inside)


def error_interval(sum_bb, bound_bb, max_bb, valid, ties):
    """[lo, hi] for the float f = sqrtf((float) sum) / (float) valid when the sum is within bound_bb + ties * max_bb of
    sum_bb and the count within `ties` of valid (needs valid - ties > 100); three float roundings (conversion,
    square root, division) on top."""
    lim = bound_bb + max_bb * ties
    hi = math.sqrt(sum_bb + lim) / (valid - ties)
    lo = math.sqrt(max(sum_bb - lim, 0.0)) / (valid + ties)
    return lo - 3.0 * EPS * hi, hi + 3.0 * EPS * hi


def error_value(sum_bb, valid):
    """f = sqrt(sum b^2) / valid, or 1e5 when valid <= 100."""
    return math.sqrt(sum_bb) / valid if valid > 100 else 1e5


# ---------------------------------------------------------------------------------------------------------------------
# the host side: ApplyDelta, SetInvM + Coerce, the Levenberg-Marquardt loop
# ---------------------------------------------------------------------------------------------------------------------
def tinc(delta, type):
    """ApplyDelta's increment: I - [r]x with translation t, r = step[0:3], t = step[3:6]."""
    s = np.zeros(6)
    if type == ROTATION:
        s[:3] = delta[:3]
    elif type == TRANSLATION:
        s[3:] = delta[:3]
    else:
        s[:] = delta[:6]
    T = np.eye(4)
    T[0, 1], T[0, 2], T[0, 3] = s[2], -s[1], s[3]
    T[1, 0], T[1, 2], T[1, 3] = -s[2], s[0], s[4]
    T[2, 0], T[2, 1], T[2, 3] = s[1], -s[0], s[5]
    return T


def coerce(M):
    """Gram-Schmidt on the rotation's columns (first kept, second made orthogonal, third their cross product),
    bottom row (0, 0, 0, 1): the stand-in for upstream's parameter round trip."""
    M = np.array(M, np.float64)
    c0 = M[:3, 0] / np.linalg.norm(M[:3, 0])
    c1 = M[:3, 1] - (c0 @ M[:3, 1]) * c0
    c1 /= np.linalg.norm(c1)
    M[:3, 0], M[:3, 1], M[:3, 2] = c0, c1, np.cross(c0, c1)
    M[3] = (0.0, 0.0, 0.0, 1.0)
    return M


def apply_step(approx_inv_pose, delta, type):
    """approxInvPose' = Tinc * approxInvPose; pose = Coerce(inverse); returns (pose M, its inverse)."""
    M = coerce(np.linalg.inv(tinc(delta, type) @ approx_inv_pose))
    return M, np.linalg.inv(M)


def _full(sums, npara):
    Hm = np.zeros((npara, npara))
    for slot, (k, j) in enumerate(hessian_slots(npara)):
        Hm[k, j] = Hm[j, k] = sums[slot]
    return Hm, sums[21:21 + npara].copy()


def track(depth, intr, points, normals, scene_pose, pose, levels=5, run_till_level=0, dist_thresh=0.01,
          termination_threshold=1e-3, regime=(3, 3, 1, 1, 1), derived_ties=False):
    """The whole coarse-to-fine loop in float64.  Returns (pose M, list of per-iteration records).  derived_ties: evaluate's."""
    pyr = pyramid(depth, intr, levels)
    iters, dist = level_schedule(levels, dist_thresh)
    regime = (list(regime) + [NONE] * 8)[:8]
    M = np.asarray(pose, np.float64).copy()
    log = []
    H_good, g_good = np.zeros((6, 6)), np.zeros(6)  # one pair for the whole call (A.12): a level starts with the last level's
    for level in range(levels - 1, run_till_level - 1, -1):
        type = regime[level]
        if type == NONE:
            continue
        npara = 6 if type == BOTH else 3
        inv = np.linalg.inv(M)
        good_M, f_old, lam = M.copy(), 1e20, 1.0
        for _ in range(iters[level]):
            ev = evaluate(pyr[level][0], pyr[level][1], points, normals, pyr[0][1], inv, scene_pose, dist[level], type,
                          inv_err=None, derived_ties=derived_ties)
            valid = int(ev["sums"][28])
            f_new = error_value(ev["sums"][27], valid)
            rejected = valid <= 0 or f_new > f_old
            # (two evaluations with valid <= 100 both give the constant 1e5: equal, accepted, and no tie)
            accept_tie = valid > 0 and f_old < 1e19 and abs(f_new - f_old) <= 1e-5 * f_old and not (f_new == f_old == 1e5)
            if rejected:
                M = good_M.copy()
                inv = np.linalg.inv(M)
                lam *= 10.0
            else:
                good_M, f_old = M.copy(), f_new
                Hm, g = _full(ev["sums"], npara)
                H_good[:], g_good[:] = 0.0, 0.0
                H_good[:npara, :npara], g_good[:npara] = Hm / valid, g / valid
                lam /= 10.0
            A = H_good[:npara, :npara].copy()
            A[np.diag_indices(npara)] *= 1.0 + lam
            try:
                step = np.linalg.solve(A, g_good[:npara])
            except np.linalg.LinAlgError:
                step = np.zeros(npara)
            M, inv = apply_step(inv, step, type)
            log.append(dict(level=level, type=type, valid=valid, f=f_new, accepted=not rejected, accept_tie=accept_tie,
                            lam=lam, step=step, pose=M.copy(), ties=int(ev["tie"].sum()), sum_bb=ev["sums"][27],
                            bound_bb=ev["bound"][27], max_bb=ev["max_term"][27],
                            p_max=float(np.abs(ev["p"]).max()) if valid else 0.0))
            if math.sqrt(float(step @ step)) / 6.0 < termination_threshold:
                break
    return M, log
