"""Float64 references of the hot-path operations, written from SURVEY.md Appendix A and upstream InfiniTAM v2 semantics.

Vectorised numpy, no compiled code.  The rule every function follows:
  * a threshold predicate (an image bound, a nearest-pixel rounding, the depth cut eta >= -mu, the colour gate, the
    weight law's rounding, the bounding-box floor / ceil) is evaluated with the spec's float32 expression in the spec's
    operation order, element-wise in np.float32 (numpy never fuses a multiply-add), so it takes the same branch as a
    correct float32 kernel;
  * the values themselves (sdf, colour, positions, depths) are computed in float64.
Where the float32 and float64 forms of a predicate disagree, the element is a "tie" and is reported: a kernel that
reordered or contracted that expression could take the other branch there.

The ray march is the exception to the first rule: its predicates (nearest-voxel rounding, the [-0.5, 0.1]
interpolation window, sdf <= 0, len < lenMax) act on march positions that float32 and float64 reach by different
rounding, so `cast_rays` evaluates them in float64 and flags every ray that passed within `tie_tol` of one of them.
"""
import numpy as np

F = np.float32
FAR_AWAY, VERY_CLOSE = F(999999.9), F(0.05)
MEAN_SIGMA_L = 1.2232


class Scale:
    """How a bound grows with the size of the coordinates.  `P` is the largest |voxel coordinate| of a fixture and `u`
    float32's spacing there; `scale(origin, c)` is max(origin, c u): the bound that holds at the world origin, or c
    float32 roundings of a position-sized quantity, whichever is larger.  Up to P = 256 (every fixture at the origin) u
    counts as 0, so each bound is exactly the origin's."""

    def __init__(self, P=0):
        self.P = int(P)
        self.u = float(np.spacing(F(P))) if P > 256 else 0.0

    def __call__(self, origin, c):
        return max(origin, c * self.u)


ORIGIN = Scale(0)


def mat_vec_f32(M, p):
    """ORUtils Matrix4f * Vector4f(p, 1) in float32: row r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 (no FMA)."""
    M = np.asarray(M, F)
    x, y, z = (p[..., k].astype(F) for k in range(3))
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], -1)


def mat_vec_f64(M, p):
    M = np.asarray(M, np.float64)
    return p @ M[:3, :3].T + M[:3, 3]


def project_f32(intr, pc):
    """u = fx * x / z + cx, v = fy * y / z + cy, float32 in that order."""
    fx, fy, cx, cy = (F(v) for v in intr)
    return (fx * pc[..., 0]) / pc[..., 2] + cx, (fy * pc[..., 1]) / pc[..., 2] + cy


def project_f64(intr, pc):
    fx, fy, cx, cy = (float(F(v)) for v in intr)
    return fx * pc[..., 0] / pc[..., 2] + cx, fy * pc[..., 1] / pc[..., 2] + cy


# ---------------------------------------------------------------------------------------------------------------------
# A.3 depth conversion and UpdateView's bilateral filter
# ---------------------------------------------------------------------------------------------------------------------
def depth_to_float(mm, a=1.0 / 1000.0, b=0.0):
    mm = np.asarray(mm, np.int64)
    return np.where((mm <= 0) | (mm > 32000), -1.0, mm * float(F(a)) + float(F(b)))


def filter_depth_pass(src, dst):
    """Upstream filterDepth over the interior [2, W-3] x [2, H-3] of `dst` (its border is left as it is): a hole
    (z < 0) stays -1; otherwise the 5x5 weighted mean of the non-negative taps, weight
    exp(-0.5 ((|i| + |j|) sigma_L^2 + (z' - z)^2 sigma_z^2)), sigma_z = 1 / (0.0012 + 0.0019 (z - 0.4)^2 + 0.0001 / sqrt(z) / 4)."""
    H, W = src.shape
    z = src[2:H - 2, 2:W - 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        sz = 1.0 / (0.0012 + 0.0019 * (z - 0.4) ** 2 + 0.0001 / np.sqrt(z) * 0.25)
    num = np.zeros_like(z)
    den = np.zeros_like(z)
    for i in range(-2, 3):
        for j in range(-2, 3):
            t = src[2 + i:H - 2 + i, 2 + j:W - 2 + j]
            w = np.exp(-0.5 * ((abs(i) + abs(j)) * MEAN_SIGMA_L ** 2 + (t - z) ** 2 * sz ** 2))
            w = np.where(t < 0.0, 0.0, w)
            num += w * np.where(t < 0.0, 0.0, t)
            den += w
    with np.errstate(invalid="ignore", divide="ignore"):
        dst[2:H - 2, 2:W - 2] = np.where(z < 0.0, -1.0, num / den)


def bilateral_update_view(depth):
    """ITMViewBuilder::UpdateView with filtering on: five passes alternating between the depth image and floatImage,
    a zero-initialised image whose border is never written; the result is floatImage (zero border)."""
    a = np.array(depth, np.float64)
    b = np.zeros_like(a)
    filter_depth_pass(a, b)
    filter_depth_pass(b, a)
    filter_depth_pass(a, b)
    filter_depth_pass(b, a)
    filter_depth_pass(a, b)
    return b


# ---------------------------------------------------------------------------------------------------------------------
# A.5 / A.11 voxel update and de-integration
# ---------------------------------------------------------------------------------------------------------------------
LOCAL = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)[..., ::-1].reshape(512, 3)


def round_half_away_f32(x):
    """roundf on float32 values (exact: the float64 of a float32 plus 0.5 is exact)."""
    x = x.astype(np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def new_weight(d32, wp):
    """SURVEY A.11 WeightParams law: depthWeighting ? max(1, (int)roundf(maxNewW (1 - min(d, maxD) / maxD))) : 1."""
    if wp is None or not wp[0]:
        return np.ones(d32.shape, np.int64)
    max_new_w, maxd = F(wp[1]), F(wp[2])
    dd = np.minimum(d32, maxd)
    w = round_half_away_f32(max_new_w * (F(1) - dd / maxd)).astype(np.int64)
    return np.clip(w, 1, int(wp[1]))


def bilinear_rgb(rgba, u32, v32, u64, v64):
    """Bilinear RGB at (u, v): the 2x2 neighbourhood comes from floor of the float32 position, the weights from the
    float64 one."""
    W = rgba.shape[1]
    ix, iy = np.floor(u32).astype(np.int64), np.floor(v32).astype(np.int64)
    dx, dy = u64 - ix, v64 - iy
    flat = rgba.reshape(-1, 4)[:, :3].astype(np.float64)
    a, b = flat[ix + iy * W], flat[ix + 1 + iy * W]
    c, d = flat[ix + (iy + 1) * W], flat[ix + 1 + (iy + 1) * W]
    return (a * ((1 - dx) * (1 - dy))[:, None] + b * (dx * (1 - dy))[:, None] + c * ((1 - dx) * dy)[:, None]
            + d * (dx * dy)[:, None])


def integrate(vox, block_pos, depth, rgba, M_d, intr, vs, mu, max_w, M_rgb=None, intr_rgb=None, stop_at_max=False,
              wp=None, deintegrate=False):
    """The voxel update of A.5 (or the de-integration of A.11) applied to the blocks `vox` [n, 512] at block
    positions [n, 3].  `depth` is the view's float32 depth image, `rgba` [H, W, 4].  Returns (new voxels, tie count)."""
    M_rgb = M_d if M_rgb is None else M_rgb
    intr_rgb = intr if intr_rgb is None else intr_rgb
    out = vox.copy()
    n = len(block_pos)
    if n == 0:
        return out, 0
    Hd, Wd = depth.shape
    Hr, Wr = rgba.shape[:2]
    vi = (np.asarray(block_pos, np.int64)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    v = out.reshape(-1)
    pm32 = vi.astype(F) * F(vs)
    pm64 = vi * float(F(vs))
    mu32, mu64 = F(mu), float(F(mu))
    upd = np.ones(len(vi), bool)
    if stop_at_max and not deintegrate:
        upd &= v["w_depth"] != max_w
    # -- depth -----------------------------------------------------------------------------------------------------
    pc32, pc64 = mat_vec_f32(M_d, pm32), mat_vec_f64(M_d, pm64)
    ok = pc32[:, 2] > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u32, w32 = project_f32(intr, pc32)
        u64, w64 = project_f64(intr, pc64)
    ok &= (u32 >= 1) & (u32 <= F(Wd - 2)) & (w32 >= 1) & (w32 <= F(Hd - 2))
    ok64 = (pc64[:, 2] > 0) & (u64 >= 1) & (u64 <= Wd - 2) & (w64 >= 1) & (w64 <= Hd - 2)
    ties = ok != ok64
    ui, wi = np.zeros(len(vi), np.int64), np.zeros(len(vi), np.int64)
    ui[ok] = (u32[ok] + F(0.5)).astype(np.int64)
    wi[ok] = (w32[ok] + F(0.5)).astype(np.int64)
    both = ok & ok64
    ties |= both & (((u64 + 0.5).astype(np.int64) != ui) | ((w64 + 0.5).astype(np.int64) != wi))
    dm32 = np.where(ok, depth.reshape(-1)[ui + wi * Wd], F(-1))
    ok &= dm32 > 0
    eta32 = dm32 - pc32[:, 2]
    eta64 = dm32.astype(np.float64) - pc64[:, 2]
    ties |= ok & ((eta32 < -mu32) != (eta64 < -mu64))
    ok &= eta32 >= -mu32
    ok &= upd
    oldF = v["sdf"].astype(np.float64) / 32767.0
    oldW = v["w_depth"].astype(np.int64)
    # (the spec takes a voxel only with eta32 >= -mu32, so its newF is >= -1; eta64 may lie below -mu64 where the two
    # disagree -- a tie -- and the value stored for it must not leave int16's range)
    newF = np.clip(eta64 / mu64, -1.0, 1.0)
    newW = new_weight(dm32, wp)
    if not deintegrate:
        Wsum = oldW + newW
        Fn = (oldW * oldF + newW * newF) / Wsum
        sdf = np.trunc(Fn * 32767.0)
        v["sdf"] = np.where(ok, sdf, v["sdf"]).astype(np.int16)
        v["w_depth"] = np.where(ok, np.minimum(Wsum, max_w), oldW).astype(np.uint8)
    else:
        rem = oldW - newW
        d_ok = ok & (rem >= 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            Fn = np.clip((oldW * oldF - newW * newF) / rem, -1.0, 1.0)
        sdf = np.where(rem == 0, 32767, np.trunc(Fn * 32767.0))
        v["sdf"] = np.where(d_ok, sdf, v["sdf"]).astype(np.int16)
        v["w_depth"] = np.where(d_ok, rem, oldW).astype(np.uint8)
    # -- colour: only where the depth measurement was taken, and only close to the surface --------------------------
    with np.errstate(divide="ignore", invalid="ignore"):
        gate32 = (eta32 > mu32) | (np.abs(eta32 / mu32) > F(0.25))
        gate64 = (eta64 > mu64) | (np.abs(eta64 / mu64) > 0.25)
    ties |= ok & (gate32 != gate64)
    c_ok = ok & ~gate32
    pr32, pr64 = mat_vec_f32(M_rgb, pm32), mat_vec_f64(M_rgb, pm64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ru32, rw32 = project_f32(intr_rgb, pr32)
        ru64, rw64 = project_f64(intr_rgb, pr64)
    inb32 = (ru32 >= 1) & (ru32 <= F(Wr - 2)) & (rw32 >= 1) & (rw32 <= F(Hr - 2))
    inb64 = (ru64 >= 1) & (ru64 <= Wr - 2) & (rw64 >= 1) & (rw64 <= Hr - 2)
    ties |= c_ok & (inb32 != inb64)
    c_ok &= inb32
    idx = np.nonzero(c_ok)[0]
    if len(idx):
        c = bilinear_rgb(rgba, ru32[idx], rw32[idx], ru64[idx], rw64[idx]) / 255.0
        oldC = v["clr"][idx].astype(np.float64) / 255.0
        oWc = v["w_color"][idx].astype(np.float64)[:, None]
        if not deintegrate:
            C = (oldC * oWc + c) / (oWc + 1.0)
            v["clr"][idx] = np.trunc(C * 255.0).astype(np.uint8)
            v["w_color"][idx] = np.minimum(oWc[:, 0] + 1, max_w).astype(np.uint8)
        else:
            has = oWc[:, 0] >= 1
            rem = oWc - 1.0
            with np.errstate(divide="ignore", invalid="ignore"):
                C = np.clip((oldC * oWc - c) / rem, 0.0, 1.0)
            newc = np.where(rem == 0, 0, np.trunc(C * 255.0))
            sel = idx[has]
            v["clr"][sel] = newc[has].astype(np.uint8)
            v["w_color"][sel] = rem[has, 0].astype(np.uint8)
    return out, int(ties.sum())


# ---------------------------------------------------------------------------------------------------------------------
# A.5 / A.11 once more, value by value: what a float32 evaluation in the spec's operation order may store
# ---------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24  # the relative size of one float32 rounding


def _bilinear_f64(rgba, ix, iy, dx, dy):
    W = rgba.shape[1]
    flat = rgba.reshape(-1, 4)[:, :3].astype(np.float64)
    a, b = flat[ix + iy * W], flat[ix + 1 + iy * W]
    c, d = flat[ix + (iy + 1) * W], flat[ix + 1 + (iy + 1) * W]
    return (a * ((1 - dx) * (1 - dy))[:, None] + b * (dx * (1 - dy))[:, None] + c * ((1 - dx) * dy)[:, None]
            + d * (dx * dy)[:, None])


def _permitted(q, band, lo_clip, hi_clip):
    """trunc(q - band), trunc(q + band) (C's conversion: toward zero), each clamped as the spec clamps the quotient."""
    a = np.clip(np.trunc(np.clip(q - band, lo_clip, hi_clip)), lo_clip, hi_clip).astype(np.int64)
    b = np.clip(np.trunc(np.clip(q + band, lo_clip, hi_clip)), lo_clip, hi_clip).astype(np.int64)
    return a, b


def update_exact(vox, block_pos, depth, rgba, M_d, intr, vs, mu, max_w, M_rgb=None, intr_rgb=None, stop_at_max=False,
                 wp=None, deintegrate=False):
    """`integrate` above with every stored value pinned instead of allowed 1 LSB.  Same arguments.  Returns (lo, hi, info)
    in the style of combine_stored: two voxel arrays that agree in every weight and pad byte and hold, value by value, the
    two results trunc(q - band) and trunc(q + band) a float32 evaluation in the spec's order may store; q is the exact
    value (float64 of integer and dyadic operands: its own error, 1e-12 LSB, is nothing beside the bands) and a value is
    a *tie* where the two differ.  S = 32767 for the sdf and 255 for a colour channel, u = 2^-24, W / w the stored and the
    new weight, F = sdf / S, f = min(1, eta / mu); every operand has magnitude <= 1 before a weight scales it.

    Bands (absolute, in LSB of the stored value; derived from the roundings alone, before any engine ran):
      fusion, sdf.  RN(sdf / S): u.  RN(W F): u W more, 2 u W in the numerator.  RN(eta / mu): u (none when mu is a power
        of two; eta itself is exact for dyadic inputs, and |eta32 - eta64| w / mu is added where it is not).  RN(w f): 2 u w
        in the numerator.  The sum: u (W + w).  Numerator: 3 u (W + w), i.e. 3 u after the exact division; the quotient's
        rounding u, the product with S u: 5 u S = 0.0098.  One more u for the second-order terms: band = 6 u S = 0.0117.
      fusion, colour.  The bilinear sample at the float32 position (dx, 1 - dx, dy, 1 - dy are exact in float32): two
        roundings per term, three sums, 5 u m.  RN(m / 255): 6 u in c.  RN(C / 255), RN(C' Wc): 2 u Wc.  The sum:
        u (Wc + 1).  Numerator (3 Wc + 7) u over Wc + 1, quotient u, product u, one u more:
        band = 255 u ((3 Wc + 7) / (Wc + 1) + 3), between 6 u 255 = 9.1e-5 and 10 u 255 = 1.5e-4; plus the distance
        between the value at the float32 position and at the float64 one (a kernel may round the projection otherwise).
      de-integration, sdf.  Numerator W F - w f: 2 u W + 2 u w + u |N|, divided by r = W - w; quotient Q = N / r rounds by
        u |Q|, the clamped product by u S: band = u S ((2 W + 2 w) / r + 2 |Q| + 2) (the last u as above): it grows with
        W / (W - w).  A quotient beyond +-1 by more than the band is exactly +-S.
      de-integration, colour.  Likewise with w = 1, 6 u in c: band = 255 u ((2 Wc + 6) / r + 2 |Q| + 2), r = Wc - 1,
        clamped to [0, 255], plus the position term.
    Weights are exact: min(W + w, max_w); W - w where W >= w (0: the empty voxel, sdf 32767), else the depth half is left
    alone while the colour half still updates (it needs Wc >= 1; Wc - 1 = 0 gives colour 0); stopIntegratingAtMaxW is a
    fusion rule and a de-integration ignores it.
    Predicates (depth > 0, eta < -mu, image bounds, the pixel picked, the 0.25 gate; W >= w is an integer test) are taken
    in float32 with float64 beside them, as `integrate` does; a voxel where they disagree is in info['pred_tie'] and its
    values are not pinned.
    info: q_sdf, q_clr, tie_sdf, tie_clr, band_sdf, band_clr, pred_tie; the masks projected (into the depth image), seen (a
    depth > 0 there: eta is defined), taken (eta >= -mu), upd_depth, colour_seen (inside the gate and the colour image),
    upd_colour; eta, f, w_new and the colour sample."""
    M_rgb = M_d if M_rgb is None else M_rgb
    intr_rgb = intr if intr_rgb is None else intr_rgb
    lo = vox.copy()
    Hd, Wd = depth.shape
    Hr, Wr = rgba.shape[:2]
    vi = (np.asarray(block_pos, np.int64)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    v = lo.reshape(-1)
    pm32, pm64 = vi.astype(F) * F(vs), vi * float(F(vs))
    mu32, mu64 = F(mu), float(F(mu))
    # -- the measurement ---------------------------------------------------------------------------------------------
    pc32, pc64 = mat_vec_f32(M_d, pm32), mat_vec_f64(M_d, pm64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u32, w32 = project_f32(intr, pc32)
        u64, w64 = project_f64(intr, pc64)
    ok = (pc32[:, 2] > 0) & (u32 >= 1) & (u32 <= F(Wd - 2)) & (w32 >= 1) & (w32 <= F(Hd - 2))
    ok64 = (pc64[:, 2] > 0) & (u64 >= 1) & (u64 <= Wd - 2) & (w64 >= 1) & (w64 <= Hd - 2)
    ties = ok != ok64
    projected = ok.copy()
    ui, wi = np.zeros(len(vi), np.int64), np.zeros(len(vi), np.int64)
    ui[ok] = (u32[ok] + F(0.5)).astype(np.int64)
    wi[ok] = (w32[ok] + F(0.5)).astype(np.int64)
    both = ok & ok64
    with np.errstate(invalid="ignore"):
        ties |= both & (((u64 + 0.5).astype(np.int64) != ui) | ((w64 + 0.5).astype(np.int64) != wi))
    dm32 = np.where(ok, depth.reshape(-1)[ui + wi * Wd], F(-1))
    ok &= dm32 > 0
    eta32 = dm32 - pc32[:, 2]
    eta64 = dm32.astype(np.float64) - pc64[:, 2]
    ties |= ok & ((eta32 < -mu32) != (eta64 < -mu64))
    seen = ok.copy()  # a depth measurement exists; eta is defined
    ok &= eta32 >= -mu32
    taken = ok.copy()
    if stop_at_max and not deintegrate:
        ok &= v["w_depth"] != max_w
    S = 32767.0
    s = v["sdf"].astype(np.float64)
    W = v["w_depth"].astype(np.int64)
    em = eta64 / mu64
    f = np.minimum(1.0, em)
    w = new_weight(dm32, wp)
    d_eta = np.abs(eta32.astype(np.float64) - eta64) / mu64 * S
    with np.errstate(divide="ignore", invalid="ignore"):
        if not deintegrate:
            upd_d = ok
            q = (W * s + w * f * S) / (W + w)
            band = np.full(len(vi), 6 * U32 * S) + d_eta * w / (W + w)
            a, b = _permitted(q, band, -S, S)
            new_w = np.minimum(W + w, max_w)
        else:
            r = W - w
            upd_d = ok & (r >= 0)
            q = (W * s - w * f * S) / r
            band = U32 * S * ((2 * W + 2 * w) / r + 2 * np.abs(q) / S + 2) + d_eta * w / r
            a, b = _permitted(q, band, -S, S)
            a, b, q = (np.where(r == 0, 32767, x) for x in (a, b, q))
            band = np.where(r == 0, 0.0, band)
            new_w = r
    hi = lo.copy()
    vh = hi.reshape(-1)
    for out, val in ((v, np.minimum(a, b)), (vh, np.maximum(a, b))):
        out["sdf"] = np.where(upd_d, val, out["sdf"]).astype(np.int16)
        out["w_depth"] = np.where(upd_d, new_w, W).astype(np.uint8)
    q_sdf, band_sdf = np.where(upd_d, q, s), np.where(upd_d, band, 0.0)
    tie_sdf = upd_d & (a != b)
    # -- colour: only where the depth measurement was taken, and only close to the surface --------------------------
    with np.errstate(divide="ignore", invalid="ignore"):
        gate32 = (eta32 > mu32) | (np.abs(eta32 / mu32) > F(0.25))
        gate64 = (eta64 > mu64) | (np.abs(em) > 0.25)
    ties |= ok & (gate32 != gate64)
    c_ok = ok & ~gate32
    pr32, pr64 = mat_vec_f32(M_rgb, pm32), mat_vec_f64(M_rgb, pm64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ru32, rw32 = project_f32(intr_rgb, pr32)
        ru64, rw64 = project_f64(intr_rgb, pr64)
    inb32 = (ru32 >= 1) & (ru32 <= F(Wr - 2)) & (rw32 >= 1) & (rw32 <= F(Hr - 2))
    inb64 = (ru64 >= 1) & (ru64 <= Wr - 2) & (rw64 >= 1) & (rw64 <= Hr - 2)
    ties |= c_ok & (inb32 != inb64)
    c_ok &= inb32
    Wc = v["w_color"].astype(np.int64)
    colour_seen = c_ok.copy()
    if deintegrate:
        c_ok &= Wc >= 1
    q_clr = v["clr"].astype(np.float64)
    sample = np.full((len(vi), 3), np.nan)
    band_clr = np.zeros((len(vi), 3))
    tie_clr = np.zeros((len(vi), 3), bool)
    idx = np.nonzero(c_ok)[0]
    if len(idx):
        ix, iy = np.floor(ru32[idx]).astype(np.int64), np.floor(rw32[idx]).astype(np.int64)
        m = _bilinear_f64(rgba, ix, iy, ru32[idx].astype(np.float64) - ix, rw32[idx].astype(np.float64) - iy)
        m_at64 = _bilinear_f64(rgba, ix, iy, ru64[idx] - ix, rw64[idx] - iy)
        C, wc = q_clr[idx], Wc[idx].astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            if not deintegrate:
                q = (C * wc + m) / (wc + 1)
                band = 255 * U32 * ((3 * wc + 7) / (wc + 1) + 3) + np.abs(m - m_at64) / (wc + 1)
                new_wc = np.minimum(wc[:, 0] + 1, max_w)
            else:
                r = wc - 1
                q = (C * wc - m) / r
                band = 255 * U32 * ((2 * wc + 6) / r + 2 * np.abs(q) / 255 + 2) + np.abs(m - m_at64) / r
                new_wc = r[:, 0]
            a, b = _permitted(q, band, 0.0, 255.0)
            if deintegrate:
                a, b, q = (np.where(r == 0, 0, x) for x in (a, b, q))
                band = np.where(r == 0, 0.0, band)
        for out, val in ((v, np.minimum(a, b)), (vh, np.maximum(a, b))):
            out["clr"][idx] = val.astype(np.uint8)
            out["w_color"][idx] = new_wc.astype(np.uint8)
        q_clr[idx], band_clr[idx], tie_clr[idx], sample[idx] = q, band, a != b, m
    shp = vox.shape
    info = dict(q_sdf=q_sdf.reshape(shp), q_clr=q_clr.reshape(shp + (3,)), tie_sdf=tie_sdf.reshape(shp),
                tie_clr=tie_clr.reshape(shp + (3,)), pred_tie=ties.reshape(shp), projected=projected.reshape(shp),
                upd_depth=upd_d.reshape(shp), upd_colour=c_ok.reshape(shp), seen=seen.reshape(shp),
                taken=taken.reshape(shp), colour_seen=colour_seen.reshape(shp), sample=sample.reshape(shp + (3,)),
                eta=np.where(seen, eta64, np.nan).reshape(shp), f=f.reshape(shp), w_new=w.reshape(shp), band_sdf=band_sdf.reshape(shp),
                band_clr=band_clr.reshape(shp + (3,)))
    return lo, hi, info


def update_tie_share(info, sel=None):
    """Ties among the updated values (one sdf per updated depth half, three channels per updated colour half) of the
    blocks `sel` (all by default)."""
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    n = int(pick(info["upd_depth"]).sum()) + 3 * int(pick(info["upd_colour"]).sum())
    return (int(pick(info["tie_sdf"]).sum()) + int(pick(info["tie_clr"]).sum())) / max(n, 1)


def check_updated(got, lo, hi, info, what=""):
    """`got` against update_exact's answer: weights and pad exact, every value one of its permitted results (so a non-tie
    value equals trunc(q) exactly), |got - q| <= 1 on every voxel that is no tie and <= 1 + band at a tie (with q just
    above an integer k the lower permitted result is k - 1: the distance can pass 1 by the band, never by more); voxels
    with a predicate tie are left out.  Returns the figures DESIGN 4c records."""
    got = np.asarray(got)
    keep = ~info["pred_tie"]
    for f in ("w_depth", "w_color", "_pad"):
        bad = (got[f] != lo[f]) & keep
        assert not bad.any(), f"{what}: {f} differs in {int(bad.sum())} voxels, first got {got[f][bad][:4]}, want {lo[f][bad][:4]}"
    out = {}
    for f, q, tie, band in (("sdf", info["q_sdf"], info["tie_sdf"], info["band_sdf"]),
                            ("clr", info["q_clr"], info["tie_clr"], info["band_clr"])):
        k = keep if f == "sdf" else keep[..., None]
        g = got[f].astype(np.int64)
        bad = (g != lo[f]) & (g != hi[f]) & k
        assert not bad.any(), (f"{what}: {int(bad.sum())} {f} values are none of the permitted results; first got "
                               f"{g[bad][:4]}, permitted {lo[f][bad][:4]} / {hi[f][bad][:4]}, q {q[bad][:4]}")
        ends = (-32767.0, 32767.0) if f == "sdf" else (0.0, 255.0)
        err = np.where(k, np.abs(g - np.clip(q, *ends)), 0.0)
        over = err - 1.0 - np.where(tie, band, 0.0)
        assert over.max(initial=-1.0) <= 0.0, f"{what}: |got - q| = {err[over > 0][:4]} for {f}, bands {band[over > 0][:4]}"
        out[f] = dict(ties=int(tie.sum()), worst_err=float(err.max(initial=0.0)),
                      at_upper_result=int((tie & (g == hi[f]) & k).sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# A.8 the merge of a host copy into a resident block (upstream CombineVoxelInformation), in exact integer arithmetic
# ---------------------------------------------------------------------------------------------------------------------
# The merged value is trunc(q), q = (w_h v_h + w_d v_d) / (w_h + w_d): a rational with denominator w_h + w_d, computed
# here from integers.  A float32 engine evaluates ((w_h (v_h / s) + w_d (v_d / s)) / (w_h + w_d)) s with s = 32767 (sdf)
# or 255 (colour): every operand and intermediate has magnitude <= 1 before the weights scale it, and a term passes
# five roundings of relative size u = 2^-24 on its way (v / s, the product with its weight, the sum, the quotient, the
# product with s; the weights and their sum are exact), so the float32 result lies within 5 u s of q: 0.0098 for the sdf,
# 7.6e-5 for a colour channel.  The bands below cover that (1 / 100 and 1 / 1000); only where an integer lies within the
# band of q can a correct float32 merge land on the other side of the truncation: a *tie*.  Everywhere else the value is
# exact.  The denominators are at most 510, so a colour q within 1e-3 of an integer IS that integer (1 / 510 > 1e-3).
SDF_BAND_INV, CLR_BAND_INV = 100, 1000


def _trunc_div(n, d):
    """n / d truncated toward zero, integers, d > 0."""
    return np.sign(n) * (np.abs(n) // d)


def _merge_half(vh, wh, vd, wd, band_inv):
    """One half of one merge on int64 arrays (values, their weights).  Returns (lo, hi, q, tie): the permitted results
    are trunc(q - band) and trunc(q + band) (equal unless an integer lies inside the band), q as float64, and whether q
    lies within the band of an integer."""
    num, den = wh * vh + wd * vd, np.maximum(wh + wd, 1)
    lo = _trunc_div(num * band_inv - den, den * band_inv)
    hi = _trunc_div(num * band_inv + den, den * band_inv)
    r = np.abs(num) % den  # |q|'s distance below / above the neighbouring integers, in units of 1 / den
    tie = np.minimum(r, den - r) * band_inv <= den
    return lo, hi, num / den, tie


def combine_stored(host_block, device_block, max_w):
    """SURVEY A.8's merge of a stored block into the resident one, voxel by voxel; the depth half (sdf, w_depth) and the
    colour half (clr, w_color) independently.  A half whose host weight is 0 is left byte-identical; otherwise its
    weight becomes min(w_host + w_device, max_w) and its value the weighted mean truncated toward zero.
    Returns (lo, hi, info): two voxel arrays that agree in every weight (and the pad byte, which is the device's) and
    hold, value by value, the two results a float32 evaluation may reach (lo == hi except at a tie).  info: the exact
    quotients (`q_sdf`, `q_clr`), which halves merged (`merged_depth`, `merged_colour`) and the tie masks."""
    h, d = np.asarray(host_block), np.asarray(device_block)
    lo, hi = d.copy(), d.copy()
    i64 = lambda a: a.astype(np.int64)
    md, mc = h["w_depth"] != 0, h["w_color"] != 0
    a, b, q_s, tie_s = _merge_half(i64(h["sdf"]), i64(h["w_depth"]), i64(d["sdf"]), i64(d["w_depth"]), SDF_BAND_INV)
    w = np.minimum(i64(h["w_depth"]) + i64(d["w_depth"]), max_w)
    for out, v in ((lo, np.minimum(a, b)), (hi, np.maximum(a, b))):
        out["sdf"] = np.where(md, v, d["sdf"])
        out["w_depth"] = np.where(md, w, d["w_depth"])
    wh, wd = i64(h["w_color"])[..., None], i64(d["w_color"])[..., None]
    a, b, q_c, tie_c = _merge_half(i64(h["clr"]), wh, i64(d["clr"]), wd, CLR_BAND_INV)
    w = np.minimum(wh[..., 0] + wd[..., 0], max_w)
    for out, v in ((lo, np.minimum(a, b)), (hi, np.maximum(a, b))):
        out["clr"] = np.where(mc[..., None], v, d["clr"])
        out["w_color"] = np.where(mc, w, d["w_color"])
    info = dict(q_sdf=np.where(md, q_s, d["sdf"]), q_clr=np.where(mc[..., None], q_c, d["clr"]), merged_depth=md,
                merged_colour=mc, tie_sdf=md & tie_s, tie_clr=mc[..., None] & tie_c)
    return lo, hi, info


def merge_tie_share(info):
    """Ties among the merged values (one sdf and three colour channels per voxel, each counted where its half merged)."""
    n = int(info["merged_depth"].sum()) + 3 * int(info["merged_colour"].sum())
    return (int(info["tie_sdf"].sum()) + int(info["tie_clr"].sum())) / max(n, 1)


def check_combined(got, lo, hi, info, what=""):
    """`got` against combine_stored's answer: weights and pad exact, every value one of its permitted results (so a
    non-tie value equals trunc(q) exactly and |got - q| <= 1 everywhere).  Returns the figures DESIGN 4c records."""
    got = np.asarray(got)
    for f in ("w_depth", "w_color", "_pad"):
        bad = got[f] != lo[f]
        assert not bad.any(), f"{what}: {f} differs in {int(bad.sum())} voxels, first got {got[f][bad][:4]}, want {lo[f][bad][:4]}"
    out = {}
    for f, q, tie in (("sdf", info["q_sdf"], info["tie_sdf"]), ("clr", info["q_clr"], info["tie_clr"])):
        g = got[f].astype(np.int64)
        bad = (g != lo[f]) & (g != hi[f])
        assert not bad.any(), (f"{what}: {int(bad.sum())} {f} values are none of the permitted results; first got "
                               f"{g[bad][:4]}, permitted {lo[f][bad][:4]} / {hi[f][bad][:4]}, q {q[bad][:4]}")
        err = np.abs(g - q)
        assert err.max(initial=0.0) <= 1.0, f"{what}: |got - q| = {err.max()} for {f}"
        other = g != np.trunc(q).astype(np.int64)  # (a float64 quotient of integers truncates as the rational does)
        dist = np.abs(q - np.round(q))
        out[f] = dict(ties=int(tie.sum()), worst_err=float(err.max(initial=0.0)), off_truncation=int(other.sum()),
                      worst_distance_off_truncation=float(dist[other].max(initial=0.0)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# A.2 / A.7 reads, castRay, the shading normal
# ---------------------------------------------------------------------------------------------------------------------
def read_trilinear(m, p):
    """A.7 read_trilinear at voxel-unit positions p [n, 3]: the 8 corner shorts (missing = 32767), lerped in x, then
    y, then z, / 32767.  Also returns whether any corner was missing."""
    p0 = np.floor(p)
    c = p - p0
    p0 = p0.astype(np.int64)
    acc = np.zeros(len(p))
    miss = np.zeros(len(p), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                s, _, f = m.lookup(p0 + np.array([dx, dy, dz]))
                w = (c[:, 0] if dx else 1 - c[:, 0]) * (c[:, 1] if dy else 1 - c[:, 1]) * (c[:, 2] if dz else 1 - c[:, 2])
                acc += w * s
                miss |= ~f
    return acc / 32767.0, miss


def read_colour_trilinear(m, p):
    p0 = np.floor(p)
    c = p - p0
    p0 = p0.astype(np.int64)
    acc = np.zeros((len(p), 3))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                _, clr, _ = m.lookup(p0 + np.array([dx, dy, dz]))
                w = (c[:, 0] if dx else 1 - c[:, 0]) * (c[:, 1] if dy else 1 - c[:, 1]) * (c[:, 2] if dz else 1 - c[:, 2])
                acc += w[:, None] * clr
    return acc


def sdf_normal(m, p):
    """computeSingleNormalFromSDF: per axis, the trilinear field one voxel ahead minus one voxel behind (the 6 taps,
    each a trilinear read of 8 corners); normalised.  Also returns whether any tap touched a missing voxel."""
    g = np.zeros((len(p), 3))
    miss = np.zeros(len(p), bool)
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        a, ma = read_trilinear(m, p + e)
        b, mb = read_trilinear(m, p - e)
        g[:, k] = a - b
        miss |= ma | mb
    with np.errstate(invalid="ignore", divide="ignore"):  # (no gradient away from the surface: NaN there)
        return g / np.linalg.norm(g, axis=1, keepdims=True), miss


def light_of(M):
    """The shading light direction: minus the camera's z axis in world coordinates (-invM.getColumn(2))."""
    return -np.linalg.inv(np.asarray(M, np.float64))[:3, 2]


def shaded_grey(angle):
    """drawPixelGrey: (uchar)((0.8 angle + 0.2) * 255)."""
    return np.trunc((0.8 * angle + 0.2) * 255.0)


def normal_colour(n):
    """drawPixelNormal (upstream InfiniTAM v2, ITMVisualisationEngine_Shared.h): (uchar)((0.3 + (1 - n) * 0.35) * 255)
    per channel.  SURVEY A.7's shorthand ((n + 1) / 2) * 255 is not what upstream draws; DESIGN.md 4c records this."""
    return np.trunc((0.3 + (1.0 - n) * 0.35) * 255.0)


def icp_normals(p, hit, tie, vs, light):
    """processPixelICP<true, false>'s normal from the raycast points p [H, W, 3] (voxel units) and hits [H, W]:
    pixels within 3 of the image border get none; otherwise the points +-2 pixels away in x and y, unless one of them
    is no hit or the longer of the two differences exceeds 0.15 m, in which case the points +-1 away, which must all
    be hits.  n = -(dx x dy), normalised; kept where n . light > 0.  Returns (normals [H, W, 3], found [H, W], tap
    distance [H, W] (2 or 1), tie [H, W]): tie where a tap pixel is a tie ray or the 0.15 m switch, the
    angle > 0 cut or a tap's hit depended on a near-threshold value."""
    H, W = hit.shape
    n = np.zeros((H, W, 3))
    found = hit.copy()
    found[:3] = found[-3:] = False
    found[:, :3] = found[:, -3:] = False
    tap = np.full((H, W), 2)
    t_out = tie.copy()

    def sh(a, dy, dx):  # a[y + dy, x + dx] (wrapping; only used away from the border)
        return np.roll(a, (-dy, -dx), axis=(0, 1))

    h2 = sh(hit, 0, 2) & sh(hit, 0, -2) & sh(hit, 2, 0) & sh(hit, -2, 0)
    dx2, dy2 = sh(p, 0, 2) - sh(p, 0, -2), sh(p, 2, 0) - sh(p, -2, 0)
    ld = np.maximum((dx2 ** 2).sum(-1), (dy2 ** 2).sum(-1)) * vs * vs
    plus1 = ~h2 | (ld > 0.15 ** 2)
    t_out |= h2 & (np.abs(ld - 0.15 ** 2) < 1e-6 * 0.15 ** 2)
    dx1, dy1 = sh(p, 0, 1) - sh(p, 0, -1), sh(p, 1, 0) - sh(p, -1, 0)
    h1 = sh(hit, 0, 1) & sh(hit, 0, -1) & sh(hit, 1, 0) & sh(hit, -1, 0)
    found &= ~plus1 | h1
    tap[plus1] = 1
    dx = np.where(plus1[..., None], dx1, dx2)
    dy = np.where(plus1[..., None], dy1, dy2)
    for dy_, dx_ in ((0, 1), (0, 2), (1, 0), (2, 0), (0, -1), (0, -2), (-1, 0), (-2, 0)):
        t_out |= sh(tie, dy_, dx_)
    c = -np.cross(dx, dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = c / np.linalg.norm(c, axis=-1, keepdims=True)
    angle = c @ light
    t_out |= found & (np.abs(angle) < 1e-6)
    found &= angle > 0
    n[found] = c[found]
    return n, found, tap, t_out


def visible_blocks(m, M, intr, W, H):
    """A.6 on every block of the map (no swapping): any of the 8 corners with z >= 1e-10 inside [0, W) x [0, H)."""
    fac = F(8) * F(m.vs)
    vis = np.zeros(len(m.block_pos), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = m.block_pos.astype(F) * fac + np.array([dx, dy, dz], F) * fac
                pc = mat_vec_f32(M, c)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    u, v = project_f32(intr, pc)
                vis |= (pc[:, 2] >= F(1e-10)) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    return vis


def expected_depths(m, M, intr, W, H, z32=False):
    """A.7 CreateExpectedDepths on the visible blocks: per 8x8 tile the (min, max) camera z of the blocks whose
    projected corner bbox covers it.  Returns [ceil(H/8), ceil(W/8), 2]; no block = (FAR_AWAY, VERY_CLOSE).
    `z32`: the corners' camera z from the float32 mat-vec, as an engine forms it, in place of the float64 one."""
    tw, th = -(-W // 8), -(-H // 8)
    rng = np.empty((th, tw, 2))
    rng[..., 0], rng[..., 1] = FAR_AWAY, VERY_CLOSE
    bp = m.block_pos[visible_blocks(m, M, intr, W, H)]
    if len(bp) == 0:
        return rng
    fac = F(8) * F(m.vs)
    zs, us, vs_, goods = [], [], [], []
    for corner in range(8):
        d = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
        c32 = (bp + d).astype(F) * fac
        pc = mat_vec_f32(M, c32)
        good = pc[:, 2] >= F(1e-6)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u, v = project_f32(intr, pc)
        zs.append(pc[:, 2].astype(np.float64) if z32 else mat_vec_f64(M, (bp + d) * float(fac))[:, 2])
        us.append(u / F(8))
        vs_.append(v / F(8))
        goods.append(good)
    z, u, v, g = (np.stack(a, 1) for a in (zs, us, vs_, goods))
    with np.errstate(invalid="ignore"):
        ulx = np.minimum(W // 8, np.where(g, np.floor(u), np.inf).min(1))
        uly = np.minimum(H // 8, np.where(g, np.floor(v), np.inf).min(1))
        lrx = np.maximum(-1, np.where(g, np.ceil(u), -np.inf).max(1))
        lry = np.maximum(-1, np.where(g, np.ceil(v), -np.inf).max(1))
    zmin = np.where(g, z, np.inf).min(1)
    zmax = np.where(g, z, -np.inf).max(1)
    ulx, uly = np.maximum(ulx, 0), np.maximum(uly, 0)
    lrx, lry = np.minimum(lrx, W - 1), np.minimum(lry, H - 1)
    ok = (ulx <= lrx) & (uly <= lry) & (zmax >= float(VERY_CLOSE))
    zmin = np.maximum(zmin, float(VERY_CLOSE))
    for i in np.nonzero(ok)[0]:
        x0, x1 = int(ulx[i]), min(int(lrx[i]), tw - 1)
        y0, y1 = int(uly[i]), min(int(lry[i]), th - 1)
        if x0 > x1 or y0 > y1:
            continue
        t = rng[y0:y1 + 1, x0:x1 + 1]
        t[..., 0] = np.minimum(t[..., 0], zmin[i])
        t[..., 1] = np.maximum(t[..., 1], zmax[i])
    return rng


def _iround(x):
    """(int)((x < 0) ? x - 0.5 : x + 0.5)"""
    return np.trunc(np.where(x < 0, x - 0.5, x + 0.5)).astype(np.int64)


def cast_rays(m, M, intr, W, H, tie_tol=1e-4, max_steps=4000, by_outcome=False):
    """A.7 castRay for every pixel on map `m`.  Returns dict(p [H, W, 3] hit position in voxel units (world), hit
    [H, W], tie [H, W], miss_cell [H, W]: a read at the stop point or after either refinement touched a missing voxel, dir: the unit ray,
    p_stop / sdf_stop: where the march stopped and the read that stopped it, before the two refinement steps).

    `tie_tol` (voxels) is how far a float32 march position may lie from this one; every branch test uses it.  Far from the
    origin it grows with float32's spacing (placement_checks.py), and the plain rule -- a tie wherever a position comes
    within tie_tol of a nearest-voxel rounding boundary or a read within tie_tol of a threshold -- would call most rays
    ties.  `by_outcome` states the same tests by what they decide:
      * a nearest-voxel rounding within tie_tol of its boundary on one axis is a tie only if the voxel on the other side
        would make the march do something else: the two differ in being found, or in lying inside the interpolation
        window (inside it the trilinear read replaces the value, whichever voxel), or, both outside it, in value (the
        value is the step); two axes near their boundaries at once are a tie;
      * the nearest-voxel value is an integer / 32767 and meets 0.1, -0.5 and 0 the same way in float32 and float64: no
        tolerance applies to it; a trilinear read moves with the position by at most sqrt(3) vs / mu per voxel, so its
        hit test is a tie within sqrt(3) (vs / mu) tie_tol of 0."""
    vs, mu = float(F(m.vs)), float(F(m.mu))
    rng = expected_depths(m, M, intr, W, H)
    fx, fy, cx, cy = (float(F(v)) for v in intr)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
    r = rng[(ys // 8).astype(int), (xs // 8).astype(int)]
    invM = np.linalg.inv(np.asarray(M, np.float64))

    def at(z):
        pc = np.stack([z * ((xs - cx) / fx), z * ((ys - cy) / fy), z], -1)
        return np.linalg.norm(pc, axis=1) / vs, mat_vec_f64(invM, pc) / vs

    total, ps = at(r[:, 0])
    total_max, pe = at(r[:, 1])
    d = pe - ps
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
    step_scale = mu / vs
    sdf_tol = np.sqrt(3.0) * tie_tol / step_scale
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
        q = p[idx]
        frac = np.abs(q) - np.floor(np.abs(q))
        near = np.abs(frac - 0.5) < tie_tol
        r = _iround(q)
        s16, _, found = m.lookup(r)
        s = s16 / 32767.0
        step = np.full(len(idx), 8.0)
        win = found & (s <= 0.1) & (s >= -0.5)
        if not by_outcome:
            tie[idx] |= np.any(near, axis=1)
            tie[idx] |= found & ((np.abs(s - 0.1) < tie_tol) | (np.abs(s + 0.5) < tie_tol))
        else:
            tie[idx] |= near.sum(axis=1) > 1
            for ax in range(3):
                k = np.nonzero(near[:, ax])[0]
                if len(k) == 0:
                    continue
                alt = r[k].copy()
                alt[:, ax] += np.where(q[k, ax] > r[k, ax], 1, -1)
                a16, _, afound = m.lookup(alt)
                sa = a16 / 32767.0
                awin = afound & (sa <= 0.1) & (sa >= -0.5)
                same = (afound == found[k]) & (~afound | (awin & win[k]) | (~awin & ~win[k] & (a16 == s16[k])))
                tie[idx[k]] |= ~same
        if win.any():
            s[win] = read_trilinear(m, q[win])[0]
        stop = found & (s <= 0.0)
        tie[idx] |= (win & (np.abs(s) < sdf_tol)) if by_outcome else (found & (np.abs(s) < tie_tol))
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
    miss_cell = np.zeros(n, bool)
    miss_cell[h] = read_trilinear(m, p[h])[1]
    p[h] += (sdf[h] * step_scale)[:, None] * d[h]
    s, miss1 = read_trilinear(m, p[h])
    p[h] += (s * step_scale)[:, None] * d[h]
    miss_cell[h] |= miss1 | read_trilinear(m, p[h])[1]
    return dict(p=p.reshape(H, W, 3), hit=hit.reshape(H, W), tie=tie.reshape(H, W), miss_cell=miss_cell.reshape(H, W),
                dir=d.reshape(H, W, 3), p_stop=p_stop.reshape(H, W, 3),
                sdf_stop=sdf.reshape(H, W))


def camera_depth(M, p_vox, vs):
    """IMAGE_DEPTH: camera-frame z (metres) of a hit position in voxel units."""
    return mat_vec_f64(M, p_vox * float(F(vs)))[..., 2]


# ---------------------------------------------------------------------------------------------------------------------
# marching cubes: the vertex on a cube edge (the case table is csrc/mc_tables.h, validated by test_mc_tables.py)
# ---------------------------------------------------------------------------------------------------------------------
def edge_vertex(a, b, v1, v2):
    """sdfInterp: a + (0 - v1) / (v2 - v1) (b - a), with upstream's early-outs |v1| < 1e-5 -> a, |v2| < 1e-5 -> b,
    |v1 - v2| < 1e-5 -> a decided on the float32 sdf values."""
    f1, f2 = v1.astype(F), v2.astype(F)
    t = np.where(np.abs(F(0) - f1) < F(1e-5), 0.0,
                 np.where(np.abs(F(0) - f2) < F(1e-5), 1.0,
                          np.where(np.abs(f1 - f2) < F(1e-5), 0.0, (0.0 - v1) / np.where(v2 == v1, 1.0, v2 - v1))))
    return a + t[..., None] * (b - a)


def mesh(m, corner_offsets, edge_corners, table):
    """MeshScene on map `m`, in upstream's CPU-engine order: hash entries in index order (those holding a block),
    their voxels z-major, the table's triangles in order.  A cube is used when its 8 corners are present with
    sdf != 32767; its case index comes from the corner signs; vertices by `edge_vertex`.  Returns [n, 3, 3] in
    voxel units."""
    co = np.asarray(corner_offsets, np.int64)
    ent = np.nonzero(m.hash["ptr"] >= 0)[0]
    bpos = m.hash["pos"][ent].astype(np.int64)
    bases = (bpos[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)  # LOCAL: x fastest, then y, then z
    s = np.empty((len(bases), 8), np.int64)
    ok = np.ones(len(bases), bool)
    for k in range(8):
        sk, _, f = m.lookup(bases + co[k])
        s[:, k] = sk
        ok &= f & (sk != 32767)
    bases, s = bases[ok], s[ok]
    v = s / 32767.0
    v32 = s.astype(F) / F(32767)
    cube = ((v32 < 0).astype(np.int64) << np.arange(8)).sum(1)
    tab = np.full((256, 5, 3), -1, np.int64)
    cnt = np.zeros(256, np.int64)
    for c in range(256):
        row = [e for e in table[c] if e != -1]
        cnt[c] = len(row) // 3
        if cnt[c]:
            tab[c, :cnt[c]] = np.reshape(row, (-1, 3))
    per = cnt[cube]
    rep = np.repeat(np.arange(len(cube)), per)
    slot = np.arange(len(rep)) - np.repeat(np.cumsum(per) - per, per)
    edges = tab[cube[rep], slot]  # [n, 3]
    ec = np.asarray(edge_corners, np.int64)
    ia, ib = ec[edges, 0], ec[edges, 1]
    b = bases[rep][:, None, :]
    vr = v[rep]
    return edge_vertex((b + co[ia]).astype(np.float64), (b + co[ib]).astype(np.float64),
                       np.take_along_axis(vr, ia, 1), np.take_along_axis(vr, ib, 1))
