"""References of the view path: what turns the caller's images into the colour, raw depth and float depth every fusion,
de-integration and re-fusion reads.  Plain numpy, whole-image rules, written from the text that defines them --
CvToItm (InfiniTamDriver.cpp:84-103), FloatDepthmapToShort / ...ToInt16 (:167-200), ReadPrecomputed's loop
(PrecomputedDepthProvider.cpp:30-64), the pixel loop of DenseSlam::depthPostProcessing (DenseSlam.cpp:489-529) -- and
SURVEY.md Appendix A, not from the oracle or the kernels.

Rule of the file: a decision that is an integer rule is computed in integers and the rule is derived here; a decision
on a float expression is taken from the float32 evaluation in the text's own operation order (np.float32 element-wise,
never fused), with the float64 evaluation beside it, and the pixel is a TIE where the float64 value lies within a
derived margin of the decision's edge.  A tie pixel may go either way in a correct float32 engine.

The depth conversion itself is ref64.depth_to_float.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24  # unit roundoff of float32: one rounding moves a value by at most U times its magnitude


# ---------------------------------------------------------------------------------------------------------------------
# CvToItm: BGR -> RGBA
# ---------------------------------------------------------------------------------------------------------------------
def bgr_to_rgba(bgr):
    """.b = col[0], .g = col[1], .r = col[2], .a = 255 for every pixel: a byte permutation."""
    bgr = np.asarray(bgr, np.uint8)
    out = np.empty(bgr.shape[:-1] + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = bgr[..., 2], bgr[..., 1], bgr[..., 0], 255
    return out


# ---------------------------------------------------------------------------------------------------------------------
# dataset wire formats
# ---------------------------------------------------------------------------------------------------------------------
def wrap_i16(v):
    """An integer taken modulo 2^16 into int16.  The text casts a float straight to int16_t, which C leaves undefined
    outside [-32768, 32767]; the project defines it as the conversion to int32 followed by keeping the low 16 bits
    (what the x86 instruction sequence does), for every value inside int32."""
    v = np.asarray(v, np.int64)
    return (((v + 32768) % 65536) - 32768).astype(np.int16)


def trunc_div(n, d):
    """n / d truncated toward zero, in integers (C's float -> int conversion truncates toward zero)."""
    n = np.asarray(n, np.int64)
    return np.sign(n) * (np.abs(n) // d)


def max_mm_short(max_m):
    """(int16_t)round(max_m * 1000.0f): the product in float32, round() half away from zero, then the int16 wrap.  A
    max_m whose millimetre value does not fit int16 (above 32.767 m) therefore wraps: 40 m gives 40000 - 65536 =
    -25536, and every /5 value compares greater than that, so the whole image becomes 0."""
    mm = float(F(max_m) * F(1000.0))
    return int(wrap_i16(int(np.sign(mm) * np.floor(abs(mm) + 0.5))))


def dataset_depth(raw, fmt, max_m):
    """Raw 16-bit dataset depth -> int16 millimetres.

    fmt 0: millimetres already, the identity.

    fmt 1 (KITTI, depth * 256): `if (d > max_m * 256) d = 0; d = (int16)((float)d * (1000.0 / 256.0))`.
      The compare is float32 on (float)d against the float32 product max_m * 256 (float times int); d is an integer,
      so it is the integer rule d > floor(product).  It acts on the RAW value, before the scaling.  The factor is
      3.90625 = 125 / 32: |d| < 2^15 times 125 < 2^7 needs 22 bits, so the float32 product is exact for every int16
      and the result is trunc(d * 1000 / 256) toward zero, wrapped.  No tie exists.  Negative inputs are never cut
      (max_m >= 0) and scale to negative values (-1 -> -3.90625 -> -3).

    fmt 2 (TUM / ICL-NUIM, /5): `d = (int16)((float)d / 5.0); if (d > max_s) d = 0`.
      (float)d / 5.0 is a double quotient; where 5 does not divide d the exact quotient is at least 0.2 from an integer,
      2^37 times the double rounding, so the result is trunc(d / 5) toward zero exactly; |d / 5| <= 6553 never wraps.
      The compare is int16 against max_s = max_mm_short(max_m) and acts AFTER the scaling.  Negative inputs stay
      negative (-7 -> -1) and are cut only when max_s is below them, which takes a max_m beyond int16 (max_mm_short)."""
    raw = np.asarray(raw, np.int16)
    d = raw.astype(np.int64)
    if fmt == 0:
        return raw.copy()
    if fmt == 1:
        cut = int(np.floor(float(F(max_m) * F(256.0))))
        d = np.where(d > cut, 0, d)
        return wrap_i16(trunc_div(d * 1000, 256))
    if fmt == 2:
        q = trunc_div(d, 5)
        return wrap_i16(np.where(q > max_mm_short(max_m), 0, q))
    raise ValueError(fmt)


# ---------------------------------------------------------------------------------------------------------------------
# FloatDepthmapToShort (x1000) / FloatDepthmapToInt16 (x256)
# ---------------------------------------------------------------------------------------------------------------------
def depth_to_int16(depth_f32, scale):
    """(int16)(pixel * scale): float times int is a float32 product, truncated toward zero, through int32 into the low
    16 bits (wrap_i16).  Returns (image, tie): tie where the float64 product truncates to another integer than the
    float32 product (the single rounding carried the value across an integer)."""
    d = np.asarray(depth_f32, F)
    p32 = (d * F(scale)).astype(np.float64)
    p64 = d.astype(np.float64) * float(scale)
    return wrap_i16(np.trunc(p32).astype(np.int64)), np.trunc(p32) != np.trunc(p64)


# ---------------------------------------------------------------------------------------------------------------------
# depthPostProcessing
# ---------------------------------------------------------------------------------------------------------------------
def _gate_rule():
    """`float z = (float)raw / 1000.0; if (z < 0.005) continue;` -- the quotient is a double, rounded to float32 by the
    store, and the compare promotes it back to double.  float32(0.005) = 0.004999999888..., below the double 0.005, so
    raw 5 mm is SKIPPED although 5 / 1000.0 == 0.005 as doubles; float32(0.006) = 0.00600000005... passes.  The
    quotient is monotone, so the rule is: a raw value passes iff it is >= 6 (current depth, read signed: negatives
    never pass; previous depth, read unsigned: 0..5 are skipped and a negative int16 passes as 65.5 m)."""
    raw = np.arange(0, 65536, dtype=np.float64)
    passes = ~((raw / 1000.0).astype(F).astype(np.float64) < 0.005)
    assert not passes[:6].any() and passes[6:].all()
    return 6


GATE_MM = _gate_rule()

TIE_ROW, TIE_COL, TIE_RATIO, TIE_BEHIND = 1, 2, 4, 8  # reasons, or-ed per pixel


def depth_post_processing(curr, prev, Tpc, intr, threshold, area):
    """The pixel loop of DenseSlam.cpp:489-529 over whole images.  curr, prev: int16 [rows, cols]; Tpc: 4x4 (row-major
    numpy) previous-from-current; intr = (fx, fy, cx, cy).  Returns (blanked image, count, tie mask, reasons).

    As the text has it, for pixel (row, col):
      z = (float)((float)curr / 1000.0); skipped unless raw >= 6 (_gate_rule)
      X = z * (row - cx) * inv_fx,  Y = z * (col - cy) * inv_fy   -- ROW pairs with (cx, fx), COL with (cy, fy);
          float32, left to right; inv_fx = (float)(1.0 / fx)
      P = R (X, Y, z) + t: a cv::Mat product of CV_32F operands, accumulated in double and rounded to float32 once,
          then the translation added in float32
      row_u = (int)(fx * P0 * (1.0 / P2) + cx + 0.5): fx * P0 is float32, everything after it double; likewise col_v
      skipped if row_u < 1, col_v < 1, row_u >= rows or col_v >= cols  (the text's `< 0.1` and `(row_u + 1) > rows`
          on ints).  The double -> int conversion is undefined for NaN and outside int; the project's rule is
          saturation with NaN -> INT_MIN, so all of those fail this test.
      p = (float)((float)prev[row_u, col_v] / 1000.0) with prev read as UNSIGNED 16 bit; skipped unless raw >= 6
      diff = abs(p - P2) in float32 (the text writes abs() on a float; read as fabsf: DESIGN 4c)
      blanked iff diff / P2 > threshold (float32) and row > area * rows (int against float32: a float32 compare)
      count is incremented for every pixel that gets this far, blanked or not.

    Ties.  The float64 evaluation starts from the same float32 inputs (z, the previous depth, inv_fx, R, t, fx, cx:
    all of them values the text stores in floats) and differs from the float32 one by the roundings below; u is the
    unit roundoff 2^-24 and every bound is first order in u.
      X: the difference row - cx, two products: 3 roundings, |dX| <= 3 u |X|; the same for Y.
      P_k: the products and sums of the matrix row are double (2^-53: ignored), so they only carry dX and dY:
           3 u (|r_k0 X| + |r_k1 Y|); rounding the sum to float32: u |acc|; adding t_k: u |P_k|.  With
           M_k = |r_k0 X| + |r_k1 Y| + |r_k2 z| + |t_k|, which bounds each of the three magnitudes: |dP_k| <= 5 u M_k.
      P2 against 0: a tie (TIE_BEHIND) when |P2| <= 5 u M_2 in float64 -- unless both evaluations give exactly 0,
           which happens only when no operation rounded (R's third row a unit vector and t_z = -z); then the edge value
           itself is decided by the text (1.0 / 0 is infinite, the projection saturates) and the pixel is no tie.
      the projected coordinate c = fx P0 / P2 + cx + 0.5 before truncation: fx * P0 rounds once (u |fx P0|), the rest
           is double; dP0 and dP2 propagate as |fx| dP0 / |P2| and |fx P0| dP2 / P2^2:
           |dc| <= u |fx / P2| (6 M_0 + 5 M_2 |P0 / P2|)  (+ 2^-40 (|c| + 1) for the double operations).
           Truncation is toward zero and everything below 1 fails, so the edges are the integers 1 .. rows (1 .. cols):
           a tie (TIE_ROW / TIE_COL) when c lies within that margin of one of them.  Crossing an interior integer
           changes which previous pixel is read, crossing 1 or rows whether the pixel is counted at all.
      q = diff / P2 against the threshold: diff = |p - P2| carries dP2 and one rounding, the quotient dP2 again and one
           more: |dq| <= u (5 (M_2 / |P2|) (1 + |q|) + 2 |q|).  A tie (TIE_RATIO) when |q - threshold| is within it, on
           rows that pass the area test (elsewhere the outcome does not depend on q) -- unless both evaluations give
           exactly the threshold (again: nothing rounded, e.g. 1 m against 1.5 m at a threshold of 0.5); then the
           text's strict `>` decides and the pixel is kept.
    The area test and both gates are exact rules and have no tie.  The tie mask must contain every pixel at which the
    two evaluations take different decisions; refview_checks asserts that from the reference alone."""
    curr = np.asarray(curr, np.int16)
    prev_u = np.asarray(prev, np.int16).view(np.uint16)
    rows, cols = curr.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    inv_fx, inv_fy = F(1.0 / float(fx)), F(1.0 / float(fy))
    T = np.asarray(Tpc, F)
    R, t = T[:3, :3], T[:3, 3]
    thr = F(threshold)
    rr, cc = np.mgrid[0:rows, 0:cols]
    area_ok = rr.astype(F) > F(area) * F(rows)

    live = curr.astype(np.int64) >= GATE_MM
    z32 = (curr.astype(np.float64) / 1000.0).astype(F)
    z = z32.astype(np.float64)

    with np.errstate(all="ignore"):
        # float32, in the text's order
        X32 = (z32 * (rr.astype(F) - cx)) * inv_fx
        Y32 = (z32 * (cc.astype(F) - cy)) * inv_fy
        Xd, Yd = X32.astype(np.float64), Y32.astype(np.float64)
        P32 = [(float(R[k, 0]) * Xd + float(R[k, 1]) * Yd + float(R[k, 2]) * z).astype(F) + t[k] for k in range(3)]
        P2d = P32[2].astype(np.float64)
        c32 = [(f * P32[k]).astype(np.float64) * (1.0 / P2d) + float(c0) + 0.5 for k, f, c0 in ((0, fx, cx), (1, fy, cy))]
        # float64 from the same float32 inputs
        X64 = z * (rr - float(cx)) * float(inv_fx)
        Y64 = z * (cc - float(cy)) * float(inv_fy)
        P64 = [float(R[k, 0]) * X64 + float(R[k, 1]) * Y64 + float(R[k, 2]) * z + float(t[k]) for k in range(3)]
        M = [abs(float(R[k, 0])) * np.abs(X64) + abs(float(R[k, 1])) * np.abs(Y64) + abs(float(R[k, 2])) * z + abs(float(t[k]))
             for k in range(3)]
        c64 = [float(f) * P64[k] / P64[2] + float(c0) + 0.5 for k, f, c0 in ((0, fx, cx), (1, fy, cy))]
        mc = [U * np.abs(float(f) / P64[2]) * (6.0 * M[k] + 5.0 * M[2] * np.abs(P64[k] / P64[2])) + 2.0 ** -40 * (np.abs(c64[k]) + 1.0)
              for k, f in ((0, fx), (1, fy))]

    def decide(c, P2, lim):
        """(in bounds, index) of one projected coordinate: saturation makes NaN and anything outside int fail."""
        ok = np.isfinite(c) & (c >= 1.0) & (c < float(lim))
        return ok, np.where(ok, np.trunc(np.where(ok, c, 1.0)), 0).astype(np.int64)

    def outcome(c, P, lims):
        ok_r, iu = decide(c[0], P[2], lims[0])
        ok_c, iv = decide(c[1], P[2], lims[1])
        inb = live & ok_r & ok_c
        pr = prev_u[np.where(inb, iu, 0), np.where(inb, iv, 0)].astype(np.int64)
        counted = inb & (pr >= GATE_MM)
        return inb, iu, iv, pr, counted

    with np.errstate(all="ignore"):
        inb32, iu32, iv32, pr32, counted32 = outcome(c32, P32, (rows, cols))
        p32 = (pr32.astype(np.float64) / 1000.0).astype(F)
        q32 = np.abs(p32 - P32[2]) / P32[2]
        blank32 = counted32 & (q32 > thr) & area_ok

        inb64, iu64, iv64, pr64, counted64 = outcome(c64, P64, (rows, cols))
        p64 = (pr64.astype(np.float64) / 1000.0).astype(F).astype(np.float64)
        q64 = np.abs(p64 - P64[2]) / P64[2]
        blank64 = counted64 & (q64 > float(thr)) & area_ok
        mq = U * (5.0 * (M[2] / np.abs(P64[2])) * (1.0 + np.abs(q64)) + 2.0 * np.abs(q64))

        reasons = np.zeros((rows, cols), np.uint8)
        both_zero = (P2d == 0.0) & (P64[2] == 0.0)
        reasons |= np.where(live & ~both_zero & (np.abs(P64[2]) <= 5.0 * U * M[2]), TIE_BEHIND, 0).astype(np.uint8)
        for k, lim, bit in ((0, rows, TIE_ROW), (1, cols, TIE_COL)):
            near = np.isfinite(c64[k]) & (c64[k] >= 1.0 - mc[k]) & (c64[k] <= lim + mc[k])
            near &= np.abs(c64[k] - np.rint(c64[k])) <= mc[k]
            reasons |= np.where(live & near, bit, 0).astype(np.uint8)
        # the ratio decides only where the pixel is counted and its row can be blanked; a non-finite q64 there would
        # mean P2 = 0 in bounds, which the bounds test excludes
        near_q = (counted32 | counted64) & area_ok & (np.abs(q64 - float(thr)) <= mq)
        near_q &= ~((q32 == thr) & (q64 == float(thr)))  # both exactly on the edge: the text's strict > decides
        reasons |= np.where(near_q, TIE_RATIO, 0).astype(np.uint8)

    tie = reasons != 0
    differ = (counted32 != counted64) | (blank32 != blank64) | (counted32 & counted64 & ((iu32 != iu64) | (iv32 != iv64)))
    out = np.where(blank32, 0, curr).astype(np.int16)
    info = dict(live=live, inb=inb32, counted=counted32, blank=blank32, row_u=iu32, col_v=iv32, prev_raw=pr32,
                P2=P32[2], q=q32, area_ok=area_ok, differ=differ, c=c32)
    return out, int(counted32.sum()), tie, reasons, info


def depth_to_float32(mm, a=1.0 / 1000.0, b=0.0):
    """SURVEY A.3 in float32, as the text evaluates it: (float)d * a + b with the product rounded before the sum (the
    project builds every engine without fused multiply-add).  Equal to ref64.depth_to_float's float64 value rounded
    once whenever b = 0."""
    mm = np.asarray(mm, np.int64)
    v = mm.astype(F) * F(a) + F(b)
    return np.where((mm <= 0) | (mm > 32000), F(-1.0), v).astype(F)
