"""The semi-global stereo law of include/dslam_fusion.h in plain numpy, written from the text of the
law: grey, census, cost, the eight-path aggregation, selection with the uniqueness filter, the left-right check, the
sub-pixel step, and the float32 depth conversion.  All integers up to the conversion, so the device must give the same bytes."""
import numpy as np

INVALID, COST_OUT, MAX_SIZE, MAX_P2 = 0xFFFF, 63, 4096, 192
CENSUS_LEFT, CENSUS_RIGHT, WHAT_S = 0, 1, 2
DEFAULTS = dict(max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max=1, channels=1)
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))   # r = (dy, dx)
BIG = 1 << 20


def resolve(encoded=None):
    """The block's encoding -> what the law takes: 0 selects the default; uniqueness -1 -> 0 (off); lr_max -1 stays -1 (the
    check is off), -2 -> 0 (exact).  Raises ValueError for what dslam_stereo_create rejects."""
    p = dict(DEFAULTS)
    for key, value in (encoded or {}).items():
        if key not in DEFAULTS:
            raise KeyError(key)
        if value != 0:
            p[key] = int(value)
    ok = (p["max_disparity"] in (64, 128) and 1 <= p["p1"] <= p["p2"] <= MAX_P2 and -1 <= p["uniqueness"] <= 99
          and -2 <= p["lr_max"] <= p["max_disparity"] and p["channels"] in (1, 4))
    if not ok:
        raise ValueError(p)
    if p["uniqueness"] == -1:
        p["uniqueness"] = 0
    if p["lr_max"] == -2:
        p["lr_max"] = 0
    return p


def encode(max_disparity=None, p1=None, p2=None, uniqueness=None, lr_max=None, channels=None):
    """What the law takes (None: the default; uniqueness 0 = off; lr_max -1 = off, 0 = exact) -> the block's encoding."""
    return dict(max_disparity=max_disparity or 0, p1=p1 or 0, p2=p2 or 0,
                uniqueness=0 if uniqueness is None else (-1 if uniqueness == 0 else uniqueness),
                lr_max=0 if lr_max is None else (-2 if lr_max == 0 else lr_max), channels=channels or 0)


def grey(img, channels):
    img = np.asarray(img, dtype=np.uint8)
    if channels == 1:
        return img.reshape(img.shape[0], img.shape[1]).astype(np.int32)
    c = img.astype(np.int32)
    return (c[..., 0] + 2 * c[..., 1] + c[..., 2]) >> 2


def census(g):
    """uint64 [H, W]: 62 bits, 9 x 7 window, clamped coordinates, row-major neighbours, the centre skipped."""
    H, W = g.shape
    pad = np.pad(g, ((3, 3), (4, 4)), mode="edge")
    code = np.zeros((H, W), dtype=np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
            code = (code << np.uint64(1)) | (nb < g).astype(np.uint64)
    return code


def popcount64(v):
    return np.unpackbits(np.ascontiguousarray(v, dtype="<u8").view(np.uint8).reshape(v.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int32)


def cost(cl, cr, D):
    """int32 [H, W, D]"""
    H, W = cl.shape
    C = np.full((H, W, D), COST_OUT, dtype=np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount64(cl[:, d:] ^ cr[:, :W - d])
    return C


def _step(prev, c, p1, p2):
    """One step of the recurrence for a batch of lines: prev, c [N, D]."""
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, BIG)
    hi = np.full_like(prev, BIG)
    lo[:, 1:] = prev[:, :-1]
    hi[:, :-1] = prev[:, 1:]
    return c + np.minimum(np.minimum(prev, np.minimum(lo, hi) + p1), m + p2) - m


def path_costs(C, dy, dx, p1, p2):
    """L_r int32 [H, W, D] for r = (dy, dx)."""
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(L[:, x - dx], C[:, x], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]
            continue
        q = np.arange(W) - dx                       # the predecessor's column
        inside = (q >= 0) & (q < W)
        row = C[y].copy()
        row[inside] = _step(L[y - dy][q[inside]], C[y][inside], p1, p2)
        L[y] = row
    return L


def aggregate(C, p1, p2, each=False):
    """S = the sum of the eight L_r, int32 [H, W, D] (each: the list of the eight as well)."""
    Ls = [path_costs(C, dy, dx, p1, p2) for dy, dx in DIRECTIONS]
    S = sum(Ls)
    return (S, Ls) if each else S


def right_disparity(S):
    """dR int32 [H, W]: argmin_d S(y, xr + d, d) over xr + d < W, the smallest d on ties."""
    H, W, D = S.shape
    R = np.full((H, W, D), np.iinfo(np.int64).max, dtype=np.int64)
    for d in range(min(D, W)):
        R[:, :W - d, d] = S[:, d:, d]
    return R.argmin(axis=2).astype(np.int32)


def select(S, uniqueness, lr_max):
    """Steps 5-7 on S [H, W, D] (any integer type): uint16 [H, W] in 1/16 pixel, INVALID where rejected."""
    S = np.asarray(S).astype(np.int64)
    H, W, D = S.shape
    d = np.arange(D)
    ds = S.argmin(axis=2)
    s0 = np.take_along_axis(S, ds[..., None], axis=2)[..., 0]
    far = np.abs(d[None, None, :] - ds[..., None]) > 1
    s2 = np.where(far, S, np.iinfo(np.int64).max // 256).min(axis=2)
    reject = s2 * (100 - uniqueness) < s0 * 100
    x = np.arange(W)[None, :]
    xr = x - ds
    reject |= xr < 0
    if lr_max >= 0:
        dR = right_disparity(S)
        at = np.take_along_axis(dR, np.clip(xr, 0, W - 1), axis=1)
        reject |= np.abs(at - ds) > lr_max
    sm = np.take_along_axis(S, np.clip(ds - 1, 0, D - 1)[..., None], axis=2)[..., 0]
    sp = np.take_along_axis(S, np.clip(ds + 1, 0, D - 1)[..., None], axis=2)[..., 0]
    den = sm + sp - 2 * s0
    step = (ds > 0) & (ds < D - 1) & (den > 0)
    delta = np.where(step, (16 * (sm - sp) + den) // np.where(step, 2 * den, 1), 0)   # numpy's // is the floor
    d16 = 16 * ds + delta
    return np.where(reject, INVALID, d16).astype(np.uint16)


def match(left, right, params=None, each=False):
    """params: what resolve() returns (or None).  dict(census_left, census_right, S uint16, disp uint16 [, L: the eight])."""
    p = dict(DEFAULTS) if params is None else params
    cl, cr = census(grey(left, p["channels"])), census(grey(right, p["channels"]))
    C = cost(cl, cr, p["max_disparity"])
    out = dict(census_left=cl, census_right=cr)
    if each:
        S, out["L"] = aggregate(C, p["p1"], p["p2"], each=True)
    else:
        S = aggregate(C, p["p1"], p["p2"])
    out["S"] = S.astype(np.uint16)
    out["disp"] = select(S, p["uniqueness"], p["lr_max"])
    return out


def depth_mm(d16, focal_length_px, baseline_m, scale, min_depth_m, max_depth_m):
    """Step 8 in float32, operation by operation: int16, 0 where there is no depth."""
    F = np.float32
    if F(max_depth_m) * F(1000.0) >= F(32767.0):
        raise ValueError("max_depth_m * 1000 >= 32767")
    d16 = np.asarray(d16, dtype=np.uint16)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        disp = d16.astype(F) * F(0.0625)
        z = (F(focal_length_px) * F(baseline_m)) / disp
        mm_f = (F(1000.0) * F(scale)) * z
        fits = mm_f < F(2147483648.0)
        mm = np.where(fits, mm_f, F(0)).astype(np.int32)
    lo, hi = int(np.int32(F(min_depth_m) * F(1000.0))), int(np.int32(F(max_depth_m) * F(1000.0)))
    none = (d16 == INVALID) | (d16 == 0) | ~fits | (mm > hi) | (mm < lo)
    return np.where(none, 0, mm).astype(np.int16)
