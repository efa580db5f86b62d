"""Seeded inputs of the stereo tests: random uint8 pairs, the random-dot stereogram, and crafted S volumes that reach the
corners of the selection (ref_stereo.select) no image pair reaches on demand."""
import functools

import numpy as np

import ref_stereo as rs

BIG_S = 2000   # a cost no crafted minimum comes near; within S's range (8 * 255 = 2040)


def random_pair(W, H, channels=1, seed=0):
    """Two independent random images: every stage still has a definite answer, and nearly every tie-break is exercised."""
    rng = np.random.default_rng([seed, W, H, channels])
    shape = (H, W) if channels == 1 else (H, W, 4)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


def shifted_pair(W, H, shift, channels=1, seed=0):
    """A random left image and the right image of a fronto-parallel plane at disparity `shift`: right(x) = left(x + shift),
    random bytes where nothing maps; a little of the left image is then disturbed so that costs are not all 0."""
    rng = np.random.default_rng([seed, W, H, shift, channels])
    shape = (H, W) if channels == 1 else (H, W, 4)
    left = rng.integers(0, 256, shape, dtype=np.uint8)
    right = rng.integers(0, 256, shape, dtype=np.uint8)
    if shift < W:
        right[:, :W - shift] = left[:, shift:]
    noise = rng.random(shape) < 0.1
    left = np.where(noise, rng.integers(0, 256, shape, dtype=np.uint8), left)
    return left, right


def stereogram(W, H, D, seed=0):
    """(left, right, disparity int [H, W], visible bool [H, W]): three horizontal bands D/16, D/16 + 2, D/16 + 4 and a box of
    disparity D/2 over rows H/4 .. 3H/4, columns W/2 .. 7W/8; the right image painted far to near, holes random."""
    rng = np.random.default_rng([seed, W, H, D])
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    disp = np.empty((H, W), dtype=np.int64)
    for i, b in enumerate(np.array_split(np.arange(H), 3)):
        disp[b] = D // 16 + 2 * i
    disp[H // 4:3 * H // 4, W // 2:7 * W // 8] = D // 2
    owner = np.full((H, W), -1, dtype=np.int64)   # the left column painted last at each right pixel
    ys, xs = np.mgrid[0:H, 0:W]
    for d in np.unique(disp):                     # ascending disparity = far to near
        sel = (disp == d) & (xs - d >= 0)
        right[ys[sel], xs[sel] - d] = left[sel]
        owner[ys[sel], xs[sel] - d] = xs[sel]
    xr = xs - disp
    visible = (xr >= 0) & (np.take_along_axis(owner, np.clip(xr, 0, W - 1), axis=1) == xs)
    return left, right, disp, visible


@functools.lru_cache(maxsize=None)
def reference(kind, W, H, seed=0, **encoded):
    """ref_stereo.match of a fixture pair under the encoded parameters, computed once per session and shared (read only)."""
    p = rs.resolve(encoded)
    if kind == "random":
        left, right = random_pair(W, H, p["channels"], seed)
    elif kind == "shifted":
        left, right = shifted_pair(W, H, 5, p["channels"], seed)
    else:
        raise KeyError(kind)
    out = rs.match(left, right, p)
    out["left"], out["right"] = left, right
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- crafted S volumes: (name, S uint16 [H, W, D], what the case is for) --------------------------------------------
def flat(W, D, H=1):
    return np.full((H, W, D), BIG_S, dtype=np.uint16)


def crafted(D):
    """{name: (S, uniqueness, lr_max)}.  The volumes are W = D + 8 wide (one row, but for floor_residues), so x - d* >= 0 can hold for every d*."""
    W = D + 8
    X = D + 4          # a column at which every d* is reachable
    out = {}

    def one(name, fill, u=0, lr=-1):
        S = flat(W, D)
        fill(S)
        out[name] = (S, u, lr)

    # ties of the minimum: the smaller d wins
    for a in (0, D // 2, D - 2):
        def tie(S, a=a):
            S[0, X, a] = S[0, X, a + 1] = 100
        one(f"tie_{a}_{a + 1}", tie)
    # d* at either end: no sub-pixel step whatever the neighbours are
    one("end_0", lambda S: S[0, X, :2].__setitem__(slice(None), (100, 130)))
    one("end_last", lambda S: S[0, X, D - 2:].__setitem__(slice(None), (130, 100)))
    # a plateau of three: d* is its first d, the sub-pixel step its largest (den == 0 itself cannot arise: it needs
    # S(d* - 1) == s0, and the smallest d wins ties)
    one("plateau", lambda S: S[0, X, 9:12].__setitem__(slice(None), (100, 100, 100)))
    # sm - sp negative, over many (den, sm - sp): every residue of the floor division that den admits, the exact negative
    # quotients among them ((13, 19), (11, 21): num = -64, -128 over 2 den = 64); one pixel per pair, d* = 11
    pairs = [(a, b) for a in range(6) for b in range(a + 1, a + 13)] + [(15, 17), (13, 19), (11, 21)]
    cols = list(range(20, W))
    rows = -(-len(pairs) // len(cols))
    S = flat(W, D, rows)
    for i, (a, b) in enumerate(pairs):
        S[i // len(cols), cols[i % len(cols)], 10:13] = (100 + a, 100, 100 + b)
    out["floor_residues"] = (S, 0, -1)
    # uniqueness: s2 (100 - u) == 100 s0 and one either side, u = 20: s0 = 80, s2 = 100 (equal: kept), 99 (rejected), 101
    def uniq(S):
        for i, s2 in enumerate((100, 99, 101)):
            S[0, X - 3 * i, 30] = 80
            S[0, X - 3 * i, 29] = S[0, X - 3 * i, 31] = 81    # the neighbours do not count
            S[0, X - 3 * i, 40] = s2
    one("uniqueness_edge", uniq, u=20)
    # x - d* < 0
    one("left_of_image", lambda S: S[0, 5, 9:12].__setitem__(slice(None), (120, 100, 130)))
    # a right-image minimum tied between two d: pixel xr sees S(xr + 3, 3) == S(xr + 7, 7); dR = 3.  The left pixels xr + 3 and
    # xr + 7 choose d* = 3 and 7: with lr_max = 1 the first passes, the second does not
    def right_tie(S):
        xr = 40
        S[0, xr + 3, 3] = 100
        S[0, xr + 7, 7] = 100
    one("right_tie", right_tie, lr=1)
    one("right_tie_exact", right_tie, lr=0)
    one("right_tie_wide", right_tie, lr=D)
    return out


def random_S(W, H, D, seed=0, levels=12):
    """Few distinct values, so ties everywhere; 70 % of the pixels also have a valley at a disparity their row shares, so the
    left-right check has something to pass."""
    rng = np.random.default_rng([seed, W, H, D])
    S = rng.integers(100, 100 + levels, (H, W, D))
    ys, xs = np.nonzero(rng.random((H, W)) < 0.7)
    S[ys, xs, 7 + ys % 3] = 90
    return S.astype(np.uint16)
