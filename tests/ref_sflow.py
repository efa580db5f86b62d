"""The sparse scene-flow law of dslam_sflow_* (include/dslam_fusion.h) in numpy, all integer.

It restates what libviso2's Matcher returns from getRawMatches() after two pushBack calls and matchFeatures(method) without a
motion prior; tests/golden/sflow_*.npz hold that library's own output, and test_sflow_ref.py holds this file to it.

One simplification against the header's wording, which the device does not share (it walks the bins): find_match here does
not visit bins.  A candidate inside the window lies in a bin inside the clamped bin range, because floor(x / binsize) and the
clamps are monotone in x; so the bin range excludes nothing the window admits, and all that the bins decide is the ORDER in
which candidates are met: bin column, then bin row, then feature index.  That order is the tie rule."""
import numpy as np

MARGIN = 9
MAX_SIZE = 4096
MAX_NMS_N = 32
MAX_BINS = 65536
MAX_FEATURES = 1 << 22
MAX_COST = 32 * 255
FEATURE_WORDS = 12
FEATURE_BYTES = 48
MATCH_WORDS = 12
IMAGE_1C, IMAGE_2C, IMAGE_1P, IMAGE_2P = 0, 1, 2, 3
FILTER_DU, FILTER_DV, FILTER_F1, FILTER_F2 = 0, 1, 2, 3
SOBEL_BOUND, CHECKER_BOUND, BLOB_BOUND = 12240, 2040, 4080

DEFAULTS = dict(nms_n=3, nms_tau=50, match_binsize=50, match_radius=200, match_disp_tolerance=2, half_resolution=1, channels=1)
# the descriptor: 16 (dx, dy) taps, du then dv at each
TAPS = ((-3, -1), (-3, 1), (-1, -1), (-1, 1), (3, -1), (3, 1), (1, -1), (1, 1),
        (-1, -5), (-1, 5), (1, -5), (1, 5), (-5, -3), (-5, 3), (5, -3), (5, 3))


def resolve(encoded):
    """The ABI's block (0 = default, half_resolution -1 = off) -> the values the law takes."""
    p = dict(DEFAULTS)
    for k, v in encoded.items():
        if k not in DEFAULTS:
            raise ValueError(k)
        if v != 0:
            p[k] = v
    if p["half_resolution"] == -1:
        p["half_resolution"] = 0
    if p["nms_n"] > MAX_NMS_N:
        raise ValueError("nms_n")
    if p["nms_n"] < 1 or p["nms_tau"] < 1 or p["match_binsize"] < 1 or p["match_radius"] < 1 or p["match_disp_tolerance"] < 1:
        raise ValueError("nms_n, nms_tau, match_binsize, match_radius and match_disp_tolerance must be positive")
    if p["half_resolution"] not in (0, 1) or p["channels"] not in (1, 4):
        raise ValueError("half_resolution is 1 or -1 (off); channels is 1 or 4")
    return p


def encode(**effective):
    """The block that selects these effective values."""
    e = dict(effective)
    if "half_resolution" in e:
        e["half_resolution"] = 1 if e["half_resolution"] else -1
    return e


def check_size(width, height, p):
    """What dslam_sflow_create rejects beyond the parameters themselves."""
    s = 2 if p["half_resolution"] else 1
    if not (s <= width <= MAX_SIZE and s <= height <= MAX_SIZE):
        raise ValueError("size")
    if 4 * bins_of(width, p["match_binsize"]) * bins_of(height, p["match_binsize"]) > MAX_BINS:
        raise ValueError("bins")
    if 4 * num_cells(width // s, height // s, p["nms_n"]) > MAX_FEATURES:
        raise ValueError("features")


def sparse_n(nms_n):
    n = 3 * nms_n
    return max(nms_n, 10) if n > 10 else n


def bins_of(size, binsize):
    return -(-size // binsize)


def cells_along(size, n):
    """The cells start at n + 9, step n + 1, while start < size - n - 9."""
    return max(0, -(-(size - 2 * n - 2 * MARGIN) // (n + 1)))


def num_cells(w, h, n):
    return cells_along(w, n) * cells_along(h, n)


def grey(img, channels):
    img = np.asarray(img)
    if channels == 1:
        return img.astype(np.int32).reshape(img.shape[0], img.shape[1])
    c = img.astype(np.int32)
    return (c[..., 0] + 2 * c[..., 1] + c[..., 2]) >> 2


def matching_image(g, half_resolution):
    if not half_resolution:
        return g
    h, w = g.shape[0] // 2, g.shape[1] // 2
    g = g[:2 * h, :2 * w]
    return (g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2]) >> 2


def _cols(g, k):
    h = g.shape[0]
    return sum(k[i] * g[i:h - 4 + i, :] for i in range(5) if k[i])


def _rows(t, k):
    w = t.shape[1]
    return sum(k[i] * t[:, i:w - 4 + i] for i in range(5) if k[i])


def filters(m):
    """du, dv (uint8), f1, f2 (int16) of a matching image: the law on the interior 2 <= x <= w - 3, 2 <= y <= h - 3, zero
    outside it (the reference leaves those pixels undefined and never reads them)."""
    h, w = m.shape
    du, dv = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    f1, f2 = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    if w < 5 or h < 5:
        return du, dv, f1, f2
    m = m.astype(np.int32)
    smooth, deriv = (1, 4, 6, 4, 1), (1, 2, 0, -2, -1)
    su, sv = _rows(_cols(m, smooth), deriv), _rows(_cols(m, deriv), smooth)
    assert max(np.abs(su).max(), np.abs(sv).max()) <= SOBEL_BOUND
    du[2:-2, 2:-2] = np.clip((su >> 7) + 128, 0, 255)
    dv[2:-2, 2:-2] = np.clip((sv >> 7) + 128, 0, 255)
    box5 = _rows(_cols(m, (1, 1, 1, 1, 1)), (1, 1, 1, 1, 1))
    box3 = _rows(_cols(m, (0, 1, 1, 1, 0)), (0, 1, 1, 1, 0))
    blob = -box5 + 2 * box3 + 7 * m[2:-2, 2:-2]
    step = (1, 1, 0, -1, -1)
    checker = _rows(_cols(m, step), step)
    assert np.abs(blob).max() <= BLOB_BOUND and np.abs(checker).max() <= CHECKER_BOUND
    f1[2:-2, 2:-2] = blob
    f2[2:-2, 2:-2] = checker
    return du, dv, f1, f2


def _first_extremum(cell, sign):
    """Position (di, dj) of the first strict extremum of a cell scanned column by column; cell is indexed [row, column]."""
    c = (sign * cell).T            # [column, row]: C order is the scan order
    k = int(np.argmax(c))          # the first of equal maxima
    return k // c.shape[1], k % c.shape[1]


def nms(f1, f2, n, tau):
    """[(u, v, class)] in the reference's order: cell column outermost, then cell row, then class."""
    h, w = f1.shape
    out = []
    fs = (f1.astype(np.int32), f2.astype(np.int32))
    for i in range(n + MARGIN, w - n - MARGIN, n + 1):
        for j in range(n + MARGIN, h - n - MARGIN, n + 1):
            for c in range(4):
                f, sign = fs[c >> 1], (1 if c & 1 else -1)
                di, dj = _first_extremum(f[j:j + n + 1, i:i + n + 1], sign)
                u, v = i + di, j + dj
                val = sign * f[v, u]
                hood = sign * f[v - n:min(v + n, h - 1 - MARGIN) + 1, u - n:min(u + n, w - 1 - MARGIN) + 1]
                # nothing of the cell itself beats its extremum, so a better value anywhere in the hood is outside the cell
                if hood.max() > val:
                    continue
                if val >= tau:
                    out.append((u, v, c))
    return out


def feature_records(du, dv, maxima, s):
    rec = np.zeros((len(maxima), FEATURE_WORDS), np.int32)
    desc = rec.view(np.uint8).reshape(len(maxima), FEATURE_BYTES)
    for k, (u, v, c) in enumerate(maxima):
        rec[k, :4] = (u * s, v * s, 0, c)
        for t, (dx, dy) in enumerate(TAPS):
            desc[k, 16 + 2 * t] = du[v + dy, u + dx]
            desc[k, 17 + 2 * t] = dv[v + dy, u + dx]
    return rec


def image_features(img, p):
    """{'filters': (du, dv, f1, f2), 0: sparse records, 1: dense records} of one image."""
    m = matching_image(grey(img, p["channels"]), p["half_resolution"])
    du, dv, f1, f2 = filters(m)
    s = 2 if p["half_resolution"] else 1
    out = {"filters": (du, dv, f1, f2)}
    for which, n in ((0, sparse_n(p["nms_n"])), (1, p["nms_n"])):
        out[which] = feature_records(du, dv, nms(f1, f2, n, p["nms_tau"]), s)
    return out


def bin_of(x, binsize, nbins):
    return np.minimum(np.asarray(x) // binsize, nbins - 1)


class Target:
    """A feature set as find_match sees it."""

    def __init__(self, rec, width, height, binsize):
        self.rec = rec
        self.desc = rec.view(np.uint8).reshape(len(rec), FEATURE_BYTES)[:, 16:].astype(np.int32)
        ub, vb = bin_of(rec[:, 0], binsize, bins_of(width, binsize)), bin_of(rec[:, 1], binsize, bins_of(height, binsize))
        order = np.lexsort((np.arange(len(rec)), vb, ub))     # bin column, bin row, index
        self.rank = np.empty(len(rec), np.int64)
        self.rank[order] = np.arange(len(rec))


def find_match(query, target, flow, p):
    """The index in target.rec of the best candidate for the record `query`; 0 when there is none."""
    radius = p["match_radius"] // 2 if p["half_resolution"] else p["match_radius"]
    rv = radius if flow else p["match_disp_tolerance"]
    t = target.rec
    if len(t) == 0:
        return 0
    ok = (t[:, 3] == query[3]) & (np.abs(t[:, 0] - query[0]) <= radius) & (np.abs(t[:, 1] - query[1]) <= rv)
    if not ok.any():
        return 0
    qd = query.view(np.uint8)[16:].astype(np.int32)
    cost = np.abs(target.desc - qd).sum(axis=1)
    key = np.where(ok, cost * (1 << 32) + target.rank, np.iinfo(np.int64).max)
    return int(np.argmin(key))


def match(sets, method, width, height, p):
    """sets: {IMAGE_*: records of the chosen set}.  int32 [n, 12] match records."""
    need = {0: (IMAGE_1P, IMAGE_1C), 1: (IMAGE_1C, IMAGE_2C), 2: (IMAGE_1P, IMAGE_2P, IMAGE_1C, IMAGE_2C)}[method]
    if any(len(sets[i]) == 0 for i in need):
        return np.zeros((0, MATCH_WORDS), np.int32)
    T = {i: Target(sets[i], width, height, p["match_binsize"]) for i in need}
    out, taken = [], set()
    if method == 2:
        for i1p, q in enumerate(sets[IMAGE_1P]):
            i2p = find_match(q, T[IMAGE_2P], False, p)
            i2c = find_match(sets[IMAGE_2P][i2p], T[IMAGE_2C], True, p)
            i1c = find_match(sets[IMAGE_2C][i2c], T[IMAGE_1C], False, p)
            back = find_match(sets[IMAGE_1C][i1c], T[IMAGE_1P], True, p)
            a, b, c, d = q, sets[IMAGE_2P][i2p], sets[IMAGE_1C][i1c], sets[IMAGE_2C][i2c]
            if back == i1p and a[0] >= b[0] and c[0] >= d[0]:
                out.append((a[0], a[1], i1p, b[0], b[1], i2p, c[0], c[1], i1c, d[0], d[1], i2c))
    else:
        other = IMAGE_2C if method == 1 else IMAGE_1P
        flow = method == 0
        for i1c, q in enumerate(sets[IMAGE_1C]):
            io = find_match(q, T[other], flow, p)
            o = sets[other][io]
            if find_match(o, T[IMAGE_1C], flow, p) != i1c or (method == 1 and q[0] < o[0]):
                continue
            if (q[0], q[1]) in taken:       # one match per current-left pixel: the first in index order
                continue
            taken.add((q[0], q[1]))
            rec = [-1] * 12
            rec[6:9] = (q[0], q[1], i1c)
            rec[(9 if method == 1 else 0):(12 if method == 1 else 3)] = (o[0], o[1], io)
            out.append(tuple(rec))
    return np.array(out, np.int32).reshape(len(out), MATCH_WORDS)


class Matcher:
    """The two-frame ring of dslam_sflow_push and the calls on it."""

    def __init__(self, width, height, encoded=None):
        self.p = resolve(encoded or {})
        check_size(width, height, self.p)
        self.w, self.h = width, height
        self.cur = self.prev = None

    def _image(self, img):
        if img is None:
            e = np.zeros((0, FEATURE_WORDS), np.int32)
            return {"filters": None, 0: e, 1: e}
        shape = (self.h, self.w) if self.p["channels"] == 1 else (self.h, self.w, 4)
        return image_features(np.asarray(img, np.uint8).reshape(shape), self.p)

    def push(self, left, right=None, replace=False):
        if not replace:
            self.prev = self.cur
        self.cur = (self._image(left), self._image(right))

    def features(self, image, which):
        frame = self.cur if image in (IMAGE_1C, IMAGE_2C) else self.prev
        if frame is None:
            return np.zeros((0, FEATURE_WORDS), np.int32)
        return frame[image & 1][which]

    def filter_images(self, side):
        return self.cur[side]["filters"]

    def match(self, method, which):
        sets = {i: self.features(i, which) for i in range(4)}
        if which == 0:   # the reference checks the dense sets before its first pass, and returns nothing without them
            need = {0: (IMAGE_1P, IMAGE_1C), 1: (IMAGE_1C, IMAGE_2C), 2: (0, 1, 2, 3)}[method]
            if any(len(self.features(i, 1)) == 0 for i in need):
                return np.zeros((0, MATCH_WORDS), np.int32)
        return match(sets, method, self.w, self.h, self.p)
