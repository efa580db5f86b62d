"""The law of the fern keyframe index (include/dslam_fusion.h) in numpy and Python integers: fern
table, thumbnails, code, dissimilarity, query order, harvest rule.  Written from the statement of the law alone; it shares no
text with the C side.  Everything is an integer, so the device has to give exactly these numbers."""
import numpy as np

MAX_MATCHES = 64
MAX_QUERIES = 64
CODE_DWORDS = 64
MASK64 = (1 << 64) - 1

DEFAULTS = dict(num_ferns=512, cell=8, channels=1, depth_min_mm=300, depth_max_mm=10000, seed=0)


def resolve(params=None):
    """The parameters with 0 replaced by the default (seed has none)."""
    p = dict(DEFAULTS)
    for key, value in (params or {}).items():
        if key == "seed" or value != 0:
            p[key] = int(value)
    assert p["num_ferns"] % 8 == 0 and 8 <= p["num_ferns"] <= 512
    assert 1 <= p["cell"] <= 32 and p["channels"] in (1, 2)
    assert p["depth_min_mm"] <= p["depth_max_mm"] <= 32767
    return p


class SplitMix64:
    def __init__(self, seed):
        self.state = seed & MASK64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)


def thumb_size(width, height, cell):
    return width // cell, height // cell


def table(params, width, height):
    """int32 [F, 4, 3]: (cell, channel, threshold) per decision, drawn fern by fern, decision by decision."""
    p = resolve(params)
    tw, th = thumb_size(width, height, p["cell"])
    assert tw * th >= 1
    rng = SplitMix64(p["seed"])
    out = np.zeros((p["num_ferns"], 4, 3), dtype=np.int32)
    for f in range(p["num_ferns"]):
        for j in range(4):
            cell = rng.next() % (tw * th)
            channel = (rng.next() & 1) if p["channels"] == 2 else 0
            if channel == 0:
                threshold = p["depth_min_mm"] + rng.next() % (p["depth_max_mm"] - p["depth_min_mm"] + 1)
            else:
                threshold = rng.next() % 255
            out[f, j] = (cell, channel, threshold)
    return out


def thumbnails(depth_mm, rgba, cell):
    """(D, G): int64 [TH, TW] each.  depth_mm: int16 [H, W]; rgba: uint8 [H, W, 4] or None (G is then zero)."""
    depth = np.asarray(depth_mm).astype(np.int64)
    height, width = depth.shape
    tw, th = thumb_size(width, height, cell)
    used = depth[:th * cell, :tw * cell].reshape(th, cell, tw, cell)
    valid = used > 0
    n = valid.sum(axis=(1, 3))
    total = np.where(valid, used, 0).sum(axis=(1, 3))
    D = np.where(2 * n >= cell * cell, total // np.maximum(n, 1), 0)
    G = np.zeros_like(D)
    if rgba is not None:
        c = np.asarray(rgba).astype(np.int64)
        assert c.shape[:2] == depth.shape
        grey = c[..., 0] + 2 * c[..., 1] + c[..., 2]
        G = grey[:th * cell, :tw * cell].reshape(th, cell, tw, cell).sum(axis=(1, 3)) // (4 * cell * cell)
    return D, G


def code_from_thumbnails(tab, D, G):
    """uint32 [64]: fern f in dword f // 8, bits 4 (f % 8) .. 4 (f % 8) + 3."""
    values = np.stack([D.ravel(), G.ravel()])
    bits = values[tab[..., 1], tab[..., 0]] > tab[..., 2]          # [F, 4]
    nibbles = (bits.astype(np.int64) << np.arange(4)).sum(axis=1)  # [F]
    out = np.zeros(CODE_DWORDS, dtype=np.uint64)
    for f, nib in enumerate(nibbles):
        out[f // 8] |= np.uint64(int(nib) << (4 * (f % 8)))
    return out.astype(np.uint32)


def encode(params, depth_mm, rgba=None, tab=None):
    p = resolve(params)
    height, width = np.asarray(depth_mm).shape
    if tab is None:
        tab = table(p, width, height)
    D, G = thumbnails(depth_mm, rgba if p["channels"] == 2 else None, p["cell"])
    return code_from_thumbnails(tab, D, G)


def nibbles_of(code, num_ferns=512):
    code = np.asarray(code, dtype=np.uint32)
    return ((code[..., :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).reshape(code.shape[:-1] + (512,))[..., :num_ferns]


def dissimilarity(a, b, num_ferns=512):
    """The ferns f < F whose nibbles differ."""
    return int((nibbles_of(a, num_ferns) != nibbles_of(b, num_ferns)).sum())


class Index:
    """The index of the law: codes in order of insertion, query and harvest rule."""

    def __init__(self, capacity, num_ferns=512):
        self.capacity, self.num_ferns = capacity, num_ferns
        self.codes = []

    @property
    def count(self):
        return len(self.codes)

    def distances(self, code):
        if not self.codes:
            return np.zeros(0, dtype=np.int64)
        return (nibbles_of(np.stack(self.codes), self.num_ferns) != nibbles_of(code, self.num_ferns)).sum(axis=1)

    def query(self, code, first_id, last_id, k, dist=None):
        """[(id, dissimilarity)] of the first k candidates of [first_id, last_id) n [0, count).  dist: distances(code), if
        the caller already has them."""
        assert 1 <= k <= MAX_MATCHES and 0 <= first_id <= last_id
        lo, hi = min(first_id, self.count), min(last_id, self.count)
        if dist is None:
            dist = self.distances(code)
        order = lo + np.argsort(dist[lo:hi], kind="stable")     # stable: equal dissimilarities stay in id order
        return [(int(i), int(dist[i])) for i in order[:k]]

    def process(self, code, harvest_min_dissimilarity, first_id, last_id, k):
        """(matches, added id or -1, full): the query, then the harvest rule over ALL stored ids."""
        assert harvest_min_dissimilarity >= 0
        matches = self.query(code, first_id, last_id, k)
        dist = self.distances(code)
        want = self.count == 0 or int(dist.min()) >= harvest_min_dissimilarity
        if not want:
            return matches, -1, False
        if self.count >= self.capacity:
            return matches, -1, True
        self.codes.append(np.asarray(code, dtype=np.uint32).copy())
        return matches, self.count - 1, False

    def reset(self):
        self.codes = []
