"""The overlap survey and the pair selection stated from the text: the survey in numpy with float32
element operations in the stated order and integer shifts, the selection in plain Python.  Shares no text with the engine.

Survey.  N maps, each a hash table (analytic_maps.HASH_ENTRY_DTYPE, `num_buckets` bucket heads followed by the excess
area) with T_i: world -> map i, 4 x 4 in metres, taken as float32.  For every ordered pair (s, d), s != d:
X~_sd = T~_d inv(T~_s) by section 15's pair transform (ref64_register_graph.pair_transform: float64, translation in voxels,
the stated scalar order), its 12 entries rounded to float32.  A resident block of s (an entry with ptr >= 0) at block
position B has 8 octant centres c = 8 B + (1.5 + 4 ox, 1.5 + 4 oy, 1.5 + 4 oz); q = X~ c with each row evaluated as
((a x + b y) + c z) + d in float32 (an X~ that rounds to the identity: q = c); cell = (int)floor(q), D = cell >> 3; the
octant is shared when every component of D lies in [-32768, 32767] and map d holds a resident entry at D, found by the
bucket-plus-excess-chain lookup.  A q that no int holds is not shared.
"""
import numpy as np

import analytic_maps as am
import ref64_register as rr
import ref64_register_graph as rg

MAX_REGISTER_PAIRS = 128
DEFAULT_MIN_SHARED = 64

OCTANTS = np.array([[1.5 + 4.0 * (o & 1), 1.5 + 4.0 * ((o >> 1) & 1), 1.5 + 4.0 * (o >> 2)] for o in range(8)], np.float32)


class Table:
    """A map as the survey sees it: the hash table and where its excess area begins."""

    def __init__(self, table, num_buckets):
        self.table, self.num_buckets = np.asarray(table), int(num_buckets)

    @classmethod
    def of_map(cls, m):
        return cls(m.hash, m.num_buckets)

    @classmethod
    def of_scene(cls, api, scene):
        return cls(api.download_hash_table(scene), scene.params.num_buckets)

    def resident_blocks(self):
        return self.table["pos"][self.table["ptr"] >= 0].astype(np.int64)

    def holds(self, D):
        """Whether a resident entry sits at each block position D [n, 3] (int64, every component within int16): the
        bucket of D's hash, then the excess chain, every probe walking in step."""
        D = np.asarray(D, np.int64)
        idx = am.hash_index(D, self.num_buckets)
        found = np.zeros(len(D), bool)
        walking = np.ones(len(D), bool)
        for _ in range(len(self.table) + 1):
            if not walking.any():
                break
            e = self.table[idx]
            hit = walking & np.all(e["pos"].astype(np.int64) == D, axis=-1) & (e["ptr"] >= 0)
            found |= hit
            walking &= ~hit & (e["offset"] >= 1)
            idx = np.where(walking, self.num_buckets + e["offset"].astype(np.int64) - 1, idx)
        return found


def pair_transforms32(T, vs):
    """X~_sd rounded to float32, [N, N, 3, 4] (the diagonal is left as zeros: nothing is probed there)."""
    Tt = np.stack([rr.voxel_transform(np.asarray(t, np.float32).astype(np.float64), float(np.float32(vs))) for t in T])
    n = len(Tt)
    X = np.zeros((n, n, 3, 4), np.float32)
    for s in range(n):
        for d in range(n):
            if s != d:
                X[s, d] = rg.pair_transform(Tt, s, d).astype(np.float32)
    return X


def shared_mask(src, dst, X32):
    """[blocks of src, 8] bool: which octants of src's resident blocks are shared with dst under X32 [3, 4] float32."""
    B = src.resident_blocks()
    c = ((B * 8).astype(np.float32)[:, None, :] + OCTANTS[None]).reshape(-1, 3)   # exact
    X32 = np.asarray(X32, np.float32)
    identity = np.array_equal(X32, np.eye(4, dtype=np.float32)[:3])
    if identity:
        q = c
    else:
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        q = np.stack([((X32[r, 0] * x + X32[r, 1] * y) + X32[r, 2] * z) + X32[r, 3] for r in range(3)], -1)
        assert q.dtype == np.float32
    with np.errstate(invalid="ignore"):
        f = np.floor(q)
        fits = np.isfinite(f) & (np.abs(f) < 2147483648.0)          # an int holds it
    cell = np.where(fits, f, 0.0).astype(np.int64)
    D = cell >> 3
    ok = np.all(fits & (D >= -32768) & (D <= 32767), axis=-1)
    shared = np.zeros(len(c), bool)
    if ok.any():
        shared[ok] = dst.holds(D[ok])
    return shared.reshape(-1, 8)


def survey(tables, T, vs):
    """(live [N], shared_blocks [N, N], shared_octants [N, N]) int64; rows are sources."""
    n = len(tables)
    X = pair_transforms32(T, vs)
    live = np.array([int((t.table["ptr"] >= 0).sum()) for t in tables], np.int64)
    blocks, octants = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for s in range(n):
        for d in range(n):
            if s == d:
                blocks[s, d], octants[s, d] = live[s], 8 * live[s]
                continue
            m = shared_mask(tables[s], tables[d], X[s, d])
            blocks[s, d], octants[s, d] = int(m.any(axis=1).sum()), int(m.sum())
    return live, blocks, octants


# ---------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------
def kept_pairs(live, shared, min_shared, one_direction):
    """Steps 1 and 2: (the qualifying pairs, the pairs kept), both by (s, d) ascending."""
    n = len(live)
    qualifying = [(s, d) for s in range(n) for d in range(n) if s != d and int(shared[s][d]) >= min_shared]
    if not one_direction:
        return qualifying, list(qualifying)
    q = set(qualifying)
    kept = []
    for s, d in qualifying:
        if (d, s) in q:
            a, b = min(s, d), max(s, d)
            keep_ab = int(shared[a][b]) * int(live[b]) >= int(shared[b][a]) * int(live[a])   # (a tie keeps (a, b))
            if (s, d) != ((a, b) if keep_ab else (b, a)):
                continue
        kept.append((s, d))
    return qualifying, kept


def select(live, shared, min_shared_octants=0, one_direction=0, max_pairs=0):
    """dslam_select_register_pairs: (pairs as a list of (s, d), component [N], dict(qualifying, selected, num_components),
    and -- for the tests -- the pairs pass 1 took)."""
    n = len(live)
    min_shared = min_shared_octants or DEFAULT_MIN_SHARED
    max_pairs = max_pairs or MAX_REGISTER_PAIRS
    assert n - 1 <= max_pairs <= MAX_REGISTER_PAIRS
    qualifying, kept = kept_pairs(live, shared, min_shared, one_direction)
    # 3. components of the qualifying pairs, undirected: the smallest index of each
    component = list(range(n))
    changed = True
    while changed:
        changed = False
        for s, d in qualifying:
            low = min(component[s], component[d])
            if component[s] != low or component[d] != low:
                component[s] = component[d] = low
                changed = True
    # 4. the cap
    ranked = sorted(kept, key=lambda p: (-int(shared[p[0]][p[1]]), p[0], p[1]))
    sets = [{i} for i in range(n)]
    where = list(range(n))
    pass1 = []
    for s, d in ranked:
        if where[s] != where[d]:
            gone = where[d]
            sets[where[s]] |= sets[gone]
            for i in sets[gone]:
                where[i] = where[s]
            pass1.append((s, d))
    taken = list(pass1)
    for p in ranked:
        if len(taken) >= max_pairs:
            break
        if p not in pass1:
            taken.append(p)
    pairs = sorted(taken)
    return pairs, component, dict(qualifying=len(kept), selected=len(pairs), num_components=len(set(component))), pass1
