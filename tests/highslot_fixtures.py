"""Maps whose voxel blocks sit in pool slots above 2 GiB and near 4 GiB, and a map state free of slot names.

Every kernel reaches a block through its pool slot `ptr`, at byte 4096 * ptr of the voxel pool.  The fixtures here put a
map's blocks into three bands of a pool of POOL = DSLAM_MAX_LOCAL_BLOCKS slots: the lowest slots, the slots either side
of M31 (byte 2^31, where a signed 32-bit byte offset turns negative) and the highest slots (the last bytes below 2^32,
where an unsigned one ends).  The law the tests build on them: no result depends on which slots hold the blocks.

Nothing here holds a host array of the whole voxel pool (4 GiB): a relocated map keeps its blocks' voxels and their slots,
and voxels travel one contiguous run of slots at a time.  The int32 lists that are one word per slot (allocation list,
last_seen: 4 MiB each) are handled whole."""
import copy

import numpy as np

import analytic_maps as am

POOL = 0x100000      # DSLAM_MAX_LOCAL_BLOCKS: 4 GiB of voxels
M31 = 0x80000        # the slot at byte 2^31
TOP = POOL - 1
MIN_BAND, MIN_SIDE, MIN_CROSS_PAIRS = 8, 8, 20


def band_of(slots, n, pool=POOL):
    """0 low [0, n), 1 around the middle mark [pool/2 - n, pool/2 + n), 2 top [pool - n, pool), -1 elsewhere."""
    s = np.asarray(slots, np.int64)
    mid = pool // 2
    out = np.full(s.shape, -1, np.int64)
    out[(s >= 0) & (s < n)] = 0
    out[(s >= mid - n) & (s < mid + n)] = 1
    out[(s >= pool - n) & (s < pool)] = 2
    return out


def banded_slots(n_blocks, pool=POOL):
    """(slots [n_blocks] in the order of allocation, n): allocation k takes lane k % 4 -- low upwards from 0, below the
    middle mark downwards from pool/2 - 1, above it upwards from pool/2, top downwards from pool - 1 -- so the bands are
    [0, n), [pool/2 - n, pool/2 + n), [pool - n, pool) with n = ceil(n_blocks / 4), the extreme slots go first, and
    consecutive allocations never share a band."""
    n = -(-n_blocks // 4)
    assert 4 * n <= pool // 4, "the bands must not meet"
    k = np.arange(n_blocks, dtype=np.int64)
    j, lane = k // 4, k % 4
    mid = pool // 2
    slots = np.choose(lane, [j, mid - 1 - j, mid + j, pool - 1 - j])
    return slots, n


def banded_alloc_list(n_blocks, pool=POOL):
    """A full allocation list (a permutation of 0 .. pool - 1, last_free = pool - 1) whose top n_blocks entries -- the
    first n_blocks allocations, taken from the top down -- are banded_slots; below them every other slot, ascending."""
    slots, _ = banded_slots(n_blocks, pool)
    free = np.ones(pool, bool)
    free[slots] = False
    out = np.empty(pool, np.int32)
    out[:pool - n_blocks] = np.nonzero(free)[0]
    out[pool - n_blocks:] = slots[::-1]
    return out


def relocate(m, pool=POOL):
    """Map `m` (analytic_maps.Map) with block i, the i-th allocation, in slot banded_slots[i] of a pool of `pool` blocks:
    the same table with the new slot names, the allocation list that leaves, no `vba`."""
    n = len(m.block_pos)
    slots, _ = banded_slots(n, pool)
    assert np.array_equal(m.ptrs, m.num_local_blocks - 1 - np.arange(n)), "the map's blocks are not its first allocations"
    r = copy.copy(m)
    r.hash = m.hash.copy()
    live = r.hash["ptr"] >= 0
    r.hash["ptr"][live] = slots[m.num_local_blocks - 1 - m.hash["ptr"][live].astype(np.int64)]
    r.ptrs = slots
    r.num_local_blocks = pool
    r.alloc_list = banded_alloc_list(n, pool)
    r.last_free = pool - 1 - n
    r.vba = None                      # upload_sparse is the only way in
    r.upload = upload_sparse          # (what ref64_checks.load_map and check_mesh call)
    return r


def slot_runs(slots):
    """[(first, count, places)]: the slots as maximal runs of consecutive numbers; `places` indexes `slots`, ascending."""
    slots = np.asarray(slots, np.int64)
    order = np.argsort(slots, kind="stable")
    s = slots[order]
    assert len(s) == 0 or (np.diff(s) > 0).all(), "a slot is named twice"
    cuts = np.nonzero(np.diff(s) != 1)[0] + 1
    return [(int(s[p[0]]), len(p), order[p]) for p in np.split(np.arange(len(s)), cuts) if len(p)]


def upload_sparse(api, scene, m):
    """Map `m` into a fresh scene: table and lists, then the blocks one contiguous slot run at a time."""
    assert scene.params.num_local_blocks == m.num_local_blocks
    api.upload_scene_state(scene, m.hash, m.alloc_list, m.last_free, m.excess_list, m.last_free_ex)
    for first, count, places in slot_runs(m.ptrs):
        api.upload_voxel_blocks(scene, first, m.voxels[places])


def download_blocks(api, scene, slots):
    """The voxel blocks in `slots` ([n] -> [n, 512]), downloaded by slot run."""
    out = np.empty((len(slots), 512), am.VOXEL_DTYPE)
    for first, count, places in slot_runs(slots):
        out[places] = api.download_voxel_blocks(scene, first, count)
    return out


def upload_blocks(api, scene, slots, voxels):
    """voxels [n, 512] into `slots` [n], by slot run."""
    voxels = np.ascontiguousarray(voxels).view(am.VOXEL_DTYPE).reshape(len(slots), 512)
    for first, count, places in slot_runs(slots):
        api.upload_voxel_blocks(scene, first, voxels[places])


class SparsePool:
    """Some slots of a pool, indexed by slot as the laws of ref_shard.py index a whole-pool array: pool[slots] reads,
    pool[slots] = rows writes (voxel records or their uint64 words), copy() copies.  Rows are kept as 512 uint64."""

    def __init__(self, slots, rows):
        self.slots = np.asarray(slots, np.int64)
        assert (np.diff(self.slots) > 0).all()
        self.rows = np.ascontiguousarray(rows).view(np.uint64).reshape(len(self.slots), 512)

    def _at(self, slots):
        slots = np.asarray(slots, np.int64)
        at = np.searchsorted(self.slots, slots)
        assert (at < len(self.slots)).all() and np.array_equal(self.slots[at], slots), "a slot this pool does not hold"
        return at

    def __getitem__(self, slots):
        return self.rows[self._at(slots)]

    def __setitem__(self, slots, rows):
        at = self._at(slots)
        self.rows[at] = np.ascontiguousarray(rows).view(np.uint64).reshape(len(at), 512)

    def copy(self):
        return SparsePool(self.slots, self.rows.copy())

    def upload(self, api, scene):
        upload_blocks(api, scene, self.slots, self.rows)

    @classmethod
    def download(cls, api, scene, slots):
        return cls(slots, download_blocks(api, scene, slots))


def canonical(api, scene, rs=None):
    """The map state with no slot named: the table with ptr >= 0 replaced by 0 (live; -1 swapped out and -2 empty stay),
    per live entry in table order its 4 KiB and last_seen; the free excess stack; the counters (blocks in use instead of
    last_free_block_id).  Asserts that the live slots and the free part of the allocation list partition the pool."""
    st = api.stats(scene, rs)
    nl = scene.params.num_local_blocks
    h = api.download_hash_table(scene)
    live = h["ptr"] >= 0
    slots = h["ptr"][live].astype(np.int64)
    lf = st["last_free_block_id"]
    free = api.download_allocation_list(scene)[:lf + 1].astype(np.int64)
    assert len(slots) + len(free) == nl, f"{len(slots)} live + {len(free)} free slots in a pool of {nl}"
    assert free.min(initial=0) >= 0 and free.max(initial=0) < nl and slots.max(initial=0) < nl, "a slot outside the pool"
    seen = np.zeros(nl, bool)
    seen[slots] = True
    seen[free] = True
    assert seen.all(), "live and free slots do not partition the pool"
    flags = h.copy()
    flags["ptr"][live] = 0
    counters = {k: v for k, v in st.items() if k not in ("last_free_block_id", "num_allocated_blocks")}
    counters["blocks_in_use"] = nl - 1 - lf
    out = dict(table=flags, blocks=download_blocks(api, scene, slots), last_seen=api.download_last_seen(scene)[slots],
               excess=api.download_excess_list(scene)[:st["last_free_excess_id"] + 1], counters=counters, slots=slots)
    if scene.params.use_swapping:
        out["swap_states"] = api.download_swap_states(scene)
    if rs is not None:
        out["visible_ids"] = api.download_visible_ids(rs)
        out["visible_types"] = api.download_visible_types(rs)
    return out


def assert_same_canonical(a, b, what=""):
    """Byte for byte; `slots` is the one part that may differ."""
    assert a["counters"] == b["counters"], f"{what}: counters {a['counters']} != {b['counters']}"
    for k in sorted(set(a) | set(b)):
        if k in ("counters", "slots"):
            continue
        assert k in a and k in b, f"{what}: {k} on one side only"
        if k == "blocks":
            va, vb = a[k].view(np.uint64), b[k].view(np.uint64)
            assert va.shape == vb.shape, f"{what}: {len(va)} against {len(vb)} live blocks"
            bad = np.argwhere(va != vb)
            assert not len(bad), (f"{what}: {len(bad)} voxels differ, first in live block {bad[0][0]} (slots "
                                  f"{a['slots'][bad[0][0]]:#x} / {b['slots'][bad[0][0]]:#x}) voxel {bad[0][1]}")
        else:
            assert a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape, f"{what}: {k} differs"


def teeth(block_pos, slots, pool=POOL):
    """Asserts that the blocks at `block_pos` [n, 3] in `slots` [n] exercise the marks: MIN_BAND blocks in each band,
    MIN_SIDE on each side of the middle mark, MIN_CROSS_PAIRS face-adjacent pairs whose slots lie in different bands.
    The bands are as wide as banded_slots makes them for this many blocks.  Returns the figures."""
    pos = np.asarray(block_pos, np.int64)
    slots = np.asarray(slots, np.int64)
    n = -(-len(slots) // 4)
    band = band_of(slots, n, pool)
    per_band = [int((band == b).sum()) for b in range(3)]
    assert min(per_band) >= MIN_BAND, f"blocks per band {per_band}"
    below = int(((band == 1) & (slots < pool // 2)).sum())
    above = int(((band == 1) & (slots >= pool // 2)).sum())
    assert min(below, above) >= MIN_SIDE, f"{below} blocks below and {above} above the middle mark"
    where = {tuple(p): b for p, b in zip(pos.tolist(), band.tolist())}
    cross = 0
    for p, b in where.items():
        for axis in range(3):
            q = list(p)
            q[axis] += 1
            bq = where.get(tuple(q))
            cross += bq is not None and b >= 0 and bq >= 0 and bq != b
    assert cross >= MIN_CROSS_PAIRS, f"{cross} face-adjacent pairs across bands"
    ext = dict(slot0=bool((slots == 0).any()), below_mark=bool((slots == pool // 2 - 1).any()),
               at_mark=bool((slots == pool // 2).any()), top=bool((slots == pool - 1).any()))
    return dict(per_band=per_band, below=below, above=above, cross_pairs=int(cross), **ext)


def scene_teeth(api, scene, pool=POOL):
    """`teeth` of a scene's live blocks as the engine placed them."""
    h = api.download_hash_table(scene)
    live = h["ptr"] >= 0
    return teeth(h["pos"][live], h["ptr"][live], pool)
