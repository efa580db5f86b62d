"""The law of the sharded re-integration (include/dslam_fusion.h, "sharded re-integration"), stated on
sets of voxel-block slots in plain numpy: who owns a slot, what a voxel-writing call may change on a replica, which slots
a call marks, and what plan, pack and unpack do with the marks.  Nothing here walks the pool in the engine's "virtual"
order or in the oracle's loop order: a shard's list is `the dirty slots it owns, sorted`.

A pool is an array of shape (N, ...) whose first axis is the slot; a block is 512 voxels of 8 bytes = 4096 bytes."""
import numpy as np

BLOCK_BYTES = 4096
MAX_SHARDS = 64


def owner(slot, shards, chunk):
    return (np.asarray(slot, np.int64) // chunk) % shards


def owned(slot, shard=0, shards=1, chunk=1, first=0, count=-1):
    """Both gates: dslam_scene_set_shard(shard, shards, chunk) and dslam_scene_set_shard_range(first, count)."""
    slot = np.asarray(slot, np.int64)
    shard_gate = np.ones(slot.shape, bool) if shards <= 1 else owner(slot, shards, chunk) == shard
    range_gate = np.ones(slot.shape, bool) if count < 0 else (slot >= first) & (slot < first + count)
    return shard_gate & range_gate


def effect(before, unsharded_after, **gates):
    """A replica's pool after a voxel-writing call: the unsharded result in the blocks it owns, its old bytes elsewhere."""
    own = owned(np.arange(len(before)), **gates)
    out = before.copy()
    out[own] = unsharded_after[own]
    return out


def marks(ptr, ids, pos_now=None, pos_stored=None):
    """Slots one call marks: the resident blocks of the entries it lists.  For a list stored with a keyframe (pos_stored:
    one block position per listed entry) the entry must still hold the block it held then."""
    ids = np.asarray(ids, np.int64)
    p = np.asarray(ptr, np.int64)[ids]
    keep = p >= 0
    if pos_stored is not None:
        keep &= (np.asarray(pos_now)[ids] == np.asarray(pos_stored)).all(-1)
    return set(int(v) for v in p[keep])


def valid_layout(n, shards, chunk):
    return 1 <= shards <= MAX_SHARDS and chunk >= 1 and n % (shards * chunk) == 0


def plan(dirty, n, shards, chunk):
    """Per shard the ascending list of its dirty slots, and their lengths."""
    if not valid_layout(n, shards, chunk):
        raise ValueError((n, shards, chunk))
    d = np.array(sorted(dirty), np.int64)
    assert len(d) == 0 or (d[0] >= 0 and d[-1] < n)
    who = owner(d, shards, chunk)
    lists = [d[who == r] for r in range(shards)]
    return lists, [len(x) for x in lists]


def pack(voxels, lists, r, cap):
    """The first min(count_r, cap) blocks of shard r's list, in list order."""
    return voxels[lists[r][:max(min(len(lists[r]), cap), 0)]]


def unpack(voxels, lists, skip, recv, stride):
    """recv: (shards, stride, ...).  Every shard but `skip` puts the first min(count_r, stride) blocks of its row in place."""
    out = voxels.copy()
    for r, slots in enumerate(lists):
        if r == skip:
            continue
        k = max(min(len(slots), stride), 0)
        out[slots[:k]] = recv[r, :k]
    return out
