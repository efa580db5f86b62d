"""Inputs of the shard tests (law: ref_shard.py; check bodies: refshard_checks.py).  They let a test CHOOSE the set D of
dirty slots through calls the ABI already has: a crafted hash table gives every slot an entry, an uploaded visible list
names the entries of D, and an integration of an all-zero depth image marks them without changing a voxel.  Signature
blocks make a packed buffer name its slots; send and recv buffers carry guard blocks at both ends."""
import numpy as np

import ref_shard as rs_law

PATTERN = 0xA5            # guard and untouched-capacity bytes of a send buffer
PADDING = 0x5A            # a recv row behind its shard's last block: nothing may read it
GUARD = 2                 # guard blocks at each end of a buffer
TILE = 1024               # slots per workgroup of the ordered compaction (4 per thread, 256 threads)
NUM_BUCKETS, NUM_EXCESS = 0x1000, 0x100

LAYOUTS = {          # name -> (N, shards, chunk)
    "0x300-2x1": (0x300, 2, 1),
    "0x300-3x256": (0x300, 3, 256),
    "0x300-64x4": (0x300, 64, 4),          # 12 slots per shard: less than a wavefront
    "0x900-3x16": (0x900, 3, 16),          # 2.25 compaction tiles
    "0x900-9x256": (0x900, 9, 256),
    "0x800-64x1": (0x800, 64, 1),
    "0x300-1xN": (0x300, 1, 0x300),
}
# what each layout is there for, asserted from the law alone when a fixture is built
PER_SHARD_OFF_256 = {"0x300-2x1", "0x300-64x4", "0x800-64x1"}
SEVERAL_TILES = {"0x900-3x16", "0x900-9x256", "0x800-64x1"}
PARTIAL_LAST_TILE = {"0x900-3x16", "0x900-9x256"}

DIRTY_SETS = ("empty", "one", "ends", "one_chunk", "all", "last_shard_only", "first_shard_only", "third")


def assert_layout_reach(layout):
    n, shards, chunk = LAYOUTS[layout]
    assert rs_law.valid_layout(n, shards, chunk)
    if layout in PER_SHARD_OFF_256:
        assert (n // shards) % 256 != 0
    if layout in SEVERAL_TILES:
        assert n > TILE
    if layout in PARTIAL_LAST_TILE:
        assert n % TILE != 0


def is_hip(api):
    return api.prefix == "dslam_"


def sync(api):
    """The HIP engine works on a stream of its own; the oracle has nothing to wait for."""
    if is_hip(api):
        api.synchronize()


def dirty_set(name, n, shards, chunk):
    slots = np.arange(n)
    if name == "empty":
        return set()
    if name == "one":
        return {n // 3}
    if name == "ends":
        return {0, n - 1}
    if name == "one_chunk":
        c = (n // chunk) // 2
        return set(range(c * chunk, (c + 1) * chunk))
    if name == "all":
        return set(range(n))
    if name == "last_shard_only":      # every other shard, with a count of 0, sits in front of it
        return set(int(s) for s in slots[rs_law.owner(slots, shards, chunk) == shards - 1])
    if name == "first_shard_only":     # ... and here behind it
        return set(int(s) for s in slots[rs_law.owner(slots, shards, chunk) == 0])
    if name == "third":
        rng = np.random.default_rng(n * 131 + shards * 7 + chunk)
        return set(int(s) for s in rng.choice(n, n // 3, replace=False))
    raise ValueError(name)


def signatures(n, replica):
    """(n, 512) uint64: voxel v of block s on replica q holds q << 48 | s << 16 | v."""
    s = np.arange(n, dtype=np.uint64)[:, None]
    v = np.arange(512, dtype=np.uint64)[None, :]
    return (np.uint64(replica) << np.uint64(48)) | (s << np.uint64(16)) | v


def decode(blocks):
    """(replica, slot) of each signature block; asserts that every block is one whole signature."""
    blocks = np.ascontiguousarray(blocks).view(np.uint64).reshape(-1, 512)
    q = (blocks[:, 0] >> np.uint64(48)).astype(np.int64)
    s = ((blocks[:, 0] >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    want = (blocks[:, :1] & ~np.uint64(0xFFFF)) | np.arange(512, dtype=np.uint64)[None, :]
    assert np.array_equal(blocks, want), "a packed block is not one whole block of the pool"
    return q, s


def as_voxels(pkg, u64):
    return np.ascontiguousarray(u64).view(pkg.VOXEL_DTYPE).reshape(-1, 512)


class Buffer:
    """`blocks` blocks of 4096 bytes between two guards: a torch tensor on the device for the HIP engine, a numpy array for
    the oracle.  Offsets count blocks from the end of the front guard."""

    def __init__(self, api, blocks):
        self.blocks, self.total = blocks, blocks + 2 * GUARD
        self.hip = is_hip(api)
        if self.hip:
            import torch
            self.torch = torch
            self.t = torch.empty((self.total, rs_law.BLOCK_BYTES), dtype=torch.uint8, device="cuda")
        else:
            self.a = np.empty((self.total, rs_law.BLOCK_BYTES), np.uint8)

    @property
    def ptr(self):
        base = self.t.data_ptr() if self.hip else self.a.ctypes.data
        return base + GUARD * rs_law.BLOCK_BYTES

    def fill(self, byte):
        if self.hip:
            self.t.fill_(byte)
            self.torch.cuda.synchronize()
        else:
            self.a.fill(byte)

    def load(self, body):
        """body: (blocks, 4096) uint8, placed behind the front guard."""
        body = np.ascontiguousarray(body).view(np.uint8).reshape(-1, rs_law.BLOCK_BYTES)
        assert len(body) == self.blocks
        if self.hip:
            self.t[GUARD:GUARD + self.blocks].copy_(self.torch.from_numpy(body))
            self.torch.cuda.synchronize()
        else:
            self.a[GUARD:GUARD + self.blocks] = body

    def host(self, lo=0, hi=None):
        """Rows lo .. hi of the WHOLE buffer, guards included."""
        hi = self.total if hi is None else hi
        return self.t[lo:hi].cpu().numpy() if self.hip else self.a[lo:hi].copy()

    def guards_intact(self, byte):
        return bool((self.host(0, GUARD) == byte).all() and (self.host(self.total - GUARD) == byte).all())


class Crafted:
    """A scene of N slots whose table gives every slot one entry (in a seeded order that is not the slot order) and holds
    two entries without a block (ptr -1 and -2), a render state and a view whose depth image is all zero."""

    def __init__(self, api, pkg, layout):
        self.api, self.pkg, self.name = api, pkg, layout
        self.n, self.shards, self.chunk = n, shards, chunk = LAYOUTS[layout]
        assert rs_law.valid_layout(n, shards, chunk)
        self.per_shard = n // shards
        assert_layout_reach(layout)
        self.W, self.H = 16, 12
        p = pkg.SceneParams(voxel_size=0.02, mu=0.08, max_w=100, frustum_min=0.2, frustum_max=3.0, num_local_blocks=n,
                            num_buckets=NUM_BUCKETS, num_excess=NUM_EXCESS, history_words=1)
        self.scene = api.create_scene(p)
        self.rs = api.create_render_state(self.scene, self.W, self.H)
        self.view = api.create_view(self.W, self.H)
        api.view_update(self.view, np.zeros((self.H, self.W, 4), np.uint8), np.zeros((self.H, self.W), np.int16))
        rng = np.random.default_rng(n + 1000 * shards + chunk)
        table = api.download_hash_table(self.scene)
        assert (table["ptr"] < -1).all()
        where = rng.choice(NUM_BUCKETS, n + 2, replace=False)
        self.entry_of_slot = where[:n].astype(np.int64)
        self.no_block = where[n:].astype(np.int64)
        table["ptr"][self.entry_of_slot] = np.arange(n)
        table["ptr"][self.no_block] = (-1, -2)
        # block positions: distinct, a few blocks in front of an identity camera
        k = np.arange(n + 2)
        table["pos"][where] = np.stack([k % 16 - 8, (k // 16) % 16 - 8, 10 + k // 256], 1)
        # checked on the CPU before anything is uploaded: an out-of-range ptr would index the pool out of bounds on the device
        ptr = table["ptr"].astype(np.int64)
        used = ptr[ptr >= 0]
        assert len(used) == n and np.array_equal(np.sort(used), np.arange(n)), "ptr values must be distinct and in 0 .. N-1"
        assert (ptr >= -2).all() and (ptr < n).all()
        self.table = table
        api.upload_scene_state(self.scene, hash_table=table, allocation_list=np.zeros(n, np.int32), last_free_block_id=-1)
        self.M = np.eye(4, dtype=np.float32)
        self.intr = np.array([20.0, 20.0, 7.5, 5.5], np.float32)

    def upload_signatures(self, replica):
        pool = signatures(self.n, replica)
        self.api.upload_voxel_blocks(self.scene, 0, as_voxels(self.pkg, pool))
        return pool

    def pool(self):
        return self.api.download_voxel_blocks(self.scene).view(np.uint64).reshape(self.n, 512)

    def mark(self, dirty, seed=0):
        """track_dirty(1), then two integrations of the zero depth image over lists that between them name the entries of
        `dirty` (shuffled) and the two entries without a block.  No voxel may change."""
        api = self.api
        before = self.pool()
        api.track_dirty(self.scene, True)
        ids = np.concatenate([self.entry_of_slot[sorted(dirty)], self.no_block]).astype(np.int32)
        np.random.default_rng(seed + len(ids)).shuffle(ids)
        assert (ids >= 0).all() and (ids < self.scene.n_entries).all()
        for part in (ids[:len(ids) // 2], ids[len(ids) // 2:]):
            assert len(part) <= self.n
            api.upload_visible_ids(self.rs, part)
            api.integrate_into_scene(self.scene, self.view, self.rs, self.M, self.intr)
        assert np.array_equal(self.pool(), before), "marking changed a voxel"


def other_layout(n, shards, chunk):
    """A second valid layout of the same pool, for the plan that must NOT govern."""
    return (2, 1) if (shards, chunk) != (2, 1) else (1, n)
