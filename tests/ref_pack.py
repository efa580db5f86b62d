"""The packed-map law of DESIGN.md section 21 in plain numpy, written from the law and not from any kernel:
pack(state) -> bytes and unpack(bytes, params) -> state.

A state is what util.snapshot downloads plus the scene's geometry:
    hash         [num_buckets + num_excess] HASH_ENTRY_DTYPE
    voxels       [num_local_blocks, 512] of 8-byte voxels (any 8-byte dtype)
    alloc_list   [num_local_blocks] int32        last_free_block_id
    excess_list  [num_excess] int32              last_free_excess_id
    last_seen    [num_local_blocks] int32        (unpack only: as a reset leaves it)
    params       num_buckets, num_excess, num_local_blocks, voxel_size, mu
Every value is an integer or a bit pattern, so nothing here has a tolerance.
"""
import struct
from types import SimpleNamespace

import numpy as np

from refmap import HASH_ENTRY_DTYPE

HEADER = struct.Struct("<4sI4i2I2q3h3hI")   # magic, version, buckets, excess, n, f, voxel_size, mu, offsets, bbox, 0
assert HEADER.size == 64
EMPTY_VOXEL = np.uint64(0x7FFF)             # sdf = 32767, everything else 0
MAGIC, VERSION = b"DSPK", 1


class PackError(ValueError):
    pass


def layout(n, f):
    """(blocks_offset, total_bytes) of a packed map of n blocks and f free excess slots."""
    end = 64 + 16 * n + 4 * f
    blocks_offset = -(-end // 4096) * 4096
    return blocks_offset, blocks_offset + 4096 * n


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def geometry(params):
    return SimpleNamespace(num_buckets=int(params.num_buckets), num_excess=int(params.num_excess),
                           num_local_blocks=int(params.num_local_blocks), voxel_size=float(np.float32(params.voxel_size)),
                           mu=float(np.float32(params.mu)))


def state_of(snap, params, last_seen=None):
    """A state from a util.snapshot."""
    st = dict(hash=snap["hash"], voxels=snap["voxels"], alloc_list=snap["alloc_list"], excess_list=snap["excess_list"],
              last_free_block_id=int(snap["stats"]["last_free_block_id"]),
              last_free_excess_id=int(snap["stats"]["last_free_excess_id"]), params=geometry(params))
    if last_seen is not None:
        st["last_seen"] = last_seen
    return st


def header_fields(raw):
    """The header of a packed map as a dict; PackError if it is none: magic, version, counts, the layout identities."""
    if len(raw) < 64:
        raise PackError("shorter than a header")
    magic, version, nb, nx, n, f, vs, mu, off, total, l0, l1, l2, h0, h1, h2, zero = HEADER.unpack(bytes(raw[:64]))
    if magic != MAGIC or version != VERSION or zero != 0:
        raise PackError("magic, version or reserved word")
    if nb < 0 or nx < 0 or n < 0 or f < 0 or f > nx:
        raise PackError("counts")
    if (off, total) != layout(n, f):
        raise PackError("layout")
    return dict(num_buckets=nb, num_excess=nx, blocks=n, free_excess=f, voxel_size_bits=vs, mu_bits=mu, blocks_offset=off,
                total_bytes=total, bbox_min=[l0, l1, l2], bbox_max=[h0, h1, h2])


def pack(state, params=None):
    p = geometry(params if params is not None else state["params"])
    h = np.asarray(state["hash"])
    ranks = np.nonzero(h["ptr"] >= 0)[0]          # the resident entries, ascending by hash index
    n, f = len(ranks), int(state["last_free_excess_id"]) + 1
    blocks_offset, total = layout(n, f)
    out = bytearray(total)                        # (the padding is zeros)
    pos = h["pos"][ranks].astype(np.int64).reshape(n, 3)
    lo = pos.min(axis=0) if n else [32767] * 3
    hi = pos.max(axis=0) if n else [-32768] * 3
    out[:64] = HEADER.pack(MAGIC, VERSION, p.num_buckets, p.num_excess, n, f, f32_bits(p.voxel_size), f32_bits(p.mu),
                           blocks_offset, total, *(int(v) for v in lo), *(int(v) for v in hi), 0)
    rec = np.zeros(n, HASH_ENTRY_DTYPE)
    rec["pos"], rec["offset"], rec["ptr"] = h["pos"][ranks], h["offset"][ranks], ranks
    out[64:64 + 16 * n] = rec.tobytes()
    out[64 + 16 * n:64 + 16 * n + 4 * f] = np.asarray(state["excess_list"], "<i4")[:f].tobytes()
    vox = np.ascontiguousarray(state["voxels"]).view(np.uint64).reshape(-1, 512)
    out[blocks_offset:total] = vox[h["ptr"][ranks]].tobytes()
    return bytes(out)


def unpack(raw, params):
    """The state an unpack leaves in a scene of `params`; PackError for what it rejects."""
    p = geometry(params)
    hd = header_fields(raw)
    n, f, N = hd["blocks"], hd["free_excess"], p.num_local_blocks
    if (hd["num_buckets"], hd["num_excess"]) != (p.num_buckets, p.num_excess):
        raise PackError("table geometry")
    if (hd["voxel_size_bits"], hd["mu_bits"]) != (f32_bits(p.voxel_size), f32_bits(p.mu)):
        raise PackError("voxel_size or mu")
    if n > N or len(raw) < hd["total_bytes"]:
        raise PackError("pool or buffer too small")
    raw = bytes(raw)
    rec = np.frombuffer(raw, HASH_ENTRY_DTYPE, n, 64)
    free = np.frombuffer(raw, "<i4", f, 64 + 16 * n)
    idx = rec["ptr"].astype(np.int64)
    n_entries = p.num_buckets + p.num_excess
    if ((idx < 0) | (idx >= n_entries)).any() or (np.diff(idx) <= 0).any():
        raise PackError("record indices")
    if ((rec["offset"] < 0) | (rec["offset"] > p.num_excess)).any() or ((free < 0) | (free >= p.num_excess)).any():
        raise PackError("offsets or free list")
    h = np.zeros(n_entries, HASH_ENTRY_DTYPE)
    h["ptr"] = -2
    slots = N - 1 - np.arange(n)
    h["pos"][idx], h["offset"][idx], h["ptr"][idx] = rec["pos"], rec["offset"], slots
    vox = np.full((N, 512), EMPTY_VOXEL, np.uint64)
    vox[slots] = np.frombuffer(raw, "<u8", 512 * n, hd["blocks_offset"]).reshape(n, 512)
    excess = np.arange(p.num_excess, dtype=np.int32)
    excess[:f] = free
    return dict(hash=h, voxels=vox, alloc_list=np.arange(N, dtype=np.int32), last_free_block_id=N - 1 - n,
                excess_list=excess, last_free_excess_id=f - 1, last_seen=np.full(N, -1, np.int32), params=p,
                stats=dict(last_free_block_id=N - 1 - n, last_free_excess_id=f - 1, decayed_block_count=0, slid_block_count=0,
                           frame_counter=0, fusion_fifo_len=0, defusion_fifo_len=0, alloc_failures=0))


def as_function(state):
    """The map as a function: block position -> (entry index, offset, the block's 512 voxels as bytes)."""
    h = np.asarray(state["hash"])
    vox = np.ascontiguousarray(state["voxels"]).view(np.uint64).reshape(-1, 512)
    return {tuple(int(c) for c in h["pos"][t]): (int(t), int(h["offset"][t]), vox[h["ptr"][t]].tobytes())
            for t in np.nonzero(h["ptr"] >= 0)[0]}


def free_excess_stack(state):
    return np.asarray(state["excess_list"])[:int(state["last_free_excess_id"]) + 1].tolist()
