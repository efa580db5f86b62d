"""Map states for the packed-map tests, driven through refmap.MapModel: blocks are committed one at a time by the COMMIT
rule of its allocate (an empty bucket head takes the block; otherwise the end of the chain links a popped excess slot) and
released by its release, heads and middles of chains included, so that the free excess stack ends up out of order.
Voxel contents are seeded random bytes with w_depth > 0: the tests compare bytes, not surfaces."""
import numpy as np

import ref_pack
import refmap

EMPTY = np.uint64(0x7FFF)


def scene_params(pkg, nb, nx, nl, **kw):
    return pkg.SceneParams(num_local_blocks=nl, num_buckets=nb, num_excess=nx, **kw)


def commit(m, b):
    """One block through MapModel.allocate's COMMIT step.  Returns its entry, or None when a pool is exhausted."""
    b = tuple(int(c) for c in b)
    assert b not in m.index
    h = int(refmap.hash_index(b, m.nb))
    if m.hash["ptr"][h] < -1:
        if m.last_free < 0:
            return None
        t = h
    else:
        if m.last_free < 0 or m.last_free_ex < 0:
            return None
        o = int(m.excess_list[m.last_free_ex])
        m.hash["offset"][m.chain(h)[-1]] = o + 1
        m.last_free_ex -= 1
        t = m.nb + o
    m.hash[t] = (b, 0, 0, m.alloc_list[m.last_free])
    m.last_free -= 1
    m.index[b] = t
    return t


_GRID = np.stack(np.meshgrid(*[np.arange(-30, 31)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]   # x fastest


def colliding(nb, bucket, count, start=0):
    """`count` block positions, small and of both signs, that hash into `bucket` (from the `start`-th such position on)."""
    hits = _GRID[refmap.hash_index(_GRID, nb) == bucket][start:start + count]
    assert len(hits) == count, "no colliding positions found"
    return [tuple(int(c) for c in b) for b in hits]


def heads_only(nb, count, seed=0):
    """`count` block positions in `count` different buckets: a map without a chain."""
    rng = np.random.default_rng(seed)
    pos = rng.permutation(_GRID)
    _, first = np.unique(refmap.hash_index(pos, nb), return_index=True)
    assert len(first) >= count
    return [tuple(int(c) for c in b) for b in pos[np.sort(first)[:count]]]


def build(params, blocks, release=(), seed=0):
    """The state after committing `blocks` in order and then releasing the batches of blocks in `release`, one batch after
    the other (a batch returns its excess slots in ascending order, so it takes two to leave the stack out of order)."""
    m = refmap.MapModel(params, 8, 8)
    for b in blocks:
        assert commit(m, b) is not None, "the fixture's pools are too small"
    for batch in release:
        m.release(sorted(m.index[tuple(int(c) for c in b)] for b in batch))
    rng = np.random.default_rng(seed)
    vox = np.full((m.nl, 512), EMPTY, np.uint64)
    res = np.nonzero(m.hash["ptr"] >= 0)[0]
    fill = rng.integers(0, 1 << 63, (len(res), 512), dtype=np.uint64) | np.uint64(1 << 16)   # (w_depth >= 1)
    vox[m.hash["ptr"][res]] = fill
    return dict(hash=m.hash.copy(), voxels=vox, alloc_list=m.alloc_list.copy(), last_free_block_id=int(m.last_free),
                excess_list=m.excess_list.copy(), last_free_excess_id=int(m.last_free_ex), params=ref_pack.geometry(params),
                stats=dict(last_free_block_id=int(m.last_free), last_free_excess_id=int(m.last_free_ex)))


def chained_state(pkg, nb=64, nx=64, nl=96, seed=1, **kw):
    """Chains of 6 to 10 entries in a small table, then releases of heads, middles and tails: the free excess stack is
    out of order afterwards.  Returns (params, state)."""
    params = scene_params(pkg, nb, nx, nl, **kw)
    blocks, release = [], []
    for bucket, length in ((3, 6), (17, 8), (40, 10), (63, 7)):
        ch = colliding(nb, bucket, length)
        blocks += ch
        # the chains committed first hold the highest excess slots: their batches go first, the lower slots land on top
        release.append([ch[0], ch[2], ch[length - 1]] if bucket != 40 else [ch[4], ch[5]])
    blocks += [(-32767, 5, 32767), (32767, -32767, -1), (-1, -1, -1)]
    st = build(params, blocks, release, seed)
    return params, st


def states(pkg):
    """(name, source params, state): an empty map, one block, chains with an out-of-order excess stack, a stack that is
    empty, and a map without a chain (full stack)."""
    out = []
    p = scene_params(pkg, 64, 64, 96)
    out.append(("empty", p, build(p, [])))
    out.append(("one block", p, build(p, [(-3, 4, -5)], seed=2)))
    out.append(("chains and releases",) + chained_state(pkg))
    p = scene_params(pkg, 16, 16, 40)
    out.append(("excess stack empty", p, build(p, colliding(16, 5, 9) + colliding(16, 9, 9), seed=3)))
    p = scene_params(pkg, 256, 16, 40)
    out.append(("excess stack full", p, build(p, heads_only(256, 4), seed=4)))
    return out
