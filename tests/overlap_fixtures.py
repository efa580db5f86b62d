"""What the overlap tests share (test_overlap_ref.py on the CPU, test_gpu_overlap.py on the GPU): maps made of block
positions alone whose overlap follows from set arithmetic, and the random count matrices of the selection tests."""
import functools
import random

import numpy as np

import analytic_maps as am
import register_fixtures as fx

# a voxel size that is a power of two: 8 S vs and (8 S vs) / vs are exact in float32 and float64, so a T that moves a map by
# whole (or half) blocks gives an X~ of exact integers
VS_EXACT = 1.0 / 256.0


def blocks_map(block_pos, vs=VS_EXACT, num_buckets=0x400):
    """A map that holds the blocks `block_pos` [n, 3] with empty voxels: the survey reads the table only."""
    block_pos = np.asarray(block_pos, np.int64)
    n = len(block_pos)
    vox = np.zeros((n, 512), am.VOXEL_DTYPE)
    vox["sdf"] = 32767
    nx = max(0x100, n)
    nx += (-(num_buckets + nx)) % 16
    return am.Map(vs, am.MU, block_pos, vox, num_buckets, nx, max(0x100, 2 * n), None)


class SetCase:
    """Two maps whose shared counts are known from set operations on block coordinates: `want` = (blocks a->b, octants
    a->b, blocks b->a, octants b->a)."""

    def __init__(self, name, map_a, map_b, T, want):
        self.name, self.maps, self.T, self.want = name, [map_a, map_b], np.asarray(T, np.float32), want


def _keys(blocks):
    return {tuple(int(v) for v in b) for b in blocks}


@functools.lru_cache(maxsize=None)
def set_cases():
    A = fx._box_source().block_pos            # 268 blocks around a box corner, both signs of x and y
    rng = np.random.default_rng(11)
    part = A[rng.random(len(A)) < 0.7]        # map B images only a part of A ...
    stray = A[:40] + np.array([60, -45, 30])  # ... and holds blocks no block of A is taken to
    cases = []

    # 1. whole blocks under a rotation of 90 degrees about z: a voxel (x, y, z) goes to (-y, x, z) + 8 S, so the cube of
    # block (bx, by, bz) goes to the cube of block (-by - 1, bx, bz) + S
    S = np.array([5, -3, 2])
    image = lambda B: np.stack([-B[:, 1] - 1, B[:, 0], B[:, 2]], -1) + S
    preimage = lambda B: np.stack([(B - S)[:, 1], -(B - S)[:, 0] - 1, (B - S)[:, 2]], -1)
    Bb = np.concatenate([image(part), stray])
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = 8.0 * S * VS_EXACT
    ab = len(_keys(image(A)) & _keys(Bb))
    ba = len(_keys(preimage(Bb)) & _keys(A))
    assert ab == len(part) and ba == len(part) and 0 < ab < len(A)
    cases.append(SetCase("rotation", blocks_map(A), blocks_map(Bb), np.stack([np.eye(4, dtype=np.float32), T]),
                         (ab, 8 * ab, ba, 8 * ba)))

    # 2. whole blocks without a rotation, both poses off the identity: map a sits S_a blocks from the world's origin and map
    # b S_b, so block B of a is block B + (S_b - S_a) of b
    Sa, Sb = np.array([-2, 7, 1]), np.array([4, 4, -6])
    Bb = np.concatenate([part + (Sb - Sa), stray])
    Ta, Tb = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    Ta[:3, 3], Tb[:3, 3] = 8.0 * Sa * VS_EXACT, 8.0 * Sb * VS_EXACT
    ab = len(_keys(A + (Sb - Sa)) & _keys(Bb))
    cases.append(SetCase("shift", blocks_map(A), blocks_map(Bb), np.stack([Ta, Tb]), (ab, 8 * ab, ab, 8 * ab)))

    # 3. part of a block along x, map b's frame t voxels from map a's.  t = 4: the octants with ox = 0 of block B of a (centre
    # 1.5 + 4 = 5.5) lie in block B of b, those with ox = 1 (5.5 + 4 = 9.5) in block B + (1, 0, 0); back, ox = 0 of b's block B
    # (1.5 - 4 < 0) lies in a's block B - (1, 0, 0) and ox = 1 (5.5 - 4 = 1.5) in B.  t = 6.25: 1.5 + 6.25 = 7.75 still lies in
    # B -- by a quarter of a voxel, which is what pins the 1.5 -- and 5.5 + 6.25 in B + (1, 0, 0); back, both 1.5 - 6.25 and
    # 5.5 - 6.25 are negative: B - (1, 0, 0).
    Bb = np.concatenate([part, stray])
    kb, ka = _keys(Bb), _keys(A)
    x1 = np.array([1, 0, 0])
    held = lambda keys, blocks: np.array([tuple(int(v) for v in b) in keys for b in blocks])
    for name, t, to_b, to_a in (("half block", 4.0, (0, 1), (-1, 0)), ("three quarters of a block", 6.25, (0, 1), (-1, -1))):
        Tb = np.eye(4, dtype=np.float32)
        Tb[0, 3] = t * VS_EXACT
        fwd = [held(kb, A + k * x1) for k in to_b]       # per ox: is the block that octant falls into held by b?
        back = [held(ka, Bb + k * x1) for k in to_a]
        want = (int((fwd[0] | fwd[1]).sum()), int(4 * fwd[0].sum() + 4 * fwd[1].sum()),
                int((back[0] | back[1]).sum()), int(4 * back[0].sum() + 4 * back[1].sum()))
        assert (fwd[0] ^ fwd[1]).any()             # (some block shares exactly four octants)
        cases.append(SetCase(name, blocks_map(A), blocks_map(Bb), np.stack([np.eye(4, dtype=np.float32), Tb]), want))

    # 4. the identity: q = c itself
    ab = len(ka & kb)
    cases.append(SetCase("identity", blocks_map(A), blocks_map(Bb), np.stack([np.eye(4, dtype=np.float32)] * 2),
                         (ab, 8 * ab, ab, 8 * ab)))
    return cases


@functools.lru_cache(maxsize=None)
def selection_cases(count=200, seed=2024):
    """[(live [N], shared [N, N], dict of parameters)]: N from 2 to 12, sparse and dense matrices, counts around the
    thresholds, equal counts (ties of rank and of coverage), caps that bind and max_pairs = N - 1."""
    rnd = random.Random(seed)
    cases = []
    for k in range(count):
        n = rnd.randint(2, 12)
        live = [rnd.choice([1, 2, 8, 8, 50, 300, rnd.randint(1, 500)]) for _ in range(n)]
        density = rnd.choice([0.15, 0.3, 0.6, 1.0])
        shared = [[0] * n for _ in range(n)]
        for s in range(n):
            for d in range(n):
                if s == d:
                    shared[s][d] = 8 * live[s]
                elif rnd.random() < density:
                    v = rnd.choice([rnd.randint(0, 8 * live[s]), 63, 64, 65, 16, rnd.randint(0, 8 * live[s])])
                    shared[s][d] = min(v, 8 * live[s])
        if k % 5 == 0:       # symmetric counts on equal maps: coverage ties
            for s in range(n):
                for d in range(s):
                    if live[s] == live[d]:
                        shared[s][d] = shared[d][s]
        pairs_all = n * (n - 1)
        params = dict(min_shared_octants=rnd.choice([0, 0, 1, 16, 64, 100]), one_direction=rnd.choice([0, 1]),
                      max_pairs=rnd.choice([0, n - 1, n, rnd.randint(n - 1, min(128, max(n - 1, pairs_all)))]))
        if params["max_pairs"] == 0 and n == 1:
            params["max_pairs"] = 1
        cases.append((live, shared, params))
    return cases
