"""The two laws of dslam_mark_occupancy / dslam_distance_transform in numpy, independent of the
kernels: `mark` (which cells of a world-aligned grid the voxels of posed maps observe and occupy) and `edt` (the exact
squared Euclidean distance to the nearest seed cell).  Both are all-integer behind one float32 transform per voxel, so
the GPU is held to them bit for bit.

A grid is (origin [3], cell, dims [3]) in world voxel units; every per-cell array is x-fastest, returned here as a flat
array of dims[0] * dims[1] * dims[2] elements (index x + dims[0] * (y + dims[1] * z))."""
import collections

import numpy as np

F = np.float32
OBSERVED, OCCUPIED = 1, 2
SEED_OCCUPIED, SEED_UNKNOWN = 1, 2
FAR = 0x7FFFFFFF
MAX_COORD = F(1048576.0)   # 2^20 voxels
_INF = np.int64(1) << 40

Grid = collections.namedtuple("Grid", "origin cell dims")

LOCAL = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)[..., ::-1].reshape(512, 3)  # x + 8y + 64z


def grid_of(origin, cell, dims):
    return Grid(tuple(int(v) for v in origin), int(cell), tuple(int(v) for v in dims))


def cells(grid):
    return int(np.prod(grid.dims))


def B_of(T, voxel_size):
    """float32(rigid_inverse(voxel_pose(T, (double)voxel_size))): T world -> map, 4 x 4, metres (taken as float32, as the
    ABI takes it); the result maps the map's voxel coordinates to world voxel coordinates, 3 x 4."""
    T = np.asarray(T, F)
    vs = float(F(voxel_size))
    X = [[float(T[r, c]) for c in range(3)] + [float(T[r, 3]) / vs] for r in range(3)]
    B = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            B[r, c] = X[c][r]
        B[r, 3] = -((X[0][r] * X[0][3] + X[1][r] * X[1][3]) + X[2][r] * X[2][3])
    return B.astype(F)


def transform(B, p):
    """w = B p, float32, each row ((a x + b y) + c z) + d; p [..., 3] integers."""
    B = np.asarray(B, F)
    x, y, z = (np.asarray(p[..., k]).astype(F) for k in range(3))
    return np.stack([((B[r, 0] * x + B[r, 1] * y) + B[r, 2] * z) + B[r, 3] for r in range(3)], -1)


def threshold(occupied_below, mu):
    return int(np.floor(float(F(occupied_below)) / float(F(mu)) * 32767.0))


def mark(maps, grid, voxel_size, mu, min_weight=0, occupied_below=0.0, rounding="floor", use_T=False, gate="w_depth", strict=False):
    """Law 1.  maps: [(block_pos [n, 3], voxels [n, 512] of the voxel dtype, T)], the blocks resident in each map.  Returns
    one state byte per cell (0 unknown, 1 observed free, 3 occupied).

    rounding / use_T / gate / strict select the laws a kernel must NOT follow (round to nearest in place of floorf, T_i in
    place of B_i, the gate on w_color, sdf < thr); the defaults are the law."""
    origin, cell, dims = np.array(grid.origin, np.int64), grid.cell, np.array(grid.dims, np.int64)
    thr = threshold(occupied_below, mu)
    need = max(int(min_weight), 1)
    out = np.zeros(cells(grid), np.uint8)
    for block_pos, voxels, T in maps:
        block_pos = np.asarray(block_pos, np.int64).reshape(-1, 3)
        if len(block_pos) == 0:
            continue
        if use_T:
            Tm = np.asarray(T, F)
            B = np.concatenate([Tm[:3, :3], (Tm[:3, 3:4].astype(np.float64) / float(F(voxel_size))).astype(F)], axis=1)
        else:
            B = B_of(T, voxel_size)
        p = block_pos[:, None, :] * 8 + LOCAL[None]
        with np.errstate(invalid="ignore", over="ignore"):
            w = transform(B, p)
            ok = (np.abs(w) <= MAX_COORD).all(axis=-1)   # false for a NaN
            g = (np.floor(w) if rounding == "floor" else np.rint(w))
        g = np.where(ok[..., None], g, 0).astype(np.int64)
        c = (g - origin) // cell
        ok &= ((c >= 0) & (c < dims)).all(axis=-1)
        observed = ok & (voxels[gate].astype(np.int64) >= need)
        sdf = voxels["sdf"].astype(np.int64)
        occupied = observed & ((sdf < thr) if strict else (sdf <= thr))
        idx = c[..., 0] + dims[0] * (c[..., 1] + dims[1] * c[..., 2])
        out[idx[observed]] |= OBSERVED
        out[idx[occupied]] |= OBSERVED | OCCUPIED
    return out


def resident(table, blocks):
    """(block_pos, voxels) of a downloaded hash table and voxel pool: the entries with ptr >= 0."""
    live = table["ptr"] >= 0
    return table["pos"][live].astype(np.int64), blocks[table["ptr"][live]]


def seed_mask(states, seeds):
    s = np.asarray(states, np.uint8)
    m = np.zeros(s.shape, bool)
    if seeds & SEED_OCCUPIED:
        m |= (s & 2) != 0
    if seeds & SEED_UNKNOWN:
        m |= (s & 3) == 0
    return m


def _min_plus(f, axis):
    """out[j] = min_i f[i] + (i - j)^2 along `axis`, int64."""
    n = f.shape[axis]
    j = np.arange(n, dtype=np.int64).reshape([-1 if a == axis else 1 for a in range(f.ndim)])
    out = np.full(f.shape, _INF, np.int64)
    for i in range(n):
        fi = np.take(f, [i], axis=axis)
        if (fi >= _INF).all():
            continue
        np.minimum(out, fi + (j - i) ** 2, out=out)
    return np.minimum(out, _INF)


def edt(states, grid, seeds=SEED_OCCUPIED, max_cells=0):
    """Law 2: d2[c] = min over seed cells s of |c - s|^2 as int32, FAR where there is no seed or d2 > max_cells^2."""
    d0, d1, d2 = grid.dims
    f = np.where(seed_mask(states, seeds).reshape(d2, d1, d0), np.int64(0), _INF)
    for axis in (2, 1, 0):   # x, y, z
        f = _min_plus(f, axis)
    far = f >= _INF
    if max_cells:
        far |= f > int(max_cells) ** 2
    return np.where(far, FAR, f).astype(np.int32).reshape(-1)


def edt_brute(states, grid, seeds=SEED_OCCUPIED, max_cells=0):
    """The same by a brute force over all (cell, seed) pairs; small grids only."""
    d0, d1, d2 = grid.dims
    z, y, x = np.meshgrid(np.arange(d2), np.arange(d1), np.arange(d0), indexing="ij")
    pts = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.int64)
    s = pts[seed_mask(states, seeds).reshape(-1)]
    if len(s) == 0:
        return np.full(len(pts), FAR, np.int32)
    d = ((pts[:, None, :] - s[None]) ** 2).sum(-1).min(axis=1)
    if max_cells:
        d = np.where(d > int(max_cells) ** 2, FAR, d)
    return d.astype(np.int32)


def to_metres(d2, cell, voxel_size):
    """The metres form: sqrtf((float)d2) * ((float)cell * voxel_size), +inf for FAR."""
    d2 = np.asarray(d2, np.int32)
    scale = F(cell) * F(voxel_size)
    with np.errstate(over="ignore"):
        m = np.sqrt(d2.astype(F)) * scale
    return np.where(d2 == FAR, F(np.inf), m).astype(F)
