"""Exact TSDF maps of closed-form geometry, built in numpy and uploaded into either engine (HIP or oracle).

A map is the voxel-block hash of SURVEY.md A.1/A.2 filled directly from a signed distance function: every voxel of
every kept block holds sdf = trunc(clamp(d/mu, -1, 1) * 32767) with w_depth >= 1.  Nothing here calls the engine
except `upload`, so the raycast / mesh kernels can be checked against geometry that is known in closed form.

Each map lies in a band of blocks around its surface and can be built with
  * holes: blocks left out at random (they read as the default voxel, A.2);
  * negative block coordinates: every map straddles the world origin, where the cameras sit;
  * a small bucket count, so that most blocks live in excess-list chains (`Map.max_chain` reports the longest).
"""
import numpy as np

VOXEL_DTYPE = np.dtype(
    {"names": ["sdf", "w_depth", "clr", "w_color", "_pad"], "formats": ["<i2", "u1", ("u1", 3), "u1", "u1"],
     "offsets": [0, 2, 3, 6, 7], "itemsize": 8})
HASH_ENTRY_DTYPE = np.dtype(
    {"names": ["pos", "_pad", "offset", "ptr"], "formats": [("<i2", 3), "<i2", "<i4", "<i4"], "offsets": [0, 6, 8, 12],
     "itemsize": 16})


def hash_index(b, num_buckets):
    """SURVEY A.1 hashIndex on int block coordinates [..., 3] (uint32 wrap-around, as C does)."""
    b = np.asarray(b, np.int64) & 0xFFFFFFFF
    h = ((b[..., 0] * 73856093) & 0xFFFFFFFF) ^ ((b[..., 1] * 19349669) & 0xFFFFFFFF) ^ ((b[..., 2] * 83492791) & 0xFFFFFFFF)
    return (h & (num_buckets - 1)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# geometry: signed distance in metres, positive on the side the cameras look from
# ---------------------------------------------------------------------------------------------------------------------
class Plane:
    """n . x = c with unit normal n; d = n . x - c."""

    def __init__(self, n, c):
        self.n = np.asarray(n, np.float64) / np.linalg.norm(n)
        self.c = float(c)

    def sdf(self, x):
        return x @ self.n - self.c

    def normal(self, x):
        return np.broadcast_to(self.n, x.shape)

    def ray_depth(self, origin, dirs):
        """t > 0 with origin + t dirs on the surface, nan where the ray does not reach it (all geometries alike)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (self.c - origin @ self.n) / (dirs @ self.n)
        return np.where(t > 0, t, np.nan)


class Sphere:
    """Seen from outside (inside=False: d = |x - c| - r) or from inside (d = r - |x - c|)."""

    def __init__(self, c, r, inside=False):
        self.c, self.r, self.inside = np.asarray(c, np.float64), float(r), inside

    def sdf(self, x):
        d = np.linalg.norm(x - self.c, axis=-1) - self.r
        return -d if self.inside else d

    def normal(self, x):
        v = x - self.c
        v = v / np.linalg.norm(v, axis=-1, keepdims=True)
        return -v if self.inside else v

    def ray_depth(self, origin, dirs):
        """Nearer root from outside, farther root from inside."""
        o = np.asarray(origin, np.float64) - self.c
        a, hb, c = np.sum(dirs * dirs, -1), dirs @ o, o @ o - self.r ** 2
        with np.errstate(invalid="ignore"):
            s = np.sqrt(hb * hb - a * c)
        t = (-hb + s) / a if self.inside else (-hb - s) / a
        return np.where(t > 0, t, np.nan)


class BoxCorner:
    """The concave corner of three axis-aligned walls x = a, y = b, z = e seen from the side x < a, y < b, z < e:
    free space is the open octant, d = min(a - x, b - y, e - z) (exact distance inside the octant up to the
    medial planes; the walls are each a plane, so away from the corner edges the field is exactly linear)."""

    def __init__(self, corner):
        self.k = np.asarray(corner, np.float64)

    def sdf(self, x):
        return np.min(self.k - x, axis=-1)

    def normal(self, x):
        i = np.argmin(self.k - x, axis=-1)
        out = np.zeros(x.shape)
        np.put_along_axis(out, i[..., None], -1.0, axis=-1)
        return out

    def ray_depth(self, origin, dirs):
        """The first of the three walls a ray from inside the octant meets."""
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(dirs > 0, (self.k - origin) / dirs, np.inf).min(axis=-1)
        return np.where(np.isfinite(t) & (t > 0), t, np.nan)


class Map:
    """Blocks, their voxels and the hash structures that hold them."""

    def __init__(self, vs, mu, block_pos, voxels, num_buckets, num_excess, num_local_blocks, geom, colour=None):
        self.vs, self.mu, self.geom, self.colour = vs, mu, geom, colour
        self.block_pos = np.asarray(block_pos, np.int64)  # [n, 3]
        self.voxels = voxels  # [n, 512] VOXEL_DTYPE, local index x + 8y + 64z
        self.num_buckets, self.num_excess, self.num_local_blocks = num_buckets, num_excess, num_local_blocks
        self._build_hash()
        self._build_grid()

    # -- SURVEY A.4 COMMIT / A.10 layout: buckets first, then the excess area; pools handed out from the top -----------
    def _build_hash(self):
        nb, nx, nl = self.num_buckets, self.num_excess, self.num_local_blocks
        n = len(self.block_pos)
        assert n <= nl and n <= nb + nx
        table = np.zeros(nb + nx, HASH_ENTRY_DTYPE)
        table["ptr"] = -2
        alloc = np.arange(nl, dtype=np.int32)
        excess = np.arange(nx, dtype=np.int32)
        last_free, last_ex = nl - 1, nx - 1
        ptrs = np.empty(n, np.int64)
        chain_len = np.zeros(nb, np.int64)
        for i, (b, h) in enumerate(zip(self.block_pos, hash_index(self.block_pos, nb))):
            ptr = int(alloc[last_free])
            last_free -= 1
            ptrs[i] = ptr
            if table["ptr"][h] == -2:
                t = h
            else:
                tail = h
                while table["offset"][tail] >= 1:
                    tail = nb + table["offset"][tail] - 1
                o = int(excess[last_ex])
                last_ex -= 1
                table["offset"][tail] = o + 1
                t = nb + o
            table["pos"][t] = b
            table["ptr"][t] = ptr
            chain_len[h] += 1
        self.hash, self.alloc_list, self.excess_list = table, alloc, excess
        self.last_free, self.last_free_ex = last_free, last_ex
        self.ptrs = ptrs
        self.max_chain = int(chain_len.max()) if n else 0
        self.vba = np.zeros((nl, 512), VOXEL_DTYPE)
        self.vba["sdf"] = 32767
        self.vba[ptrs] = self.voxels

    # -- a dense voxel grid over the blocks' bounding box, missing blocks as the default voxel (A.2) ----------------------
    def _build_grid(self):
        lo = self.block_pos.min(axis=0) - 1
        hi = self.block_pos.max(axis=0) + 2
        self.grid_lo = lo * 8  # voxel coordinate of grid[0, 0, 0]
        shape = tuple(int(v) for v in (hi - lo) * 8)
        self.grid_sdf = np.full(shape, 32767, np.int16)
        self.grid_found = np.zeros(shape, bool)
        self.grid_clr = np.zeros(shape + (3,), np.uint8)
        self.grid_wd = np.zeros(shape, np.uint8)
        self.grid_wc = np.zeros(shape, np.uint8)
        v = self.voxels.reshape(-1, 8, 8, 8)  # [n, z, y, x]
        for i, b in enumerate(self.block_pos - lo):
            sl = tuple(slice(int(c) * 8, int(c) * 8 + 8) for c in b)
            self.grid_sdf[sl] = v[i]["sdf"].transpose(2, 1, 0)
            self.grid_clr[sl] = v[i]["clr"].transpose(2, 1, 0, 3)
            self.grid_wd[sl] = v[i]["w_depth"].transpose(2, 1, 0)
            self.grid_wc[sl] = v[i]["w_color"].transpose(2, 1, 0)
            self.grid_found[sl] = True

    def lookup(self, p):
        """(sdf int16, clr, found) of integer voxel coordinates p [..., 3]; outside the grid = missing."""
        q = np.asarray(p, np.int64) - self.grid_lo
        shape = np.array(self.grid_sdf.shape)
        ok = np.all((q >= 0) & (q < shape), axis=-1)
        qc = np.where(ok[..., None], q, 0)
        idx = (qc[..., 0], qc[..., 1], qc[..., 2])
        found = ok & self.grid_found[idx]
        sdf = np.where(found, self.grid_sdf[idx], np.int16(32767))
        clr = np.where(found[..., None], self.grid_clr[idx], 0)
        return sdf, clr, found

    def lookup_weights(self, p):
        """(w_depth, w_color) of integer voxel coordinates p [..., 3], 0 where the voxel is missing."""
        q = np.asarray(p, np.int64) - self.grid_lo
        ok = np.all((q >= 0) & (q < np.array(self.grid_wd.shape)), axis=-1)
        qc = np.where(ok[..., None], q, 0)
        idx = (qc[..., 0], qc[..., 1], qc[..., 2])
        return np.where(ok, self.grid_wd[idx], np.uint8(0)), np.where(ok, self.grid_wc[idx], np.uint8(0))

    def scene_params(self, pkg, **over):
        kw = dict(voxel_size=self.vs, mu=self.mu, max_w=100, frustum_min=0.05, frustum_max=5.0,
                  num_local_blocks=self.num_local_blocks, num_buckets=self.num_buckets, num_excess=self.num_excess)
        kw.update(over)
        return pkg.SceneParams(**kw)


def build_map(geom, vs, mu, box_lo, box_hi, band=None, holes=0.0, seed=0, num_buckets=0x400, num_excess=None,
              colour=None, w_depth=1, local_factor=8, max_blocks=6000, w_depth_field=None, w_color_field=None,
              keep_sdf=False):
    """Every block inside the metric box [box_lo, box_hi) with a voxel within `band` (default 1.5 mu) of the surface.
    `holes`: fraction of those blocks left out (seeded).  `colour(x)` -> [..., 3] float in [0, 255] fills clr and
    sets w_color = 1.  The voxel pool holds `local_factor` times the blocks, so the mesh never saturates.

    `w_depth_field(p)` / `w_color_field(p)`: integers in 0 .. 255 per integer voxel coordinate p [..., 3], in place of the
    one `w_depth` / the w_color of 1.  A voxel whose w_depth is 0 is stored as fusion leaves a voxel it never observed
    (sdf 32767, no weight, no colour) -- except where `keep_sdf` (True, or a callable on p that returns a mask) says to
    keep the analytic sdf and the colour under the weight 0: a voxel the law is defined for, which fusion cannot
    produce, and the only one on which the weight alone decides a read.  A w_color of 0 keeps the voxel's colour bytes."""
    band = 1.5 * mu if band is None else band
    bs = 8 * vs
    blo = np.floor(np.asarray(box_lo) / bs).astype(np.int64)
    bhi = np.ceil(np.asarray(box_hi) / bs).astype(np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(blo, bhi)], indexing="ij"), -1).reshape(-1, 3)
    loc = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)  # [z, y, x, (z,y,x)]
    loc = loc[..., ::-1].reshape(512, 3)  # (x, y, z), local index x + 8y + 64z
    keep, vox_d = [], []
    for chunk in np.array_split(grid, max(1, len(grid) // 2048)):
        pts = (chunk[:, None, :] * 8 + loc[None]) * vs  # metric voxel centres (A.1)
        d = geom.sdf(pts)
        k = np.abs(d).min(axis=1) <= band
        keep.append(chunk[k])
        vox_d.append(d[k])
    bpos = np.concatenate(keep)
    d = np.concatenate(vox_d)
    rng = np.random.default_rng(seed)
    if holes > 0:
        k = rng.random(len(bpos)) >= holes
        bpos, d = bpos[k], d[k]
    assert 0 < len(bpos) <= max_blocks, len(bpos)
    vox = np.zeros((len(bpos), 512), VOXEL_DTYPE)
    vox["sdf"] = np.trunc(np.clip(d / mu, -1.0, 1.0) * 32767.0).astype(np.int16)
    vox["w_depth"] = w_depth
    if colour is not None:
        pts = (bpos[:, None, :] * 8 + loc[None]) * vs
        vox["clr"] = np.clip(np.floor(colour(pts)), 0, 255).astype(np.uint8)
        vox["w_color"] = 1
    if w_depth_field is not None or w_color_field is not None:
        P = bpos[:, None, :] * 8 + loc[None]
        if w_color_field is not None:
            vox["w_color"] = np.asarray(w_color_field(P)).astype(np.uint8)
        if w_depth_field is not None:
            wd = np.asarray(w_depth_field(P))
            assert wd.min() >= 0 and wd.max() <= 255
            vox["w_depth"] = wd.astype(np.uint8)
            keep = np.asarray(keep_sdf(P), bool) if callable(keep_sdf) else np.full(wd.shape, bool(keep_sdf))
            unobserved = np.zeros((), VOXEL_DTYPE)
            unobserved["sdf"] = 32767
            vox[(wd == 0) & ~keep] = unobserved
    n = len(bpos)
    nl = max(0x100, local_factor * n)
    nx = num_excess if num_excess is not None else max(0x100, n)
    nx += (-(num_buckets + nx)) % 16
    return Map(vs, mu, bpos, vox, num_buckets, nx, nl, geom, colour)


def upload(api, scene, m):
    """Load map `m` into `scene` (HIP engine or oracle): hash table, pools, every voxel block.  A map that brings its own
    `upload` (highslot_fixtures.relocate: no whole-pool `vba`) is loaded by that."""
    if getattr(m, "upload", None) is not None:
        return m.upload(api, scene, m)
    api.upload_scene_state(scene, m.hash, m.alloc_list, m.last_free, m.excess_list, m.last_free_ex)
    api.upload_voxel_blocks(scene, 0, m.vba)


# ---------------------------------------------------------------------------------------------------------------------
# the maps the tests use (5 mm voxels, mu = 2 cm: the S-room scene parameters)
# ---------------------------------------------------------------------------------------------------------------------
VS, MU = 0.005, 0.02


def tilted_plane(tilt_deg=20.0, depth=0.5, **kw):
    """A plane `depth` m in front of a camera at the origin looking down +z, its normal tilted about y."""
    t = np.deg2rad(tilt_deg)
    n = np.array([np.sin(t), 0.0, -np.cos(t)])  # faces the camera
    geom = Plane(n, float(n @ np.array([0.0, 0.0, depth])))
    return build_map(geom, VS, MU, (-0.45, -0.33, depth - 0.35), (0.45, 0.33, depth + 0.35), **kw)


def sphere_outside(**kw):
    geom = Sphere((0.03, -0.02, 0.45), 0.16)
    return build_map(geom, VS, MU, (-0.17, -0.22, 0.24), (0.23, 0.18, 0.66), **kw)


def sphere_inside(**kw):
    geom = Sphere((0.0, 0.0, 0.02), 0.30, inside=True)
    return build_map(geom, VS, MU, (-0.34, -0.34, -0.06), (0.34, 0.34, 0.36), **kw)


def box_corner(**kw):
    geom = BoxCorner((0.16, 0.12, 0.55))
    return build_map(geom, VS, MU, (-0.40, -0.30, 0.10), (0.24, 0.20, 0.62), **kw)


def colour_plane(**kw):
    """A fronto-parallel-ish plane whose colour is a linear field of position (gradient in 1/m per channel)."""
    geom = Plane((0.1, 0.05, -1.0), -0.40)
    grad = np.array([[300.0, 0.0, 40.0], [0.0, 250.0, -60.0], [60.0, 80.0, 0.0]])  # d(r,g,b)/d(x,y,z)

    def colour(x):
        return 128.0 + (x - np.array([0.0, 0.0, 0.4])) @ grad

    m = build_map(geom, VS, MU, (-0.3, -0.22, 0.2), (0.3, 0.22, 0.62), colour=colour, **kw)
    m.colour_grad = grad
    return m
