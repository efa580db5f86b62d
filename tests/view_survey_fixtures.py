"""What the view-survey tests share (test_view_survey_ref.py on the CPU, test_gpu_view_survey.py on the GPU): seeded views,
maps made of block positions alone whose blocks are placed against the reference's own plane values, hand-made tables for
the walk's edges, and the random count matrices of the selection tests.  Each fixture is built once per process."""
import functools
import random

import numpy as np

import analytic_maps as am
import ref64_checks as rc
import ref_view_survey as rv

VS = am.VS
I4 = np.eye(4, dtype=np.float32)


class TableMap(am.Map):
    """analytic_maps.Map without its dense voxel grid: the survey reads the table only, and a grid cannot span blocks at
    both ends of the int16 range."""

    def _build_grid(self):
        pass


def blocks_map(block_pos, num_buckets=0x400, vs=VS):
    """overlap_fixtures.blocks_map for block positions anywhere in the int16 range."""
    block_pos = np.asarray(block_pos, np.int64).reshape(-1, 3)
    n = len(block_pos)
    vox = np.zeros((n, 512), am.VOXEL_DTYPE)
    vox["sdf"] = 32767
    nx = max(0x100, n)
    nx += (-(num_buckets + nx)) % 16
    return TableMap(vs, am.MU, block_pos, vox, num_buckets, nx, max(0x100, 2 * n), None)


def rigid(rng, max_t):
    """A random rigid 4 x 4 (float32) whose translation has a length of at most max_t."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t / np.linalg.norm(t) * rng.uniform(0.0, max_t)
    return T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def random_views(count=240, seed=7):
    """[(View, voxel size)]: any pose, image sizes from 1 x 1 to 1280 x 960, principal points inside and outside the image,
    near_m = 0 and far_m = 0 among them."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        w, h = (1, 1) if k % 10 == 3 else (int(rng.integers(1, 1281)), int(rng.integers(1, 961)))
        f = float(rng.uniform(0.3, 2.5)) * max(w, 8)
        cx, cy = (w - 1) / 2 + rng.uniform(-0.2, 0.2) * w, (h - 1) / 2 + rng.uniform(-0.2, 0.2) * h
        if k % 10 == 5:     # the principal point outside the image
            cx, cy = (-0.4 * w - 3.0, 1.7 * h + 2.0) if k % 20 == 5 else (1.3 * w + 5.0, -0.2 * h - 1.0)
        near = 0.0 if k % 4 == 1 else float(rng.uniform(0.01, 0.5))
        far = 0.0 if k % 5 == 2 else near + float(rng.uniform(0.05, 8.0))
        vs = float(rng.choice([0.005, 0.01, 1.0 / 256.0, 0.0037]))
        out.append((rv.View(rigid(rng, 30.0), (f, f * rng.uniform(0.9, 1.1), cx, cy), w, h, near, far), vs))
    return out


@functools.lru_cache(maxsize=None)
def selection_cases(count=240, seed=99):
    """[(reach [V][N], nearest [V][N], dict of parameters)]: caps that bite, always_keep with and without reach, ties on
    the nearest depth and on the sums."""
    rnd = random.Random(seed)
    cases = []
    for k in range(count):
        n, nv = rnd.randint(1, 90), rnd.randint(1, 4)
        reach = [[rnd.choice([0, 0, 1, 2, 5, 5, 40, rnd.randint(0, 3000)]) for _ in range(n)] for _ in range(nv)]
        nearest = [[rnd.choice([3, 3, 10, 10, 25, rnd.randint(-50, 400)]) if reach[v][i] else rv.INT32_MAX for i in range(n)]
                   for v in range(nv)]
        keep = rnd.choice([-1, -1, rnd.randrange(n)])
        if keep >= 0 and k % 3 == 0:
            for v in range(nv):
                reach[v][keep], nearest[v][keep] = 0, rv.INT32_MAX
        params = dict(min_blocks=rnd.choice([0, 0, 1, 2, 6, 41]), max_maps=rnd.choice([0, 0, 1, 2, 5, 17, 64]), always_keep=keep)
        cases.append((reach, nearest, params))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the fixture set: 5 posed maps against 3 views
# ---------------------------------------------------------------------------------------------------------------------
class FixtureSet:
    def __init__(self, maps, T, views, notes):
        self.maps, self.T, self.views, self.notes = maps, np.stack(T).astype(np.float32), views, notes

    @property
    def tables(self):
        return [m.hash for m in self.maps]


def views3(w=96, h=72):
    cams = [rc.camera(w, h, yaw=0.1, pitch=-0.05, t=(0.02, -0.01, 0.03)), rc.camera(w, h, yaw=-0.35, pitch=0.2, roll=0.3, t=(0.3, 0.1, -0.2)),
            rc.camera(w, h, yaw=0.6, roll=-0.2, t=(-0.25, 0.05, 0.1), f_scale=1.4)]
    return [rv.View(cams[0][0], cams[0][1], w, h, 0.5, 1.6), rv.View(cams[1][0], cams[1][1], w, h, 0.4, 0.0),
            rv.View(cams[2][0], cams[2][1], w, h, 0.45, 1.1)]


def lattice(centre, radius):
    """Every block position within `radius` blocks of `centre` per axis that an int16 holds."""
    ax = [np.arange(max(c - radius, -32768), min(c + radius, 32767) + 1) for c in centre]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def fixture_set():
    """Blocks placed from the reference's own s_k: well inside, within 0.25 voxel of s_k = -rho on either side for each of
    the six planes, behind the camera, beyond far, at the ends of the block range, in excess chains; one entry that would
    reach made non-resident."""
    import multimesh_fixtures as mf
    views = views3()
    planes = [rv.frustum_planes(v, VS) for v in views]
    rho = rv.rho_of(0.0)
    # map 4 lives at the corner of the block range: its frame is the world's moved by (almost) 32767 blocks
    far_corner = np.eye(4, dtype=np.float32)
    far_corner[:3, 3] = np.array([32700, -32700, 32700]) * 8 * VS
    T = [mf.pose(yaw=0.2, pitch=-0.1, t=(0.05, 0.02, -0.03)), I4.copy(), mf.pose(yaw=-0.15, roll=0.2, t=(-0.04, 0.01, 0.06)),
         mf.rot_x(0.4, (0.3, -0.2, 0.1)), far_corner]
    notes = dict(boundary=[], inside=[], behind=[], beyond=[], ends=[])
    maps = []
    for i, Ti in enumerate(T):
        # the blocks around the point 0.7 m in front of view 0, in map i's frame
        Minv = np.linalg.inv(views[0].M.astype(np.float64))
        centre_w = Minv @ np.array([0.0, 0.0, 0.7, 1.0])
        centre = np.floor((Ti.astype(np.float64) @ centre_w)[:3] / (8 * VS)).astype(np.int64)
        cand = lattice(centre, 45)
        p = rv.world_points(cand, Ti, VS)
        S = [rv.plane_values(pl, p)[0].astype(np.float64) for pl in planes]
        chosen = []
        for v in range(3):
            s = S[v]
            inside = np.flatnonzero(np.all(s[:, :6] >= 1.0, axis=1))
            assert len(inside) > 8
            chosen += [cand[j] for j in inside[:: max(1, len(inside) // 6)][:6]]
            notes["inside"].append((i, v))
            for k in range(6):
                if not np.isfinite(planes[v][k, 3]):
                    continue        # (no far plane)
                # (the other five planes passed with a voxel to spare, so plane k alone decides)
                others = np.all(np.delete(s, k, axis=1) >= -float(rho) + 1.0, axis=1)
                just_in = np.flatnonzero(others & (s[:, k] >= -float(rho)) & (s[:, k] < -float(rho) + 0.25))
                just_out = np.flatnonzero(others & (s[:, k] < -float(rho)) & (s[:, k] > -float(rho) - 0.25))
                if len(just_in) and len(just_out):
                    chosen += [cand[just_in[0]], cand[just_out[0]]]
                    notes["boundary"].append((i, v, k, tuple(cand[just_in[0]]), tuple(cand[just_out[0]])))
            behind = np.flatnonzero(s[:, 4] < -40.0)
            chosen += [cand[behind[0]], cand[behind[-1]]]
            if np.isfinite(planes[v][5, 3]):
                beyond = np.flatnonzero((s[:, 5] < -20.0) & np.all(s[:, :4] >= 1.0, axis=1))
                chosen += [cand[beyond[0]]]
        ends = [[32767, 32767, 32767], [-32768, -32768, -32768], [32767, -32768, 0], [-32767, 32767, -32767]]
        chosen += ends
        pos = np.unique(np.array(chosen, np.int64), axis=0)
        rng = np.random.default_rng(100 + i)
        pos = pos[rng.permutation(len(pos))]
        m = blocks_map(pos, num_buckets=0x10)     # 16 buckets: most blocks live in excess chains
        assert m.max_chain >= 3
        maps.append(m)
    # one entry that would reach is made non-resident (as a swapped-out block's)
    m = maps[0]
    p = rv.world_points(m.block_pos, T[0], VS)
    ok = rv.reaching(planes[0], p, rho)[0]
    victim = m.block_pos[np.flatnonzero(ok)[0]]
    entry = int(np.flatnonzero(np.all(m.hash["pos"] == victim, axis=1) & (m.hash["ptr"] >= 0))[0])
    m.hash["ptr"][entry] = -1
    notes["not_resident"] = (0, entry)
    return FixtureSet(maps, T, views, notes)


# ---------------------------------------------------------------------------------------------------------------------
# hand-made tables: the walk's edges
# ---------------------------------------------------------------------------------------------------------------------
class RawTable:
    """A hash table with resident entries at chosen indices (the survey reads entries, it never looks one up)."""

    def __init__(self, num_buckets, num_excess, entries):
        self.num_buckets, self.num_excess = num_buckets, num_excess
        self.hash = np.zeros(num_buckets + num_excess, am.HASH_ENTRY_DTYPE)
        self.hash["ptr"] = -2
        for slot, (index, pos) in enumerate(sorted(entries.items())):
            self.hash["pos"][index] = pos
            self.hash["ptr"][index] = slot
        self.num_local_blocks = max(0x100, len(entries))

    def scene_params(self, pkg):
        return pkg.SceneParams(voxel_size=VS, mu=am.MU, max_w=100, frustum_min=0.05, frustum_max=5.0,
                               num_local_blocks=self.num_local_blocks, num_buckets=self.num_buckets, num_excess=self.num_excess)


def in_front(view, count, seed, depth=(0.6, 1.0)):
    """`count` distinct block positions (world frame = map frame) whose centres lie well inside `view`."""
    rng = np.random.default_rng(seed)
    Minv = np.linalg.inv(view.M.astype(np.float64))
    fx, fy, cx, cy = (float(v) for v in view.intr)
    out = set()
    while len(out) < count:
        x, y, d = rng.uniform(0.2, 0.8) * view.width, rng.uniform(0.2, 0.8) * view.height, rng.uniform(*depth)
        pw = Minv @ np.array([d * (x - cx) / fx, d * (y - cy) / fy, d, 1.0])
        out.add(tuple(int(v) for v in np.floor(pw[:3] / (8 * VS))))
    return np.array(sorted(out), np.int64)


@functools.lru_cache(maxsize=None)
def two_tile_table():
    """0x8000 buckets + 0x1000 excess entries: more than one 32768-entry bit tile, ending in the middle of one.  Resident
    entries at entry 0, at 32767 and 32768, at the last entry, a few more in the first 8192 -- and none in 8192 .. 32766."""
    blocks = in_front(views3()[0], 9, 5)
    behind = np.array([[0, 0, -300], [5, 5, -320]])
    where = [0, 32767, 32768, 0x9000 - 1, 17, 4095, 8191, 33000, 36000, 1, 32769]
    entries = {idx: tuple(b) for idx, b in zip(where, np.concatenate([blocks, behind]))}
    return RawTable(0x8000, 0x1000, entries)
