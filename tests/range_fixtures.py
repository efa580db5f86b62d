"""What the range-image tests share (test_oracle_range_image.py on the CPU, test_gpu_range_image.py on the GPU): maps made
of block positions alone, the poses they are seen from, and the reference of ref_range.py at each pose.  Voxel content
does not matter to FindVisibleBlocks / CreateExpectedDepths, so only the table is uploaded.

Every fixture asserts, from the reference alone, that it reaches what it is there for and that it stays inside the tie
cap: tie blocks at most 1 % of the listed blocks, tie cells at most 5 % of the corner's cells.  A pose that misses the cap
is changed; the cap is not.  Each fixture is built once per process."""
import functools

import numpy as np

import analytic_maps as am
import ref_range as rr
import refmap
import view_survey_fixtures as vf

VS = am.VS                      # 5 mm voxels: a block edge of 4 cm
BS = 8 * VS
TIE_BLOCKS, TIE_CELLS = 0.01, 0.05
BIG_BOX = 32                    # cells of one 16 x 16-cell tile above which the fill kernel queues a box for the workgroup
ROUND = 8192                    # list entries the fill kernel's workgroups take per round


def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """World -> camera 4 x 4 (float32) of a camera at t whose axes are rotated by yaw (about y), pitch (x), roll (z), as
    ref64_checks.camera; built as [R^T | -R^T t], with exact zeros where an angle is 0."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
         @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R.T, -R.T @ np.asarray(t, np.float64)
    return M.astype(np.float32)


class Case:
    """One map, one image size, two poses (the second one only separates two runs on one render state)."""

    def __init__(self, name, m, W, H, intr, M, M_other):
        self.name, self.m, self.W, self.H = name, m, W, H
        self.intr = np.asarray(intr, np.float32)
        self.M, self.M_other = M, M_other
        self.table = m.hash
        self.ref = self.law(M)
        self.ref_other = self.law(M_other)
        for r in (self.ref, self.ref_other):
            blocks, cells = r.tie_shares()
            assert blocks <= TIE_BLOCKS and cells <= TIE_CELLS, (name, r.n_tie_blocks, len(r.ids), cells)
        assert len(self.ref.ids) > 0 and (self.table["ptr"][self.ref.ids] >= 0).all()
        # a range image that is not reset between the two poses must show: cells the first pose covers, the second does not
        a, b = self.ref, self.ref_other
        self.reset_witnesses = int(((a.image[..., 0] != rr.FAR_AWAY) & (b.image[..., 0] == rr.FAR_AWAY)
                                    & ~a.tie_cells & ~b.tie_cells).sum())
        assert self.reset_witnesses >= 4, (name, self.reset_witnesses)

    def law(self, M, budget=rr.MAX_RENDERING_BLOCKS):
        return rr.RangeLaw(self.table, M, self.intr, self.m.vs, self.W, self.H, budget)

    def params(self, pkg):
        return self.m.scene_params(pkg)

    def upload(self, api, scene):
        m = self.m
        api.upload_scene_state(scene, self.table, m.alloc_list, m.last_free, m.excess_list, m.last_free_ex)


def _table_map(blocks, num_buckets):
    """view_survey_fixtures.blocks_map, kept for its table and pools alone: the voxel arrays (tens of megabytes for the
    sheet) are let go, nothing here uploads them."""
    m = vf.blocks_map(blocks, num_buckets=num_buckets)
    m.voxels = m.vba = None
    return m


def _last_entry(blocks, outlier, num_buckets):
    """`blocks` with `outlier` added so that it gets the table's last entry: the excess list is handed out from the top, so
    the first block that lands in an occupied bucket sits at the highest index.  The budget rule drops the list's last
    entries first; a block that alone decides some cells makes that visible."""
    blocks = np.asarray(blocks, np.int64)
    same = np.nonzero(am.hash_index(blocks, num_buckets) == am.hash_index(np.asarray(outlier), num_buckets))[0]
    assert len(same), "no block shares the outlier's bucket: choose another one"
    rest = np.delete(blocks, same[0], axis=0)
    return np.concatenate([blocks[same[:1]], np.asarray([outlier], np.int64), rest])


def _park_every_7th(m):
    """Every 7th occupied entry loses its voxel block (ptr = -1, as an entry parked on the host): never listed."""
    occ = np.nonzero(m.hash["ptr"] >= 0)[0]
    m.hash["ptr"][occ[::7]] = -1
    return occ[::7]


# ---------------------------------------------------------------------------------------------------------------------
# shell: a thinned sphere shell of 0.8 m around the camera
# ---------------------------------------------------------------------------------------------------------------------
SHELL_OUTLIER = (1, 0, 30)


@functools.lru_cache(maxsize=None)
def _shell_map():
    r = int(round(0.8 / BS))
    g = np.arange(-r - 1, r + 2)
    b = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d = np.linalg.norm(b + 0.5, axis=1)
    b = b[(np.abs(d - r) <= 0.5) & (b[:, 2] > 0.45 * r)]          # the cap in front of the camera
    b = b[np.random.default_rng(3).random(len(b)) < 0.3]
    b = _last_entry(b, SHELL_OUTLIER, 0x100)                     # one block further out, the table's last entry
    m = _table_map(b, 0x100)
    parked = _park_every_7th(m)
    assert 300 <= len(b) <= 900 and m.max_chain >= 3 and len(parked) > 40
    assert m.hash["ptr"][-1] >= 0 and tuple(m.hash["pos"][-1]) == SHELL_OUTLIER
    return m


@functools.lru_cache(maxsize=None)
def shell(W, H):
    m = _shell_map()
    intr = {(61, 47): (52.3, 50.9, 30.7, 22.6), (200, 136): (163.7, 161.3, 98.6, 69.3)}[(W, H)]
    # the small image looks at the rim of the cap, so that some of its 8 x 6 cells stay empty
    yaw, yaw_other = {(61, 47): (0.9, -1.0), (200, 136): (0.07, 1.1)}[(W, H)]
    c = Case(f"shell_{W}x{H}", m, W, H, intr, pose(yaw, -0.05, 0.3, (0.013, -0.007, 0.011)),
             pose(yaw_other, 0.2, -0.2, (0.05, 0.02, -0.03)))
    r = c.ref
    assert c.ref.cw % 16 and c.ref.ch % 16                           # a partial 16 x 16-cell tile
    if (W, H) == (61, 47):
        assert W % 8 and H % 8                                       # partial cells
    if (W, H) == (200, 136):
        assert r.cw > 16 and r.ch > 16                               # 2 x 2 tiles
        assert (r.box[:, 0] < 16).any() and (r.box[:, 2] >= 16).any() and (r.box[:, 1] < 16).any() and (r.box[:, 3] >= 16).any()
    # entries without a voxel block that would pass the frustum test: the list must leave them out
    parked = np.nonzero(m.hash["ptr"] == -1)[0]
    seen, _ = refmap.block_visibility(m.hash["pos"][parked], c.M, c.intr, m.vs, W, H)
    assert seen.sum() >= 5 and not np.isin(parked, r.ids).any()
    assert len(r.ids) >= 30 and (r.req != 0).all()
    free = (r.image[..., 0] == rr.FAR_AWAY) & ~r.tie_cells
    assert free.sum() >= 3, "no cell that must stay (FAR_AWAY, VERY_CLOSE)"
    # cells in the last column / row of the corner, which only a stride of W (not ceil(W/8)) addresses correctly from row 1 on
    assert (r.image[1:, :, 0] != rr.FAR_AWAY).any()
    return c


# ---------------------------------------------------------------------------------------------------------------------
# close: a slab the camera stands inside, looking along it
# ---------------------------------------------------------------------------------------------------------------------
CLOSE_T = (1.0e-4, -1.3e-4, -5.0e-4)


@functools.lru_cache(maxsize=None)
def close():
    g = np.stack(np.meshgrid(np.arange(-6, 6), np.arange(-2, 2), np.arange(-3, 25), indexing="ij"), -1).reshape(-1, 3)
    g = _last_entry(g, (1, 0, 30), 0x100)                        # one block past the slab's far end, the table's last entry
    m = _table_map(g, 0x100)
    assert tuple(m.hash["pos"][-1]) == (1, 0, 30)
    W, H = 200, 136
    # The camera rolls about its own z axis only, so camera z = world z - t_z exactly: the corners on the plane z = 0 of the
    # world lie 0.5 mm in front of it (inside [1e-6, 1e-3): projected, not skipped), the planes behind it are skipped.  It
    # stands a tenth of a millimetre off the block edge x = y = 0, so the four blocks behind that edge have one corner in
    # the image: listed with four corners skipped and the other four at 0.5 mm.  zmax starts at VERY_CLOSE, so the law's
    # `zmax < VERY_CLOSE` never rejects them: they render with z = (VERY_CLOSE, VERY_CLOSE).
    c = Case("close", m, W, H, (163.7, 161.3, 98.6, 69.3), pose(roll=0.3, t=CLOSE_T), pose(yaw=-1.2, pitch=0.1, roll=0.1, t=(0.6, 0.0, 0.3)))
    r = c.ref
    assert (r.tile_cells() > BIG_BOX).sum() >= 20 and r.tile_cells().max() == 256
    some_behind = r.skipped.any(1) & ~r.skipped.all(1)
    assert some_behind.sum() >= 4 and (r.req[some_behind] != 0).all() and (r.z[some_behind] == rr.VERY_CLOSE).all()
    # wholly behind: resident, not listed
    behind = m.block_pos[:, 2] <= -2
    assert behind.sum() > 50 and not np.isin(r.pos[:, 2], [-3, -2]).any() and r.ids[-1] == len(m.hash) - 1
    live = r.req != 0
    b = r.box[live]
    assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == W - 1).any() and (b[:, 3] == H - 1).any()
    assert (r.z[live, 0] == rr.VERY_CLOSE).sum() >= 4                # zmin raised
    # corners between z = 1e-6 and z = 1e-3 that are projected: the threshold itself is under test
    z = _corner_z(r.pos, c.M)
    assert (((z >= 1e-6) & (z < 1e-3)).any(1) & live).sum() >= 4
    return c


@functools.lru_cache(maxsize=None)
def sliver():
    """The pose of `close` in front of three lone blocks: in the slab every cell a corner at 0.5 mm reaches is covered by
    other blocks as well; here the block ahead of the camera decides cells by those corners alone."""
    g = np.array([[0, 0, 0], [0, 0, -1], [3, 1, 14], [-4, -1, 14], [2, -2, 20]])
    m = _table_map(g, 0x100)
    W, H = 200, 136
    c = Case("sliver", m, W, H, (163.7, 161.3, 98.6, 69.3), pose(roll=0.3, t=CLOSE_T), pose(yaw=0.5, pitch=-0.3, t=(0.1, 0.0, -0.2)))
    r = c.ref
    z = _corner_z(r.pos, c.M)
    assert ((z >= 1e-6) & (z < 1e-3)).any(1).sum() >= 2 and len(r.ids) == len(g)
    other = rr.RangeLaw(c.table, c.M, c.intr, m.vs, W, H, skip_below=1e-3)
    assert ((other.image != r.image).any(-1) & ~r.tie_cells).sum() >= 4, "the 1e-6 threshold decides no cell"
    return c


def _corner_z(pos, M):
    out = []
    for corner in range(8):
        p = (pos + np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])) * float(np.float32(BS))
        out.append(p @ np.asarray(M, np.float64)[2, :3] + float(M[2, 3]))
    return np.stack(out, 1)


# ---------------------------------------------------------------------------------------------------------------------
# many: a flat sheet 3 m below the camera, more than one round of the fill kernel's stride
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many():
    g = np.stack(np.meshgrid(np.arange(-58, 58), np.arange(-44, 44), [75], indexing="ij"), -1).reshape(-1, 3)
    m = _table_map(g, 0x1000)
    W, H = 320, 240
    c = Case("many", m, W, H, (207.3, 205.9, 158.7, 118.4), pose(0.011, -0.007, 0.004, (0.013, 0.009, 0.002)),
             pose(yaw=0.9, pitch=0.1, t=(0.3, 0.1, 0.0)))
    r = c.ref
    assert len(r.ids) > ROUND and len(r.ids) % 256 != 0, len(r.ids)
    assert len(r.ids) >= 0.85 * len(g)
    # the second round decides some cells: leaving the entries past the first 8192 out changes the image off the ties
    first = rr.splat(r.box[:ROUND], r.z[:ROUND, 0], r.z[:ROUND, 1], r.cw, r.ch, rr.FAR_AWAY, rr.VERY_CLOSE)
    assert ((first != r.image).any(-1) & ~r.tie_cells).sum() >= 10
    return c


# ---------------------------------------------------------------------------------------------------------------------
# budget
# ---------------------------------------------------------------------------------------------------------------------
BUDGET_KINDS = ("T+1", "T", "T//2", "1")


@functools.lru_cache(maxsize=None)
def budget(which, kind):
    """(case, budget, reference under that budget)."""
    c = close() if which == "close" else shell(200, 136)
    T = c.ref.total
    b = {"T+1": T + 1, "T": T, "T//2": T // 2, "1": 1}[kind]
    r = c.law(c.M, b)
    # the sequence of accepted totals must not hang on a tie: every listed block has one req in both number types
    assert (r.req == r.req64).all() and len(r.vis_tie_ids) == 0, (which, "a tie block would shift the budget sequence")
    full = c.ref
    changed = ((r.image != full.image).any(-1) & ~r.tie_cells).sum()
    live = r.req != 0
    if kind == "T+1":
        assert not r.budget_on and r.accepted[live].all() and changed == 0
    else:
        assert r.budget_on and not r.accepted[live].all()
        assert changed >= 1, (which, kind, "the dropped entries decide no cell")
    if kind == "T":      # exactly the last entry with tiles reaches the budget
        assert (~r.accepted & live).sum() == 1 and not r.accepted[np.nonzero(live)[0][-1]]
    if kind == "T//2" and which == "close":   # a dropped big block followed by an accepted smaller one
        drop = np.nonzero(~r.accepted & live)[0]
        acc = np.nonzero(r.accepted)[0]
        assert len(drop) and len(acc) and acc.max() > drop.min()
        first = drop.min()
        assert (r.req[acc[acc > first]] < r.req[first]).any()
    if kind == "1":
        assert not r.accepted.any() and (r.image[..., 0] == rr.FAR_AWAY).all()
    return c, b, r


ALL_CASES = {"shell_61x47": lambda: shell(61, 47), "shell_200x136": lambda: shell(200, 136), "close": close, "sliver": sliver,
             "many": many}
