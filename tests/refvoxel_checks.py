"""Check bodies shared by test_oracle_voxel_update.py (CPU oracle) and test_gpu_voxel_update.py (HIP engine): the voxel
update of SURVEY A.5 and its inverse (A.11) on voxels and measurements the test chooses, every stored value against
ref64.update_exact.

The exactness comes from the inputs.  The voxel size is 2^-6 m, the poses are signed axis permutations with translations
of whole voxels, and the depth is uploaded with affine_a = 2^-10, so every camera-frame coordinate, every depth and every
eta = depth - z is a dyadic number that float32 holds exactly whatever the evaluation order.  The focal length is an
integer and the principal point dyadic, so a projection that is not exactly on a pixel boundary is at least 1 / (2 z / vs)
> 1e-3 pixel away from it, far above float32's 1e-5: no pixel pick and no image bound is a tie.

Every visible block is overwritten before the one call under test: the blocks at even places of the visible list with
seeded-random voxels over the full ranges, those at odd places with one edge row each (`edge_rows`).  Reach, tie shares
and their caps come from the crafted data and the reference alone; the engine only says which blocks exist."""
import numpy as np

import analytic_maps as am
import ref64

W_IMG, H_IMG = 61, 47
VS = 2.0 ** -6
STEP = 2.0 ** -10                      # the depth unit: 16 steps per voxel
INTR = np.array([16.0, 16.0, 30.0, 23.0], np.float32)
MU_STEPS = (64, 48)                    # mu = 2^-4 (eta / mu is exact) and 3 * 2^-6 (the quotient rounds)
# Every pose puts the block boundaries at camera depths of 8 k + 2 voxels.  Image rows from FLAT_ROW on see a plane on the
# voxel grid at Z_NEAR + mu, the other rows a random whole number of voxels up to Z_SPAN - 1 behind it plus a class offset:
# the nearest allocated block starts where eta = mu, so few voxels lie in front of the band (f = 1 with a small weight makes
# the quotient a ratio of small integers: nearly half of those are ties at max_w = 4, whatever the band).
FLAT_ROW, Z_NEAR, Z_SPAN = 30, 50, 2
# Depth weighting: w = roundf(n (1 - d / 2)), exact for dyadic d.  Every crafted depth lies in 0.82 .. 0.88 m, so a case
# meets ONE new weight: 3 with max_new_w = 5 (the fusions and the batch); the depth-weighted de-integrations take
# max_new_w = 4, 5, 7, 9 in turn with the pose, which gives w = 2, 3, 4, 5.
WP = (True, 5, 2.0)
WP_DEINT = ((True, 5, 2.0), (True, 4, 2.0), (True, 7, 2.0), (True, 9, 2.0))
FORMS = ("plain", "stop", "depth_weights", "two_cameras", "deprocess", "deprocess_two_cameras", "deprocess_stop",
         "deprocess_depth_weights", "deprocess_two_cameras_depth_weights")
MAX_WS = (100, 4, 255)
TIE_CAP = {100: 0.05, 255: 0.05, 4: 0.15}
PRED_TIE_LIMIT = 1e-3
REACH_MIN = 512


def pose(k, D=(0, 0, 0)):
    """World -> camera: the identity or a quarter turn about y, x or z, then a translation of whole voxels.  `D`: the
    world moved by that many blocks (D / 8 m each: every entry stays a dyadic number float32 holds exactly)."""
    R = [np.eye(3), [[0, 0, -1], [0, 1, 0], [1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]]][k % 4]
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.array([3, -5, 2]) * VS
    T = np.eye(4)
    T[:3, 3] = -8.0 * VS * np.asarray(D, np.float64)
    out = (M @ T).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), M @ T), "the moved pose is not exact in float32"
    return out


def rgb_camera(M):
    """A colour camera two voxels to the side of and one above the depth camera: an exact translation."""
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = np.array([2, -1, 0]) * VS
    return (T @ M).astype(np.float32)


def offsets(mu_steps):
    """Sub-voxel depth offsets (in steps) that put eta on -mu, 0, +-mu / 4 and mu and one step either side of each."""
    q = (mu_steps // 4) % 16
    return sorted({0, 1, 15, q, (q + 1) % 16, (q - 1) % 16, (16 - q) % 16, (17 - q) % 16, (15 - q) % 16})


def images(mu_steps, seed):
    """(rgba, raw depth): the plane below FLAT_ROW, random depths with the class offsets above it, holes (0 and negative
    raw values) everywhere; colours random on the left, 255 in the middle, 0 on the right."""
    rng = np.random.default_rng(seed)
    off = np.array(offsets(mu_steps))
    flat = Z_NEAR * 16 + mu_steps
    raw = flat + rng.integers(0, Z_SPAN, (H_IMG, W_IMG)) * 16 + off[rng.integers(0, len(off), (H_IMG, W_IMG))]
    yy, xx = np.mgrid[FLAT_ROW:H_IMG, 0:W_IMG]
    raw[FLAT_ROW:] = flat + 7 * ((xx + yy) % 2)  # on the voxel grid (eta = -mu is met exactly) and 7 steps behind it, in turn
    hole = rng.random((H_IMG, W_IMG))
    raw[hole < 0.015] = 0
    raw[(hole >= 0.015) & (hole < 0.03)] = -rng.integers(1, 2000, (H_IMG, W_IMG))[(hole >= 0.015) & (hole < 0.03)]
    rgba = rng.integers(0, 256, (H_IMG, W_IMG, 4)).astype(np.uint8)
    rgba[:, 27:40, :3] = 255
    rgba[:, 48:, :3] = 0
    return rgba, raw.astype(np.int16)


def edge_rows(max_w):
    """The cycles an edge block draws from: (sdf values, depth weights, colours, colour weights).  The lengths 7 and 10,
    3 and 7 are coprime, so the block sequence meets every pair.  Depth weights: 0, 1, max_w - 1, max_w, 255, and 2 .. 6:
    whichever new weight w = 1 .. 5 a de-integration case runs with (one per case: 1 without depth weighting, else
    WP_DEINT), the rows hold W == w, W == w + 1 (amplification w + 1, the largest) and W < w.  +-30000 with W == w + 1
    makes the de-integration's quotient clamp on either side."""
    return ([32767, -32767, 12345, -20000, 0, 30000, -30000], [0, 1, max_w - 1, max_w, 255, 2, 6, 3, 5, 4],
            [(0, 0, 0), (255, 255, 255), (10, 250, 128)], [0, 1, 2, 7, max(max_w - 1, 0), max_w, 255])


def crafted_voxels(n, max_w, seed, minus_blocks):
    """n voxel blocks: even ones random, odd ones an edge row each; `minus_blocks` (a mask) get sdf -32767."""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 512), am.VOXEL_DTYPE)
    v["sdf"] = rng.integers(-32767, 32768, (n, 512))
    v["clr"] = rng.integers(0, 256, (n, 512, 3))
    v["w_depth"] = rng.integers(0, max_w + 1, (n, 512))
    v["w_color"] = rng.integers(0, max_w + 1, (n, 512))
    v["_pad"] = rng.integers(0, 256, (n, 512))
    sdfs, wds, clrs, wcs = edge_rows(max_w)
    for i in range(1, n, 2):
        j = i // 2
        v["sdf"][i] = -32767 if minus_blocks[i] else sdfs[j % len(sdfs)]
        v["w_depth"][i] = wds[j % len(wds)]
        v["clr"][i] = clrs[j % len(clrs)]
        v["w_color"][i] = wcs[j % len(wcs)]
    return v


def reach(vox, info, mu_steps, max_w, deintegrate, wp):
    """Voxels that meet each edge, from the crafted voxels and the reference's measurements."""
    W, Wc, s = vox["w_depth"].astype(np.int64), vox["w_color"].astype(np.int64), vox["sdf"].astype(np.int64)
    t, cs, w = info["taken"], info["colour_seen"], info["w_new"]
    with np.errstate(invalid="ignore"):
        e = np.where(info["seen"], np.round(info["eta"] / STEP), 1 << 40).astype(np.int64)
    m = info["sample"]
    out = {}
    for name, at in (("-mu", -mu_steps), ("0", 0), ("mu/4", mu_steps // 4), ("-mu/4", -(mu_steps // 4)), ("mu", mu_steps)):
        for d in (-1, 0, 1):
            out[f"eta={name}{d:+d}"] = int((e == at + d).sum())
    out["eta>mu"] = int(((e > mu_steps + 1) & info["seen"]).sum())
    for k in (0, 1, max_w - 1, max_w, 255):
        out[f"W={k}"] = int((t & (W == k)).sum())
    for k in (0, 1, max_w, 255):
        out[f"Wc={k}"] = int((cs & (Wc == k)).sum())
    out["sdf+S_meets_f+1"] = int((t & (s == 32767) & (info["f"] == 1)).sum())
    out["sdf-S_meets_f-1"] = int((t & (s == -32767) & (info["f"] == -1)).sum())
    out["colour_0_meets_255"] = int((cs & (vox["clr"] == 0).all(-1) & (m == 255).all(-1)).sum())
    out["colour_255_meets_0"] = int((cs & (vox["clr"] == 255).all(-1) & (m == 0).all(-1)).sum())
    if deintegrate:
        q = info["q_sdf"]
        out["W==w"] = int((t & (W == w)).sum())
        out["W<w"] = int((t & (W < w)).sum())
        out["W<w_colour_updates"] = int((info["upd_colour"] & (W < w)).sum())
        out["W==w+1"] = int((t & (W == w + 1)).sum())
        out["clamps_high"] = int((info["upd_depth"] & (W > w) & (q > 32767 + 1)).sum())
        out["clamps_low"] = int((info["upd_depth"] & (W > w) & (q < -32767 - 1)).sum())
        out["colour_clamps"] = int((info["upd_colour"][..., None] & ((info["q_clr"] > 256) | (info["q_clr"] < -1))).sum())
    elif wp is not None and max_w == 255:
        out["W+w>255"] = int((info["upd_depth"] & (W + w > 255)).sum())
    return out


def _entries(api, scene, rs):
    h = api.download_hash_table(scene)
    e = h[api.download_visible_ids(rs)]
    e = e[e["ptr"] >= 0]
    return e["ptr"].astype(np.int64), e["pos"].astype(np.int64)


class Case:
    """One scene with its crafted measurement, allocated and overwritten; `expect` is the reference's answer to a call."""

    def __init__(self, api, pkg, max_w, mu_steps, form, pose_k=0, D=(0, 0, 0), **scene_kw):
        self.api, self.form, self.max_w, self.mu_steps = api, form, max_w, mu_steps
        self.deint = form.startswith("deprocess")
        self.stop = form.endswith("stop")
        self.wp = (WP_DEINT[pose_k % 4] if self.deint else WP) if form.endswith("depth_weights") else None
        self.mu = mu_steps * STEP
        self.M = pose(pose_k, D)
        self.M_rgb = rgb_camera(self.M) if "two_cameras" in form else None
        kw = dict(voxel_size=VS, mu=self.mu, max_w=max_w, frustum_min=0.2, frustum_max=3.0, num_local_blocks=0x800,
                  num_buckets=0x1000, num_excess=0x400, stop_integrating_at_max_w=int(self.stop))
        kw.update(scene_kw)
        self.scene = api.create_scene(pkg.SceneParams(**kw))
        self.rs = api.create_render_state(self.scene, W_IMG, H_IMG)
        self.view = api.create_view(W_IMG, H_IMG)
        self.seed = 1000 * max_w + 10 * mu_steps + pose_k
        self.rgba, self.raw = images(mu_steps, self.seed)
        api.view_update(self.view, self.rgba, self.raw, affine_a=STEP)
        self.depth = api.download_view_depth(self.view)
        assert np.array_equal(self.depth, ref64.depth_to_float(self.raw, a=STEP).astype(np.float32)), "depth conversion (A.3)"
        n = -1  # (a pass allocates one block per bucket: repeated until a pass finds every block in place)
        while api.stats(self.scene, self.rs)["no_visible_entries"] != n:
            n = api.stats(self.scene, self.rs)["no_visible_entries"]
            api.allocate_scene_from_depth(self.scene, self.view, self.rs, self.M, INTR)
        self.ptrs, self.pos = _entries(api, self.scene, self.rs)
        assert len(np.unique(self.ptrs)) == len(self.ptrs) >= 200, len(self.ptrs)
        # where eta is exactly -mu (f = -1): blocks that hold at least 16 such voxels get the sdf -32767 row
        probe = self.expect(np.zeros((len(self.ptrs), 512), am.VOXEL_DTYPE))[2]
        at_minus_mu = (probe["taken"] & (probe["f"] == -1)).sum(axis=1)
        self.crafted = crafted_voxels(len(self.ptrs), max_w, self.seed + 1, at_minus_mu >= 16)
        self.before = api.download_voxel_blocks(self.scene)
        self.before[self.ptrs] = self.crafted
        api.upload_voxel_blocks(self.scene, 0, self.before)
        self.lo, self.hi, self.info = self.expect(self.crafted)
        self.figures = self._reference_alone()

    def expect(self, vox):
        return ref64.update_exact(vox, self.pos, self.depth, self.rgba, self.M, INTR, VS, self.mu, self.max_w, M_rgb=self.M_rgb,
                                  stop_at_max=self.stop, wp=self.wp, deintegrate=self.deint)

    def _reference_alone(self):
        """Reach, tie shares and their caps: no engine value enters."""
        info = self.info
        r = reach(self.crafted, info, self.mu_steps, self.max_w, self.deint, self.wp)
        if self.wp is not None:  # the one new weight this case meets
            want = {WP: 3, WP_DEINT[1]: 2, WP_DEINT[2]: 4, WP_DEINT[3]: 5}[self.wp]
            assert np.unique(info["w_new"][info["taken"]]).tolist() == [want]
        short = {k: v for k, v in r.items() if v < REACH_MIN}
        if self.stop and not self.deint:  # (the voxels at max_w are met and, by the rule under test, left alone)
            assert not info["upd_depth"][self.crafted["w_depth"] == self.max_w].any()
        assert not short, f"edges reached in fewer than {REACH_MIN} voxels: {short}"
        random_half = np.arange(len(self.ptrs)) % 2 == 0
        share = ref64.update_tie_share(info, random_half)
        assert share <= TIE_CAP[self.max_w], f"tie share of the random half {share:.4f}"
        pred = int(info["pred_tie"].sum())
        assert pred <= PRED_TIE_LIMIT * int(info["projected"].sum()), f"{pred} predicate ties"
        changed = (self.lo.view(np.uint64) != self.crafted.view(np.uint64)) | (self.hi.view(np.uint64) != self.crafted.view(np.uint64))
        assert changed.sum() > 20000, int(changed.sum())
        return dict(blocks=len(self.ptrs), reach=r, tie_share_random_half=share, tie_share_all=ref64.update_tie_share(info),
                    predicate_ties=pred, updated_depth=int(info["upd_depth"].sum()), updated_colour=int(info["upd_colour"].sum()))

    def conditions(self):
        """What selects the kernel form in csrc/integrate.hip, read back from the scene and the case: the scene's
        stopIntegratingAtMaxW and swapping, depth weighting, a second camera; dirty marks and shards are off unless a call
        turns them on, and no case does."""
        p = self.scene.params
        return dict(stop=p.stop_integrating_at_max_w, swapping=p.use_swapping, depth_weights=self.wp is not None,
                    two_cameras=self.M_rgb is not None, deintegrate=self.deint)

    def call(self, process_frame=False):
        """The one call under test; `process_frame`: ProcessFrame (its allocation pass finds every block in place) instead
        of IntegrateIntoScene."""
        api, kw = self.api, dict(M_rgb=self.M_rgb, intr_rgb=None if self.M_rgb is None else INTR)
        if self.wp is not None:
            api.set_fusion_weight_params(*self.wp)
        try:
            if self.deint:
                api.deprocess_frame(self.scene, self.view, self.rs, self.M, INTR, **kw)
            elif process_frame:
                api.process_frame(self.scene, self.view, self.rs, self.M, INTR, **kw)
            else:
                api.integrate_into_scene(self.scene, self.view, self.rs, self.M, INTR, **kw)
        finally:
            if self.wp is not None:
                api.set_fusion_weight_params()

    def check(self):
        """The engine's voxels after the call: the visible blocks against the reference, every other block byte for byte."""
        api = self.api
        ptrs, _ = _entries(api, self.scene, self.rs)
        assert np.array_equal(np.sort(ptrs), np.sort(self.ptrs)), "the call changed the set of visible blocks"
        after = api.download_voxel_blocks(self.scene)
        what = f"{self.form}, max_w {self.max_w}, mu {self.mu_steps} / 1024"
        self.figures["values"] = ref64.check_updated(after[self.ptrs], self.lo, self.hi, self.info, what)
        rest = np.ones(len(after), bool)
        rest[self.ptrs] = False
        assert after[rest].tobytes() == self.before[rest].tobytes(), f"{what}: a block outside the visible list changed"
        return self.figures


def cases():
    """(max_w, mu in steps, form, pose): every form at every max_w with mu = 2^-4, and at max_w 100 with the other mu."""
    out = []
    for i, mw in enumerate(MAX_WS):
        for j, form in enumerate(FORMS):
            out.append((mw, MU_STEPS[0], form, (i + j) % 4))
    for j, form in enumerate(FORMS):
        out.append((100, MU_STEPS[1], form, (j + 1) % 4))
    return out


def case_id(c):
    return f"maxw{c[0]}-mu{c[1]}-{c[2]}-pose{c[3]}"


def run_case(api, pkg, max_w, mu_steps, form, pose_k):
    c = Case(api, pkg, max_w, mu_steps, form, pose_k)
    c.call()
    return c.check()


# ---------------------------------------------------------------------------------------------------------------------
# The re-integration batch: three crafted keyframes in a frame store, corrected keyframe by keyframe from their lists
# ---------------------------------------------------------------------------------------------------------------------
# The lists are the engine's own (the render state's visible list when the keyframe was fused, and again after its
# re-fusion); nothing here models which blocks a step touches.  Every step's voxels are checked against update_exact on
# the engine's bytes before that step, and the bytes after it are the next step's input.
SHARD_CHUNK = 8
BATCH_MODES = {"unit": (None, False), "depth": (WP, False), "unit_shard": (None, True), "depth_shard": (WP, True)}
KEYFRAME_SHIFTS = ((0, 0, 0), (4, -3, 0), (-5, 2, 0))   # the old poses: whole voxels, the depth layers kept (they overlap)


def _shift(M, voxels):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = np.array(voxels) * VS
    return (T @ M).astype(np.float32)


def corrected(M, k):
    """The new pose of keyframe k: an exact translation, a quarter turn about the optical axis, both."""
    roll = np.eye(4, dtype=np.float32)
    roll[:2, :2] = [[0, -1], [1, 0]]
    return [_shift(M, (2, 1, 0)), (roll @ M).astype(np.float32), _shift(roll @ M, (-1, 3, 0))][k]


def batch_cases():
    """(mode, max_w, mu in steps, pose)"""
    return [("unit", 100, MU_STEPS[1], 0), ("depth", 255, MU_STEPS[0], 1), ("unit_shard", 4, MU_STEPS[0], 2),
            ("depth_shard", 100, MU_STEPS[1], 3)]


class Batch:
    """`build` gives one copy of the state: three keyframes fused and kept in a store with their lists, then every block
    of those lists overwritten with crafted voxels.  `loop` corrects the keyframes one by one and checks every step;
    `batch` corrects them in one reintegrate_batch call."""

    def __init__(self, api, pkg, mode, max_w, mu_steps, pose_k, D=(0, 0, 0)):
        self.api, self.pkg, self.mode, self.max_w, self.mu_steps = api, pkg, mode, max_w, mu_steps
        self.wp, self.sharded = BATCH_MODES[mode]
        self.mu = mu_steps * STEP
        self.old = [_shift(pose(pose_k, D), t) for t in KEYFRAME_SHIFTS]
        self.new = [corrected(M, k) for k, M in enumerate(self.old)]
        self.seed = 7000 * max_w + 10 * mu_steps + pose_k
        self.frames = [images(mu_steps, self.seed + 100 * k) for k in range(3)]
        self.depths = [ref64.depth_to_float(raw, a=STEP).astype(np.float32) for _, raw in self.frames]
        self.what = f"batch {mode}, max_w {max_w}, mu {mu_steps} / 1024"

    def _weights(self, on=True):
        if self.wp is not None:
            self.api.set_fusion_weight_params(*(self.wp if on else ()))

    def conditions(self, h):
        """What selects the kernel form, read back from the scene and the case."""
        return dict(stop=h["scene"].params.stop_integrating_at_max_w, swapping=h["scene"].params.use_swapping,
                    depth_weights=self.wp is not None, sharded=self.sharded)

    def build(self):
        api = self.api
        scene = api.create_scene(self.pkg.SceneParams(voxel_size=VS, mu=self.mu, max_w=self.max_w, frustum_min=0.2, frustum_max=3.0,
                                                      num_local_blocks=0x800, num_buckets=0x1000, num_excess=0x400))
        if self.sharded:
            api.set_shard(scene, 0, 2, SHARD_CHUNK)
        rs, view = api.create_render_state(scene, W_IMG, H_IMG), api.create_view(W_IMG, H_IMG)
        store = api.create_frame_store(W_IMG, H_IMG, 3)
        api.frame_store_enable_lists(store, scene)
        lists = []
        self._weights()
        try:
            for k, (rgba, raw) in enumerate(self.frames):
                api.view_update(view, rgba, raw, affine_a=STEP, timestamp=float(k))
                api.frame_store_put_view(store, k, view)
                api.process_frame(scene, view, rs, self.old[k], INTR)
                api.frame_store_put_visible_list(store, k, scene, rs)
                lists.append(_entries(api, scene, rs))
        finally:
            self._weights(False)
        ptrs, first = np.unique(np.concatenate([p for p, _ in lists]), return_index=True)
        pos = np.concatenate([q for _, q in lists])[first]
        assert min(len(p) for p, _ in lists) >= 150 and len(ptrs) < 0.7 * sum(len(p) for p, _ in lists), "the keyframes must overlap"
        probe = ref64.update_exact(np.zeros((len(ptrs), 512), am.VOXEL_DTYPE), pos, self.depths[0], self.frames[0][0], self.old[0],
                                   INTR, VS, self.mu, self.max_w, wp=self.wp, deintegrate=True)[2]
        minus = (probe["taken"] & (probe["f"] == -1)).sum(axis=1) >= 16
        state = api.download_voxel_blocks(scene)
        state[ptrs] = crafted_voxels(len(ptrs), self.max_w, self.seed + 1, minus)
        api.upload_voxel_blocks(scene, 0, state)
        return dict(scene=scene, rs=rs, view=view, store=store, lists=lists, crafted=(ptrs, pos), state=state)

    def _step(self, h, before, entries, k, M, deint, figures):
        """One de-integration or re-fusion of keyframe k over the blocks `entries`: this rank's against update_exact on
        `before`, every other block byte for byte.  Returns the engine's bytes after it."""
        ptrs, pos = entries
        own = (ptrs // SHARD_CHUNK) % 2 == 0 if self.sharded else np.ones(len(ptrs), bool)
        assert own.sum() >= 50 and (not self.sharded or (~own).sum() >= 50), "both ranks must own blocks of the list"
        lo, hi, info = ref64.update_exact(before[ptrs[own]], pos[own], self.depths[k], self.frames[k][0], M, INTR, VS, self.mu,
                                          self.max_w, wp=self.wp, deintegrate=deint)
        assert info["upd_depth"].sum() > 5000, int(info["upd_depth"].sum())
        pred = int(info["pred_tie"].sum())
        assert pred <= PRED_TIE_LIMIT * int(info["projected"].sum()), f"{pred} predicate ties"
        name = f"keyframe {k} {'de-integrated' if deint else 're-fused'}"
        fig = dict(blocks=int(own.sum()), updated_depth=int(info["upd_depth"].sum()), tie_share=ref64.update_tie_share(info),
                   new_weights=np.unique(info["w_new"][info["taken"]]).tolist())
        if not figures:  # the first step meets the crafted voxels: the caps and the de-integration's edges, reference alone
            places = np.searchsorted(h["crafted"][0], ptrs[own])
            fig["tie_share_random_half"] = ref64.update_tie_share(info, places % 2 == 0)
            assert fig["tie_share_random_half"] <= TIE_CAP[self.max_w], fig
            r = reach(before[ptrs[own]], info, self.mu_steps, self.max_w, True, self.wp)
            fig["reach"] = {e: r[e] for e in ("W==w", "W<w", "W<w_colour_updates", "W==w+1", "clamps_high", "clamps_low")}
            if not self.sharded:  # (a rank sees half of the blocks)
                short = {e: n for e, n in fig["reach"].items() if n < REACH_MIN}
                assert not short, f"edges reached in fewer than {REACH_MIN} voxels: {short}"
        after = self.api.download_voxel_blocks(h["scene"])
        fig["values"] = ref64.check_updated(after[ptrs[own]], lo, hi, info, f"{self.what}, {name}")
        rest = np.ones(len(after), bool)
        rest[ptrs[own]] = False
        assert after[rest].tobytes() == before[rest].tobytes(), f"{self.what}, {name}: a block outside the list (or of the other rank) changed"
        figures[name] = fig
        return after

    def loop(self, h):
        """The per-keyframe calls that define the batch, each step checked.  Returns the figures per step."""
        api, scene, rs, view, store = self.api, h["scene"], h["rs"], h["view"], h["store"]
        state, figures = h["state"], {}
        self._weights()
        try:
            for k in range(3):
                api.view_update_from_store(view, store, k, affine_a=STEP, timestamp=float(k))
                assert np.array_equal(api.download_view_depth(view), self.depths[k]), "the stored keyframe's depth"
                api.deprocess_frame_stored(scene, view, store, k, self.old[k], INTR)
                state = self._step(h, state, h["lists"][k], k, self.old[k], True, figures)
                api.process_frame(scene, view, rs, self.new[k], INTR, is_defusion=True)
                entries = _entries(api, scene, rs)   # the list the re-fusion ran over: as the engine built it
                state = self._step(h, state, entries, k, self.new[k], False, figures)
                api.frame_store_put_visible_list(store, k, scene, rs)
        finally:
            self._weights(False)
        return figures

    def batch(self, h):
        self._weights()
        try:
            self.api.reintegrate_batch(h["scene"], h["view"], h["rs"], h["store"], [0, 1, 2], self.old, self.new, INTR, affine_a=STEP)
        finally:
            self._weights(False)


def run_batch(api, pkg, mode, max_w, mu_steps, pose_k, D=(0, 0, 0)):
    """Two copies of one state; the checked loop on the first, one batch call on the second; the two must be equal byte
    for byte (map, table, free lists, render state).  Returns (batch rig, the second copy, figures)."""
    import scenarios
    b = Batch(api, pkg, mode, max_w, mu_steps, pose_k, D)
    h1, h2 = b.build(), b.build()
    assert h1["state"].tobytes() == h2["state"].tobytes() and all(np.array_equal(x[0], y[0]) for x, y in zip(h1["lists"], h2["lists"]))
    figures = b.loop(h1)
    b.batch(h2)
    scenarios.assert_same_full_state(scenarios.full_state(api, h2["scene"], h2["rs"]), scenarios.full_state(api, h1["scene"], h1["rs"]),
                                     f"{b.what}: one batch call vs the checked per-keyframe loop")
    return b, h2, figures
