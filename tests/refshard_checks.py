"""Check bodies of the shard tests: an engine's ownership gate, dirty marks, plan, pack and unpack against the law of
ref_shard.py.  They take an `api` (the HIP engine or the CPU oracle) and are run by test_oracle_shard.py and
test_gpu_shard.py.  Every comparison is of bytes: there is no tolerance anywhere."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import ref_shard as law
import refmap_checks as rm
import scenarios
import shard_fixtures as sf

BLOCK = law.BLOCK_BYTES


def _bytes(u64_blocks):
    return np.ascontiguousarray(u64_blocks).view(np.uint8).reshape(-1, BLOCK)


def caps_for(count):
    """count, count + 2, count - 1, 1 and 0, each once and none below zero."""
    return sorted({c for c in (count, count + 2, count - 1, 1, 0) if c >= 0})


def check_pack(api, scene, send, pool, lists, r, cap, what):
    """One pack at capacity `cap` into a buffer of pattern bytes: the first min(count_r, cap) blocks of the capacity hold the
    law's blocks, and every other byte of the buffer -- the rest of the capacity and the guards -- is still the pattern."""
    send.fill(sf.PATTERN)
    api.shard_dirty_pack(scene, r, send.ptr, cap)
    sf.sync(api)
    got = send.host()
    want = np.full_like(got, sf.PATTERN)
    blocks = law.pack(pool, lists, r, cap)
    want[sf.GUARD:sf.GUARD + len(blocks)] = _bytes(blocks)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(1))[0] - sf.GUARD
        raise AssertionError(f"{what}: shard {r}, cap {cap}, count {len(lists[r])}: buffer blocks {bad[:8].tolist()} "
                             f"({len(bad)} in all, counted from the start of the capacity) differ from the law")


def gathered(n, lists, stride, shards):
    """What the all-gather delivers at `stride`: row r holds the first `stride` blocks of shard r as REPLICA r packed them
    (signature blocks: replica r, slot), and padding behind its last block."""
    body = np.full((shards, stride, 512), np.uint64(sf.PADDING) * np.uint64(0x0101010101010101), np.uint64)
    for r, slots in enumerate(lists):
        k = min(len(slots), stride)
        body[r, :k] = sf.signatures(n, r)[slots[:k]]
    return body


def check_exchange(api, pkg, layout, which):
    """One dirty set on one layout: counts, pack at every capacity for every shard, unpack on every replica at the full and
    at a truncated stride; a plan with another layout first, which must not govern; after a fresh track_dirty(1) pack and
    unpack want a new plan.  Returns the counts (the tests print them)."""
    c = sf.Crafted(api, pkg, layout)
    n, shards, chunk = c.n, c.shards, c.chunk
    dirty = sf.dirty_set(which, n, shards, chunk)
    what = f"{layout}, {which}"
    pool = c.upload_signatures(0)
    c.mark(dirty, seed=shards)

    # two plans on the same marks: the second governs
    o_shards, o_chunk = sf.other_layout(n, shards, chunk)
    assert api.shard_dirty_plan(c.scene, o_shards, o_chunk) == law.plan(dirty, n, o_shards, o_chunk)[1], f"{what}: counts of the first plan"
    lists, counts = law.plan(dirty, n, shards, chunk)
    assert api.shard_dirty_plan(c.scene, shards, chunk) == counts, f"{what}: counts"
    if shards > 1 and which == "last_shard_only":
        assert counts[-1] > 0 and not any(counts[:-1]), "fixture: shards with a count of 0 in front of one that has blocks"
    if shards > 1 and which == "first_shard_only":
        assert counts[0] > 0 and not any(counts[1:]), "fixture: shards with a count of 0 behind one that has blocks"

    send = sf.Buffer(api, max(counts) + 2)
    for r in range(shards):
        for cap in caps_for(counts[r]):
            check_pack(api, c.scene, send, pool, lists, r, cap, what)
    with pytest.raises(pkg.DslamError):
        api.shard_dirty_pack(c.scene, shards, send.ptr, 0)

    # unpack: replica q holds signature blocks of its own and skips its own shard; once nothing is skipped
    for stride in (max(counts), max(counts) - 1):
        if stride < 1:
            continue
        body = gathered(n, lists, stride, shards)
        recv = sf.Buffer(api, shards * stride)
        recv.fill(sf.PATTERN)
        recv.load(body)
        for q, skip in [(r, r) for r in range(shards)] + [(shards, -1)]:
            mine = c.upload_signatures(q)
            api.shard_dirty_unpack(c.scene, skip, recv.ptr, stride)
            sf.sync(api)
            want = law.unpack(mine, lists, skip, body, stride)
            got = c.pool()
            if not np.array_equal(got, want):
                bad = np.nonzero((got != want).any(1))[0]
                raise AssertionError(f"{what}: unpack on replica {q} (skip {skip}) at stride {stride}: blocks {bad[:8].tolist()} "
                                     f"({len(bad)} in all) differ from the law")
            assert recv.guards_intact(sf.PATTERN), f"{what}: unpack wrote to its recv buffer's guards"
        assert np.array_equal(recv.host(sf.GUARD, sf.GUARD + recv.blocks), _bytes(body)), f"{what}: unpack wrote to its recv buffer"

    # new marks: the plan is forgotten
    api.track_dirty(c.scene, True)
    with pytest.raises(pkg.DslamError):
        api.shard_dirty_pack(c.scene, 0, send.ptr, 0)
    with pytest.raises(pkg.DslamError):
        api.shard_dirty_unpack(c.scene, -1, send.ptr, 0)
    assert api.shard_dirty_plan(c.scene, shards, chunk) == [0] * shards, f"{what}: track_dirty(1) did not clear the marks"
    api.track_dirty(c.scene, False)
    return counts


def check_refusals(api, pkg):
    c = sf.Crafted(api, pkg, "0x300-3x256")
    with pytest.raises(pkg.DslamError):
        api.shard_dirty_plan(c.scene, 3, 256)          # track_dirty was never enabled
    c.upload_signatures(0)
    c.mark({5, 300, 700})
    for shards, chunk in ((5, 16), (2, 256), (65, 1), (0, 1), (3, 0), (-3, -256)):   # 768 = 3 * 256 is no multiple of 80 or 512
        assert not law.valid_layout(c.n, shards, chunk)
        with pytest.raises(pkg.DslamError):
            _plan(api, c.scene, shards, chunk)
    assert api.shard_dirty_plan(c.scene, 64, 4) == law.plan({5, 300, 700}, c.n, 64, 4)[1]    # the limit itself is legal
    buf = sf.Buffer(api, 4)
    buf.fill(sf.PATTERN)
    for shard in (64, -1):
        with pytest.raises(pkg.DslamError):
            api.shard_dirty_pack(c.scene, shard, buf.ptr, 4)
    sf.sync(api)
    assert (buf.host() == sf.PATTERN).all()


def _plan(api, scene, shards, chunk):
    """shard_dirty_plan for argument values the wrapper cannot size a result for."""
    counts = (C.c_int32 * 128)()
    api._call("shard_dirty_plan", api._engine, scene.ptr, C.c_int(shards), C.c_int(chunk), counts)
    return list(counts)


# ---- ownership and marks of the real calls ---------------------------------------------------------------------------
W, H = 96, 72
VOXEL = 0.0062                    # metres: the six keyframes below fill three quarters of the pool
N_REAL, REAL_BUCKETS, REAL_EXCESS = 0xF00, 0x400, 0x1000      # 0xF00 is a multiple of 3 * 16 and of 64 * 4
KEYFRAMES = (0, 1, 2, 3, 4, 5)    # frames of s_tiny, 2 degrees of yaw apart: every keyframe sees most of what the others saw
UPKEEP_AFTER = 4                  # the window and decay step runs after this keyframe ...
STORED_K = 4                      # ... so this keyframe's stored list names blocks that have gone or moved since
NEW_FRAME = 6
BATCH = (5, 3, 4)                 # (its re-fusions run the pool dry: allocation is replicated, so on every rank alike)
# "stream" / "deprocess_stream": the same call with every launch told to take the streaming cache policy (HIP engine only).
# The fusion has a streaming instantiation for its plain form alone, so only the unsharded, unmarked twin takes it; the
# one-camera de-integration has one that carries the gate and the mark, and the replicas take it too.
FORMS = ("process_frame", "stream", "two_cameras", "deprocess_frame", "deprocess_stream", "deprocess_stored", "batch_unit",
         "batch_weighted")
HIP_ONLY_FORMS = ("stream", "deprocess_stream")
SETTINGS = ("shard-2x1", "shard-3x16", "shard-64x4", "range", "both", "off")
REACH = 30                        # blocks the twin changes that the replica owns, and that it does not own
REACH_SKIPPED = 10                # stored entries the position or residency rule skips

_frames = {}


def _frame(synth, i):
    if i not in _frames:
        _frames[i] = synth.s_tiny(W, H).frame(i)
    return _frames[i]


def _corrected(synth, i, n):
    wl = synth.s_tiny(W, H)
    return synth.world_to_camera(wl.pose(i) @ synth.pose_matrix(synth.look_rotation(0.003 * (n + 1), -0.002), [0.004, 0.001 * n, -0.003]))


class Real:
    """One replay of the base sequence: six keyframes into a frame store with their lists, a window and decay step in
    between.  With record=True the lists are also kept on the host, with the block positions at the time they were stored."""

    def __init__(self, api, pkg, synth, record=False):
        self.api, self.pkg, self.synth, self.record = api, pkg, synth, record
        self.intr = synth.s_tiny(W, H).intr
        p = rm.scene_params(pkg, vs=VOXEL, num_local_blocks=N_REAL, num_buckets=REAL_BUCKETS, num_excess=REAL_EXCESS, history_words=1)
        self.scene = api.create_scene(p)
        self.rs, self.view = api.create_render_state(self.scene, W, H), api.create_view(W, H)
        self.store = api.create_frame_store(W, H, len(KEYFRAMES))
        api.frame_store_enable_lists(self.store, self.scene)
        self.poses, self.stored = {}, {}
        for k, f in enumerate(KEYFRAMES):
            rgba, mm, M = _frame(synth, f)
            api.view_update(self.view, rgba, mm, timestamp=float(f))
            api.frame_store_put_view(self.store, k, self.view)
            api.process_frame(self.scene, self.view, self.rs, M, self.intr)
            self.put_list(k)
            self.poses[k] = M
            if k == UPKEEP_AFTER:
                api.slide_window(self.scene, self.rs, 2)
                api.decay(self.scene, self.rs, 1, 0, True)

    def put_list(self, k):
        self.api.frame_store_put_visible_list(self.store, k, self.scene, self.rs)
        if self.record:
            ids = self.api.download_visible_ids(self.rs)
            self.stored[k] = (ids, self.api.download_hash_table(self.scene)["pos"][ids].copy())

    def voxels(self):
        return self.api.download_voxel_blocks(self.scene).view(np.uint64).reshape(N_REAL, 512)

    def state(self):
        return scenarios.full_state(self.api, self.scene, self.rs)


@contextlib.contextmanager
def _streaming(api, on, launches):
    """With `on`, every launch inside counts as larger than the cache (dslam_debug_set_push_job_min(0)), and `launches` of
    them must have taken a streaming instantiation."""
    if not on:
        yield
        return
    before = api.debug_stream_launches()
    api.debug_set_push_job_min(0)
    try:
        yield
    finally:
        api.debug_set_push_job_min(65536)
    assert api.debug_stream_launches() - before == launches, "not the instantiation this form is about"


def run_form(R, form):
    """The call under test.  On a recording replay (the unsharded twin) the batch forms run as the loop that defines them, and
    the return value is (D, skipped): the slots the law says are marked, from downloads alone, and the number of stored
    entries the position or residency rule skipped."""
    api, synth, rec = R.api, R.synth, R.record
    D, skipped = set(), 0
    table = (lambda: api.download_hash_table(R.scene)) if rec else (lambda: None)
    vis = (lambda: api.download_visible_ids(R.rs)) if rec else (lambda: None)

    def stored_step(k, old_M):
        nonlocal D, skipped
        api.view_update_from_store(R.view, R.store, k, timestamp=float(KEYFRAMES[k]))
        if rec:
            t, (ids, pos) = table(), R.stored[k]
            m = law.marks(t["ptr"], ids, t["pos"], pos)
            same = (t["pos"][ids] == pos).all(-1) & (t["ptr"][ids] >= 0)
            assert len(m) == int(same.sum())
            skipped += int((~same).sum())
            D |= m
        api.deprocess_frame_stored(R.scene, R.view, R.store, k, old_M, R.intr)

    if form in ("process_frame", "stream"):
        rgba, mm, M = _frame(synth, NEW_FRAME)
        api.view_update(R.view, rgba, mm, timestamp=float(NEW_FRAME))
        with _streaming(api, form == "stream", 1 if rec else 0):
            api.process_frame(R.scene, R.view, R.rs, M, R.intr)
        if rec:
            D = law.marks(table()["ptr"], vis())
    elif form == "two_cameras":     # the last keyframe's images once more, over the list its fusion left, colour from a camera of its own
        k = len(KEYFRAMES) - 1
        M_rgb = _corrected(synth, KEYFRAMES[k], 3)
        intr_rgb = R.intr * np.float32(0.97)
        if rec:
            D = law.marks(table()["ptr"], vis())
        api.integrate_into_scene(R.scene, R.view, R.rs, _corrected(synth, KEYFRAMES[k], 0), R.intr, M_rgb=M_rgb, intr_rgb=intr_rgb)
    elif form in ("deprocess_frame", "deprocess_stream"):
        k = len(KEYFRAMES) - 2
        api.view_update_from_store(R.view, R.store, k, timestamp=float(KEYFRAMES[k]))
        with _streaming(api, form == "deprocess_stream", 1):
            api.deprocess_frame(R.scene, R.view, R.rs, R.poses[k], R.intr)
        if rec:
            D = law.marks(table()["ptr"], vis())
    elif form == "deprocess_stored":
        stored_step(STORED_K, R.poses[STORED_K])
    elif form in ("batch_unit", "batch_weighted"):
        new = [_corrected(synth, KEYFRAMES[k], n) for n, k in enumerate(BATCH)]
        old = [R.poses[k] for k in BATCH]
        if form == "batch_weighted":
            api.set_fusion_weight_params(True, 5, 2.5)
        try:
            if rec:   # include/dslam_fusion.h: the loop that defines the batch
                for k, o, m in zip(BATCH, old, new):
                    stored_step(k, o)
                    api.process_frame(R.scene, R.view, R.rs, m, R.intr, is_defusion=True)
                    D |= law.marks(table()["ptr"], vis())
                    R.put_list(k)
            else:
                api.reintegrate_batch(R.scene, R.view, R.rs, R.store, list(BATCH), old, new, R.intr)
        finally:
            if form == "batch_weighted":
                api.set_fusion_weight_params(False, 1, 1.0)
    else:
        raise ValueError(form)
    return D, skipped


class Twin:
    """The unsharded run of one form, and what the law needs of it."""

    def __init__(self, api, pkg, synth, form):
        R = Real(api, pkg, synth, record=True)
        self.before = R.voxels()
        self.D, self.skipped = run_form(R, form)
        self.after = R.state()
        self.after_voxels = self.after["voxels"].view(np.uint64).reshape(N_REAL, 512)
        self.changed = (self.before != self.after_voxels).any(1)
        assert self.changed[sorted(self.D)].sum() == self.changed.sum(), "a block changed that the law does not mark"
        if form == "deprocess_stored":
            assert self.skipped >= REACH_SKIPPED, f"fixture: only {self.skipped} stored entries are skipped"

    def gates(self, setting):
        """The replica's gates, chosen from the twin alone so that the reach is there.  The range runs from the changed slot
        nearest the 30 % quantile of the changed slots to the one nearest the 70 % quantile, neither on a chunk border: the
        first slot inside and the first slot behind the range are both blocks the twin changes, so either end, off by one,
        shows.  The shard is the one that owns most of the changed blocks; with both gates, the one that owns the slot
        behind the range."""
        ch = np.nonzero(self.changed)[0]
        inner = ch[ch % 16 != 0]
        first, end = (int(inner[np.abs(inner - ch[int(q * len(ch))]).argmin()]) for q in (0.3, 0.7))
        count = end - first
        assert first % 16 and end % 16 and count > 0 and self.changed[first] and self.changed[end]
        if setting == "off":
            return dict(shard=0, shards=1, chunk=7, first=0, count=-1)
        g = dict(first=first, count=count) if setting in ("range", "both") else dict(first=0, count=-1)
        if setting == "range":
            return dict(g, shard=0, shards=1, chunk=256)
        shards, chunk = {"shard-2x1": (2, 1), "shard-3x16": (3, 16), "shard-64x4": (64, 4), "both": (3, 16)}[setting]
        best = int(np.bincount(law.owner(ch, shards, chunk), minlength=shards).argmax())
        g.update(shards=shards, chunk=chunk, shard=int(law.owner(end, shards, chunk)) if setting == "both" else best)
        return g


class Twins:
    """The unsharded twins of an engine, each computed once and left unchanged."""

    def __init__(self, api, pkg, synth):
        self.args, self.made = (api, pkg, synth), {}

    def __getitem__(self, form):
        if form not in self.made:
            self.made[form] = Twin(*self.args, form)
        return self.made[form]


def check_real_call(api, pkg, synth, twin, form, setting):
    """One form on one replica setting against the twin: the ownership law per block, everything that is not voxels equal,
    and D -- read by signatures -- equal to the D the law predicts from the twin's downloads."""
    g = twin.gates(setting)
    own = law.owned(np.arange(N_REAL), **g)
    reach = int((twin.changed & own).sum()), int((twin.changed & ~own).sum())
    what = f"{form}, {setting} {g}"
    print(f"{what}: the twin changes {reach[0]} blocks the replica owns and {reach[1]} it does not; |D| = {len(twin.D)}, "
          f"{twin.skipped} stored entries skipped")
    if setting != "off":
        assert min(reach) >= REACH, f"fixture: {what} reaches {reach}"
    R = Real(api, pkg, synth)
    before = R.voxels()
    assert np.array_equal(before, twin.before), f"{what}: the replays differ before the call"
    api.set_shard(R.scene, g["shard"], g["shards"], g["chunk"])
    api.set_shard_range(R.scene, g["first"], g["count"])
    api.track_dirty(R.scene, True)
    run_form(R, form)
    got = R.state()
    want = law.effect(before, twin.after_voxels, **g)
    gv = got["voxels"].view(np.uint64).reshape(N_REAL, 512)
    if not np.array_equal(gv, want):
        bad = (gv != want).any(1)
        raise AssertionError(f"{what}: {int(bad.sum())} blocks break the ownership law ({int((bad & own).sum())} of them owned), "
                             f"first slot {int(np.nonzero(bad)[0][0])}")
    if setting == "off":
        assert np.array_equal(gv, twin.after_voxels)
    scenarios.assert_same_full_state(dict(got, voxels=twin.after["voxels"]), twin.after, f"{what}: beside the voxels")
    assert read_dirty(api, pkg, R.scene, len(twin.D)) == sorted(twin.D), f"{what}: the marks are not the law's"


def read_dirty(api, pkg, scene, expected):
    """D of a scene, by signatures: its voxels are overwritten.  (The count is compared before anything is packed: a pack
    trusts the plan's counts, and a list longer than its marks would be read past its end.)"""
    n = scene.params.num_local_blocks
    api.upload_voxel_blocks(scene, 0, sf.as_voxels(pkg, sf.signatures(n, 0)))
    count, = api.shard_dirty_plan(scene, 1, n)
    assert count == expected, f"{count} slots are marked, the law says {expected}"
    buf = sf.Buffer(api, count)
    buf.fill(sf.PATTERN)
    api.shard_dirty_pack(scene, 0, buf.ptr, count)
    sf.sync(api)
    assert buf.guards_intact(sf.PATTERN)
    q, slots = sf.decode(buf.host(sf.GUARD, sf.GUARD + count))
    assert (q == 0).all()
    return slots.tolist()


def check_world_of_three(api, pkg, synth, twin):
    """The one assembled exchange: three replicas run the unit-weight batch as ranks of a world of 3 and exchange their dirty
    blocks at cap = max(counts); each must end as the unsharded twin did."""
    world, chunk = 3, 16
    ranks = [Real(api, pkg, synth) for _ in range(world)]
    lists, counts = law.plan(twin.D, N_REAL, world, chunk)
    for r, R in enumerate(ranks):
        api.track_dirty(R.scene, True)
        api.set_shard(R.scene, r, world, chunk)
        run_form(R, "batch_unit")
        assert api.shard_dirty_plan(R.scene, world, chunk) == counts, f"rank {r}: counts"
    cap = max(counts)
    assert min(counts) >= REACH
    recv = sf.Buffer(api, world * cap)
    recv.fill(sf.PATTERN)
    for r, R in enumerate(ranks):
        api.shard_dirty_pack(R.scene, r, recv.ptr + r * cap * BLOCK, cap)
    sf.sync(api)
    for r, R in enumerate(ranks):
        assert not np.array_equal(R.voxels(), twin.after_voxels), "before the exchange a rank holds only its own shard's updates"
        api.shard_dirty_unpack(R.scene, r, recv.ptr, cap)
        api.set_shard(R.scene, 0, 1, chunk)
        api.track_dirty(R.scene, False)
        scenarios.assert_same_full_state(R.state(), twin.after, f"rank {r} of {world} after the exchange")
    assert recv.guards_intact(sf.PATTERN)
