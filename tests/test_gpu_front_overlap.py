"""GetImage's front end beside the fusion launch: where a ProcessFrame's sweep runs on the auxiliary stream, the
selection over alloc_bits and the range pass for its pose follow the sweep there -- the selection sees the entries the sweep
created, whose table stores still wait for k_publish_entries, through the engine's array of their positions -- the fusion
launch is the plain one, and a GetImage at that pose adopts a record whose range image is already filled and runs the march
alone.  Every output must be bit-identical to an engine opened with DSLAM_OVERLAP_FRONT=0, the map, the free-view visible
list, its count and the corner of the range image must equal the CPU oracle's, and dslam_debug_front_overlap_counts must say
which front ends took which way.

Shapes (front_overlap_fixtures.py): 160x120, 12 frames, a table on which the passes that overlap create bucket entries and
excess entries that the GetImage lists, and a second pool that runs dry in the middle of a pass
(test_front_overlap_abi.py shows both on the oracle).  Frames go the pipelined way; "after every frame" is checked by
running every prefix of the sequence, as a read-back inside it would cost the next pass its overlap."""
import os

import numpy as np
import pytest

import front_overlap_fixtures as ffx
import sweep_overlap_fixtures as fx
import util

pytestmark = pytest.mark.gpu

M = ffx.M


def _open(pkg, value):
    old = os.environ.get("DSLAM_OVERLAP_FRONT")
    os.environ["DSLAM_OVERLAP_FRONT"] = value   # (read when an engine is opened)
    try:
        return pkg.open_engine(0)
    finally:
        if old is None:
            del os.environ["DSLAM_OVERLAP_FRONT"]
        else:
            os.environ["DSLAM_OVERLAP_FRONT"] = old


@pytest.fixture(scope="module")
def on(pkg):
    return _open(pkg, "1")


@pytest.fixture(scope="module")
def off(pkg):
    return _open(pkg, "0")


class _Ring:
    """Page-locked arrays carved out of one block, round and round.  A rig takes 1.6 MB and at most a handful are alive at a
    time, each done with (its engine synchronised) long before the ring comes round to it again.  One allocation of its own,
    given back when the module is done, so that these tests leave the library's small-buffer arenas as they found them."""
    BYTES = 32 << 20

    def __init__(self, api):
        self.api, self.block, self.at = api, api.host_alloc((self.BYTES,), np.uint8), 0

    def take(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.at + n > self.BYTES:
            self.at = 0
        a = self.block[self.at:self.at + n].view(dtype).reshape(shape)
        self.at += (n + 255) & ~255
        return a


_ring = None


@pytest.fixture(scope="module", autouse=True)
def _pinned(on):
    global _ring
    _ring = _Ring(on)
    yield
    on.set_async(False)
    on.host_free(_ring.block)
    _ring = None


class Rig:
    """One scene with its fusion and free-view render states, view, page-locked frames and outputs on a HIP engine."""

    def __init__(self, api, pkg, wl, frames, params, free_scale=1):
        api.set_async(False)
        self.api, self.pkg, self.wl, self.frames = api, pkg, wl, frames
        self.fw, self.fh = wl.W // free_scale, wl.H // free_scale
        self.free_intr = [v / free_scale for v in wl.intr]
        self.scene = api.create_scene(params)
        self.rs = api.create_render_state(self.scene, wl.W, wl.H)
        self.free = api.create_render_state(self.scene, self.fw, self.fh)
        self.view = api.create_view(wl.W, wl.H)
        self.fence = api.fence_create()
        n = len(frames)
        self.rgba = _ring.take((n, wl.H, wl.W, 4), np.uint8)
        self.mm = _ring.take((n, wl.H, wl.W), np.int16)
        self.out = _ring.take((n, self.fh, self.fw), np.float32)
        self.out[...] = np.nan
        for i, (rgba, mm, _) in enumerate(frames):
            self.rgba[i] = rgba
            self.mm[i] = mm

    def frame(self, i, image=True, pose_of=None, read_back=False):
        api, Mi = self.api, self.frames[i][2]
        api.view_update(self.view, self.rgba[i], self.mm[i], timestamp=float(i))
        api.process_frame(self.scene, self.view, self.rs, Mi, self.wl.intr)
        if image if isinstance(image, bool) else image(i):
            api.get_image(self.scene, self.free, self.frames[pose_of(i) if pose_of else i][2], self.free_intr, self.pkg.IMAGE_DEPTH,
                          out=np.empty((self.fh, self.fw), np.float32) if read_back else self.out[i])
            api.fence_record(self.fence)

    def counts(self):
        """(front ends on the auxiliary stream, in the fusion launch, adopted by a GetImage)"""
        return self.api.debug_front_overlap_counts() + (self.api.debug_front_end_counts()[1],)

    def run(self, n, between=None, is_async=True, **kw):
        """n pipelined frames; between(i) is called between frame i - 1's GetImage and frame i's UpdateView.
        Returns (the n images, the map state, the counts of the run)."""
        api = self.api
        c0 = self.counts()
        api.set_async(is_async)
        try:
            for i in range(n):
                if between is not None and i > 0:
                    between(i)
                self.frame(i, **kw)
            api.synchronize()
        finally:
            api.set_async(False)
        c1 = self.counts()
        return np.array(self.out[:n]), util.snapshot(api, self.scene, self.rs), tuple(b - a for a, b in zip(c0, c1))

    def front_end(self):
        """What GetImage's front end left in the free-view render state: (visible list, its count, range-image corner)."""
        api = self.api
        return (api.download_visible_ids(self.free), api.stats(self.scene, self.free)["no_visible_entries"],
                ffx.corner(api, self.free, self.fw, self.fh))


def _same_images(a, b, what):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: depth images differ"


def _rig(api, pkg, synth, pool="roomy", **kw):
    wl, frames = fx.frames(synth)
    over = {k: kw.pop(k) for k in list(kw) if k in ("use_swapping",)}
    return Rig(api, pkg, wl, frames, ffx.params(pkg, wl, pool, **over), **kw)


@pytest.mark.parametrize("pool", ["roomy", "dry"])
def test_on_off_and_oracle_agree_after_every_frame(pkg, synth, on, off, oracle, pool):
    ref = ffx.oracle_reference(oracle, pkg, synth, pool)
    img_ref = np.array([r["image"] for r in ref])
    for n in range(1, M + 1):
        a, b = _rig(on, pkg, synth, pool), _rig(off, pkg, synth, pool)
        img_on, snap_on, cnt_on = a.run(n)
        img_off, snap_off, cnt_off = b.run(n)
        assert cnt_on == (n - 1, 1, n) and cnt_off == (0, n, n)
        what = f"{pool}, {n} frames"
        _same_images(img_on, img_off, what)
        util.assert_same_state(snap_on, snap_off, f"{what}, front overlap on vs off")
        util.assert_same_state(snap_on, ref[n - 1]["snap"], f"{what}, front overlap on vs oracle")
        for name, rig in (("on", a), ("off", b)):
            vis, count, corner = rig.front_end()
            assert np.array_equal(vis, ref[n - 1]["visible"]), f"{what}, {name}: free-view visible list differs from the oracle"
            assert count == ref[n - 1]["count"], f"{what}, {name}: visible count"
            assert np.array_equal(corner.view(np.uint32), ref[n - 1]["corner"].view(np.uint32)), f"{what}, {name}: range-image corner"
        assert np.allclose(img_on, img_ref[:n], atol=1e-4), f"{what}: depth differs from the oracle"
    assert (img_on[-1] > 0).sum() > 100


def test_counters_tell_the_paths_apart(pkg, synth, on):
    assert _rig(on, pkg, synth).run(M)[2] == (M - 1, 1, M)                          # a GetImage after every ProcessFrame
    assert _rig(on, pkg, synth).run(M, image=False)[2] == (0, M, 0)                 # no GetImage between frames
    assert _rig(on, pkg, synth).run(M, is_async=False)[2] == (0, M, M)              # a synchronous engine
    assert _rig(on, pkg, synth).run(M, read_back=True)[2] == (0, M, M)              # every GetImage waits for its image
    assert _rig(on, pkg, synth, use_swapping=1).run(M)[2] == (0, 0, 0)              # a scene with swapping: no front end at all


def _decay(api, scene, rs, view, frames, wl, i):
    api.decay(scene, rs, 2, 3, True)


def _slide(api, scene, rs, view, frames, wl, i):
    api.slide_window(scene, rs, 2)


def _reset(api, scene, rs, view, frames, wl, i):
    api.reset_scene(scene)


def _deprocess(api, scene, rs, view, frames, wl, i):
    api.deprocess_frame(scene, view, rs, frames[i - 1][2], wl.intr)


@pytest.mark.parametrize("call", [_decay, _slide, _reset, _deprocess], ids=["decay", "slide_window", "reset_scene", "deprocess_frame"])
def test_a_call_in_between_costs_that_frame_its_overlap_only(pkg, synth, on, off, oracle, call):
    """The ProcessFrame behind the call runs in the stream and computes its front end in the fusion launch; every other frame
    keeps its way.  (DeProcessFrame's own allocation pass takes the overlap; it computes no front end.)"""
    wl, frames = fx.frames(synth)
    at = 4
    res = []
    for eng in (on, off):
        rig = _rig(eng, pkg, synth)
        res.append(rig.run(M, between=lambda i: call(eng, rig.scene, rig.rs, rig.view, frames, wl, i) if i == at else None))
    assert res[0][2] == (M - 2, 2, M)
    assert res[1][2] == (0, M, M)
    _same_images(res[0][0], res[1][0], call.__name__)
    util.assert_same_state(res[0][1], res[1][1], f"{call.__name__}, front overlap on vs off")
    _, snaps_ref = fx.oracle_run(oracle, pkg, wl, frames, M, ffx.params(pkg, wl, "roomy"),
                                 between=lambda api, s, rs, v, i: call(api, s, rs, v, frames, wl, i) if i == at else None)
    util.assert_same_state(res[0][1], snaps_ref[-1], f"{call.__name__}, front overlap on vs oracle")


@pytest.mark.parametrize("kind", ["other_pose", "other_size"])
def test_another_pose_or_size_gets_a_correct_image_and_the_next_frame_overlaps(pkg, synth, on, off, kind):
    """Nobody adopts the record: the GetImage sits out the auxiliary stream, computes its own front end, and grants the next
    pass its overlap all the same."""
    kw = dict(pose_of=lambda i: i + 1) if kind == "other_pose" else {}
    scale = 2 if kind == "other_size" else 1
    img_on, snap_on, cnt = _rig(on, pkg, synth, free_scale=scale).run(M, **kw)
    img_off, snap_off, cnt_off = _rig(off, pkg, synth, free_scale=scale).run(M, **kw)
    assert cnt == (M - 1, 1, 0) and cnt_off == (0, M, 0)
    _same_images(img_on, img_off, kind)
    util.assert_same_state(snap_on, snap_off, f"{kind}, front overlap on vs off")
    assert (img_on[-1] > 0).sum() > 100


def test_a_process_frame_without_a_get_image_then_one_with(pkg, synth, on, off):
    """Frames 3 and 7 have no GetImage behind them: their records are waited for and dropped, the passes behind them run in
    the stream, and everything else is as ever."""
    image = lambda i: i not in (3, 7)
    a, b = _rig(on, pkg, synth), _rig(off, pkg, synth)
    img_on, snap_on, cnt = a.run(M, image=image)
    img_off, snap_off, cnt_off = b.run(M, image=image)
    assert cnt == (M - 3, 3, M - 2) and cnt_off == (0, M, M - 2)
    keep = [i for i in range(M) if image(i)]
    _same_images(img_on[keep], img_off[keep], "frames with a GetImage")
    util.assert_same_state(snap_on, snap_off, "a ProcessFrame without a GetImage, front overlap on vs off")
    for x, y in zip(a.front_end(), b.front_end()):
        assert np.array_equal(x, y)


def test_a_fence_waited_for_directly_returns_with_the_complete_image(pkg, synth, on, off):
    ref, _, _ = _rig(off, pkg, synth).run(5)
    rig = _rig(on, pkg, synth)
    c0 = rig.counts()
    on.set_async(True)
    try:
        for i in range(5):
            rig.frame(i)            # frames 1 .. 4: tail, GetImage and fence record are all held when this returns
            on.fence_wait(rig.fence)
            assert np.array_equal(np.array(rig.out[i]).view(np.uint8), ref[i].view(np.uint8)), f"frame {i}: image not complete behind the fence"
        assert tuple(b - a for a, b in zip(c0, rig.counts())) == (4, 1, 5)   # (a fence says nothing to the engine: the passes still overlap)
    finally:
        on.synchronize()
        on.set_async(False)


def test_frames_rewritten_right_after_update_view(pkg, synth, on, oracle):
    """After UpdateView returns the caller may rewrite its images -- also though the copy was enqueued between the held calls."""
    wl, frames = fx.frames(synth)
    ref = ffx.oracle_reference(oracle, pkg, synth, "roomy")
    rig = _rig(on, pkg, synth)
    rgba1 = _ring.take((wl.H, wl.W, 4), np.uint8)
    mm1 = _ring.take((wl.H, wl.W), np.int16)
    c0 = rig.counts()
    on.set_async(True)
    try:
        for i in range(M):
            rgba1[...] = frames[i][0]
            mm1[...] = frames[i][1]
            on.view_update(rig.view, rgba1, mm1, timestamp=float(i))
            rgba1[...] = 0x5a
            mm1[...] = 1234
            on.process_frame(rig.scene, rig.view, rig.rs, frames[i][2], wl.intr)
            on.get_image(rig.scene, rig.free, frames[i][2], rig.free_intr, pkg.IMAGE_DEPTH, out=rig.out[i])
            on.fence_record(rig.fence)
        on.synchronize()
    finally:
        on.set_async(False)
    assert tuple(b - a for a, b in zip(c0, rig.counts())) == (M - 1, 1, M)
    util.assert_same_state(util.snapshot(on, rig.scene, rig.rs), ref[-1]["snap"], "frames rewritten after UpdateView")


def test_two_async_engines_interleaved(pkg, synth, on, oracle):
    wl, frames = fx.frames(synth)
    second = _open(pkg, "1")
    prm = ffx.params(pkg, wl, "roomy")
    orders = [list(range(M)), list(range(M - 1, -1, -1))]
    rigs = [Rig(on, pkg, wl, [frames[i] for i in orders[0]], prm), Rig(second, pkg, wl, [frames[i] for i in orders[1]], prm)]
    c0 = [r.counts() for r in rigs]
    try:
        for r in rigs:
            r.api.set_async(True)
        for i in range(M):
            for r in rigs:
                r.frame(i)
    finally:
        for r in rigs:
            r.api.synchronize()
            r.api.set_async(False)
    for k, r in enumerate(rigs):
        assert tuple(b - a for a, b in zip(c0[k], r.counts())) == (M - 1, 1, M)
        img_ref, snaps_ref = fx.oracle_run(oracle, pkg, wl, r.frames, M, prm)
        util.assert_same_state(util.snapshot(r.api, r.scene, r.rs), snaps_ref[-1], f"engine {k} vs oracle")
        assert np.allclose(np.array(r.out[:M]), img_ref, atol=1e-4), f"engine {k}: depth differs from the oracle"


@pytest.mark.parametrize("bits,what", [(1, "order key"), (2, "tile count")])
def test_an_injected_error_is_told_once(pkg, synth, on, bits, what):
    wl, frames = fx.frames(synth)
    rig = _rig(on, pkg, synth)
    c0 = rig.counts()
    on.set_async(True)
    try:
        rig.frame(0)
        rig.frame(1)
        on.view_update(rig.view, rig.rgba[2], rig.mm[2], timestamp=2.0)
        on.process_frame(rig.scene, rig.view, rig.rs, frames[2][2], wl.intr)     # overlapped: its tail is held
        on.debug_inject_device_error(rig.scene, bits)                            # runs the tail, waits for its front end, enqueues
        on.get_image(rig.scene, rig.free, frames[2][2], rig.free_intr, pkg.IMAGE_DEPTH, out=rig.out[2])
        rig.frame(3)                                                             # overlapped again, nothing waited yet
        assert tuple(b - a for a, b in zip(c0, rig.counts()))[:2] == (3, 1)
        with pytest.raises(pkg.DslamError, match=what):
            on.synchronize()
        on.synchronize()
        on.fence_wait(rig.fence)
    finally:
        on.set_async(False)
    on.reset_scene(rig.scene)   # (the scene's own sticky flags)
