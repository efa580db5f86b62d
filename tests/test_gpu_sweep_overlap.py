"""The next frame's allocation sweep beside the previous GetImage's ray march: behind the overlapped k_mark the
sweep runs on the auxiliary stream too, puts its hash-table writes on a list, and k_publish_entries scatters them behind the
march; the ProcessFrame returns when the two kernels are launched, and its tail -- with a GetImage and a fence record behind
it -- is held by the engine until the caller's thread comes back (UpdateView, or any other call).  Every output must be
bit-identical to an engine opened with DSLAM_OVERLAP_SWEEP=0, the map must equal the CPU oracle's, and
dslam_debug_sweep_overlap_counts must say which passes took which way.

Shapes (sweep_overlap_fixtures.py): 160x120, 12 frames, a table so small that every pass after the first has excess
requests, and a second pool that runs dry in the middle of a pass (test_sweep_overlap_abi.py shows both on the oracle).
Frames go the pipelined way; a read-back waits for the stream and so costs the next pass its overlap, so "after every
frame" is checked by running every prefix of the sequence without a read-back inside it."""
import os

import numpy as np
import pytest

import sweep_overlap_fixtures as fx
import util

pytestmark = pytest.mark.gpu

M = fx.M


def _open(pkg, value):
    old = os.environ.get("DSLAM_OVERLAP_SWEEP")
    os.environ["DSLAM_OVERLAP_SWEEP"] = value   # (read when an engine is opened)
    try:
        return pkg.open_engine(0)
    finally:
        if old is None:
            del os.environ["DSLAM_OVERLAP_SWEEP"]
        else:
            os.environ["DSLAM_OVERLAP_SWEEP"] = old


@pytest.fixture(scope="module")
def on(pkg):
    return _open(pkg, "1")


@pytest.fixture(scope="module")
def off(pkg):
    return _open(pkg, "0")


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
        self.rgba = api.host_alloc((n, wl.H, wl.W, 4), np.uint8)
        self.mm = api.host_alloc((n, wl.H, wl.W), np.int16)
        self.out = api.host_alloc((n, self.fh, self.fw), np.float32)
        self.out[...] = np.nan
        for i, (rgba, mm, _) in enumerate(frames):
            self.rgba[i] = rgba
            self.mm[i] = mm

    def frame(self, i, image=True, pose_of=None, read_back=False, only_visible_at=(), after_process=None):
        api, Mi = self.api, self.frames[i][2]
        api.view_update(self.view, self.rgba[i], self.mm[i], timestamp=float(i))
        api.process_frame(self.scene, self.view, self.rs, Mi, self.wl.intr, only_update_visible_list=i in only_visible_at)
        if after_process is not None:
            after_process(i)
        if image:
            api.get_image(self.scene, self.free, self.frames[pose_of(i) if pose_of else i][2], self.free_intr, self.pkg.IMAGE_DEPTH,
                          out=np.empty((self.fh, self.fw), np.float32) if read_back else self.out[i])
            api.fence_record(self.fence)

    def counts(self):
        return self.api.debug_mark_overlap_counts() + self.api.debug_sweep_overlap_counts()

    def run(self, n, between=None, is_async=True, **kw):
        """n pipelined frames; between(i) is called between frame i - 1's GetImage and frame i's UpdateView.
        Returns (the n images, the map state, passes of the run: (k_mark overlapped, in stream, sweep overlapped, in stream))."""
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

    def close(self):
        for a in (self.rgba, self.mm, self.out):
            self.api.host_free(a)


def _same_images(a, b, what):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: depth images differ"


def _rig(api, pkg, synth, pool="roomy", **kw):
    wl, frames = fx.frames(synth)
    over = {k: kw.pop(k) for k in list(kw) if k in ("use_swapping",)}
    return Rig(api, pkg, wl, frames, fx.params(pkg, wl, pool, **over), **kw)


@pytest.mark.parametrize("pool", ["roomy", "dry"])
def test_on_off_and_oracle_agree_after_every_frame(pkg, synth, on, off, oracle, pool):
    img_ref, snaps_ref = fx.oracle_reference(oracle, pkg, synth, pool)
    for n in range(1, M + 1):
        a, b = _rig(on, pkg, synth, pool), _rig(off, pkg, synth, pool)
        img_on, snap_on, cnt_on = a.run(n)
        img_off, snap_off, cnt_off = b.run(n)
        assert cnt_on == (n - 1, 1, n - 1, 1) and cnt_off == (n - 1, 1, 0, n)
        _same_images(img_on, img_off, f"{pool}, {n} frames")
        util.assert_same_state(snap_on, snap_off, f"{pool}, {n} frames, sweep overlap on vs off")
        util.assert_same_state(snap_on, snaps_ref[n - 1], f"{pool}, {n} frames, sweep overlap on vs oracle")
        assert np.allclose(img_on, img_ref[:n], atol=1e-4), f"{pool}, {n} frames: depth differs from the oracle"
        a.close()
        b.close()
    assert (img_on[-1] > 0).sum() > 100


def test_counters_tell_the_paths_apart(pkg, synth, on):
    assert _rig(on, pkg, synth).run(M)[2] == (M - 1, 1, M - 1, 1)                    # a GetImage after every ProcessFrame
    assert _rig(on, pkg, synth).run(M, image=False)[2] == (0, M, 0, M)               # no GetImage between frames
    assert _rig(on, pkg, synth).run(M, is_async=False)[2] == (0, M, 0, M)            # a synchronous engine
    assert _rig(on, pkg, synth).run(M, read_back=True)[2] == (0, M, 0, M)            # every GetImage waits for its image
    assert _rig(on, pkg, synth, use_swapping=1).run(M)[2] == (0, M, 0, M)            # a scene with swapping


# What each call does to the engine (on a Rig) and to the oracle.  DeProcessFrame is an allocation pass itself: it directly
# follows the GetImage, so ITS k_mark and sweep are the ones that overlap, and the ProcessFrame behind it runs in the stream
# like every pass behind any other call.
def _decay(api, scene, rs, view, frames, wl, i):
    api.decay(scene, rs, 2, 3, True)


def _slide(api, scene, rs, view, frames, wl, i):
    api.slide_window(scene, rs, 2)


def _reset(api, scene, rs, view, frames, wl, i):
    api.reset_scene(scene)


def _deprocess(api, scene, rs, view, frames, wl, i):
    api.deprocess_frame(scene, view, rs, frames[i - 1][2], wl.intr)


@pytest.mark.parametrize("call,expect", [(_decay, (M - 2, 2, M - 2, 2)), (_slide, (M - 2, 2, M - 2, 2)), (_reset, (M - 2, 2, M - 2, 2)),
                                         (_deprocess, (M - 1, 2, M - 1, 2))],
                         ids=["decay", "slide_window", "reset_scene", "deprocess_frame"])
def test_a_call_in_between_costs_that_frame_its_overlap_only(pkg, synth, on, off, oracle, call, expect):
    wl, frames = fx.frames(synth)
    at = 4
    res = []
    for eng in (on, off):
        rig = _rig(eng, pkg, synth)
        res.append(rig.run(M, between=lambda i: call(eng, rig.scene, rig.rs, rig.view, frames, wl, i) if i == at else None))
    assert res[0][2] == expect
    assert res[1][2][2] == 0
    _same_images(res[0][0], res[1][0], call.__name__)
    util.assert_same_state(res[0][1], res[1][1], f"{call.__name__}, sweep overlap on vs off")
    _, snaps_ref = fx.oracle_run(oracle, pkg, wl, frames, M, fx.params(pkg, wl, "roomy"),
                                 between=lambda api, s, rs, v, i: call(api, s, rs, v, frames, wl, i) if i == at else None)
    util.assert_same_state(res[0][1], snaps_ref[-1], f"{call.__name__}, sweep overlap on vs oracle")


def test_a_list_only_pass_in_the_sequence(pkg, synth, on, off, oracle):
    """only_update_visible_list: no commits, nothing to publish; the pass and the ones around it keep their places."""
    wl, frames = fx.frames(synth)
    at = (3, 7)
    img_on, snap_on, cnt = _rig(on, pkg, synth).run(M, only_visible_at=at)
    img_off, snap_off, _ = _rig(off, pkg, synth).run(M, only_visible_at=at)
    assert cnt == (M - 1, 1, M - 1, 1)
    _same_images(img_on, img_off, "list-only passes")
    util.assert_same_state(snap_on, snap_off, "list-only passes, sweep overlap on vs off")
    _, snaps_ref = fx.oracle_run(oracle, pkg, wl, frames, M, fx.params(pkg, wl, "roomy"), only_visible_at=at)
    util.assert_same_state(snap_on, snaps_ref[-1], "list-only passes, sweep overlap on vs oracle")


@pytest.mark.parametrize("kind", ["other_pose", "other_size"])
def test_another_pose_or_size_still_overlaps(pkg, synth, on, off, kind):
    kw = dict(pose_of=lambda i: i + 1) if kind == "other_pose" else {}
    scale = 2 if kind == "other_size" else 1
    img_on, snap_on, cnt = _rig(on, pkg, synth, free_scale=scale).run(M, **kw)
    img_off, snap_off, _ = _rig(off, pkg, synth, free_scale=scale).run(M, **kw)
    assert cnt == (M - 1, 1, M - 1, 1)
    _same_images(img_on, img_off, kind)
    util.assert_same_state(snap_on, snap_off, f"{kind}, sweep overlap on vs off")


@pytest.mark.parametrize("what", ["stats", "hash_table", "counters"])
def test_a_call_behind_a_held_process_frame_sees_the_published_state(pkg, synth, on, off, oracle, what):
    """Between ProcessFrame and GetImage the tail of the ProcessFrame is still held by the engine; a call that looks at the
    map or at the engine's counters gets it run first."""
    _, snaps_ref = fx.oracle_reference(oracle, pkg, synth, "roomy")

    def run(eng):
        rig = _rig(eng, pkg, synth)
        seen = {}
        f0 = eng.debug_front_end_counts()
        c0 = eng.debug_sweep_overlap_counts()

        def look(i):
            if i < 2:
                return
            if what == "stats":
                st = eng.stats(rig.scene, rig.rs)
                seen[i] = {k: st[k] for k in ("last_free_block_id", "last_free_excess_id", "no_visible_entries", "frame_counter")}
            elif what == "hash_table":
                seen[i] = eng.download_hash_table(rig.scene)
            else:
                seen[i] = (sum(eng.debug_sweep_overlap_counts()) - sum(c0), eng.debug_front_end_counts()[0] - f0[0])

        _, snap, cnt = rig.run(6, after_process=look)
        return seen, snap, cnt

    seen, snap, cnt = run(on)
    util.assert_same_state(snap, snaps_ref[5], f"looking at {what} in between")
    # (the GetImage behind the look is enqueued on a stream the look left empty, and the next pass runs beside it as ever)
    assert cnt == (5, 1, 5, 1)
    seen_off = run(off)[0] if what == "counters" else None
    for i, got in seen.items():
        ref = snaps_ref[i]
        if what == "stats":
            assert got == {k: ref["stats"][k] for k in got}, f"frame {i}"
        elif what == "hash_table":
            assert np.array_equal(got, ref["hash"]), f"frame {i}"
        else:
            # frames 0 .. i have been processed: the held tail's fusion launch is counted like the engine that holds nothing counts it
            assert got[0] == i + 1 and got == seen_off[i], f"frame {i}"


@pytest.mark.parametrize("how", ["fence_wait", "fence_query"])
def test_a_fence_behind_held_calls_returns_with_the_complete_image(pkg, synth, on, off, how):
    ref, _, _ = _rig(off, pkg, synth).run(5)
    rig = _rig(on, pkg, synth)
    c0 = on.debug_sweep_overlap_counts()
    on.set_async(True)
    try:
        for i in range(5):
            rig.frame(i)            # frames 1 .. 4: tail, GetImage and fence record are all held when this returns
            if how == "fence_wait":
                on.fence_wait(rig.fence)
            else:
                while not on.fence_query(rig.fence):
                    pass
            assert np.array_equal(np.array(rig.out[i]).view(np.uint8), ref[i].view(np.uint8)), f"frame {i}: image not complete behind {how}"
        assert on.debug_sweep_overlap_counts()[0] - c0[0] == 4   # (a fence says nothing to the engine: the passes still overlap)
    finally:
        on.synchronize()
        on.set_async(False)


def test_frames_rewritten_right_after_update_view(pkg, synth, on, oracle):
    """After UpdateView returns the caller may rewrite its images -- also while the engine still holds the previous frame's calls."""
    wl, frames = fx.frames(synth)
    _, snaps_ref = fx.oracle_reference(oracle, pkg, synth, "roomy")
    rig = _rig(on, pkg, synth)
    rgba1 = on.host_alloc((wl.H, wl.W, 4), np.uint8)
    mm1 = on.host_alloc((wl.H, wl.W), np.int16)
    c0 = on.debug_sweep_overlap_counts()
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
    assert on.debug_sweep_overlap_counts()[0] - c0[0] == M - 1
    util.assert_same_state(util.snapshot(on, rig.scene, rig.rs), snaps_ref[-1], "frames rewritten after UpdateView")
    on.host_free(rgba1)
    on.host_free(mm1)


def test_two_async_engines_interleaved(pkg, synth, on, oracle):
    wl, frames = fx.frames(synth)
    second = _open(pkg, "1")
    prm = fx.params(pkg, wl, "roomy")
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
        assert tuple(b - a for a, b in zip(c0[k], r.counts())) == (M - 1, 1, M - 1, 1)
        img_ref, snaps_ref = fx.oracle_run(oracle, pkg, wl, r.frames, M, prm)
        util.assert_same_state(util.snapshot(r.api, r.scene, r.rs), snaps_ref[-1], f"engine {k} vs oracle")
        assert np.allclose(np.array(r.out[:M]), img_ref, atol=1e-4), f"engine {k}: depth differs from the oracle"


@pytest.mark.parametrize("bits,what", [(1, "order key"), (2, "tile count")])
def test_an_error_behind_a_held_process_frame_is_told_once(pkg, synth, on, bits, what):
    wl, frames = fx.frames(synth)
    rig = _rig(on, pkg, synth)
    c0 = on.debug_sweep_overlap_counts()
    on.set_async(True)
    try:
        rig.frame(0)
        rig.frame(1)
        on.view_update(rig.view, rig.rgba[2], rig.mm[2], timestamp=2.0)
        on.process_frame(rig.scene, rig.view, rig.rs, frames[2][2], wl.intr)     # overlapped: its tail is held
        on.debug_inject_device_error(rig.scene, bits)                            # runs the tail, enqueues, returns
        on.get_image(rig.scene, rig.free, frames[2][2], rig.free_intr, pkg.IMAGE_DEPTH, out=rig.out[2])
        rig.frame(3)                                                             # overlapped again, nothing waited yet
        assert on.debug_sweep_overlap_counts()[0] - c0[0] == 3
        with pytest.raises(pkg.DslamError, match=what):
            on.synchronize()
        on.synchronize()
        on.fence_wait(rig.fence)
    finally:
        on.set_async(False)
    on.reset_scene(rig.scene)   # (the scene's own sticky flags)
