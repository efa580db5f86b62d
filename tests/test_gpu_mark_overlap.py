"""The next frame's k_mark beside the previous GetImage's ray march: on an asynchronous engine an allocation pass
that directly follows a GetImage runs its marking kernel on the engine's auxiliary stream, ordered by the host.  It is the
same kernel on the same inputs, so every output must be bit-identical to an engine opened with DSLAM_OVERLAP_MARK=0, the
map must equal the CPU oracle's, and dslam_debug_mark_overlap_counts must say which passes took which way.

Frames go the pipelined way: page-locked input, view_update -> process_frame -> get_image(out=page-locked) -> fence_record.
A read-back waits for the stream and so withdraws the permission to overlap; "after every frame" is therefore checked by
running every prefix of the sequence without a read-back inside it."""
import os

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

N = 7   # frames of a sequence


def _open(pkg, value):
    old = os.environ.get("DSLAM_OVERLAP_MARK")
    os.environ["DSLAM_OVERLAP_MARK"] = value   # (read when an engine is opened)
    try:
        return pkg.open_engine(0)
    finally:
        if old is None:
            del os.environ["DSLAM_OVERLAP_MARK"]
        else:
            os.environ["DSLAM_OVERLAP_MARK"] = old


@pytest.fixture(scope="module")
def on(pkg):
    return _open(pkg, "1")


@pytest.fixture(scope="module")
def off(pkg):
    return _open(pkg, "0")


_FRAMES = {}


def _frames(synth, size):
    """(workload, [(rgba, mm, M)] for N + 1 frames) of s_tiny at `size`, rendered once per module."""
    if size not in _FRAMES:
        wl = synth.s_tiny(*size)
        _FRAMES[size] = (wl, [wl.frame(i) for i in range(N + 1)])
    return _FRAMES[size]


class Rig:
    """One scene with its fusion and free-view render states, view, page-locked frames and outputs on a HIP engine."""

    def __init__(self, api, pkg, wl, frames, params=None, free_scale=1):
        api.set_async(False)
        self.api, self.pkg, self.wl, self.frames = api, pkg, wl, frames
        self.fw, self.fh = wl.W // free_scale, wl.H // free_scale
        self.free_intr = [v / free_scale for v in wl.intr]
        self.scene = api.create_scene(params or util.small_params(pkg, wl))
        self.rs = api.create_render_state(self.scene, wl.W, wl.H)
        self.free = api.create_render_state(self.scene, self.fw, self.fh)
        self.view = api.create_view(wl.W, wl.H)
        self.fence = api.fence_create()
        n = len(frames)
        self.rgba = api.host_alloc((n, wl.H, wl.W, 4), np.uint8)
        self.mm = api.host_alloc((n, wl.H, wl.W), np.int16)
        self.out = api.host_alloc((n, self.fh, self.fw), np.float32)
        for i, (rgba, mm, _) in enumerate(frames):
            self.rgba[i] = rgba
            self.mm[i] = mm

    def frame(self, i, image=True, pose_of=None, read_back=False):
        api, M = self.api, self.frames[i][2]
        api.view_update(self.view, self.rgba[i], self.mm[i], timestamp=float(i))
        api.process_frame(self.scene, self.view, self.rs, M, self.wl.intr)
        if image:
            api.get_image(self.scene, self.free, self.frames[pose_of(i) if pose_of else i][2], self.free_intr, self.pkg.IMAGE_DEPTH,
                          out=np.empty((self.fh, self.fw), np.float32) if read_back else self.out[i])
            api.fence_record(self.fence)

    def run(self, n, between=None, is_async=True, **kw):
        """n pipelined frames; between(i) is called between frame i - 1's GetImage and frame i's ProcessFrame.
        Returns (the n images, the map state, (overlapped, in-stream) passes of the run)."""
        api = self.api
        c0 = api.debug_mark_overlap_counts()
        api.set_async(is_async)
        try:
            for i in range(n):
                if between is not None and i > 0:
                    between(i)
                self.frame(i, **kw)
            api.synchronize()
        finally:
            api.set_async(False)
        c1 = api.debug_mark_overlap_counts()
        return np.array(self.out[:n]), util.snapshot(api, self.scene, self.rs), (c1[0] - c0[0], c1[1] - c0[1])

    def close(self):
        for a in (self.rgba, self.mm, self.out):
            self.api.host_free(a)


def _oracle_run(oracle, pkg, wl, frames, n, params=None, free_scale=1, pose_of=None, between=None):
    scene = oracle.create_scene(params or util.small_params(pkg, wl))
    rs = oracle.create_render_state(scene, wl.W, wl.H)
    free = oracle.create_render_state(scene, wl.W // free_scale, wl.H // free_scale)
    view = oracle.create_view(wl.W, wl.H)
    free_intr = [v / free_scale for v in wl.intr]
    imgs = []
    for i in range(n):
        if between is not None and i > 0:
            between(oracle, scene, rs, view, i)
        rgba, mm, M = frames[i]
        oracle.view_update(view, rgba, mm, timestamp=float(i))
        oracle.process_frame(scene, view, rs, M, wl.intr)
        imgs.append(oracle.get_image(scene, free, frames[pose_of(i) if pose_of else i][2], free_intr, pkg.IMAGE_DEPTH))
    return np.array(imgs), util.snapshot(oracle, scene, rs)


def _same_images(a, b, what):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: depth images differ"


@pytest.mark.parametrize("size", [(70, 45), (64, 48)])
def test_on_off_and_oracle_agree_after_every_frame(pkg, synth, on, off, oracle, size):
    wl, frames = _frames(synth, size)
    for n in range(1, N + 1):
        a, b = Rig(on, pkg, wl, frames), Rig(off, pkg, wl, frames)
        img_on, snap_on, cnt_on = a.run(n)
        img_off, snap_off, cnt_off = b.run(n)
        assert cnt_on == (n - 1, 1) and cnt_off == (0, n)
        _same_images(img_on, img_off, f"{n} frames")
        util.assert_same_state(snap_on, snap_off, f"{n} frames, overlap on vs off")
        img_ref, snap_ref = _oracle_run(oracle, pkg, wl, frames, n)
        util.assert_same_state(snap_on, snap_ref, f"{n} frames, overlap on vs oracle")
        assert np.allclose(img_on, img_ref, atol=1e-4), f"{n} frames: depth differs from the oracle"
        a.close()
        b.close()
    assert (img_on[-1] > 0).sum() > 100


def test_counters_tell_the_paths_apart(pkg, synth, on):
    wl, frames = _frames(synth, (70, 45))
    assert Rig(on, pkg, wl, frames).run(N)[2] == (N - 1, 1)                   # a GetImage after every ProcessFrame
    assert Rig(on, pkg, wl, frames).run(N, image=False)[2] == (0, N)          # no GetImage between frames
    assert Rig(on, pkg, wl, frames).run(N, is_async=False)[2] == (0, N)       # a synchronous engine
    assert Rig(on, pkg, wl, frames).run(N, read_back=True)[2] == (0, N)       # every GetImage waits for its image: nothing to run beside
    swapping = util.small_params(pkg, wl, use_swapping=1)
    assert Rig(on, pkg, wl, frames, params=swapping).run(N)[2] == (0, N)      # a scene with swapping


# What each call does to the engine (on a Rig) and to the oracle, and how many allocation passes of its own it adds in
# the stream.  DeProcessFrame is an allocation pass itself: it directly follows the GetImage, so ITS k_mark is the one
# that overlaps, and the ProcessFrame behind it runs in the stream like every pass behind any other call.
def _decay(api, scene, rs, view, rig_frames, wl, i):
    api.decay(scene, rs, 2, 3, True)


def _slide(api, scene, rs, view, rig_frames, wl, i):
    api.slide_window(scene, rs, 2)


def _reset(api, scene, rs, view, rig_frames, wl, i):
    api.reset_scene(scene)


def _deprocess(api, scene, rs, view, rig_frames, wl, i):
    api.deprocess_frame(scene, view, rs, rig_frames[i - 1][2], wl.intr)


def _find_visible(api, scene, rs, view, rig_frames, wl, i):
    api.find_visible_blocks(scene, rs, rig_frames[i][2], wl.intr)


@pytest.mark.parametrize("call,expect", [(_decay, (N - 2, 2)), (_slide, (N - 2, 2)), (_reset, (N - 2, 2)),
                                         (_deprocess, (N - 1, 2)), (_find_visible, (N - 2, 2))],
                         ids=["decay", "slide_window", "reset_scene", "deprocess_frame", "find_visible_blocks"])
def test_a_call_in_between_falls_back_for_that_frame_only(pkg, synth, on, off, oracle, call, expect):
    wl, frames = _frames(synth, (70, 45))
    at = 3
    res = []
    for eng in (on, off):
        rig = Rig(eng, pkg, wl, frames)
        res.append(rig.run(N, between=lambda i: call(eng, rig.scene, rig.rs, rig.view, frames, wl, i) if i == at else None))
    assert res[0][2] == expect
    assert res[1][2][0] == 0
    _same_images(res[0][0], res[1][0], call.__name__)
    util.assert_same_state(res[0][1], res[1][1], f"{call.__name__}, overlap on vs off")
    _, snap_ref = _oracle_run(oracle, pkg, wl, frames, N,
                              between=lambda api, s, rs, v, i: call(api, s, rs, v, frames, wl, i) if i == at else None)
    util.assert_same_state(res[0][1], snap_ref, f"{call.__name__}, overlap on vs oracle")


@pytest.mark.parametrize("kind", ["other_pose", "other_size"])
def test_the_stamp_does_not_depend_on_the_view(pkg, synth, on, off, oracle, kind):
    wl, frames = _frames(synth, (64, 48))
    kw = dict(pose_of=lambda i: i + 1) if kind == "other_pose" else {}
    scale = 2 if kind == "other_size" else 1
    img_on, snap_on, cnt = Rig(on, pkg, wl, frames, free_scale=scale).run(N, **kw)
    img_off, snap_off, _ = Rig(off, pkg, wl, frames, free_scale=scale).run(N, **kw)
    assert cnt == (N - 1, 1)
    _same_images(img_on, img_off, kind)
    util.assert_same_state(snap_on, snap_off, f"{kind}, overlap on vs off")
    img_ref, snap_ref = _oracle_run(oracle, pkg, wl, frames, N, free_scale=scale, **kw)
    util.assert_same_state(snap_on, snap_ref, f"{kind}, overlap on vs oracle")
    assert np.allclose(img_on, img_ref, atol=1e-4), f"{kind}: depth differs from the oracle"


# A wait changes no result.  Which way the pass goes: a fence wait says nothing to the engine, so the pass still overlaps (the
# stamp is there at once); dslam_engine_synchronize leaves the stream empty -- nothing to run beside -- and withdraws the
# permission, as every call that waits for the stream does (the reference's unchanged caller reads an image back every
# keyframe and would pay the auxiliary stream's launch and wait for nothing).
@pytest.mark.parametrize("wait,expect", [("fence_wait", (N - 1, 1)), ("synchronize", (0, N))])
def test_a_wait_in_between_changes_nothing(pkg, synth, on, off, wait, expect):
    wl, frames = _frames(synth, (70, 45))
    rig = Rig(on, pkg, wl, frames)
    img_on, snap_on, cnt = rig.run(N, between=lambda i: on.fence_wait(rig.fence) if wait == "fence_wait" else on.synchronize())
    img_off, snap_off, _ = Rig(off, pkg, wl, frames).run(N)
    assert cnt == expect
    _same_images(img_on, img_off, wait)
    util.assert_same_state(snap_on, snap_off, f"{wait}, overlap on vs off")


def test_two_async_engines_interleaved(pkg, synth, on, oracle):
    wl, frames = _frames(synth, (70, 45))
    second = _open(pkg, "1")
    orders = [list(range(N)), list(range(N - 1, -1, -1))]
    rigs = [Rig(on, pkg, wl, [frames[i] for i in orders[0]]), Rig(second, pkg, wl, [frames[i] for i in orders[1]])]
    c0 = [r.api.debug_mark_overlap_counts() for r in rigs]
    try:
        for r in rigs:
            r.api.set_async(True)
        for i in range(N):
            for r in rigs:
                r.frame(i)
    finally:
        for r in rigs:
            r.api.synchronize()
            r.api.set_async(False)
    for k, r in enumerate(rigs):
        c1 = r.api.debug_mark_overlap_counts()
        assert (c1[0] - c0[k][0], c1[1] - c0[k][1]) == (N - 1, 1)
        img_ref, snap_ref = _oracle_run(oracle, pkg, wl, r.frames, N)
        util.assert_same_state(util.snapshot(r.api, r.scene, r.rs), snap_ref, f"engine {k} vs oracle")
        assert np.allclose(np.array(r.out[:N]), img_ref, atol=1e-4), f"engine {k}: depth differs from the oracle"


@pytest.mark.parametrize("bits,what", [(1, "order key"), (2, "tile count")])
def test_an_error_in_an_overlapped_frame_is_told_once(pkg, synth, on, bits, what):
    """Bit 1 is the one k_mark itself reports, through its own page-locked word; bit 2 travels in the shared word."""
    wl, frames = _frames(synth, (70, 45))
    rig = Rig(on, pkg, wl, frames)
    c0 = on.debug_mark_overlap_counts()
    on.set_async(True)
    try:
        rig.frame(0)
        rig.frame(1)
        on.view_update(rig.view, rig.rgba[2], rig.mm[2], timestamp=2.0)
        on.process_frame(rig.scene, rig.view, rig.rs, frames[2][2], wl.intr)     # overlapped
        on.debug_inject_device_error(rig.scene, bits)                            # enqueued, returns
        on.get_image(rig.scene, rig.free, frames[2][2], rig.free_intr, pkg.IMAGE_DEPTH, out=rig.out[2])
        rig.frame(3)                                                             # overlapped again, nothing waited yet
        assert on.debug_mark_overlap_counts()[0] - c0[0] == 3
        with pytest.raises(pkg.DslamError, match=what):
            on.synchronize()
        on.synchronize()
        on.fence_wait(rig.fence)
    finally:
        on.set_async(False)
    on.reset_scene(rig.scene)   # (the scene's own sticky flags)
