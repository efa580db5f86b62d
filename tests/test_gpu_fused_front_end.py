"""GetImage's front end computed by ProcessFrame at its own pose (FrontEndRecord): the selection tiles ride at the front of
the fusion launch and a GetImage with the same scene version, pose, intrinsics and image size adopts their result.  Every
output must be bit-identical to the same calls on an engine opened with DSLAM_SPECULATIVE_FRONT_END=0 (which runs
FindVisibleBlocks inside GetImage, as before), and the visible lists and depths must match the CPU oracle."""
import os

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_off(pkg):
    old = os.environ.get("DSLAM_SPECULATIVE_FRONT_END")
    os.environ["DSLAM_SPECULATIVE_FRONT_END"] = "0"   # (read when an engine is opened)
    try:
        eng = pkg.open_engine(0)
    finally:
        if old is None:
            del os.environ["DSLAM_SPECULATIVE_FRONT_END"]
        else:
            os.environ["DSLAM_SPECULATIVE_FRONT_END"] = old
    return eng


def _render_outputs(api, pkg, scene, rs, M, intr):
    depth = api.get_image(scene, rs, M, intr, pkg.IMAGE_DEPTH)
    return [depth, api.download_raycast_result(rs), api.download_visible_ids(rs), api.download_range_image(rs),
            np.array([api.stats(scene, rs)["no_visible_entries"]])]


def _assert_bit_identical(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: output {k} shape/type"
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: output {k} differs"


def _sequence(api, pkg, wl, params, n, free_state=True, async_mode=True):
    """ProcessFrame + GetImage(depth) at the fusion pose every frame, into a free-view render state as the reference's GUI.
    async_mode None: an API without engine modes (the oracle)."""
    out = []
    if async_mode is not None:
        api.set_async(False)
    scene = api.create_scene(params)
    rs = api.create_render_state(scene, wl.W, wl.H)
    free = api.create_render_state(scene, wl.W, wl.H) if free_state else rs
    view = api.create_view(wl.W, wl.H)
    if async_mode is None:
        for i in range(n):
            rgba, mm, M = wl.frame(i)
            api.view_update(view, rgba, mm, timestamp=float(i))
            api.process_frame(scene, view, rs, M, wl.intr)
            out.append(_render_outputs(api, pkg, scene, free, M, wl.intr))
        return out, util.snapshot(api, scene, rs)
    api.set_async(async_mode)
    try:
        for i in range(n):
            rgba, mm, M = wl.frame(i)
            api.view_update(view, rgba, mm, timestamp=float(i))
            api.process_frame(scene, view, rs, M, wl.intr)
            out.append(_render_outputs(api, pkg, scene, free, M, wl.intr))
    finally:
        api.synchronize()
        api.set_async(False)
    return out, util.snapshot(api, scene, rs)


@pytest.mark.parametrize("which", ["tiny", "street"])
@pytest.mark.parametrize("free_state", [True, False])
def test_every_frame_matches_off_and_oracle(pkg, synth, gpu, gpu_off, oracle, which, free_state):
    wl = synth.s_tiny() if which == "tiny" else synth.s_street(320, 240)
    p = util.small_params(pkg, wl) if which == "tiny" else pkg.SceneParams(num_local_blocks=0x8000, **wl.scene_kwargs)
    n = 8
    c0, o0 = gpu.debug_front_end_counts(), gpu_off.debug_front_end_counts()
    on, snap_on = _sequence(gpu, pkg, wl, p, n, free_state)
    off, snap_off = _sequence(gpu_off, pkg, wl, p, n, free_state)
    c1, o1 = gpu.debug_front_end_counts(), gpu_off.debug_front_end_counts()
    # every ProcessFrame computed the front end and every GetImage took it; the engine with the switch off never did
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (n, n)
    assert o1 == o0
    for i in range(n):
        _assert_bit_identical(on[i], off[i], f"{which} frame {i}")
    util.assert_same_state(snap_on, snap_off, "speculation on vs off")
    ref, _ = _sequence(oracle, pkg, wl, p, n, free_state, async_mode=None)
    for i in range(n):
        assert np.array_equal(on[i][2], ref[i][2]), f"{which} frame {i}: visible list differs from the oracle"
        assert np.allclose(on[i][0], ref[i][0], atol=1e-4), f"{which} frame {i}: depth differs from the oracle"
    assert (on[-1][0] > 0).sum() > 100


def _mixed_calls(api, pkg, wl, synchronous):
    """ProcessFrame followed by GetImages the record must not serve, and calls in between that must invalidate it."""
    out = []
    api.set_async(False)
    p = util.small_params(pkg, wl)
    scene = api.create_scene(p)
    other = api.create_scene(p)
    rs = api.create_render_state(scene, wl.W, wl.H)
    rs_other = api.create_render_state(other, wl.W, wl.H)
    free = api.create_render_state(scene, wl.W, wl.H)
    half = api.create_render_state(scene, wl.W // 2, wl.H // 2)
    view = api.create_view(wl.W, wl.H)
    api.set_async(not synchronous)
    intr2 = [v * 1.01 for v in wl.intr]
    intr_half = [v * 0.5 for v in wl.intr]
    try:
        for i in range(10):
            rgba, mm, M = wl.frame(i)
            _, _, M_next = wl.frame(i + 1)
            api.view_update(view, rgba, mm, timestamp=float(i))
            api.process_frame(scene, view, rs, M, wl.intr)
            k = i % 5
            if k == 0:     # another pose, another intrinsics, another size: all fall back
                out.append(_render_outputs(api, pkg, scene, free, M_next, wl.intr))
                out.append(_render_outputs(api, pkg, scene, free, M, intr2))
                out.append(_render_outputs(api, pkg, scene, half, M, intr_half))
            elif k == 1:   # decay between ProcessFrame and GetImage
                api.decay(scene, rs, 2, 3, True)
            elif k == 2:   # a second scene on the same engine fuses in between
                api.process_frame(other, view, rs_other, M, wl.intr)
                out.append(_render_outputs(api, pkg, other, rs_other, M, wl.intr))
            elif k == 3:   # DeProcessFrame of the frame just fused
                api.deprocess_frame(scene, view, rs, M, wl.intr)
            out.append(_render_outputs(api, pkg, scene, free, M, wl.intr))
            out.append(_render_outputs(api, pkg, scene, free, M, wl.intr))   # (memo path where it applies)
            if i == 6:
                api.reset_scene(scene)
                out.append(_render_outputs(api, pkg, scene, free, M, wl.intr))
    finally:
        api.synchronize()
        api.set_async(False)
    return out, util.snapshot(api, scene, rs)


@pytest.mark.parametrize("synchronous", [False, True])
def test_fallbacks_and_invalidation(pkg, synth, gpu, gpu_off, synchronous):
    wl = synth.s_tiny()
    c0, o0 = gpu.debug_front_end_counts(), gpu_off.debug_front_end_counts()
    on, snap_on = _mixed_calls(gpu, pkg, wl, synchronous)
    off, snap_off = _mixed_calls(gpu_off, pkg, wl, synchronous)
    c1, o1 = gpu.debug_front_end_counts(), gpu_off.debug_front_end_counts()
    # 12 ProcessFrames (two of them on the second scene).  The record serves the first GetImage at the fusion pose of the
    # same scene and size: frames 0 and 5 behind three fall-backs, 4 and 9, 2 and 7 after the other scene has taken its
    # own; not after a decay (frames 1, 6) or a DeProcessFrame (3, 8), nor the second GetImage of a frame (the memo)
    assert c1[0] - c0[0] == 12
    assert c1[1] - c0[1] == 8
    assert o1 == o0
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        _assert_bit_identical(a, b, f"image {i}")
    util.assert_same_state(snap_on, snap_off, "speculation on vs off")


def test_swapping_scene(pkg, synth, gpu, gpu_off):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl, use_swapping=1)
    c0 = gpu.debug_front_end_counts()
    on, snap_on = _sequence(gpu, pkg, wl, p, 6)
    off, snap_off = _sequence(gpu_off, pkg, wl, p, 6)
    assert gpu.debug_front_end_counts() == c0   # (never computed for a swapping scene)
    for i in range(6):
        _assert_bit_identical(on[i], off[i], f"swapping frame {i}")
    util.assert_same_state(snap_on, snap_off, "speculation on vs off")


def test_two_engines_interleaved(pkg, synth, gpu, gpu_off):
    """Two engines with speculation on, calls interleaved without waits, against the same runs on one engine with it off."""
    wl = synth.s_street(320, 240)
    p = pkg.SceneParams(num_local_blocks=0x8000, **wl.scene_kwargs)
    second = pkg.open_engine(0)
    n = 12
    frames = [wl.frame(i) for i in range(n)]

    def order(k, i):
        return frames[i] if k == 0 else frames[n - 1 - i]

    objs = []
    for eng in (gpu, second):
        s = eng.create_scene(p)
        objs.append((eng, s, eng.create_render_state(s, wl.W, wl.H), eng.create_view(wl.W, wl.H), eng.create_render_state(s, wl.W, wl.H)))
    imgs = [[], []]
    try:
        for eng, *_ in objs:
            eng.set_async(True)
        for i in range(n):
            for k, (eng, s, rs, v, free) in enumerate(objs):
                rgba, mm, M = order(k, i)
                eng.view_update(v, rgba, mm, timestamp=float(i))
                eng.process_frame(s, v, rs, M, wl.intr)
                imgs[k].append(eng.get_image(s, free, M, wl.intr, pkg.IMAGE_DEPTH))
    finally:
        for eng, *_ in objs:
            eng.synchronize()
            eng.set_async(False)
    for k in range(2):
        s = gpu_off.create_scene(p)
        rs, v, free = gpu_off.create_render_state(s, wl.W, wl.H), gpu_off.create_view(wl.W, wl.H), gpu_off.create_render_state(s, wl.W, wl.H)
        for i in range(n):
            rgba, mm, M = order(k, i)
            gpu_off.view_update(v, rgba, mm, timestamp=float(i))
            gpu_off.process_frame(s, v, rs, M, wl.intr)
            ref = gpu_off.get_image(s, free, M, wl.intr, pkg.IMAGE_DEPTH)
            assert np.array_equal(imgs[k][i].view(np.uint8), ref.view(np.uint8)), f"engine {k} frame {i}"
    assert second.debug_front_end_counts() == (n, n)
