"""Parity of voxel decay, sliding window and swapping (HIP engine vs CPU oracle), bit-exact after every frame.
Replays DenseSlam::ProcessFrame steps 10-13 (reference DenseSlam.cpp:210-232) with the param.yaml knobs
voxel_decay / min_decay_age / max_decay_weight / slide_window / max_age (SystemEntry.cpp:138-149)."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


def _run_pair(gpu, oracle, pkg, wl, params, n_frames, decay=None, slide=None, swap_flush_at=None, extra=None):
    objs = {}
    for name, api in (("gpu", gpu), ("oracle", oracle)):
        s = api.create_scene(params)
        objs[name] = (api, s, api.create_render_state(s, wl.W, wl.H), api.create_view(wl.W, wl.H))
    last = None
    for i in range(n_frames):
        rgba, mm, M = wl.frame(i)
        snaps = {}
        for name, (api, s, rs, v) in objs.items():
            api.view_update(v, rgba, mm, timestamp=float(i))
            api.process_frame(s, v, rs, M, wl.intr)
            if slide is not None and api.stats(s, rs)["fusion_fifo_len"] > slide:
                api.slide_window(s, rs, slide)
            if decay is not None:
                api.decay(s, rs, decay[0], decay[1], decay[2])
            if swap_flush_at is not None and i == swap_flush_at:
                api.save_to_global_memory(s)
            if extra is not None:
                extra(i, api, s, rs, v)
            snaps[name] = util.snapshot(api, s, rs)
            snaps[name]["last_seen"] = api.download_last_seen(s)
            if params.use_swapping:
                snaps[name]["swap"] = api.download_swap_states(s)
        util.assert_same_state(snaps["gpu"], snaps["oracle"], f"frame {i}")
        assert np.array_equal(snaps["gpu"]["last_seen"], snaps["oracle"]["last_seen"]), f"frame {i}: last_seen"
        if params.use_swapping:
            assert np.array_equal(snaps["gpu"]["swap"], snaps["oracle"]["swap"]), f"frame {i}: swap states"
            st0, st1 = snaps["gpu"]["stats"], snaps["oracle"]["stats"]
            assert (st0["last_swapped_in"], st0["last_swapped_out"]) == (st1["last_swapped_in"], st1["last_swapped_out"])
        last = snaps
    util.check_invariants(last["gpu"], objs["gpu"][1].params)
    # raycast the maintained maps too: released / relinked chains must still resolve
    rgba, mm, M = wl.frame(n_frames - 1)
    imgs = {}
    for name, (api, s, rs, v) in objs.items():
        rs_free = api.create_render_state(s, wl.W, wl.H)
        imgs[name] = api.get_image(s, rs_free, M, wl.intr, pkg.IMAGE_DEPTH)
    assert np.array_equal(imgs["gpu"] > 0, imgs["oracle"] > 0), "raycast hit mask differs after maintenance"
    assert np.abs(imgs["gpu"] - imgs["oracle"]).max() <= 1e-4
    return objs, last


@pytest.mark.parametrize("mode", ["aged_list", "full_sweep"])
def test_decay(pkg, synth, gpu, oracle, mode):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl)
    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 10, decay=(2, 2, mode == "full_sweep"))
    assert last["gpu"]["stats"]["decayed_block_count"] > 0


def test_decay_strong_releases_chained_entries(pkg, synth, gpu, oracle):
    """A tiny bucket table forces long excess chains, so releases hit heads with chains and chained entries."""
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl, num_buckets=0x100, num_excess=0x800)
    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 10, decay=(255, 1, False))
    st = last["gpu"]["stats"]
    assert st["decayed_block_count"] > 300


def test_slide_window(pkg, synth, gpu, oracle):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl, num_buckets=0x400, num_excess=0x800)
    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 14, slide=3)
    st = last["gpu"]["stats"]
    assert st["fusion_fifo_len"] == 3 and st["slid_block_count"] > 0


def test_ring_push_by_trailing_workgroups(pkg, synth, gpu, oracle):
    """From 65536 visible blocks on, ProcessFrame's fusion kernel queues the visible list on the ring from extra workgroups
    at the end of its grid instead of from its block waves (integrate.hip, kPushJobMin).  The threshold is lowered to 0 here,
    so that every frame of a window + decay sequence takes that path: rings (through what the window releases), last_seen
    and the map must be the oracle's after every frame."""
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl)
    gpu.debug_set_push_job_min(0)
    try:
        objs, last = _run_pair(gpu, oracle, pkg, wl, p, 14, decay=(1, 2, True), slide=4)
    finally:
        gpu.debug_set_push_job_min(65536)
    assert last["gpu"]["stats"]["slid_block_count"] > 0


def test_streaming_instantiations_of_fusion_and_deintegration(pkg, synth, gpu, oracle):
    """Launches over at least push_job_min visible blocks run the STREAM instantiations of k_integrate (non-temporal loads and
    stores of the voxel blocks, chosen by the host from the visible count the allocation sweep reported;
    integrate.hip STREAM: load_nt / store_nt).  With the threshold at 0 every fusion AND de-integration of an online-correction sequence takes
    them: same map as the oracle after every frame."""
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl)

    def extra(i, api, s, rs, v):
        if i >= 3:
            j = i - 3
            rgba, mm, M_old = wl.frame(j)
            M_new = synth.world_to_camera(wl.pose(j) @ synth.pose_matrix(synth.look_rotation(0.01, 0.0), [0.01, 0.0, 0.005]))
            api.view_update(v, rgba, mm, timestamp=float(j))
            api.deprocess_frame(s, v, rs, M_old, wl.intr)
            api.process_frame(s, v, rs, M_new, wl.intr, is_defusion=True)

    before = gpu.debug_stream_launches()
    gpu.debug_set_push_job_min(0)
    try:
        _run_pair(gpu, oracle, pkg, wl, p, 8, slide=4, extra=extra)
    finally:
        gpu.debug_set_push_job_min(65536)
    assert gpu.debug_stream_launches() - before == 8 + 2 * 5   # every fusion, de-integration and re-fusion
    # ... and an ordinary sequence never takes them
    _run_pair(gpu, oracle, pkg, wl, p, 3)
    assert gpu.debug_stream_launches() - before == 8 + 2 * 5


def test_slide_window_and_decay_together(pkg, synth, gpu, oracle):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl)
    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 14, decay=(1, 2, True), slide=4)
    st = last["gpu"]["stats"]
    assert st["slid_block_count"] > 0


def test_defusion_ring_and_reintegration(pkg, synth, gpu, oracle):
    """DenseSlam::OnlineCorrection (DenseSlam.cpp:390-403): de-integrate at the old pose, re-integrate with
    isDefusion=true; then SlideWindowDefusionPart trims the defusion ring."""
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl)

    def extra(i, api, s, rs, v):
        if i >= 3:
            j = i - 3
            rgba, mm, M_old = wl.frame(j)
            M_new = synth.world_to_camera(wl.pose(j) @ synth.pose_matrix(synth.look_rotation(0.01, 0.0), [0.01, 0.0, 0.005]))
            api.view_update(v, rgba, mm, timestamp=float(j))
            api.deprocess_frame(s, v, rs, M_old, wl.intr)
            api.process_frame(s, v, rs, M_new, wl.intr, is_defusion=True)
            api.slide_window_defusion_part(s, rs, 4, 2)

    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 9, slide=4, extra=extra)
    st = last["gpu"]["stats"]
    assert st["defusion_fifo_len"] == 2 and st["fusion_fifo_len"] == 4


def test_swapping_every_frame_and_flush(pkg, synth, gpu, oracle):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl, use_swapping=1)
    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 8, swap_flush_at=5)
    (g, gs, grs, gv), (o, os_, ors, ov) = objs["gpu"], objs["oracle"]
    h = last["gpu"]["hash"]
    out = np.nonzero(h["ptr"] == -1)[0]
    assert len(out) > 0, "nothing is swapped out at the end"
    occupied = np.nonzero(h["ptr"] >= -1)[0]
    n_stored = 0
    for t in list(out) + list(occupied[::7][:80]):
        a, ba = g.download_stored_block(gs, int(t))
        b, bb = o.download_stored_block(os_, int(t))
        assert a == b
        if a:
            n_stored += 1
            assert np.array_equal(ba.view(np.uint64), bb.view(np.uint64))
    assert n_stored > 20


def test_swapping_with_sliding_window(pkg, synth, gpu, oracle):
    """BASELINE config 2: decay + host swap-out as the sliding-window memory path."""
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl, use_swapping=1)
    objs, last = _run_pair(gpu, oracle, pkg, wl, p, 12, decay=(1, 2, True), slide=3)
    # with swapping on, SaveToGlobalMemory already moved every block that left the view to the host each frame,
    # so the window pop finds nothing resident to move; the memory bound comes from the swap-out itself
    assert (last["gpu"]["hash"]["ptr"] == -1).sum() > 0
    used = p.num_local_blocks - 1 - last["gpu"]["stats"]["last_free_block_id"]
    assert used == (last["gpu"]["hash"]["ptr"] >= 0).sum()
