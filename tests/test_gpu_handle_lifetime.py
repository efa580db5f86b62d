"""An engine outlives the handles made from it (include/dslam_fusion.h, dslam_engine_destroy): handles may be destroyed
in any order.  dslam_debug_live_engines counts the engine objects not yet freed, which makes the deferral observable.
On a tree without the hook the test stops at its first assertion, before it does anything that was undefined there."""
import pytest

import util

pytestmark = pytest.mark.gpu

ORDERS = {"scene last": ("store", "view", "rs", "scene"), "store last": ("rs", "scene", "view", "store")}


def open_with_handles(pkg, synth):
    wl = synth.s_tiny()
    api = pkg.open_engine(0)
    scene = api.create_scene(util.small_params(pkg, wl))
    rs = api.create_render_state(scene, wl.W, wl.H)
    view = api.create_view(wl.W, wl.H)
    store = api.create_frame_store(wl.W, wl.H, 2)
    rgba, mm, M = wl.frame(0)
    api.view_update(view, rgba, mm)
    api.process_frame(scene, view, rs, M, wl.intr)   # (the handles have been used, not only made)
    return api, dict(scene=scene, rs=rs, view=view, store=store)


@pytest.mark.parametrize("order", list(ORDERS), ids=list(ORDERS))
def test_an_engine_closed_first_goes_with_its_last_handle(pkg, synth, gpu, order):
    assert "dslam_debug_live_engines" in pkg.exported_symbols(), "the library has no dslam_debug_live_engines"
    base = gpu.debug_live_engines()
    api, handles = open_with_handles(pkg, synth)
    assert gpu.debug_live_engines() == base + 1
    api.close()                                      # the engine first: its handles keep the object and its streams
    assert gpu.debug_live_engines() == base + 1
    names = ORDERS[order]
    for name in names[:-1]:
        handles[name].close()
        assert gpu.debug_live_engines() == base + 1, name
    handles[names[-1]].close()                       # the count drops exactly at the last handle
    assert gpu.debug_live_engines() == base
    # the session's engine is none the worse for it
    assert gpu.selftest_division(1 << 12) == 0


def test_an_engine_without_handles_goes_at_once(pkg, synth, gpu):
    assert "dslam_debug_live_engines" in pkg.exported_symbols(), "the library has no dslam_debug_live_engines"
    base = gpu.debug_live_engines()
    api, handles = open_with_handles(pkg, synth)
    for name in ("scene", "rs", "view", "store"):    # the handles first, as before
        handles[name].close()
        assert gpu.debug_live_engines() == base + 1
    api.close()
    assert gpu.debug_live_engines() == base
    api = pkg.open_engine(0)                         # ... and an engine that never had one
    assert gpu.debug_live_engines() == base + 1
    api.close()
    assert gpu.debug_live_engines() == base
