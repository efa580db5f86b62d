"""The map model of refmap.py against the HIP engine: the check bodies of refmap_checks.py (the same ones
test_oracle_mapmodel.py runs on the CPU oracle), the state compared exactly after every call."""
import pytest

import refmap_checks as mc

pytestmark = pytest.mark.gpu

FRAMES = [("tiny_61x47", mc.MU_OFF), ("tiny_61x47", mc.MU_SHIPPED), ("room_61x47", mc.MU_OFF),
          ("room_61x47", mc.MU_SHIPPED), ("room_640x480", mc.MU_OFF)]


@pytest.mark.parametrize("which,mu_vox", FRAMES)
def test_frames(pkg, gpu, synth, which, mu_vox):
    print(mc.case_frames(gpu, pkg, synth, which, mu_vox)["ties"])


def test_three_coordinate_planes(pkg, gpu, synth):
    print(mc.case_three_planes(gpu, pkg, synth))


def test_depth_gates(pkg, gpu):
    print(mc.case_gates(gpu, pkg))


@pytest.mark.parametrize("num_buckets", [256, 1024])
def test_chains_and_contended_slots(pkg, gpu, synth, num_buckets):
    print(mc.case_chains(gpu, pkg, synth, num_buckets)["max_chain"])


@pytest.mark.parametrize("which", ["blocks", "excess", "both"])
def test_pool_exhaustion(pkg, gpu, synth, which):
    print(mc.case_exhaustion(gpu, pkg, synth, which))


def test_only_update_visible_list(pkg, gpu, synth):
    mc.case_only_visible(gpu, pkg, synth)


@pytest.mark.parametrize("swapping", [False, True])
def test_visible_retest(pkg, gpu, synth, swapping):
    print(mc.case_retest(gpu, pkg, synth, swapping))


def test_decay_thresholds(pkg, gpu, synth):
    print(mc.case_decay_thresholds(gpu, pkg, synth))


def test_decay_modes_agree(pkg, gpu, synth):
    print(mc.case_decay_modes_agree(gpu, pkg, synth))


@pytest.mark.parametrize("seed", [0, 1])
def test_batch_release(pkg, gpu, synth, seed):
    print(mc.case_release(gpu, pkg, synth, seed)["first"])


def test_slide_window_and_wrapped_ring(pkg, gpu, synth):
    print(mc.case_slide_window(gpu, pkg, synth)["total"])


def test_swapping_scene_window_and_decay(pkg, gpu, synth):
    print(mc.case_swapping_window(gpu, pkg, synth)["reach"])


@pytest.mark.parametrize("max_w", [100, 4, 255])
def test_crafted_merge(pkg, gpu, synth, max_w):
    out = mc.case_crafted_merge(gpu, pkg, synth, max_w)
    print(out["tie_share_random_half"], out["tie_share_all"], out["figures"], out["figures_random_half"])


def test_flush_to_the_host_store(pkg, gpu, synth):
    print(mc.case_flush(gpu, pkg, synth)["reach"])


@pytest.mark.parametrize("first_ring", [0, 1])
@pytest.mark.parametrize("swapping", [False, True])
def test_defusion_ring(pkg, gpu, synth, swapping, first_ring):
    print(mc.case_defusion_ring(gpu, pkg, synth, swapping, first_ring)["reach"])


def test_sequence_flush_then_merge(pkg, gpu, synth):
    print(mc.case_flush_sequence(gpu, pkg, synth)["merges"])


@pytest.mark.parametrize("seed", mc.seeds())
def test_sequence(pkg, gpu, synth, seed):
    print(mc.run_sequence(gpu, pkg, synth, seed)["ties"])


def test_sequence_at_shipped_mu(pkg, gpu, synth):
    out = mc.run_sequence(gpu, pkg, synth, 3, mu_vox=mc.MU_SHIPPED)
    assert out["ties"]["step_tie_samples"] > 0
    print(out["ties"])


@pytest.mark.parametrize("case", sorted(mc.geometry_cases()))
def test_band_geometry(pkg, gpu, case):
    print(mc.check_geometry(gpu, pkg, case))
