"""The HIP kernels' voxel update and de-integration (A.11) on crafted voxels and measurements, every stored
value against ref64.update_exact, once per kernel form (refvoxel_checks.py).  The form a case runs follows from
the launch conditions of csrc/integrate.hip, which each case sets up: the plain kernel (one camera, no option), the general
one-camera kernel (stopIntegratingAtMaxW or depth weighting), the two-camera kernel, the one- and two-camera
de-integrations (each also with depth weights), the block kernel of the re-integration batch; the streaming and front-end
instantiations are shown by the engine's own counters."""
import pytest

import refvoxel_checks as rv

pytestmark = pytest.mark.gpu

# form -> (stopIntegratingAtMaxW, depth weighting, a second camera, de-integration): what launch_integrate chooses by
LAUNCH_CONDITIONS = {"plain": (0, False, False, False), "stop": (1, False, False, False), "depth_weights": (0, True, False, False),
                     "two_cameras": (0, False, True, False), "deprocess": (0, False, False, True),
                     "deprocess_two_cameras": (0, False, True, True), "deprocess_stop": (1, False, False, True),
                     "deprocess_depth_weights": (0, True, False, True), "deprocess_two_cameras_depth_weights": (0, True, True, True)}


@pytest.mark.parametrize("case", rv.cases(), ids=rv.case_id)
def test_crafted_update(pkg, gpu, case):
    before = gpu.debug_stream_launches(), gpu.debug_front_end_counts()[0]
    c = rv.Case(gpu, pkg, *case)
    stop, weights, two, deint = LAUNCH_CONDITIONS[case[2]]
    assert c.conditions() == dict(stop=stop, swapping=0, depth_weights=weights, two_cameras=two, deintegrate=deint)
    c.call()
    fig = c.check()
    assert (gpu.debug_stream_launches(), gpu.debug_front_end_counts()[0]) == before, "not the instantiation this case is about"
    print(rv.case_id(case), fig)


@pytest.mark.parametrize("case", rv.batch_cases(), ids=lambda c: "-".join(map(str, c)))
def test_batch_equals_the_checked_loop(pkg, gpu, case):
    """k_reintegrate_blocks (batch_op / batch_colour_word): three crafted keyframes corrected by the per-keyframe loop over
    their stored lists, every step against update_exact, and by one reintegrate_batch call on a second copy of the state,
    which must equal the loop byte for byte.  Unit and depth weights, whole blocks and (sharded) half blocks; the block
    kernel ran if the batch's own statistics say so."""
    b, h, fig = rv.run_batch(gpu, pkg, *case)
    assert b.conditions(h) == dict(stop=0, swapping=0, depth_weights="depth" in case[0], sharded="shard" in case[0])
    blocks, operations = gpu.reintegrate_batch_stats(h["scene"])
    assert blocks > 0 and operations >= blocks, (blocks, operations)
    print(case, fig, blocks, operations)


@pytest.mark.parametrize("form", ["plain", "deprocess"])
@pytest.mark.parametrize("max_w, mu_steps", [(100, rv.MU_STEPS[1]), (255, rv.MU_STEPS[0])])
def test_streaming_instantiations(pkg, gpu, form, max_w, mu_steps):
    """k_integrate<0,1,1,0,1,0> and <1,1,0,0,1,0>: with push_job_min at 0 the launch counts itself as streaming."""
    c = rv.Case(gpu, pkg, max_w, mu_steps, form, 3)
    before = gpu.debug_stream_launches()
    gpu.debug_set_push_job_min(0)
    try:
        c.call()
    finally:
        gpu.debug_set_push_job_min(65536)
    assert gpu.debug_stream_launches() - before == 1
    print(form, max_w, mu_steps, c.check())


@pytest.mark.parametrize("max_w, mu_steps", [(100, rv.MU_STEPS[1]), (4, rv.MU_STEPS[0]), (255, rv.MU_STEPS[0])])
def test_front_end_instantiation(pkg, gpu, max_w, mu_steps):
    """k_integrate<0,1,1,0,0,1>: ProcessFrame's plain fusion with GetImage's selection tiles at the head of the launch."""
    c = rv.Case(gpu, pkg, max_w, mu_steps, "plain", 1)
    before = gpu.debug_front_end_counts()[0]
    c.call(process_frame=True)
    assert gpu.debug_front_end_counts()[0] - before == 1
    print(max_w, mu_steps, c.check())
