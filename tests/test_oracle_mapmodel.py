"""The map model of refmap.py against the CPU oracle: check
bodies in refmap_checks.py, shared with test_gpu_mapmodel.py.  Plus what needs no engine: the reach counts and tie caps
of every case from the model alone, and the model's own building blocks against hand-derived answers."""
import ctypes

import numpy as np
import pytest

import refmap
import refmap_checks as mc

FRAMES = [("tiny_61x47", mc.MU_OFF), ("tiny_61x47", mc.MU_SHIPPED), ("room_61x47", mc.MU_OFF),
          ("room_61x47", mc.MU_SHIPPED), ("room_640x480", mc.MU_OFF)]


@pytest.mark.parametrize("which,mu_vox", FRAMES)
def test_frames(pkg, oracle, synth, which, mu_vox):
    print(mc.case_frames(oracle, pkg, synth, which, mu_vox)["ties"])


def test_three_coordinate_planes(pkg, oracle, synth):
    print(mc.case_three_planes(oracle, pkg, synth))


def test_depth_gates(pkg, oracle):
    print(mc.case_gates(oracle, pkg))


@pytest.mark.parametrize("num_buckets", [256, 1024])
def test_chains_and_contended_slots(pkg, oracle, synth, num_buckets):
    print(mc.case_chains(oracle, pkg, synth, num_buckets)["max_chain"])


@pytest.mark.parametrize("which", ["blocks", "excess", "both"])
def test_pool_exhaustion(pkg, oracle, synth, which):
    print(mc.case_exhaustion(oracle, pkg, synth, which))


def test_only_update_visible_list(pkg, oracle, synth):
    mc.case_only_visible(oracle, pkg, synth)


@pytest.mark.parametrize("swapping", [False, True])
def test_visible_retest(pkg, oracle, synth, swapping):
    print(mc.case_retest(oracle, pkg, synth, swapping))


def test_decay_thresholds(pkg, oracle, synth):
    print(mc.case_decay_thresholds(oracle, pkg, synth))


def test_decay_modes_agree(pkg, oracle, synth):
    print(mc.case_decay_modes_agree(oracle, pkg, synth))


@pytest.mark.parametrize("seed", [0, 1])
def test_batch_release(pkg, oracle, synth, seed):
    print(mc.case_release(oracle, pkg, synth, seed)["first"])


def test_slide_window_and_wrapped_ring(pkg, oracle, synth):
    print(mc.case_slide_window(oracle, pkg, synth)["total"])


def test_swapping_scene_window_and_decay(pkg, oracle, synth):
    print(mc.case_swapping_window(oracle, pkg, synth)["reach"])


@pytest.mark.parametrize("max_w", [100, 4, 255])
def test_crafted_merge(pkg, oracle, synth, max_w):
    out = mc.case_crafted_merge(oracle, pkg, synth, max_w)
    print(out["tie_share_random_half"], out["tie_share_all"], out["figures"], out["figures_random_half"])


def test_flush_to_the_host_store(pkg, oracle, synth):
    print(mc.case_flush(oracle, pkg, synth)["reach"])


@pytest.mark.parametrize("first_ring", [0, 1])
@pytest.mark.parametrize("swapping", [False, True])
def test_defusion_ring(pkg, oracle, synth, swapping, first_ring):
    print(mc.case_defusion_ring(oracle, pkg, synth, swapping, first_ring)["reach"])


def test_sequence_flush_then_merge(pkg, oracle, synth):
    print(mc.case_flush_sequence(oracle, pkg, synth)["merges"])


@pytest.mark.parametrize("seed", mc.seeds())
def test_sequence(pkg, oracle, synth, seed):
    print(mc.run_sequence(oracle, pkg, synth, seed)["ties"])


def test_sequence_at_shipped_mu(pkg, oracle, synth):
    out = mc.run_sequence(oracle, pkg, synth, 3, mu_vox=mc.MU_SHIPPED)
    assert out["ties"]["step_tie_samples"] > 0  # the step count is a float32 rounding matter there: counted apart
    print(out["ties"])


@pytest.mark.parametrize("case", sorted(mc.geometry_cases()))
def test_band_geometry(pkg, oracle, case):
    print(mc.check_geometry(oracle, pkg, case))


# ---- the model alone: reach and tie caps need no engine -----------------------------------------------------------------
def test_reach_and_tie_caps_from_the_model_alone(pkg, synth):
    """Every case body with api=None: its reach floors and tie caps are assertions about the inputs and the model."""
    for which, mu_vox in FRAMES:
        mc.case_frames(None, pkg, synth, which, mu_vox)
    mc.case_three_planes(None, pkg, synth)
    mc.case_gates(None, pkg)
    for num_buckets in (256, 1024):
        mc.case_chains(None, pkg, synth, num_buckets)
    for which in ("blocks", "excess", "both"):
        mc.case_exhaustion(None, pkg, synth, which)
    mc.case_only_visible(None, pkg, synth)
    for swapping in (False, True):
        mc.case_retest(None, pkg, synth, swapping)
    mc.case_decay_thresholds(None, pkg, synth)
    mc.case_decay_modes_agree(None, pkg, synth)
    for seed in (0, 1):
        mc.case_release(None, pkg, synth, seed)
    mc.case_slide_window(None, pkg, synth)
    mc.case_swapping_window(None, pkg, synth)
    for seed in [s for s in mc.seeds() if s < mc.FIRST_NEW_SEED]:  # (the later seeds: in the test below)
        mc.run_sequence(None, pkg, synth, seed)
    mc.run_sequence(None, pkg, synth, 3, mu_vox=mc.MU_SHIPPED)


def test_reach_of_the_swapping_and_defusion_cases_from_the_model_alone(pkg, synth):
    """The crafted merge's edge rows (each in >= 512 voxels) and tie cap, the flush's and the defusion ring's reach
    floors, and what the new seeds draw: no engine in the loop."""
    for max_w in (100, 4, 255):
        out = mc.case_crafted_merge(None, pkg, synth, max_w)
        assert min(out["reach"].values()) >= 512
    mc.case_flush(None, pkg, synth)
    for swapping in (False, True):
        for first_ring in (0, 1):
            mc.case_defusion_ring(None, pkg, synth, swapping, first_ring)
    mc.case_flush_sequence(None, pkg, synth)
    ops, merged = {}, 0
    for seed in [s for s in mc.seeds() if s >= mc.FIRST_NEW_SEED]:
        out = mc.run_sequence(None, pkg, synth, seed)
        assert out["swapping"] == (seed % 3 == 0)
        merged += out["merges"]["blocks"]
        for op in out["ops"]:
            ops[op] = ops.get(op, 0) + 1
    if mc.seeds() == list(range(18)):
        assert all(ops.get(op, 0) >= 3 for op in ("refuse", "slide_defusion", "decay_defusion", "swap_in", "swap_out", "flush")), ops
        assert merged >= 300, merged


def test_combine_stored_by_hand():
    """SURVEY A.8's merge on voxels worked out by hand."""
    import analytic_maps as am
    import ref64
    h, d = np.zeros(6, am.VOXEL_DTYPE), np.zeros(6, am.VOXEL_DTYPE)
    #            sdf   w  colour        w
    rows = [((100, 1, (10, 20, 30), 1), (-101, 1, (11, 20, 33), 3)),    # -1/2 -> 0;   (10+33)/4 = 10.75, 20, (30+99)/4 = 32.25
            ((-7, 3, (0, 0, 255), 2), (-8, 1, (255, 0, 0), 2)),         # -29/4 = -7.25 -> -7;  127.5 -> 127, 0, 127
            ((5, 0, (1, 2, 3), 0), (9, 2, (4, 5, 6), 1)),               # no host measurement: nothing changes
            ((32767, 200, (255, 255, 255), 200), (32767, 100, (255, 255, 255), 90)),  # weights clamp at 255
            ((300, 2, (9, 9, 9), 0), (0, 0, (7, 7, 7), 5)),             # depth: the host's value and weight; colour idle
            ((3, 1, (1, 1, 1), 1), (4, 2, (1, 1, 2), 2))]               # 11/3 -> 3; colour 1, 1, 5/3 -> 1
    for i, (a, b) in enumerate(rows):
        h[i], d[i] = mc._const_block(*a)[0], mc._const_block(*b)[0]
    lo, hi, info = ref64.combine_stored(h, d, 255)
    # a quotient that is an integer n > 0 is a tie (float32 may end just below it): n - 1 and n are permitted; every
    # other quotient here is far from an integer and has one permitted result
    for f, tie in (("sdf", info["tie_sdf"]), ("clr", info["tie_clr"])):
        assert np.array_equal(hi[f].astype(int) - lo[f], tie & (hi[f] > 0)), f
    assert info["tie_sdf"].tolist() == [False, False, False, True, True, False]
    assert info["tie_clr"].tolist() == [[False, True, False], [False, True, False], [False] * 3, [True] * 3, [False] * 3, [True, True, False]]
    lo = hi
    want = [(0, 2, (10, 20, 32), 4), (-7, 4, (127, 0, 127), 4), (9, 2, (4, 5, 6), 1), (32767, 255, (255, 255, 255), 255),
            (300, 2, (7, 7, 7), 5), (3, 3, (1, 1, 1), 3)]
    for i, wnt in enumerate(want):
        got = (int(lo[i]["sdf"]), int(lo[i]["w_depth"]), tuple(int(c) for c in lo[i]["clr"]), int(lo[i]["w_color"]))
        assert got == wnt, (i, got, wnt)
    # a tie: 199 x 1 + 1 x 2 over 200 = 1.005, within 1/100 of 1 but on its far side; 99 x 1 + 1 x 0 over 100 = 0.99
    h, d = np.zeros(2, am.VOXEL_DTYPE), np.zeros(2, am.VOXEL_DTYPE)
    h[0], d[0] = mc._const_block(1, 199, 0, 0)[0], mc._const_block(2, 1, 0, 0)[0]
    h[1], d[1] = mc._const_block(1, 99, 0, 0)[0], mc._const_block(0, 1, 0, 0)[0]
    lo, hi, info = ref64.combine_stored(h, d, 255)
    assert list(lo["sdf"]) == [0, 0] and list(hi["sdf"]) == [1, 1] and info["tie_sdf"].all()
    assert list(lo["w_depth"]) == [200, 100]


def test_step_count_is_a_rounding_matter_at_the_shipped_mu(synth):
    """mu = 4 voxelSize: 2 |dir| = 2.0 give or take an ulp, so ceil gives 2 or 3 by rounding; mu = 3.46: never."""
    wl = synth.s_tiny(96, 72)
    rgba, mm, _ = wl.frame(4)
    depth = np.where((mm <= 0), -1.0, mm * np.float64(np.float32(0.001))).astype(np.float32)
    M = mc.turned(synth, wl, 4, 0.21, -0.13)
    shipped = refmap.Walk(depth, M, wl.intr, 0.02, 0.08, 0.2, 3.0)
    off = refmap.Walk(depth, M, wl.intr, 0.02, 0.02 * mc.MU_OFF, 0.2, 3.0)
    s = shipped.steps[shipped.steps > 0]
    assert set(np.unique(s)) == {2, 3} and min((s == 2).mean(), (s == 3).mean()) > 0.1
    assert shipped.step_tie_pixels > 0.1 * shipped.n_pixels
    assert off.step_tie_pixels == 0 and off.gate_ties == 0 and off.block_tie.sum() <= 1e-3 * off.n
    assert set(np.unique(off.steps[off.steps > 0])) == {2}  # ceil(mu / (2 voxelSize)) = ceil(1.73)


def test_float32_inverse_is_the_engines(oracle):
    """inv_f32 restates Matrix4::inv operation by operation; the oracle exports the function it uses."""
    rng = np.random.default_rng(5)
    f = oracle.lib.oracle_invert_matrix
    for _ in range(50):
        a = rng.normal(size=3)
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        M = np.eye(4, dtype=np.float32)
        M[:3, :3], M[:3, 3] = R, a
        src = np.ascontiguousarray(M.T).ravel()
        dst = np.zeros(16, np.float32)
        assert f(src.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), dst.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
        assert np.array_equal(dst.reshape(4, 4).T, refmap.inv_f32(M))


def test_hash_index_known_answers():
    """SURVEY Appendix C."""
    kat = {(0, 0, 0): 0, (1, 0, 0): 455773, (0, 1, 0): 475301, (0, 0, 1): 655287, (1, 2, 3): 363058,
           (-1, -1, -1): 505009, (-5, 7, 100): 531920, (32767, -32768, 12): 915255, (10, -3, 25): 413036}
    for b, h in kat.items():
        assert refmap.hash_index(np.array(b), 0x100000) == h


def test_release_by_hand(pkg):
    """A chain head -> a -> b -> c (excess slots 3, 1, 2): releasing the head and a pulls b into the head, keeps c
    behind it, and frees excess slots 1 and 3 in ascending order."""
    p = pkg.SceneParams(num_local_blocks=8, num_buckets=4, num_excess=4, history_words=1)
    m = refmap.MapModel(p, 8, 8)
    h = m.hash.copy()
    pos = [b for b in ((x, y, 0) for x in range(40) for y in range(40)) if refmap.hash_index(np.array(b), 4) == 2][:4]
    for t, b, off, ptr in ((2, pos[0], 4, 7), (4 + 3, pos[1], 2, 6), (4 + 1, pos[2], 3, 5), (4 + 2, pos[3], 0, 4)):
        h[t] = (b, 0, off, ptr)
    m.load(h, np.arange(8), 3, np.array([0, 0, 0, 0]), 0)
    assert m.chain(2) == [2, 7, 5, 6]
    reach = m.release([2, 7])
    assert reach["head_and_first_child"] == 1 and reach["multi"] == 1
    assert tuple(m.hash["pos"][2]) == pos[2] and m.hash["ptr"][2] == 5 and m.hash["offset"][2] == 3
    assert tuple(m.hash["pos"][6]) == pos[3] and m.hash["offset"][6] == 0
    assert m.hash["ptr"][7] == -2 and m.hash["ptr"][5] == -2
    assert list(m.alloc_list[:m.last_free + 1]) == [0, 1, 2, 3, 7, 6]
    assert list(m.excess_list[:m.last_free_ex + 1]) == [0, 1, 3]
