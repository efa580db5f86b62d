"""highslot_fixtures.py checked without a GPU: the banded allocation list, the teeth of every fixture the GPU file relocates,
that a relocated map holds no whole-pool array, and -- on the CPU oracle, in a pool small enough for the host --
upload_sparse, download_blocks and canonical against the whole-pool snapshot, and the law itself."""
import tracemalloc

import numpy as np
import pytest

import analytic_maps as am
import highslot_fixtures as hs
import ref64_checks as rc
import register_fixtures as rf
import register_graph_fixtures as gf
import track_sdf_fixtures as tf
import util

SMALL = 0x8000   # an oracle pool with the same band structure: the middle mark at SMALL / 2


def test_marks():
    assert hs.POOL == 0x100000 and hs.M31 * 4096 == 1 << 31 and (hs.TOP + 1) * 4096 == 1 << 32


@pytest.mark.parametrize("n_blocks,pool", [(37, hs.POOL), (0x2000, hs.POOL), (1, SMALL), (0x2000, SMALL)])
def test_banded_alloc_list(n_blocks, pool):
    a = hs.banded_alloc_list(n_blocks, pool)
    assert a.dtype == np.int32 and len(a) == pool and np.array_equal(np.sort(a), np.arange(pool))
    taken = a[::-1][:n_blocks].astype(np.int64)          # in the order of allocation
    slots, n = hs.banded_slots(n_blocks, pool)
    assert np.array_equal(taken, slots) and n == -(-n_blocks // 4)
    assert taken[:4].tolist()[:n_blocks] == [0, pool // 2 - 1, pool // 2, pool - 1][:n_blocks]
    band = hs.band_of(taken, n, pool)
    assert (band >= 0).all() and (band[1:] != band[:-1]).sum() >= (n_blocks - 1) // 2   # (the two middle lanes share a band)
    assert (np.diff(band.reshape(-1)[: n_blocks // 4 * 4].reshape(-1, 4), axis=0) == 0).all()
    rest = a[:pool - n_blocks]
    assert (np.diff(rest) > 0).all()
    with pytest.raises(AssertionError):
        hs.banded_slots(pool // 4 + 4, pool)


def fixture_maps():
    out = {f"raycast {k}": v[0] for k, v in rc.raycast_cases().items() if k in ("colour_plane", "box_corner", "sphere_inside")}
    out["mesh sphere_outside"] = rc.mesh_cases()["sphere_outside"][0]
    for i in range(3):
        out[f"three_maps {i}"] = lambda i=i: tf.three_maps().maps[i]
        out[f"graph {i}"] = lambda i=i: gf.map_set("small").maps[i]
    out["box src"] = lambda: rf.box_pair("small").src_map
    out["box dst"] = lambda: rf.box_pair("small").dst_map
    return out


@pytest.mark.parametrize("name", sorted(fixture_maps()))
def test_relocated_fixture_has_teeth_and_no_pool_array(name):
    m = fixture_maps()[name]()
    tracemalloc.start()
    r = hs.relocate(m)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < 64 << 20, f"relocate held {peak >> 20} MiB"          # (the whole pool would be 4 GiB)
    held = sum(v.nbytes for v in vars(r).values() if isinstance(v, np.ndarray) and not any(v is w for w in vars(m).values()))
    assert r.vba is None and held < 16 << 20 and m.vba is not None and m.num_local_blocks < hs.POOL
    fig = hs.teeth(r.block_pos, r.ptrs)
    print(name, len(r.ptrs), fig)
    assert fig["slot0"] and fig["below_mark"] and fig["at_mark"] and fig["top"]
    # the same table under other slot names
    live = m.hash["ptr"] >= 0
    assert np.array_equal(r.hash["pos"], m.hash["pos"]) and np.array_equal(r.hash["offset"], m.hash["offset"])
    assert np.array_equal(r.hash["ptr"] >= 0, live) and np.array_equal(r.hash["ptr"][~live], m.hash["ptr"][~live])
    by_pos = {tuple(p): s for p, s in zip(r.block_pos.tolist(), r.ptrs.tolist())}
    assert all(by_pos[tuple(p)] == s for p, s in zip(r.hash["pos"][live].tolist(), r.hash["ptr"][live].tolist()))
    assert r.last_free == hs.POOL - 1 - len(r.ptrs) and not np.isin(r.alloc_list[:r.last_free + 1], r.ptrs).any()


def test_slot_runs():
    slots = np.array([9, 3, 4, 100, 5, 8])
    runs = hs.slot_runs(slots)
    assert [(f, n) for f, n, _ in runs] == [(3, 3), (8, 2), (100, 1)]
    assert [slots[p].tolist() for _, _, p in runs] == [[3, 4, 5], [8, 9], [100]]
    assert hs.slot_runs(np.array([], np.int64)) == []
    with pytest.raises(AssertionError):
        hs.slot_runs([1, 1])


def test_teeth_bite():
    """teeth refuses a placement that misses a band, a side of the mark, or keeps neighbours together."""
    m = am.colour_plane(num_buckets=0x40)
    n = len(m.block_pos)
    slots, _ = hs.banded_slots(n)
    hs.teeth(m.block_pos, slots)
    with pytest.raises(AssertionError, match="per band"):
        hs.teeth(m.block_pos, hs.POOL - 1 - np.arange(n))
    with pytest.raises(AssertionError, match="middle mark"):
        hs.teeth(m.block_pos, np.where(slots >= hs.M31, slots, np.where(slots > hs.M31 // 2, slots - hs.M31 + 2 * n, slots)))
    with pytest.raises(AssertionError, match="face-adjacent"):
        hs.teeth(m.block_pos * 2, slots)       # the same slots, but no block has a face neighbour


# ---------------------------------------------------------------------------------------------------------------------
# on the CPU oracle, in a pool the host can hold
# ---------------------------------------------------------------------------------------------------------------------
def _reference_canonical(api, scene, rs=None):
    """canonical restated on the whole-pool snapshot."""
    snap = util.snapshot(api, scene, rs)
    util.check_invariants(snap, scene.params)
    h = snap["hash"]
    live = h["ptr"] >= 0
    return snap["voxels"][h["ptr"][live]], api.download_last_seen(scene)[h["ptr"][live]], h["ptr"][live]


def test_sparse_upload_and_canonical_on_the_oracle(pkg, oracle):
    m = am.colour_plane(num_buckets=0x40)
    r = hs.relocate(m, SMALL)
    hs.teeth(r.block_pos, r.ptrs, SMALL)
    low, high = oracle.create_scene(m.scene_params(pkg)), oracle.create_scene(r.scene_params(pkg))
    am.upload(oracle, low, m)
    am.upload(oracle, high, r)                      # (goes through r.upload = upload_sparse)
    whole = oracle.download_voxel_blocks(high)
    assert whole[r.ptrs].tobytes() == m.voxels.tobytes()
    rest = np.ones(SMALL, bool)
    rest[r.ptrs] = False
    fresh = oracle.download_voxel_blocks(oracle.create_scene(r.scene_params(pkg)))
    assert whole[rest].tobytes() == fresh[rest].tobytes(), "upload_sparse wrote outside the map's slots"
    assert hs.download_blocks(oracle, high, r.ptrs).tobytes() == m.voxels.tobytes()
    c_low, c_high = hs.canonical(oracle, low), hs.canonical(oracle, high)
    hs.assert_same_canonical(c_low, c_high, "colour plane")
    blocks, seen, slots = _reference_canonical(oracle, high)
    assert c_high["blocks"].tobytes() == blocks.tobytes() and np.array_equal(c_high["last_seen"], seen)
    assert np.array_equal(c_high["slots"], slots) and not np.array_equal(c_high["slots"], c_low["slots"])
    # the law on the oracle: the same image from either placement
    W, H = 64, 48
    M, intr = rc.camera(W, H, roll=0.2)
    imgs = [oracle.get_image(s, oracle.create_render_state(s, W, H), M, intr, pkg.IMAGE_COLOUR_FROM_VOLUME) for s in (low, high)]
    assert imgs[0].tobytes() == imgs[1].tobytes() and (imgs[0][..., 3] > 0).sum() > 500
    # canonical notices a changed voxel, a changed last_seen order and a broken partition
    v = oracle.download_voxel_blocks(high, int(r.ptrs[5]), 1)
    v["sdf"][0, 17] ^= 1
    oracle.upload_voxel_blocks(high, int(r.ptrs[5]), v)
    with pytest.raises(AssertionError, match="voxels differ"):
        hs.assert_same_canonical(c_low, hs.canonical(oracle, high), "one voxel changed")
    oracle.upload_scene_state(high, allocation_list=r.alloc_list, last_free_block_id=r.last_free + 1)
    with pytest.raises(AssertionError, match="live"):
        hs.canonical(oracle, high)


@pytest.mark.parametrize("w,h", [(61, 47), (96, 72)])
def test_s_tiny_in_a_banded_pool_on_the_oracle(pkg, synth, oracle, w, h):
    """S-tiny's first four frames from the banded allocation list: the teeth on the blocks as fusion places them, and the
    law against a plain scene after every frame."""
    wl = synth.s_tiny(w, h)
    n_fuse = 0x2000
    p_low, p_high = util.small_params(pkg, wl, num_local_blocks=n_fuse), util.small_params(pkg, wl, num_local_blocks=SMALL)
    low, high = oracle.create_scene(p_low), oracle.create_scene(p_high)
    oracle.upload_scene_state(high, allocation_list=hs.banded_alloc_list(n_fuse, SMALL), last_free_block_id=SMALL - 1)
    rs = [oracle.create_render_state(s, wl.W, wl.H) for s in (low, high)]
    view = oracle.create_view(wl.W, wl.H)
    for i in range(4):
        rgba, mm, M = wl.frame(i)
        oracle.view_update(view, rgba, mm, timestamp=float(i))
        for s, r in zip((low, high), rs):
            oracle.process_frame(s, view, r, M, wl.intr)
        c = [hs.canonical(oracle, s, r) for s, r in zip((low, high), rs)]
        hs.assert_same_canonical(*c, f"frame {i}")
        print(i, hs.scene_teeth(oracle, high, SMALL))
    blocks, seen, slots = _reference_canonical(oracle, high, rs[1])
    assert c[1]["blocks"].tobytes() == blocks.tobytes() and np.array_equal(c[1]["last_seen"], seen)
    assert c[1]["counters"]["blocks_in_use"] == len(slots) > 200
