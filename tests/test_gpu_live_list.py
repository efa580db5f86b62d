"""The calls that read a map's live list, back to back on one engine.

pack, mesh, register, merge, unmerge and the overlap survey all get the list of a scene's resident entries from one
launcher and one kernel (csrc/live_list.hip), on an engine whose ticket chain and scratch lists they share.  Here they run
one after the other on one engine, over two scenes whose tables differ in size, and every call must give what the same
call gives on an engine that has run nothing else; the packs are also held to the packed-map law (tests/ref_pack.py) and
the merge and the unmerge to theirs (tests/ref_merge.py, tests/ref_unmerge.py).  Everything compared is integers or bytes.

B's table has resident entries at hash indices 8191 and 8192 (the last entry of selection tile 0 and the first of tile 1,
a tile being 8192 entries), at the last bucket head, in the excess area, and an entry with ptr == -1 (swapped out), which
no live list may hold.  (upload_scene_state sets an entry's bit in alloc_bits for ptr >= 0 only, so that entry's bit is
clear here; a scene that sets it for ptr == -1 swaps, and a swapping scene cannot be packed.)"""
import contextlib

import numpy as np
import pytest

import analytic_maps as am
import pack_fixtures as pf
import ref_merge as rm
import ref_pack
import ref_unmerge as ru
import refmap
from test_gpu_pack import DeviceBuffer, load, pack_into

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)
NB_A, NX_A, NB_B, NX_B = 0x400, 16, 0x4000, 64
TILE = 8192                    # entries of one selection tile (csrc/dslam_bits.h)
FAR = (29, -29, 29)            # the swapped-out entry's block: no block of A is near it


def voxels(rng, n):
    """n blocks of voxels a merge into empty voxels and the unmerge behind it give back exactly: any sdf, depth weights far
    below max_w, no colour."""
    v = np.zeros((n, 512), am.VOXEL_DTYPE)
    v["sdf"] = rng.integers(-32767, 32768, (n, 512))
    v["w_depth"] = rng.integers(1, 41, (n, 512))
    return v.view(np.uint64).reshape(n, 512)


def params_of(pkg, nb, nx, nl):
    return pf.scene_params(pkg, nb, nx, nl, voxel_size=am.VS, mu=am.MU, max_w=100)


def as_state(st, nb):
    return rm.State(st["hash"], st["alloc_list"], st["last_free_block_id"], st["excess_list"], st["last_free_excess_id"],
                    st["voxels"].view(am.VOXEL_DTYPE), nb, am.VS, am.MU)


@pytest.fixture(scope="module")
def maps(pkg):
    """((params, state) of A, (params, state) of B), tables built as test_gpu_pack.heads_and_one_chain builds them."""
    rng = np.random.default_rng(23)
    # A: 36 bucket heads and one chain of 4
    heads = [b for b in pf.heads_only(NB_A, 48, seed=9) if int(refmap.hash_index(b, NB_A)) != 5 and b != FAR][:36]
    blocks_a = pf.colliding(NB_A, 5, 4) + heads
    pa = params_of(pkg, NB_A, NX_A, len(blocks_a) + 4)
    a = pf.build(pa, blocks_a, seed=1)
    res = np.flatnonzero(a["hash"]["ptr"] >= 0)
    a["voxels"][a["hash"]["ptr"][res]] = voxels(rng, len(res))
    # B: every block of A (empty voxels: the merge allocates nothing and the unmerge restores them), one block in each
    # bucket named above, a chain of 4 in bucket 77, and FAR
    taken = set(blocks_a) | {FAR}
    own = []
    for bucket, count in ((TILE - 1, 1), (TILE, 1), (NB_B - 1, 1), (77, 4)):
        own += [b for b in pf.colliding(NB_B, bucket, count + 4) if b not in taken][:count]
    assert len(own) == 7 and int(refmap.hash_index(FAR, NB_B)) not in (TILE - 1, TILE, NB_B - 1, 77)
    pb = params_of(pkg, NB_B, NX_B, len(blocks_a) + len(own) + 5)
    b = pf.build(pb, blocks_a + own + [FAR], seed=2)
    h = b["hash"]
    at = {tuple(int(c) for c in h["pos"][t]): int(t) for t in np.flatnonzero(h["ptr"] >= 0)}
    b["voxels"][:] = pf.EMPTY
    b["voxels"][[h["ptr"][at[blk]] for blk in own]] = voxels(rng, len(own))
    h["ptr"][at[FAR]] = -1
    live = np.flatnonzero(h["ptr"] >= 0)
    assert {TILE - 1, TILE, NB_B - 1} <= set(live.tolist()) and (live >= NB_B).sum() >= 3 and at[FAR] not in live
    assert (np.flatnonzero(a["hash"]["ptr"] >= 0) >= NB_A).sum() == 3
    return (pa, a), (pb, b)


def same_bytes(x, y):
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same_bytes(p, q) for p, q in zip(x, y))
    if x is None or y is None:
        return x is y
    return bytes(np.ascontiguousarray(x)) == bytes(np.ascontiguousarray(y)) if isinstance(x, np.ndarray) else bytes(x) == bytes(y)


def test_every_reader_of_the_live_list_on_one_engine(pkg, maps):
    (pa, a), (pb, b) = maps
    src, dst = as_state(a, NB_A), as_state(b, NB_B)
    # the reference: the merge allocates nothing and the unmerge gives B back exactly
    merged = dst.copy()
    want_merge = rm.merge(src, merged, I4)
    back = merged.copy()
    want_unmerge = ru.unmerge(src, back, I4)
    assert want_merge["blocks_allocated"] == 0 and want_merge["voxels_changed"] == want_merge["src_candidates"] == 40 * 512
    assert want_unmerge["voxels_changed"] == 40 * 512 and not dst.differences(back) and dst.differences(merged)
    b_merged = dict(b, voxels=merged.vba.view(np.uint64).reshape(-1, 512))
    image_a, image_b = ref_pack.pack(a), ref_pack.pack(b)
    one = pkg.RegisterParams(max_evaluations=1)

    def pack(api, scene):
        buf = DeviceBuffer(api.pack_scene(scene).total_bytes)
        try:
            info, raw = pack_into(api, scene, buf)
            return bytes(info), raw
        finally:
            buf.release()

    # (name, B's state in front of the call, the call)
    steps = [
        ("pack A", b, lambda api, sa, sb: pack(api, sa)),
        ("mesh B", b, lambda api, sa, sb: api.mesh_scene(sb)),
        ("pack B", b, lambda api, sa, sb: pack(api, sb)),
        ("register A -> B", b, lambda api, sa, sb: api.register_maps(sa, sb, I4, one)),
        ("merge A -> B", b, lambda api, sa, sb: api.merge_maps(sa, sb, I4)),
        ("unmerge A -> B", b_merged, lambda api, sa, sb: api.unmerge_maps(sa, sb, I4)),
        ("survey [A, B]", b, lambda api, sa, sb: api.survey_overlaps([sa, sb], [I4, I4])),
        ("pack A again", b, lambda api, sa, sb: pack(api, sa)),
        ("pack B again", b, lambda api, sa, sb: pack(api, sb)),
    ]
    got = {}
    with contextlib.ExitStack() as stack:
        api = pkg.open_engine(0)
        stack.callback(api.close)
        sa, sb = load(api, pkg, pa, a), load(api, pkg, pb, b)
        for name, _, call in steps:
            got[name] = call(api, sa, sb)
            if name == "merge A -> B":
                assert not merged.differences(rm.State.download(api, sb, dst)), "the merged destination is not the reference's"
            if name == "unmerge A -> B":
                assert not dst.differences(rm.State.download(api, sb, dst)), "the unmerge did not give B back"
        assert not src.differences(rm.State.download(api, sa, src)), "A changed"
        sb.close(), sa.close()
    # the laws
    assert got["pack A"][1] == image_a == got["pack A again"][1] and got["pack A"][0] == image_a[:64]
    assert got["pack B"][1] == image_b == got["pack B again"][1] and got["pack B"][0] == image_b[:64]
    assert ref_pack.header_fields(image_a)["blocks"] == 40 and ref_pack.header_fields(image_b)["blocks"] == 47
    assert got["merge A -> B"].as_dict() == want_merge and got["unmerge A -> B"].as_dict() == want_unmerge
    live, shared, _ = got["survey [A, B]"]
    assert live.tolist() == [40, 47] and shared[0, 1] == shared[1, 0] == 40
    assert len(got["mesh B"][0]) > 0
    # each call on an engine that has run nothing else (the second packs are the first ones' calls on the same states)
    for name, b_before, call in steps[:-2]:
        with contextlib.ExitStack() as stack:
            fresh = pkg.open_engine(0)
            stack.callback(fresh.close)
            sa, sb = load(fresh, pkg, pa, a), load(fresh, pkg, pb, b_before)
            alone = call(fresh, sa, sb)
            sb.close(), sa.close()
        assert same_bytes(got[name], alone), f"{name}: not what the call gives on a fresh engine"
