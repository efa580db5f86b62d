"""dslam_pack_scene / dslam_unpack_scene on the device against the packed-map law in numpy (tests/ref_pack.py; DESIGN.md
section 21).  Every comparison is of integers or bytes.  The check bodies are refpack_checks.py's, whose sensitivity
test_pack_checks_ref.py shows without a GPU."""
import contextlib

import numpy as np
import pytest

import pack_fixtures as pf
import ref_pack
import refmap
import refpack_checks as rc
import util

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 4096, 0xA5
PACK_GRID = 512   # workgroups of the block kernels (csrc/pack.hip kPackGrid)


# ---- states ---------------------------------------------------------------------------------------------------------
def heads_and_one_chain(pkg, n, chain, nb=1024, nx=16, seed=7):
    """n blocks: one bucket with `chain` entries (chain - 1 excess slots used, f = nx - chain + 1), the rest bucket heads."""
    bucket = 5
    heads = [b for b in pf.heads_only(nb, n, seed=seed) if int(refmap.hash_index(b, nb)) != bucket][:n - chain]
    assert len(heads) == n - chain
    p = pf.scene_params(pkg, nb, nx, n + 4)
    return p, pf.build(p, pf.colliding(nb, bucket, chain) + heads, seed=seed)


def edge_table(pkg):
    """A 0x8000 + 0x1000 table with resident entries written directly at the selection-tile and bit-tile edges."""
    nb, nx, nl = 0x8000, 0x1000, 8
    p = pf.scene_params(pkg, nb, nx, nl)
    idx = [0, 8191, 8192, 32767, 32768, 0x8FFF]
    h = np.zeros(nb + nx, pkg.HASH_ENTRY_DTYPE)
    h["ptr"] = -2
    for j, t in enumerate(idx):
        h[t] = ((j + 1, -(j + 1), 3 * j - 7), 0, 0, nl - 1 - j)
    rng = np.random.default_rng(11)
    vox = np.full((nl, 512), pf.EMPTY, np.uint64)
    vox[nl - len(idx):] = rng.integers(0, 1 << 63, (len(idx), 512), dtype=np.uint64) | np.uint64(1 << 16)
    lf = nl - 1 - len(idx)
    return p, dict(hash=h, voxels=vox, alloc_list=np.arange(nl, dtype=np.int32), last_free_block_id=lf,
                   excess_list=np.arange(nx, dtype=np.int32), last_free_excess_id=nx - 1, params=ref_pack.geometry(p),
                   stats=dict(last_free_block_id=lf, last_free_excess_id=nx - 1))


@pytest.fixture(scope="module")
def cases(pkg):
    """name -> (params, state, the reference's image), computed once."""
    out = {name: (p, st) for name, p, st in pf.states(pkg)}
    p = pf.scene_params(pkg, 1024, 16, 600)
    out["two trips"] = (p, pf.build(p, pf.heads_only(1024, PACK_GRID + 72 + 1), seed=5))   # 585: a second trip, partial
    out["records end on a boundary"] = heads_and_one_chain(pkg, 252, 17)                   # (n, f) = (252, 0)
    out["one word past a boundary"] = heads_and_one_chain(pkg, 252, 16)                    # (252, 1)
    out["tile edges"] = edge_table(pkg)
    full = {name: (p, st, ref_pack.pack(st)) for name, (p, st) in out.items()}
    hd = {name: ref_pack.header_fields(raw) for name, (_, _, raw) in full.items()}
    assert hd["two trips"]["blocks"] == 585
    assert (hd["records end on a boundary"]["blocks"], hd["records end on a boundary"]["free_excess"]) == (252, 0)
    assert (hd["one word past a boundary"]["blocks"], hd["one word past a boundary"]["free_excess"]) == (252, 1)
    assert hd["records end on a boundary"]["blocks_offset"] == 4096 and hd["one word past a boundary"]["blocks_offset"] == 8192
    return full


FIXTURES = ["empty", "one block", "chains and releases", "excess stack empty", "excess stack full"]
EXTRA = ["two trips", "records end on a boundary", "one word past a boundary", "tile edges"]


# ---- plumbing -------------------------------------------------------------------------------------------------------
def load(api, pkg, params, st):
    scene = api.create_scene(params)
    api.upload_scene_state(scene, st["hash"], st["alloc_list"], int(st["last_free_block_id"]), st["excess_list"],
                           int(st["last_free_excess_id"]))
    api.upload_voxel_blocks(scene, 0, np.ascontiguousarray(st["voxels"]).view(pkg.VOXEL_DTYPE))
    return scene


class DeviceBuffer:
    """`nbytes` of device memory between two guards."""
    def __init__(self, nbytes, content=None):
        import torch
        self.torch, self.nbytes = torch, nbytes
        host = np.full(nbytes + 2 * GUARD, GUARD_BYTE, np.uint8)
        if content is not None:
            host[GUARD:GUARD + nbytes] = np.frombuffer(bytes(content), np.uint8)
        self.t = torch.from_numpy(host).to("cuda:0")
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def read(self):
        self.torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def release(self):
        self.t = None


class HostBuffer:
    """The same in page-locked host memory."""
    def __init__(self, api, nbytes):
        self.api, self.nbytes = api, nbytes
        self.arr = api.host_alloc((nbytes + 2 * GUARD,), np.uint8)
        self.arr[:] = GUARD_BYTE
        self.ptr = self.arr.ctypes.data + GUARD
        assert self.ptr % 16 == 0

    def read(self):
        return self.arr.copy()

    def release(self):
        self.api.host_free(self.arr)
        self.arr = None


def split(whole, nbytes):
    """(payload bytes, guards untouched?)"""
    ok = (whole[:GUARD] == GUARD_BYTE).all() and (whole[GUARD + nbytes:] == GUARD_BYTE).all()
    return whole[GUARD:GUARD + nbytes].tobytes(), bool(ok)


def pack_into(api, scene, buf):
    info = api.pack_scene(scene, buf.ptr, buf.nbytes)
    raw, guards = split(buf.read(), buf.nbytes)
    assert guards, "a pack wrote outside [0, total_bytes)"
    return info, raw


def full_snapshot(api, scene):
    snap = util.snapshot(api, scene)
    snap["last_seen"] = api.download_last_seen(scene)
    return snap


def same_snapshot(a, b):
    util.assert_same_state(a, b)
    for k in ("alloc_list", "excess_list", "last_seen"):
        assert np.array_equal(a[k], b[k]), k


def rejected(call):
    with pytest.raises(Exception) as err:
        call()
    assert "failed with status -1" in str(err.value), err.value   # DSLAM_ERR_INVALID, not a HIP failure
    return err


# ---- pack -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES + EXTRA)
def test_pack_equals_the_reference(gpu, pkg, cases, name):
    p, st, want = cases[name]
    scene = load(gpu, pkg, p, st)
    query = gpu.pack_scene(scene)
    assert query.total_bytes == len(want) and bytes(query) == want[:64], "size query"
    dev, host = DeviceBuffer(len(want)), HostBuffer(gpu, len(want))
    try:
        info, raw_dev = pack_into(gpu, scene, dev)
        print(name, "n", info.blocks, "f", info.free_excess, "bytes", info.total_bytes)
        assert bytes(info) == want[:64] == bytes(query)
        rc.check_packed(raw_dev, st)
        info_h, raw_host = pack_into(gpu, scene, host)
        assert raw_host == raw_dev and bytes(info_h) == want[:64], "page-locked and device buffers differ"
        assert pack_into(gpu, scene, dev)[1] == raw_dev, "a second pack differs"
    finally:
        dev.release(), host.release()
        scene.close()


def test_size_query_writes_nothing_and_leaves_the_scene_alone(gpu, pkg, cases):
    p, st, want = cases["chains and releases"]
    scene = load(gpu, pkg, p, st)
    before = full_snapshot(gpu, scene)
    info = gpu.pack_scene(scene, None, 0)
    assert bytes(info) == want[:64] and bytes(gpu.pack_scene(scene, None, 1 << 40)) == want[:64]
    dev = DeviceBuffer(len(want))
    assert bytes(pack_into(gpu, scene, dev)[0]) == bytes(info)
    same_snapshot(full_snapshot(gpu, scene), before)
    dev.release()
    scene.close()


# ---- round trip -----------------------------------------------------------------------------------------------------
def dirty(api, pkg, scene):
    """Leave something in every table of the destination that an unpack has to clear."""
    q = scene.params
    rng = np.random.default_rng(3)
    h = np.zeros(q.num_buckets + q.num_excess, pkg.HASH_ENTRY_DTYPE)
    h["ptr"] = -2
    h[1] = ((9, 9, 9), 0, 0, 0)
    h[q.num_buckets + q.num_excess - 1] = ((8, 8, 8), 0, 0, q.num_local_blocks - 1)
    api.upload_scene_state(scene, h, rng.permutation(q.num_local_blocks).astype(np.int32), 0,
                           rng.permutation(q.num_excess).astype(np.int32), 0)
    api.upload_voxel_blocks(scene, 0, rng.integers(0, 1 << 63, (q.num_local_blocks, 512), dtype=np.uint64).view(pkg.VOXEL_DTYPE))


@pytest.mark.parametrize("name", FIXTURES + ["two trips"])
def test_round_trip(gpu, pkg, cases, name):
    p, st, want = cases[name]
    n = ref_pack.header_fields(want)["blocks"]
    src = DeviceBuffer(len(want), want)
    out = DeviceBuffer(len(want))
    try:
        for N in dict.fromkeys((max(1, n), n + 7, p.num_local_blocks)):
            q = pf.scene_params(pkg, p.num_buckets, p.num_excess, N)
            scene = gpu.create_scene(q)
            dirty(gpu, pkg, scene)
            info = gpu.unpack_scene(scene, src.ptr, len(want))
            assert bytes(info) == want[:64]
            got, ref = full_snapshot(gpu, scene), ref_pack.unpack(want, q)
            rc.check_unpacked(got, ref)
            util.assert_same_state(got, ref, f"{name} into {N}", ignore_stats=("no_visible_entries",))
            assert np.array_equal(got["last_seen"], ref["last_seen"])
            util.check_invariants(got, q)
            assert pack_into(gpu, scene, out)[1] == want, "packing the unpacked scene gives other bytes"
            scene.close()
        assert split(src.read(), len(want)) == (want, True), "an unpack wrote to its source"
    finally:
        src.release(), out.release()


# ---- life after unpack ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_map(gpu, pkg, synth):
    """Three S-tiny frames: (workload, params, packed bytes of the map)."""
    wl = synth.s_tiny()
    params = util.small_params(pkg, wl)
    scene, rs, view = util.run_sequence(gpu, pkg, wl, params, 3)
    total = gpu.pack_scene(scene).total_bytes
    dev = DeviceBuffer(total)
    info, raw = pack_into(gpu, scene, dev)
    rc.check_packed(raw, ref_pack.state_of(util.snapshot(gpu, scene), params))
    dev.release()
    for h in (view, rs, scene):
        h.close()
    return wl, params, raw


def test_frames_after_an_unpack_equal_frames_on_the_reference_state(gpu, pkg, tiny_map):
    wl, params, raw = tiny_map
    n = ref_pack.header_fields(raw)["blocks"]
    assert n > 100
    q = util.small_params(pkg, wl, num_local_blocks=n + 64)
    src = DeviceBuffer(len(raw), raw)
    unpacked = gpu.create_scene(q)
    gpu.unpack_scene(unpacked, src.ptr, len(raw))
    twin = load(gpu, pkg, q, ref_pack.unpack(raw, q))
    sides = [(s, gpu.create_render_state(s, wl.W, wl.H), gpu.create_view(wl.W, wl.H)) for s in (unpacked, twin)]
    for i in range(3, 7):
        rgba, mm, M = wl.frame(i)
        got = []
        for scene, rs, view in sides:
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, M, wl.intr)
            if i == 5:
                gpu.decay(scene, rs, 1, 0, True)   # one decayed frame: walks alloc_bits, releases through the free lists
            img = gpu.get_image(scene, rs, M, wl.intr, pkg.IMAGE_DEPTH)
            snap = util.snapshot(gpu, scene, rs)
            snap["last_seen"] = gpu.download_last_seen(scene)
            got.append((snap, img, gpu.download_raycast_result(rs)))
        util.assert_same_state(got[0][0], got[1][0], f"frame {i}")
        assert np.array_equal(got[0][0]["last_seen"], got[1][0]["last_seen"]), i
        assert got[0][1].tobytes() == got[1][1].tobytes() and got[0][2].tobytes() == got[1][2].tobytes(), f"image of frame {i}"
        if i == 5:
            assert got[0][0]["stats"]["decayed_block_count"] > 0
    assert (got[0][1] > 0).sum() > 100
    src.release()
    for scene, rs, view in sides:
        for h in (view, rs, scene):
            h.close()


def test_a_render_after_an_unpack_is_the_new_maps(gpu, pkg, synth, tiny_map):
    wl, params, raw = tiny_map
    _, _, M = wl.frame(2)
    # another map: one frame only
    other, rs_o, view_o = util.run_sequence(gpu, pkg, wl, params, 1)
    scene = gpu.create_scene(params)
    rs = gpu.create_render_state(scene, wl.W, wl.H)
    src = DeviceBuffer(len(raw), raw)
    gpu.unpack_scene(scene, src.ptr, len(raw))
    first = gpu.get_image(scene, rs, M, wl.intr, pkg.IMAGE_DEPTH).copy()
    assert np.array_equal(first, gpu.get_image(scene, rs, M, wl.intr, pkg.IMAGE_DEPTH))   # (memoised or not: the same)
    total = gpu.pack_scene(other).total_bytes
    buf = DeviceBuffer(total)
    pack_into(gpu, other, buf)
    gpu.unpack_scene(scene, buf.ptr, total)
    second = gpu.get_image(scene, rs, M, wl.intr, pkg.IMAGE_DEPTH)
    want = gpu.get_image(other, rs_o, M, wl.intr, pkg.IMAGE_DEPTH)
    assert second.tobytes() == want.tobytes(), "the image after an unpack is not the new map's"
    assert second.tobytes() != first.tobytes()
    src.release(), buf.release()
    for h in (rs, scene, view_o, rs_o, other):
        h.close()


# ---- a pack behind work in flight -----------------------------------------------------------------------------------
def test_a_pack_sees_the_frame_enqueued_before_it(pkg, synth):
    wl = synth.s_tiny()
    with contextlib.ExitStack() as stack:   # handles go in reverse order, the engine last (any order is legal now)
        api = pkg.open_engine(0)
        stack.callback(api.close)
        scene = api.create_scene(util.small_params(pkg, wl))
        stack.callback(scene.close)
        rs = api.create_render_state(scene, wl.W, wl.H)
        stack.callback(rs.close)
        view = api.create_view(wl.W, wl.H)
        stack.callback(view.close)
        api.set_async(True)
        for i in range(2):
            rgba, mm, M = wl.frame(i)
            api.view_update(view, rgba, mm, timestamp=float(i))
            api.process_frame(scene, view, rs, M, wl.intr)
        total = api.pack_scene(scene).total_bytes      # (waits; the next frame is enqueued behind it)
        rgba, mm, M = wl.frame(2)
        api.view_update(view, rgba, mm, timestamp=2.0)
        api.process_frame(scene, view, rs, M, wl.intr)
        # the third frame allocates, so the size may have grown: room for it, then the pack right behind the frame
        buf = DeviceBuffer(2 * total)
        info = api.pack_scene(scene, buf.ptr, buf.nbytes)
        in_flight = buf.read()[GUARD:GUARD + info.total_bytes].tobytes()
        api.synchronize()
        buf2 = DeviceBuffer(info.total_bytes)
        info2, settled = pack_into(api, scene, buf2)
        assert info.total_bytes == info2.total_bytes and in_flight == settled
        api.set_async(False)
        rc.check_packed(settled, ref_pack.state_of(util.snapshot(api, scene), scene.params))
        buf.release(), buf2.release()


# ---- rejections -----------------------------------------------------------------------------------------------------
def test_pack_rejections_write_nothing(gpu, pkg, cases):
    p, st, want = cases["chains and releases"]
    scene = load(gpu, pkg, p, st)
    dev = DeviceBuffer(len(want))
    untouched = lambda: (dev.read() == GUARD_BYTE).all()
    # a buffer one byte short
    rejected(lambda: gpu.pack_scene(scene, dev.ptr, len(want) - 1))
    assert untouched()
    # a pageable pointer; one that is not 16-byte aligned
    pageable = np.full(len(want) + 64, GUARD_BYTE, np.uint8)
    ptr = (pageable.ctypes.data + 15) & ~15
    rejected(lambda: gpu.pack_scene(scene, ptr, len(want)))
    assert (pageable == GUARD_BYTE).all()
    rejected(lambda: gpu.pack_scene(scene, dev.ptr + 4, len(want)))
    assert untouched()
    # a swapping scene, a sharded scene, a shard range
    swapping = gpu.create_scene(pf.scene_params(pkg, 64, 64, 96, use_swapping=1))
    rejected(lambda: gpu.pack_scene(swapping, dev.ptr, len(want)))
    rejected(lambda: gpu.pack_scene(swapping))
    sharded = load(gpu, pkg, p, st)
    gpu.set_shard(sharded, 0, 2)
    rejected(lambda: gpu.pack_scene(sharded, dev.ptr, len(want)))
    ranged = load(gpu, pkg, p, st)
    gpu.set_shard_range(ranged, 0, 8)
    rejected(lambda: gpu.pack_scene(ranged, dev.ptr, len(want)))
    assert untouched()
    # another engine's scene
    with contextlib.ExitStack() as stack:
        other = pkg.open_engine(0)
        stack.callback(other.close)
        foreign = load(other, pkg, p, st)
        stack.callback(foreign.close)
        rejected(lambda: gpu.pack_scene(foreign, dev.ptr, len(want)))
        assert untouched()
        before = full_snapshot(other, foreign)
        src = DeviceBuffer(len(want), want)
        rejected(lambda: gpu.unpack_scene(foreign, src.ptr, len(want)))
        same_snapshot(full_snapshot(other, foreign), before)
        src.release()
    # ... and the scene packs as before
    assert pack_into(gpu, scene, dev)[1] == want
    dev.release()
    for h in (scene, swapping, sharded, ranged):
        h.close()


def corrupt(raw, at, value):
    bad = bytearray(raw)
    bad[at:at + 4] = np.int32(value).tobytes()
    return bad


def test_unpack_rejections_leave_the_scene_as_it_was(gpu, pkg, cases):
    p, st, want = cases["chains and releases"]
    hd = ref_pack.header_fields(want)
    n, f = hd["blocks"], hd["free_excess"]
    assert f > 0

    def refused(data, params=p, nbytes=None, like=None):
        """ref_pack.unpack refuses it, and so does the library, with the destination unchanged."""
        with pytest.raises(ref_pack.PackError):
            ref_pack.unpack(bytes(data)[:len(data) if nbytes is None else nbytes], params)
        scene = load(gpu, pkg, params, like) if like is not None else gpu.create_scene(params)
        before = full_snapshot(gpu, scene)
        src = DeviceBuffer(len(data), data)
        rejected(lambda: gpu.unpack_scene(scene, src.ptr, len(data) if nbytes is None else nbytes))
        same_snapshot(full_snapshot(gpu, scene), before)
        src.release()
        scene.close()

    # the eight of tests/test_pack_ref.py
    refused(want, pf.scene_params(pkg, p.num_buckets, p.num_excess, n - 1))
    refused(want, pf.scene_params(pkg, p.num_buckets * 2, p.num_excess, p.num_local_blocks))
    refused(want, pf.scene_params(pkg, p.num_buckets, p.num_excess, p.num_local_blocks,
                                  mu=float(np.nextafter(np.float32(p.mu), np.float32(1)))))
    refused(want, nbytes=len(want) - 1, like=st)
    refused(corrupt(want, 64 + 12, p.num_buckets + p.num_excess), like=st)
    swapped = bytearray(want)
    swapped[64:80], swapped[80:96] = want[80:96], want[64:80]
    refused(swapped, like=st)
    refused(corrupt(want, 64 + 8, p.num_excess + 1), like=st)
    refused(corrupt(want, 64 + 16 * n, p.num_excess), like=st)
    # a negative record index; a pageable source; a header that is none
    refused(corrupt(want, 64 + 12, -1), like=st)
    scene = load(gpu, pkg, p, st)
    before = full_snapshot(gpu, scene)
    pageable = np.frombuffer(bytearray(want) + bytearray(32), np.uint8)
    rejected(lambda: gpu.unpack_scene(scene, (pageable.ctypes.data + 15) & ~15, len(want)))
    src = DeviceBuffer(len(want), b"DSPX" + want[4:])
    rejected(lambda: gpu.unpack_scene(scene, src.ptr, len(want)))
    same_snapshot(full_snapshot(gpu, scene), before)
    # ... and the image itself is taken
    good = DeviceBuffer(len(want), want)
    gpu.unpack_scene(scene, good.ptr, len(want))
    rc.check_unpacked(full_snapshot(gpu, scene), ref_pack.unpack(want, p))
    src.release(), good.release()
    scene.close()


def test_unpack_validates_the_last_record_and_the_last_free_value(gpu, pkg, cases):
    """The tail lanes of the validation kernel: 585 records are two full workgroups and 73 lanes of a third."""
    p, st, want = cases["two trips"]
    hd = ref_pack.header_fields(want)
    n, f = hd["blocks"], hd["free_excess"]
    assert n == 585 and f == 16
    scene = gpu.create_scene(p)
    before = full_snapshot(gpu, scene)
    for bad in (corrupt(want, 64 + 16 * (n - 1) + 12, p.num_buckets + p.num_excess),   # last index: past the table
                corrupt(want, 64 + 16 * (n - 1) + 12, 0),                               # ... not ascending
                corrupt(want, 64 + 16 * (n - 1) + 8, -1),                               # last offset
                corrupt(want, 64 + 16 * n + 4 * (f - 1), -1)):                          # last free value
        with pytest.raises(ref_pack.PackError):
            ref_pack.unpack(bytes(bad), p)
        src = DeviceBuffer(len(bad), bad)
        rejected(lambda: gpu.unpack_scene(scene, src.ptr, len(bad)))
        src.release()
        same_snapshot(full_snapshot(gpu, scene), before)
    scene.close()


# ---- the mirror -----------------------------------------------------------------------------------------------------
def test_mirror_compact_local_map(pkg, gpu, synth, tmp_path):
    """pack_harness: ITMMainEngine::CompactLocalMap on two S-tiny maps, one after the other.  The compacted map 0 is
    ref_pack.unpack of the map before, into n + headroom blocks; its render before and after is bit-identical, and so is
    GetImageAllLocalMaps of both maps after each compaction (pools then differ); the map takes another keyframe."""
    import os
    import struct
    import subprocess
    harness = os.path.join(os.path.dirname(pkg.CSRC_DIR), "itmlib", "tests", "pack_harness")
    wl = synth.s_tiny(80, 60)
    p = util.small_params(pkg, wl)
    n_frames, headroom = 4, 64
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n_frames))
        for i in range(n_frames):
            rgba, mm, M = wl.frame(2 * i)
            f.write(rgba.tobytes()); f.write(mm.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        f.write(struct.pack("<i", headroom))
    run = subprocess.run([harness, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    info = pkg.PackInfo.from_buffer_copy(raw[:64])
    pool, = struct.unpack_from("<i", raw, 64)
    at, npix = 68, wl.W * wl.H
    depth_before = np.frombuffer(raw, np.float32, npix, at); at += 4 * npix
    depth_after = np.frombuffer(raw, np.float32, npix, at); at += 4 * npix
    all_before, all_after, all_after_both = (np.frombuffer(raw, np.float32, npix, at + 4 * npix * k) for k in range(3))
    at += 12 * npix
    n_entries = p.num_buckets + p.num_excess

    def read_map(at, n_local, with_last_seen):
        lf, lx = struct.unpack_from("<2i", raw, at); at += 8
        out = dict(hash=np.frombuffer(raw, pkg.HASH_ENTRY_DTYPE, n_entries, at)); at += 16 * n_entries
        out["alloc_list"] = np.frombuffer(raw, np.int32, n_local, at); at += 4 * n_local
        out["excess_list"] = np.frombuffer(raw, np.int32, p.num_excess, at); at += 4 * p.num_excess
        out["voxels"] = np.frombuffer(raw, np.uint64, n_local * 512, at).reshape(n_local, 512); at += 4096 * n_local
        if with_last_seen:
            out["last_seen"] = np.frombuffer(raw, np.int32, n_local, at); at += 4 * n_local
        out["last_free_block_id"], out["last_free_excess_id"] = lf, lx
        out["stats"] = dict(last_free_block_id=lf, last_free_excess_id=lx, decayed_block_count=0, slid_block_count=0,
                            frame_counter=0, fusion_fifo_len=0, defusion_fifo_len=0, alloc_failures=0)
        return out, at

    before, at = read_map(at, p.num_local_blocks, False)
    after, at = read_map(at, pool, True)
    no_visible, last_free_later = struct.unpack_from("<2i", raw, at); at += 8
    assert at == len(raw)
    before["params"] = ref_pack.geometry(p)
    image = ref_pack.pack(before)
    n = int((before["hash"]["ptr"] >= 0).sum())
    assert n > 100 and info.blocks == n and pool == n + headroom and bytes(info) == image[:64]
    q = util.small_params(pkg, wl, num_local_blocks=pool)
    want = ref_pack.unpack(image, q)
    for check in rc.UNPACK_CHECKS:
        if check is not rc.check_reset_stats:    # (the harness dumps the two stack pointers, not the rings' counters)
            check(after, want)
    util.check_invariants(after, q)
    assert depth_before.tobytes() == depth_after.tobytes() and (depth_before > 0).sum() > 100
    assert no_visible > 0 and last_free_later <= after["last_free_block_id"]
    # both maps in one image: a compacted map next to one with the settings' pool, then two compacted maps of different pools
    assert all_before.tobytes() == all_after.tobytes() == all_after_both.tobytes()
    assert (all_before > 0).sum() > 100


def test_device_alloc_holds_a_packed_map(gpu, pkg, cases):
    """dslam_device_alloc / dslam_device_free: memory a pack writes and an unpack reads."""
    p, st, want = cases["chains and releases"]
    scene = load(gpu, pkg, p, st)
    ptr = gpu.device_alloc(len(want))
    assert ptr and ptr % 256 == 0
    try:
        assert bytes(gpu.pack_scene(scene, ptr, len(want))) == want[:64]
        q = pf.scene_params(pkg, p.num_buckets, p.num_excess, ref_pack.header_fields(want)["blocks"] + 7)
        back = gpu.create_scene(q)
        gpu.unpack_scene(back, ptr, len(want))
        rc.check_unpacked(full_snapshot(gpu, back), ref_pack.unpack(want, q))
        back.close()
    finally:
        gpu.device_free(ptr)
    gpu.device_free(None)
    rejected(lambda: gpu.device_alloc(0))
    scene.close()
