"""The packed-map law without a GPU: the numpy restatement (ref_pack.py) round-trips states driven
through refmap.MapModel and states its layout, header and rejections; the library's two host-only functions,
dslam_pack_layout and dslam_pack_header_read, equal it.  (The device calls are not in the library: section 21 says why.)"""
import ctypes

import numpy as np
import pytest

import pack_fixtures as pf
import ref_pack
import util


def test_fixture_states_reach_what_they_claim(pkg):
    by = {name: st for name, _, st in pf.states(pkg)}
    assert by["excess stack empty"]["last_free_excess_id"] == -1
    assert by["excess stack full"]["last_free_excess_id"] == 15
    st = by["chains and releases"]
    stack = ref_pack.free_excess_stack(st)
    assert stack != sorted(stack) and stack != sorted(stack, reverse=True), "the releases left the stack in order"
    pos = st["hash"]["pos"][st["hash"]["ptr"] >= 0]
    assert pos.min() == -32767 and pos.max() == 32767
    assert (st["hash"]["offset"][st["hash"]["ptr"] >= 0] > 0).sum() >= 10


@pytest.mark.parametrize("headroom", [0, 7, None])
def test_round_trip(pkg, headroom):
    for name, p, st in pf.states(pkg):
        util.check_invariants(st, p)
        raw = ref_pack.pack(st)
        n = int((st["hash"]["ptr"] >= 0).sum())
        hd = ref_pack.header_fields(raw)
        assert hd["blocks"] == n and len(raw) == hd["total_bytes"], name
        # a pool as large as the map needs, one with headroom, the source's own
        N = p.num_local_blocks if headroom is None else max(1, n + headroom)
        q = pf.scene_params(pkg, p.num_buckets, p.num_excess, N)
        back = ref_pack.unpack(raw, q)
        util.check_invariants(back, q)
        assert back["last_free_block_id"] == N - 1 - n, name
        assert ref_pack.as_function(back) == ref_pack.as_function(st), name
        assert ref_pack.free_excess_stack(back) == ref_pack.free_excess_stack(st), name
        # entries keep their indices: the tables differ in ptr alone
        for field in ("pos", "offset"):
            assert np.array_equal(back["hash"][field], st["hash"][field]), name
        assert np.array_equal(back["hash"]["ptr"] >= 0, st["hash"]["ptr"] >= 0), name
        # a fixed point, byte for byte
        raw2 = ref_pack.pack(back)
        assert raw2 == raw, name
        again = ref_pack.unpack(raw2, q)
        for k in ("hash", "voxels", "alloc_list", "excess_list", "last_seen"):
            assert np.array_equal(again[k], back[k]), (name, k)


def test_layout_of_the_image(pkg):
    p, st = pf.chained_state(pkg)
    raw = ref_pack.pack(st)
    hd = ref_pack.header_fields(raw)
    n, f = hd["blocks"], hd["free_excess"]
    assert raw[:4] == b"DSPK" and f == st["last_free_excess_id"] + 1
    rec = np.frombuffer(raw, ref_pack.HASH_ENTRY_DTYPE, n, 64)
    assert (np.diff(rec["ptr"]) > 0).all() and (rec["_pad"] == 0).all()
    assert np.array_equal(rec["ptr"], np.nonzero(st["hash"]["ptr"] >= 0)[0])
    end = 64 + 16 * n + 4 * f
    assert hd["blocks_offset"] % 4096 == 0 and 0 <= hd["blocks_offset"] - end < 4096
    assert raw[end:hd["blocks_offset"]] == bytes(hd["blocks_offset"] - end)
    pos = st["hash"]["pos"][st["hash"]["ptr"] >= 0].astype(int)
    assert hd["bbox_min"] == pos.min(axis=0).tolist() and hd["bbox_max"] == pos.max(axis=0).tolist()
    assert hd["bbox_min"][0] == -32767 and hd["bbox_max"][2] == 32767
    empty = ref_pack.header_fields(ref_pack.pack(pf.build(p, [])))
    assert empty["bbox_min"] == [32767] * 3 and empty["bbox_max"] == [-32768] * 3 and empty["total_bytes"] == 4096


def test_unpack_rejections(pkg):
    p, st = pf.chained_state(pkg)
    raw = bytearray(ref_pack.pack(st))
    n = ref_pack.header_fields(raw)["blocks"]
    f = ref_pack.header_fields(raw)["free_excess"]

    def rejected(data, params=p):
        with pytest.raises(ref_pack.PackError):
            ref_pack.unpack(bytes(data), params)

    rejected(raw, pf.scene_params(pkg, p.num_buckets, p.num_excess, n - 1))
    rejected(raw, pf.scene_params(pkg, p.num_buckets * 2, p.num_excess, p.num_local_blocks))
    rejected(raw, pf.scene_params(pkg, p.num_buckets, p.num_excess, p.num_local_blocks, mu=float(np.nextafter(np.float32(p.mu), np.float32(1)))))
    rejected(raw[:-1])
    bad = bytearray(raw); bad[64 + 12:64 + 16] = np.int32(p.num_buckets + p.num_excess).tobytes(); rejected(bad)
    bad = bytearray(raw); bad[64:80], bad[80:96] = raw[80:96], raw[64:80]; rejected(bad)
    bad = bytearray(raw); bad[64 + 8:64 + 12] = np.int32(p.num_excess + 1).tobytes(); rejected(bad)
    bad = bytearray(raw); bad[64 + 16 * n:64 + 16 * n + 4] = np.int32(p.num_excess).tobytes(); rejected(bad)
    assert f > 0
    ref_pack.unpack(bytes(raw), p)


# ---- the layout and the header ---------------------------------------------------------------------------------------------
def sweep():
    """(n, f): zero, values where 64 + 16 n + 4 f is an exact multiple of 4096, their neighbours either side (the section
    grows by whole words, so the nearest sizes are 4 bytes away), seeded random ones and the largest counts."""
    cases = [(0, 0), (1, 0), (0, 1), (252, 0), (0, 1008), (251, 4), (100, 608)]   # 4096 exactly: 64 + 16 n + 4 f = 4096
    cases += [(252, 1), (251, 3), (251, 5), (0, 1007), (0, 1009), (508, 0), (507, 4), (507, 3), (507, 5)]
    rng = np.random.default_rng(21)
    cases += [(int(a), int(b)) for a, b in zip(rng.integers(0, 1 << 20, 200), rng.integers(0, 1 << 20, 200))]
    cases += [(0x7fffffff, 0x7fffffff), (0x40000, 0x20000)]
    return cases


def test_layout_is_the_smallest_4096_multiple_that_holds_the_sections():
    exact = 0
    for n, f in sweep():
        off, total = ref_pack.layout(n, f)
        end = 64 + 16 * n + 4 * f
        assert off % 4096 == 0 and end <= off < end + 4096 and total == off + 4096 * n, (n, f)
        exact += off == end
    assert exact >= 5


def make_header(blocks, free, nb=1 << 20, nx=1 << 20, **over):
    off, total = ref_pack.layout(blocks, free)
    v = dict(magic=b"DSPK", version=1, nb=nb, nx=nx, n=blocks, f=free, vs=ref_pack.f32_bits(0.005), mu=ref_pack.f32_bits(0.02), off=off,
             total=total, lo=(-3, -2, -1), hi=(4, 5, 6), zero=0)
    v.update(over)
    return ref_pack.HEADER.pack(v["magic"], v["version"], v["nb"], v["nx"], v["n"], v["f"], v["vs"], v["mu"], v["off"], v["total"],
                                *v["lo"], *v["hi"], v["zero"])


def test_header_fields_at_the_offsets_the_law_states():
    raw = make_header(1000, 80)
    hd = ref_pack.header_fields(raw)
    assert raw[:4] == b"DSPK" and np.frombuffer(raw, "<u4", 1, 4)[0] == 1
    assert np.frombuffer(raw, "<i4", 4, 8).tolist() == [1 << 20, 1 << 20, 1000, 80]
    assert np.frombuffer(raw, "<u4", 2, 24).tolist() == [hd["voxel_size_bits"], hd["mu_bits"]]
    assert np.frombuffer(raw, "<i8", 2, 32).tolist() == [hd["blocks_offset"], hd["total_bytes"]]
    assert np.frombuffer(raw, "<i2", 6, 48).tolist() == [-3, -2, -1, 4, 5, 6] and np.frombuffer(raw, "<u4", 1, 60)[0] == 0


def test_a_header_with_one_field_corrupted_is_rejected():
    n, f = 1000, 80   # (the free list ends on a 4096 boundary: one more value moves the blocks)
    off, total = ref_pack.layout(n, f)
    assert off == 64 + 16 * n + 4 * f
    for over in (dict(magic=b"DSPX"), dict(magic=b"dSPK"), dict(version=0), dict(version=2), dict(nb=-1), dict(nx=-1), dict(nx=f - 1),
                 dict(n=-1), dict(n=n + 1), dict(n=n - 1), dict(f=-1), dict(f=f + 1), dict(off=off + 4096), dict(off=off - 1),
                 dict(total=total + 1), dict(total=total - 4096), dict(zero=1)):
        with pytest.raises(ref_pack.PackError):
            ref_pack.header_fields(make_header(n, f, **over))
    ref_pack.header_fields(make_header(n, f))


# ---- the library's host-only functions ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(pkg):
    return ctypes.CDLL(pkg.LIB_PATH)


def test_pack_layout_equals_the_reference(lib):
    off, total = ctypes.c_int64(-1), ctypes.c_int64(-1)
    for n, f in sweep():
        assert lib.dslam_pack_layout(ctypes.c_int32(n), ctypes.c_int32(f), ctypes.byref(off), ctypes.byref(total)) == 0
        assert (off.value, total.value) == ref_pack.layout(n, f), (n, f)
    off.value = total.value = -7
    for n, f in ((-1, 0), (0, -1), (-0x80000000, -0x80000000)):
        assert lib.dslam_pack_layout(ctypes.c_int32(n), ctypes.c_int32(f), ctypes.byref(off), ctypes.byref(total)) < 0
    assert lib.dslam_pack_layout(ctypes.c_int32(1), ctypes.c_int32(1), None, ctypes.byref(total)) < 0
    assert lib.dslam_pack_layout(ctypes.c_int32(1), ctypes.c_int32(1), ctypes.byref(off), None) < 0
    assert (off.value, total.value) == (-7, -7)


def read_header(pkg, lib, raw):
    """(return code, the PackInfo, whether it still holds the sentinel it was filled with)."""
    info = pkg.PackInfo()
    sentinel = bytes([0xA5]) * 64
    ctypes.memmove(ctypes.byref(info), sentinel, 64)
    rc = lib.dslam_pack_header_read(ctypes.c_char_p(raw), ctypes.byref(info))
    return rc, info, bytes(info) == sentinel


def test_pack_header_read_equals_the_reference(pkg, lib):
    for n, f in sweep():
        if f > 1 << 20:   # (f <= num_excess)
            continue
        raw = make_header(n, f)
        rc, info, untouched = read_header(pkg, lib, raw)
        assert rc == 0 and not untouched and bytes(info) == raw, (n, f)
        got = info.as_dict()
        for k, v in ref_pack.header_fields(raw).items():
            assert got[k] == v, (n, f, k)
        assert info.magic == b"DSPK" and info.version == 1 and info.reserved == 0
    # ... and the header of a packed state, read where it lies (an odd address)
    p, st = pf.chained_state(pkg)
    raw = ref_pack.pack(st)
    shifted = ctypes.create_string_buffer(b"x" + raw[:64])
    info = pkg.PackInfo()
    assert lib.dslam_pack_header_read(ctypes.byref(shifted, 1), ctypes.byref(info)) == 0
    assert info.as_dict()["bbox_min"] == ref_pack.header_fields(raw)["bbox_min"] and info.total_bytes == len(raw)


def test_the_library_rejects_a_header_with_one_field_corrupted_and_leaves_out_untouched(pkg, lib):
    n, f = 1000, 80
    off, total = ref_pack.layout(n, f)
    for over in (dict(magic=b"DSPX"), dict(magic=b"dSPK"), dict(version=0), dict(version=2), dict(nb=-1), dict(nx=-1), dict(nx=f - 1),
                 dict(n=-1), dict(n=n + 1), dict(n=n - 1), dict(f=-1), dict(f=f + 1), dict(off=off + 4096), dict(off=off - 1),
                 dict(total=total + 1), dict(total=total - 4096), dict(zero=1)):
        rc, _, untouched = read_header(pkg, lib, make_header(n, f, **over))
        assert rc < 0 and untouched, over
    info = pkg.PackInfo()
    assert lib.dslam_pack_header_read(None, ctypes.byref(info)) < 0
    assert lib.dslam_pack_header_read(ctypes.c_char_p(make_header(n, f)), None) < 0
    # the fields the function does not judge pass through: parameters and the bounding box are the caller's to compare
    rc, info, _ = read_header(pkg, lib, make_header(n, f, vs=0, mu=0xFFFFFFFF, lo=(9, 9, 9), hi=(-9, -9, -9)))
    assert rc == 0 and info.mu_bits == 0xFFFFFFFF and list(info.bbox_min) == [9, 9, 9]
