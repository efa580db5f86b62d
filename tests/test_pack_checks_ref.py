"""The packed-map checks are sensitive (no GPU): the check bodies of refpack_checks.py pass on the reference's own output
and each of ten single defects -- what a wrong kernel would produce -- fails the check named for it.  This stands in for
running deliberately wrong kernels on a device."""
import struct

import numpy as np
import pytest

import pack_fixtures as pf
import ref_pack
import refpack_checks as rc
from refmap import HASH_ENTRY_DTYPE


@pytest.fixture(scope="module")
def case(pkg):
    """The chained fixture state, its image, and its unpacked state in a pool with headroom."""
    p, st = pf.chained_state(pkg)
    raw = ref_pack.pack(st)
    hd = ref_pack.header_fields(raw)
    q = pf.scene_params(pkg, p.num_buckets, p.num_excess, hd["blocks"] + 7)
    return st, raw, hd, q


def fresh(raw, q):
    return ref_pack.unpack(raw, q)


def test_the_checks_pass_on_the_reference(pkg, case):
    st, raw, hd, q = case
    rc.check_packed(raw, st)
    rc.check_packed(np.frombuffer(raw, np.uint8), st)
    rc.check_unpacked(fresh(raw, q), fresh(raw, q))
    for name, p, state in pf.states(pkg):
        rc.check_packed(ref_pack.pack(state), state)
    assert hd["blocks"] >= 20 and hd["free_excess"] >= 4 and hd["blocks_offset"] > 64 + 16 * hd["blocks"] + 4 * hd["free_excess"]


# ---- defects of a packed image ------------------------------------------------------------------------------------------
def bbox_max_taken_with_min(raw, st, hd):
    out = bytearray(raw)
    out[54:60] = struct.pack("<3h", *hd["bbox_min"])
    return out


def nonzero_padding_byte(raw, st, hd):
    out = bytearray(raw)
    out[hd["blocks_offset"] - 1] = 1
    return out


def two_records_swapped(raw, st, hd):
    out = bytearray(raw)
    out[64 + 16 * 3:64 + 16 * 4], out[64 + 16 * 4:64 + 16 * 5] = raw[64 + 16 * 4:64 + 16 * 5], raw[64 + 16 * 3:64 + 16 * 4]
    return out


def ptr_left_as_the_pool_slot(raw, st, hd):
    out = bytearray(raw)
    rec = np.frombuffer(raw, HASH_ENTRY_DTYPE, hd["blocks"], 64).copy()
    rec["ptr"] = st["hash"]["ptr"][rec["ptr"]]
    out[64:64 + 16 * hd["blocks"]] = rec.tobytes()
    return out


def free_list_reversed(raw, st, hd):
    out = bytearray(raw)
    a, f = 64 + 16 * hd["blocks"], hd["free_excess"]
    out[a:a + 4 * f] = np.frombuffer(raw, "<i4", f, a)[::-1].tobytes()
    return out


def blocks_in_slot_order(raw, st, hd):
    out = bytearray(raw)
    h = st["hash"]
    slots = np.sort(h["ptr"][h["ptr"] >= 0])
    out[hd["blocks_offset"]:] = np.ascontiguousarray(st["voxels"]).view(np.uint64).reshape(-1, 512)[slots].tobytes()
    return out


PACK_DEFECTS = [(bbox_max_taken_with_min, "check_header"), (nonzero_padding_byte, "check_padding"),
                (two_records_swapped, "check_records"), (ptr_left_as_the_pool_slot, "check_records"),
                (free_list_reversed, "check_free_list"), (blocks_in_slot_order, "check_blocks")]


@pytest.mark.parametrize("defect,check", PACK_DEFECTS, ids=[d.__name__ for d, _ in PACK_DEFECTS])
def test_a_defective_image_fails_its_check(case, defect, check):
    st, raw, hd, q = case
    bad = defect(raw, st, hd)
    assert len(bad) == len(raw) and bytes(bad) != raw, "the defect changed nothing"
    assert rc.failing(rc.PACK_CHECKS, bad, st) == [check]
    with pytest.raises(AssertionError):
        rc.check_packed(bad, st)


# ---- defects of an unpacked state ---------------------------------------------------------------------------------------
def ptr_counts_up(got, n, N):
    h = got["hash"]
    idx = np.nonzero(h["ptr"] >= 0)[0]
    h["ptr"][idx] = np.arange(n)   # ptr = k instead of N-1-k


def last_free_block_id_off_by_one(got, n, N):
    got["stats"]["last_free_block_id"] += 1
    got["last_free_block_id"] += 1


def stale_last_seen(got, n, N):
    got["last_seen"][N - 1] = 3


def unused_slot_not_empty(got, n, N):
    got["voxels"][0, 17] = np.uint64(0x0001000000007FFE)


UNPACK_DEFECTS = [(ptr_counts_up, "check_table"), (last_free_block_id_off_by_one, "check_free_blocks"),
                  (stale_last_seen, "check_last_seen"), (unused_slot_not_empty, "check_unused_slots")]


@pytest.mark.parametrize("defect,check", UNPACK_DEFECTS, ids=[d.__name__ for d, _ in UNPACK_DEFECTS])
def test_a_defective_state_fails_its_check(case, defect, check):
    st, raw, hd, q = case
    got, want = fresh(raw, q), fresh(raw, q)
    defect(got, hd["blocks"], q.num_local_blocks)
    assert rc.failing(rc.UNPACK_CHECKS, got, want) == [check]
    with pytest.raises(AssertionError):
        rc.check_unpacked(got, want)
