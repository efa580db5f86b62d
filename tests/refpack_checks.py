"""The check bodies of the packed-map tests: functions that take bytes or snapshots and assert, section by section, against
tests/ref_pack.py.  The GPU tests (test_gpu_pack.py) feed them what the library produced; test_pack_checks_ref.py feeds
them the reference's own output with one defect each, which shows that every check can fail -- without a wrong kernel.
Everything compared is an integer or a byte: no tolerance anywhere."""
import numpy as np

import ref_pack
from refmap import HASH_ENTRY_DTYPE


def _u64(vox):
    return np.ascontiguousarray(vox).view(np.uint64).reshape(-1, 512)


def _sections(raw):
    hd = ref_pack.header_fields(raw)
    n, f = hd["blocks"], hd["free_excess"]
    return hd, n, f, 64 + 16 * n, 64 + 16 * n + 4 * f


# ---- a packed image against the state it was packed from ------------------------------------------------------------------
def check_header(raw, state):
    want = ref_pack.header_fields(ref_pack.pack(state))
    got = ref_pack.header_fields(raw)          # (raises for a header that is none)
    for k in want:
        assert got[k] == want[k], f"header field {k}: {got[k]} != {want[k]}"
    assert bytes(raw[:64]) == ref_pack.pack(state)[:64], "header bytes differ"


def check_records(raw, state):
    hd, n, f, rec_end, _ = _sections(raw)
    h = np.asarray(state["hash"])
    ranks = np.nonzero(h["ptr"] >= 0)[0]
    assert n == len(ranks), f"{n} records for {len(ranks)} resident entries"
    rec = np.frombuffer(bytes(raw), HASH_ENTRY_DTYPE, n, 64)
    assert np.array_equal(rec["ptr"], ranks), "record ptr is not the resident entries' hash indices, ascending"
    assert np.array_equal(rec["pos"], h["pos"][ranks]) and np.array_equal(rec["offset"], h["offset"][ranks]), "record pos / offset"
    assert (rec["_pad"] == 0).all(), "record _pad"


def check_free_list(raw, state):
    hd, n, f, rec_end, free_end = _sections(raw)
    assert f == int(state["last_free_excess_id"]) + 1
    free = np.frombuffer(bytes(raw), "<i4", f, rec_end)
    assert np.array_equal(free, np.asarray(state["excess_list"])[:f]), "the free excess list is not carried verbatim"


def check_padding(raw, state):
    hd, n, f, rec_end, free_end = _sections(raw)
    assert bytes(raw[free_end:hd["blocks_offset"]]) == bytes(hd["blocks_offset"] - free_end), "padding is not zero"


def check_blocks(raw, state):
    hd, n, f, _, _ = _sections(raw)
    h = np.asarray(state["hash"])
    ranks = np.nonzero(h["ptr"] >= 0)[0]
    assert len(raw) >= hd["total_bytes"]
    got = np.frombuffer(bytes(raw), "<u8", 512 * n, hd["blocks_offset"]).reshape(n, 512)
    want = _u64(state["voxels"])[h["ptr"][ranks]]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} packed blocks differ from the pool's, first at rank {bad[0]}"


PACK_CHECKS = (check_header, check_records, check_free_list, check_padding, check_blocks)


def check_packed(raw, state):
    """Every section, then the whole image byte for byte."""
    for check in PACK_CHECKS:
        check(raw, state)
    want = ref_pack.pack(state)
    assert len(raw) == len(want) and bytes(raw) == want, "packed bytes differ from the reference"


# ---- an unpacked scene against the image it was unpacked from -------------------------------------------------------------
# `got`: hash, voxels, alloc_list, excess_list, last_seen, stats (a util.snapshot plus last_seen); `want`: ref_pack.unpack's.
def check_table(got, want):
    a, b = np.asarray(got["hash"]), np.asarray(want["hash"])
    for field in ("pos", "offset", "ptr"):
        bad = np.nonzero(a[field] != b[field])[0] if field != "pos" else np.nonzero((a[field] != b[field]).any(axis=1))[0]
        assert len(bad) == 0, f"hash table: {len(bad)} entries differ in {field}, first entry {bad[0]}: {a[bad[0]]} vs {b[bad[0]]}"


def check_free_blocks(got, want):
    lf = int(want["stats"]["last_free_block_id"])
    assert int(got["stats"]["last_free_block_id"]) == lf, "last_free_block_id"
    assert np.array_equal(np.asarray(got["alloc_list"])[:lf + 1], np.asarray(want["alloc_list"])[:lf + 1]), "voxel free list"


def check_free_excess(got, want):
    lx = int(want["stats"]["last_free_excess_id"])
    assert int(got["stats"]["last_free_excess_id"]) == lx, "last_free_excess_id"
    assert np.array_equal(np.asarray(got["excess_list"]), np.asarray(want["excess_list"])), "excess list (free part and the rest)"


def check_last_seen(got, want):
    assert np.array_equal(np.asarray(got["last_seen"]), np.asarray(want["last_seen"])), "last_seen is not a reset's"


def check_reset_stats(got, want):
    for k in ("decayed_block_count", "slid_block_count", "frame_counter", "fusion_fifo_len", "defusion_fifo_len", "alloc_failures"):
        assert int(got["stats"][k]) == int(want["stats"][k]), f"stats[{k}]"


def check_live_slots(got, want):
    slots = np.asarray(want["hash"])["ptr"]
    slots = slots[slots >= 0]
    a, b = _u64(got["voxels"]), _u64(want["voxels"])
    bad = [int(s) for s in slots if not np.array_equal(a[s], b[s])]
    assert not bad, f"{len(bad)} live slots differ, first slot {bad[0]}"


def check_unused_slots(got, want):
    slots = np.asarray(want["hash"])["ptr"]
    unused = np.setdiff1d(np.arange(len(_u64(want["voxels"]))), slots[slots >= 0])
    bad = unused[(_u64(got["voxels"])[unused] != ref_pack.EMPTY_VOXEL).any(axis=1)]
    assert len(bad) == 0, f"{len(bad)} unused slots are not empty, first slot {bad[0]}"


UNPACK_CHECKS = (check_table, check_free_blocks, check_free_excess, check_last_seen, check_reset_stats, check_live_slots,
                 check_unused_slots)


def check_unpacked(got, want):
    for check in UNPACK_CHECKS:
        check(got, want)


def failing(checks, *args):
    """The names of the checks that fail on the arguments."""
    out = []
    for check in checks:
        try:
            check(*args)
        except (AssertionError, ref_pack.PackError):
            out.append(check.__name__)
    return out
