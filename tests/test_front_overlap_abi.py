"""Without a GPU: dslam_debug_front_overlap_counts is declared, exported and bound; and the shapes the GPU tests of the front
end on the auxiliary stream run at (front_overlap_fixtures.py) have what the selection's hidden-entry path exists for, shown
on the oracle: entries a pass creates -- bucket heads and excess entries both -- that the GetImage at the same pose lists."""
import os
import re

import numpy as np
import front_overlap_fixtures as ffx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "dslam_debug_front_overlap_counts"


def test_the_call_is_declared_exported_and_bound(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dslam_fusion.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + CALL + r"\s*\(\s*dslam_engine\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*\)", txt)
    assert CALL in pkg.exported_symbols()
    assert callable(getattr(pkg.CApi, "debug_front_overlap_counts", None))


def _listed_new(ref, i):
    """(new bucket entries, new excess entries) of pass i that the GetImage at the same pose lists"""
    before, after = ref[i]["hash_before"], ref[i]["snap"]["hash"]
    new = np.flatnonzero((before["ptr"] < 0) & (after["ptr"] >= 0))
    listed = np.intersect1d(new, ref[i]["visible"])
    nb = ffx.TABLE["num_buckets"]
    return int((listed < nb).sum()), int((listed >= nb).sum())


def test_the_passes_that_overlap_create_listed_entries_of_both_kinds(pkg, synth, oracle):
    """A pass that can overlap (every one after the first) leaves entries whose table stores wait for k_publish_entries while
    the selection already runs, and the selection must list them.  Every such pass of the sequence creates at least one
    entry that the GetImage at its pose lists.  Both kinds in EVERY pass is more than 12 consecutive frames of s_tiny can
    give at any table size: frames 6 and 7 bring one new block each into view (on tables of 0x400 to 0x4000 buckets alike).
    With 0x800 buckets the passes that create two entries or more have both kinds but for one, and the single-entry passes
    cover a bucket entry alone (6, 7) and an excess entry alone (10)."""
    ref = ffx.oracle_reference(oracle, pkg, synth, "roomy")
    kinds = [_listed_new(ref, i) for i in range(1, ffx.M)]
    assert all(b + x >= 1 for b, x in kinds), kinds
    assert sum(b >= 1 and x >= 1 for b, x in kinds) > (ffx.M - 1) // 2, kinds
    assert any(b >= 1 and x == 0 for b, x in kinds) and any(b == 0 and x >= 1 for b, x in kinds), kinds
    assert all(r["snap"]["stats"]["alloc_failures"] == 0 for r in ref)


def test_the_small_pool_runs_dry_in_a_pass_that_overlaps(pkg, synth, oracle):
    ref = ffx.oracle_reference(oracle, pkg, synth, "dry")
    st = [r["snap"]["stats"] for r in ref]
    dry = next(i for i, s in enumerate(st) if s["alloc_failures"] > 0)
    assert dry >= 2, "the pass that runs dry must be one that can overlap, with an overlapped pass in front of it"
    b, x = _listed_new(ref, dry)
    assert b >= 1 and x >= 1, "the pass that runs dry still creates listed entries of both kinds"
    assert all(s["last_free_block_id"] == -1 for s in st[dry:])
