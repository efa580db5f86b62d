"""Without a GPU: dslam_debug_sweep_overlap_counts is declared, exported and bound; and the shapes the GPU tests of the
overlapped sweep run at (sweep_overlap_fixtures.py) do what they are chosen for, shown on the oracle."""
import os
import re

import sweep_overlap_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "dslam_debug_sweep_overlap_counts"


def test_the_call_is_declared_exported_and_bound(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dslam_fusion.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + CALL + r"\s*\(\s*dslam_engine\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*\)", txt)
    assert CALL in pkg.exported_symbols()
    assert callable(getattr(pkg.CApi, "debug_sweep_overlap_counts", None))


def test_every_pass_after_the_first_has_excess_requests(pkg, synth, oracle):
    """A type-2 request needs an occupied bucket, so the first pass on an empty table has none; every later pass -- every pass
    that can overlap -- takes at least one slot off the excess list and one voxel block with it."""
    _, snaps = fx.oracle_reference(oracle, pkg, synth, "roomy")
    ex = [s["stats"]["last_free_excess_id"] for s in snaps]
    blocks = [s["stats"]["last_free_block_id"] for s in snaps]
    assert all(b < a for a, b in zip(ex, ex[1:])), ex
    assert all(s["stats"]["alloc_failures"] == 0 for s in snaps) and blocks[-1] > 0
    # ... and bucket heads are still being filled in overlapped passes (type-1 requests): more blocks go than excess slots
    assert sum((blocks[i] - blocks[i + 1]) > (ex[i] - ex[i + 1]) for i in range(fx.M - 1)) >= 3


def test_the_small_pool_runs_dry_in_the_middle_of_a_pass(pkg, synth, oracle):
    _, snaps = fx.oracle_reference(oracle, pkg, synth, "dry")
    st = [s["stats"] for s in snaps]
    dry = next(i for i, s in enumerate(st) if s["alloc_failures"] > 0)
    assert dry >= 2, "the pass that runs dry must be one that can overlap, with overlapped passes in front of it"
    # that pass served some requests and failed others; every pass behind it finds the pool empty and fails all of its own
    assert st[dry - 1]["last_free_block_id"] >= 0 and st[dry]["last_free_block_id"] == -1
    assert all(s["alloc_failures"] > 0 and s["last_free_block_id"] == -1 for s in st[dry:])
    assert dry < fx.M - 2
