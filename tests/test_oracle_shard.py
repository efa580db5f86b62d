"""Shard ownership and the dirty-block exchange on the CPU oracle against the law of ref_shard.py (check bodies in
refshard_checks.py, shared with test_gpu_shard.py).  The reference-only tests come first: the law by hand, and every
fixture reaching what it is there for before any engine is in the loop."""
import numpy as np
import pytest

import ref_shard as law
import refshard_checks as chk
import shard_fixtures as sf

EXCHANGES = [(l, d) for l in sf.LAYOUTS for d in sf.DIRTY_SETS]
FORMS = [f for f in chk.FORMS if f not in chk.HIP_ONLY_FORMS]       # (the streaming instantiations are the HIP engine's)


def test_law_by_hand():
    """12 slots, 2 shards, chunks of 3: shard 0 owns 0-2 and 6-8, shard 1 owns 3-5 and 9-11."""
    assert law.owner(np.arange(12), 2, 3).tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert law.owned(np.arange(12), shard=1, shards=2, chunk=3, first=4, count=6).tolist() == [False] * 4 + [True, True] + [False] * 3 + [True] + [False] * 2
    assert law.owned(np.arange(3), shard=5, shards=1, chunk=1).all()          # one shard: the gate is off whatever `shard` says
    lists, counts = law.plan({11, 0, 4, 7, 3}, 12, 2, 3)
    assert [x.tolist() for x in lists] == [[0, 7], [3, 4, 11]] and counts == [2, 3]
    pool = np.arange(12) * 10
    assert law.pack(pool, lists, 1, 2).tolist() == [30, 40] and law.pack(pool, lists, 1, 5).tolist() == [30, 40, 110]
    assert len(law.pack(pool, lists, 0, 0)) == 0
    recv = np.array([[-1, -2, -3], [-4, -5, -6]])
    assert law.unpack(pool, lists, 0, recv, 3).tolist() == [0, 10, 20, -4, -5, 50, 60, 70, 80, 90, 100, -6]
    assert law.unpack(pool, lists, 7, recv, 1).tolist() == [-1, 10, 20, -4, 40, 50, 60, 70, 80, 90, 100, 110]
    with pytest.raises(ValueError):
        law.plan(set(), 12, 5, 1)
    ptr, pos = np.array([4, -1, 9, -2, 2]), np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]])
    assert law.marks(ptr, [0, 1, 2, 3]) == {4, 9}
    assert law.marks(ptr, [4, 2, 0], pos, [[4, 0, 0], [2, 0, 1], [0, 0, 0]]) == {2, 4}


@pytest.mark.parametrize("layout", sorted(sf.LAYOUTS))
def test_fixtures_reach_their_edges_from_the_law_alone(layout):
    n, shards, chunk = sf.LAYOUTS[layout]
    sf.assert_layout_reach(layout)
    seen = {}
    for which in sf.DIRTY_SETS:
        d = sf.dirty_set(which, n, shards, chunk)
        lists, counts = law.plan(d, n, shards, chunk)
        assert sorted(int(s) for x in lists for s in x) == sorted(d)
        seen[which] = counts
    print(layout, {k: (v if shards <= 9 else f"max {max(v)}, {sum(c == 0 for c in v)} empty") for k, v in seen.items()})
    assert sum(seen["empty"]) == 0 and sum(seen["one"]) == 1 and sum(seen["ends"]) == 2 and sum(seen["all"]) == n
    assert sum(seen["one_chunk"]) == chunk and max(seen["one_chunk"]) == chunk
    assert sum(seen["third"]) == n // 3
    if shards > 1:
        assert not any(seen["last_shard_only"][:-1]) and seen["last_shard_only"][-1] == n // shards     # zeros in FRONT of a count
        assert not any(seen["first_shard_only"][1:]) and seen["first_shard_only"][0] == n // shards     # ... and behind one
        assert 0 in seen["one"]


def test_signatures_name_replica_and_slot():
    blocks = np.concatenate([sf.signatures(700, 3)[[699, 0, 5]], sf.signatures(9, 63)[[8]]])
    q, s = sf.decode(blocks.view(np.uint8))
    assert q.tolist() == [3, 3, 3, 63] and s.tolist() == [699, 0, 5, 8]
    blocks[1, 17] += np.uint64(1)
    with pytest.raises(AssertionError):
        sf.decode(blocks)
    for byte in (sf.PATTERN, sf.PADDING):   # neither filler is a signature of any replica (q <= 64) and slot
        assert (np.uint64(byte) * np.uint64(0x0101010101010101)) >> np.uint64(48) > 64


@pytest.mark.parametrize("layout,which", EXCHANGES)
def test_exchange(pkg, oracle, layout, which):
    print(chk.check_exchange(oracle, pkg, layout, which))


def test_refusals(pkg, oracle):
    chk.check_refusals(oracle, pkg)


@pytest.fixture(scope="module")
def twins(pkg, synth, oracle):
    return chk.Twins(oracle, pkg, synth)


@pytest.mark.parametrize("setting", chk.SETTINGS)
@pytest.mark.parametrize("form", FORMS)
def test_real_call(pkg, synth, oracle, twins, form, setting):
    chk.check_real_call(oracle, pkg, synth, twins[form], form, setting)


def test_world_of_three(pkg, synth, oracle, twins):
    chk.check_world_of_three(oracle, pkg, synth, twins["batch_unit"])
