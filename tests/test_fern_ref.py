"""The fern index's law (ref_fern.py) against its own properties, without a GPU: what identical images, ties, windows, the
harvest threshold, the hole rule and negative millimetres must give -- and that the codes tell places apart on the synthetic
room and street."""
import numpy as np
import pytest

import ref_fern as rf


def _images(seed, h=24, w=32):
    rng = np.random.RandomState(seed)
    depth = rng.randint(300, 5000, size=(h, w)).astype(np.int16)
    rgba = rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    return depth, rgba


def _code_with(fern_nibbles):
    """A code whose fern f has nibble fern_nibbles[f] (zero elsewhere)."""
    code = np.zeros(rf.CODE_DWORDS, dtype=np.uint32)
    for f, nib in fern_nibbles.items():
        code[f // 8] |= np.uint32(nib << (4 * (f % 8)))
    return code


def test_splitmix64_first_outputs():
    # the published first outputs of splitmix64 seeded with 0 and with 1234567
    rng = rf.SplitMix64(0)
    assert [rng.next() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    rng = rf.SplitMix64(1234567)
    assert [rng.next() for _ in range(2)] == [6457827717110365317, 3203168211198807973]


def test_table_ranges_and_draw_order():
    for channels in (1, 2):
        p = dict(num_ferns=64, cell=4, channels=channels, depth_min_mm=400, depth_max_mm=4000, seed=9)
        tab = rf.table(p, 32, 24)
        assert tab.shape == (64, 4, 3) and tab.dtype == np.int32
        assert tab[..., 0].min() >= 0 and tab[..., 0].max() < 8 * 6
        depth_rows = tab[tab[..., 1] == 0]
        assert depth_rows[:, 2].min() >= 400 and depth_rows[:, 2].max() <= 4000
        if channels == 1:
            assert (tab[..., 1] == 0).all()
        else:
            grey_rows = tab[tab[..., 1] == 1]
            assert len(grey_rows) > 0 and len(depth_rows) > 0 and grey_rows[:, 2].max() <= 254
    # one channel draws two numbers per decision: the first decision is next() % cells, then the threshold
    rng = rf.SplitMix64(9)
    first = rf.table(dict(num_ferns=8, cell=4, channels=1, depth_min_mm=400, depth_max_mm=4000, seed=9), 32, 24)[0, 0]
    assert first[0] == rng.next() % 48 and first[2] == 400 + rng.next() % 3601
    assert rf.resolve(None) == dict(num_ferns=512, cell=8, channels=1, depth_min_mm=300, depth_max_mm=10000, seed=0)
    assert (rf.MAX_MATCHES, rf.MAX_QUERIES, rf.CODE_DWORDS) == (64, 64, 64)


def test_identical_images_give_identical_codes_and_layout():
    p = dict(num_ferns=504, cell=4, channels=2, depth_min_mm=300, depth_max_mm=5000, seed=3)
    depth, rgba = _images(1)
    a, b = rf.encode(p, depth, rgba), rf.encode(p, depth.copy(), rgba.copy())
    assert a.dtype == np.uint32 and a.shape == (64,) and np.array_equal(a, b)
    assert a[63] == 0 and a[:63].any()            # the dwords of ferns >= F are zero
    assert rf.dissimilarity(a, b, 504) == 0
    other = rf.encode(p, *_images(2))
    assert 0 < rf.dissimilarity(a, other, 504) <= 504
    # alpha never counts, nor do remainder rows and columns
    rgba2 = rgba.copy()
    rgba2[..., 3] ^= 0xFF
    assert np.array_equal(a, rf.encode(p, depth, rgba2))
    wide_d = np.pad(depth, ((0, 3), (0, 3)), constant_values=777)
    wide_c = np.pad(rgba, ((0, 3), (0, 3), (0, 0)), constant_values=200)
    tab = rf.table(p, 32, 24)   # (the padded image has the same thumbnail size)
    assert rf.thumb_size(35, 27, 4) == (8, 6)
    assert np.array_equal(a, rf.encode(p, wide_d, wide_c, tab=tab))


def test_dissimilarity_counts_ferns_not_bits():
    a = _code_with({0: 0xF, 9: 0x1, 511: 0x8})
    b = _code_with({0: 0x0, 9: 0x1, 511: 0x4, 100: 0x2})
    assert rf.dissimilarity(a, b) == 3            # ferns 0, 511, 100
    assert rf.dissimilarity(a, b, 504) == 2       # fern 511 is not one of 504
    assert rf.dissimilarity(a, a) == 0


def test_hole_rule_at_the_boundary_and_negative_millimetres():
    c = 4
    depth = np.zeros((4, 12), dtype=np.int16)
    depth[:, 0:4].flat[:8] = 1000        # exactly c c / 2 valid pixels: kept
    depth[:, 4:8].flat[:7] = 1000        # one fewer: a hole
    depth[:, 8:12] = 1000
    depth[0, 8] = -5                     # a negative value is invalid, not part of the sum
    depth[1, 8] = 1003
    D, G = rf.thumbnails(depth, None, c)
    assert D.tolist() == [[1000, 0, (14 * 1000 + 1003) // 15]] and not G.any()
    # floor division, and the extreme values
    d2 = np.array([[1, 2], [2, 32767]], dtype=np.int16)
    assert rf.thumbnails(d2, None, 2)[0].tolist() == [[(1 + 2 + 2 + 32767) // 4]]
    assert rf.thumbnails(d2, None, 1)[0].tolist() == [[1, 2], [2, 32767]]
    # a hole never passes a decision, whatever the threshold
    tab = np.array([[[0, 0, 0]] * 4] * 8, dtype=np.int32)
    assert not rf.code_from_thumbnails(tab, np.zeros((1, 1), np.int64), np.zeros((1, 1), np.int64)).any()
    assert rf.code_from_thumbnails(tab, np.ones((1, 1), np.int64), np.zeros((1, 1), np.int64))[0] == 0xFFFFFFFF
    # grey: (r + 2 g + b) / 4 averaged with one floor
    rgba = np.zeros((2, 2, 4), dtype=np.uint8)
    rgba[..., 0], rgba[..., 1], rgba[..., 2] = 255, 255, 255
    assert rf.thumbnails(d2, rgba, 2)[1].tolist() == [[255]]
    rgba[0, 0, 1] = 254
    assert rf.thumbnails(d2, rgba, 2)[1].tolist() == [[254]]


def test_query_order_ties_windows_and_k():
    idx = rf.Index(capacity=8)
    assert idx.query(_code_with({}), 0, 100, 5) == []          # the empty index
    base = _code_with({1: 3})
    far = _code_with({1: 4, 2: 1, 3: 1})
    for code in (far, base, base, far, base):
        assert idx.process(code, 0, 0, 0, 1)[1] == idx.count - 1
    q = _code_with({1: 3, 7: 2})                                # 1 from base, 4 from far
    assert idx.query(q, 0, 5, 64) == [(1, 1), (2, 1), (4, 1), (0, 4), (3, 4)]   # ties: the lower id first; k > candidates
    assert idx.query(q, 0, 5, 2) == [(1, 1), (2, 1)]
    assert idx.query(q, 2, 4, 5) == [(2, 1), (3, 4)]           # window clipping
    assert idx.query(q, 3, 100, 5) == [(4, 1), (3, 4)]         # ... and a window that straddles count
    assert idx.query(q, 2, 2, 5) == [] and idx.query(q, 7, 9, 5) == []


def test_harvest_threshold_at_the_boundary_and_a_full_index():
    idx = rf.Index(capacity=3)
    a = _code_with({0: 1})
    assert idx.process(a, 500, 0, 0, 1) == ([], 0, False)      # the empty index always takes the frame
    b = _code_with({0: 1, 5: 2, 6: 2})                          # 2 from a
    assert idx.process(b, 3, 0, 9, 4) == ([(0, 2)], -1, False)  # smallest 2 < 3: not added
    assert idx.process(b, 2, 0, 9, 4) == ([(0, 2)], 1, False)   # smallest 2 >= 2: added
    # the test looks at ALL ids, whatever the window: id 1 is at 0 from b
    assert idx.process(b, 1, 0, 1, 4) == ([(0, 2)], -1, False)
    assert idx.process(b, 0, 0, 1, 4) == ([(0, 2)], 2, False)   # 0 always appends
    assert idx.process(b, 0, 0, 9, 1) == ([(1, 0)], -1, True)   # full: the matches are still there
    assert idx.count == 3
    idx.reset()
    assert idx.count == 0 and idx.process(a, 7, 0, 0, 1)[1] == 0


@pytest.fixture(scope="module")
def room_frames(synth):
    wl = synth.s_room(160, 120)
    key_frames = list(range(0, 30 * 6, 6))
    query_of = {3 * j: 6 * 3 * j + 2 for j in range(10)}      # 2 frames after every third keyframe
    frames = {i: wl.frame(i)[:2] for i in key_frames + list(query_of.values())}
    return frames, key_frames, query_of


@pytest.fixture(scope="module")
def street_frames(synth):
    wl = synth.s_street(160, 120, loop_at=60)
    key_frames = list(range(0, 60, 4))                        # the first lap
    # The second lap revisits the first one's poses: the loop closure.  The queries are the revisits of every third keyframe.
    # (Frames BETWEEN keyframes are not claimed on this street: its facade relief repeats every 6 m and its cars every 9 m while
    # the camera moves 1 m per frame, and at 160 x 120 the law itself sends 7 of 45 such frames to a keyframe one period away
    # with depth alone and 20 of 45 with grey -- DESIGN.md section 29.)
    queries = [60 + j for j in (0, 12, 24, 36, 48)]
    frames = {i: wl.frame(i)[:2] for i in key_frames + queries}
    return frames, key_frames, queries


@pytest.mark.parametrize("channels", [1, 2])
def test_codes_tell_the_rooms_places_apart(room_frames, channels):
    frames, key_frames, query_of = room_frames
    p = dict(num_ferns=512, cell=8, channels=channels, depth_min_mm=300, depth_max_mm=5000, seed=12345)
    tab = rf.table(p, 160, 120)
    idx = rf.Index(capacity=len(key_frames))
    for i in key_frames:
        idx.process(rf.encode(p, frames[i][1], frames[i][0], tab=tab), 0, 0, 0, 1)
    assert len(query_of) == 10
    for true_kf, i in query_of.items():
        (best, dist), = idx.query(rf.encode(p, frames[i][1], frames[i][0], tab=tab), 0, idx.count, 1)
        assert abs(best - true_kf) <= 1, (true_kf, best, dist)


@pytest.mark.parametrize("channels", [1, 2])
def test_codes_tell_the_streets_places_apart(street_frames, channels):
    frames, key_frames, queries = street_frames
    p = dict(num_ferns=512, cell=8, channels=channels, depth_min_mm=500, depth_max_mm=30000, seed=12345)
    tab = rf.table(p, 160, 120)
    idx = rf.Index(capacity=len(key_frames))
    for i in key_frames:
        idx.process(rf.encode(p, frames[i][1], frames[i][0], tab=tab), 0, 0, 0, 1)
    assert len(queries) == 5
    for i in queries:
        (best, dist), = idx.query(rf.encode(p, frames[i][1], frames[i][0], tab=tab), 0, idx.count, 1)
        assert abs(best - (i - 60) / 4.0) <= 1.0, (i, best, dist)
