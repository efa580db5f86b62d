"""The fern keyframe index on the device against the law in ref_fern.py.  Everything is an integer, so every comparison is
for equality: tables, codes, match lists (order included), counts."""
import ctypes as C

import numpy as np
import pytest

import ref_fern as rf
import util

pytestmark = pytest.mark.gpu

KINDS = ("half", "half-1", "none", "all", "max", "one", "mixed")


# ---------------------------------------------------------------------------------------------------------------------
# images whose cells sit on every edge of the thumbnail law
# ---------------------------------------------------------------------------------------------------------------------
def make_images(seed, W, H, c, count):
    """`count` (rgba, depth) pairs.  Cell i of image k is of kind KINDS[(i + k) % 7]: exactly the number of valid pixels
    that still makes a depth (2 n >= c c), one fewer, none, all, all at 32767, all at 1, a mix with negative values."""
    rng = np.random.RandomState(seed)
    tw, th = W // c, H // c
    n_pass = (c * c + 1) // 2
    out = []
    for k in range(count):
        depth = rng.randint(-3000, 32768, size=(H, W)).astype(np.int16)   # (remainder rows and columns keep this noise)
        for ty in range(th):
            for tx in range(tw):
                kind = KINDS[(ty * tw + tx + k) % 7]
                blk = rng.randint(300, 9000, size=c * c).astype(np.int16)
                invalid = np.where(rng.rand(c * c) < 0.5, 0, -rng.randint(1, 32768, size=c * c)).astype(np.int16)
                if kind in ("half", "half-1", "none"):
                    keep = {"half": n_pass, "half-1": n_pass - 1, "none": 0}[kind]
                    sel = rng.permutation(c * c)[keep:]
                    blk[sel] = invalid[sel]
                elif kind == "max":
                    blk[:] = 32767
                elif kind == "one":
                    blk[:] = 1
                elif kind == "mixed":
                    sel = rng.rand(c * c) < 0.3
                    blk[sel] = invalid[sel]
                depth[ty * c:(ty + 1) * c, tx * c:(tx + 1) * c] = blk.reshape(c, c)
        rgba = rng.randint(0, 256, size=(H, W, 4)).astype(np.uint8)
        out.append((rgba, depth))
    return out


def valid_counts(depth, c):
    H, W = depth.shape
    tw, th = W // c, H // c
    return (depth[:th * c, :tw * c].reshape(th, c, tw, c) > 0).sum(axis=(1, 3))


def as_list(matches):
    return [(int(m["id"]), int(m["dissimilarity"])) for m in matches]


def params_of(pkg, p):
    return pkg.FernParams(**p)


SHAPES = [(64, 48, 8, 7), (70, 45, 8, 7), (70, 45, 4, 7), (37, 29, 1, 7), (40, 36, 32, 7), (640, 480, 8, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the table
# ---------------------------------------------------------------------------------------------------------------------
def test_table_and_defaults(pkg, gpu):
    idx = gpu.create_fern_index(640, 480, 4)
    p, table = gpu.fern_index_table(idx)
    assert p.as_dict() == rf.resolve(None) and gpu.fern_index_count(idx) == 0
    assert table.dtype == np.int32 and np.array_equal(table, rf.table(None, 640, 480))
    for p in (dict(num_ferns=504, cell=4, channels=1, depth_min_mm=500, depth_max_mm=30000, seed=12345),
              dict(num_ferns=512, cell=8, channels=2, depth_min_mm=300, depth_max_mm=5000, seed=12345),
              dict(num_ferns=8, cell=32, channels=2, depth_min_mm=32767, depth_max_mm=32767, seed=0xFFFFFFFF),
              dict(num_ferns=64, cell=1, channels=2, depth_min_mm=0, depth_max_mm=0, seed=7)):
        idx = gpu.create_fern_index(70, 45, 2, params_of(pkg, p))
        got_p, got = gpu.fern_index_table(idx)
        assert got_p.as_dict() == rf.resolve(p), p
        assert np.array_equal(got, rf.table(p, 70, 45)), p
        if p["channels"] == 2:
            assert set(np.unique(got[..., 1])) == {0, 1}


# ---------------------------------------------------------------------------------------------------------------------
# 2. encode: every shape, F, channel count and source of the images
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,c,count", SHAPES, ids=["%dx%d cell %d" % s[:3] for s in SHAPES])
def test_encode(pkg, gpu, W, H, c, count):
    import torch
    images = make_images(100 + W + c, W, H, c, count)
    # each kind of cell occurs (with one cell per image the images take the kinds in turn)
    n_pass = (c * c + 1) // 2
    counts = np.concatenate([valid_counts(d, c).ravel() for _, d in images])
    if count == 7:
        assert {n_pass, n_pass - 1, 0, c * c} <= set(counts.tolist())
        assert any((d == 1).any() for _, d in images) and any((d == 32767).any() for _, d in images)
        assert any((d[:H // c * c, :W // c * c] < 0).any() for _, d in images)
        big = max(int(np.where(d > 0, d.astype(np.int64), 0)[:H // c * c, :W // c * c].reshape(H // c, c, W // c, c).sum(axis=(1, 3)).max())
                  for _, d in images)
        assert big == c * c * 32767            # the largest sum a cell can hold
    view = gpu.create_view(W, H)
    store = gpu.create_frame_store(W, H, len(images))
    thumbs, nonzero = {}, {}
    for channels in (1, 2):
        for F in (8, 504, 512):
            p = dict(num_ferns=F, cell=c, channels=channels, depth_min_mm=300, depth_max_mm=9000, seed=F + channels)
            idx = gpu.create_fern_index(W, H, 1, params_of(pkg, p))
            tab = rf.table(p, W, H)
            assert np.array_equal(gpu.fern_index_table(idx)[1], tab)
            for k, (rgba, depth) in enumerate(images):
                if (k, channels) not in thumbs:
                    thumbs[(k, channels)] = rf.thumbnails(depth, rgba if channels == 2 else None, c)
                want = rf.code_from_thumbnails(tab, *thumbs[(k, channels)])
                assert not want[F // 8:].any()         # (a one-cell image that is a hole has the all-zero code)
                nonzero[(channels, F)] = nonzero.get((channels, F), False) or bool(want.any())
                # a host upload
                gpu.view_update(view, rgba, depth)
                assert np.array_equal(gpu.download_view_raw_depth(view), depth)
                got = gpu.fern_encode(idx, view)
                assert got.dtype == np.uint32 and np.array_equal(got, want), ("host", F, channels, k)
                # the caller's device images; the depth image starts 2 bytes off any alignment
                t_c = torch.from_numpy(rgba).cuda()
                t_d = torch.zeros(depth.size + 1, dtype=torch.int16, device="cuda")
                t_d[1:] = torch.from_numpy(depth.ravel()).cuda()
                torch.cuda.synchronize()
                gpu.view_update_device(view, t_c.data_ptr(), t_d.data_ptr() + 2)
                assert np.array_equal(gpu.fern_encode(idx, view), want), ("device", F, channels, k)
                # a frame-store slot read in place
                gpu.frame_store_put(store, k, rgba, depth)
                gpu.view_update_from_store(view, store, k)
                assert np.array_equal(gpu.fern_encode(idx, view), want), ("store", F, channels, k)
                assert gpu.fern_index_count(idx) == 0
            idx.close()
    assert all(nonzero.values()) and len(nonzero) == 6   # no comparison above was of zeros with zeros alone


# ---------------------------------------------------------------------------------------------------------------------
# 3. add / process
# ---------------------------------------------------------------------------------------------------------------------
def test_process_harvest_rule_full_index_and_reset(pkg, gpu):
    W, H, c = 64, 48, 8
    p = dict(num_ferns=512, cell=c, channels=2, depth_min_mm=300, depth_max_mm=9000, seed=5)
    images = make_images(7, W, H, c, 4)
    codes = [rf.encode(p, d, r) for r, d in images]
    view = gpu.create_view(W, H)
    idx = gpu.create_fern_index(W, H, 3, params_of(pkg, p))
    ref = rf.Index(3)

    def step(k_img, harvest, first, last, k):
        gpu.view_update(view, *images[k_img])
        got = gpu.fern_process(idx, view, harvest, first, last, k)
        want = ref.process(codes[k_img], harvest, first, last, k)
        assert (as_list(got[0]), got[1], got[2]) == want, (k_img, harvest, first, last, k)
        assert gpu.fern_index_count(idx) == ref.count
        return want

    assert step(0, 500, 0, 10, 4) == ([], 0, False)                 # the empty index takes the frame whatever the threshold
    d01 = rf.dissimilarity(codes[0], codes[1])
    assert d01 > 1
    assert step(1, d01 + 1, 0, 10, 4) == ([(0, d01)], -1, False)    # one above the smallest: not added
    assert step(1, d01, 0, 10, 4) == ([(0, d01)], 1, False)         # at the smallest: added, the next id
    assert step(1, 1, 0, 1, 4)[1] == -1                             # the test looks at ALL ids: id 1 is at 0, outside the window
    assert step(2, 0, 1, 2, 1)[1] == 2                              # 0 always appends
    full = step(3, 0, 0, 3, 64)                                     # full: DSLAM_ERR_UNSUPPORTED, the matches all the same
    assert full[1:] == (-1, True) and len(full[0]) == 3 and gpu.fern_index_count(idx) == 3
    assert step(2, 1, 0, 3, 2)[1:] == (-1, False)
    gpu.view_update(view, *images[3])
    assert as_list(gpu.fern_query(idx, view, 0, 3, 64)) == ref.query(codes[3], 0, 3, 64)   # ... and the index is unchanged
    gpu.fern_index_reset(idx)
    ref.reset()
    assert gpu.fern_index_count(idx) == 0 and as_list(gpu.fern_query(idx, view, 0, 3, 5)) == []
    assert step(3, 9, 0, 3, 5) == ([], 0, False)


@pytest.mark.parametrize("W,H,c,channels", [(64, 48, 8, 2), (70, 45, 4, 2), (37, 29, 1, 1)])
def test_add_from_store_equals_the_per_slot_loop(pkg, gpu, W, H, c, channels):
    p = dict(num_ferns=504, cell=c, channels=channels, depth_min_mm=300, depth_max_mm=9000, seed=11)
    images = make_images(21, W, H, c, 21)
    codes = [rf.encode(p, d, r) for r, d in images]
    assert len({cd.tobytes() for cd in codes}) == 21
    store = gpu.create_frame_store(W, H, 21)
    for s, (rgba, depth) in enumerate(images):
        gpu.frame_store_put(store, s, rgba, depth)
    view = gpu.create_view(W, H)
    batch, loop = (gpu.create_fern_index(W, H, 21, params_of(pkg, p)) for _ in range(2))
    first = 0
    for n in (1, 3, 17):
        assert gpu.fern_add_from_store(batch, store, first, n) == first
        for s in range(first, first + n):
            gpu.view_update_from_store(view, store, s)
            assert gpu.fern_process(loop, view, 0, 0, 0, 1)[1:] == (s, False)
        first += n
        assert gpu.fern_index_count(batch) == first == gpu.fern_index_count(loop)
    for idx in (batch, loop):
        own = gpu.fern_query_stored(idx, list(range(21)), 0, 21, 2)
        for s in range(21):
            assert as_list(gpu.fern_query_stored(idx, [s], s, s + 1, 1)[0]) == [(s, 0)]
            gpu.view_update_from_store(view, store, s)
            assert np.array_equal(gpu.fern_encode(idx, view), codes[s])
            dist = [rf.dissimilarity(codes[s], cd, 504) for cd in codes]
            order = sorted(range(21), key=lambda i: (dist[i], i))[:2]
            assert as_list(own[s]) == [(i, dist[i]) for i in order] and order[0] == s
            assert as_list(gpu.fern_query(idx, view, 0, 21, 2)) == as_list(own[s])


# ---------------------------------------------------------------------------------------------------------------------
# 4. scan and selection
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def code_pool(pkg, gpu):
    """4097 images of 8 x 8 at cell 1 in a frame store, drawn from a pool of 48: six random images, seven variations of each
    (a few pixels changed: small dissimilarities, many ties) and plain duplicates.  The reference codes, once."""
    W = H = 8
    p = dict(num_ferns=512, cell=1, channels=1, depth_min_mm=300, depth_max_mm=9000, seed=99)
    rng = np.random.RandomState(4)
    pool = []
    for b in range(6):
        base = rng.randint(300, 9000, size=(H, W)).astype(np.int16)
        pool.append(base)
        for v in range(7):
            img = base.copy()
            for _ in range(v + 1):
                img[rng.randint(H), rng.randint(W)] = rng.randint(0, 9000)
            pool.append(img)
    tab = rf.table(p, W, H)
    pool_codes = np.stack([rf.encode(p, img, None, tab=tab) for img in pool])
    which = rng.randint(0, len(pool), size=4097)
    which[::7] = 0                               # one code at every seventh id: ties across every boundary
    which[[62, 63, 64, 65, 255, 256, 999, 4095, 4096]] = 9
    store = gpu.create_frame_store(W, H, 4097)
    rgba = np.zeros((H, W, 4), np.uint8)
    for s in range(4097):
        gpu.frame_store_put(store, s, rgba, pool[which[s]])
    return dict(p=p, pool=pool, pool_codes=pool_codes, which=which, store=store, rgba=rgba)


def windows_of(n):
    return [(0, n), (0, n + 1000), (n // 2, n // 2), (n // 3, n // 3 + 1), (max(n - 3, 0), n + 10), (n, n + 5), (n // 5, (4 * n) // 5 + 1),
            (0, 0), (n + 2, n + 9)]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000, 4097, 5 * 4097])
def test_query_matches_the_reference_order(pkg, gpu, code_pool, count):
    cp = code_pool
    idx = gpu.create_fern_index(8, 8, count, params_of(pkg, cp["p"]))
    ref = rf.Index(count)
    for first in range(0, count, 4097):          # (20485: the same 4097 slots five times -- more than one slice of the window)
        n = min(4097, count - first)
        assert gpu.fern_add_from_store(idx, cp["store"], 0, n) == first
        ref.codes.extend(cp["pool_codes"][cp["which"][:n]])
    assert gpu.fern_index_count(idx) == count
    view = gpu.create_view(8, 8)
    probe = cp["pool"][3].copy()
    probe[0, 0] = 0                               # a code that is not stored
    for q_img in (cp["pool"][0], cp["pool"][9], probe):
        code = rf.encode(cp["p"], q_img, None)
        gpu.view_update(view, cp["rgba"], q_img)
        assert np.array_equal(gpu.fern_encode(idx, view), code)
        dist = ref.distances(code)
        for k in (1, 5, 64):
            for first, last in windows_of(count):
                got = as_list(gpu.fern_query(idx, view, first, last, k))
                assert got == ref.query(code, first, last, k, dist=dist), (count, k, first, last)
    # ties at the cut: more ids at dissimilarity 0 than k, and the lower ids win
    if count >= 65:
        gpu.view_update(view, cp["rgba"], cp["pool"][0])
        zero = np.nonzero(ref.distances(cp["pool_codes"][0]) == 0)[0]
        assert len(zero) > 5
        assert as_list(gpu.fern_query(idx, view, 0, count, 5)) == [(int(i), 0) for i in zero[:5]]
    assert gpu.fern_index_count(idx) == count


@pytest.mark.parametrize("count", [65, 4097, 2 * 4097])   # (8194: two slices of the window)
def test_query_stored(pkg, gpu, code_pool, count):
    cp = code_pool
    idx = gpu.create_fern_index(8, 8, count, params_of(pkg, cp["p"]))
    ref = rf.Index(count)
    for first in range(0, count, 4097):
        n = min(4097, count - first)
        gpu.fern_add_from_store(idx, cp["store"], 0, n)
        ref.codes.extend(cp["pool_codes"][cp["which"][:n]])
    rng = np.random.RandomState(count)
    view = gpu.create_view(8, 8)
    ids64 = [0, count - 1, 63, 64, 7, 14] + rng.randint(0, count, size=58).tolist()
    dists = {q: ref.distances(ref.codes[q]) for q in set(ids64)}
    for k, (first, last) in ((1, (0, count)), (5, (count // 4, count // 2 + 3)), (64, (0, count + 7)), (64, (60, 66)), (3, (9, 9))):
        rows = gpu.fern_query_stored(idx, ids64, first, last, k)
        assert len(rows) == 64
        for q, row in zip(ids64, rows):
            assert as_list(row) == ref.query(ref.codes[q], first, last, k, dist=dists[q]), (q, k, first, last)
            if first <= q < min(last, count) and k == 64 and last - first <= 64:
                assert (q, 0) in as_list(row)                  # a query inside its window is a candidate like any other
        # one query: the same row; and the same as the view's query
        for q in ids64[:4]:
            one = gpu.fern_query_stored(idx, [q], first, last, k)
            assert len(one) == 1 and as_list(one[0]) == as_list(rows[ids64.index(q)])
            gpu.view_update(view, cp["rgba"], cp["pool"][cp["which"][q % 4097]])
            assert as_list(gpu.fern_query(idx, view, first, last, k)) == as_list(one[0])
        # permuting the queries permutes the rows and changes nothing else
        perm = rng.permutation(64)
        again = gpu.fern_query_stored(idx, [ids64[j] for j in perm], first, last, k)
        for row, j in zip(again, perm):
            assert as_list(row) == as_list(rows[j])
    assert gpu.fern_index_count(idx) == count


# ---------------------------------------------------------------------------------------------------------------------
# 5. read-only; asynchronous engines
# ---------------------------------------------------------------------------------------------------------------------
def test_bystanders_stay_byte_identical_and_an_asynchronous_engine_waits(pkg, gpu, synth):
    wl = synth.s_tiny()
    scene = gpu.create_scene(util.small_params(pkg, wl))
    rs = gpu.create_render_state(scene, wl.W, wl.H)
    fused = gpu.create_view(wl.W, wl.H)
    for i in range(2):
        rgba, mm, M = wl.frame(i)
        gpu.view_update(fused, rgba, mm, timestamp=float(i))
        gpu.process_frame(scene, fused, rs, M, wl.intr)
    gpu.get_image(scene, rs, M, wl.intr, pkg.IMAGE_DEPTH)
    before = util.snapshot(gpu, scene, rs)
    before_view = (gpu.download_view_rgba(fused).tobytes(), gpu.download_view_raw_depth(fused).tobytes())
    before_range = gpu.download_range_image(rs).tobytes()
    p = dict(num_ferns=512, cell=8, channels=2, depth_min_mm=300, depth_max_mm=5000, seed=1)
    idx = gpu.create_fern_index(wl.W, wl.H, 8, params_of(pkg, p))
    store = gpu.create_frame_store(wl.W, wl.H, 4)
    view = gpu.create_view(wl.W, wl.H)
    ref = rf.Index(8)
    frames = [wl.frame(i)[:2] for i in range(5)]
    codes = [rf.encode(p, d, r) for r, d in frames]
    for s in range(4):
        gpu.frame_store_put(store, s, *frames[s])
    stored_before = [a.copy() for s in range(4) for a in gpu.frame_store_get(store, s)]
    gpu.fern_add_from_store(idx, store, 0, 3)
    ref.codes.extend(codes[:3])
    try:
        gpu.set_async(True)                       # every call waits for the stream all the same
        gpu.view_update(view, *frames[4])
        assert np.array_equal(gpu.fern_encode(idx, view), codes[4])
        assert as_list(gpu.fern_query(idx, view, 0, 8, 8)) == ref.query(codes[4], 0, 8, 8)
        got = gpu.fern_process(idx, view, 1, 0, 8, 8)
        assert (as_list(got[0]), got[1], got[2]) == ref.process(codes[4], 1, 0, 8, 8)
        assert gpu.fern_add_from_store(idx, store, 3, 1) == ref.count
        ref.codes.append(codes[3])
        assert [as_list(r) for r in gpu.fern_query_stored(idx, [0, 4], 0, 8, 3)] == [ref.query(ref.codes[q], 0, 8, 3) for q in (0, 4)]
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert gpu.fern_index_count(idx) == ref.count == 5
    # the codes changed only where the law says: each stored id is still at 0 from its own code, in order
    for i in range(5):
        gpu.view_update(view, *(frames[i] if i < 3 else frames[4] if i == 3 else frames[3]))
        assert as_list(gpu.fern_query(idx, view, i, i + 1, 1)) == [(i, 0)]
    util.assert_same_state(before, util.snapshot(gpu, scene, rs), "the bystanding scene and render state")
    assert before["stats"] == gpu.stats(scene, rs)
    assert before_view == (gpu.download_view_rgba(fused).tobytes(), gpu.download_view_raw_depth(fused).tobytes())
    assert before_range == gpu.download_range_image(rs).tobytes()
    for a, b in zip(stored_before, [a for s in range(4) for a in gpu.frame_store_get(store, s)]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 6. rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_outputs_untouched(pkg, gpu):
    W, H = 64, 48
    p2 = params_of(pkg, dict(channels=2, seed=3))
    idx = gpu.create_fern_index(W, H, 4, p2)
    view, never = gpu.create_view(W, H), gpu.create_view(W, H)
    other_size, other_rgb = gpu.create_view(32, 24), gpu.create_view(32, 24, W, H)
    store, small_store = gpu.create_frame_store(W, H, 3), gpu.create_frame_store(32, 24, 3)
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign_view, foreign_idx, foreign_store = second.create_view(W, H), second.create_fern_index(W, H, 4, p2), second.create_frame_store(W, H, 3)
    rgba, depth = make_images(1, W, H, 8, 1)[0]
    for api, v in ((gpu, view), (gpu, other_size), (gpu, other_rgb), (second, foreign_view)):
        api.view_update(v, np.zeros((v.height, v.width, 4), np.uint8), np.full((v.height_d, v.width_d), 1000, np.int16))
    gpu.view_update(view, rgba, depth)
    for s in range(3):
        gpu.frame_store_put(store, s, rgba, depth)
        second.frame_store_put(foreign_store, s, rgba, depth)
    assert gpu.fern_add_from_store(idx, store, 0, 2) == 0
    i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

    def rejected(name, *args, outs):
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call(name, *args)
        assert all((o.view(np.int32) == -7).all() for o in outs), name
        assert gpu.fern_index_count(idx) == 2

    def outputs():
        return (np.full(64, -7, np.int32), np.full((64, 2), -7, np.int32), np.full(64, -7, np.int32), np.full(1, -7, np.int32))

    def ptr(a, t=i32):
        return None if a is None else a.ctypes.data_as(t)

    def encode(i=idx, v=view, null_out=False):
        code, *_ = outs = outputs()
        rejected("fern_encode", gpu._engine, i and i.ptr, v and v.ptr, None if null_out else ptr(code.view(np.uint32), u32), outs=outs)

    def query(i=idx, v=view, first=0, last=4, k=2, null=()):
        _, m, n, _ = outs = outputs()
        rejected("fern_query", gpu._engine, i and i.ptr, v and v.ptr, C.c_int(first), C.c_int(last), C.c_int(k),
                 None if "m" in null else util_ptr(m), None if "n" in null else ptr(n), outs=outs)

    def process(i=idx, v=view, harvest=1, first=0, last=4, k=2, null=()):
        _, m, n, a = outs = outputs()
        rejected("fern_process", gpu._engine, i and i.ptr, v and v.ptr, C.c_int(harvest), C.c_int(first), C.c_int(last), C.c_int(k),
                 None if "m" in null else util_ptr(m), None if "n" in null else ptr(n), None if "a" in null else ptr(a), outs=outs)

    def stored(i=idx, ids=(0, 1), nq=None, first=0, last=4, k=2, null=()):
        _, m, n, _ = outs = outputs()
        q = np.asarray(ids, np.int32)
        rejected("fern_query_stored", gpu._engine, i and i.ptr, None if "q" in null else ptr(q), C.c_int(len(q) if nq is None else nq),
                 C.c_int(first), C.c_int(last), C.c_int(k), None if "m" in null else util_ptr(m), None if "n" in null else ptr(n), outs=outs)

    def add(i=idx, s=store, first=0, n=1, null_out=False):
        *_, a = outs = outputs()
        rejected("fern_add_from_store", gpu._engine, i and i.ptr, s and s.ptr, C.c_int(first), C.c_int(n), None if null_out else ptr(a), outs=outs)

    def util_ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    for call in (encode, query, process):
        call(i=None)
        call(v=None)
        call(i=foreign_idx)
        call(v=foreign_view)
        call(v=never)
        call(v=other_size)
        call(v=other_rgb)            # the grey channel needs an RGB image of the depth image's size
    encode(null_out=True)
    for call in (query, process, stored):
        call(null=("m",))
        call(null=("n",))
        call(k=0)
        call(k=65)
        call(first=3, last=2)
        call(first=-1)
        call(first=-2, last=-1)
        call(i=foreign_idx) if call is stored else None
    process(null=("a",))
    process(harvest=-1)
    stored(i=None)
    stored(null=("q",))
    stored(ids=(0, 2))               # count is 2
    stored(ids=(-1,))
    stored(nq=0)
    stored(ids=tuple([0] * 65))
    add(i=None)
    add(s=None)
    add(null_out=True)
    add(i=foreign_idx)
    add(s=foreign_store)
    add(s=small_store)
    add(n=0)
    add(first=-1)
    add(first=2, n=2)                # past the store's last slot
    add(first=0, n=3)                # more than the index has room for
    # creation: parameters outside their ranges, sizes the cell does not fit
    for bad in (dict(num_ferns=12), dict(num_ferns=520), dict(num_ferns=-8), dict(cell=33), dict(cell=-1), dict(channels=3),
                dict(depth_min_mm=6000, depth_max_mm=5000), dict(depth_max_mm=32768), dict(depth_min_mm=-1)):
        h = C.c_void_p(77)
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("fern_index_create", gpu._engine, C.c_int(W), C.c_int(H), C.byref(params_of(pkg, bad)), C.c_int(4), C.byref(h))
        assert h.value == 77, bad
    for w, h_, cap, pp in ((0, H, 4, None), (W, -1, 4, None), (W, H, 0, None), (W, H, (1 << 22) + 1, None), (16, 7, 4, None)):
        h = C.c_void_p(77)
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("fern_index_create", gpu._engine, C.c_int(w), C.c_int(h_), pp, C.c_int(cap), C.byref(h))
        assert h.value == 77
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("fern_index_create", gpu._engine, C.c_int(W), C.c_int(H), None, C.c_int(4), None)
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("fern_index_reset", gpu._engine, foreign_idx.ptr)
    # ... and the index still answers
    assert as_list(gpu.fern_query(idx, view, 0, 4, 4)) == [(0, 0), (1, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# 7. lifetime
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["index last", "index first", "index before the engine"])
def test_an_index_may_go_before_or_after_the_other_handles(pkg, gpu, synth, order):
    wl = synth.s_tiny()
    base = gpu.debug_live_engines()
    api = pkg.open_engine(0)
    scene = api.create_scene(util.small_params(pkg, wl))
    view = api.create_view(wl.W, wl.H)
    store = api.create_frame_store(wl.W, wl.H, 2)
    idx = api.create_fern_index(wl.W, wl.H, 4)
    rgba, mm, _ = wl.frame(0)
    api.view_update(view, rgba, mm)
    api.frame_store_put(store, 0, rgba, mm)
    assert api.fern_process(idx, view, 0, 0, 4, 1)[1] == 0 and api.fern_add_from_store(idx, store, 0, 1) == 1
    assert gpu.debug_live_engines() == base + 1
    others = (scene, view, store)
    if order == "index before the engine":
        idx.close()
        for h in others:
            h.close()
        assert gpu.debug_live_engines() == base + 1
        api.close()
    else:
        api.close()                                  # the engine first: its handles keep the object and its streams
        for h in ((idx,) + others if order == "index first" else others + (idx,)):
            assert gpu.debug_live_engines() == base + 1
            h.close()
    assert gpu.debug_live_engines() == base
    assert gpu.selftest_division(1 << 12) == 0
