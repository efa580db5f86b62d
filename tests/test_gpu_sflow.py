"""dslam_sflow_* on the MI355X, everything bit for bit: the filter images, the features of both sets
of all four images and the matches of every method, each separately, against tests/ref_sflow.py and against libviso2's own
output (tests/golden/sflow_*.npz); the ring, the forms of the calls, the crafted corners of the law and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import ref_sflow as rf
import sflow_fixtures as sf

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
# the golden cases by size, and 37 x 45: a width that is no multiple of 16 with exactly one sparse cell
SIZE_CASES = ["quad_96x64", "quad_160x96", "quad_131x77", "quad_320x128_half", "quad_30x30", "quad_40x40", "37x45"]


def params_of(pkg, encoded):
    return pkg.SflowParams(**encoded)


def dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).to("cuda:0")       # (a copy: the shared references are read-only)
    torch.cuda.synchronize()
    return t


def dev_pattern(words):
    import torch
    t = torch.full((words,), PATTERN, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def case(name):
    """(W, H, encoded parameters, pushes, reference, golden or None)"""
    if name == "37x45":
        f, ref = sf.size_reference(37, 45, 0)
        return 37, 45, rf.encode(half_resolution=0), [(f["1p"], f["2p"]), (f["1c"], f["2c"])], ref, None
    W, H = sf.CASES[name][:2]
    g = sf.golden(name)
    return W, H, sf.case_params(name), [(g["img_1p"], g["img_2p"]), (g["img_1c"], g["img_2c"])], sf.reference(name), g


def push_all(gpu, h, pushes):
    for left, right in pushes:
        gpu.sflow_push(h, left, right)


def check_filters(pkg, gpu, h, ref, what):
    for side, images in ref["filters"].items():
        for which, want in enumerate(images):
            got = gpu.debug_sflow_download(h, side, which)
            assert got.dtype == want.dtype and np.array_equal(got, want), (what, "filter", side, which)


def check_features(pkg, gpu, h, ref, what):
    for (image, which), want in ref["features"].items():
        got, n = gpu.sflow_features(h, image, which)
        assert n == len(want) and np.array_equal(got, want), (what, "features", image, which)


def check_matches(pkg, gpu, h, ref, what):
    for (method, which), want in ref["matches"].items():
        got, n = gpu.sflow_match(h, method, which)
        assert n == len(want) and np.array_equal(got, want), (what, "matches", method, which)


def check_stages(pkg, gpu, h, ref, what):
    """Filters, then features, then matches: a failure names its stage."""
    check_filters(pkg, gpu, h, ref, what)
    check_features(pkg, gpu, h, ref, what)
    check_matches(pkg, gpu, h, ref, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every stage at every size, against the law and against the library's own output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SIZE_CASES)
def test_every_stage_equals_the_reference(pkg, gpu, name):
    W, H, enc, pushes, ref, g = case(name)
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    assert h.params.effective() == rf.resolve(enc)
    push_all(gpu, h, pushes)
    check_stages(pkg, gpu, h, ref, name)
    if name == "37x45":
        assert rf.num_cells(37, 45, rf.sparse_n(3)) == 1 and len(ref["features"][(rf.IMAGE_1C, 1)]) > 0
    h.close()


@pytest.mark.parametrize("name", list(sf.CASES))
def test_the_device_equals_the_library(pkg, gpu, name):
    """The golden files directly, without this repository's statement of the law in between."""
    W, H, enc, pushes, ref, g = case(name)
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    push_all(gpu, h, pushes)
    for key, (image, which) in sf.SETS.items():
        if key in g:
            got, n = gpu.sflow_features(h, image, which)
            assert n == len(g[key]) and np.array_equal(got, g[key]), key
    if "raw_matches" in g:
        got, n = gpu.sflow_match(h, int(g["method"]), 0)
        assert n == len(g["raw_matches"]) and np.array_equal(got, g["raw_matches"])
    else:   # the library's dense matches after its outlier removal: a subset of the dense set matched without a prior
        got, n = gpu.sflow_match(h, 2, 1)
        ours = set(map(tuple, got.tolist()))
        assert n == len(ours) >= len(g["matches"]) >= 300 and all(tuple(m) in ours for m in g["matches"].tolist())
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the forms of the calls
# ---------------------------------------------------------------------------------------------------------------------
def test_rgba_equals_grey_of_the_same_images(pkg, gpu):
    W, H = 96, 64
    rng = np.random.RandomState(5)
    f = sf.frames(W, H, 5, (2, 1), 2)
    pushes4, pushes1 = [], []
    for pair in (("1p", "2p"), ("1c", "2c")):
        rgba = []
        for k in pair:
            # a colour image whose grey is not any of its channels
            c = np.stack([f[k], np.roll(f[k], 3, axis=1), np.roll(f[k], 5, axis=0), rng.randint(0, 256, (H, W)).astype(np.uint8)], axis=-1)
            rgba.append(np.ascontiguousarray(c))
        pushes4.append(tuple(rgba))
        pushes1.append(tuple(rf.grey(c, 4).astype(np.uint8) for c in rgba))
    ref = sf.reference_of(W, H, rf.encode(half_resolution=0), pushes1, methods=(2,))
    assert len(ref["matches"][(2, 1)]) > 20
    h4 = gpu.create_sflow(W, H, params_of(pkg, dict(half_resolution=-1, channels=4)))
    h1 = gpu.create_sflow(W, H, params_of(pkg, dict(half_resolution=-1)))
    push_all(gpu, h4, pushes4)
    push_all(gpu, h1, pushes1)
    check_stages(pkg, gpu, h4, ref, "rgba")
    check_stages(pkg, gpu, h1, ref, "grey")
    h4.close(), h1.close()


def test_rgba_at_half_resolution(pkg, gpu):
    W, H = 128, 96
    f = sf.frames(W, H, 6, (2, 2), 3)
    pushes4 = [tuple(np.ascontiguousarray(np.stack([f[k], f[k][::-1], f[k][:, ::-1], f[k]], axis=-1)) for k in pair) for pair in (("1p", "2p"), ("1c", "2c"))]
    m = rf.Matcher(W, H, dict(channels=4))
    for left, right in pushes4:
        m.push(left, right)
    h = gpu.create_sflow(W, H, params_of(pkg, dict(channels=4)))
    push_all(gpu, h, pushes4)
    for side in (0, 1):
        for which, want in enumerate(m.filter_images(side)):
            assert np.array_equal(gpu.debug_sflow_download(h, side, which), want), (side, which)
    for image in range(4):
        assert np.array_equal(gpu.sflow_features(h, image, 1)[0], m.features(image, 1)), image
    assert np.array_equal(gpu.sflow_match(h, 2, 1)[0], m.match(2, 1))
    h.close()


def test_the_ring_rotates_and_replace_overwrites(pkg, gpu):
    W, H = 96, 64
    enc = rf.encode(half_resolution=0)
    a, b, c = sf.frames(W, H, 5, (2, 1), 2), sf.frames(W, H, 5, (2, 1), 9), sf.frames(W, H, 4, (1, 2), 11)
    seq = [(a["1p"], a["2p"], False), (a["1c"], a["2c"], False), (b["1p"], b["2p"], False), (b["1c"], b["2c"], True), (c["1c"], c["2c"], False),
           (c["1p"], c["2p"], True), (a["1p"], a["2p"], True)]
    m = rf.Matcher(W, H, enc)
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    # before the first frame, and with one frame only, nothing matches
    assert gpu.sflow_match(h, 2, 0)[1] == 0 and gpu.sflow_features(h, rf.IMAGE_1P, 1)[1] == 0
    for k, (left, right, replace) in enumerate(seq):
        m.push(left, right, replace)
        gpu.sflow_push(h, left, right, replace)
        for image in range(4):
            for which in (0, 1):
                assert np.array_equal(gpu.sflow_features(h, image, which)[0], m.features(image, which)), (k, image, which)
        for method in (0, 1, 2):
            assert np.array_equal(gpu.sflow_match(h, method, 1)[0], m.match(method, 1)), (k, method)
        assert np.array_equal(gpu.sflow_match(h, 2, 0)[0], m.match(2, 0)), k
    assert len(m.match(2, 1)) > 20
    h.close()


def test_without_a_right_image_only_flow_matches(pkg, gpu):
    W, H = 96, 64
    enc = rf.encode(half_resolution=0)
    f = sf.frames(W, H, 5, (2, 1), 2)
    m = rf.Matcher(W, H, enc)
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    gpu.sflow_push(h, f["1p"], f["2p"])                 # a stereo frame first: its right lists must not be seen again below
    gpu.sflow_push(h, f["1p"], None, replace=True)
    gpu.sflow_push(h, f["1c"], None)
    m.push(f["1p"], None), m.push(f["1c"], None)
    for which in (0, 1):
        got, n = gpu.sflow_match(h, 0, which)
        assert n == len(m.match(0, which)) and np.array_equal(got, m.match(0, which))
        assert gpu.sflow_match(h, 1, which)[1] == 0 and gpu.sflow_match(h, 2, which)[1] == 0
        assert gpu.sflow_features(h, rf.IMAGE_2C, which)[1] == 0 and gpu.sflow_features(h, rf.IMAGE_2P, which)[1] == 0
    assert len(m.match(0, 1)) > 50
    h.close()


def test_device_forms_and_a_small_capacity(pkg, gpu):
    name = "quad_131x77"
    W, H, enc, pushes, ref, g = case(name)
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    images = [(dev(left), dev(right)) for left, right in pushes]
    for left, right in images:
        gpu.sflow_push_device(h, left.data_ptr(), right.data_ptr())
    gpu.synchronize()
    check_stages(pkg, gpu, h, ref, "device push")
    for method, which in ((2, 0), (2, 1), (1, 1), (0, 0)):
        want = ref["matches"][(method, which)]
        assert len(want) > 8
        for capacity in (len(want) + 3, len(want), 5):
            out, count = dev_pattern(12 * (capacity + 2)), dev_pattern(4)
            gpu.sflow_match_device(h, method, which, out.data_ptr(), capacity, count.data_ptr())
            gpu.synchronize()
            got, n = host(out).reshape(-1, 12), host(count)
            assert n[0] == len(want) and (n[1:] == PATTERN).all(), (method, which, capacity)
            k = min(capacity, len(want))
            assert np.array_equal(got[:k], want[:k]) and (got[k:] == PATTERN).all(), (method, which, capacity)
        # the host form with too little room: the full count, the first records, nothing behind them
        room = np.full((7, 12), PATTERN, np.int32)
        got, n = gpu.sflow_match(h, method, which, capacity=5, out=room)
        assert n == len(want) and np.array_equal(got, want[:5]) and (room[5:] == PATTERN).all()
    got, n = gpu.sflow_features(h, rf.IMAGE_1C, 1, capacity=4)
    assert n == len(ref["features"][(rf.IMAGE_1C, 1)]) and np.array_equal(got, ref["features"][(rf.IMAGE_1C, 1)][:4])
    # a second match on the same handle gives the same
    check_matches(pkg, gpu, h, ref, "again")
    h.close()


def test_two_handles_of_different_sizes_do_not_disturb_each_other(pkg, gpu):
    Wa, Ha, enca, pa, ra, _ = case("quad_96x64")
    Wb, Hb, encb, pb, rb, _ = case("quad_320x128_half")
    a, b = gpu.create_sflow(Wa, Ha, params_of(pkg, enca)), gpu.create_sflow(Wb, Hb, None)
    assert b.params.as_dict() == rf.DEFAULTS
    for (la, ra_), (lb, rb_) in zip(pa, pb):
        gpu.sflow_push(a, la, ra_)
        gpu.sflow_push(b, lb, rb_)
    check_matches(pkg, gpu, b, rb, "b")
    check_stages(pkg, gpu, a, ra, "a after b ran")
    check_stages(pkg, gpu, b, rb, "b after a ran")
    a.close(), b.close()


def test_a_matcher_outlives_its_engine(pkg, gpu):
    base = gpu.debug_live_engines()
    api = pkg.open_engine(0)
    W, H, enc, pushes, ref, _ = case("quad_96x64")
    h = api.create_sflow(W, H, params_of(pkg, enc))
    push_all(api, h, pushes)
    check_matches(pkg, api, h, ref, "before")
    api.close()
    assert gpu.debug_live_engines() == base + 1
    h.close()
    assert gpu.debug_live_engines() == base


# ---------------------------------------------------------------------------------------------------------------------
# 3. the corners of the law
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sf.CRAFTED)
def test_crafted_cases(pkg, gpu, name):
    c, ref = sf.crafted_reference(name)
    h = gpu.create_sflow(c["W"], c["H"], params_of(pkg, sf.FULL))
    push_all(gpu, h, c["pushes"])
    check_stages(pkg, gpu, h, ref, name)
    h.close()


@pytest.mark.parametrize("enc", [dict(nms_n=1, half_resolution=-1), dict(nms_n=4, nms_tau=20, half_resolution=-1),
                                 dict(match_binsize=7, match_radius=20, match_disp_tolerance=1, half_resolution=-1),
                                 dict(match_binsize=500, match_radius=5, half_resolution=1)],
                         ids=lambda e: "-".join(f"{k}{v}" for k, v in e.items()))
def test_parameter_corners(pkg, gpu, enc):
    """One pixel cells, the sparse distance at its cap of 10, bins smaller than the window and one bin for everything, a radius
    that integer division halves to 2."""
    W, H = 96, 64
    f = sf.frames(W, H, 4, (2, 2), 2)
    pushes = [(f["1p"], f["2p"]), (f["1c"], f["2c"])]
    ref = sf.reference_of(W, H, enc, pushes, methods=(0, 2))
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    assert h.params.effective() == rf.resolve(enc)
    push_all(gpu, h, pushes)
    check_stages(pkg, gpu, h, ref, enc)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument checks: the error, and nothing written
# ---------------------------------------------------------------------------------------------------------------------
def test_create_rejects_what_the_header_says(pkg, gpu):
    base = gpu.debug_live_engines()
    for W, H in ((0, 8), (8, 0), (4097, 8), (8, 4097), (-1, 8), (1, 8), (8, 1)):
        with pytest.raises(pkg.DslamError):
            gpu.create_sflow(W, H)
    gpu.create_sflow(1, 1, params_of(pkg, dict(half_resolution=-1))).close()      # full resolution: one pixel is a size
    for bad in (dict(nms_n=-1), dict(nms_n=33), dict(nms_tau=-5), dict(match_binsize=-1), dict(match_radius=-1), dict(match_disp_tolerance=-1),
                dict(half_resolution=2), dict(half_resolution=-2), dict(channels=2), dict(channels=3)):
        with pytest.raises(ValueError):
            rf.resolve(bad)
        with pytest.raises(pkg.DslamError):
            gpu.create_sflow(64, 48, params_of(pkg, bad))
    with pytest.raises(ValueError):
        rf.check_size(4096, 4096, rf.resolve(dict(match_binsize=1)))
    with pytest.raises(pkg.DslamError):
        gpu.create_sflow(4096, 4096, params_of(pkg, dict(match_binsize=1)))            # more bin lists than DSLAM_SFLOW_MAX_BINS
    p = pkg.SflowParams()
    p.pad = 1
    with pytest.raises(pkg.DslamError):
        gpu.create_sflow(64, 48, p)
    h = C.c_void_p()
    assert gpu._fn("sflow_create")(gpu._engine, C.c_int(64), C.c_int(48), None, None) == -1
    assert gpu._fn("sflow_create")(None, C.c_int(64), C.c_int(48), None, C.byref(h)) == -1 and not h.value
    assert gpu.debug_live_engines() == base


def test_calls_reject_bad_arguments_and_write_nothing(pkg, gpu):
    W, H, enc, pushes, ref, _ = case("quad_96x64")
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    with pytest.raises(pkg.DslamError):
        gpu.debug_sflow_download(h, 0, pkg.SFLOW_FILTER_F1)                     # no frame yet
    push_all(gpu, h, pushes)
    want = ref["matches"][(2, 1)]
    room = np.full((len(want) + 2, 12), PATTERN, np.int32)
    count = C.c_int32(PATTERN)
    left, right = dev(pushes[1][0]), dev(pushes[1][1])
    out_dev, count_dev = dev_pattern(12 * len(room)), dev_pattern(4)

    def untouched():
        assert (room == PATTERN).all() and count.value == PATTERN
        assert (host(out_dev) == PATTERN).all() and (host(count_dev) == PATTERN).all()

    e, s = gpu._engine, h.ptr
    lp, rp, op = (a.ctypes.data_as(C.c_void_p) for a in (pushes[1][0], pushes[1][1], room))
    cp, cap = C.byref(count), C.c_int(len(room))
    ld, rd, od, cd = (C.c_void_p(t.data_ptr()) for t in (left, right, out_dev, count_dev))
    i0, i1, i2 = C.c_int(0), C.c_int(1), C.c_int(2)
    for name, args in (("sflow_push", (e, s, None, rp, i0)), ("sflow_push", (None, s, lp, rp, i0)), ("sflow_push", (e, None, lp, rp, i0)),
                       ("sflow_push_device", (e, s, None, rd, i0)),
                       ("sflow_push_device", (e, s, C.c_void_p(left.data_ptr() + 1), rd, i0)),
                       ("sflow_push_device", (e, s, ld, C.c_void_p(right.data_ptr() + 4), i0)),
                       ("sflow_match", (e, s, i2, i1, None, cap, cp)), ("sflow_match", (e, s, i2, i1, op, cap, None)),
                       ("sflow_match", (None, s, i2, i1, op, cap, cp)), ("sflow_match", (e, None, i2, i1, op, cap, cp)),
                       ("sflow_match", (e, s, C.c_int(3), i1, op, cap, cp)), ("sflow_match", (e, s, C.c_int(-1), i1, op, cap, cp)),
                       ("sflow_match", (e, s, i2, i2, op, cap, cp)), ("sflow_match", (e, s, i2, C.c_int(-1), op, cap, cp)),
                       ("sflow_match", (e, s, i2, i1, op, C.c_int(-1), cp)),
                       ("sflow_match_device", (e, s, i2, i1, None, cap, cd)), ("sflow_match_device", (e, s, i2, i1, od, cap, None)),
                       ("sflow_match_device", (e, s, i2, i1, C.c_void_p(out_dev.data_ptr() + 4), cap, cd)),
                       ("sflow_match_device", (e, s, i2, i1, od, cap, C.c_void_p(count_dev.data_ptr() + 4))),
                       ("sflow_match_device", (e, s, C.c_int(3), i1, od, cap, cd)),
                       ("sflow_features", (e, s, C.c_int(4), i1, op, cap, cp)), ("sflow_features", (e, s, C.c_int(-1), i1, op, cap, cp)),
                       ("sflow_features", (e, s, i0, i2, op, cap, cp)), ("sflow_features", (e, s, i0, i1, None, cap, cp)),
                       ("sflow_features", (e, s, i0, i1, op, cap, None)), ("sflow_features", (e, s, i0, i1, op, C.c_int(-1), cp)),
                       ("debug_sflow_download", (e, s, i0, i0, None)), ("debug_sflow_download", (e, s, i2, i0, op)),
                       ("debug_sflow_download", (e, s, i0, C.c_int(4), op)), ("debug_sflow_download", (e, s, i0, C.c_int(-1), op)),
                       ("debug_sflow_phases", (None, s, i0, None)), ("debug_sflow_phases", (e, None, i0, None)),
                       ("sflow_get_params", (s, None)), ("sflow_get_params", (None, cp))):
        assert gpu._fn(name)(*args) == -1, (name, args)
    untouched()
    # a handle used on another engine
    other = pkg.open_engine(0)
    for call in (lambda: other.sflow_push(h, pushes[0][0], pushes[0][1]),
                 lambda: other.sflow_push_device(h, left.data_ptr(), right.data_ptr()),
                 lambda: other.sflow_match(h, 2, 1, capacity=len(room), out=room),
                 lambda: other.sflow_match_device(h, 2, 1, out_dev.data_ptr(), len(room), count_dev.data_ptr()),
                 lambda: other.sflow_features(h, 0, 1),
                 lambda: other.debug_sflow_download(h, 0, 0),
                 lambda: other.sflow_phases(h)):
        with pytest.raises(pkg.DslamError):
            call()
    other.close()
    untouched()
    # the handle is none the worse for any of it: no rejected push rotated the ring
    check_stages(pkg, gpu, h, ref, "after the rejected calls")
    assert gpu._fn("sflow_destroy")(None) == 0
    h.close()


def test_phase_times_are_recorded_when_asked(pkg, gpu):
    W, H, enc, pushes, ref, _ = case("quad_96x64")
    h = gpu.create_sflow(W, H, params_of(pkg, enc))
    assert gpu.sflow_phases(h) == [-1.0] * 6
    gpu.sflow_phases(h, enable=1, read=False)
    push_all(gpu, h, pushes)
    check_matches(pkg, gpu, h, ref, "timed")
    ms = gpu.sflow_phases(h, enable=0)
    assert all(0.0 <= t < 1000.0 for t in ms), ms
    h.close()
