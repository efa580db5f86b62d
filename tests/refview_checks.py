"""Check bodies shared by test_oracle_view_reference.py (CPU oracle) and test_gpu_view_reference.py (HIP engine): each
takes an `api`, runs the real entry points of the view path and compares them with refview.py / ref64.py.  With
`api=None` the depth post-processing cases run the reference alone: the reach floors and the tie cap every case
asserts come from the reference and the inputs, never from an engine."""
import functools

import numpy as np

import analytic_maps as am
import ref64
import ref64_checks as rc
import refview as rv

F = np.float32
ALL_INT16 = np.arange(-32768, 32768).astype(np.int16).reshape(256, 256)  # every int16 value once


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# plain conversion, every int16
# ---------------------------------------------------------------------------------------------------------------------
CONVERSION_PAIRS = {"default": (1.0 / 1000.0, 0.0), "tum_5000": (1.0 / 5000.0, 0.0), "offset": (1.0 / 1000.0, 0.25)}


def check_conversion(api, pair):
    a, b = CONVERSION_PAIRS[pair]
    v = api.create_view(256, 256)
    api.view_update(v, np.zeros((256, 256, 4), np.uint8), ALL_INT16, affine_a=a, affine_b=b)
    got = api.download_view_depth(v)
    want64 = ref64.depth_to_float(ALL_INT16, a, b)
    valid = (ALL_INT16 > 0) & (ALL_INT16 <= 32000)
    assert np.array_equal(got == -1.0, ~valid), "the gate r <= 0 || r > 32000"
    assert valid.sum() == 32000 and got[ALL_INT16 == 32000][0] > 0 and got[ALL_INT16 == 32001][0] == -1.0
    if b == 0.0:
        # one rounding: the float64 value rounded to float32 is the float32 product, bit for bit
        assert np.array_equal(_bits(got), _bits(want64.astype(F))), "depth conversion against ref64.depth_to_float"
    else:
        # product and sum round separately (no engine fuses them): the float32 evaluation bit for bit, and the float64
        # value within the two roundings
        assert np.array_equal(_bits(got), _bits(rv.depth_to_float32(ALL_INT16, a, b)))
        assert (np.abs(got.astype(np.float64) - want64)[valid] <= 2 * rv.U * np.abs(want64[valid])).all()
    assert np.array_equal(api.download_view_raw_depth(v), ALL_INT16)


# ---------------------------------------------------------------------------------------------------------------------
# dataset formats, every int16
# ---------------------------------------------------------------------------------------------------------------------
# (format, max_m): a cut that falls on an attained value, max_m just either side of it, and one that cuts nothing;
# for /5 also a max_m beyond int16, which wraps negative and blanks the image (refview.max_mm_short)
DATASET_CASES = [(0, 0.0),
                 (1, 20.0), (1, 19.998), (1, 20.004), (1, 128.0),
                 (2, 4.0), (2, 3.9994), (2, 4.0006), (2, 10.0), (2, 40.0)]


def check_dataset(api, fmt, max_m):
    rng = np.random.default_rng(100 * fmt + int(max_m))
    rgba = rng.integers(0, 256, (256, 256, 4), dtype=np.uint8)
    rgba[..., 3] = 255
    bgr = np.ascontiguousarray(rgba[..., 2::-1])
    want = rv.dataset_depth(ALL_INT16, fmt, max_m)
    # the laws, from the reference alone
    pos = ALL_INT16.astype(np.int64)
    at = lambda d: int(want[pos == d][0])  # noqa: E731
    if fmt == 0:
        assert np.array_equal(want, ALL_INT16)
    elif fmt == 1:
        cut = int(np.floor(float(F(max_m) * F(256))))
        if cut < 32767:
            assert at(cut) == cut * 1000 // 256 and at(cut + 1) == 0 and not want[pos > cut].any()
        else:
            assert at(32767) == 127996 - 2 * 65536 and at(16777) == -1 and at(16778) == 3  # nothing is cut; 127996 wraps twice
        assert at(-1) == -3 and at(0) == 0 and at(1) == 3 and at(256) == 1000
        assert cut < 8389 or at(8388) == 32765 and at(8389) == 32769 - 65536, "the wrap past int16"
    else:
        ms = rv.max_mm_short(max_m)
        if max_m == 40.0:
            assert ms == 40000 - 65536 and not want.any()
        elif ms > 6553:  # nothing is cut: 32767 / 5 = 6553
            assert at(32767) == 6553 and at(32765) == 6553 and at(32764) == 6552 and (want[pos >= 5] > 0).all()
        else:
            assert 0 < ms and at(5 * ms + 4) == ms and at(5 * ms + 5) == 0 and at(5 * ms - 1) == ms - 1
        if ms >= 0:
            assert at(-7) == -1 and at(-4) == 0 and at(4) == 0 and at(-32768) == -6553
        assert {4.0: 4000, 3.9994: 3999, 4.0006: 4001, 10.0: 10000, 40.0: -25536}[max_m] == ms
    v = api.create_view(256, 256)
    for colour in (rgba, bgr):
        api.view_update_dataset(v, colour, ALL_INT16, fmt, max_m)
        assert np.array_equal(api.download_view_raw_depth(v), want), f"format {fmt}, max {max_m}: raw depth"
        assert np.array_equal(_bits(api.download_view_depth(v)), _bits(ref64.depth_to_float(want).astype(F))), "float depth"
        assert np.array_equal(api.download_view_rgba(v), rgba), f"colour from {colour.shape[-1]} channels"


# ---------------------------------------------------------------------------------------------------------------------
# BGR -> RGBA
# ---------------------------------------------------------------------------------------------------------------------
# W x H with W * H = 1, 2, 3, 4, 5, 7, 1023, 1024, 1025 and 641 x 3: every npix % 4, and n4 == 0
BGR_SHAPES = [(1, 1), (2, 1), (1, 3), (4, 1), (5, 1), (7, 1), (1023, 1), (32, 32), (205, 5), (641, 3)]


def check_bgr(api, W, H, device=False):
    rng = np.random.default_rng(W * 1000 + H)
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mm = rng.integers(0, 4000, (H, W)).astype(np.int16)
    v = api.create_view(W, H)
    api.view_update(v, np.full((H, W, 4), 7, np.uint8), mm)  # something else first: a stale image would show
    if device:
        import torch
        t_bgr, t_mm = torch.from_numpy(bgr).cuda(), torch.from_numpy(mm).cuda()
        torch.cuda.synchronize()
        assert t_bgr.data_ptr() % 4 == 0
        api.view_update_bgr_device(v, t_bgr.data_ptr(), t_mm.data_ptr())
    else:
        api.view_update_bgr(v, bgr, mm)
    assert np.array_equal(api.download_view_rgba(v), rv.bgr_to_rgba(bgr))
    assert np.array_equal(api.download_view_raw_depth(v), mm)
    assert np.array_equal(_bits(api.download_view_depth(v)), _bits(ref64.depth_to_float(mm).astype(F)))


# ---------------------------------------------------------------------------------------------------------------------
# every upload route leaves the same view
# ---------------------------------------------------------------------------------------------------------------------
def check_routes(api, device_routes=False):
    """Colour 37 x 21, depth 61 x 47.  Every route gets images of its own and is compared with the numpy reference,
    not with another route; the bilateral flag alternates, so each route also follows a call that left the view's
    buffers in the other arrangement."""
    Wc, Hc, Wd, Hd = 37, 21, 61, 47
    v = api.create_view(Wc, Hc, Wd, Hd)
    fs = api.create_frame_store(Wc, Hc, 3, Wd, Hd)
    rng = np.random.default_rng(31)
    keep = []
    done = []

    def images(i):
        rgba = rng.integers(0, 256, (Hc, Wc, 4), dtype=np.uint8)
        mm = rc.filter_input(Wd, Hd, seed=50 + i)
        return rgba, np.ascontiguousarray(rgba[..., 2::-1]), mm

    def expect(what, rgba_want, mm, bilateral):
        assert np.array_equal(api.download_view_rgba(v), rgba_want), f"{what}: colour"
        assert np.array_equal(api.download_view_raw_depth(v), mm), f"{what}: raw depth"
        got = api.download_view_depth(v)
        plain = ref64.depth_to_float(mm).astype(F)
        if not bilateral:
            assert np.array_equal(_bits(got), _bits(plain)), f"{what}: float depth"
        else:
            _compare_filtered(got.astype(np.float64), ref64.bilateral_update_view(plain), 1e-5, what)
        done.append(what)

    def bgr_want(rgba):
        out = rgba.copy()
        out[..., 3] = 255
        return out

    routes = ["view_update", "view_update_bgr", "view_update_dataset", "view_update_dataset_bgr", "store_put",
              "store_put_bgr", "store_put_view"]
    if device_routes:
        assert api.has("view_update_device") and api.has("view_update_bgr_device")
        import torch
        routes += ["view_update_device", "view_update_bgr_device"]
    for i, route in enumerate(routes):
        bil = i % 2 == 1
        rgba, bgr, mm = images(i)
        if route == "view_update":
            api.view_update(v, rgba, mm, bilateral=bil)
            expect(route, rgba, mm, bil)
        elif route == "view_update_bgr":
            api.view_update_bgr(v, bgr, mm, bilateral=bil)
            expect(route, bgr_want(rgba), mm, bil)
        elif route == "view_update_dataset":
            api.view_update_dataset(v, rgba, mm, 0, 0.0, bilateral=bil)
            expect(route, rgba, mm, bil)
        elif route == "view_update_dataset_bgr":
            api.view_update_dataset(v, bgr, mm, 0, 0.0, bilateral=bil)
            expect(route, bgr_want(rgba), mm, bil)
        elif route == "store_put":
            api.frame_store_put(fs, 0, rgba, mm)
            api.view_update_from_store(v, fs, 0, bilateral=bil)
            expect(route, rgba, mm, bil)
        elif route == "store_put_bgr":
            api.frame_store_put_bgr(fs, 1, bgr, mm)
            api.view_update_from_store(v, fs, 1, bilateral=bil)
            expect(route, bgr_want(rgba), mm, bil)
        elif route == "store_put_view":
            api.view_update(v, rgba, mm, bilateral=True)  # the store keeps the RAW depth, whatever the view's filter did
            api.frame_store_put_view(fs, 2, v)
            other = images(100 + i)
            api.view_update(v, other[0], other[2])
            api.view_update_from_store(v, fs, 2, bilateral=bil)
            expect(route, rgba, mm, bil)
            # the earlier slots are still what was put there
            api.view_update_from_store(v, fs, 0)
            expect("slot 0 again", *keep[0], False)
        elif route == "view_update_device":
            t_c, t_d = torch.from_numpy(rgba).cuda(), torch.from_numpy(mm).cuda()
            torch.cuda.synchronize()
            api.view_update_device(v, t_c.data_ptr(), t_d.data_ptr(), bilateral=bil)
            expect(route, rgba, mm, bil)
        elif route == "view_update_bgr_device":
            t_c, t_d = torch.from_numpy(bgr).cuda(), torch.from_numpy(mm).cuda()
            torch.cuda.synchronize()
            api.view_update_bgr_device(v, t_c.data_ptr(), t_d.data_ptr(), bilateral=bil)
            expect(route, bgr_want(rgba), mm, bil)
        if route == "store_put":
            keep.append((rgba, mm))
    return done


# ---------------------------------------------------------------------------------------------------------------------
# bilateral filter at the tile's edges
# ---------------------------------------------------------------------------------------------------------------------
# 16 x 16 output tiles with a 10-pixel halo: one tile exactly, one pixel more than a tile / two tiles, a second tile
# that is all halo-clipped border (26 = 16 + 10), and odd sizes; rc.filter_input serves from 6 x 3 up
FILTER_SIZES = [(16, 16), (17, 33), (26, 26), (37, 21)]


def _compare_filtered(got, want, rel_tol, what="bilateral filter"):
    """The assertions of ref64_checks.check_view_filter on a given pair of images."""
    H, W = want.shape
    border = np.ones((H, W), bool)
    border[2:H - 2, 2:W - 2] = False
    assert np.array_equal(got[border], want[border]), f"{what}: border differs from upstream's zero floatImage border"
    inner = ~border
    assert np.array_equal(got[inner] == -1.0, want[inner] == -1.0), f"{what}: holes differ"
    ok = inner & (want > 0)
    rel = np.abs(got[ok] - want[ok]) / want[ok]
    worst = float(rel.max()) if ok.any() else 0.0
    assert worst <= rel_tol, f"{what}: relative error {worst:.3g}"
    return worst


def hand_5x5(variant):
    """filter_input's regions need 6 columns; by hand: one jump (columns 3-4 are 0.4 m farther), one hole."""
    mm = np.array([[1000, 1003, 1001, 1400, 1404],
                   [1002, 0, 1004, 1402, 1401],
                   [1001, 1005, 1002, 1403, 1400],
                   [1004, 1002, 1003, 1401, 1405],
                   [1003, 1001, 1000, 1404, 1402]], np.int16)
    if variant == "centre_hole":  # the only interior pixel is the hole
        mm[1, 1], mm[2, 2] = 1003, 0
    return mm


def check_filter_image(api, mm, rel_tol=1e-5):
    H, W = mm.shape
    v = api.create_view(W, H)
    api.view_update(v, np.zeros((H, W, 4), np.uint8), mm, bilateral=True)
    got = api.download_view_depth(v).astype(np.float64)
    want = ref64.bilateral_update_view(ref64.depth_to_float(mm).astype(F))
    return _compare_filtered(got, want, rel_tol)


def check_filter_refused_below_5(api, err):
    """4 x 7 has no interior at all.  Both engines refuse the filter below 5 x 5 (include/dslam_fusion.h) rather than
    deliver the all-zero image upstream's loops would leave, and the view stays usable."""
    W, H = 4, 7
    mm = np.full((H, W), 1000, np.int16)
    v = api.create_view(W, H)
    rgba = np.zeros((H, W, 4), np.uint8)
    try:
        api.view_update(v, rgba, mm, bilateral=True)
    except err:
        pass
    else:
        raise AssertionError("a 4 x 7 image was filtered")
    api.view_update(v, rgba, mm)
    assert np.array_equal(api.download_view_depth(v), np.full((H, W), F(1000) * F(0.001), F))


# ---------------------------------------------------------------------------------------------------------------------
# depth post-processing
# ---------------------------------------------------------------------------------------------------------------------
def _pose(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(F)


POSES = {
    "identity": _pose(),
    "small": _pose(0.004, -0.006, 0.003, (0.01, -0.02, 0.05)),
    "large": _pose(0.08, -0.05, 0.1, (0.3, 0.1, -0.5)),
    "behind": _pose(0.0, 3.1, 0.0, (0.02, 0.0, -0.1)),  # half a turn about y: P2 < 0, the projection still lands inside
}
POST_SHAPES = [(1, 1), (63, 3), (64, 4), (65, 5), (130, 9)]  # (cols, rows): around the kernel's 64 x 4 tile
CURR_SPECIAL = np.array([-5, 0, 4, 5, 6, 7, -32768], np.int16)
PREV_SPECIAL = np.array([0, 4, 5, 6, 7, -1, -30000], np.int16)  # the negatives read back as 65.535 m and 35.536 m


def post_intrinsics(cols, rows):
    """The text pairs rows with (fx, cx): cx sits in the row range and fx scales with the rows, so that projections stay
    inside.  Integer principal points for odd sizes, half-integer ones for even sizes."""
    return (F(0.9 * max(rows, 2)), F(0.9 * max(cols, 2)), F((rows - 1) / 2.0), F((cols - 1) / 2.0))


def post_images(cols, rows, seed):
    """A sloping surface around 2 m.  The previous depth agrees with it to 2 % in the left half and is 8 % farther in
    the right half (either side of a 5 % threshold); both images carry the special values of the gates."""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:rows, 0:cols]
    curr = (2000 + 7 * rr + 3 * cc + rng.integers(-2, 3, (rows, cols))).astype(np.int16)
    far = cc >= cols // 2
    prev = np.where(far, curr * 1.08, curr * 1.02).astype(np.int16)
    n = rows * cols
    k = max(n // 6, min(n, 7) if n > 1 else 0)
    at = rng.permutation(n)
    curr.reshape(-1)[at[:k]] = CURR_SPECIAL[np.arange(k) % len(CURR_SPECIAL)]
    prev.reshape(-1)[at[k:2 * k]] = PREV_SPECIAL[np.arange(k) % len(PREV_SPECIAL)]
    return curr, prev


@functools.lru_cache(maxsize=None)
def post_cases():
    """name -> dict(cols, rows, curr, prev, Tpc, intr, threshold, area, floors).  `floors` are lower bounds on the reach
    counters of _post_reach, asserted on the reference alone."""
    cases = {}
    for cols, rows in POST_SHAPES + [(912, 228)]:
        for pose in POSES if (cols, rows) != (912, 228) else ["small"]:
            curr, prev = post_images(cols, rows, seed=cols * 7 + rows)
            area = 0.5 if rows in (3, 4) else 0.3  # 0.5 * 4 = 2 exactly: row 2 stays, row 3 can go
            floors = {}
            if rows >= 3:
                floors = dict(curr_negative=1, curr_zero=1, curr_4_5=1, curr_6_7=1)
            if rows >= 3 and pose == "identity":
                floors.update(counted=cols * rows // 3, blanked=1, kept_over_threshold_above_area=1, under_threshold=1,
                              prev_zero=1, prev_4_5=1, prev_6_7=1, prev_negative=1, row_u_0=1, row_u_1=1, row_u_last=1,
                              col_v_0=1, col_v_1=1, col_v_last=1)
                if rows == 4:
                    floors.update(area_edge_row_kept=1)
            if rows >= 5 and pose == "small":
                floors.update(counted=cols * rows // 3, blanked=1, under_threshold=1, row_u_0=1, col_v_0=1)
            if rows >= 3 and pose == "large":  # the scene comes 0.5 m closer: projections spread past rows and cols
                floors.update(counted=cols * rows // 8, outside=cols * rows // 8, row_u_rows=1, col_v_cols=1)
            if rows >= 3 and pose == "behind":
                floors.update(counted_behind=cols * rows // 4)
            cases[f"{cols}x{rows}_{pose}"] = dict(cols=cols, rows=rows, curr=curr, prev=prev, Tpc=POSES[pose],
                                                  intr=post_intrinsics(cols, rows), threshold=0.05, area=area, floors=floors)
    # P2 exactly 0: R = I and t_z = -z for the pixels at 2000 mm; on the row of cx (an integer) X = 0 too, and with
    # t_x = 0 the projection is 0 * inf = NaN.  The pixels at 20 m have P2 = 18 and project normally.
    cols, rows = 65, 5
    rng = np.random.default_rng(9)
    curr = np.where(rng.random((rows, cols)) < 0.6, 2000, 20000).astype(np.int16)
    prev = np.full((rows, cols), 16000, np.int16)
    z0 = F(np.float64(2000.0) / 1000.0)
    cases["65x5_p2_zero"] = dict(cols=cols, rows=rows, curr=curr, prev=prev, Tpc=_pose(t=(0.0, 0.0, -float(z0))),
                                 intr=post_intrinsics(cols, rows), threshold=0.05, area=0.0,
                                 floors=dict(p2_zero=100, nan_projection=20, counted=10, blanked=5))
    # exactly on both edges: identity, 1 m against 1.5 m (no operation rounds: q = 0.5 = the threshold, kept by the
    # strict >), 1.501 m (blanked) and 1.499 m (kept); 0.5 * 4 rows = 2 exactly, so row 2 is kept whatever q is and
    # only row 3 can be blanked; column 0 projects to col_v = 0 and is never compared
    cols, rows = 64, 4
    curr = np.full((rows, cols), 1000, np.int16)
    prev = np.tile(np.array([1500, 1501, 1499, 1500], np.int16), (rows, cols // 4))
    cases["64x4_exact_edges"] = dict(cols=cols, rows=rows, curr=curr, prev=prev, Tpc=_pose(), intr=post_intrinsics(cols, rows),
                                     threshold=0.5, area=0.5,
                                     floors=dict(q_equals_threshold=2 * cols // 4 - 1, blanked=cols // 4 - 1, area_edge_row_kept=cols // 4 - 1))
    # the matrix product accumulates in double and rounds once.  At pixel (row 2, col 1), with z = 1, fx = fy = 1 and
    # cx = cy = 1 - 2^-12: X = 1 + 2^-12 and Y = 2^-12 exactly.  Third row (1 + 2^-12, 2^-12, 0): the products are
    # 1 + 2^-11 + 2^-24 and 2^-24, their sum 1 + 2^-11 + 2^-23 is a float, and t_z is its negative, so P2 = 0 exactly in
    # float32 and in float64 alike (no tie) and the projection is NaN: not counted.  Rounding each product to float32
    # first gives 1 + 2^-11 twice over (round to even), P2 = -2^-23, and the pixel is counted.  Rows 0 and 1 of the
    # matrix are zero, so every other pixel projects onto (cx + 0.5, cy + 0.5) -> previous pixel (1, 1).
    cols, rows = 5, 4
    e = 2.0 ** -12
    T = np.zeros((4, 4), F)
    T[2, 0], T[2, 1], T[2, 3], T[3, 3] = 1 + e, e, -(1 + 2 * e + 2.0 ** -23), 1
    cases["5x4_double_accumulation"] = dict(cols=cols, rows=rows, curr=np.full((rows, cols), 1000, np.int16),
                                            prev=np.full((rows, cols), 1000, np.int16), Tpc=T,
                                            intr=(F(1), F(1), F(1 - e), F(1 - e)), threshold=0.05, area=0.0,
                                            floors=dict(p2_zero=1, nan_projection=1, counted=8))
    return cases


def _post_reach(c, info, tie):
    curr, prev, rows, cols = c["curr"], c["prev"], c["rows"], c["cols"]
    live, counted, inb, blank = info["live"], info["counted"], info["inb"], info["blank"]
    with np.errstate(all="ignore"):
        tu = np.where(np.isfinite(info["c"][0]), np.trunc(info["c"][0]), np.nan)
        tv = np.where(np.isfinite(info["c"][1]), np.trunc(info["c"][1]), np.nan)
        over = counted & (info["q"] > F(c["threshold"]))
    pr = info["prev_raw"]
    edge = float(F(c["area"]) * F(rows))
    rr = np.mgrid[0:rows, 0:cols][0]
    return dict(
        curr_negative=int((curr < 0).sum()), curr_zero=int((curr == 0).sum()),
        curr_4_5=int(((curr == 4) | (curr == 5)).sum()), curr_6_7=int((live & (curr <= 7)).sum()),
        counted=int(counted.sum()), blanked=int(blank.sum()), ties=int(tie.sum()),
        kept_over_threshold_above_area=int((over & ~info["area_ok"]).sum()),
        under_threshold=int((counted & ~over & info["area_ok"] & (info["P2"] > 0)).sum()),
        area_edge_row_kept=int((over & (rr == edge)).sum()) if edge == int(edge) else 0,
        prev_zero=int((inb & (pr == 0)).sum()), prev_4_5=int((inb & ((pr == 4) | (pr == 5))).sum()),
        prev_6_7=int((inb & ((pr == 6) | (pr == 7))).sum()), prev_negative=int((counted & (pr >= 32768)).sum()),
        row_u_0=int((live & (tu == 0)).sum()), row_u_1=int((live & (tu == 1)).sum()),
        row_u_last=int((live & (tu == rows - 1)).sum()), row_u_rows=int((live & (tu == rows)).sum()),
        col_v_0=int((live & (tv == 0)).sum()), col_v_1=int((live & (tv == 1)).sum()),
        col_v_last=int((live & (tv == cols - 1)).sum()), col_v_cols=int((live & (tv == cols)).sum()),
        outside=int((live & ~inb).sum()), counted_behind=int((counted & (info["P2"] < 0)).sum()),
        q_equals_threshold=int((counted & info["area_ok"] & (info["q"] == F(c["threshold"])) & ~tie).sum()),
        p2_zero=int((live & (info["P2"] == 0)).sum()),
        nan_projection=int((live & (np.isnan(info["c"][0]) | np.isnan(info["c"][1]))).sum()))


@functools.lru_cache(maxsize=None)
def post_reference(name):
    """Computed once per case and shared by the tests that need it; nothing writes to it."""
    c = post_cases()[name]
    return rv.depth_post_processing(c["curr"], c["prev"], c["Tpc"], c["intr"], c["threshold"], c["area"])


TIE_CAP = 0.02  # of the pixels that reach the comparison, per case


def check_post(api, name, device=False):
    """One case.  api=None: the reference alone (reach floors, the tie cap, and that every pixel at which the float32
    and float64 evaluations decide differently lies inside the tie mask)."""
    c = post_cases()[name]
    want, count, tie, reasons, info = post_reference(name)
    reach = _post_reach(c, info, tie)
    for k, floor in c["floors"].items():
        assert reach[k] >= floor, f"{name}: reach {k} = {reach[k]}, floor {floor}"
    assert not (info["differ"] & ~tie).any(), f"{name}: float32 and float64 decide differently outside the tie mask"
    assert reach["ties"] <= TIE_CAP * reach["counted"], f"{name}: {reach['ties']} ties for {reach['counted']} compared pixels"
    assert not (info["blank"] & (info["P2"] < 0)).any()
    if api is None:
        return reach
    if device:
        import torch
        tc, tp = torch.from_numpy(c["curr"].copy()).cuda(), torch.from_numpy(c["prev"].copy()).cuda()
        torch.cuda.synchronize()
        got_count = api.depth_post_processing_device(tc.data_ptr(), tp.data_ptr(), c["cols"], c["rows"], c["Tpc"], c["intr"],
                                                     c["threshold"], c["area"])
        api.synchronize()
        got = tc.cpu().numpy()
    else:
        got, got_count = api.depth_post_processing(c["curr"], c["prev"], c["Tpc"], c["intr"], c["threshold"], c["area"])
    assert np.array_equal(got[~tie], want[~tie]), f"{name}: {(got != want)[~tie].sum()} non-tie pixels differ"
    kept = got != 0
    assert np.array_equal(got[kept], c["curr"][kept]), f"{name}: a pixel that was not blanked changed"
    lo = int((info["counted"] & ~tie).sum())
    assert lo <= got_count <= lo + int(tie.sum()), f"{name}: count {got_count} outside [{lo}, {lo + int(tie.sum())}]"
    return reach


# ---------------------------------------------------------------------------------------------------------------------
# int16 depth output
# ---------------------------------------------------------------------------------------------------------------------
def check_depth_int16(api, pkg):
    """FloatDepthmapToShort (x1000) and FloatDepthmapToInt16 (x256) of a raycast of an analytic plane, against
    refview.depth_to_int16 of the float64 march's depth.  The depth agrees within 1e-4 m outside the march's ties; times
    1000 that is 0.1 of a unit (0.026 at 256), so truncation moves the integer by at most one."""
    W, H = 64, 48
    m = am.tilted_plane(num_buckets=0x40)
    M, intr = rc.camera(W, H, yaw=0.1, roll=0.3)
    scene, rs = rc.load_map(api, pkg, m, W, H)
    ref = ref64.cast_rays(m, M, intr, W, H)
    dref = np.where(ref["hit"], ref64.camera_depth(M, ref["p"], m.vs), 0.0)
    d = api.get_image(scene, rs, M, intr, pkg.IMAGE_DEPTH)
    out = {}
    for scale in (1000, 256):
        got = api.get_depth_image_int16(scene, rs, M, intr, scale)
        assert np.array_equal(got, (d * F(scale)).astype(np.int32).astype(np.int16)), "not the cast of the engine's own float image"
        want, _ = rv.depth_to_int16(dref.astype(F), scale)
        ok = ~ref["tie"]
        assert np.array_equal((got > 0)[ok], ref["hit"][ok]), f"scale {scale}: hit mask"
        both = ok & ref["hit"]
        assert both.sum() > 0.1 * W * H
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))[both]
        assert diff.max() <= 1, f"scale {scale}: off by {diff.max()}"
        out[scale] = dict(hits=int(both.sum()), off_by_one=int((diff == 1).sum()))
    return out
