"""dslam_stereo_* and dslam_disparity_to_depth on the MI355X, everything bit for bit against
tests/ref_stereo.py: census, S and the disparity separately at every shape at which a kernel can still go wrong, the
parameter corners, the selection on crafted S volumes, the depth conversion over every disparity, the way into
dslam_view_update_device, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import ref_stereo as rs
import stereo_fixtures as sf
import util

pytestmark = pytest.mark.gpu

# (W, H, D): partial lanes in x and fewer rows than two census windows; two disparities per lane; W < D; odd sizes with
# diagonals of every length; one window; one pixel; more than one workgroup in every pass
SHAPES = [(80, 24, 64), (200, 20, 128), (48, 16, 64), (131, 37, 64), (9, 7, 64), (1, 1, 64), (320, 96, 128)]
CALIBS = [(480.0, 0.54, 1.0, 0.5, 30.0), (707.09, 0.537, 0.5, 0.0, 32.7)]
PATTERN = 0xA5A5


def params_of(pkg, encoded):
    return pkg.StereoParams(**encoded)


def dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).to("cuda:0")       # (a copy: the shared references are read-only)
    torch.cuda.synchronize()
    return t


def dev_pattern(n, dtype):
    import torch
    t = torch.full((n * np.dtype(dtype).itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def host(t, dtype, shape):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype).reshape(shape)


def check_stages(pkg, gpu, st, ref, disp, what):
    """The intermediate results of the most recent match, then the disparity: a failure names its stage."""
    assert np.array_equal(gpu.debug_stereo_download(st, pkg.STEREO_CENSUS_LEFT), ref["census_left"]), (what, "left census")
    assert np.array_equal(gpu.debug_stereo_download(st, pkg.STEREO_CENSUS_RIGHT), ref["census_right"]), (what, "right census")
    assert np.array_equal(gpu.debug_stereo_download(st, pkg.STEREO_S), ref["S"]), (what, "S")
    assert disp.dtype == np.uint16 and np.array_equal(disp, ref["disp"]), (what, "disparity")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the match, stage by stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D", SHAPES, ids=lambda v: str(v))
def test_every_stage_equals_the_reference(pkg, gpu, W, H, D):
    st = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=D)))
    for kind in ("shifted", "random"):
        ref = sf.reference(kind, W, H, max_disparity=D)
        disp = gpu.stereo_match(st, ref["left"], ref["right"])
        check_stages(pkg, gpu, st, ref, disp, kind)
        if kind == "shifted" and W >= 48:
            assert (ref["disp"] != rs.INVALID).mean() > 0.3   # (a match worth the name; the random pair is mostly rejected)
    # the device form gives the same, and so does a second match on the same handle
    ref = sf.reference("shifted", W, H, max_disparity=D)
    left, right, out = dev(ref["left"]), dev(ref["right"]), dev_pattern(W * H, np.uint16)
    for again in range(2):
        gpu.stereo_match_device(st, left.data_ptr(), right.data_ptr(), out.data_ptr())
        gpu.synchronize()
        check_stages(pkg, gpu, st, ref, host(out, np.uint16, (H, W)), ("device", again))
    st.close()


def test_two_handles_of_different_sizes_do_not_disturb_each_other(pkg, gpu):
    a, b = gpu.create_stereo(80, 24, params_of(pkg, dict(max_disparity=64))), gpu.create_stereo(200, 20, None)
    ra, rb = sf.reference("shifted", 80, 24, max_disparity=64), sf.reference("shifted", 200, 20, max_disparity=128)
    da = gpu.stereo_match(a, ra["left"], ra["right"])
    db = gpu.stereo_match(b, rb["left"], rb["right"])
    check_stages(pkg, gpu, a, ra, da, "a after b ran")      # a's intermediates are still a's
    check_stages(pkg, gpu, b, rb, db, "b")
    assert np.array_equal(gpu.stereo_match(a, ra["left"], ra["right"]), ra["disp"])
    assert gpu.stereo_get_params(b).as_dict() == rs.DEFAULTS
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. parameters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoded", [dict(p1=1, p2=1), dict(p1=192, p2=192), dict(uniqueness=-1), dict(uniqueness=99), dict(lr_max=-1),
                                     dict(lr_max=-2), dict(lr_max=64)], ids=lambda e: "-".join(f"{k}{v}" for k, v in e.items()))
def test_parameter_corners(pkg, gpu, encoded):
    W, H = 80, 24
    encoded = dict(encoded, max_disparity=64)
    st = gpu.create_stereo(W, H, params_of(pkg, encoded))
    assert st.params.effective() == rs.resolve(encoded)
    ref = sf.reference("shifted", W, H, **encoded)
    check_stages(pkg, gpu, st, ref, gpu.stereo_match(st, ref["left"], ref["right"]), encoded)
    base = sf.reference("shifted", W, H, max_disparity=64)
    if "p1" in encoded:
        assert not np.array_equal(ref["S"], base["S"])
        if encoded["p1"] == 192:
            assert ref["S"].max() > 8 * (63 + 120)            # beyond what the default penalties allow: no L_r wrapped at 255
    else:
        assert np.array_equal(ref["S"], base["S"]) and not np.array_equal(ref["disp"], base["disp"])
    st.close()


def test_rgba_equals_grey_of_the_same_images(pkg, gpu):
    W, H = 80, 24
    left4, right4 = sf.shifted_pair(W, H, 5, channels=4, seed=1)
    grey_l, grey_r = rs.grey(left4, 4).astype(np.uint8), rs.grey(right4, 4).astype(np.uint8)
    assert len(np.unique(left4[..., 0].astype(int) - left4[..., 1])) > 100     # a colour image, not three copies of one channel
    ref = rs.match(grey_l, grey_r, rs.resolve(dict(max_disparity=64)))
    st4 = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=64, channels=4)))
    st1 = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=64)))
    check_stages(pkg, gpu, st4, ref, gpu.stereo_match(st4, left4, right4), "rgba")
    check_stages(pkg, gpu, st1, ref, gpu.stereo_match(st1, grey_l, grey_r), "grey")
    st4.close(), st1.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the selection on crafted S
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_selection_corners_on_crafted_volumes(pkg, gpu, D):
    handles = {}
    for name, (S, u, lr) in sf.crafted(D).items():
        key = (S.shape[0], u, lr)
        if key not in handles:
            handles[key] = gpu.create_stereo(S.shape[1], S.shape[0], params_of(pkg, rs.encode(max_disparity=D, uniqueness=u, lr_max=lr)))
        got = gpu.debug_stereo_select(handles[key], S)
        assert np.array_equal(got, rs.select(S, u, lr)), name
    # ties everywhere, all filters on, more than one row and workgroup
    S = sf.random_S(D + 37, 5, D)
    st = gpu.create_stereo(D + 37, 5, params_of(pkg, dict(max_disparity=D)))
    want = rs.select(S, 5, 1)
    assert np.array_equal(gpu.debug_stereo_select(st, S), want) and 0.02 < (want != rs.INVALID).mean() < 0.98
    # values up to the top of uint16
    S = (sf.random_S(D + 37, 5, D, seed=1, levels=4000).astype(np.uint32) * 16 - 1600 + 1535).astype(np.uint16)
    assert S.max() > 60000
    assert np.array_equal(gpu.debug_stereo_select(st, S), rs.select(S, 5, 1))
    for h in list(handles.values()) + [st]:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. depth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calib", CALIBS, ids=lambda c: str(c[0]))
@pytest.mark.parametrize("D", [64, 128])
def test_depth_of_every_disparity(pkg, gpu, D, calib):
    d16 = np.concatenate([np.arange(16 * (D - 1) + 1), [rs.INVALID]]).astype(np.uint16)
    W, H = len(d16), 1
    st = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=D)))
    want = rs.depth_mm(d16, *calib).reshape(H, W)
    assert (want > 0).sum() > 16 * D // 2 and (want[0, :8] == 0).all()
    got = gpu.disparity_to_depth(st, d16, calib)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    src, out = dev(d16), dev_pattern(W * H, np.int16)
    gpu.disparity_to_depth_device(st, src.data_ptr(), calib, out.data_ptr())
    gpu.synchronize()
    assert np.array_equal(host(out, np.int16, (H, W)), want)
    st.close()


def test_stereo_depth_is_match_then_conversion(pkg, gpu):
    W, H, D = 131, 37, 64
    ref = sf.reference("shifted", W, H, max_disparity=D)
    calib = (60.0, 0.1, 1.0, 0.2, 3.0)
    want = rs.depth_mm(ref["disp"], *calib)
    assert (want > 0).mean() > 0.3
    st = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=D)))
    depth, disp = gpu.stereo_depth(st, ref["left"], ref["right"], calib)
    assert np.array_equal(disp, ref["disp"]) and np.array_equal(depth, want)
    depth, disp = gpu.stereo_depth(st, ref["left"], ref["right"], calib, want_disp=False)
    assert disp is None and np.array_equal(depth, want)
    left, right = dev(ref["left"]), dev(ref["right"])
    for with_disp in (True, False):
        d_out, z_out = dev_pattern(W * H, np.uint16), dev_pattern(W * H, np.int16)
        gpu.stereo_depth_device(st, left.data_ptr(), right.data_ptr(), calib, z_out.data_ptr(), d_out.data_ptr() if with_disp else None)
        gpu.synchronize()
        assert np.array_equal(host(z_out, np.int16, (H, W)), want), with_disp
        assert np.array_equal(host(d_out, np.uint16, (H, W)), ref["disp"] if with_disp else np.full((H, W), PATTERN, np.uint16))
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing: the depth image goes straight into the view
# ---------------------------------------------------------------------------------------------------------------------
def test_the_depth_image_feeds_view_update_device(pkg, gpu, synth):
    W, H, D = 80, 24, 64
    wl = synth.s_room(W, H, scale=4.0)
    calib = (60.0, 0.1, 1.0, 0.2, 3.0)                       # disparity 5 px -> 1.2 m, inside the room's frustum
    ref = sf.reference("shifted", W, H, max_disparity=D)
    want = rs.depth_mm(ref["disp"], *calib)
    rgba, _, M = wl.frame(0)
    st = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=D)))
    left, right, colour, depth = dev(ref["left"]), dev(ref["right"]), dev(rgba), dev_pattern(W * H, np.int16)
    snaps = []
    for route in ("device", "host"):
        scene = gpu.create_scene(util.small_params(pkg, wl))
        rstate = gpu.create_render_state(scene, W, H)
        view = gpu.create_view(W, H)
        if route == "device":
            gpu.stereo_depth_device(st, left.data_ptr(), right.data_ptr(), calib, depth.data_ptr())
            gpu.view_update_device(view, colour.data_ptr(), depth.data_ptr())
        else:
            gpu.view_update(view, rgba, want)
        gpu.process_frame(scene, view, rstate, M, wl.intr)
        snaps.append(util.snapshot(gpu, scene, rstate))
        for h in (view, rstate, scene):
            h.close()
    assert np.array_equal(host(depth, np.int16, (H, W)), want)
    assert snaps[1]["stats"]["no_visible_entries"] > 10          # a map was built
    util.assert_same_state(snaps[0], snaps[1], "stereo depth on the device vs the same image through the host")
    st.close()


def test_a_matcher_outlives_its_engine(pkg, gpu):
    base = gpu.debug_live_engines()
    api = pkg.open_engine(0)
    st = api.create_stereo(48, 16, params_of(pkg, dict(max_disparity=64)))
    ref = sf.reference("shifted", 48, 16, max_disparity=64)
    assert np.array_equal(api.stereo_match(st, ref["left"], ref["right"]), ref["disp"])
    api.close()
    assert gpu.debug_live_engines() == base + 1
    st.close()
    assert gpu.debug_live_engines() == base


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument checks: the error, and nothing written
# ---------------------------------------------------------------------------------------------------------------------
def test_create_rejects_what_the_header_says(pkg, gpu):
    base = gpu.debug_live_engines()
    for W, H in ((0, 8), (8, 0), (4097, 8), (8, 4097), (-1, 8)):
        with pytest.raises(pkg.DslamError):
            gpu.create_stereo(W, H)
    for bad in (dict(max_disparity=96), dict(max_disparity=32), dict(p1=11, p2=10), dict(p2=193), dict(p1=-1), dict(uniqueness=100),
                dict(uniqueness=-2), dict(lr_max=-3), dict(lr_max=65, max_disparity=64), dict(lr_max=129), dict(channels=2), dict(channels=3)):
        with pytest.raises(ValueError):
            rs.resolve(bad)
        with pytest.raises(pkg.DslamError):
            gpu.create_stereo(16, 8, params_of(pkg, bad))
    p = pkg.StereoParams()
    p.pad[1] = 1
    with pytest.raises(pkg.DslamError):
        gpu.create_stereo(16, 8, p)
    h = C.c_void_p()
    assert gpu._fn("stereo_create")(gpu._engine, C.c_int(16), C.c_int(8), None, None) == -1
    assert gpu._fn("stereo_create")(None, C.c_int(16), C.c_int(8), None, C.byref(h)) == -1 and not h.value
    assert gpu.debug_live_engines() == base


def test_calls_reject_bad_arguments_and_write_nothing(pkg, gpu):
    W, H, D = 48, 16, 64
    st = gpu.create_stereo(W, H, params_of(pkg, dict(max_disparity=D)))
    ref = sf.reference("shifted", W, H, max_disparity=D)
    with pytest.raises(pkg.DslamError):
        gpu.debug_stereo_download(st, pkg.STEREO_S)                      # nothing matched yet
    good = (480.0, 0.54, 1.0, 0.5, 30.0)
    bad_calibs = [(480.0, 0.54, 1.0, 0.5, 33.0), (480.0, 0.54, 1.0, 0.5, 32.767001), (0.0, 0.54, 1.0, 0.5, 30.0), (480.0, -0.54, 1.0, 0.5, 30.0),
                  (480.0, 0.54, float("nan"), 0.5, 30.0), (480.0, 0.54, 1.0, -0.5, 30.0), (480.0, 0.54, 1.0, 5.0, 3.0),
                  (float("inf"), 0.54, 1.0, 0.5, 30.0)]
    disp = np.full((H, W), PATTERN, np.uint16)
    depth = np.full((H, W), PATTERN, np.uint16).view(np.int16)
    left, right = dev(ref["left"]), dev(ref["right"])
    d_out, z_out = dev_pattern(W * H, np.uint16), dev_pattern(W * H, np.int16)

    def untouched():
        assert (disp == PATTERN).all() and (depth.view(np.uint16) == PATTERN).all()
        assert (host(d_out, np.uint16, (H, W)) == PATTERN).all() and (host(z_out, np.uint16, (H, W)) == PATTERN).all()

    for calib in bad_calibs:
        with pytest.raises(pkg.DslamError):
            gpu.disparity_to_depth(st, ref["disp"], calib, out=depth)
        with pytest.raises(pkg.DslamError):
            gpu.stereo_depth(st, ref["left"], ref["right"], calib, depth_out=depth, disp_out=disp)
        with pytest.raises(pkg.DslamError):
            gpu.disparity_to_depth_device(st, d_out.data_ptr(), calib, z_out.data_ptr())
        with pytest.raises(pkg.DslamError):
            gpu.stereo_depth_device(st, left.data_ptr(), right.data_ptr(), calib, z_out.data_ptr(), d_out.data_ptr())
        untouched()
    # misaligned device addresses
    with pytest.raises(pkg.DslamError):
        gpu.stereo_match_device(st, left.data_ptr() + 1, right.data_ptr(), d_out.data_ptr())
    with pytest.raises(pkg.DslamError):
        gpu.stereo_match_device(st, left.data_ptr(), right.data_ptr(), d_out.data_ptr() + 2)
    with pytest.raises(pkg.DslamError):
        gpu.stereo_depth_device(st, left.data_ptr(), right.data_ptr(), good, z_out.data_ptr() + 2, d_out.data_ptr())
    # NULL pointers
    lp, rp, dp, zp = (a.ctypes.data_as(C.c_void_p) for a in (ref["left"], ref["right"], disp, depth))
    cal = C.byref(pkg.StereoCalib(*good))
    e, s = gpu._engine, st.ptr
    for name, args in (("stereo_match", (e, s, None, rp, dp)), ("stereo_match", (e, s, lp, None, dp)), ("stereo_match", (e, s, lp, rp, None)),
                       ("stereo_match", (None, s, lp, rp, dp)), ("stereo_match", (e, None, lp, rp, dp)),
                       ("stereo_match_device", (e, s, None, C.c_void_p(right.data_ptr()), C.c_void_p(d_out.data_ptr()))),
                       ("stereo_match_device", (e, s, C.c_void_p(left.data_ptr()), C.c_void_p(right.data_ptr()), None)),
                       ("disparity_to_depth", (e, s, None, cal, zp)), ("disparity_to_depth", (e, s, dp, None, zp)),
                       ("disparity_to_depth", (e, s, dp, cal, None)), ("disparity_to_depth_device", (e, s, None, cal, C.c_void_p(z_out.data_ptr()))),
                       ("stereo_depth", (e, s, lp, rp, None, zp, dp)), ("stereo_depth", (e, s, lp, rp, cal, None, dp)),
                       ("stereo_depth", (e, s, None, rp, cal, zp, dp)),
                       ("stereo_depth_device", (e, s, C.c_void_p(left.data_ptr()), C.c_void_p(right.data_ptr()), cal, None, None)),
                       ("debug_stereo_download", (e, s, C.c_int(2), None)), ("debug_stereo_select", (e, s, None, dp)),
                       ("debug_stereo_select", (e, s, dp, None)), ("stereo_get_params", (s, None)), ("stereo_get_params", (None, cal))):
        assert gpu._fn(name)(*args) == -1, (name, args)
    untouched()
    # a handle used on another engine
    other = pkg.open_engine(0)
    for call in (lambda: other.stereo_match(st, ref["left"], ref["right"], out=disp),
                 lambda: other.stereo_match_device(st, left.data_ptr(), right.data_ptr(), d_out.data_ptr()),
                 lambda: other.disparity_to_depth(st, ref["disp"], good, out=depth),
                 lambda: other.stereo_depth(st, ref["left"], ref["right"], good, depth_out=depth, disp_out=disp),
                 lambda: other.debug_stereo_select(st, np.zeros((H, W, D), np.uint16), out=disp),
                 lambda: other.debug_stereo_download(st, pkg.STEREO_S)):
        with pytest.raises(pkg.DslamError):
            call()
    other.close()
    untouched()
    # an unknown `what`, and the handle is none the worse for any of it
    assert np.array_equal(gpu.stereo_match(st, ref["left"], ref["right"]), ref["disp"])
    for what in (-1, 3):
        assert gpu._fn("debug_stereo_download")(e, s, C.c_int(what), dp) == -1
    assert gpu._fn("stereo_destroy")(None) == 0
    st.close()
