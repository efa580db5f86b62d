"""The view path on the HIP engine against the references of refview.py (check bodies in refview_checks.py, shared
with test_oracle_view_reference.py): the same cases as on the oracle, plus the device-resident entry points."""
import pytest

import refview_checks as vc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pair", sorted(vc.CONVERSION_PAIRS))
def test_plain_conversion_of_every_int16(gpu, pair):
    vc.check_conversion(gpu, pair)


@pytest.mark.parametrize("fmt,max_m", vc.DATASET_CASES)
def test_dataset_formats_of_every_int16(gpu, fmt, max_m):
    vc.check_dataset(gpu, fmt, max_m)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("W,H", vc.BGR_SHAPES)
def test_bgr_to_rgba(gpu, W, H, device):
    vc.check_bgr(gpu, W, H, device=device)


def test_bgr_device_image_must_be_dword_aligned(pkg, gpu):
    """k_bgr_to_rgba loads dwords from the image; the entry point refuses a pointer that is not 4-byte aligned before
    anything is launched (include/dslam_fusion.h), and the view keeps what it held."""
    import numpy as np
    import torch
    W, H = 8, 4
    v = gpu.create_view(W, H)
    rgba = np.full((H, W, 4), 9, np.uint8)
    mm = np.full((H, W), 1000, np.int16)
    gpu.view_update(v, rgba, mm)
    buf, t_mm = torch.zeros(W * H * 3 + 8, dtype=torch.uint8).cuda(), torch.from_numpy(mm).cuda()
    torch.cuda.synchronize()
    for off in (1, 2, 3):
        with pytest.raises(pkg.DslamError, match="aligned"):
            gpu.view_update_bgr_device(v, buf.data_ptr() + off, t_mm.data_ptr())
    assert np.array_equal(gpu.download_view_rgba(v), rgba)


def test_every_upload_route_leaves_the_reference_view(gpu):
    done = vc.check_routes(gpu, device_routes=True)
    assert len(done) == 10, done


@pytest.mark.parametrize("W,H", vc.FILTER_SIZES)
def test_bilateral_filter_at_tile_edges(gpu, W, H):
    print(f"{W}x{H}: worst relative error {vc.rc.check_view_filter(gpu, W, H, rel_tol=1e-5):.3g}")


@pytest.mark.parametrize("variant", ["hole_beside", "centre_hole"])
def test_bilateral_filter_5x5(gpu, variant):
    print(f"5x5 {variant}: worst relative error {vc.check_filter_image(gpu, vc.hand_5x5(variant)):.3g}")


def test_bilateral_filter_refused_without_interior(pkg, gpu):
    vc.check_filter_refused_below_5(gpu, pkg.DslamError)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", sorted(vc.post_cases()))
def test_depth_post_processing(gpu, case, device):
    vc.check_post(gpu, case, device=device)


def test_depth_image_int16_output(pkg, gpu):
    print(vc.check_depth_int16(gpu, pkg))
