"""The view path -- plain conversion, dataset formats, BGR->RGBA, every upload route, the bilateral filter at tile
edges, depthPostProcessing and the int16 depth output -- on the CPU oracle against the references of refview.py, which
were written from the text that defines these steps (check bodies in refview_checks.py, shared with
test_gpu_view_reference.py).  The reference-only tests assert what the cases reach and that they stay inside the tie
cap before any engine is in the loop."""
import pytest

import refview_checks as vc


@pytest.mark.parametrize("case", sorted(vc.post_cases()))
def test_post_processing_cases_reach_their_edges_from_the_reference_alone(case):
    reach = vc.check_post(None, case)
    print(f"{case}: {reach['ties']} ties of {reach['counted']} compared pixels; {({k: v for k, v in reach.items() if v})}")


@pytest.mark.parametrize("pair", sorted(vc.CONVERSION_PAIRS))
def test_plain_conversion_of_every_int16(oracle, pair):
    vc.check_conversion(oracle, pair)


@pytest.mark.parametrize("fmt,max_m", vc.DATASET_CASES)
def test_dataset_formats_of_every_int16(oracle, fmt, max_m):
    vc.check_dataset(oracle, fmt, max_m)


@pytest.mark.parametrize("W,H", vc.BGR_SHAPES)
def test_bgr_to_rgba(oracle, W, H):
    vc.check_bgr(oracle, W, H)


def test_every_upload_route_leaves_the_reference_view(oracle):
    done = vc.check_routes(oracle)
    assert len(done) == 8, done


@pytest.mark.parametrize("W,H", vc.FILTER_SIZES)
def test_bilateral_filter_at_tile_edges(oracle, W, H):
    print(f"{W}x{H}: worst relative error {vc.rc.check_view_filter(oracle, W, H, rel_tol=1e-5):.3g}")


@pytest.mark.parametrize("variant", ["hole_beside", "centre_hole"])
def test_bilateral_filter_5x5(oracle, variant):
    print(f"5x5 {variant}: worst relative error {vc.check_filter_image(oracle, vc.hand_5x5(variant)):.3g}")


def test_bilateral_filter_refused_without_interior(pkg, oracle):
    vc.check_filter_refused_below_5(oracle, pkg.DslamError)


@pytest.mark.parametrize("case", sorted(vc.post_cases()))
def test_depth_post_processing(oracle, case):
    vc.check_post(oracle, case)


def test_depth_image_int16_output(pkg, oracle):
    print(vc.check_depth_int16(oracle, pkg))
