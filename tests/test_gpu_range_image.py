"""The visible list and the range image on the HIP engine against the law of ref_range.py (check bodies in
refrange_checks.py, shared with test_oracle_range_image.py, which also holds the reference-only tests of the fixtures):
SelFrustum / check_block_vis, project_single_block through each of its three producers (k_project_blocks, the selection
that projects as it lists, the front end adopted from the fusion launch) and every path of k_fill_range_tiles -- small
boxes, boxes taken by the whole workgroup, a second round over the list, the budget replay."""
import pytest

import range_fixtures as rf
import refrange_checks as chk

pytestmark = pytest.mark.gpu

CASES = sorted(rf.ALL_CASES)
BUDGETS = [(w, k) for w in ("close", "shell") for k in rf.BUDGET_KINDS]


@pytest.mark.parametrize("name", CASES)
def test_separate_calls(pkg, gpu, name):
    chk.check_separate_calls(gpu, pkg, rf.ALL_CASES[name]())


@pytest.mark.parametrize("name", CASES)
def test_get_image(pkg, gpu, name):
    chk.check_get_image(gpu, pkg, rf.ALL_CASES[name]())


@pytest.mark.parametrize("which,kind", BUDGETS)
def test_budget(pkg, gpu, which, kind):
    chk.check_budget(gpu, pkg, which, kind)


def test_fused(pkg, synth, gpu):
    assert chk.is_hip(gpu)
    chk.check_fused(gpu, pkg, synth)
