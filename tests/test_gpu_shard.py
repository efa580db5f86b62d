"""Shard ownership and the dirty-block exchange on the HIP engine against the law of ref_shard.py (check bodies in
refshard_checks.py, shared with test_oracle_shard.py, which also holds the reference-only tests of the law and the
fixtures): k_dirty_permute, k_dirty_counts, k_dirty_pack, k_dirty_unpack and the ordered compaction on chosen dirty sets,
with guard blocks around every buffer; the ownership gate and the dirty mark of k_integrate (its general, streaming,
two-camera and de-integrating forms) and of k_reintegrate_blocks (unit and depth weights) on real calls."""
import pytest

import refshard_checks as chk
import shard_fixtures as sf

pytestmark = pytest.mark.gpu

EXCHANGES = [(l, d) for l in sf.LAYOUTS for d in sf.DIRTY_SETS]


@pytest.mark.parametrize("layout,which", EXCHANGES)
def test_exchange(pkg, gpu, layout, which):
    assert sf.is_hip(gpu)
    print(chk.check_exchange(gpu, pkg, layout, which))


def test_refusals(pkg, gpu):
    chk.check_refusals(gpu, pkg)


@pytest.fixture(scope="module")
def twins(pkg, synth, gpu):
    return chk.Twins(gpu, pkg, synth)


@pytest.mark.parametrize("setting", chk.SETTINGS)
@pytest.mark.parametrize("form", chk.FORMS)
def test_real_call(pkg, synth, gpu, twins, form, setting):
    chk.check_real_call(gpu, pkg, synth, twins[form], form, setting)


def test_world_of_three(pkg, synth, gpu, twins):
    chk.check_world_of_three(gpu, pkg, synth, twins["batch_unit"])
