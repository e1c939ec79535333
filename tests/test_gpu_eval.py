"""GPU (-m gpu): the map-quality evaluation on the MI355X -- the checks of tests/eval_cases.py (references and tolerances are stated there) on the
real kernels.  Nothing here reads the reference or scipy: the references are the fp64 torch restatements of tests/eval_cases.py."""
import pytest

from tests import eval_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W", ec.SMALL)
def test_sums_and_flags(hip, H, W):
    ec.check_sums_and_flags(hip, H, W)


@pytest.mark.parametrize("H,W", ec.SMALL)
def test_ssim_same(hip, H, W):
    ec.check_ssim_same(hip, H, W)


@pytest.mark.parametrize("H,W", ec.MS_SIZES)
def test_ms_ssim(hip, H, W):
    ec.check_ms_ssim(hip, H, W)


def test_clamp(hip):
    ec.check_clamp(hip)


def test_identities_and_ieee_rows(hip):
    ec.check_identities(hip)


def test_golden(hip):
    ec.check_golden(hip)


def test_two_evaluators_are_bit_identical(hip):
    ec.check_repeatable(hip)


def test_refusals_and_write(hip):
    ec.check_refusals_and_write(hip)


def test_evaluate_map_and_the_mapper_hook(hip):
    ec.check_evaluate_map(hip)


def test_evaluate_map_with_ms_ssim(hip):
    ec.check_evaluate_map_ms_ssim(hip)


def test_mapper_default_is_unchanged(hip):
    ec.check_mapper_default_is_unchanged(hip, deterministic_mapping=False)
