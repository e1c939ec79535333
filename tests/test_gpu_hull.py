"""GPU (-m gpu): the on-device cluster hull volumes on the MI355X -- the checks of tests/hull_cases.py (references and tolerances are stated
there) on the real kernels.  Nothing here reads scipy or the reference: the fixture and the numpy restatement do."""
import pytest

from tests import hull_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(hc.small_cases()))
def test_small_cases(hip, name):
    hc.check_small(hip, name)


@pytest.mark.parametrize("seed", hc.cc.SEEDS)
def test_global_fields_match_scipy_and_the_reference(hip, seed):
    hc.check_global(hip, seed)


def test_refusals(hip):
    hc.check_refusals(hip)


def test_two_calls_are_bit_identical(hip):
    hc.check_repeatable(hip)


@pytest.mark.parametrize("K,zero_at", [(2, None), (5, 2)])
def test_global_invisibility_scores(hip, K, zero_at):
    hc.check_scores(hip, K, zero_at)


def test_scores_raise_when_the_cluster_table_is_too_small(hip):
    hc.check_scores_raise_when_truncated(hip)


def test_mapper_method(hip):
    hc.check_mapper(hip)
