"""GPU (-m gpu): the completion / accuracy judge on the MI355X -- the checks of tests/completion_cases.py (references and tolerances are stated
there) on the real kernels.  Nothing here reads scipy or the reference: the numpy restatements do."""
import pytest

from tests import completion_cases as cc

pytestmark = pytest.mark.gpu


def test_exact_arithmetic(hip):
    cc.check_exact(hip)


def test_remainders(hip):
    cc.check_remainders(hip)


def test_large_coordinates(hip):
    cc.check_large_coordinates(hip)


def test_depth_cloud(hip):
    cc.check_depth_cloud(hip)


def test_validity_frames(hip):
    cc.check_validity_frames(hip)


def test_running_state(hip):
    cc.check_running_state(hip)


def test_two_judges_are_bit_identical(hip):
    cc.check_repeatable(hip)


def test_map_distances(hip):
    cc.check_map_distances(hip)


def test_mapper_with_and_without_a_judge(hip):
    cc.check_mapper(hip, deterministic_mapping=False)


def test_refusals_and_write(hip):
    cc.check_refusals_and_write(hip)
