"""GPU (-m gpu): TSDF fusion and surface extraction on the MI355X -- the checks of tests/volume_cases.py (restatements and bars are stated there)
on the real kernels."""
import pytest

from tests import volume_cases as vc

pytestmark = pytest.mark.gpu


def test_integration(hip):
    vc.check_integration(hip)


def test_batch_weight_cap_and_repeatability(hip):
    vc.check_batch_cap_repeat(hip)


def test_tails(hip):
    vc.check_tails(hip)


def test_extraction(hip):
    vc.check_extraction(hip)


def test_all_sign_patterns(hip):
    vc.check_all_sign_patterns(hip)


def test_random_volumes_are_manifold(hip):
    vc.check_random_volumes_are_manifold(hip)


def test_sphere(hip):
    vc.check_sphere(hip)


def test_sensor_loop(hip):
    vc.check_sensor_loop(hip)


def test_mapper(hip):
    vc.check_mapper(hip)


def test_refusals(hip):
    vc.check_refusals(hip)
