"""GPU (-m gpu): textures of the mesh RGB-D sensor on the MI355X -- the checks of tests/texture_cases.py (where the expected values come from is
stated there) on the real kernels."""
import pytest

from tests import texture_cases as tc

pytestmark = pytest.mark.gpu


def test_mip_chains(hip):
    tc.check_mip_chains(hip)


def test_random_textured_scene(hip):
    tc.check_random_scene(hip)


def test_cases_worked_by_hand(hip):
    tc.check_worked_by_hand(hip)


def test_grazing_floor(hip):
    tc.check_grazing(hip)


def test_identity_with_the_untextured_render(hip):
    tc.check_identity(hip)


def test_guarded_abi_call_and_refusals(hip):
    tc.check_guarded_abi(hip)


def test_repeatable_and_texture_order_independent(hip):
    tc.check_repeatable(hip)


def test_python_validation(hip):
    tc.check_python_validation(hip)


def test_sensor_and_mapper(hip):
    tc.check_sensor_and_mapper(hip)
