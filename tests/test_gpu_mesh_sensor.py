"""GPU (-m gpu): the mesh RGB-D sensor on the MI355X -- the checks of tests/mesh_cases.py (where the expected values come from is stated there)
on the real kernels."""
import pytest

from tests import mesh_cases as mc

pytestmark = pytest.mark.gpu


def test_random_scene(hip):
    mc.check_random_scene(hip)


def test_partial_tiles(hip):
    mc.check_partial_tiles(hip)


def test_closed_bumpy_room_is_watertight(hip):
    mc.check_closed_room(hip)


def test_near_plane_crossing(hip):
    mc.check_near_plane(hip)


def test_known_answers(hip):
    mc.check_known_answers(hip)


def test_capacity(hip):
    mc.check_capacity(hip)


def test_repeatable_and_order_independent(hip):
    mc.check_repeatable(hip)


def test_refusals(hip):
    mc.check_refusals(hip)


def test_sample_surface(hip):
    mc.check_sample_surface(hip)


def test_render_and_back_projection_round_trip(hip):
    mc.check_round_trip(hip)


def test_mapper_run_sensor(hip):
    mc.check_mapper(hip)
