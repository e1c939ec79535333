"""GPU (-m gpu): the planner roadmap on the MI355X -- the checks of tests/roadmap_cases.py (references and cases are stated there) on the real
kernels, plus the two that need the rasteriser."""
import pytest

from tests import roadmap_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", rc.CASES)
def test_stages(hip, name):
    rc.check_case(hip, name)


def test_two_doors(hip):
    rc.check_two_doors(hip)


def test_serpentine(hip):
    rc.check_serpentine(hip)


def test_repeatable(hip):
    rc.check_repeatable(hip)


def test_status_bits(hip):
    rc.check_status_bits(hip)


def test_refusals(hip):
    rc.check_refusals(hip)


def test_a_gaussian_lands_on_the_pixel_world_to_pixel_names(hip):
    rc.check_gaussian_lands_on_its_pixel(hip)


def test_mapper_roadmap_and_plan_step(hip):
    rc.check_mapper_plan_step(hip)
