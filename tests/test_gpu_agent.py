"""GPU (-m gpu): the simulated agent on the MI355X -- the checks of tests/agent_cases.py (references and cases are stated there) on the real
kernels, plus the closed loop through two rooms."""
import pytest

from tests import agent_cases as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ac.SOUP_SEEDS)
def test_random_soup(hip, seed):
    ac.check_soup(hip, seed)


def test_dyadic_room(hip):
    ac.check_room(hip)


def test_odd_sizes_and_meshes(hip):
    ac.check_odd_sizes(hip)


def test_capacity_and_allocation_guards(hip):
    ac.check_capacity_and_guards(hip)


def test_repeatable(hip):
    ac.check_repeatable(hip)


def test_refusals(hip):
    ac.check_refusals(hip)


def test_navgrid_erosion(hip):
    ac.check_navgrid_erosion(hip)


def test_judge_actions(hip):
    ac.check_judge_actions(hip)


def test_frames(hip):
    ac.check_frames(hip)


def test_closed_loop_short(hip):
    ac.check_closed_loop_short(hip)


def test_closed_loop_two_rooms(hip):
    ac.check_closed_loop_two_rooms(hip)
