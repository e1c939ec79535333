"""GPU (-m gpu): the roadmap subregions on the MI355X -- the checks of tests/policy_cases.py (references and cases are stated there) on the
real kernels, plus plan_step under a SubregionPolicy through the rasteriser."""
import pytest

from tests import policy_cases as pc
from tests import roadmap_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", rc.CASES)
def test_node_distances(hip, name):
    pc.check_node_distances_case(hip, name)


def test_node_distances_two_doors(hip):
    pc.check_node_distances_two_doors(hip)


def test_node_distances_serpentine(hip):
    pc.check_node_distances_serpentine(hip)


def test_node_distances_small(hip):
    pc.check_node_distances_small(hip)


def test_node_distances_forced_paths(hip):
    pc.check_node_distances_paths(hip)


def test_segment_clearance(hip):
    pc.check_segment_clearance(hip)


def test_horizon_and_shortcut(hip):
    pc.check_horizon_and_shortcut(hip)


@pytest.mark.parametrize("key", [c[0] for c in pc.SUBREGION_CASES])
def test_subregions(hip, key):
    pc.check_subregions(hip, key)


def test_subregions_edges(hip):
    pc.check_subregions_edges(hip)


def test_repeatable(hip):
    pc.check_repeatable(hip)


def test_refusals(hip):
    pc.check_refusals(hip)


def test_mapper_plan_step_with_a_policy(hip):
    pc.check_mapper_plan_step_policy(hip)


def test_no_cpu_fallback_after_unload(hip):
    pc.check_no_cpu_fallback()
