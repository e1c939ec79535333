"""CPU: the roadmap subregions on the host-emulated kernels (roadmap.node_distances, segment_clearance, nodes_in_horizon, shortcut_path,
subregions; gs_node_distances, gs_segment_clearance, gs_subregions) and the host-side target choice (activesplat_amd/policy.py).  The checks,
their references and cases: tests/policy_cases.py.  The device checks run again on the MI355X in tests/test_gpu_policy.py."""
import pytest

from tests import policy_cases as pc
from tests import roadmap_cases as rc


def test_the_references_meet_the_conditions_of_the_case_set():
    pc.check_subregion_conditions()


def test_the_line_rule_restated():
    pc.check_line_rule()


@pytest.mark.parametrize("key", [c[0] for c in pc.SUBREGION_CASES])
def test_restatement_scipy_and_the_reference_agree(key):
    pc.check_subregion_restatement(key)


def test_node_scores():
    pc.check_node_scores()


def test_choose_branch_by_branch():
    pc.check_choose()


def test_subregions_have_no_cpu_fallback():
    pc.check_no_cpu_fallback()


@pytest.mark.parametrize("name", rc.CASES)
def test_emulated_node_distances(emu, name):
    pc.check_node_distances_case(emu, name)


def test_emulated_node_distances_two_doors(emu):
    pc.check_node_distances_two_doors(emu)


def test_emulated_node_distances_serpentine(emu):
    pc.check_node_distances_serpentine(emu)


def test_emulated_node_distances_small(emu):
    pc.check_node_distances_small(emu)


def test_emulated_node_distances_forced_paths(emu):
    pc.check_node_distances_paths(emu)


def test_emulated_segment_clearance(emu):
    pc.check_segment_clearance(emu)


def test_emulated_horizon_and_shortcut(emu):
    pc.check_horizon_and_shortcut(emu)


@pytest.mark.parametrize("key", [c[0] for c in pc.SUBREGION_CASES])
def test_emulated_subregions(emu, key):
    pc.check_subregions(emu, key)


def test_emulated_subregions_edges(emu):
    pc.check_subregions_edges(emu)


def test_emulated_repeatable(emu):
    pc.check_repeatable(emu)


def test_emulated_refusals(emu):
    pc.check_refusals(emu)
