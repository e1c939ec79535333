"""CPU (host-emulated kernels): the simulated agent (activesplat_amd/agent.py, activesplat_amd/explore.py; gs_mesh_navgrid).  The checks, their
references and cases: tests/agent_cases.py.  The same checks run on the MI355X in tests/test_gpu_agent.py."""
import pytest

from tests import agent_cases as ac


def test_the_restatement_meets_the_conditions_of_the_case_set():
    ac.check_reference_conditions()


def test_navgrid_has_no_cpu_fallback():
    ac.check_no_cpu_fallback()


@pytest.mark.parametrize("seed", ac.SOUP_SEEDS)
def test_emulated_random_soup(emu, seed):
    ac.check_soup(emu, seed)


def test_emulated_dyadic_room(emu):
    ac.check_room(emu)


def test_emulated_odd_sizes_and_meshes(emu):
    ac.check_odd_sizes(emu)


def test_emulated_capacity_and_allocation_guards(emu):
    ac.check_capacity_and_guards(emu)


def test_emulated_repeatable(emu):
    ac.check_repeatable(emu)


def test_emulated_refusals(emu):
    ac.check_refusals(emu)


def test_navgrid_erosion(emu):
    ac.check_navgrid_erosion(emu)


def test_agent_actions(emu, tmp_path):
    ac.check_agent(emu, tmp_path)


def test_agent_follows_the_sensor_poses(emu):
    ac.check_agent_follows_sensor_poses(emu)


def test_emulated_judge_actions(emu):
    ac.check_judge_actions(emu)


def test_emulated_frames(emu):
    ac.check_frames(emu)


def test_emulated_closed_loop_short(emu):
    ac.check_closed_loop_short(emu)
