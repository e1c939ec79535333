"""CPU (host-emulated kernels): the planner roadmap (activesplat_amd/roadmap.py; gs_traversable_map .. gs_trace_path).  The checks, their
references and cases: tests/roadmap_cases.py.  The same checks run on the MI355X in tests/test_gpu_roadmap.py."""
import numpy as np
import pytest
import torch

from tests import roadmap_cases as rc


def test_the_references_meet_the_conditions_of_the_case_set():
    rc.check_reference_conditions()


def test_pixel_world_round_trip():
    rc.check_pixel_world_round_trip()


def test_roadmap_has_no_cpu_fallback():
    from activesplat_amd import _lib
    from activesplat_amd import roadmap as RM
    _lib.unload_for_tests()
    cs = rc.case("48x40")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.traversable_map(torch.from_numpy(cs.free), torch.from_numpy(cs.unseen), cs.agent)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.grid_geodesic(torch.from_numpy(cs.free), cs.agent)
    with pytest.raises(TypeError):
        RM.clearance_field(np.asarray(cs.free))


@pytest.mark.parametrize("name", rc.CASES)
def test_emulated_stages(emu, name):
    rc.check_case(emu, name)


def test_emulated_two_doors(emu):
    rc.check_two_doors(emu)


def test_emulated_serpentine(emu):
    rc.check_serpentine(emu)


def test_emulated_repeatable(emu):
    rc.check_repeatable(emu)


def test_emulated_status_bits(emu):
    rc.check_status_bits(emu)


def test_emulated_refusals(emu):
    rc.check_refusals(emu)
