"""CPU: gs_set_forward_priority on the host-emulated kernels.  The emulator has no issue arbiter (its s_setprio does nothing), so this checks that
the estimate's control flow -- ballots, thresholds, the priority ladder, in every mode -- leaves each forward output bit-identical, on a scene
that asserts its own branches (tests/forward_priority_cases.py), and that the knob refuses what it does not take."""
import pytest

from tests import forward_priority_cases as fp


@pytest.mark.parametrize("fused", [False, True], ids=["dropin", "rgbd"])
def test_priority_modes_leave_the_forward_bit_identical(emu, fused):
    fp.check_bit_identical("cpu", fused)


def test_knob_refusals(emu):
    fp.check_refusals()
