"""GPU (-m gpu): the forward blend with its walkers' issue priority off and in every mode of gs_set_forward_priority -- colour, depth, opacity,
radii, final_T and n_contrib are bit-identical (tests/forward_priority_cases.py; no gradient check: the order of the backward's atomics is not
fixed, and the existing suites cover the backward)."""
import pytest

from tests import forward_priority_cases as fp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", [False, True], ids=["dropin", "rgbd"])
def test_priority_modes_leave_the_forward_bit_identical(hip, fused):
    fp.check_bit_identical(hip, fused)
