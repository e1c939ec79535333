"""The blend kernels pixel by pixel and row by row at their rare branches, on the device (tests/blendpix_cases.py; the host-emulated twin is
tests/test_blendpix.py)."""
import pytest

from tests import blendpix_cases as bp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", bp.FEW)
def test_few_tile(hip, oracle64, oracle32, name):
    bp.check_few(name, hip, oracle64, oracle32)


@pytest.mark.parametrize("name", bp.MANY)
def test_many_tile(hip, oracle64, oracle32, name):
    bp.check_many(name, hip, oracle64, oracle32)


def test_segmented(hip, oracle64, oracle32):
    bp.check_segmented("few/segmented", hip, oracle64, oracle32)


@pytest.mark.parametrize("pieces", [3, 2])
def test_resumed_chained(hip, oracle64, oracle32, pieces):
    bp.check_chained("many/resumed", pieces, hip, oracle64, oracle32)


def test_deep_saturated_report_only(hip, oracle64, oracle32):
    bp.check_report_only("few/deep_saturated", hip, oracle64, oracle32)
