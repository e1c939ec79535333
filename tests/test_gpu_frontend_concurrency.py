"""GPU: the drop-in call's per-(thread, device, stream) state on the MI355X -- side streams, a second Python thread of this process, and the
64-entry evictions of the stream and layout tables (tests/frontend_cases.py, section C), through the C++ front-end and through the Python twin."""
import pytest

from tests import frontend_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[True, False], ids=["frontend", "twin"])
def route(request, hip):
    if request.param:
        from activesplat_amd import _frontend
        _frontend.get()                                      # (the run is about the C++ route: no quiet use of the twin)
    return request.param


def test_two_side_streams(hip, route):
    fc.check_two_side_streams(hip, route)


@pytest.mark.parametrize("side_stream", [True, False], ids=["side_stream", "default_stream"])
def test_two_threads(hip, route, side_stream):
    fc.check_two_threads(hip, route, side_stream)


def test_stream_table_eviction(hip, route):
    fc.check_stream_table_eviction(hip, route)


def test_layout_table_eviction(hip, route):
    fc.check_layout_table_eviction(hip, route)
