"""GPU (-m gpu): the entries of tests/workspace_cases.py on the MI355X inside guarded_allocations, float allocations poisoned with NaN (the byte
fills belong to the emulated build: an uninitialised index has to fault on a CPU), and the harness self-test on the device.  The emulated
variants of the same entries (tests/test_workspace.py) run under all four fills on every CPU run of the suite."""
import pytest

from tests import guard_selftest as S
from tests import workspace_cases as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.CASES)
def test_gpu_guard(hip, case):
    getattr(S, "check_" + case)(hip)


@pytest.mark.parametrize("e", W.ENTRIES, ids=[f"{e.family}-{e.name}" for e in W.ENTRIES])
def test_gpu_workspace(hip, oracle32, oracle64, e):
    n, _regions, _const = W.run_entry(e, hip, "float_nan", oracle32, oracle64)
    assert n > 0
