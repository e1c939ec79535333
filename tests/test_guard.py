"""Self-test of tests/guard.py on the host: detection is proven with plain in-bounds torch writes through the BASE tensor of a guarded
allocation -- no kernel, emulated or real, is asked to overrun anything.  tests/test_gpu_workspace.py repeats the cases on the device."""
import pytest
import torch

from tests import guard_selftest as S


@pytest.mark.parametrize("case", S.CASES)
def test_guard(case):
    getattr(S, "check_" + case)("cpu")


def test_bytes_poison_is_refused_on_a_gpu_device():
    with pytest.raises(ValueError, match="host-emulated build only"):
        S.G.guarded_allocations(torch.device("cuda", 0), poison="bytes")
