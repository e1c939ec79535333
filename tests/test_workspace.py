"""CPU: every entry of tests/workspace_cases.py on the host-emulated kernels inside guarded_allocations -- bands around every allocation,
padding of the published layouts, const inputs -- under all four interior fills: as allocated, NaN in float tensors, byte 0xFF and byte 0x5A in
every empty* allocation.  The wrapped checks keep their own bars.  tests/test_gpu_workspace.py runs the table on the device (NaN fill)."""
import pytest

from tests import workspace_cases as W

FILLS = [("none", 0), ("float_nan", 0), ("bytes", 0xFF), ("bytes", 0x5A)]
EMULATED = [e for e in W.ENTRIES if e.emulated]


def test_the_table_names_every_family():
    assert W.FAMILIES == sorted(["dropin", "optimistic_miss", "rgbd", "topdown", "losses", "optim", "growth", "rows", "stats", "planner", "sensing"])
    assert len({(e.family, e.name) for e in W.ENTRIES}) == len(W.ENTRIES)


@pytest.mark.parametrize("poison,byte", FILLS, ids=["none", "float_nan", "bytes_ff", "bytes_5a"])
@pytest.mark.parametrize("e", EMULATED, ids=[f"{e.family}-{e.name}" for e in EMULATED])
def test_emulated_workspace(emu, oracle32, oracle64, e, poison, byte):
    n, _regions, _const = W.run_entry(e, emu, poison, oracle32, oracle64, byte=byte)
    assert n > 0
