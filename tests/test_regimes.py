"""CPU: the size regimes of tests/regime_cases.py on the host-emulated kernels (tests/hipemu) -- tile lists of exactly a sort threshold's length and
one more, blend lists of exactly a chunk multiple and its neighbours, images of 2049 .. 8192 tiles on the LDS path, the radix path past its
one-trip sizes.  tests/test_gpu_regimes.py runs the same cases on the device."""
import pytest

from tests import regime_cases as rc


@pytest.mark.parametrize("case", list(rc.SORT_CASES))
def test_emulated_sort_selection_boundaries(emu, oracle32, case):
    rc.check_sort_boundary(case, emu, oracle32)


@pytest.mark.parametrize("grid", list(rc.BLEND_GRIDS))
def test_emulated_blend_chunk_edges(emu, oracle32, oracle64, grid):
    rc.check_blend_edges(grid, emu, oracle32, oracle64)


@pytest.mark.parametrize("case", list(rc.LARGE_CASES))
def test_emulated_large_images_and_counts(emu, oracle32, oracle64, case):
    rc.check_large(case, emu, oracle32, oracle64)
