"""GPU (-m gpu): the size regimes of tests/regime_cases.py on the device -- tile lists of exactly a sort threshold's length and one more, blend
lists of exactly a chunk multiple and its neighbours, images of 2049 .. 8192 tiles on the LDS path, the radix path past its one-trip sizes.
Same cases, same bars as tests/test_regimes.py (the emulated kernels)."""
import pytest

from tests import regime_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(rc.SORT_CASES))
def test_sort_selection_boundaries(hip, oracle32, case):
    rc.check_sort_boundary(case, hip, oracle32)


@pytest.mark.parametrize("grid", list(rc.BLEND_GRIDS))
def test_blend_chunk_edges(hip, oracle32, oracle64, grid):
    rc.check_blend_edges(grid, hip, oracle32, oracle64)


@pytest.mark.parametrize("case", list(rc.LARGE_CASES))
def test_large_images_and_counts(hip, oracle32, oracle64, case):
    rc.check_large(case, hip, oracle32, oracle64)
