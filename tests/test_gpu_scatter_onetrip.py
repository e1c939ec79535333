"""GPU (-m gpu): the one-trip scatter pass of tile binning against the fp32 oracle (tests/scatter_onetrip_cases.py)."""
import pytest

from tests import scatter_onetrip_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", sc.SIZES)
def test_sizes(hip, oracle32, P):
    sc.check_size(P, hip, oracle32)


def test_large_rects_take_the_emitter(hip, oracle32):
    sc.check_large_rects(hip, oracle32)


def test_culled_rows_over_garbage(hip, oracle32):
    sc.check_culled_rows_over_garbage(hip, oracle32)


def test_pile_on_one_tile(hip, oracle32):
    sc.check_pile_on_one_tile(hip, oracle32)


def test_odd_tile_count(hip, oracle32):
    sc.check_odd_tile_count(hip, oracle32)


def test_more_tiles_than_cursor_rounds(hip, oracle32):
    sc.check_more_tiles_than_cursor_rounds(hip, oracle32)


def test_cov3d_precomp(hip, oracle32):
    sc.check_cov3d_precomp(hip, oracle32)


def test_backward(hip, oracle64, oracle32):
    sc.check_backward(hip, oracle64, oracle32)
