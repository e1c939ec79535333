"""CPU: the one-trip scatter pass of tile binning on the host-emulated kernels, against the fp32 oracle (tests/scatter_onetrip_cases.py)."""
import pytest

from tests import scatter_onetrip_cases as sc


@pytest.mark.parametrize("P", sc.SIZES)
def test_sizes(emu, oracle32, P):
    sc.check_size(P, "cpu", oracle32)


def test_large_rects_take_the_emitter(emu, oracle32):
    sc.check_large_rects("cpu", oracle32)


def test_culled_rows_over_garbage(emu, oracle32):
    sc.check_culled_rows_over_garbage("cpu", oracle32)


def test_pile_on_one_tile(emu, oracle32):
    sc.check_pile_on_one_tile("cpu", oracle32)


def test_odd_tile_count(emu, oracle32):
    sc.check_odd_tile_count("cpu", oracle32)


def test_more_tiles_than_cursor_rounds(emu, oracle32):
    sc.check_more_tiles_than_cursor_rounds("cpu", oracle32)


def test_cov3d_precomp(emu, oracle32):
    sc.check_cov3d_precomp("cpu", oracle32)


def test_backward(emu, oracle64, oracle32):
    sc.check_backward("cpu", oracle64, oracle32)
