"""The per-Gaussian backward row by row at its rare branches, on the device (tests/rowgrad_cases.py; the host-emulated twin is
tests/test_rowgrad.py)."""
import pytest

from tests import rowgrad_cases as rg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", rg.SCENES)
def test_rows(hip, oracle64, oracle32, name):
    rg.check_scene(name, hip, oracle64, oracle32)


@pytest.mark.parametrize("name", ["sh_clamped_deg0", "sh_clamped_deg1", "sh_clamped_deg2"])
def test_rows_of_16_coefficients_below_degree_3(hip, oracle64, oracle32, name):
    """Degree 0, 1, 2 in rows of 16 coefficients: the 16-coefficient instantiation with its coefficient loop predicated (k < nb <= k < M)."""
    rg.check_scene(name, hip, oracle64, oracle32, width=16)


@pytest.mark.parametrize("iso", [False, True], ids=["anisotropic", "isotropic"])
@pytest.mark.parametrize("P", rg.SPARSE_P)
def test_sparse_live(hip, oracle64, oracle32, P, iso):
    rg.check_sparse(P, iso, hip, oracle64, oracle32)
