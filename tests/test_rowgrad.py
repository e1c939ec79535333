"""The per-Gaussian backward row by row at its rare branches, on the host-emulated kernels (tests/rowgrad_cases.py; the device twin is
tests/test_gpu_rowgrad.py)."""
import pytest

from tests import rowgrad_cases as rg
from tests.pose_cases import one_openmp_thread


def test_fp32_oracle_alone_sets_floor_and_cap(oracle64, oracle32):
    """FLOOR and CAP come from the two oracles alone: the fp32 oracle's largest per-row relative error over every scene and entry point is
    printed (rowgrad_cases.MEASURED_ORACLE32_ROW_ERROR records it) and FLOOR must be at least twice it, so a generator change that moves it
    shows here.  Building the references also asserts, scene by scene, the class majorities and that no pixel sits at the alpha = 1/255
    threshold, the 0.99 clamp or the T stop."""
    worst = (0.0, None)
    for label, ref in rg.all_references(oracle64, oracle32):
        e, k, row = rg.oracle_row_error(ref)
        print(f"[rowgrad] fp32 oracle alone: {label:36s} visible {int(ref['visible'].sum()):4d} worst row {row:4d} of {k}: {e:.3e}")
        if e > worst[0]:
            worst = (e, label)
    print(f"[rowgrad] fp32 oracle alone: largest per-row relative error {worst[0]:.3e} ({worst[1]}); FLOOR {rg.FLOOR:g}, CAP {rg.CAP:g}")
    assert 2.0 * worst[0] <= rg.FLOOR, worst


@pytest.mark.parametrize("name", rg.SCENES)
def test_rows(emu, oracle64, oracle32, name):
    with one_openmp_thread():
        rg.check_scene(name, emu, oracle64, oracle32, exact_adam=True)


@pytest.mark.parametrize("name", ["sh_clamped_deg0", "sh_clamped_deg1", "sh_clamped_deg2"])
def test_rows_of_16_coefficients_below_degree_3(emu, oracle64, oracle32, name):
    """Degree 0, 1, 2 in rows of 16 coefficients: the 16-coefficient instantiation with its coefficient loop predicated (k < nb <= k < M)."""
    rg.check_scene(name, emu, oracle64, oracle32, width=16)


@pytest.mark.parametrize("iso", [False, True], ids=["anisotropic", "isotropic"])
@pytest.mark.parametrize("P", rg.SPARSE_P)
def test_sparse_live(emu, oracle64, oracle32, P, iso):
    with one_openmp_thread():
        rg.check_sparse(P, iso, emu, oracle64, oracle32, exact_adam=True)
