"""The mapping step's non-raster kernels (loss, growth, compaction / gather / densify, activations) on the MI355X against float64 /
exact pure-torch references: the cases of tests/mapstep_cases.py.  The same cases run on the host-emulated build in tests/test_mapstep_fp64.py."""
import pytest

from tests import mapstep_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_gpu_mapping_loss_against_fp64(hip, kind):
    for H, W in C.LOSS_SHAPES:
        C.check_mapping_loss(hip, H, W, kind)


def test_gpu_mapping_loss_without_a_valid_depth_pixel(hip):
    C.check_mapping_loss(hip, 37, 50, "smooth", all_invalid=True)


@pytest.mark.parametrize("variant", C.GROW_VARIANTS)
def test_gpu_growth_decisions_are_exact_and_rows_match_fp64(hip, variant):
    for H, W in C.GROW_FRAMES:
        C.check_grow(hip, H, W, variant)


@pytest.mark.parametrize("n", C.COMPACT_N)
def test_gpu_build_index_equals_nonzero(hip, n):
    C.check_build_index(hip, n)


@pytest.mark.parametrize("n", C.COMPACT_N)
def test_gpu_compact_index3_equals_nonzero(hip, n):
    C.check_compact_index3(hip, n)


@pytest.mark.parametrize("width,misaligned", [(1, False), (3, False), (4, False), (48, False), (4, True)],
                         ids=["1", "3", "4", "48", "4-misaligned"])
def test_gpu_gather_rows_past_one_grid_pass(hip, width, misaligned):
    C.check_gather_rows(hip, width, misaligned)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_gpu_remove_points_equals_pure_torch(hip, iso):
    C.check_remove_points(hip, iso)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_gpu_prune_equals_pure_torch(hip, iso):
    C.check_prune(hip, iso)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_gpu_densify_equals_pure_torch(hip, iso):
    C.check_densify(hip, iso)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("P", C.ACTIVATE_P)
def test_gpu_activations_against_fp64(hip, P, iso):
    C.check_activate(hip, P, iso)
