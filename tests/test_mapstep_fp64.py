"""The mapping step's non-raster kernels (loss, growth, compaction / gather / densify, activations) on the host-emulated build against float64 /
exact pure-torch references: the cases of tests/mapstep_cases.py.  The same cases run on the device in tests/test_gpu_mapstep_fp64.py."""
import pytest

from tests import mapstep_cases as C


@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_emulated_mapping_loss_against_fp64(emu, kind):
    for H, W in C.LOSS_SHAPES:
        C.check_mapping_loss("cpu", H, W, kind)


def test_emulated_mapping_loss_without_a_valid_depth_pixel(emu):
    C.check_mapping_loss("cpu", 37, 50, "smooth", all_invalid=True)


@pytest.mark.parametrize("variant", C.GROW_VARIANTS)
def test_emulated_growth_decisions_are_exact_and_rows_match_fp64(emu, variant):
    for H, W in C.GROW_FRAMES:
        C.check_grow("cpu", H, W, variant)


@pytest.mark.parametrize("n", C.COMPACT_N)
def test_emulated_build_index_equals_nonzero(emu, n):
    C.check_build_index("cpu", n)


@pytest.mark.parametrize("n", C.COMPACT_N)
def test_emulated_compact_index3_equals_nonzero(emu, n):
    C.check_compact_index3("cpu", n)


@pytest.mark.parametrize("width,misaligned", [(1, False), (3, False), (4, False), (48, False), (4, True)],
                         ids=["1", "3", "4", "48", "4-misaligned"])
def test_emulated_gather_rows_past_one_grid_pass(emu, width, misaligned):
    C.check_gather_rows("cpu", width, misaligned)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_emulated_remove_points_equals_pure_torch(emu, iso):
    C.check_remove_points("cpu", iso)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_emulated_prune_equals_pure_torch(emu, iso):
    C.check_prune("cpu", iso)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
def test_emulated_densify_equals_pure_torch(emu, iso):
    C.check_densify("cpu", iso)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("P", C.ACTIVATE_P)
def test_emulated_activations_against_fp64(emu, P, iso):
    C.check_activate("cpu", P, iso)
