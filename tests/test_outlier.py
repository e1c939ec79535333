"""ignore_outlier_depth_loss on the fused paths, on the host-emulated kernels: the exact multi-workgroup median select against torch.median, the
outlier forms of the mapping and tracking loss kernels against restated torch references, the plain entry points unchanged, and the option
through mapping_iteration, get_loss, tracking_iteration, track_frame and SplatMapper.  Rules and tolerances: tests/outlier_cases.py."""
import pytest

from tests import mapstep_cases as MC
from tests import outlier_cases as OC
from tests import pose_cases as PC


@pytest.mark.parametrize("variant", OC.MEDIAN_VARIANTS)
@pytest.mark.parametrize("frame", OC.MEDIAN_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_emulated_median_is_torch_median(emu, frame, variant):
    OC.check_median(emu, *frame, variant)


@pytest.mark.parametrize("variant", OC.MEDIAN_VARIANTS)
def test_emulated_median_at_chunk_edges(emu, variant):
    OC.check_median_at_chunk_edges(emu, variant)


@pytest.mark.parametrize("frame", OC.MEDIAN_LARGE, ids=lambda f: f"{f[0]}x{f[1]}")
def test_emulated_median_at_frame_sizes(emu, frame):
    OC.check_median(emu, *frame, "random")


@pytest.mark.parametrize("shape", MC.LOSS_SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_mapping_loss_with_outlier_rejection(emu, shape):
    with PC.one_openmp_thread():
        OC.check_mapping_loss(emu, *shape)


@pytest.mark.parametrize("special", OC.LOSS_SPECIALS)
def test_emulated_mapping_loss_special_inputs(emu, special):
    with PC.one_openmp_thread():
        OC.check_mapping_loss(emu, 37, 50, special)


@pytest.mark.parametrize("size", OC.TRACK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_tracking_loss_with_outlier_rejection(emu, size):
    OC.check_tracking_loss(emu, *size)


@pytest.mark.parametrize("special", OC.LOSS_SPECIALS)
def test_emulated_tracking_loss_special_inputs(emu, special):
    OC.check_tracking_loss(emu, 45, 67, special)


def test_emulated_infinite_median_is_the_plain_mapping_loss(emu):
    with PC.one_openmp_thread():
        OC.check_infinite_median_is_the_plain_mapping_loss(emu)


def test_emulated_infinite_median_is_the_plain_tracking_loss(emu):
    OC.check_infinite_median_is_the_plain_tracking_loss(emu)


def test_emulated_mapping_iteration_with_the_option(emu):
    with PC.one_openmp_thread():
        OC.check_mapping_iteration_with_the_option(emu)


def test_emulated_fused_loss_matches_the_reference_pattern(emu):
    OC.check_fused_loss_against_the_reference_pattern(emu)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True)], ids=["aniso", "iso"])
def test_emulated_first_tracking_iteration_with_the_option(emu, kw):
    OC.check_first_tracking_iteration(emu, **kw)


def test_emulated_track_frame_with_the_option(emu):
    with PC.one_openmp_thread():
        OC.check_track_frame_with_the_option(emu)


def test_emulated_mapper_with_the_option(emu):
    OC.check_mapper_with_the_option(emu)
