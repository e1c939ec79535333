"""ignore_outlier_depth_loss on the fused paths on the MI355X: the checks of tests/test_outlier.py on the device.  Rules and tolerances:
tests/outlier_cases.py."""
import pytest

from tests import mapstep_cases as MC
from tests import outlier_cases as OC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", OC.MEDIAN_VARIANTS)
def test_gpu_median_is_torch_median(hip, variant):
    for frame in OC.MEDIAN_FRAMES:
        OC.check_median(hip, *frame, variant)
    OC.check_median_at_chunk_edges(hip, variant)


@pytest.mark.parametrize("frame", OC.MEDIAN_LARGE, ids=lambda f: f"{f[0]}x{f[1]}")
def test_gpu_median_at_frame_sizes(hip, frame):
    OC.check_median(hip, *frame, "random")


@pytest.mark.parametrize("shape", MC.LOSS_SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_mapping_loss_with_outlier_rejection(hip, shape):
    OC.check_mapping_loss(hip, *shape, im_exact=False)


@pytest.mark.parametrize("special", OC.LOSS_SPECIALS)
def test_gpu_mapping_loss_special_inputs(hip, special):
    OC.check_mapping_loss(hip, 37, 50, special, im_exact=False)


@pytest.mark.parametrize("size", OC.TRACK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_tracking_loss_with_outlier_rejection(hip, size):
    OC.check_tracking_loss(hip, *size)


@pytest.mark.parametrize("special", OC.LOSS_SPECIALS)
def test_gpu_tracking_loss_special_inputs(hip, special):
    OC.check_tracking_loss(hip, 45, 67, special)


def test_gpu_infinite_median_is_the_plain_mapping_loss(hip):
    OC.check_infinite_median_is_the_plain_mapping_loss(hip, exact=False)


def test_gpu_infinite_median_is_the_plain_tracking_loss(hip):
    OC.check_infinite_median_is_the_plain_tracking_loss(hip)


def test_gpu_mapping_iteration_with_the_option(hip):
    OC.check_mapping_iteration_with_the_option(hip, exact=False)


def test_gpu_fused_loss_matches_the_reference_pattern(hip):
    OC.check_fused_loss_against_the_reference_pattern(hip)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True)], ids=["aniso", "iso"])
def test_gpu_first_tracking_iteration_with_the_option(hip, kw):
    OC.check_first_tracking_iteration(hip, **kw)


def test_gpu_track_frame_with_the_option(hip):
    OC.check_track_frame_with_the_option(hip, exact=False)


def test_gpu_mapper_with_the_option(hip):
    OC.check_mapper_with_the_option(hip)
