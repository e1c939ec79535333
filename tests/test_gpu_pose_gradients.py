"""Camera-pose gradients of the fused raster paths on the MI355X: the checks of tests/test_pose_gradients.py on the device, plus the two
workload sizes of the timing script (256 x 256 with 200 k Gaussians, 640 x 480 with 500 k).  Tolerances: tests/pose_cases.py."""
import pytest

from tests import parity_cases as pc
from tests import pose_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True), dict(sh=True, iso=True), dict(white=True)],
                         ids=["aniso", "iso", "sh16", "sh16-iso", "white-bg"])
def test_gpu_pose_gradient_equals_the_torch_chain(hip, kw):
    P.check_pose_against_torch(hip, 600, 64, 48, **kw)
    P.check_pose_against_torch(hip, 20000, 160, 120, **kw)


@pytest.mark.parametrize("size", [(200_000, 256, 256), (500_000, 640, 480)], ids=["256x256-200k", "640x480-500k"])
def test_gpu_pose_gradient_at_workload_sizes(hip, size):
    n, W, H = size
    P.check_pose_against_torch(hip, n, W, H)
    P.check_close_ba_and_pose_only(hip, n, W, H)


def test_gpu_pose_gradient_radix_path_and_chained_backward(hip):
    from activesplat_amd import _lib
    lib = _lib.get()
    pc.set_sort_path("radix")
    try:
        P.check_pose_against_torch(hip, 20000, 160, 120)
    finally:
        pc.set_sort_path("auto")
    try:
        _lib.check(lib.gs_set_backward_chain(3, 256))
        P.check_pose_against_torch(hip, 5000, 288, 272)
    finally:
        _lib.check(lib.gs_set_backward_chain(3, -1))


def test_gpu_pose_gradient_with_culled_and_nonfinite_gaussians(hip):
    P.check_nonfinite_scene(hip)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True)], ids=["aniso", "iso", "sh16"])
def test_gpu_ba_gaussian_gradients_and_pose_only(hip, kw):
    P.check_close_ba_and_pose_only(hip, **kw)


def test_gpu_pose_reduction_is_deterministic(hip):
    P.check_pose_reduction_is_deterministic(hip)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True)], ids=["aniso", "iso", "sh16"])
def test_gpu_pose_gradient_against_fp64_dense_render(hip, kw):
    P.check_against_fp64(hip, **kw)


def test_gpu_get_loss_tracking_and_ba_fused_equal_unfused(hip):
    P.check_get_loss_modes(hip)


def test_gpu_frozen_camera_tensors_backpropagate_like_no_camera(hip):
    P.check_frozen_camera(hip, exact=False)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True)], ids=["aniso", "iso"])
def test_gpu_unit_leaf_camera_gets_the_reference_gradient(hip, kw):
    P.check_unit_leaf_camera(hip, **kw)
