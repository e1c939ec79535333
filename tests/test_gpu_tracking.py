"""Camera tracking on the fused path on the MI355X: the checks of tests/test_tracking.py on the device, plus the two workload sizes of the
timing script (256 x 256 with 200 k Gaussians, 640 x 480 with 500 k).  Tolerances: tests/tracking_cases.py."""
import pytest

from tests import tracking_cases as T

pytestmark = pytest.mark.gpu


def test_gpu_tracking_loss_matches_torch(hip):
    T.check_tracking_loss(hip)
    T.check_tracking_loss(hip, W=640, H=480)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True)], ids=["aniso", "iso", "sh16"])
def test_gpu_device_pose_matches_host_pose(hip, kw):
    T.check_device_pose_matches_host_pose(hip, exact_ok=False, **kw)
    T.check_device_pose_matches_host_pose(hip, 20000, 160, 120, exact_ok=False, **kw)


def test_gpu_tracking_step_matches_torch_adam(hip):
    T.check_step_matches_torch_adam(hip)


def test_gpu_candidate_and_doubling(hip):
    T.check_candidate_and_doubling(hip)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True)], ids=["aniso", "iso"])
def test_gpu_first_iteration_matches_reference_pattern(hip, kw):
    T.check_first_iteration_parity(hip, **kw)


def test_gpu_tracking_converges_like_the_reference(hip):
    T.check_tracking_converges_like_the_reference(hip)
    T.check_tracking_converges_like_the_reference(hip, 20000, 160, 120)


def test_gpu_track_frame_is_deterministic(hip):
    T.check_track_frame_deterministic(hip, exact=False)


@pytest.mark.parametrize("size", [(200_000, 256, 256), (500_000, 640, 480)], ids=["256x256-200k", "640x480-500k"])
def test_gpu_tracking_at_workload_sizes(hip, size):
    n, W, H = size
    T.check_tracking_loss(hip, W=W, H=H)
    T.check_first_iteration_parity(hip, n, W, H)
    T.check_track_frame_deterministic(hip, n, W, H, iters=40, exact=False)
