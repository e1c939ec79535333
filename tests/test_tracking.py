"""Camera tracking on the fused path (mapping.tracking_iteration / track_frame, gs_tracking_* in include/gsplat_hip.h) on the host-emulated
kernels: the tracking loss kernel against the torch loss, the device-pose forward / backward against the host-pose calls, the tracking step
against torch.optim.Adam, SplaTAM's candidate and doubling rules, and the fused loop against the reference call pattern.
Tolerances: tests/tracking_cases.py."""
import pytest

from tests import pose_cases as PC
from tests import tracking_cases as T


def test_emulated_tracking_loss_matches_torch(emu):
    T.check_tracking_loss(emu)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True)], ids=["aniso", "iso", "sh16"])
def test_emulated_device_pose_matches_host_pose(emu, kw):
    T.check_device_pose_matches_host_pose(emu, **kw)


def test_emulated_tracking_step_matches_torch_adam(emu):
    T.check_step_matches_torch_adam(emu)


def test_emulated_candidate_and_doubling(emu):
    with PC.one_openmp_thread():
        T.check_candidate_and_doubling(emu)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True)], ids=["aniso", "iso"])
def test_emulated_first_iteration_matches_reference_pattern(emu, kw):
    T.check_first_iteration_parity(emu, **kw)


def test_emulated_tracking_converges_like_the_reference(emu):
    T.check_tracking_converges_like_the_reference(emu)


def test_emulated_track_frame_is_deterministic(emu):
    with PC.one_openmp_thread():
        T.check_track_frame_deterministic(emu)


def test_tracking_optimizer_eps_is_torch_adams():
    import torch
    from activesplat_amd import optim as O
    params = {k: torch.nn.Parameter(torch.zeros(2, 3)) for k in ("cam_unnorm_rots", "cam_trans", "means3D")}
    opt = O.initialize_optimizer(params, dict(cam_unnorm_rots=1e-3, cam_trans=4e-3, means3D=0.0), tracking=True)
    assert [g["eps"] for g in opt.param_groups] == [1e-8] * 3
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 4e-3, 0.0]
    mapping = O.initialize_optimizer(params, dict(cam_unnorm_rots=1e-3, cam_trans=4e-3, means3D=0.0))
    assert [g["eps"] for g in mapping.param_groups] == [1e-15] * 3


def test_emulated_mapper_tracks_like_the_reference_pattern(emu):
    T.check_mapper_tracking(emu)


def test_emulated_mapper_default_keeps_the_frame_poses(emu):
    T.check_mapper_default_keeps_frame_poses(emu)
