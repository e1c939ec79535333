"""Camera-pose gradients of the fused raster paths (tracking / bundle adjustment) on the host-emulated kernels: render_rgbd_raw(camera=...),
fused_rendervar(camera_grad=True) and get_loss(tracking=True / do_ba=True) against torch autograd through transform_to_frame(camera_grad=True)
on the same library, and against an fp64 dense render.  Tolerances: tests/pose_cases.py."""
import pytest
import torch

from tests import parity_cases as pc
from tests import pose_cases as P


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True), dict(sh=True, iso=True), dict(white=True)],
                         ids=["aniso", "iso", "sh16", "sh16-iso", "white-bg"])
def test_emulated_pose_gradient_equals_the_torch_chain(emu, kw):
    P.check_pose_against_torch("cpu", 600, 64, 48, **kw)          # (64 x 48: a few-tile image -> the segmented backward walk)


def test_emulated_pose_gradient_radix_path_and_chained_backward(emu):
    from activesplat_amd import _lib
    lib = _lib.get()
    pc.set_sort_path("radix")
    try:
        P.check_pose_against_torch("cpu", 600, 64, 48)
        P.check_pose_against_torch("cpu", 600, 64, 48, sh=True)
    finally:
        pc.set_sort_path("auto")
    try:
        _lib.check(lib.gs_set_backward_chain(3, 256))           # (the threshold lowered: a 306-tile image walks its lists in chained pieces)
        P.check_pose_against_torch("cpu", 3000, 288, 272)
    finally:
        _lib.check(lib.gs_set_backward_chain(3, -1))


def test_emulated_pose_gradient_with_culled_and_nonfinite_gaussians(emu):
    P.check_nonfinite_scene("cpu")


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True)], ids=["aniso", "iso", "sh16"])
def test_emulated_ba_leaves_gaussian_gradients_bit_identical_and_pose_only_matches(emu, kw):
    with P.one_openmp_thread():
        P.check_ba_bit_identity_and_pose_only("cpu", **kw)


def test_emulated_pose_reduction_is_deterministic(emu):
    P.check_pose_reduction_is_deterministic("cpu", n=5000)


@pytest.mark.parametrize("kw", [dict(), dict(iso=True), dict(sh=True), dict(white=True)], ids=["aniso", "iso", "sh16", "white-bg"])
def test_emulated_pose_gradient_against_fp64_dense_render(emu, kw):
    P.check_against_fp64("cpu", **kw)


def test_emulated_get_loss_tracking_and_ba_fused_equal_unfused(emu):
    P.check_get_loss_modes("cpu")


def test_camera_arguments_are_validated_before_any_launch(emu):
    from activesplat_amd import optim as O
    params, cam, t = P.make_scene(50, 32, 32, "cpu")
    m2d = torch.empty_like(params["means3D"], requires_grad=True)
    args = (cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"], params["unnorm_rotations"], None)
    with pytest.raises(Exception, match="pose-only"):
        from activesplat_amd import rasterizer as R
        R.render_rgbd_raw(*args, colors_precomp=params["rgb_colors"], gaussians_grad=False)
    with pytest.raises(Exception, match="4 values"):
        R.render_rgbd_raw(*args, colors_precomp=params["rgb_colors"], camera=(torch.zeros(3, requires_grad=True), torch.zeros(3)))
    opt = O.initialize_optimizer(params, dict(means3D=1e-4, rgb_colors=1e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3,
                                              cam_unnorm_rots=1e-3, cam_trans=1e-3))
    with pytest.raises(Exception, match="exclude each other"):
        R.render_rgbd_raw(*args, colors_precomp=params["rgb_colors"], adam=opt,
                          camera=(torch.tensor([1.0, 0, 0, 0], requires_grad=True), torch.zeros(3)))


def test_emulated_frozen_camera_tensors_backpropagate_like_no_camera(emu):
    with P.one_openmp_thread():
        P.check_frozen_camera("cpu")


@pytest.mark.parametrize("kw", [dict(), dict(iso=True)], ids=["aniso", "iso"])
def test_emulated_unit_leaf_camera_gets_the_reference_gradient(emu, kw):
    P.check_unit_leaf_camera("cpu", **kw)
