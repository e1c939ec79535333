"""CPU: the reference's OWN caller code -- splatam.get_pointcloud -> initialize_params -> initialize_optimizer -> get_loss -> backward ->
optimizer.step, and the no-grad `render()` -- run unmodified against this repository's `diff_gaussian_rasterization` (import recipe of
SURVEY.md App. C; kernels on the host emulator) is captured in tests/golden/dropin.npz (tests/golden/make_golden.py dropin); here the
host-side mirrors in activesplat_amd.mapping, on the same drop-in and identical inputs, must agree with it."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return np.load(os.path.join(G, "dropin.npz"), allow_pickle=False)


def test_reference_get_loss_backward_step_runs_on_the_dropin(emu):
    from activesplat_amd import mapping as M
    from activesplat_amd import optim as O
    from activesplat_amd import setup_camera
    d = load()
    loss_ref, seen, m2d_grad, pc = d["loss"], d["seen"], d["m2d_grad"], d["pc"]
    # what the reference's own calls produced on the drop-in
    assert np.isfinite(loss_ref) and loss_ref > 0 and seen.sum() > 0.9 * pc.shape[0]
    assert m2d_grad.shape == (pc.shape[0], 3) and np.abs(m2d_grad[:, :2]).sum() > 0 and (m2d_grad[:, 2] == 0).all()
    assert np.abs(d["p1_means3D"] - d["p0_means3D"]).max() > 0
    # the mirror on the same inputs gives the same point cloud, loss, gradients and Adam step (same rasteriser underneath)
    color, depth, K, w2c = (torch.from_numpy(d[k]) for k in ("color", "depth", "K", "w2c"))
    H, W = color.shape[1:]
    pc2, msd2 = M.get_pointcloud(color, depth, K, w2c, compute_mean_sq_dist=True)
    np.testing.assert_allclose(pc2.numpy(), pc, rtol=1e-6, atol=1e-7)
    mp, mv = M.initialize_params(pc2, 2, msd2, "anisotropic")
    np.testing.assert_array_equal(mp["means3D"].detach().numpy(), d["p0_means3D"])
    lrs = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)
    opt = O.initialize_optimizer(mp, lrs)
    cam = setup_camera(W, H, K.numpy(), np.eye(4), device="cpu")
    gt = dict(cam=cam, im=torch.from_numpy(d["gt_im"]), depth=torch.from_numpy(d["gt_depth"]), id=0, intrinsics=K, w2c=w2c)
    loss2, mv, _ = M.get_loss(mp, gt, mv, 0, dict(im=0.5, depth=1.0))
    loss2.backward()
    np.testing.assert_allclose(loss2.item(), float(loss_ref), rtol=1e-6)
    np.testing.assert_array_equal(mv["seen"].numpy(), seen)
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        ref = d[f"grad_{k}"]
        np.testing.assert_allclose(mp[k].grad.numpy(), ref, rtol=1e-4, atol=max(1e-9, 1e-6 * float(np.abs(ref).max())), err_msg=k)
    with torch.no_grad():
        opt.step()
    step_ref = d["p1_means3D"] - d["p0_means3D"]
    np.testing.assert_allclose(mp["means3D"].detach().numpy() - d["p0_means3D"], step_ref, rtol=1e-3, atol=1e-3 * float(np.abs(step_ref).max()))


def test_reference_nograd_render_runs_on_the_dropin(emu):
    from activesplat_amd import mapping as M
    from activesplat_amd import synthetic as syn
    d = load()
    W, H, N = 80, 60, 1500
    p = syn.make_params(N, W, H, seed=4)
    params = dict(means3D=p["means3D"], rgb_colors=p["rgb_colors"], unnorm_rotations=p["unnorm_rotations"],
                  logit_opacities=p["logit_opacities"], log_scales=p["log_scales"])
    for k, v in params.items():
        np.testing.assert_array_equal(v.numpy(), d[f"render_{k}"], err_msg=k)
    w2c = np.eye(4)
    rv, dv = M.get_rendervars(params, w2c)
    got = M.render(w2c, syn.intrinsics(W, H), rv, dv, dict(viz_w=W, viz_h=H, viz_near=0.01, viz_far=100.0))
    ref = tuple(d[f"render_{k}"] for k in ("im", "depth", "opacity", "sil"))
    for name, g_, r_ in zip(("im", "depth", "opacity", "sil"), got, ref):
        np.testing.assert_allclose(g_.numpy(), r_, rtol=1e-5, atol=1e-6, err_msg=name)
    im, depth, opacity, sil = ref
    assert im.shape == (3, H, W) and depth.shape == (1, H, W) and opacity.shape == (1, H, W) and sil.shape == (1, H, W)
    # call-site invariants: silhouette channel == opacity output; white background where empty
    np.testing.assert_allclose(sil, opacity, atol=3e-6)
    assert float(opacity.min()) >= 0 and float(opacity.max()) <= 1
    empty = opacity[0] < 1e-6
    if empty.any():
        assert np.allclose(im[:, empty], 1.0)
