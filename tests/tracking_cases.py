"""Camera tracking on the fused path (mapping.tracking_iteration / track_frame, include/gsplat_hip.h gs_tracking_*): shared checks of the
emulated (CPU) and the GPU test files.  Yardsticks: the reference's torch tracking loss under autograd (get_loss(tracking=True) on the unfused
path), torch.optim.Adam, and the reference call pattern of the tracking loop (track_frame(fused=False)).

Tolerances:
  * LOSS_RTOL = 1e-5: the tracking loss sums |error| over up to 3 H W pixels in fp32 (torch) and in per-workgroup fp32 rows reduced in fp64
    (kernel): the two differ by the fp32 sum-order error of torch's sum, ~1e-7 x sqrt(terms) relative;
  * the gradient images: bit-identical (the kernel evaluates autograd's own expression);
  * POSE_RTOL (tests/pose_cases.py) for the first iteration's pose gradient against the torch chain (the same per-Gaussian products summed in
    different orders, and the torch chain's activations are not bit-identical to the kernels');
  * ADAM_ATOL = 1e-6 on the pose after 24 steps against torch.optim.Adam fed the same gradients: a few fp32 ulp of O(1) values (torch forms
    the gradient through F.normalize in fp32 autograd, the kernel in fp64; Adam's division by sqrt(v) passes that difference on);
  * DET_ATOL = 1e-4 between two device runs of track_frame (float atomics in the rasteriser's backward; the emulated kernels on one thread
    repeat to the bit);
  * the tracked pose: both loops must cut the initial error, and the fused one must end within TRACK_FACTOR x the reference loop's error plus
    TRACK_MARGIN (Adam's early steps are ~lr sign(g): the two trajectories are not the same, only equally good).
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from activesplat_amd import _lib
from activesplat_amd import mapping as M
from activesplat_amd import rasterizer as R
from activesplat_amd import synthetic as syn
from activesplat_amd.camera import setup_camera
from tests import pose_cases as PC

LOSS_RTOL = 1e-5
POSE_RTOL = PC.POSE_RTOL
ADAM_ATOL = 1e-6
TRACK_FACTOR = 2.0
TRACK_MARGIN = (2e-3, 2e-3)         # (rotation angle in rad, translation in scene units)
DET_ATOL = 1e-4                     # device runs: atomics in the rasteriser's backward (see check_track_frame_deterministic)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def quat(axis_angle):
    a = np.asarray(axis_angle, dtype=np.float64)
    th = float(np.linalg.norm(a))
    if th == 0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * a / th])


def qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def pose_error(params, t, truth):
    """(rotation angle between the column's and the true quaternion, translation distance)."""
    q = F.normalize(params["cam_unnorm_rots"][..., t].detach().double().cpu()).reshape(4).numpy()
    d = abs(float(np.dot(q, truth[0] / np.linalg.norm(truth[0]))))
    tr = params["cam_trans"][..., t].detach().double().cpu().reshape(3).numpy()
    return 2.0 * float(np.arccos(min(1.0, d))), float(np.linalg.norm(tr - truth[1]))


def track_scene(n, W, H, device, seed=3, t=2, T=4, iso=False, sh=False, rot_err=(0.012, -0.01, 0.008), trans_err=(0.015, -0.012, 0.02),
                truth_aa=(0.02, 0.03, -0.01), truth_t=(0.03, -0.02, 0.05)):
    """(params, curr_data, variables, t, truth): a map of n Gaussians, frame t rendered at the true pose (truth_aa / truth_t) as its colour and
    depth target, and column t of the camera parameters set to the truth perturbed by rot_err (axis-angle) / trans_err on all axes."""
    p = syn.make_params(n, W, H, seed=seed, sh_degree=3 if sh else None)
    if sh:
        p.pop("rgb_colors", None)
    if iso:
        p["log_scales"] = p["log_scales"][:, :1].contiguous()
    params = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
    q_true = quat(truth_aa)
    rots = np.tile(np.array([1.0, 0.0, 0.0, 0.0])[:, None], (1, T))
    trans = np.zeros((3, T))
    rots[:, t], trans[:, t] = q_true, truth_t
    params["cam_unnorm_rots"] = torch.nn.Parameter(torch.tensor(rots, dtype=torch.float32).reshape(1, 4, T).to(device))
    params["cam_trans"] = torch.nn.Parameter(torch.tensor(trans, dtype=torch.float32).reshape(1, 3, T).to(device))
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, sh_degree=3 if sh else 0)
    variables = {k: torch.zeros(params["means3D"].shape[0], device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom")}
    _, (im, _r, depth, _s, _dsq) = M.tracking_render(params, dict(cam=cam), variables, t)
    curr = dict(cam=cam, id=t, im=im.clone(), depth=depth.clone(), w2c=torch.eye(4, device=device))
    with torch.no_grad():
        q0 = qmul(quat(rot_err), q_true) * 1.1                          # (unnormalised: F.normalize is on the chain)
        params["cam_unnorm_rots"][0, :, t] = torch.tensor(q0, dtype=torch.float32)
        params["cam_trans"][0, :, t] = torch.tensor(np.asarray(truth_t) + np.asarray(trans_err), dtype=torch.float32)
        variables["max_2D_radius"].zero_()
    return params, curr, variables, t, (q_true, np.asarray(truth_t))


def clone_params(params):
    return {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}


# ---- 1. the tracking loss kernel against the torch tracking loss ----------------------------------------------------------------------------

def loss_inputs(W, H, device, seed=0, sil_thres=0.99):
    g = torch.Generator().manual_seed(seed)
    im, gt = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    depth, gtd = torch.rand(1, H, W, generator=g) * 3 + 0.5, torch.rand(1, H, W, generator=g) * 3 + 0.5
    dsq = depth * depth + torch.rand(1, H, W, generator=g) * 0.1
    sil = torch.rand(1, H, W, generator=g)
    flat = lambda x: x.view(-1)  # noqa: E731
    n = W * H
    idx = torch.randperm(n, generator=g)
    flat(depth)[idx[:40]] = float("nan")                                 # NaN depth
    flat(dsq)[idx[40:60]] = float("nan")                                 # NaN uncertainty
    flat(gtd)[idx[60:120]] = 0.0                                         # no depth measurement
    flat(sil)[idx[120:200]] = float(np.float32(sil_thres))               # silhouette exactly at the threshold: excluded
    flat(sil)[idx[200:400]] = 1.0
    im.view(3, -1)[:, idx[400:460]] = gt.view(3, -1)[:, idx[400:460]]    # im == gt: sign 0
    flat(depth)[idx[460:500]] = flat(gtd)[idx[460:500]]                  # depth == gt depth
    return [x.to(device) for x in (im, gt, depth, dsq, gtd, sil)]


def torch_tracking_loss(im, gt, depth, dsq, gtd, sil, use_sil, sil_thres, w):
    """get_loss's tracking branch (splatam.py:220-249, use_l1) with autograd on im and depth."""
    im, depth = im.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    unc = (dsq - depth ** 2).detach()
    mask = (gtd > 0) & ~torch.isnan(depth) & ~torch.isnan(unc)
    if use_sil:
        mask = mask & (sil > sil_thres)
    mask = mask.detach()
    losses = {"depth": (gtd - depth).abs()[mask].sum()}
    losses["im"] = (gt - im).abs()[torch.tile(mask, (3, 1, 1))].sum() if use_sil else (gt - im).abs().sum()
    weighted = {k: v * w[k] for k, v in losses.items()}
    loss = sum(weighted.values())
    loss.backward()
    return float(loss.detach()), float(weighted["depth"].detach()), float(weighted["im"].detach()), im.grad, depth.grad


def kernel_tracking_loss(im, gt, depth, dsq, gtd, sil, use_sil, sil_thres, w):
    lib = _lib.get()
    H, W = int(im.shape[1]), int(im.shape[2])
    dev = im.device
    grads = torch.empty(4, H, W, dtype=torch.float32, device=dev)
    rows = torch.empty(int(lib.gs_tracking_loss_scratch_bytes(W, H)), dtype=torch.uint8, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.check(lib.gs_tracking_loss(W, H, _p(im), _p(gt), _p(depth), _p(dsq), _p(gtd), _p(sil if use_sil else None), 1 if use_sil else 0,
                                    float(sil_thres), float(w["im"]), float(w["depth"]), _p(grads[:3]), _p(grads[3:]), _p(rows), _p(out),
                                    _lib.stream_ptr(dev)))
    return out.cpu(), grads[:3], grads[3:]


def check_tracking_loss(device, W=67, H=45, sil_thres=0.99):
    w = dict(im=0.5, depth=1.0)
    ins = loss_inputs(W, H, device, sil_thres=sil_thres)
    for use_sil in (True, False):
        ref = torch_tracking_loss(*ins, use_sil, sil_thres, w)
        out, d_im, d_depth = kernel_tracking_loss(*ins, use_sil, sil_thres, w)
        for got, want in zip(out.tolist(), ref[:3]):
            assert abs(got - want) <= LOSS_RTOL * abs(want), (use_sil, out.tolist(), ref[:3])
        assert torch.equal(d_im, ref[3]) and torch.equal(d_depth, ref[4]), use_sil
        assert torch.equal(torch.signbit(d_im), torch.signbit(ref[3])) and torch.equal(torch.signbit(d_depth), torch.signbit(ref[4])), use_sil
        out2, d_im2, d_depth2 = kernel_tracking_loss(*ins, use_sil, sil_thres, w)
        assert torch.equal(out, out2) and torch.equal(d_im, d_im2) and torch.equal(d_depth, d_depth2), use_sil


# ---- 2. device-pose forward / backward against the host-pose calls --------------------------------------------------------------------------

def _host_pose_render(params, curr, t, pose_col, dL_im, dL_depth):
    q = F.normalize(pose_col[0].reshape(1, 4)).reshape(4)
    cam_rot, cam_tr = q.detach().clone().requires_grad_(True), pose_col[1].detach().clone().reshape(3).requires_grad_(True)
    m2d = torch.empty_like(params["means3D"], requires_grad=True)
    mx = torch.zeros(params["means3D"].shape[0], device=params["means3D"].device)
    seen = torch.empty(mx.numel(), dtype=torch.bool, device=mx.device)
    im, radius, depth, sil, dsq = R.render_rgbd_raw(curr["cam"], params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                    params["unnorm_rotations"], None, **PC._cols(params), visibility=(mx, seen),
                                                    camera=(cam_rot, cam_tr), gaussians_grad=False)
    torch.autograd.backward([im, depth], [dL_im, dL_depth])
    return dict(im=im.detach(), radius=radius, depth=depth.detach(), sil=sil, dsq=dsq, mx=mx, seen=seen,
                pose=torch.cat([cam_rot.grad, cam_tr.grad]), m2d=m2d.grad)


def _dev_pose_render(params, curr, t, dL_im, dL_depth):
    lib = _lib.get()
    dev = params["means3D"].device
    variables = {"max_2D_radius": torch.zeros(params["means3D"].shape[0], device=dev)}
    ctx, (im, radius, depth, sil, dsq) = M.tracking_render(params, curr, variables, t)
    pscr = torch.empty(int(lib.gs_pose_grad_scratch_bytes(int(params["means3D"].shape[0]))), dtype=torch.uint8, device=dev)
    d_pose = torch.empty(7, device=dev)
    m2d = R.backward_pose_dev(ctx, dL_im, dL_depth, pscr, d_pose)
    return dict(im=im, radius=radius, depth=depth, sil=sil, dsq=dsq, mx=variables["max_2D_radius"], seen=variables["seen"], pose=d_pose, m2d=m2d)


def check_device_pose_matches_host_pose(device, n=600, W=64, H=48, exact_ok=True, **kw):
    """exact_ok=False (the device): the backward's float atomics reorder from call to call, so the exact column is held to the bit only in the
    forward (images, radii, statistics) and within POSE_RTOL in the pose gradient."""
    params, curr, _v, t, _truth = track_scene(n, W, H, device, **kw)
    g = torch.Generator().manual_seed(4)
    dL_im, dL_depth = (torch.randn(3, H, W, generator=g) * 0.01).to(device), (torch.randn(1, H, W, generator=g) * 0.01).to(device)
    for exact in (True, False):
        if exact:                                                        # (1, 0, 0, 0) x 1.7: the normalisation is exact on both sides
            with torch.no_grad():
                params["cam_unnorm_rots"][0, :, t] = torch.tensor([1.7, 0.0, 0.0, 0.0])
        col = (params["cam_unnorm_rots"][..., t].detach(), params["cam_trans"][..., t].detach())
        with PC.one_openmp_thread():
            a = _host_pose_render(params, curr, t, col, dL_im, dL_depth)
            b = _dev_pose_render(params, curr, t, dL_im, dL_depth)
        assert torch.equal(a["radius"], b["radius"]) or not exact
        assert float((a["radius"] != b["radius"]).float().mean()) < 2e-3
        for k in ("im", "depth", "sil", "dsq", "mx", "seen", "pose", "m2d"):
            if exact and (exact_ok or k not in ("pose", "m2d")):
                assert torch.equal(a[k], b[k]), k
            elif k in ("im", "depth", "sil", "dsq"):
                assert float((a[k] - b[k]).abs().max()) < 1e-4, (k, float((a[k] - b[k]).abs().max()))
        if not (exact and exact_ok):
            assert PC.rel(b["pose"], a["pose"]) < POSE_RTOL, PC.rel(b["pose"], a["pose"])


# ---- 3. the tracking step against torch.optim.Adam ------------------------------------------------------------------------------------------

def check_step_matches_torch_adam(device, steps=24, seed=1):
    lib = _lib.get()
    dev = torch.device(device)
    g = torch.Generator().manual_seed(seed)
    T, t = 3, 1
    rots = torch.randn(1, 4, T, generator=g) * 0.3
    rots[0, 0] += 1.4                                                    # a non-unit column
    trans = torch.randn(1, 3, T, generator=g)
    mine_r, mine_t = rots.clone().to(dev), trans.clone().to(dev)
    ref_r, ref_t = torch.nn.Parameter(rots.clone()), torch.nn.Parameter(trans.clone())
    opt = torch.optim.Adam([{"params": [ref_r], "lr": 1e-3}, {"params": [ref_t], "lr": 4e-3}])
    P = 100                                                              # one row of pose partial sums
    pose_rows = torch.zeros(int(lib.gs_pose_grad_scratch_bytes(P)) // 4, dtype=torch.float32, device=dev)
    loss_rows = torch.zeros(int(lib.gs_tracking_loss_scratch_bytes(16, 16)) // 4, dtype=torch.float32, device=dev)
    state = torch.empty(int(lib.gs_tracking_state_bytes()) // 4, dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.gs_tracking_begin(_p(mine_r), _p(mine_t), T, t, _p(state), st))
    for k in range(1, steps + 1):
        gq, gt = torch.randn(4, generator=g), torch.randn(3, generator=g)
        if k % 5 == 0:
            gq = gq * 1e-3                                               # (small and large steps)
        # row layout (gs_common.h kPoseAcc): dL/dt [3], dL/dR [9] (zero here), dL/dq through the rasteriser's rotation [4]
        row = torch.cat([gt, torch.zeros(9), gq])
        pose_rows[:16] = row.to(dev)
        loss_rows[:2] = torch.tensor([float(steps - k), 1.0]).to(dev)
        _lib.check(lib.gs_tracking_step(P, _p(pose_rows), 16, 16, _p(loss_rows), 0.5, 1.0, _p(mine_r), _p(mine_t), T, t, 1e-3, 4e-3, k, _p(state),
                                        None, st))
        opt.zero_grad()
        u = F.normalize(ref_r[..., t])
        ((u.reshape(4) * gq).sum() + (ref_t[..., t].reshape(3) * gt).sum()).backward()
        if k == 1:
            # the gradient the step applied: exp_avg after one step is (1 - beta1) g
            m = state[:7].cpu()
            want = torch.cat([ref_r.grad[0, :, t], ref_t.grad[0, :, t]]) * np.float32(0.1)
            assert torch.allclose(m, want, rtol=1e-5, atol=1e-9), (m, want)
        opt.step()
        assert torch.allclose(mine_r.cpu(), ref_r.detach(), rtol=0, atol=ADAM_ATOL), (k, mine_r.cpu() - ref_r.detach())
        assert torch.allclose(mine_t.cpu(), ref_t.detach(), rtol=0, atol=ADAM_ATOL), (k, mine_t.cpu() - ref_t.detach())
    # the other columns are untouched; the candidate is the post-step column of the smallest loss (the last step: losses count down)
    assert torch.equal(mine_r[..., 0].cpu(), rots[..., 0]) and torch.equal(mine_t[..., 2].cpu(), trans[..., 2])
    assert torch.equal(state[15:19].cpu(), mine_r[0, :, t].cpu()) and torch.equal(state[19:22].cpu(), mine_t[0, :, t].cpu())


# ---- 4. candidate and doubling semantics ----------------------------------------------------------------------------------------------------

def check_candidate_and_doubling(device, n=600, W=64, H=48, iters=5):
    for thres, want in ((0.0, 2 * iters), (1e30, iters)):
        params, curr, variables, t, _truth = track_scene(n, W, H, device)
        cfg = dict(tracking_iters=iters, depth_loss_thres=thres, sil_thres=0.5)
        out = M.track_frame(params, curr, variables, t, cfg, fused=True, history=True)
        assert out["iterations"] == want, (thres, out["iterations"])
        h = out["history"]
        assert h.shape == (want, 10) and bool(torch.isfinite(h).all())
        best, best_k = 1e20, None
        for k in range(want):                                            # SplaTAM's rule, replayed: strict <, the first minimum wins
            if float(h[k, 0]) < best:
                best, best_k = float(h[k, 0]), k
        got = torch.cat([params["cam_unnorm_rots"][0, :, t], params["cam_trans"][0, :, t]]).detach().cpu()
        assert torch.equal(got, h[best_k, 3:]), (best_k, got, h[best_k, 3:])
        assert out["candidate_loss"] == best and out["final_loss"] == float(h[-1, 0])


# ---- 5. fused against the reference call pattern --------------------------------------------------------------------------------------------

def check_first_iteration_parity(device, n=600, W=64, H=48, sil_thres=0.5, rtol=POSE_RTOL, **kw):
    lib = _lib.get()
    params, curr, variables, t, _truth = track_scene(n, W, H, device, **kw)
    w = dict(im=0.5, depth=1.0)
    ref_p = clone_params(params)
    loss, _v, parts = M.get_loss(ref_p, curr, {k: v.clone() for k, v in variables.items()}, t, w, True, sil_thres, tracking=True)
    loss.backward()
    ref_grad = torch.cat([ref_p["cam_unnorm_rots"].grad[0, :, t], ref_p["cam_trans"].grad[0, :, t]])
    ctx, (im, _r, depth, sil, dsq) = M.tracking_render(params, curr, variables, t)
    out, d_im, d_depth = kernel_tracking_loss(im, curr["im"], depth, dsq, curr["depth"], sil, True, sil_thres, w)
    assert abs(float(out[0]) - float(loss.detach())) <= 2e-4 * abs(float(loss.detach())), (out, float(loss.detach()))
    pscr = torch.empty(int(lib.gs_pose_grad_scratch_bytes(int(params["means3D"].shape[0]))), dtype=torch.uint8, device=params["means3D"].device)
    d_pose = torch.empty(7, device=params["means3D"].device)
    R.backward_pose_dev(ctx, d_im, d_depth, pscr, d_pose)
    x = params["cam_unnorm_rots"][..., t].detach().clone().requires_grad_(True)
    F.normalize(x).reshape(4).backward(d_pose[:4])                       # (the step kernel's F.normalize Jacobian, here through torch)
    got = torch.cat([x.grad.reshape(4), d_pose[4:]])
    assert PC.rel(got, ref_grad) < rtol, (PC.rel(got, ref_grad), got, ref_grad)


def check_tracking_converges_like_the_reference(device, n=600, W=64, H=48, iters=40, **kw):
    cfg = dict(tracking_iters=iters, sil_thres=0.5, use_depth_loss_thres=False)
    res = {}
    for fused in (False, True):
        params, curr, variables, t, truth = track_scene(n, W, H, device, **kw)
        e0 = pose_error(params, t, truth)
        out = M.track_frame(params, curr, variables, t, cfg, fused=fused)
        assert out["iterations"] == iters and np.isfinite(out["candidate_loss"])
        res[fused] = pose_error(params, t, truth)
    ref, got = res[False], res[True]
    for i in range(2):
        assert ref[i] < 0.5 * e0[i] and got[i] < 0.5 * e0[i], (e0, ref, got)
        assert got[i] <= TRACK_FACTOR * ref[i] + TRACK_MARGIN[i], (e0, ref, got)
    return e0, ref, got


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------------

def check_track_frame_deterministic(device, n=600, W=64, H=48, iters=8, exact=True, **kw):
    """exact=False (the device): the rasteriser's backward sums screen-space gradients with float atomics, so the pose gradient -- and the
    trajectory after it -- may move by fp32 rounding from run to run; the loss of the first iteration (forward and loss kernel only) must
    still repeat to the bit, the rest within DET_ATOL."""
    outs = []
    for _ in range(2):
        params, curr, variables, t, _truth = track_scene(n, W, H, device, **kw)
        out = M.track_frame(params, curr, variables, t, dict(tracking_iters=iters, sil_thres=0.5), fused=True, history=True)
        pose = torch.cat([params["cam_unnorm_rots"][0, :, t], params["cam_trans"][0, :, t]]).detach().cpu()
        assert bool(torch.isfinite(pose).all()) and np.isfinite(out["final_loss"])
        outs.append((pose, out["history"], out["final_loss"], out["candidate_loss"]))
    if exact:
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2:] == outs[1][2:]
    else:
        assert float(outs[0][1][0, 0]) == float(outs[1][1][0, 0])
        assert float((outs[0][0] - outs[1][0]).abs().max()) < DET_ATOL, (outs[0][0], outs[1][0])


# ---- 7. the mapper --------------------------------------------------------------------------------------------------------------------------

def moving_sequence(gt_params, num_frames, W, H, device, yaw_step_deg=1.0, step=(0.004, -0.002, 0.003)):
    """orbit_sequence's spin with small turns that also translates: frame i's w2c = [R_y(i yaw) | i step]."""
    import math
    from activesplat_amd.rasterizer import GaussianRasterizer
    rv = {k: v.to(device) for k, v in syn.activate(gt_params).items()}
    for i in range(num_frames):
        a = math.radians(yaw_step_deg) * i
        c, s = math.cos(a), math.sin(a)
        tr = np.asarray(step, dtype=np.float64) * i
        w2c = np.array([[c, 0, s, tr[0]], [0, 1, 0, tr[1]], [-s, 0, c, tr[2]], [0, 0, 0, 1]], dtype=np.float64)
        cam = setup_camera(W, H, syn.intrinsics(W, H), w2c, device=device)
        with torch.no_grad():
            color, _, depth, opacity = GaussianRasterizer(raster_settings=cam)(means2D=torch.zeros_like(rv["means3D"]), **rv)
        d = torch.where(opacity > 0.5, depth / opacity.clamp_min(1e-6), torch.zeros_like(depth))
        yield dict(id=i, color=color.clamp(0, 1), depth=d, quat=syn.quat_from_yaw(a), position=tr.astype(np.float32), w2c=w2c)


def run_mapper(device, cfg, n_gt=6000, W=64, H=48, frames=11):
    from activesplat_amd.mapper import SplatMapper
    gt = syn.shell_scene(n_gt, seed=2, W=W, H=H)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    seq = list(moving_sequence(gt, frames, W, H, device))
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=frames, **cfg), device=device)
    log = []
    for fr in seq:
        opt_before, it_before = mp.optimizer, mp.stats["iters"]
        mp.run(fr)
        log.append(dict(id=fr["id"], new_opt=mp.optimizer is not opt_before, iters=mp.stats["iters"] - it_before, keyframes=len(mp.keyframe_list)))
    errs = []
    for fr in seq:
        truth = (np.asarray(fr["quat"], dtype=np.float64), np.asarray(fr["position"], dtype=np.float64))
        errs.append(pose_error(mp.params, fr["id"], truth))
    return mp, seq, log, np.array(errs)


def check_schedule(log):
    """tests/test_mapper.py's schedule of the shipped config (map_every = keyframe_every = 5, mapping_iters = 2)."""
    for e in log:
        fid = e["id"]
        assert e["iters"] == (2 if fid % 5 == 0 else 0), e
        assert e["new_opt"] == (fid == 0 or (fid + 1) % 5 == 0), e
    assert log[-1]["keyframes"] == 3


def check_mapper_tracking(device, iters=40, frames=11):
    out = {}
    for fused in (False, True):
        mp, seq, log, errs = run_mapper(device, dict(tracking=dict(use_gt_poses=False, tracking_iters=iters), fused_tracking=fused), frames=frames)
        check_schedule(log)
        assert mp.stats["tracked_frames"] == frames - 1 and mp.stats["tracking_iters"] >= iters * (frames - 1)
        assert np.all(np.isfinite(errs)) and errs[0].max() == 0.0
        for kf in mp.keyframe_list:                                      # keyframes carry the ESTIMATED pose
            q = F.normalize(mp.params["cam_unnorm_rots"][..., kf["id"]].detach())
            w2c = torch.eye(4, device=q.device)
            w2c[:3, :3] = M.build_rotation(q)
            w2c[:3, 3] = mp.params["cam_trans"][..., kf["id"]].detach()
            assert torch.equal(kf["est_w2c"], w2c), kf["id"]
        for fr, g in zip(seq, mp.gt_w2c_all_frames):                     # ... and gt_w2c_all_frames the frame's own
            assert torch.allclose(g.cpu().double(), torch.tensor(fr["w2c"]), atol=1e-6)
        out[fused] = errs
    ref, got = out[False], out[True]
    for i in range(2):
        assert got[:, i].max() <= TRACK_FACTOR * ref[:, i].max() + TRACK_MARGIN[i], (ref, got)
    return ref, got


def check_mapper_default_keeps_frame_poses(device, frames=6):
    mp, seq, log, errs = run_mapper(device, dict(), frames=frames)
    assert mp.stats["tracked_frames"] == 0
    for fr in seq:
        assert torch.equal(mp.params["cam_unnorm_rots"][0, :, fr["id"]].detach().cpu(), torch.tensor(fr["quat"], dtype=torch.float32).reshape(4))
        assert torch.equal(mp.params["cam_trans"][0, :, fr["id"]].detach().cpu(), torch.tensor(fr["position"], dtype=torch.float32).reshape(3))
