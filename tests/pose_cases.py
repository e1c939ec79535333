"""Camera-pose gradients of the fused raster paths (tracking and bundle adjustment): shared checks of the emulated (CPU) and the GPU test
files.  The yardstick is torch autograd through the reference's own chain -- transform_to_frame(camera_grad=True) ->
transformed_params2rendervar -> render_rgbd -- on the same library, and an fp64 dense render (oracle/dense_torch.py) on small scenes.

Tolerances (relative L2 over the 7 pose components or over a parameter tensor):
  * fused against the torch chain, POSE_RTOL = 2e-3: both sum the same per-Gaussian fp32 products, but in different orders over P terms
    of both signs (the pose gradient is a sum over every rendered Gaussian with heavy cancellation under a random image gradient), and the
    activations of the torch chain and of the kernels are not bit-identical -- a radius or an alpha = 1/255 decision may flip for a
    boundary Gaussian, which moves that Gaussian's whole share;
  * fused against fp64, F64_RTOL = 5e-3: the fp32 rasteriser itself (colour / depth gradients of single Gaussians agree with the fp64
    oracle to ~1e-4 .. 1e-3, tests/parity_cases.check_backward), summed over the scene;
  * the Gaussians' gradients with and without the pose output: bit-identical (the same kernel arithmetic, the pose share rides along).
"""
import numpy as np
import torch
import torch.nn.functional as F

from activesplat_amd import mapping as M
from activesplat_amd import rasterizer as R
from activesplat_amd import synthetic as syn
from activesplat_amd.camera import setup_camera

POSE_RTOL = 2e-3
F64_RTOL = 5e-3
CAM_KEYS = ("cam_unnorm_rots", "cam_trans")
G_KEYS = ("means3D", "rgb_colors", "shs", "unnorm_rotations", "logit_opacities", "log_scales")


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_scene(n, W, H, device, seed=5, iso=False, sh=False, white=False, bad=False, yaw=0.12, t=(0.05, -0.03, 0.1)):
    """(params, settings, time index): a map of n Gaussians seen from camera 1 of 2 (a yawed, shifted pose)."""
    p = syn.make_params(n, W, H, seed=seed, sh_degree=3 if sh else None)
    if sh:
        p.pop("rgb_colors", None)
    if iso:
        p["log_scales"] = p["log_scales"][:, :1].contiguous()
    params = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
    rots = torch.tensor([[1.0, 0.0, 0.0, 0.0], [np.cos(yaw / 2), 0.03, np.sin(yaw / 2), -0.02]], dtype=torch.float32).T.reshape(1, 4, 2)
    params["cam_unnorm_rots"] = torch.nn.Parameter((rots * 1.3).to(device))           # (unnormalised: F.normalize is on the chain)
    params["cam_trans"] = torch.nn.Parameter(torch.tensor([[0.0, 0.0, 0.0], list(t)], dtype=torch.float32).T.reshape(1, 3, 2).to(device))
    if bad:
        nan, inf = float("nan"), float("inf")
        with torch.no_grad():
            params["means3D"][3, 0] = nan; params["means3D"][4, 2] = inf; params["means3D"][5] = -inf
            params["log_scales"][10, 0] = inf
            params["logit_opacities"][20] = nan
            params["unnorm_rotations"][31, 2] = nan
    bg = (1.0, 1.0, 1.0) if white else (0.0, 0.0, 0.0)
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, bg=bg, sh_degree=3 if sh else 0)
    return params, cam, 1


def _cols(params):
    return dict(shs=params["shs"]) if "shs" in params else dict(colors_precomp=params["rgb_colors"])


def upstream(W, H, device, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)


def run(params, cam, t, mode, dL, gaussians_grad=True):
    """One render of the frame + `L = <dLc, colour> + <dLd, depth>` backward; -> (pose grads {cam key: tensor}, Gaussian grads, means2D.grad).
    mode: 'torch' (the reference chain through transform_to_frame(camera_grad=True)), 'raw' (render_rgbd_raw(camera=...)), 'act'
    (fused_rendervar(camera_grad=True) + render_rgbd)."""
    for v in params.values():
        v.grad = None
    dLc, dLd = dL
    if mode == "torch":
        tg = M.transform_to_frame(params, t, gaussians_grad=gaussians_grad, camera_grad=True)
        rv = M.transformed_params2rendervar(dict(params, rgb_colors=params["shs"]) if "shs" in params else params, tg)
        rv.pop("colors_precomp")
        if not gaussians_grad:
            rv = {k: v.detach() if k in ("opacities", "scales") else v for k, v in rv.items()}
        col = _cols(params) if gaussians_grad else {k: v.detach() for k, v in _cols(params).items()}
        im, _r, depth, _s, _q = R.render_rgbd(cam, **col, **rv)
        m2d = rv["means2D"]
        m2d.retain_grad()
    elif mode == "raw":
        m2d = torch.empty_like(params["means3D"], requires_grad=True)
        camera = (F.normalize(params["cam_unnorm_rots"][..., t]).reshape(4), params["cam_trans"][..., t].reshape(3))
        im, _r, depth, _s, _q = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                  params["unnorm_rotations"], None, camera=camera, gaussians_grad=gaussians_grad, **_cols(params))
    else:
        p2 = dict(params, rgb_colors=params["shs"]) if "shs" in params else params
        rv = M.fused_rendervar(p2, t, camera_grad=True, gaussians_grad=gaussians_grad)
        col = rv.pop("colors_precomp")
        m2d = rv["means2D"]
        im, _r, depth, _s, _q = R.render_rgbd(cam, **({"shs": col} if "shs" in params else {"colors_precomp": col}), **rv)
    ((im * dLc).sum() + (depth * dLd).sum()).backward()
    pose = {k: params[k].grad.clone() for k in CAM_KEYS}
    gauss = {k: params[k].grad.clone() for k in G_KEYS if k in params and params[k].grad is not None}
    return pose, gauss, m2d.grad.clone()


def check_pose_against_torch(device, n, W, H, modes=("raw", "act"), rtol=POSE_RTOL, **kw):
    params, cam, t = make_scene(n, W, H, device, **kw)
    dL = upstream(W, H, device)
    ref = run(params, cam, t, "torch", dL)
    assert all(bool(torch.isfinite(v).all()) for v in ref[0].values()) and float(ref[0]["cam_trans"].norm()) > 0
    for mode in modes:
        got = run(params, cam, t, mode, dL)
        for k in CAM_KEYS:
            assert bool(torch.isfinite(got[0][k]).all()), (mode, k)
            e = rel(got[0][k][..., t], ref[0][k][..., t])
            assert e < rtol, (mode, k, e, got[0][k][..., t].tolist(), ref[0][k][..., t].tolist())
            assert float(got[0][k][..., 1 - t].abs().max()) == 0.0, (mode, k)      # the other frame's pose is not on the chain
    return params, cam, t, dL


def check_nonfinite_scene(device, n=600, W=64, H=48):
    """Culled and non-finite Gaussians: the fused pose gradient is finite and equals the torch chain's on the map WITHOUT those rows (the
    torch chain itself turns one NaN mean into a NaN pose gradient: 0 x NaN in dmean w^T)."""
    params, cam, t = make_scene(n, W, H, device, bad=True)
    dL = upstream(W, H, device)
    bad = [3, 4, 5, 10, 20, 31]
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad] = False
    keep = keep.to(device)
    clean = {k: torch.nn.Parameter(v.detach()[keep].clone()) if k not in CAM_KEYS else torch.nn.Parameter(v.detach().clone())
             for k, v in params.items()}
    ref = run(clean, cam, t, "torch", dL)
    for mode in ("raw", "act"):
        for gg in (True, False):
            got = run(params, cam, t, mode, dL, gaussians_grad=gg)
            for k in CAM_KEYS:
                assert bool(torch.isfinite(got[0][k]).all()), (mode, gg, k, got[0][k])
                assert rel(got[0][k], ref[0][k]) < POSE_RTOL, (mode, gg, k, rel(got[0][k], ref[0][k]))


def check_ba_bit_identity_and_pose_only(device, n=600, W=64, H=48, **kw):
    """With a differentiable camera the Gaussians' gradients are those of the call without one, to the bit; the pose-only backward leaves
    every Gaussian's .grad None and gives the same pose gradient to the bit; two runs give the same bits.  (Bit for bit wherever the blend
    backward's float atomics sum in a fixed order -- the emulated kernels on one OpenMP thread; on the device those sums, and with them
    every gradient of the frame, vary in the last bits from run to run: check_pose_reduction_is_deterministic pins the pose reduction
    itself there.)"""
    params, cam, t = make_scene(n, W, H, device, **kw)
    dL = upstream(W, H, device)
    # raw path without a camera (today's call)
    for v in params.values():
        v.grad = None
    m2d = torch.empty_like(params["means3D"], requires_grad=True)
    q = F.normalize(params["cam_unnorm_rots"][..., t].detach()).reshape(4)
    pose7 = torch.cat([q, params["cam_trans"][..., t].detach().reshape(3)]).cpu().tolist()
    im, _r, depth, _s, _q = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                              params["unnorm_rotations"], pose7, **_cols(params))
    ((im * dL[0]).sum() + (depth * dL[1]).sum()).backward()
    plain = {k: params[k].grad.clone() for k in G_KEYS if k in params and params[k].grad is not None}
    plain_m2d = m2d.grad.clone()
    ba = run(params, cam, t, "raw", dL)
    ba2 = run(params, cam, t, "raw", dL)
    assert set(plain) == set(ba[1])
    for k in plain:
        assert torch.equal(plain[k], ba[1][k]), k
    assert torch.equal(plain_m2d, ba[2])
    for k in CAM_KEYS:
        assert torch.equal(ba[0][k], ba2[0][k]), k
    po = run(params, cam, t, "raw", dL, gaussians_grad=False)
    assert po[1] == {}, sorted(po[1])
    assert all(params[k].grad is None for k in G_KEYS if k in params)
    for k in CAM_KEYS:
        assert torch.equal(po[0][k], ba[0][k]), (k, po[0][k], ba[0][k])
    assert torch.equal(po[2], ba[2])
    # the activation-kernel path: the same three properties
    a1 = run(params, cam, t, "act", dL)
    a2 = run(params, cam, t, "act", dL)
    ap = run(params, cam, t, "act", dL, gaussians_grad=False)
    assert ap[1] == {}
    for k in CAM_KEYS:
        assert torch.equal(a1[0][k], a2[0][k]) and torch.equal(a1[0][k], ap[0][k]), k
    for v in params.values():
        v.grad = None
    p2 = dict(params, rgb_colors=params["shs"]) if "shs" in params else params
    rv = M.fused_rendervar(p2, t, pose7)
    col = rv.pop("colors_precomp")
    im, _r, depth, _s, _q = R.render_rgbd(cam, **({"shs": col} if "shs" in params else {"colors_precomp": col}), **rv)
    ((im * dL[0]).sum() + (depth * dL[1]).sum()).backward()
    for k in a1[1]:
        assert torch.equal(a1[1][k], params[k].grad), k


def _transform_f64(params, t):
    """fp64 restatement of transform_to_frame(camera_grad=True) + transformed_params2rendervar (slam_helpers.py:252-304,124-139)."""
    d = {k: v.detach().double().cpu().requires_grad_(True) for k, v in params.items()}
    q = F.normalize(d["cam_unnorm_rots"][..., t])[0]
    qn = q / q.norm()
    r, x, y, z = qn
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)
    means = d["means3D"] @ Rm.T + d["cam_trans"][..., t][0]
    ls = d["log_scales"]
    if ls.shape[1] == 1:
        rot = F.normalize(d["unnorm_rotations"])
        ls = ls.repeat(1, 3)
    else:
        rot = F.normalize(M.quat_mult(q.expand(d["unnorm_rotations"].shape[0], 4), F.normalize(d["unnorm_rotations"])))
    return d, dict(means3D=means, rotations=rot, opacities=torch.sigmoid(d["logit_opacities"]), scales=torch.exp(ls))


def check_against_fp64(device, n=300, W=48, H=40, rtol=F64_RTOL, **kw):
    from oracle import dense_torch as DT
    from tests import util
    params, cam, t = make_scene(n, W, H, device, **kw)
    dL = upstream(W, H, device)
    d, rv = _transform_f64(params, t)
    col = dict(shs=d["shs"]) if "shs" in d else dict(colors=d["rgb_colors"])
    out = DT.render_dense(util.cam_dict(cam), rv["means3D"], rv["opacities"], scales=rv["scales"], rotations=rv["rotations"], **col)
    ((out["color"] * dL[0].double().cpu()).sum() + (out["depth"] * dL[1].double().cpu()).sum()).backward()
    for mode in ("raw", "act"):
        got = run(params, cam, t, mode, dL)
        for k in CAM_KEYS:
            e = rel(got[0][k][..., t].cpu(), d[k].grad[..., t])
            assert e < rtol, (mode, k, e, got[0][k][..., t].tolist(), d[k].grad[..., t].tolist())


def loss_scene(n, W, H, device, K=4, frozen_camera=False):
    """(params, keyframes) for get_loss: a map of n Gaussians and K keyframes (keyframe i: yaw 0.03 i, shift (0.02 i, 0, 0.01 i)) with random
    colour / depth targets.  frozen_camera: the two camera parameters do not require grad."""
    p = syn.make_params(n, W, H, seed=3)
    params = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
    rots = torch.stack([torch.tensor([np.cos(0.015 * i), 0.0, np.sin(0.015 * i), 0.0]) for i in range(K)], 1).reshape(1, 4, K)
    trans = torch.stack([torch.tensor([0.02 * i, 0.0, 0.01 * i]) for i in range(K)], 1).reshape(1, 3, K)
    params["cam_unnorm_rots"] = torch.nn.Parameter(rots.to(device), requires_grad=not frozen_camera)
    params["cam_trans"] = torch.nn.Parameter(trans.to(device), requires_grad=not frozen_camera)
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device)
    g = torch.Generator().manual_seed(9)
    kfs = [dict(cam=cam, id=i, im=torch.rand(3, H, W, generator=g).to(device), depth=(torch.rand(1, H, W, generator=g) * 3 + 0.5).to(device),
                w2c=torch.eye(4, device=device)) for i in range(K)]
    return params, kfs


def check_frozen_camera(device, n=600, W=64, H=48, exact=True, rtol=2e-5):
    """Camera tensors that do not require grad (a frozen pose): render_rgbd_raw(camera=...) and fused_rendervar(camera_grad=True) back-propagate
    like the calls without a camera (Gaussian gradients bit for bit where the blend's atomic sums are ordered -- exact -- else within rtol), and
    get_loss(do_ba=True) on a map with frozen camera parameters runs on every branch with the unfused call's loss and Gaussian gradients."""
    params, cam, t = make_scene(n, W, H, device)
    for k in CAM_KEYS:
        params[k].requires_grad_(False)
    dL = upstream(W, H, device)
    q = F.normalize(params["cam_unnorm_rots"][..., t]).reshape(4)
    tr = params["cam_trans"][..., t].reshape(3)
    pose7 = torch.cat([q, tr]).cpu().tolist()
    same = (lambda a, b: torch.equal(a, b)) if exact else (lambda a, b: rel(a, b) < rtol)
    for mode in ("raw", "act"):
        got = []
        for with_cam in (False, True):
            for v in params.values():
                v.grad = None
            if mode == "raw":
                m2d = torch.empty_like(params["means3D"], requires_grad=True)
                im, _r, depth, _s, _q = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                          params["unnorm_rotations"], pose7, camera=(q, tr) if with_cam else None, **_cols(params))
            else:
                rv = M.fused_rendervar(params, t, pose7, camera_grad=with_cam)
                im, _r, depth, _s, _q = R.render_rgbd(cam, **rv)
            ((im * dL[0]).sum() + (depth * dL[1]).sum()).backward()
            got.append({k: params[k].grad.clone() for k in G_KEYS if k in params and params[k].grad is not None})
            assert all(params[k].grad is None for k in CAM_KEYS), mode
        assert set(got[0]) == set(got[1]) and got[0], mode
        for k in got[0]:
            assert same(got[0][k], got[1][k]), (mode, k, rel(got[1][k], got[0][k]))
    w = dict(im=0.5, depth=1.0)
    out = {}
    for name, flags in dict(torch=dict(), raw=dict(fused=True, fused_preprocess=True), raw_fl=dict(fused=True, fused_loss=True, fused_preprocess=True),
                            act=dict(fused=True, fused_inputs=True)).items():
        prm, kfs = loss_scene(n, W, H, device, frozen_camera=True)
        variables = {k: torch.zeros(n, device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom")}
        loss, variables, _ = M.get_loss(prm, kfs[2], variables, 2, w, do_ba=True, mapping=True, **flags)
        loss.backward()
        assert all(prm[k].grad is None for k in CAM_KEYS), name
        out[name] = (float(loss.detach()), {k: prm[k].grad.clone() for k in ("means3D", "logit_opacities", "log_scales")})
    for name, o in out.items():
        assert abs(o[0] - out["torch"][0]) <= 2e-4 * abs(out["torch"][0]), (name, o[0], out["torch"][0])
        for k in o[1]:
            assert rel(o[1][k], out["torch"][1][k]) < 3e-4, (name, k, rel(o[1][k], out["torch"][1][k]))


def check_unit_leaf_camera(device, n=600, W=64, H=48, rtol=POSE_RTOL, **kw):
    """A unit camera quaternion passed to render_rgbd_raw(camera=...) AS THE LEAF (no F.normalize in between): its gradient is the reference's
    -- rel_w2c from build_rotation(q), which renormalises, and rot = quat_mult(q, normalize(q_i)) (slam_helpers.py:252-304) -- radial
    component included."""
    params, cam, t = make_scene(n, W, H, device, **kw)
    dL = upstream(W, H, device)
    q0 = F.normalize(params["cam_unnorm_rots"][..., t].detach()).reshape(4)
    t0 = params["cam_trans"][..., t].detach().reshape(3)
    res = []
    for mode in ("torch", "raw"):
        ql, tl = q0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
        if mode == "torch":
            Rm = M.build_rotation(ql[None])[0]
            means = params["means3D"].detach() @ Rm.T + tl
            iso = params["log_scales"].shape[1] == 1
            ur = params["unnorm_rotations"].detach()
            rot = F.normalize(ur if iso else M.quat_mult(ql.expand(ur.shape[0], 4), F.normalize(ur)))
            ls = params["log_scales"].detach()
            im, _r, depth, _s, _q = R.render_rgbd(cam, means3D=means, means2D=torch.zeros_like(means, requires_grad=True),
                                                  opacities=torch.sigmoid(params["logit_opacities"].detach()),
                                                  scales=torch.exp(ls.repeat(1, 3) if iso else ls), rotations=rot,
                                                  **{k: v.detach() for k, v in _cols(params).items()})
        else:
            m2d = torch.empty_like(params["means3D"], requires_grad=True)
            im, _r, depth, _s, _q = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                      params["unnorm_rotations"], None, camera=(ql, tl), gaussians_grad=False, **_cols(params))
        ((im * dL[0]).sum() + (depth * dL[1]).sum()).backward()
        res.append((ql.grad.clone(), tl.grad.clone()))
    for a, b, k in ((res[1][0], res[0][0], "rot"), (res[1][1], res[0][1], "trans")):
        assert rel(a, b) < rtol, (k, rel(a, b), a.tolist(), b.tolist())
    # the radial component is the reference's too (not only what survives a later normalisation)
    rad = lambda g: float((g * q0).sum())  # noqa: E731
    assert abs(rad(res[1][0]) - rad(res[0][0])) <= rtol * float(res[0][0].norm()), (rad(res[1][0]), rad(res[0][0]))


def check_get_loss_modes(device, n=600, W=64, H=48, rtol=POSE_RTOL):
    """get_loss(tracking=True) and get_loss(do_ba=True): the fused branches against the unfused (reference) call -- loss values and camera
    gradients; tracking leaves the Gaussians without gradients on the fused branches."""
    w = dict(im=0.5, depth=1.0)
    flag_sets = dict(torch=dict(), raw=dict(fused=True, fused_preprocess=True), raw_fl=dict(fused=True, fused_loss=True, fused_preprocess=True),
                     act=dict(fused=True, fused_inputs=True), one_pass=dict(fused=True))
    for call in (dict(tracking=True), dict(tracking=True, use_sil_for_loss=False), dict(tracking=True, ignore_outlier_depth_loss=True),
                 dict(do_ba=True, mapping=True), dict(do_ba=True, fused_loss_ok=True)):
        call = dict(call)
        fl_ok = call.pop("fused_loss_ok", False)
        out = {}
        for name, flags in flag_sets.items():
            if name == "raw_fl" and not fl_ok:
                continue
            params, kfs = loss_scene(n, W, H, device)
            variables = {k: torch.zeros(params["means3D"].shape[0], device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom")}
            loss, variables, parts = M.get_loss(params, kfs[2], variables, 2, w, sil_thres=0.5, **flags, **call)
            loss.backward()
            out[name] = (float(loss.detach()), {k: params[k].grad.clone() for k in CAM_KEYS},
                         {k: params[k].grad for k in G_KEYS if k in params}, variables["seen"].clone())
        ref = out["torch"]
        assert float(ref[1]["cam_trans"].norm()) > 0, call
        for name, o in out.items():
            assert abs(o[0] - ref[0]) <= 2e-4 * abs(ref[0]), (call, name, o[0], ref[0])
            for k in CAM_KEYS:
                assert bool(torch.isfinite(o[1][k]).all()), (call, name, k)
                assert rel(o[1][k], ref[1][k]) < rtol, (call, name, k, rel(o[1][k], ref[1][k]))
            if call.get("tracking") and name in ("raw", "act"):
                assert all(g is None for g in o[2].values()), (call, name)
            if call.get("do_ba"):
                for k in ("means3D", "unnorm_rotations", "logit_opacities", "log_scales"):
                    assert rel(o[2][k], ref[2][k]) < 3e-4, (call, name, k, rel(o[2][k], ref[2][k]))
            assert float((o[3] != ref[3]).float().mean()) < 5e-3, (call, name)


class one_openmp_thread:
    """The emulated kernels' block loop on one OpenMP thread: the blend backward's float atomics then sum in a fixed order."""

    def __enter__(self):
        import ctypes
        self.omp = ctypes.CDLL("libgomp.so.1")
        self.before = self.omp.omp_get_max_threads()
        self.omp.omp_set_num_threads(1)

    def __exit__(self, *exc):
        self.omp.omp_set_num_threads(self.before)


def check_close_ba_and_pose_only(device, n=600, W=64, H=48, rtol=2e-5, **kw):
    """The device form of check_ba_bit_identity_and_pose_only, path by path: equal up to the order of the blend backward's atomic sums (an
    isotropic map's rotation gradient is that rounding noise itself -- equal scales make the rotation irrelevant -- and is held to a bound
    relative to the means' gradient instead)."""
    params, cam, t = make_scene(n, W, H, device, **kw)
    dL = upstream(W, H, device)
    q = F.normalize(params["cam_unnorm_rots"][..., t].detach()).reshape(4)
    pose7 = torch.cat([q, params["cam_trans"][..., t].detach().reshape(3)]).cpu().tolist()
    iso = params["log_scales"].shape[1] == 1
    for mode in ("raw", "act"):
        for v in params.values():
            v.grad = None
        if mode == "raw":
            m2d = torch.empty_like(params["means3D"], requires_grad=True)
            im, _r, depth, _s, _q = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                      params["unnorm_rotations"], pose7, **_cols(params))
        else:
            p2 = dict(params, rgb_colors=params["shs"]) if "shs" in params else params
            rv = M.fused_rendervar(p2, t, pose7)
            col = rv.pop("colors_precomp")
            im, _r, depth, _s, _q = R.render_rgbd(cam, **({"shs": col} if "shs" in params else {"colors_precomp": col}), **rv)
        ((im * dL[0]).sum() + (depth * dL[1]).sum()).backward()
        plain = {k: params[k].grad.clone() for k in G_KEYS if k in params and params[k].grad is not None}
        ba = run(params, cam, t, mode, dL)
        po = run(params, cam, t, mode, dL, gaussians_grad=False)
        assert po[1] == {}, (mode, sorted(po[1]))
        assert set(ba[1]) == set(plain), (mode, sorted(ba[1]), sorted(plain))
        for k in plain:
            if iso and k == "unnorm_rotations":
                assert float((ba[1][k] - plain[k]).norm()) < 1e-4 * float(plain["means3D"].norm()), (mode, k)
                continue
            assert rel(ba[1][k], plain[k]) < rtol, (mode, k, rel(ba[1][k], plain[k]))
        for k in CAM_KEYS:
            assert rel(po[0][k], ba[0][k]) < rtol, (mode, k, rel(po[0][k], ba[0][k]))


def check_pose_reduction_is_deterministic(device, n=70000, seed=3):
    """gs_activate_backward_pose on fixed inputs (no rasteriser in front: nothing but the per-Gaussian shares and their reduction), twice and
    in both modes: the same bits every time; against an fp64 sum of the same shares in torch."""
    import ctypes as C
    from activesplat_amd import _lib
    lib = _lib.get()
    g = torch.Generator().manual_seed(seed)
    dev = torch.device(device)
    for iso in (0, 1):
        mk = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
        means, rots, gm, gr = mk(n, 3), mk(n, 4), mk(n, 3), mk(n, 4)
        gm[::7] = 0.0
        gr[::7] = 0.0
        means[::7] = float("nan")                               # rows without an incoming gradient add nothing, whatever they hold
        oo, os_ = torch.rand(n, 1, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
        qc = torch.tensor([0.9, 0.1, -0.3, 0.2])
        qc = qc / qc.norm()
        pose = (C.c_float * 7)(*(qc.tolist() + [0.1, -0.2, 0.3]))
        st = _lib.stream_ptr(dev)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        pscr = torch.empty(int(lib.gs_pose_grad_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        outs = []
        for pose_only in (0, 1, 0, 1):
            d = [torch.empty(n, 3, device=dev), torch.empty(n, 4, device=dev), torch.empty(n, 1, device=dev), torch.empty(n, 1 if iso else 3, device=dev)]
            dp = torch.empty(7, device=dev)
            _lib.check(lib.gs_activate_backward_pose(n, iso, pose, p(means), p(rots), p(oo), p(os_), p(gm), p(gr), None, None,
                                                     *(None if pose_only else p(x) for x in d), 0, pose_only, p(dp), p(pscr), st))
            outs.append(dp.cpu())
        assert all(torch.equal(outs[0], o) for o in outs[1:]), outs
        # fp64 restatement of the same sum
        live = (gm.abs().sum(1) + gr.abs().sum(1)) > 0
        w, dmean, q, gg = (x.double().cpu()[live.cpu()] for x in (means, gm, rots, gr))
        qcd = qc.double().requires_grad_(True)
        tt = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64, requires_grad=True)
        r, x, y, z = qcd / qcd.norm()                          # (build_rotation's normalisation is on the chain)
        Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                          2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)
        L = ((w @ Rm.T + tt) * dmean).sum()
        if not iso:
            rot = F.normalize(M.quat_mult(qcd.expand(q.shape[0], 4), F.normalize(q)))
            L = L + (rot * gg).sum()
        L.backward()
        ref = torch.cat([qcd.grad, tt.grad])
        assert rel(outs[0], ref) < 1e-5, (iso, outs[0], ref)
