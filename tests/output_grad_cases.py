"""Gradients of every image output (differentiable_outputs= of GaussianRasterizer / render_rgbd / render_rgbd_raw): the shared cases of the
emulated (tests/test_output_grads.py) and the GPU (tests/test_gpu_output_grads.py) test files.

The reference is the unchanged fp64 oracle used as two passes: pass 1 is the colour pass; pass 2 renders the per-Gaussian colours [z, 1, z^2]
(z = the view depth) over a black background, so that its three channels are depth, opacity and depth_sq, and takes
oracle.backward(fwd2, [dL/dD, dL/dO, dL/dQ]).  The two gradient sets are added; pass 2's dL/dcolors_precomp is chained into means3D as
(dc0 + 2 z dc2) V[:3, 2].

The bar is check_backward's (tests/parity_cases.py), per gradient tensor: relative L2 below 1e-3, at least 99.5 % of the elements within rtol 1e-3
and atol 1e-6 max|ref|, at most two stray elements for tensors under 400 elements.  A tensor that misses it may be decided by the fp32-oracle tier
(kernel error <= 1.5 x the fp32 oracle's own error + 1e-6): that is printed and counted, and at most TIER2_MAX tensors of one test session may
be decided that way.  There is no decision-matched tier here."""
import numpy as np
import torch
import torch.nn.functional as F

from activesplat_amd import _lib
from activesplat_amd import mapping as M
from activesplat_amd import rasterizer as R
from activesplat_amd import synthetic as syn
from activesplat_amd.camera import setup_camera
from tests import pose_cases as pc
from tests import util

GRAD_RTOL = 1e-3
MIN_FRAC = 0.995
TIER2_MAX = 2
#: tensors compared / decided by the fp32-oracle tier in this process (one test file per session on either machine)
TALLY = {"compared": 0, "tier2": 0, "where": []}

ALL = ("color", "depth", "opacity", "depth_sq")
SCENES = ("plain", "partial", "few_tile", "chained")


def scene(name, device):
    """(settings, render variables) of the issue's four scenes, built as util.scene builds them."""
    if name == "plain":
        return util.scene(400, 64, 48, seed=3, device=device, bg=(0.3, 0.1, 0.7))
    if name == "partial":
        return util.scene(600, 50, 37, seed=5, device=device, bg=(1.0, 1.0, 1.0))
    if name == "few_tile":                                   # check_few_tile_backward_segments' scene: quadrant lists 1-4 k positions deep
        rs, rv = util.scene(20000, 64, 48, seed=41, device=device, scale_jitter=0.4)
        rv["opacities"] = (rv["opacities"] * 0.03).clamp(0, 1)
        rv["scales"] = rv["scales"] * 2.0
        return rs, rv
    if name == "chained":                                    # check_chained_backward's scene: 306 tiles, walks of several chunks
        rs, rv = util.scene(5000, 288, 272, seed=33, device=device, scale_jitter=0.5)
        rv["opacities"] = (rv["opacities"] * 0.15).clamp(0, 1)
        rv["scales"] = rv["scales"] * 3.0
        return rs, rv
    raise KeyError(name)


SEEDS = dict(plain=3, partial=5, few_tile=41, chained=33)


def image_grads(rs, seed, device, which=ALL):
    """dL/d(color, depth, opacity, depth_sq) from torch.randn(seed + 100); outputs not in `which` carry None."""
    H, W = int(rs.image_height), int(rs.image_width)
    g = torch.Generator().manual_seed(seed + 100)
    full = dict(color=torch.randn(3, H, W, generator=g), depth=torch.randn(1, H, W, generator=g), opacity=torch.randn(1, H, W, generator=g),
                depth_sq=torch.randn(1, H, W, generator=g))
    return {k: (v.to(device) if k in which else None) for k, v in full.items()}


def reference(oracle, rs, rv, dL):
    """The two-pass oracle gradients (numpy, the oracle's precision) of sum_k <dL[k], output k>."""
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    H, W = int(rs.image_height), int(rs.image_width)
    real = oracle.real
    img = lambda k, c: np.zeros((c, H, W), real) if dL[k] is None else n(dL[k]).astype(real)  # noqa: E731
    cam = util.cam_dict(rs)
    geo = dict(scales=n(rv["scales"]), rotations=n(rv["rotations"]))
    f1 = oracle.forward(cam, n(rv["means3D"]), n(rv["opacities"]), colors=n(rv["colors_precomp"]), **geo)
    g1 = oracle.backward(f1, img("color", 3))
    V = cam["viewmatrix"].astype(real)
    m = n(rv["means3D"]).astype(real)
    z = m @ V[:3, 2] + V[3, 2]
    f2 = oracle.forward(dict(cam, bg=np.zeros(3, np.float32)), n(rv["means3D"]), n(rv["opacities"]), colors=np.stack([z, np.ones_like(z), z * z], 1), **geo)
    g2 = oracle.backward(f2, np.concatenate([img("depth", 1), img("opacity", 1), img("depth_sq", 1)], 0))
    out = {k: np.asarray(g1[k], np.float64) + np.asarray(g2[k], np.float64) for k in ("means2D", "means3D", "scales", "rotations", "opacities")}
    out["colors_precomp"] = np.asarray(g1["colors_precomp"], np.float64)
    dc = np.asarray(g2["colors_precomp"], np.float64)
    out["means3D"] = out["means3D"] + (dc[:, 0] + 2.0 * z.astype(np.float64) * dc[:, 2])[:, None] * V[:3, 2].astype(np.float64)[None, :]
    out["_pass2"] = dict(depth=f2["color"][0:1], opacity=f2["color"][1:2], depth_sq=f2["color"][2:3])
    out["_pass1"] = dict(color=f1["color"])
    return out


def leaves(rv):
    inp = {k: v.detach().clone().requires_grad_(True) for k, v in rv.items()}
    return inp, torch.zeros(rv["means3D"].shape[0], 3, device=rv["means3D"].device, requires_grad=True)


def loss_of(images, dL):
    """sum_k <dL[k], image k> over the outputs that carry a gradient image"""
    total = None
    for k, im in images.items():
        if dL.get(k) is not None:
            term = (im * dL[k]).sum()
            total = term if total is None else total + term
    return total


def collect(inp, m2d):
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu().numpy() for k, v in inp.items()}
    out["means2D"] = (torch.zeros_like(m2d) if m2d.grad is None else m2d.grad).detach().cpu().numpy()
    return out


def run_rgbd(rs, rv, dL, outputs):
    """render_rgbd with `outputs` requested and the loss sum_k <dL[k], output k> -> (gradients, images)."""
    inp, m2d = leaves(rv)
    color, _radii, depth, sil, dsq = R.render_rgbd(rs, means2D=m2d, differentiable_outputs=outputs, **inp)
    images = dict(color=color, depth=depth, opacity=sil, depth_sq=dsq)
    loss_of(images, dL).backward()
    return collect(inp, m2d), {k: v.detach().cpu().numpy() for k, v in images.items()}


def run_dropin(rs, rv, dL, outputs, frontend):
    """The drop-in call with `outputs` requested, through the C++ front-end or the Python twin."""
    old = R.use_frontend
    R.use_frontend = frontend
    try:
        inp, m2d = leaves(rv)
        color, _radii, depth, opacity = R.GaussianRasterizer(rs, differentiable_outputs=outputs)(means2D=m2d, **inp)
        loss_of(dict(color=color, depth=depth, opacity=opacity), dL).backward()
        return collect(inp, m2d)
    finally:
        R.use_frontend = old


def compare(got, ref, ref32=None, what=""):
    """check_backward's bar for every gradient tensor of `got` against `ref` (fp64); ref32: a callable -> the fp32 oracle's gradients, for tier 2."""
    o32 = None
    for k, g in got.items():
        r = np.asarray(ref[k], np.float64).reshape(g.shape)
        gmax = float(np.abs(r).max()) if r.size else 0.0
        if gmax == 0.0:
            assert g.size == 0 or np.abs(g).max() == 0.0, (what, k)
            continue
        assert np.isfinite(g).all(), (what, k)
        frac = util.close_frac(g, r, GRAD_RTOL, 1e-6 * gmax)
        rel = float(np.linalg.norm(g.astype(np.float64) - r) / np.linalg.norm(r))
        TALLY["compared"] += 1
        if g.size < 400 and round((1.0 - frac) * g.size) <= 2:
            frac = max(frac, MIN_FRAC)
        print(f"output grads {what} {k}: rel {rel:.3e} frac {frac:.5f}")
        if (frac < MIN_FRAC or rel >= 1e-3) and ref32 is not None:
            o32 = ref32() if o32 is None else o32
            o = np.asarray(o32[k], np.float64).reshape(g.shape)
            rel32 = float(np.linalg.norm(o - r) / np.linalg.norm(r))
            frac32 = util.close_frac(o, r, GRAD_RTOL, 1e-6 * gmax)
            TALLY["tier2"] += 1
            TALLY["where"].append((what, k, rel, frac, rel32, frac32))
            print(f"output grads {what} {k}: decided by the fp32-oracle tier: kernel rel {rel:.3e} frac {frac:.5f}, fp32 oracle rel {rel32:.3e} frac {frac32:.5f}")
            assert rel <= 1.5 * rel32 + 1e-6 and (1.0 - frac) <= 1.5 * (1.0 - frac32) + 1e-3, (what, k, rel, rel32, frac, frac32)
            assert TALLY["tier2"] <= TIER2_MAX, TALLY["where"]
            continue
        assert frac >= MIN_FRAC, (what, k, frac)
        assert rel < 1e-3, (what, k, rel)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---- case 1: the silhouette alone carries the loss (raises on a build without the feature) ---------------------------------------------
def check_silhouette_only(device, oracle64, oracle32):
    rs, rv = scene("plain", device)
    dL = image_grads(rs, SEEDS["plain"], device, which=("opacity",))
    got, _ = run_rgbd(rs, rv, dL, ("depth", "silhouette"))
    assert np.abs(got["colors_precomp"]).max() == 0.0           # no colour term in this loss
    ref = reference(oracle64, rs, rv, dL)
    compare(got, ref, lambda: reference(oracle32, rs, rv, dL), "silhouette-only")


# ---- case 2: every output against the reference ------------------------------------------------------------------------------------------
def check_all_outputs(name, device, oracle64, oracle32):
    lib = _lib.get()
    rs, rv = scene(name, device)
    rs = rs._replace(debug=False)
    dL = image_grads(rs, SEEDS[name], device)
    everything = ("depth", "silhouette", "depth_sq")
    try:
        if name == "chained":
            _lib.check(lib.gs_set_backward_chain(3, 256))
        got, images = run_rgbd(rs, rv, dL, everything)
        ref = reference(oracle64, rs, rv, dL)
        # the forward is the one it always was: pass 2's channels are the three fused outputs
        for k, v in ref["_pass2"].items():
            sc = max(1.0, float(np.abs(v).max()))
            assert util.close_frac(images[k], v, 1e-4, 1e-5 * sc) > 0.999, (name, k)
        compare(got, ref, lambda: reference(oracle32, rs, rv, dL), name)
        if name == "few_tile":
            # (a) the silhouette alone keeps the three list segments: against one walker per quadrant
            dLo = image_grads(rs, SEEDS[name], device, which=("color", "opacity"))
            three, _ = run_rgbd(rs, rv, dLo, ("depth", "silhouette"))
            # (b) depth_sq requested: one walker per quadrant whatever the knob says
            three_q = got
            _lib.check(lib.gs_set_backward_segments(1))
            one, _ = run_rgbd(rs, rv, dLo, ("depth", "silhouette"))
            one_q, _ = run_rgbd(rs, rv, dL, everything)
            for k in one:
                assert rel_l2(three[k], one[k]) <= 3e-5, ("silhouette, three segments", k, rel_l2(three[k], one[k]))
                assert rel_l2(three_q[k], one_q[k]) <= 3e-5, ("depth_sq, three segments asked", k, rel_l2(three_q[k], one_q[k]))
        if name == "chained":
            _lib.check(lib.gs_set_backward_chain(1, -1))
            one, _ = run_rgbd(rs, rv, dL, everything)
            for k in one:
                assert rel_l2(got[k], one[k]) <= 2e-5, ("chained", k, rel_l2(got[k], one[k]))
    finally:
        _lib.check(lib.gs_set_backward_segments(3))
        _lib.check(lib.gs_set_backward_chain(3, -1))


# ---- case 3: the drop-in call -------------------------------------------------------------------------------------------------------------
def check_dropin(name, device, oracle64, oracle32, frontend):
    rs, rv = scene(name, device)
    rs = rs._replace(debug=False)
    dL = image_grads(rs, SEEDS[name], device, which=("color", "depth", "opacity"))
    got = run_dropin(rs, rv, dL, ("depth", "opacity"), frontend)
    ref = reference(oracle64, rs, rv, dL)
    compare(got, ref, lambda: reference(oracle32, rs, rv, dL), f"drop-in {name} frontend={frontend}")


# ---- case 4: the raw-parameter path -------------------------------------------------------------------------------------------------------
G_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")


def raw_scene(device):
    """The plain scene as the mapper's parameters, seen from camera 1 of 2 (pose_cases.make_scene's layout)."""
    W, H = 64, 48
    p = syn.make_params(400, W, H, seed=3)
    params = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
    yaw = 0.12
    rots = torch.tensor([[1.0, 0.0, 0.0, 0.0], [np.cos(yaw / 2), 0.03, np.sin(yaw / 2), -0.02]], dtype=torch.float32).T.reshape(1, 4, 2)
    params["cam_unnorm_rots"] = torch.nn.Parameter((rots * 1.3).to(device))
    params["cam_trans"] = torch.nn.Parameter(torch.tensor([[0.0, 0.0, 0.0], [0.05, -0.03, 0.1]], dtype=torch.float32).T.reshape(1, 3, 2).to(device))
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, bg=(0.3, 0.1, 0.7), sh_degree=0)
    return params, cam, 1


def _pose7(params, t):
    q = F.normalize(params["cam_unnorm_rots"][..., t].detach()).reshape(4)
    return torch.cat([q, params["cam_trans"][..., t].detach().reshape(3)]).cpu().tolist()


def _zero(params):
    for v in params.values():
        v.grad = None


def _grads(params, keys=G_KEYS):
    return {k: params[k].grad.detach().clone() for k in keys if params[k].grad is not None}


def run_raw(params, cam, t, dL, outputs, renders=1, accumulate=False, camera=False, gaussians_grad=True):
    _zero(params)
    m2ds = []
    total = None
    for _ in range(renders):
        m2d = torch.empty_like(params["means3D"], requires_grad=True)
        kw = dict(accumulate_grads=accumulate)
        if camera:
            kw.update(camera=(F.normalize(params["cam_unnorm_rots"][..., t]).reshape(4), params["cam_trans"][..., t].reshape(3)), gaussians_grad=gaussians_grad)
        color, _r, depth, sil, dsq = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                        params["unnorm_rotations"], None if camera else _pose7(params, t),
                                                        colors_precomp=params["rgb_colors"], differentiable_outputs=outputs, **kw)
        loss = loss_of(dict(color=color, depth=depth, opacity=sil, depth_sq=dsq), dL)
        total = loss if total is None else total + loss
        m2ds.append(m2d)
    total.backward()
    return _grads(params, G_KEYS + pc.CAM_KEYS), [m.grad.detach().clone() for m in m2ds]


def run_torch_route(params, cam, t, dL, outputs, camera=False, dropin=False):
    """The same loss through torch's activations in front of render_rgbd (dropin: of the drop-in call): fused_rendervar without a camera
    gradient, the reference's transform_to_frame(camera_grad=True) chain with one."""
    _zero(params)
    if camera:
        tg = M.transform_to_frame(params, t, gaussians_grad=True, camera_grad=True)
        rv = M.transformed_params2rendervar(params, tg)
    else:
        rv = M.fused_rendervar(params, t, _pose7(params, t))
    if dropin:
        color, _r, depth, opacity = R.GaussianRasterizer(cam, differentiable_outputs=outputs)(**rv)
        images = dict(color=color, depth=depth, opacity=opacity)
    else:
        col = rv.pop("colors_precomp")
        color, _r, depth, sil, dsq = R.render_rgbd(cam, colors_precomp=col, differentiable_outputs=outputs, **rv)
        images = dict(color=color, depth=depth, opacity=sil, depth_sq=dsq)
    loss_of(images, dL).backward()
    return _grads(params, G_KEYS + pc.CAM_KEYS)


def check_raw(device):
    params, cam, t = raw_scene(device)
    everything = ("depth", "silhouette", "depth_sq")
    dL = image_grads(cam, 3, device)
    ref = run_torch_route(params, cam, t, dL, everything)
    got, _ = run_raw(params, cam, t, dL, everything)
    for k in G_KEYS:
        e = pc.rel(got[k], ref[k])
        print(f"output grads raw {k}: rel {e:.3e}")
        assert e < 3e-4, (k, e)                                   # (check_raw_parameter_mode's bar between the two routes)
    # the part that only the new outputs contribute is not small: the default call differs
    base, _ = run_raw(params, cam, t, dict(dL, opacity=None, depth_sq=None), ("depth",))
    assert pc.rel(base["means3D"], got["means3D"]) > 1e-2
    # accumulate_grads: two renders in one loss add up inside the kernel
    twice, m2 = run_raw(params, cam, t, dL, everything, renders=2, accumulate=True)
    for k in G_KEYS:
        assert pc.rel(twice[k], 2.0 * got[k]) < 1e-5, (k, pc.rel(twice[k], 2.0 * got[k]))
    # camera=: the pose gradient with all outputs of the drop-in call, against torch autograd through transform_to_frame
    dL3 = dict(dL, depth_sq=None)
    ref_cam = run_torch_route(params, cam, t, dL3, ("depth", "opacity"), camera=True, dropin=True)
    got_cam, _ = run_raw(params, cam, t, dL3, ("depth", "silhouette"), camera=True)
    for k in pc.CAM_KEYS:
        e = pc.rel(got_cam[k][..., t], ref_cam[k][..., t])
        print(f"output grads raw {k}: rel {e:.3e}")
        assert bool(torch.isfinite(got_cam[k]).all()) and e < pc.POSE_RTOL, (k, e)
    # ... and with depth_sq on top, against the same chain in front of render_rgbd; the pose-only backward rides on the same moments
    ref_q = run_torch_route(params, cam, t, dL, everything, camera=True)
    got_q, _ = run_raw(params, cam, t, dL, everything, camera=True)
    only_q, _ = run_raw(params, cam, t, dL, everything, camera=True, gaussians_grad=False)
    assert not [k for k in G_KEYS if k in only_q]
    for k in pc.CAM_KEYS:
        assert pc.rel(got_q[k][..., t], ref_q[k][..., t]) < pc.POSE_RTOL, (k, pc.rel(got_q[k][..., t], ref_q[k][..., t]))
        assert pc.rel(only_q[k][..., t], got_q[k][..., t]) < pc.POSE_RTOL, k
    for k in G_KEYS:
        assert pc.rel(got_q[k], got[k]) < 1e-5, k                 # the Gaussians' gradients are those of the call without a camera


# ---- case 5: background identity ----------------------------------------------------------------------------------------------------------
def check_background_identity(name, device):
    """Render A: bg (1, 0, 0), colour channel 0 zero, dL/dC = (h, 0, 0).  Render B: bg 0, dL/dC = 0, dL/dO = -h.  Channel 0 of A is T_final,
    B's loss is -<h, 1 - T_final>: the same function of the parameters up to a constant, so every parameter gradient agrees."""
    lib = _lib.get()
    rs, rv = scene(name, device)
    rs = rs._replace(debug=False)
    H, W = int(rs.image_height), int(rs.image_width)
    rv = dict(rv)
    rv["colors_precomp"] = rv["colors_precomp"].clone()
    rv["colors_precomp"][:, 0] = 0.0
    h = torch.randn(1, H, W, generator=torch.Generator().manual_seed(SEEDS[name] + 100)).to(device)
    zeros = torch.zeros(2, H, W, device=device)
    try:
        if name == "chained":
            _lib.check(lib.gs_set_backward_chain(3, 256))
        a, _ = run_rgbd(rs._replace(bg=torch.tensor([1.0, 0.0, 0.0], device=device)), rv, dict(color=torch.cat([h, zeros], 0)), ("depth",))
        b, _ = run_rgbd(rs._replace(bg=torch.zeros(3, device=device)), rv, dict(color=torch.zeros(3, H, W, device=device), opacity=-h),
                        ("depth", "silhouette"))
    finally:
        _lib.check(lib.gs_set_backward_chain(3, -1))
    for k in a:
        if k == "colors_precomp":                                # A's colour gradient is the blend weights x (h, 0, 0); B has no colour term
            assert np.abs(b[k]).max() == 0.0
            continue
        assert np.abs(a[k]).max() > 0.0, k
        e = rel_l2(b[k], a[k])
        print(f"output grads background identity {name} {k}: rel {e:.3e}")
        assert e <= 1e-5, (name, k, e)


# ---- case 6: defaults unchanged -----------------------------------------------------------------------------------------------------------
def check_defaults(device):
    rs, rv = scene("plain", device)
    rs = rs._replace(debug=False)
    P = rv["means3D"].shape[0]
    for frontend in (True, False):
        old = R.use_frontend
        R.use_frontend = frontend
        try:
            inp, m2d = leaves(rv)
            color, radii, depth, opacity = R.GaussianRasterizer(raster_settings=rs)(means2D=m2d, **inp)
            assert color.requires_grad and not (radii.requires_grad or depth.requires_grad or opacity.requires_grad)
            color, radii, depth, sil, dsq = R.render_rgbd(rs, means2D=m2d, **inp)
            assert color.requires_grad and depth.requires_grad and not (radii.requires_grad or sil.requires_grad or dsq.requires_grad)
            color, radii, depth, sil, dsq = R.render_rgbd(rs, means2D=m2d, differentiable_outputs=("depth", "silhouette", "depth_sq"), **inp)
            assert color.requires_grad and depth.requires_grad and sil.requires_grad and dsq.requires_grad and not radii.requires_grad
            color, radii, depth, sil, dsq = R.render_rgbd(rs, means2D=m2d, differentiable_outputs=("silhouette",), **inp)
            assert sil.requires_grad and not (depth.requires_grad or dsq.requires_grad)
            color, radii, depth, opacity = R.GaussianRasterizer(rs, differentiable_outputs=("opacity",))(means2D=m2d, **inp)
            assert opacity.requires_grad and not depth.requires_grad
        finally:
            R.use_frontend = old
    # outputs requested, the loss on colour and depth only: the default call's gradients (check_fused_rgbd's norm)
    dL = image_grads(rs, 3, device, which=("color", "depth"))
    base, _ = run_rgbd(rs, rv, dL, ("depth",))
    asked, _ = run_rgbd(rs, rv, dL, ("depth", "silhouette", "depth_sq"))
    for k in base:
        d = (asked[k].astype(np.float64) - base[k]).reshape(P, -1)
        e2 = (d ** 2).sum(1)
        scale = max(np.linalg.norm(base[k]), 1e-30)
        assert np.sqrt(max(e2.sum() - np.sort(e2)[-2:].sum(), 0.0)) < 1e-4 * scale, k
        assert np.sqrt(e2.sum()) < 1e-3 * scale, k


# ---- case 7: refusals ---------------------------------------------------------------------------------------------------------------------
def check_refusals(device):
    import pytest
    rs, rv = scene("plain", device)
    inp, m2d = leaves(rv)
    with pytest.raises(Exception, match="differentiable_outputs"):
        R.render_rgbd(rs, means2D=m2d, differentiable_outputs=("depth", "normals"), **inp)
    for bad in ("silhouette", "depth_sq"):
        with pytest.raises(Exception, match="differentiable_outputs"):
            R.GaussianRasterizer(rs, differentiable_outputs=("depth", bad))
    params, cam, t = raw_scene(device)
    opt = object()                                               # (refused on the keyword pair alone, before the optimiser is looked at)
    m2d = torch.empty_like(params["means3D"], requires_grad=True)
    with pytest.raises(Exception, match="adam="):
        R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"], params["unnorm_rotations"], _pose7(params, t),
                          colors_precomp=params["rgb_colors"], adam=opt, differentiable_outputs=("depth", "silhouette"))


# ---- empty scenes --------------------------------------------------------------------------------------------------------------------------
def check_empty(device):
    """P = 0, and a scene wholly behind the camera: zero gradients, no fault."""
    rs, rv = scene("plain", device)
    rs = rs._replace(debug=False)
    dL = image_grads(rs, 3, device)
    everything = ("depth", "silhouette", "depth_sq")
    behind = dict(rv)
    behind["means3D"] = rv["means3D"] * torch.tensor([1.0, 1.0, -1.0], device=device)
    got, images = run_rgbd(rs, behind, dL, everything)
    assert np.abs(images["opacity"]).max() == 0.0 and np.abs(images["depth_sq"]).max() == 0.0
    for k, g in got.items():
        assert np.isfinite(g).all() and np.abs(g).max() == 0.0, k
    none = {k: v[:0] for k, v in rv.items()}
    got, images = run_rgbd(rs, none, dL, everything)
    for k, g in got.items():
        assert g.shape[0] == 0, k
    got = run_dropin(rs, none, dict(dL, depth_sq=None), ("depth", "opacity"), False)
    assert all(g.shape[0] == 0 for g in got.values())
