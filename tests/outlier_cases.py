"""ignore_outlier_depth_loss on the fused paths (gs_depth_error_median, gs_mapping_loss_outlier, gs_tracking_loss_outlier and their wiring in
activesplat_amd.mapping / mapper): shared checks of the emulated (CPU) and the GPU test files.

The rule (src/mapper/splatam/splatam.py:220-228), all in fp32:
    err = |gt_depth - depth| * (gt_depth > 0);  median = torch.median(err) (the lower median over ALL pixels, NaN if any err is NaN);
    keep = err < 10 * median;  mask = keep & gt_depth > 0 & !isnan(depth) & !isnan(depth_sq - depth^2) [& silhouette > sil_thres]
References are restated here with torch on the CPU: every DECISION (torch.median, <, the mask) is a plain fp32 torch op and is held to the bit;
the SUMS over the resulting mask are float64 (the rule of tests/mapstep_cases.py).

Tolerances:
  * the median: bit-identical (a NaN reference asks for a NaN);
  * mapping loss: depth term and loss rtol 5e-6, dL/ddepth rtol 1e-6 and exactly 0 off the mask (mapstep_cases.check_mapping_loss's for the same
    sums); dL/dim and the image term bit-identical to the call without the option (the option must not touch the image term).  On the device the
    image term's partial sums meet in float atomics, so ITS value may move by their order between two calls: IM_TERM_RTOL = 1e-6 there;
  * tracking loss: tracking_cases.LOSS_RTOL on the three values, the gradient images bit-identical (signed zeros included), a second call
    identical;
  * end to end: the rules of the checks they mirror (parity_cases.check_mapping_iteration_without_autograd, check_get_loss_random_draw's loss
    tiers, tracking_cases.check_first_iteration_parity / check_tracking_converges_like_the_reference / check_track_frame_deterministic /
    check_mapper_tracking).
"""
import ctypes as C
import math

import numpy as np
import torch

from activesplat_amd import _lib
from activesplat_amd import mapping as M
from activesplat_amd import optim as O
from tests import mapstep_cases as MC
from tests import pose_cases as PC
from tests import tracking_cases as T

W_IM, W_DEPTH = MC.W_IM, MC.W_DEPTH
CHUNK, AUTO_GRID = 2048, 64                    # the library's automatic grid: one workgroup per CHUNK pixels, at most AUTO_GRID (gs_common.h)
IM_TERM_RTOL = 1e-6


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# =====================================================================================================================================
# A. the median
# =====================================================================================================================================
MEDIAN_FRAMES = [(1, 1), (1, 2), (7, 9), (8, 9), (33, 47), (120, 160)]
MEDIAN_LARGE = [(256, 256), (480, 640)]
MEDIAN_VARIANTS = ("random", "all_gt_zero", "ties", "shared_high_bits", "inf_render", "nan_render", "nan_gt", "even_n", "subnormal")


def median_inputs(H, W, variant, seed=0):
    """-> rendered depth, measured depth [H,W] (float32, CPU).  The first seven are mapstep_cases.GROW_VARIANTS, restated."""
    g = torch.Generator().manual_seed(100 * seed + 13 * H + W + 977 * MEDIAN_VARIANTS.index(variant))
    n = H * W
    gt = torch.rand(H, W, generator=g) * 6.5 + 0.3
    rd = gt + torch.randn(H, W, generator=g) * 0.5
    gt[: H // 3, : W // 2] = 0.0
    if variant == "all_gt_zero":                 # median 0
        gt.zero_()
    elif variant == "ties":                      # multiples of 1/8: many equal errors
        gt = torch.randint(0, 40, (H, W), generator=g).float() / 8
        rd = torch.randint(0, 48, (H, W), generator=g).float() / 8
    elif variant == "shared_high_bits":          # the errors agree in their top 22 bits: the third pass decides
        gt = torch.ones(H, W)
        low = torch.rand(H, W, generator=g) < 0.6
        k = torch.randint(0, 512, (H, W), generator=g).float()
        j = torch.randint(0, 1024, (H, W), generator=g).float()
        rd = torch.where(low, 2.0 + k * 2.0 ** -22, 3.0 + j * 2.0 ** -22)
    elif variant == "inf_render":
        rd.view(-1)[n - 1] = float("inf")
    elif variant == "nan_render":
        rd.view(-1)[n // 2] = float("nan")
    elif variant == "nan_gt":
        gt.view(-1)[n - 1] = float("nan")
    elif variant == "even_n":                    # n distinct exact errors k / 1024 in a random order: the two middle values differ
        gt = torch.full((H, W), 4.0)
        rd = gt + (torch.randperm(n, generator=g).float().reshape(H, W) + 1.0) / 1024.0
    elif variant == "subnormal":                 # every error is a subnormal number
        gt = torch.randint(1, 1000, (H, W), generator=g).float() * 2.0 ** -149
        rd = torch.randint(0, 1000, (H, W), generator=g).float() * 2.0 ** -149
    return rd, gt


def median_reference(rd, gt):
    return ((gt - rd).abs() * (gt > 0)).median()


def _same_bits(got, want):
    got, want = got.reshape(1).cpu(), want.reshape(1).cpu()
    if bool(torch.isnan(want)):
        return bool(torch.isnan(got))
    return torch.equal(got.view(torch.int32), want.view(torch.int32))


def check_median(device, H, W, variant):
    lib = _lib.get()
    rd, gt = median_inputs(H, W, variant)
    want = median_reference(rd, gt)
    if variant == "all_gt_zero":
        assert float(want) == 0.0
    if variant in ("nan_render", "nan_gt"):
        assert math.isnan(float(want))
    if variant == "subnormal":
        assert 0.0 < float(want) < 2.0 ** -126
    if variant == "even_n" and H * W % 2 == 0:
        assert float(want) == (H * W // 2) / 1024.0          # the LOWER of the two middle values
    auto = int(lib.gs_depth_error_median_workgroups(W, H))
    assert auto >= 1 and auto == int(lib.gs_depth_error_median_workgroups(H * W, 1))          # a function of n only
    d, g = rd[None].to(device), gt[None].to(device)
    for grid in (1, None):
        a = M.depth_error_median(d, g, grid=grid)
        b = M.depth_error_median(d, g, grid=grid)
        assert a.device.type == torch.device(device).type and a.numel() == 1
        print("median", f"{H}x{W}", variant, "grid", grid or auto, "got", float(a), "want", float(want))
        assert _same_bits(a, want), (H, W, variant, grid, float(a), float(want))
        assert _same_bits(b, want) and (torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))), (H, W, variant, grid)


def chunk_edge_frames():
    """Three frames with n one below, at and one above TWICE the library's per-workgroup pixel chunk (read from the library: the largest n
    that still gets one workgroup): the ragged last workgroup and the change G -> G + 1.  A library that runs one workgroup at every size has
    no such edge; the frames then straddle 4096 pixels."""
    lib = _lib.get()
    G = lambda n: int(lib.gs_depth_error_median_workgroups(n, 1))  # noqa: E731
    lo, hi = 1, 1 << 22
    if G(hi) == 1:
        return [(1, 4095), (1, 4096), (1, 4097)], None
    while lo < hi:                                   # the largest n with G(n) == 1 (G does not decrease with n)
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if G(mid) == 1 else (lo, mid - 1)
    c = lo
    assert G(c) == 1 and G(c + 1) == 2 and G(2 * c) == 2 and G(2 * c + 1) == 3, (c, G(2 * c), G(2 * c + 1))
    return [(1, 2 * c - 1), (1, 2 * c), (1, 2 * c + 1)], c


def check_median_at_chunk_edges(device, variant):
    frames, _chunk = chunk_edge_frames()
    for H, W in frames:
        check_median(device, H, W, variant)


# =====================================================================================================================================
# B. the loss kernels
# =====================================================================================================================================
def displace(depth, gen, every=16):
    """n / `every` random pixels of `depth` [1,H,W] moved by +-(0.5 .. 2.0), in place -> the pixel indices."""
    n = depth.numel()
    idx = torch.randperm(n, generator=gen)[: max(1, n // every)]
    amount = (0.5 + 1.5 * torch.rand(idx.numel(), generator=gen)) * (torch.randint(0, 2, (idx.numel(),), generator=gen).float() * 2 - 1)
    depth.view(-1)[idx] += amount.to(depth.dtype)
    return idx


def outlier_depths(H, W, seed=0, special=None):
    """-> depth, depth_sq, gt_depth [1,H,W] (float32, CPU): the rendered depth within 2 % of the measured one, a sixteenth of the pixels displaced
    by +-(0.5 .. 2.0), a block without measurement, NaN in depth_sq only.  special: 'majority_unmeasured' (median 0) | 'nan' (one NaN in depth)."""
    g = torch.Generator().manual_seed(5000 + 1000 * seed + 7 * H + W)
    n = H * W
    gt = torch.rand(1, H, W, generator=g) * 3 + 0.5
    d = gt + 0.02 * torch.randn(1, H, W, generator=g)
    displace(d, g)
    gt[0, : H // 3, : W // 2] = 0.0
    dsq = d * d + 0.1
    idx = torch.randperm(n, generator=g)
    dsq.view(-1)[idx[: min(40, n // 8)]] = float("nan")
    d.view(-1)[idx[40:50]] = gt.view(-1)[idx[40:50]]                     # depth == gt depth: sign 0
    if special == "majority_unmeasured":
        gt.view(-1)[idx[: n // 2 + 1]] = 0.0
    elif special == "nan":
        d.view(-1)[idx[-1]] = float("nan")
    return d, dsq, gt


def boundary_depths():
    """4 x 8, gt = 2: errors 17 x 0.0625, 8 x 0.03125, 3 x 0.625, 2 x (0.625 + 2^-20), 2 x 0.5: median 0.0625, 10 median = 0.625 exactly; 27
    pixels kept, the three AT the threshold excluded by the strict <."""
    e = torch.tensor([0.0625] * 17 + [0.03125] * 8 + [0.625] * 3 + [0.625 + 2.0 ** -20] * 2 + [0.5] * 2)
    e = e[torch.randperm(32, generator=torch.Generator().manual_seed(3))]
    sign = torch.tensor([1.0, -1.0]).repeat(16)
    gt = torch.full((1, 4, 8), 2.0)
    d = gt + (e * sign).reshape(1, 4, 8)
    assert torch.equal((gt - d).abs().reshape(-1), e)
    return d, d * d + 0.1, gt


def outlier_mask(d, dsq, gt, sil=None, sil_thres=None):
    """-> (mask, median, keep), fp32 decisions as get_loss takes them."""
    mask = gt > 0
    err = (gt - d).abs() * mask
    med = err.median()
    keep = err < 10 * med
    mask = mask & keep & ~torch.isnan(d) & ~torch.isnan(dsq - d ** 2)
    if sil is not None:
        mask = mask & (sil > sil_thres)
    return mask, med, keep


LOSS_SPECIALS = ("boundary", "majority_unmeasured", "nan")


def mapping_loss_inputs(H, W, special=None):
    if special == "boundary":
        d, dsq, gt = boundary_depths()
        H, W = 4, 8
    else:
        d, dsq, gt = outlier_depths(H, W, special=special)
    im, _d, _q, gt_im, _g = MC.loss_inputs(H, W, "noise")
    return im, d, dsq, gt_im, gt


def check_mapping_loss(device, H, W, special=None, im_exact=True):
    im, d, dsq, gt_im, gt = mapping_loss_inputs(H, W, special)
    H, W = int(d.shape[1]), int(d.shape[2])
    mask, med, keep = outlier_mask(d, dsq, gt)
    measured = (gt > 0)
    empty = special in ("majority_unmeasured", "nan")
    if special == "boundary":
        assert float(med) == 0.0625 and int(mask.sum()) == 27 and int(((gt - d).abs() == 0.625).sum()) == 3
    elif special == "majority_unmeasured":
        assert float(med) == 0.0 and not mask.any()
    elif special == "nan":
        assert math.isnan(float(med)) and not mask.any()
    else:
        assert 0 < int((measured & ~keep).sum()) < int(measured.sum()) and mask.any()          # neither full nor empty
    count = int(mask.sum())
    ref_im = MC.loss_reference64(im, d, dsq, gt_im, gt)["im"]
    ref_depth = W_DEPTH * float((gt.double() - d.double()).abs()[mask].sum()) / count if count else float("nan")
    ref_gd = torch.where(mask, W_DEPTH * torch.sign(d.double() - gt.double()) / max(count, 1), torch.zeros((), dtype=torch.float64))
    w = dict(im=W_IM, depth=W_DEPTH)
    dev = lambda t: t.clone().to(device)  # noqa: E731
    a0 = dev(im).requires_grad_(True)
    loss0, parts0 = M.fused_mapping_loss(a0, dev(d), dev(dsq), dev(gt_im), dev(gt), w)          # without the option: the image term's yardstick
    loss0.backward()
    for call in range(2):                                                                         # both parities of the persistent scratch
        a, dd = dev(im).requires_grad_(True), dev(d).requires_grad_(True)
        loss, parts = M.fused_mapping_loss(a, dd, dev(dsq), dev(gt_im), dev(gt), w, ignore_outlier_depth_loss=True)
        loss.backward()
        got = dict(loss=loss.item(), im=parts["im"].item(), depth=parts["depth"].item())
        g_im, g_depth = a.grad.cpu(), dd.grad.cpu()
        print("mapping loss", f"{H}x{W}", special, "call", call, got, "ref depth", ref_depth, "ref im", ref_im, "kept", count, "of", int(measured.sum()))
        assert torch.equal(g_im, a0.grad.cpu()) and torch.isfinite(g_im).all(), "dL/dim moved with the option"
        if im_exact:
            assert got["im"] == parts0["im"].item()
        else:
            np.testing.assert_allclose(got["im"], parts0["im"].item(), rtol=IM_TERM_RTOL, atol=0)
        np.testing.assert_allclose(got["im"], ref_im, rtol=5e-6, atol=0, err_msg="image term")
        if empty:
            assert math.isnan(got["depth"]) and math.isnan(got["loss"])
            assert torch.count_nonzero(g_depth) == 0
        else:
            np.testing.assert_allclose(got["depth"], ref_depth, rtol=5e-6, atol=0, err_msg="depth term")
            np.testing.assert_allclose(got["loss"], ref_depth + ref_im, rtol=5e-6, atol=0, err_msg="loss")
            np.testing.assert_allclose(g_depth.numpy(), ref_gd.numpy(), rtol=1e-6, atol=0)
            assert torch.count_nonzero(g_depth[~mask]) == 0
            assert torch.equal(g_depth != 0, mask & (d != gt))


TRACK_SIZES = [(45, 67), (480, 640)]


def tracking_loss_inputs(H, W, special=None, sil_thres=0.99, seed=0):
    if special == "boundary":
        d, dsq, gtd = boundary_depths()
        H, W = 4, 8
    else:
        d, dsq, gtd = outlier_depths(H, W, seed=seed + 1, special=special)
    g = torch.Generator().manual_seed(77 + seed + H + W)
    n = H * W
    im, gt = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    sil = torch.rand(1, H, W, generator=g)
    idx = torch.randperm(n, generator=g)
    sil.view(-1)[idx[: n // 16]] = float(np.float32(sil_thres))           # silhouette exactly at the threshold: excluded
    sil.view(-1)[idx[n // 16: n // 2]] = 1.0
    im.view(3, -1)[:, idx[-(n // 16 + 1):]] = gt.view(3, -1)[:, idx[-(n // 16 + 1):]]        # im == gt: sign 0
    return im, gt, d, dsq, gtd, sil


def torch_tracking_loss(im, gt, depth, dsq, gtd, sil, use_sil, sil_thres, w):
    """get_loss's tracking branch with ignore_outlier_depth_loss (splatam.py:220-249, use_l1), autograd on im and depth."""
    im, depth = im.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    unc = (dsq - depth ** 2).detach()
    mask = gtd > 0
    err = (gtd - depth).abs() * mask
    mask = mask & (err < 10 * err.median())
    mask = mask & ~torch.isnan(depth) & ~torch.isnan(unc)
    if use_sil:
        mask = mask & (sil > sil_thres)
    mask = mask.detach()
    losses = {"depth": (gtd - depth).abs()[mask].sum(), "im": (gt - im).abs()[torch.tile(mask, (3, 1, 1))].sum()}
    weighted = {k: v * w[k] for k, v in losses.items()}
    loss = sum(weighted.values())
    loss.backward()
    return (float(loss.detach()), float(weighted["depth"].detach()), float(weighted["im"].detach()), im.grad, depth.grad), mask


def kernel_tracking_loss(im, gt, depth, dsq, gtd, sil, use_sil, sil_thres, w, median=None):
    """gs_depth_error_median + gs_tracking_loss_outlier; median: a given device scalar instead of the select's."""
    lib = _lib.get()
    H, W = int(im.shape[1]), int(im.shape[2])
    dev = im.device
    grads = torch.empty(4, H, W, dtype=torch.float32, device=dev)
    rows = torch.empty(int(lib.gs_tracking_loss_scratch_bytes(W, H)), dtype=torch.uint8, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    med = M.depth_error_median(depth, gtd) if median is None else median
    _lib.check(lib.gs_tracking_loss_outlier(W, H, _p(im), _p(gt), _p(depth), _p(dsq), _p(gtd), _p(sil if use_sil else None), 1 if use_sil else 0,
                                            float(sil_thres), float(w["im"]), float(w["depth"]), _p(grads[:3]), _p(grads[3:]), _p(rows), _p(out),
                                            _p(med), _lib.stream_ptr(dev)))
    return out.cpu(), grads[:3].cpu(), grads[3:].cpu()


def check_tracking_loss(device, H, W, special=None, sil_thres=0.99):
    w = dict(im=0.5, depth=1.0)
    cpu = tracking_loss_inputs(H, W, special, sil_thres)
    ins = [x.to(device) for x in cpu]
    for use_sil in (True, False):
        ref, mask = torch_tracking_loss(*cpu, use_sil, sil_thres, w)
        out, d_im, d_depth = kernel_tracking_loss(*ins, use_sil, sil_thres, w)
        print("tracking loss", tuple(cpu[2].shape[1:]), special, "use_sil", use_sil, out.tolist(), ref[:3], "mask", int(mask.sum()))
        if special in ("majority_unmeasured", "nan"):
            assert not mask.any() and out.tolist() == [0.0, 0.0, 0.0] and ref[:3] == (0.0, 0.0, 0.0)
            assert torch.count_nonzero(d_im) == 0 and torch.count_nonzero(d_depth) == 0
        else:
            assert mask.any() and not mask.all()
        for got, want in zip(out.tolist(), ref[:3]):
            assert abs(got - want) <= T.LOSS_RTOL * abs(want), (use_sil, out.tolist(), ref[:3])
        assert torch.equal(d_im, ref[3]) and torch.equal(d_depth, ref[4]), use_sil
        assert torch.equal(torch.signbit(d_im), torch.signbit(ref[3])) and torch.equal(torch.signbit(d_depth), torch.signbit(ref[4])), use_sil
        out2, d_im2, d_depth2 = kernel_tracking_loss(*ins, use_sil, sil_thres, w)
        assert torch.equal(out, out2) and torch.equal(d_im, d_im2) and torch.equal(d_depth, d_depth2), use_sil


# ---- an infinite median is the plain rule: err < 10 inf holds for every finite error -------------------------------------------------------

def check_infinite_median_is_the_plain_mapping_loss(device, H=37, W=50, exact=True):
    """gs_mapping_loss against gs_mapping_loss_outlier(d_median = +inf) on one scratch each (memset form): the depth mask and every output
    equal.  The gradient images and the mask count (an exact fp32 sum of ones, inside dL/ddepth) to the bit.  The three loss values too with
    exact (the emulated kernels on one host thread); on the device they meet in float atomics, whose order may move their last bits between
    two calls: IM_TERM_RTOL."""
    lib = _lib.get()
    for special in (None, "boundary"):
        im, d, dsq, gt_im, gt = [x.to(device).contiguous() for x in mapping_loss_inputs(H, W, special)]
        h, w = int(d.shape[1]), int(d.shape[2])
        inf = torch.full((1,), float("inf"), device=device)
        res = []
        for outlier in (False, True):
            scratch = torch.zeros(int(lib.gs_mapping_loss_scratch_bytes(w, h)), dtype=torch.uint8, device=device)
            losses = torch.empty(4, device=device)
            grads = torch.empty(4, h, w, device=device)
            args = (w, h, _p(im), _p(gt_im), _p(d), _p(dsq), _p(gt), W_IM, W_DEPTH, _p(losses), _p(grads[:3]), _p(grads[3:]), _p(scratch), 0)
            if outlier:
                _lib.check(lib.gs_mapping_loss_outlier(*args, _p(inf), _lib.stream_ptr(im.device)))
            else:
                _lib.check(lib.gs_mapping_loss(*args, _lib.stream_ptr(im.device)))
            res.append((losses.cpu(), grads.cpu()))
        (la, ga), (lb, gb) = res
        assert torch.isfinite(la).all() and torch.equal(ga, gb), special
        if exact:                                    # (the emulated kernels on one host thread: the atomics meet in one order)
            assert torch.equal(la, lb), (special, la, lb)
        else:
            np.testing.assert_allclose(lb.numpy(), la.numpy(), rtol=IM_TERM_RTOL, atol=0)
        assert int(torch.count_nonzero(ga[3])) > 0


def check_infinite_median_is_the_plain_tracking_loss(device, H=45, W=67, sil_thres=0.99):
    """gs_tracking_loss(use_sil = 1) against gs_tracking_loss_outlier(use_sil = 1, d_median = +inf): the outlier form's colour mask is always the
    tiled mask, which is the plain form's with use_sil.  Rows, not atomics: everything to the bit."""
    w = dict(im=0.5, depth=1.0)
    for ins in (T.loss_inputs(W, H, device, sil_thres=sil_thres), [x.to(device) for x in tracking_loss_inputs(H, W, None, sil_thres)]):
        inf = torch.full((1,), float("inf"), device=device)
        a = T.kernel_tracking_loss(*ins, True, sil_thres, w)
        b = kernel_tracking_loss(*ins, True, sil_thres, w, median=inf)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].cpu(), b[1]) and torch.equal(a[2].cpu(), b[2])
        assert torch.equal(torch.signbit(a[1].cpu()), torch.signbit(b[1])) and torch.equal(torch.signbit(a[2].cpu()), torch.signbit(b[2]))
        assert float(a[0][1]) > 0.0


# =====================================================================================================================================
# C. end to end
# =====================================================================================================================================
def outlier_scene(device, n=600, W=64, H=48, **kw):
    """tracking_cases.track_scene with the outlier displacement applied to the frame's measured depth.  The camera column is track_scene's
    perturbed pose, so the rendered depth differs from the measured one everywhere by a small error (a median well above zero) and by
    0.5 .. 2.0 at the displaced pixels."""
    params, curr, variables, t, truth = T.track_scene(n, W, H, device, **kw)
    g = torch.Generator().manual_seed(91)
    depth = curr["depth"].detach().cpu().clone()
    displace(depth, g)
    curr["depth"] = depth.to(device)
    return params, curr, variables, t, truth


MAP_LRS = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)


def check_mapping_iteration_with_the_option(device, exact=True, steps=3):
    """mapping_iteration(ignore_outlier_depth_loss=True) against get_loss(fused..., fused_adam=, ignore_outlier_depth_loss=True) + backward +
    step: the rule of parity_cases.check_mapping_iteration_without_autograd."""
    w = dict(im=0.5, depth=1.0)
    outs = []
    for direct in (False, True):
        params, curr, var, t, truth = outlier_scene(device)
        var["timestep"] = torch.zeros_like(var["denom"])
        opt = O.initialize_optimizer(params, MAP_LRS)
        for _ in range(steps):
            if direct:
                loss, var, parts = M.mapping_iteration(params, curr, var, t, w, opt, ignore_outlier_depth_loss=True)
                assert all(p.grad is None for p in params.values())
            else:
                loss, var, parts = M.get_loss(params, curr, var, t, w, fused=True, fused_loss=True, fused_preprocess=True, fused_adam=opt,
                                              ignore_outlier_depth_loss=True)
                loss.backward(M.unit_gradient(loss))
                with torch.no_grad():
                    opt.step(); opt.zero_grad(set_to_none=True)
        outs.append(({k: v.detach().clone() for k, v in params.items()},
                     {k: (opt.state[v]["exp_avg"].clone(), int(opt.state[v]["step"])) for k, v in params.items() if v in opt.state and len(opt.state[v])},
                     var["means2D"].grad.clone(), var["seen"].clone(), var["max_2D_radius"].clone(), float(loss.detach()), float(parts["im"]),
                     float(parts["depth"])))
    a, b = outs
    print("mapping_iteration with the option: loss", a[5], b[5], "depth", a[7], b[7])
    assert math.isfinite(a[5]) and a[7] > 0.0
    tol = 0.0 if exact else 1e-6
    assert abs(a[5] - b[5]) <= tol * abs(a[5]) and abs(a[6] - b[6]) <= tol * abs(a[6]) and abs(a[7] - b[7]) <= tol * abs(a[7])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for k in a[1]:
        assert a[1][k][1] == b[1][k][1] == steps, k
    if exact:
        assert torch.equal(a[2], b[2])
        assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and all(torch.equal(a[1][k][0], b[1][k][0]) for k in a[1])
    else:
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))  # noqa: E731
        assert rel(a[2], b[2]) < 5e-5
        for k in a[1]:
            assert rel(a[1][k][0], b[1][k][0]) < 5e-5, (k, rel(a[1][k][0], b[1][k][0]))


class _count_library_calls:
    """Counts the calls of gs_depth_error_median[_grid], gs_mapping_loss_outlier and gs_mapping_loss through the bound library until undo()."""

    def __init__(self):
        self.lib, self.median, self.outlier, self.plain = _lib.get(), 0, 0, 0
        self.real = {k: getattr(self.lib, k) for k in ("gs_depth_error_median", "gs_depth_error_median_grid", "gs_mapping_loss_outlier",
                                                       "gs_mapping_loss")}
        for name, field in (("gs_depth_error_median", "median"), ("gs_depth_error_median_grid", "median"),
                            ("gs_mapping_loss_outlier", "outlier"), ("gs_mapping_loss", "plain")):
            setattr(self.lib, name, self._wrap(self.real[name], field))

    def _wrap(self, fn, field):
        def call(*a):
            setattr(self, field, getattr(self, field) + 1)
            return fn(*a)
        return call

    def undo(self):
        for k, v in self.real.items():
            setattr(self.lib, k, v)


def check_fused_loss_against_the_reference_pattern(device):
    """get_loss(fused=True, fused_loss=True, fused_preprocess=True, ignore_outlier_depth_loss=True) against get_loss(ignore_outlier_depth_loss=
    True) on the unfused torch path: loss 2e-5, parts 5e-5 (+ 1e-7), check_get_loss_random_draw's tiers.  The reference's own mask must reject a
    pixel and keep one, and the fused call must reach gs_depth_error_median and gs_mapping_loss_outlier (a quiet fall-back to the torch loss
    would give the same numbers)."""
    w = dict(im=0.5, depth=1.0)
    out = []
    for fused in (False, True):
        params, curr, var, t, truth = outlier_scene(device)
        if not fused:
            with torch.no_grad():                                       # the reference's depth pass (get_loss's own calls), its mask
                tg = M.transform_to_frame(params, t, gaussians_grad=False, camera_grad=False)
                depth_sil, _, _, _ = M.Renderer(raster_settings=curr["cam"])(**M.transformed_params2depthplussilhouette(params, curr["w2c"], tg))
                d, dsq = depth_sil[0:1], depth_sil[2:3]
                mask, med, keep = outlier_mask(d, dsq, curr["depth"])
                measured = curr["depth"] > 0
                print("reference mask: median", float(med), "measured", int(measured.sum()), "rejected", int((measured & ~keep).sum()), "kept", int(mask.sum()))
                assert int((measured & ~keep).sum()) >= 1 and int(mask.sum()) >= 1
        kw = dict(fused=True, fused_loss=True, fused_preprocess=True) if fused else {}
        calls = _count_library_calls()
        try:
            loss, var, parts = M.get_loss(params, curr, var, t, w, ignore_outlier_depth_loss=True, **kw)
        finally:
            calls.undo()
        # the fused call IS the kernel path -- one select, one outlier loss, no plain loss -- and the reference call touches neither
        assert (calls.median, calls.outlier, calls.plain) == ((1, 1, 0) if fused else (0, 0, 0)), (fused, calls.median, calls.outlier, calls.plain)
        if fused:                                                       # (and the statistics came out of the render: stats_in_render)
            assert var["seen"].dtype == torch.bool and var["seen"].shape == var["max_2D_radius"].shape and bool(var["seen"].any())
        out.append((float(loss.detach()), {k: float(v.detach()) for k, v in parts.items()}))
    x, y = out
    print("get_loss with the option: reference", x, "fused", y)
    assert abs(x[0] - y[0]) <= 2e-5 * abs(x[0]) + 1e-7, ("loss", x[0], y[0])
    for k in x[1]:
        assert abs(x[1][k] - y[1][k]) <= 5e-5 * abs(x[1][k]) + 1e-7, ("part", k, x[1][k], y[1][k])


TRACK_CFG = dict(sil_thres=0.5, ignore_outlier_depth_loss=True)


def check_first_tracking_iteration(device, **kw):
    """The pose column after ONE fused iteration with the option against the reference pattern (get_loss(tracking=True,
    ignore_outlier_depth_loss=True), backward, torch Adam with eps 1e-8): tracking_cases.POSE_RTOL."""
    params, curr, variables, t, _truth = outlier_scene(device, **kw)
    cfg = M.tracking_config(TRACK_CFG)
    ref_p = T.clone_params(params)
    opt = O.initialize_optimizer({k: ref_p[k] for k in ("cam_unnorm_rots", "cam_trans")}, cfg["lrs"], tracking=True)
    loss, _v, parts = M.get_loss(ref_p, curr, {k: v.clone() for k, v in variables.items()}, t, cfg["loss_weights"], cfg["use_sil_for_loss"],
                                 cfg["sil_thres"], cfg["use_l1"], True, tracking=True)
    loss.backward()
    opt.step()
    before = torch.cat([params["cam_unnorm_rots"][0, :, t], params["cam_trans"][0, :, t]]).detach().clone()
    H, W = int(curr["im"].shape[1]), int(curr["im"].shape[2])
    state = M.TrackingState(params, W, H)
    state.begin(params, t)
    row = torch.empty(10, device=params["means3D"].device)
    M.tracking_iteration(params, curr, variables, t, cfg, state, row)
    got = torch.cat([params["cam_unnorm_rots"][0, :, t], params["cam_trans"][0, :, t]]).detach()
    want = torch.cat([ref_p["cam_unnorm_rots"][0, :, t], ref_p["cam_trans"][0, :, t]]).detach()
    print("first tracking iteration: loss", float(row[0]), float(loss.detach()), "step", (got - before).tolist(), "rel", PC.rel(got, want))
    assert abs(float(row[0]) - float(loss.detach())) <= 2e-4 * abs(float(loss.detach()))
    assert float((got - before).abs().min()) > 0.0 and PC.rel(got - before, want - before) < T.POSE_RTOL, (got, want)
    assert PC.rel(got, want) < T.POSE_RTOL


def check_track_frame_with_the_option(device, iters=40, exact=True):
    """track_frame(fused=True) with the option on an outlier-corrupted frame: converges like track_frame(fused=False) under TRACK_FACTOR /
    TRACK_MARGIN, and repeats under check_track_frame_deterministic's rule."""
    cfg = dict(TRACK_CFG, tracking_iters=iters, use_depth_loss_thres=False)
    res = {}
    for fused in (False, True):
        params, curr, variables, t, truth = outlier_scene(device)
        e0 = T.pose_error(params, t, truth)
        out = M.track_frame(params, curr, variables, t, cfg, fused=fused)
        assert out["iterations"] == iters and np.isfinite(out["candidate_loss"])
        res[fused] = T.pose_error(params, t, truth)
    ref, got = res[False], res[True]
    print("track_frame with the option: initial", e0, "reference", ref, "fused", got)
    for i in range(2):
        assert ref[i] < 0.5 * e0[i] and got[i] < 0.5 * e0[i], (e0, ref, got)
        assert got[i] <= T.TRACK_FACTOR * ref[i] + T.TRACK_MARGIN[i], (e0, ref, got)
    outs = []
    for _ in range(2):
        params, curr, variables, t, _truth = outlier_scene(device)
        out = M.track_frame(params, curr, variables, t, dict(TRACK_CFG, tracking_iters=8), fused=True, history=True)
        pose = torch.cat([params["cam_unnorm_rots"][0, :, t], params["cam_trans"][0, :, t]]).detach().cpu()
        assert bool(torch.isfinite(pose).all()) and np.isfinite(out["final_loss"])
        outs.append((pose, out["history"], out["final_loss"], out["candidate_loss"]))
    if exact:
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2:] == outs[1][2:]
    else:
        assert float(outs[0][1][0, 0]) == float(outs[1][1][0, 0])
        assert float((outs[0][0] - outs[1][0]).abs().max()) < T.DET_ATOL, (outs[0][0], outs[1][0])


FUSED_MAPPER = dict(fused_render=True, fused_loss=True, fused_preprocess=True, fused_adam=True, fused_iteration=True, fused_growth=True,
                    fused_tracking=True)


def check_mapper_with_the_option(device, iters=40, frames=11):
    """SplatMapper over 11 frames at 64 x 48 with the option on for tracking AND mapping: every fused flag against the reference pattern, under
    tracking_cases.check_mapper_tracking's rule; every mapping iteration of the fused mapper goes through mapping.mapping_iteration."""
    out, direct_calls = {}, []
    real = M.mapping_iteration

    def counted(*a, **kw):
        direct_calls.append(bool(kw.get("ignore_outlier_depth_loss", False)))
        return real(*a, **kw)

    for fused in (False, True):
        cfg = dict(tracking=dict(use_gt_poses=False, tracking_iters=iters, ignore_outlier_depth_loss=True),
                   mapping=dict(ignore_outlier_depth_loss=True), **(FUSED_MAPPER if fused else {}))
        M.mapping_iteration = counted
        try:
            mp, seq, log, errs = T.run_mapper(device, cfg, frames=frames)
        finally:
            M.mapping_iteration = real
        T.check_schedule(log)
        assert mp.cfg["tracking"]["ignore_outlier_depth_loss"] and mp.cfg["mapping"]["ignore_outlier_depth_loss"]
        assert mp.stats["tracked_frames"] == frames - 1 and mp.stats["tracking_iters"] >= iters * (frames - 1)
        assert np.all(np.isfinite(errs)) and errs[0].max() == 0.0
        assert all(bool(torch.isfinite(v).all()) for v in mp.params.values())
        if fused:
            assert len(direct_calls) == mp.stats["iters"] > 0 and all(direct_calls), (len(direct_calls), mp.stats["iters"])
        else:
            assert not direct_calls
        out[fused] = errs
    ref, got = out[False], out[True]
    print("mapper with the option: reference", ref.max(0), "fused", got.max(0))
    for i in range(2):
        assert got[:, i].max() <= T.TRACK_FACTOR * ref[:, i].max() + T.TRACK_MARGIN[i], (ref, got)
