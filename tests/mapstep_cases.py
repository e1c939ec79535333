"""Shared cases of the mapping step's non-raster kernels -- loss.hip, grow.hip, compact.hip, densify.hip, activate.hip -- against references
restated HERE: torch in float64, or plain integer / boolean torch ops.  No reference calls the library (activesplat_amd._lib, optim.build_index,
optim.gather_rows or any kernel-backed function).  Run twice: tests/test_mapstep_fp64.py on the host-emulated kernels,
tests/test_gpu_mapstep_fp64.py on the device.

The rule for fp32 kernels whose error depends on the input (cancelling SSIM moments, normalisation chains): the kernel's error against float64
may be at most 2 x the error of the fp32 torch mirror -- an independent fp32 evaluation of the same formula on the same inputs, evaluated inside
the test -- with a floor for the cases where the mirror is accidentally exact.  Every other bound is derived from the number format next to it.

Every check prints the figures it asserts on and appends them to REPORT (profiles/README.md holds the device's)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

REPORT = []
U = 2.0 ** -24            # unit roundoff of float32


def _say(section, **kw):
    REPORT.append(dict(section=section, **kw))
    print(section, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


# =====================================================================================================================================
# A. gs_mapping_loss
# =====================================================================================================================================
W_IM, W_DEPTH = 0.5, 1.0
LOSS_SHAPES = [(1, 1), (5, 7), (11, 300), (16, 16), (17, 33), (37, 50), (96, 128), (160, 176)]
LOSS_KINDS = ("noise", "smooth", "flat", "bright", "equal")


def _smooth_field(H, W, g):
    """[3,H,W] float64 in 0.2 .. 0.8: one low-frequency wave per channel."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing="ij")
    f = torch.rand(3, 3, generator=g, dtype=torch.float64)
    return torch.stack([0.5 + 0.3 * torch.sin(2 * math.pi * ((0.5 + 1.5 * f[c, 0]) * xx + (0.5 + 1.5 * f[c, 1]) * yy + f[c, 2])) for c in range(3)])


def loss_inputs(H, W, kind, all_invalid=False, seed=0):
    """-> im, depth, depth_sq, gt_im, gt_depth (float32, CPU).  gt_depth has a block of zeros, depth a few NaN pixels and depth_sq one
    (where the image is large enough to hold them next to valid pixels); all_invalid: no pixel has gt_depth > 0."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 131 * LOSS_KINDS.index(kind))
    n = lambda s: torch.randn(3, H, W, generator=g, dtype=torch.float64) * s  # noqa: E731
    if kind == "noise":
        gt, im = torch.rand(3, H, W, generator=g, dtype=torch.float64), torch.rand(3, H, W, generator=g, dtype=torch.float64)
    elif kind == "smooth":                      # a late mapping iteration: the render within 1 % of a smooth target
        gt = _smooth_field(H, W, g); im = gt + n(0.01)
    elif kind == "flat":
        gt, im = 0.7 + n(1e-3), 0.7 + n(1e-3)
    elif kind == "bright":
        gt = 0.95 + 0.02 * (_smooth_field(H, W, g) - 0.2) / 0.6; im = gt + n(1e-4)
    elif kind == "equal":
        gt = _smooth_field(H, W, g); im = gt.clone()
    gt, im = gt.float(), im.float()
    if kind == "equal":
        im = gt.clone()
    depth = torch.rand(1, H, W, generator=g) * 3 + 0.5
    gt_depth = torch.rand(1, H, W, generator=g) * 3 + 0.5
    depth_sq = depth ** 2 + 0.1
    gt_depth[0, : H // 3, : W // 2] = 0.0
    npix = H * W
    if npix >= 8:
        depth.view(-1)[[npix // 2, npix - 2, npix - 1]] = float("nan")
        depth_sq.view(-1)[npix // 2 + 1] = float("nan")
    if all_invalid:
        gt_depth.zero_()
    return im, depth, depth_sq, gt, gt_depth


def _ssim64(a, b):
    """mean SSIM of two [3,H,W] float64 images: 11 x 11 Gaussian window (sigma 1.5) built from its formula, zero padding 5,
    C1 = 0.01^2, C2 = 0.03^2 (the header of loss.hip)."""
    i = torch.arange(11, dtype=torch.float64)
    w = torch.exp(-(i - 5) ** 2 / 4.5)
    w = w / w.sum()
    w2 = torch.outer(w, w).expand(3, 1, 11, 11).contiguous()
    conv = lambda x: F.conv2d(x[None], w2, padding=5, groups=3)[0]  # noqa: E731
    m1, m2 = conv(a), conv(b)
    s11, s22, s12 = conv(a * a) - m1 * m1, conv(b * b) - m2 * m2, conv(a * b) - m1 * m2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s11 + s22 + c2))).mean()


def loss_reference64(im, depth, depth_sq, gt_im, gt_depth):
    im, depth = im.double().requires_grad_(True), depth.double().requires_grad_(True)
    depth_sq, gt_im, gt_depth = depth_sq.double(), gt_im.double(), gt_depth.double()
    mask = (gt_depth > 0) & ~torch.isnan(depth.detach()) & ~torch.isnan(depth_sq - depth.detach() ** 2)
    l_depth = W_DEPTH * (gt_depth - depth).abs()[mask].mean()
    l_im = W_IM * (0.8 * (im - gt_im).abs().mean() + 0.2 * (1.0 - _ssim64(im, gt_im)))
    (l_depth + l_im).backward()
    return dict(loss=(l_depth + l_im).item(), im=l_im.item(), depth=l_depth.item(), g_im=im.grad, g_depth=depth.grad, mask=mask)


def loss_mirror32_grad(im, gt_im):
    """dL/dim of the fp32 torch mirror (mapping.calc_ssim + l1_loss_v1, CPU float32)."""
    from activesplat_amd import mapping as M
    x = im.clone().float().requires_grad_(True)
    (W_IM * (0.8 * M.l1_loss_v1(x, gt_im) + 0.2 * (1.0 - M.calc_ssim(x, gt_im)))).backward()
    return x.grad


def _grad_errors(g, g64, H, W):
    """e_inf = max |g - g64| / s and the relative L2 error, s = max(max |g64|, one L1 step): the L1 step 0.8 w_im / (3 H W) gives im == gt
    (whose gradient is zero) a scale; the L2 norm of g64 gets the same floor, the norm of an image of L1 steps."""
    g, g64 = g.double(), g64.double()
    step = 0.8 * W_IM / (3 * H * W)
    s = max(float(g64.abs().max()), step)
    return float((g - g64).abs().max()) / s, float((g - g64).norm()) / max(float(g64.norm()), step * math.sqrt(3 * H * W))


def check_mapping_loss(device, H, W, kind, all_invalid=False):
    """Two calls in a row on the same stream (both parities of the persistent scratch), each against float64.  The image term holds
    1 - mean SSIM: rtol 5e-6 of it on a render close to its target (the term is 1e-3 .. 1e-5 there, and exactly 0 for im == gt) is met because
    loss.hip sums 1 - SSIM from centred moments; a kernel that forms 1 - (a float32 mean of values near 1) from raw second moments misses it
    by 1e-4 .. 7e-3 relative."""
    from activesplat_amd import mapping as M
    im, depth, depth_sq, gt_im, gt_depth = loss_inputs(H, W, kind, all_invalid)
    ref = loss_reference64(im, depth, depth_sq, gt_im, gt_depth)
    mirror = _grad_errors(loss_mirror32_grad(im, gt_im), ref["g_im"], H, W)
    for call in range(2):
        a, d = im.clone().to(device).requires_grad_(True), depth.clone().to(device).requires_grad_(True)
        loss, parts = M.fused_mapping_loss(a, d, depth_sq.to(device), gt_im.to(device), gt_depth.to(device), dict(im=W_IM, depth=W_DEPTH))
        loss.backward()
        got = dict(loss=loss.item(), im=parts["im"].item(), depth=parts["depth"].item())
        g_im, g_depth = a.grad.cpu(), d.grad.cpu()
        kern = _grad_errors(g_im, ref["g_im"], H, W)
        _say("loss", kind=kind + ("/invalid" if all_invalid else ""), shape=f"{H}x{W}", call=call, kernel_einf=kern[0], mirror_einf=mirror[0],
             kernel_l2=kern[1], mirror_l2=mirror[1], rel_im=abs(got["im"] - ref["im"]) / max(abs(ref["im"]), 1e-300),
             abs_im=abs(got["im"] - ref["im"]))
        np.testing.assert_allclose(got["im"], ref["im"], rtol=5e-6, atol=0, err_msg="image term")
        if all_invalid:
            assert math.isnan(got["depth"]) and math.isnan(ref["depth"]) and math.isnan(got["loss"]) and math.isnan(ref["loss"])
            assert not ref["mask"].any() and torch.count_nonzero(g_depth) == 0 and torch.count_nonzero(ref["g_depth"]) == 0
        else:
            np.testing.assert_allclose(got["depth"], ref["depth"], rtol=5e-6, atol=0, err_msg="depth term")
            np.testing.assert_allclose(got["loss"], ref["loss"], rtol=5e-6, atol=0, err_msg="loss")
            # dL/ddepth = w_depth sgn(depth - gt) / count (float64 autograd's own expression of it); exactly 0 on masked pixels
            np.testing.assert_allclose(g_depth.numpy(), ref["g_depth"].numpy(), rtol=1e-6, atol=0)
            assert torch.count_nonzero(g_depth[~ref["mask"]]) == 0 and ref["mask"].any()
        assert torch.isfinite(g_im).all()
        assert kern[0] <= max(2 * mirror[0], 1e-6), f"dL/dim e_inf {kern[0]:.3e} vs mirror {mirror[0]:.3e}"
        assert kern[1] <= max(2 * mirror[1], 1e-6), f"dL/dim relative L2 {kern[1]:.3e} vs mirror {mirror[1]:.3e}"
        assert kern[1] <= 1e-3


# =====================================================================================================================================
# B. gs_grow_gaussians
# =====================================================================================================================================
GROW_FRAMES = [(1, 1), (1, 2), (7, 9), (8, 9), (33, 47), (160, 120), (32, 64), (1, 2049)]      # the last two: at, and one pixel past, a kMedianChunk boundary of the select
GROW_VARIANTS = ("random", "all_gt_zero", "ties", "shared_high_bits", "inf_render", "nan_render", "nan_gt")
SIL_THRES = 0.5


def grow_inputs(H, W, variant, seed=0):
    """-> render_depth, silhouette, gt_depth [H,W], color [3,H,W] (float32, CPU)."""
    g = torch.Generator().manual_seed(100 * seed + 13 * H + W + 977 * GROW_VARIANTS.index(variant))
    n = H * W
    color = torch.rand(3, H, W, generator=g)
    sil = 1.0 - 0.6 * torch.rand(H, W, generator=g) ** 2                 # ~9 % below the threshold: the depth test decides the rest
    gt = torch.rand(H, W, generator=g) * 6.5 + 0.3                         # some beyond the 5 m limit
    rd = gt + torch.randn(H, W, generator=g) * 0.5
    gt[: H // 3, : W // 2] = 0.0
    if variant == "all_gt_zero":
        gt.zero_()
    elif variant == "ties":
        # multiples of 1/8: every error is exact, many pixels have err == 2 median exactly and the strict > decides
        gt = torch.randint(0, 40, (H, W), generator=g).float() / 8
        rd = torch.randint(0, 48, (H, W), generator=g).float() / 8
    elif variant == "shared_high_bits":
        # gt = 1; ~60 % of the errors are 1 + k 2^-22 (k < 512: they differ in their low 10 bits only, so the third histogram pass picks the
        # median), the rest 2 + j 2^-22 (j < 1024) = 2 median + (j - 2 k_median) 2^-22: which of them exceed 2 median hangs on the exact k
        gt = torch.ones(H, W)
        low = torch.rand(H, W, generator=g) < 0.6
        k = torch.randint(0, 512, (H, W), generator=g).float()
        j = torch.randint(0, 1024, (H, W), generator=g).float()
        rd = torch.where(low, 2.0 + k * 2.0 ** -22, 3.0 + j * 2.0 ** -22)
        sil = torch.ones(H, W)
    elif variant == "inf_render":
        rd.view(-1)[n - 1] = float("inf")                                   # (where gt > 0: inf * 0 would be a NaN error)
    elif variant == "nan_render":
        rd.view(-1)[n // 2] = float("nan")
    elif variant == "nan_gt":
        gt.view(-1)[n - 1] = float("nan")
    return rd, sil, gt, color


def grow_camera(H, W):
    K = np.array([[0.9 * W + 3.3, 0.0, W / 2 - 0.3], [0.0, 0.8 * W + 2.1, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    a, b = 0.4, -0.25
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = Ry @ Rx, [0.7, -1.3, 2.1]
    return K, c2w


def grow_reference(rd, sil, gt, color, K, c2w, iso):
    """splatam.py:340-364 on float32 CPU tensors (the decisions are fp32 comparisons: bit-exact; torch.median = the lower median, NaN if any
    error is NaN) -> n_cand, the chosen pixels (row-major), and the rows in float64."""
    err = (gt - rd).abs() * (gt > 0)
    behind = (rd > gt) & (err > 2 * err.median())
    cand = ((sil < SIL_THRES) | (behind & (sil > SIL_THRES) & (gt < 5))).reshape(-1)
    take = cand & (gt > 0).reshape(-1)
    pix = torch.nonzero(take).reshape(-1)
    H, W = gt.shape
    z = gt.reshape(-1)[pix].double()
    u, v = (pix % W).double(), (pix // W).double()
    cam = torch.stack(((u - K[0][2]) / K[0][0] * z, (v - K[1][2]) / K[1][1] * z, z), dim=1)
    m = torch.from_numpy(np.asarray(c2w, dtype=np.float64))
    ls = torch.log(torch.sqrt((z / ((K[0][0] + K[1][1]) / 2)) ** 2))[:, None]
    rot = torch.zeros(pix.numel(), 4); rot[:, 0] = 1.0
    return int(cand.sum()), dict(means3D=cam @ m[:3, :3].T + m[:3, 3], rgb_colors=color.reshape(3, -1)[:, pix].T.contiguous(), unnorm_rotations=rot,
                                 logit_opacities=torch.zeros(pix.numel(), 1), log_scales=ls if iso else ls.repeat(1, 3))


def check_grow(device, H, W, variant):
    from activesplat_amd import mapping as M
    rd, sil, gt, color = grow_inputs(H, W, variant)
    K, c2w = grow_camera(H, W)
    if H * W > 1000:                                     # the inputs are what their names say
        err = (gt - rd).abs() * (gt > 0)
        med = err.median()
        if variant == "ties":
            assert int((err == 2 * med).sum()) > 5 and int((err > 2 * med).sum()) > 5
        if variant == "shared_high_bits":
            bits = err.view(torch.int32)
            assert int((bits >> 10 == med.view(torch.int32) >> 10).sum()) > H * W // 2
            assert int((err > 2 * med).sum()) > 5 and int(((err >= 2) & (err <= 2 * med)).sum()) > 5
        if variant in ("nan_render", "nan_gt"):
            assert bool(med.isnan())
        if variant == "inf_render":
            assert bool(err.isinf().any()) and bool(med.isfinite())
    for dist in ("isotropic", "anisotropic"):
        n_cand, want = grow_reference(rd, sil, gt, color, K, c2w, dist == "isotropic")
        rows, got_cand = M.grow_rows(rd.to(device), sil.to(device), gt.to(device), color.to(device), K, c2w, SIL_THRES, dist)
        n_new = want["means3D"].shape[0]
        print("grow", variant, f"{H}x{W}", dist, "candidates", got_cand, "reference", n_cand, "rows", rows["means3D"].shape[0], "reference", n_new)
        assert got_cand == n_cand, f"{variant} {H}x{W}: {got_cand} candidates, the reference pattern gives {n_cand}"
        assert rows["means3D"].shape[0] == n_new
        rows = {k: v.cpu() for k, v in rows.items()}
        assert torch.equal(rows["rgb_colors"], want["rgb_colors"])                      # row-major pixel order
        assert torch.equal(rows["unnorm_rotations"], want["unnorm_rotations"]) and torch.equal(rows["logit_opacities"], want["logit_opacities"])
        for k in ("means3D", "log_scales"):
            assert rows[k].shape == want[k].shape
            np.testing.assert_allclose(rows[k].numpy(), want[k].numpy(), atol=5e-6, rtol=1e-5, err_msg=k)
    return n_cand, n_new


# =====================================================================================================================================
# C. compaction, gather, densify
# =====================================================================================================================================
COMPACT_N = [1, 63, 64, 65, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1025, 2 ** 21 + 7]
COMPACT_MASKS = ("random37", "first", "last", "all", "none", "block_edges")
SURGERY_N = 2 ** 20 + 1025


def compact_mask(n, kind, device, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + n % 100003)
    if kind == "random37":
        m = torch.rand(n, generator=g) < 0.37
    elif kind == "all":
        m = torch.ones(n, dtype=torch.bool)
    else:
        m = torch.zeros(n, dtype=torch.bool)
        if kind == "first":
            m[0] = True
        elif kind == "last":
            m[n - 1] = True
        elif kind == "block_edges":                # first and last row of every 1024-block
            m[0::1024] = True
            m[1023::1024] = True
    return m.to(device)


def check_build_index(device, n):
    from activesplat_amd import optim as O
    for kind in COMPACT_MASKS:
        m = compact_mask(n, kind, device)
        got = O.build_index(m)
        want = torch.nonzero(m).reshape(-1).to(torch.int32)
        assert got.dtype == torch.int32 and torch.equal(got, want), f"n={n} mask={kind}: {got.numel()} rows, torch.nonzero gives {want.numel()}"


def check_compact_index3(device, n):
    """gs_compact_index3 called directly: [rows of a | rows of b | repeat_c blocks of the rows of c] and the three counts."""
    from activesplat_amd import _lib
    from activesplat_amd import optim as O
    lib = _lib.get()
    for rep in (1, 2, 3):
        a, b, c = (compact_mask(n, "random37", device, seed=3 * rep + i).to(torch.uint8).contiguous() for i in range(3))
        idx = torch.full((n * (2 + rep),), -1, dtype=torch.int32, device=device)
        cnt = torch.zeros(3, dtype=torch.int32, device=device)
        scratch = torch.empty(int(lib.gs_compact3_scratch_bytes(n)), dtype=torch.uint8, device=device)
        _lib.check(lib.gs_compact_index3(n, a.data_ptr(), b.data_ptr(), c.data_ptr(), rep, idx.data_ptr(), cnt.data_ptr(), scratch.data_ptr(),
                                         O._stream(idx)))
        nz = lambda m: torch.nonzero(m).reshape(-1)  # noqa: E731
        want = torch.cat((nz(a), nz(b), nz(c).repeat(rep))).to(torch.int32)
        assert cnt.tolist() == [int(a.sum()), int(b.sum()), int(c.sum())], f"n={n} repeat_c={rep}"
        assert torch.equal(idx[: want.numel()], want), f"n={n} repeat_c={rep}"
        assert bool((idx[want.numel():] == -1).all())              # nothing written behind the list


GATHER_CAP = 256 * 16 * 256           # elements one pass of the capped grid covers (float4s on the vec4 path)


def check_gather_rows(device, width, misaligned=False):
    """Just past one pass of the capped grid, an index list with repeats, a zero tail of 5 rows.  misaligned: the source is a view one 3-float
    row into its buffer -- not 16-byte aligned, which sends a width that is a multiple of 4 to the scalar kernel."""
    from activesplat_amd import optim as O
    g = torch.Generator().manual_seed(width + (100 if misaligned else 0))
    per_row = width // 4 if width % 4 == 0 and not misaligned else width
    n_out = GATHER_CAP // per_row + 77
    n_src = 5003
    buf = torch.randn(3 + n_src * width, generator=g).to(device)
    src = buf[3:].view(n_src, width) if misaligned else buf[: n_src * width].view(n_src, width)
    assert src.is_contiguous() and (src.data_ptr() % 16 != 0) == misaligned
    index = torch.randint(0, n_src, (n_out,), generator=g).to(torch.int32).to(device)
    assert n_out * per_row > GATHER_CAP and index.unique().numel() < n_out
    want = src[index.long()]
    got = O.gather_rows(src, index)
    assert got.shape == want.shape and torch.equal(got, want), f"width {width}"
    got = O.gather_rows_zero_tail(src, index, n_out - 5)
    want[n_out - 5:] = 0.0
    assert torch.equal(got, want) and torch.count_nonzero(want[n_out - 6]) > 0, f"width {width} (zero tail)"


KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
SCENE_RADIUS, GRAD_THRESH, N_INTO, OPACITY_THRESH = 1.7, 0.0002, 2, 0.05
LRS = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)


def surgery_map(N, iso, seed):
    """A map on which every densify / prune branch fires, as plain CPU tensors: params, exp_avg, exp_avg_sq, stats.  The decisions are fp32
    comparisons of exp / sigmoid / a quotient with a threshold, and two correct fp32 evaluations may round differently: every input is moved at
    least 1e-3 (relative, or in the logarithm) away from every threshold it is compared with, so the decisions are the same for any of them."""
    g = torch.Generator().manual_seed(seed)
    ls = torch.randn(N, 1 if iso else 3, generator=g) * 0.9 - 4.0
    for t in (0.01 * SCENE_RADIUS, 0.1 * SCENE_RADIUS, 0.1 * SCENE_RADIUS * 0.8 * N_INTO):        # clone | split, too big, a child too big
        ls[(ls - math.log(t)).abs() < 1e-3] = math.log(t) + 2e-3
    logit = torch.randn(N, 1, generator=g) * 3
    t = math.log(OPACITY_THRESH / (1 - OPACITY_THRESH))
    logit[(logit - t).abs() < 1e-3] = t + 2e-3
    params = dict(means3D=torch.randn(N, 3, generator=g), rgb_colors=torch.rand(N, 3, generator=g), unnorm_rotations=torch.randn(N, 4, generator=g),
                  logit_opacities=logit, log_scales=ls)
    exp_avg = {k: torch.randn(v.shape, generator=g) for k, v in params.items()}
    exp_avg_sq = {k: torch.rand(v.shape, generator=g) for k, v in params.items()}
    denom = (torch.rand(N, generator=g) * 3).floor()
    accum = torch.rand(N, generator=g) * 4e-4
    accum[(denom == 0) & (torch.rand(N, generator=g) < 0.5)] = 0.0                                  # 0 / 0
    score = accum / denom
    accum[(score / GRAD_THRESH - 1).abs() < 1e-3] *= 1.01
    assert not ((accum / denom / GRAD_THRESH - 1).abs() < 1e-3).any()
    stats = dict(means2D_gradient_accum=accum, denom=denom, max_2D_radius=torch.rand(N, generator=g), timestep=torch.arange(N).float())
    return params, exp_avg, exp_avg_sq, stats


def _on_device(device, params, exp_avg, exp_avg_sq, stats):
    """-> the product's objects: Parameters, a GaussianAdam whose state holds the given moments (step 1), variables."""
    from activesplat_amd import optim as O
    P = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in params.items()}
    P["cam_unnorm_rots"] = torch.nn.Parameter(torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1).repeat(1, 1, 2).to(device))
    P["cam_trans"] = torch.nn.Parameter(torch.zeros(1, 3, 2, device=device))
    opt = O.initialize_optimizer(P, LRS)
    for k in KEYS:
        opt.state[P[k]] = {"step": 1, "exp_avg": exp_avg[k].clone().to(device), "exp_avg_sq": exp_avg_sq[k].clone().to(device)}
    var = {k: v.clone().to(device) for k, v in stats.items()}
    var["scene_radius"] = torch.tensor(SCENE_RADIUS, device=device)
    return P, opt, var


def _same_event(device, got, want, n_exact=None):
    """got = (params, optimizer, variables) of the product, want = (params, exp_avg, exp_avg_sq, stats) of the pure-torch reference (on `device`).
    Exact, except means3D / log_scales of the rows from n_exact on (split children: rtol 2e-6, atol 1e-7)."""
    P, opt, var = got
    wp, wm, wv, ws = want
    n = wp["means3D"].shape[0]
    for k in KEYS:
        a, b = P[k].detach(), wp[k]
        assert a.shape == b.shape and isinstance(P[k], torch.nn.Parameter) and P[k].requires_grad, k
        head = n if n_exact is None or k not in ("means3D", "log_scales") else n_exact
        assert torch.equal(a[:head], b[:head]), k
        if head < n:
            np.testing.assert_allclose(a[head:].cpu().numpy(), b[head:].cpu().numpy(), rtol=2e-6, atol=1e-7, err_msg=k + " of the split children")
        st = opt.state[P[k]]
        assert torch.equal(st["exp_avg"], wm[k]) and torch.equal(st["exp_avg_sq"], wv[k]) and int(st["step"]) == 1, k + " moments"
    from tests import reference_pattern as RP
    for k in RP.STATS:
        assert torch.equal(var[k], ws[k]), k


def check_remove_points(device, iso, N=SURGERY_N):
    from activesplat_amd import optim as O
    from tests import reference_pattern as RP
    cpu = surgery_map(N, iso, seed=21)
    gone = compact_mask(N, "random37", device, seed=5)
    P, opt, var = _on_device(device, *cpu)
    want = RP.remove_points_torch(gone, *[{k: v.to(device) for k, v in d.items()} for d in cpu])
    P, var = O.remove_points(gone, P, var, opt)
    assert 0 < want[0]["means3D"].shape[0] < N
    _same_event(device, (P, opt, var), want)


def check_prune(device, iso, N=SURGERY_N):
    from activesplat_amd import optim as O
    from tests import reference_pattern as RP
    cpu = surgery_map(N, iso, seed=22)
    P, opt, var = _on_device(device, *cpu)
    *want, fired = RP.prune_torch(*[{k: v.to(device) for k, v in d.items()} for d in cpu], SCENE_RADIUS, OPACITY_THRESH, True)
    pdict = dict(start_after=0, remove_big_after=0, stop_after=100, prune_every=5, removal_opacity_threshold=OPACITY_THRESH,
                 final_removal_opacity_threshold=OPACITY_THRESH, reset_opacities=False, reset_opacities_every=500)
    P, var = O.prune_gaussians(P, var, opt, 5, pdict)
    print("prune", "iso" if iso else "aniso", fired, "rows", N, "->", want[0]["means3D"].shape[0])
    assert all(v > 0 for v in fired.values()), fired
    _same_event(device, (P, opt, var), want)


def check_densify(device, iso, N=SURGERY_N):
    from activesplat_amd import optim as O
    from tests import reference_pattern as RP
    cpu = surgery_map(N, iso, seed=23)
    params, _, _, stats = cpu
    score = stats["means2D_gradient_accum"] / stats["denom"]
    score[score.isnan()] = 0.0
    n_all = int(((score >= GRAD_THRESH) & (torch.exp(params["log_scales"]).max(dim=1).values > 0.01 * SCENE_RADIUS)).sum())
    samples = (torch.randn(N_INTO * n_all, 3, generator=torch.Generator().manual_seed(24)) * 0.02).to(device)
    P, opt, var = _on_device(device, *cpu)
    *want, fired = RP.densify_torch(*[{k: v.to(device) for k, v in d.items()} for d in cpu], SCENE_RADIUS, GRAD_THRESH, N_INTO, OPACITY_THRESH,
                                    True, samples)
    ddict = dict(start_after=0, remove_big_after=0, stop_after=100, densify_every=10, grad_thresh=GRAD_THRESH, num_to_split_into=N_INTO,
                 removal_opacity_threshold=OPACITY_THRESH, final_removal_opacity_threshold=OPACITY_THRESH, reset_opacities=False,
                 reset_opacities_every=3000)
    P, var = O.densify(P, var, opt, 10, ddict, samples=samples, accumulate=False)
    print("densify", "iso" if iso else "aniso", fired, "rows", N, "->", want[0]["means3D"].shape[0])
    n_head = fired.pop("rows_before_children")
    assert all(v > 0 for v in fired.values()), fired              # clone, split, 0 / 0 scores, opacity cull, too-big cull of originals and of children
    assert 0 < n_head < want[0]["means3D"].shape[0]
    _same_event(device, (P, opt, var), want, n_exact=n_head)


# =====================================================================================================================================
# D. gs_activate_forward / gs_activate_backward (mapping.fused_rendervar)
# =====================================================================================================================================
ACTIVATE_P = [1, 255, 256, 257, 5000]


def activate_inputs(P, iso, seed=0):
    """float32 CPU parameters over the working range: log-scales in [-11, 3], logits in [-20, 20] plus rows at +-100, quaternion norms spread
    over e^+-9, one all-zero quaternion (P > 3: rows 0, 1, 2 hold the special values)."""
    g = torch.Generator().manual_seed(31 * seed + P + (7 if iso else 0))
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True) * torch.exp(torch.rand(P, 1, generator=g) * 18 - 9)
    logit = torch.rand(P, 1, generator=g) * 40 - 20
    if P > 3:
        q[0] = 0.0
        logit[1], logit[2] = 100.0, -100.0
    return dict(means3D=torch.randn(P, 3, generator=g) * 3, rgb_colors=torch.rand(P, 3, generator=g), unnorm_rotations=q, logit_opacities=logit,
                log_scales=torch.rand(P, 1 if iso else 3, generator=g) * 14 - 11,
                cam_unnorm_rots=torch.randn(1, 4, 2, generator=g) * 1.7, cam_trans=torch.randn(1, 3, 2, generator=g))


def _rotation64(q):
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(3, 3)


def _quat_mult64(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def activate_reference64(p, t, iso):
    """transform_to_frame + transformed_params2rendervar (slam_helpers.py:252-304, :124-139) in float64 on float64 leaves `p`."""
    qc = F.normalize(p["cam_unnorm_rots"][..., t].detach()).reshape(4)
    R, tr = _rotation64(qc), p["cam_trans"][..., t].detach().reshape(3)
    rot = p["unnorm_rotations"] if iso else _quat_mult64(qc[None], F.normalize(p["unnorm_rotations"]))
    ls = p["log_scales"]
    return dict(means3D=p["means3D"] @ R.T + tr, rotations=F.normalize(rot), opacities=torch.sigmoid(p["logit_opacities"]),
                scales=torch.exp(ls.repeat(1, 3) if iso else ls)), R, tr


OUT = ("means3D", "rotations", "opacities", "scales")
GRAD = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales")


def check_activate(device, P, iso):
    from activesplat_amd import mapping as M
    raw = activate_inputs(P, iso)
    g = torch.Generator().manual_seed(P + 99)
    up = dict(means3D=torch.randn(P, 3, generator=g), rotations=torch.randn(P, 4, generator=g), opacities=torch.randn(P, 1, generator=g),
              scales=torch.randn(P, 3, generator=g))
    t = 1

    def leaves(dtype, dev):
        return {k: v.clone().to(dtype).to(dev).requires_grad_(k in GRAD) for k, v in raw.items()}

    def run(outs, p, dtype, dev):
        sum((outs[k] * up[k].to(dtype).to(dev)).sum() for k in OUT).backward()
        return {k: outs[k].detach().cpu().double() for k in OUT}, {k: p[k].grad.cpu().double() for k in GRAD}
    p64 = leaves(torch.float64, "cpu")
    o64, R, tr = activate_reference64(p64, t, iso)
    o64, g64 = run(o64, p64, torch.float64, "cpu")
    pm = leaves(torch.float32, "cpu")                                    # the fp32 mirror: the torch chain of mapping.py on CPU
    _, gm = run(M.transformed_params2rendervar(pm, M.transform_to_frame(pm, t, gaussians_grad=True, camera_grad=False)), pm, torch.float32, "cpu")
    pk = leaves(torch.float32, device)
    ok, gk = run(M.fused_rendervar(pk, t), pk, torch.float32, device)
    assert all(torch.isfinite(v).all() for v in list(ok.values()) + list(gk.values()))        # (the zero quaternion included)
    # ---- forward ----
    x = (raw["log_scales"].repeat(1, 3) if iso else raw["log_scales"]).double()
    # __expf = exp2(x log2 e): the fp32 product carries |x| 2^-24 relative error into the result; + the exp2 instruction's own error (1 ulp)
    # and the final rounding: (|x| + 2) 2^-24, doubled
    scale_err = float((((ok["scales"] - o64["scales"]).abs() / o64["scales"]) / ((x.abs() + 4) * 2 * U)).max())
    op_err = float((ok["opacities"] - o64["opacities"]).abs().max()) / (4 * U)
    pts = raw["means3D"].double()
    mean_err = float(((ok["means3D"] - o64["means3D"]).abs().max(dim=1).values / (8 * U * (pts.norm(dim=1) + tr.norm()))).max())   # |R| = 1
    rot_err = float((ok["rotations"] - o64["rotations"]).abs().max()) / (8 * U)
    # ---- backward, compared per row: a row's error is max |g - g64| over its components / the row's scale.  The scale is the row's largest
    # |g64|, or, where that is more, the size of the terms the row is formed from: |g_rot| / |q| for the quaternion (where the upstream gradient
    # is nearly parallel to q the projection g - u (u . g) cancels: any fp32 evaluation is then off by roundoff x |g| / |q|, however small the row
    # comes out), s (|g_0| + |g_1| + |g_2|) for an isotropic log-scale, |g_mean| for the mean.  The mirror's figures are its worst row and its mean
    # over the rows; the kernel may have 2 x each (floors: 1e-6 for a row, 8 x 2^-24 for the mean -- the forward's allowance for a normalisation
    # chain).  A row-by-row ratio of the two errors is no test: on a cancelling row each fp32 result is off by its own rounding -- of 5000 rows one
    # had the kernel at 2.7 x the mirror on that row while the two distributions agree (medians 5.9e-8 / 6.2e-8 of the row's largest |g64|, worst
    # rows 1.7e-6 / 2.1e-6).  The mean keeps one bad row of the mirror from excusing a kernel that is worse everywhere.
    qn = raw["unnorm_rotations"].double().norm(dim=1).clamp_min(1e-12)
    terms = dict(means3D=up["means3D"].double().norm(dim=1), unnorm_rotations=up["rotations"].double().norm(dim=1) / qn,
                 log_scales=(up["scales"].double().abs() * o64["scales"]).sum(dim=1) if iso else torch.zeros(P, dtype=torch.float64))
    worst, stats = {}, {}
    for k in ("means3D", "unnorm_rotations", "log_scales"):
        scale = torch.maximum(g64[k].abs().max(dim=1).values, terms[k]).clamp_min(1e-300)
        ek, em = (gk[k] - g64[k]).abs().max(dim=1).values / scale, (gm[k] - g64[k]).abs().max(dim=1).values / scale
        stats[k] = (float(ek.max()), float(em.max()), float(ek.mean()), float(em.mean()))
        worst[k] = max(float(ek.max()) / max(2 * float(em.max()), 1e-6), float(ek.mean()) / max(2 * float(em.mean()), 8 * U))
    # the fp32 form o (1 - o) cancels near |logit| > 17 for kernel and reference alike: absolute, 2^-23 |g_op|
    logit_err = float(((gk["logit_opacities"] - g64["logit_opacities"]).abs() / (2 * U * up["opacities"].double().abs())).max())
    _say("activate", P=P, iso=int(iso), scales=scale_err, opacities=op_err, means3D=mean_err, rotations=rot_err,
         d_means3D=worst["means3D"], d_rotations=worst["unnorm_rotations"], d_log_scales=worst["log_scales"], d_logit=logit_err,
         **{f"{k}_{n}": v for k in stats for n, v in zip(("kernel_worst", "mirror_worst", "kernel_mean", "mirror_mean"), stats[k])})
    assert scale_err <= 1 and op_err <= 1 and mean_err <= 1 and rot_err <= 1, "forward (fractions of the bounds)"
    assert all(v <= 1 for v in worst.values()) and logit_err <= 1, "backward (fractions of the bounds)"
