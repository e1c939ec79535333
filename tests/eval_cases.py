"""Cases, references and tolerances of the map-quality evaluation (activesplat_amd/evaluate.py; gs_eval_frame), shared by the emulated run
(tests/test_eval.py) and the MI355X run (tests/test_gpu_eval.py).  Nothing here reads the reference or scipy.

The reference for every column is an fp64 torch restatement of the reference's arithmetic (report_progress / eval of eval_helpers.py, calc_ssim of
slam_external.py, and the published MS-SSIM definition that include/gsplat_hip.h states), evaluated on the fp32 inputs.

Tolerances
  sums columns   every term of a sum is formed in fp32 with two roundings (the difference, then the square or the product with the mask) before
                 the fp64 accumulation, doubled: SUM_RTOL = 4 * 2^-23 relative on each sum.  The PSNR of a sum within that is within
                 (10 / ln 10) * SUM_RTOL dB; depth_l1 = sum / count and depth_rmse_l2^2 = sum / count carry their sum's bound (the count is
                 exact); valid_pixels is exact
  SSIM, MS-SSIM  measured: E32 = |fp32 torch evaluation of the same restatement - fp64| per case; the kernel must be within
                 max(E32 of the case, 16 * the worst E32 over the textured cases of that quantity) -- the factor covers another summation tree and
                 the power / product finish
  golden         the golden holds the reference's fp32 torch results; the bound is the measured distance golden <-> fp64 restatement plus the
                 kernel's bound above
"""
import functools
import os
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

from activesplat_amd import evaluate as E
from activesplat_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval.npz")
SUM_RTOL = 4 * 2.0 ** -23
PSNR_ATOL = 10.0 / np.log(10.0) * SUM_RTOL
SMALL = ((1, 1), (5, 17), (40, 56), (33, 47))                      # (H, W): one pixel, one partial tile, the golden's size, partial tiles on both axes
MS_SIZES = ((161, 163), (164, 176), (177, 201), (256, 256))       # the smallest legal size (odd at every level, 1 x 1 output at level 4), even then odd, ..., the sensor
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SIL_THRES = 0.98
FLAG_COMBOS = ((False, False), (True, False), (False, True), (True, True))       # (sil_mask, image_valid_mask)
NAN = float("nan")


def t(a, device):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device).contiguous()


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def textured(H, W, invalid=False):
    """gt = 0.5 + 0.4 sin(x / 9 + c) cos(y / 7 - c) + 0.1 uniform, clamped; im = gt + 0.05 normal; seeded by the size.  invalid: 10 % of the
    depth pixels are 0.  The silhouette straddles the threshold and sits exactly ON it at a grid of pixels."""
    g = torch.Generator().manual_seed(1000 * H + W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = torch.stack([0.5 + 0.4 * torch.sin(xs / 9 + c) * torch.cos(ys / 7 - c) for c in range(3)])
    gt = (gt + 0.1 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
    im = gt + 0.05 * torch.randn(3, H, W, generator=g)
    gt_depth = 1.0 + 2.0 * torch.rand(H, W, generator=g)
    depth = gt_depth + 0.05 * torch.randn(H, W, generator=g)
    sil = 0.9 + 0.1 * torch.rand(H, W, generator=g)
    sil[::3, ::4] = SIL_THRES
    drop = torch.rand(H, W, generator=g) < 0.1
    if invalid:
        gt_depth = torch.where(drop, torch.zeros(()), gt_depth)
    return dict(im=im.contiguous(), depth=depth.contiguous(), sil=sil.contiguous(), gt=gt.contiguous(), gt_depth=gt_depth.contiguous())


@functools.lru_cache(maxsize=None)
def smooth(H, W):
    """the cancellation case: a slow ramp and the same ramp plus 0.002 -- E[x^2] - mu^2 of the raw values cancels against C2 = 9e-4"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = torch.stack([0.3 + 0.4 * xs / max(W, 2) + 0.1 * c * ys / max(H, 2) for c in range(3)])
    c = dict(textured(H, W))
    c.update(gt=gt.contiguous(), im=(gt + 0.002).contiguous())
    return c


def inverted(H, W):
    """the clamp case: im = 1 - gt on the textured target, every cs term strongly negative"""
    c = dict(textured(H, W))
    c["im"] = (1.0 - c["gt"]).contiguous()
    return c


def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def golden_case(g, f):
    ds = torch.from_numpy(g["depth_sil"][f])
    return dict(im=torch.from_numpy(g["im"][f]).contiguous(), depth=ds[0].contiguous(), sil=ds[1].contiguous(),
                gt=torch.from_numpy(g["gt_color"][f]).contiguous(), gt_depth=torch.from_numpy(g["gt_depth"][f][0]).contiguous())


# ---- the restatement -------------------------------------------------------------------------------------------------
def masked_pair(c, sil_mask, image_valid_mask, dtype=torch.float64):
    m = torch.ones_like(c["gt_depth"], dtype=dtype)
    if image_valid_mask:
        m = m * (c["gt_depth"] > 0).to(dtype)
    if sil_mask:
        m = m * (c["sil"] > np.float32(SIL_THRES)).to(dtype)
    return c["im"].to(dtype) * m, c["gt"].to(dtype) * m


def restate_sums(c, sil_mask, image_valid_mask):
    """-> dict(mse [3], l1_sum, l2_sum, count, psnr, depth_l1, depth_rmse_l2): eval_helpers.py:228-245 / :476-506 in fp64"""
    x, y = masked_pair(c, sil_mask, image_valid_mask)
    mse = ((x - y) ** 2).reshape(3, -1).mean(1)
    valid = (c["gt_depth"] > 0).double()
    d = c["depth"].double() - c["gt_depth"].double()
    if sil_mask:
        d = d * (c["sil"] > np.float32(SIL_THRES)).double()
    l1, l2, n = float((d.abs() * valid).sum()), float((d * d * valid).sum()), float(valid.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = float(np.mean(20.0 * np.log10(1.0 / np.sqrt(mse.numpy()))))
        return dict(mse=mse.numpy(), l1_sum=l1, l2_sum=l2, count=n, psnr=psnr, depth_l1=float(np.float64(l1) / np.float64(n)),
                    depth_rmse_l2=float(np.sqrt(np.float64(l2) / np.float64(n))))


def window32():
    """the reference's 1-D window: fp32 VALUES, normalised in fp32 (slam_external.py:54-56; the MS-SSIM package builds its own the same way, one
    ulp apart in one tap).  Its sum is 1 - 3.1e-8, which moves an SSIM by 1e-6 against the exact Gaussian: the window is part of the definition,
    and the kernels carry these eleven floats"""
    g = torch.tensor([np.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    return g / g.sum()


def _moments(x, y, conv):
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    cs = (2 * s12 + c2) / (s11 + s22 + c2)
    return (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs, cs


def ssim_same(x, y, rounded_window=False):
    """calc_ssim (slam_external.py:66-97) in the dtype of x: the 2-D window, zero padding 5 -> the mean of the map (a float).  The 2-D window is the
    exact outer product of the eleven fp32 taps -- what a separable pass applies.  rounded_window: the outer product rounded to fp32, as the
    reference (and mapping.calc_ssim) forms it; its sum differs by some 1e-8, which moves an SSIM of 0.8 by up to 1e-6 (test_eval.py prints it,
    and the golden's measured distance contains it)"""
    w1 = window32()
    w = (w1[:, None] @ w1[None, :]) if rounded_window else (w1.double()[:, None] @ w1.double()[None, :])
    w = w.to(x.dtype).expand(3, 1, 11, 11).contiguous()
    ssim, _ = _moments(x[None], y[None], lambda v: F.conv2d(v, w, padding=5, groups=3))
    return float(ssim.double().mean())


def ms_terms(x, y):
    """the 15 per-level, per-channel spatial means of the published MS-SSIM in the dtype of x -> [5, 3] (rows 0-3: cs, row 4: ssim), before the
    clamp: valid separable 11-tap window; between levels avg_pool2d(kernel 2, padding = size % 2)"""
    w1 = window32().to(x.dtype)
    wh, wv = w1.reshape(1, 1, 1, 11).expand(3, 1, 1, 11).contiguous(), w1.reshape(1, 1, 11, 1).expand(3, 1, 11, 1).contiguous()
    conv = lambda v: F.conv2d(F.conv2d(v, wh, groups=3), wv, groups=3)  # noqa: E731
    x, y, rows = x[None], y[None], []
    for level in range(5):
        ssim, cs = _moments(x, y, conv)
        rows.append((cs if level < 4 else ssim).double().mean((0, 2, 3)))
        if level < 4:
            pad = [x.shape[2] % 2, x.shape[3] % 2]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    return torch.stack(rows)


def ms_value(terms):
    wgt = torch.tensor(MS_WEIGHTS, dtype=torch.float64)[:, None]
    return float((terms.double().clamp(min=0) ** wgt).prod(0).mean())


def restate_row(c, sil_mask, image_valid_mask, ssim=True, ms_ssim=True):
    s = restate_sums(c, sil_mask, image_valid_mask)
    x, y = masked_pair(c, sil_mask, image_valid_mask)
    return np.array([s["psnr"], s["depth_l1"], s["depth_l1"], ssim_same(x, y) if ssim else NAN, ms_value(ms_terms(x, y)) if ms_ssim else NAN,
                     s["count"], s["depth_rmse_l2"], 0.0])


def e32(c, sil_mask, image_valid_mask, quantity):
    """|fp32 torch evaluation - fp64| of the restatement -> (E32, the fp64 value)"""
    x, y = masked_pair(c, sil_mask, image_valid_mask)
    x32, y32 = masked_pair(c, sil_mask, image_valid_mask, torch.float32)
    f = ssim_same if quantity == "ssim" else (lambda a, b: ms_value(ms_terms(a, b)))
    want = f(x, y)
    return abs(f(x32, y32) - want), want


def ssim_cases(sizes):
    """(name, case, sil_mask, image_valid_mask, textured?) per size: textured, textured with 10 % invalid depth (masked images), smooth"""
    out = []
    for H, W in sizes:
        out += [(f"textured {H}x{W}", textured(H, W), False, False, True), (f"textured {H}x{W}, 10 % invalid", textured(H, W, True), False, True, True),
                (f"smooth {H}x{W}", smooth(H, W), False, False, False)]
    return out


@functools.lru_cache(maxsize=None)
def worst_textured_e32(quantity):
    sizes = SMALL if quantity == "ssim" else MS_SIZES
    return max(e32(c, sm, ivm, quantity)[0] for _, c, sm, ivm, tex in ssim_cases(sizes) if tex)


# ---- running the product ---------------------------------------------------------------------------------------------
def metrics(c, device, **kw):
    row = E.frame_metrics(t(c["im"], device), t(c["depth"], device), t(c["sil"], device), t(c["gt"], device), t(c["gt_depth"], device), SIL_THRES, **kw)
    assert row.dtype == torch.float64 and tuple(row.shape) == (8,)
    return row.cpu().numpy()


def compare_sums(got, c, sil_mask, image_valid_mask, where, extra=(0.0, 0.0, 0.0)):
    """psnr, depth_rmse, depth_l1, valid_pixels, depth_rmse_l2 of a row against the fp64 restatement; extra: added bounds (psnr dB, l1, l2)"""
    s = restate_sums(c, sil_mask, image_valid_mask)
    dpsnr = 0.0 if got[0] == s["psnr"] else abs(got[0] - s["psnr"])
    print(f"[eval sums] {where}: psnr {got[0]:.9f} (want {s['psnr']:.9f}, diff {dpsnr:.2e}, bound {PSNR_ATOL + extra[0]:.2e}) "
          f"l1 {got[2]:.9e} (rel {abs(got[2] - s['depth_l1']) / max(s['depth_l1'], 1e-300):.2e}) l2 {got[6]:.9e} valid {got[5]}")
    assert got[5] == s["count"] and got[7] == 0.0, where
    if np.isinf(s["psnr"]):
        assert got[0] == s["psnr"], where
    else:
        assert abs(got[0] - s["psnr"]) <= PSNR_ATOL + extra[0], (where, got[0], s["psnr"])
    if s["count"] == 0:
        assert np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(got[6]), where
        return
    assert got[1] == got[2], where                                      # the reference's "RMSE" IS the L1 error
    assert abs(got[2] - s["depth_l1"]) <= SUM_RTOL * s["depth_l1"] + extra[1], (where, got[2], s["depth_l1"])
    assert abs(got[6] ** 2 - s["depth_rmse_l2"] ** 2) <= SUM_RTOL * s["depth_rmse_l2"] ** 2 + extra[2], (where, got[6], s["depth_rmse_l2"])


def check_sums_and_flags(device, H, W):
    """sums columns in each of the four mask combinations, with and without invalid depth; columns switched off are NaN"""
    for invalid in (False, True):
        c = textured(H, W, invalid)
        for sil_mask, ivm in FLAG_COMBOS:
            got = metrics(c, device, sil_mask=sil_mask, image_valid_mask=ivm, ssim=False, ms_ssim=False)
            assert np.isnan(got[3]) and np.isnan(got[4])
            compare_sums(got, c, sil_mask, ivm, f"{H}x{W} invalid={invalid} sil_mask={sil_mask} image_valid_mask={ivm}")
            if H * W > 1 and invalid:                                    # the flags do something on this case
                plain = restate_sums(c, False, False)
                assert sil_mask is False or restate_sums(c, True, ivm)["l1_sum"] < plain["l1_sum"]
                assert ivm is False or restate_sums(c, sil_mask, True)["mse"][0] < restate_sums(c, sil_mask, False)["mse"][0]


def compare_ssim(got, c, sil_mask, ivm, quantity, where):
    err32, want = e32(c, sil_mask, ivm, quantity)
    bound = max(err32, 16 * worst_textured_e32(quantity))
    print(f"[eval {quantity}] {where}: got {got:.12f} want {want:.12f} |diff| {abs(got - want):.3e} E32 {err32:.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound, (where, got, want, bound)


def check_ssim_same(device, H, W):
    for name, c, sil_mask, ivm, _ in ssim_cases(((H, W),)):
        got = metrics(c, device, sil_mask=sil_mask, image_valid_mask=ivm, ssim=True, ms_ssim=False)
        assert np.isnan(got[4])
        compare_ssim(got[3], c, sil_mask, ivm, "ssim", name)
    # all four mask combinations on the case with invalid depth
    c = textured(H, W, True)
    for sil_mask, ivm in FLAG_COMBOS:
        got = metrics(c, device, sil_mask=sil_mask, image_valid_mask=ivm, ssim=True, ms_ssim=False)
        compare_ssim(got[3], c, sil_mask, ivm, "ssim", f"textured {H}x{W} sil_mask={sil_mask} image_valid_mask={ivm}")


def check_ms_ssim(device, H, W):
    for name, c, sil_mask, ivm, _ in ssim_cases(((H, W),)):
        got = metrics(c, device, sil_mask=sil_mask, image_valid_mask=ivm, ssim=True, ms_ssim=True)
        compare_ssim(got[4], c, sil_mask, ivm, "ms_ssim", name)
        compare_ssim(got[3], c, sil_mask, ivm, "ssim", name)
        compare_sums(got, c, sil_mask, ivm, name)
    c = textured(H, W, True)
    got = metrics(c, device, sil_mask=True, image_valid_mask=True, ssim=False, ms_ssim=True)
    assert np.isnan(got[3])
    compare_ssim(got[4], c, True, True, "ms_ssim", f"textured {H}x{W}, both masks")


def condition(H, W):
    """-> the smallest |term| over the 15 terms of every MS-SSIM case of this size (none may sit near the clamp at 0)"""
    worst = np.inf
    for name, c, sil_mask, ivm, _ in ssim_cases(((H, W),)) + [(f"textured {H}x{W}, both masks", textured(H, W, True), True, True, True)]:
        terms = ms_terms(*masked_pair(c, sil_mask, ivm))
        worst = min(worst, float(terms.abs().min()))
    return worst


def assert_clamp_case(terms):
    """the twelve cs terms of the inverted pair in the restatement: <= -0.9 at the two coarse levels (-0.96 and -0.97 at 161 x 163), <= -0.7 at
    every level (level 0: -0.74, where the 11-tap window sees little of the slow texture; level 1: -0.90) -- none anywhere near the clamp at 0"""
    assert float(terms[2:4].max()) <= -0.9 and float(terms[:4].max()) <= -0.7 and float(terms[4].max()) < 0.0, terms


def check_clamp(device, H=161, W=163):
    """im = 1 - gt: every cs term of the restatement is far below the clamp, the product holds factors max(0, .)^w = 0: exactly 0"""
    c = inverted(H, W)
    terms = ms_terms(*masked_pair(c, False, False))
    assert_clamp_case(terms)
    got = metrics(c, device, image_valid_mask=False)
    print(f"[eval clamp] largest cs term {float(terms[:4].max()):.3f}, ms_ssim {got[4]!r}, ssim {got[3]:.6f}")
    assert got[4] == 0.0 and got[3] < 0.0


def check_identities(device):
    """im == gt: SSIM and MS-SSIM exactly 1, PSNR +inf; all-zero gt_depth: NaN depth columns, 0 valid pixels; silhouette == sil_thres does not pass"""
    c = dict(textured(161, 163))
    c["im"] = c["gt"].clone()
    got = metrics(c, device, image_valid_mask=False)
    assert got[3] == 1.0 and got[4] == 1.0 and got[0] == np.inf, got
    for H, W in SMALL:
        c = dict(textured(H, W, True))
        c["im"] = c["gt"].clone()
        got = metrics(c, device, ms_ssim=False)
        assert got[3] == 1.0 and got[0] == np.inf and np.isnan(got[4]), (H, W, got)
        c = dict(textured(H, W))
        c["gt_depth"] = torch.zeros(H, W)
        for ivm in (False, True):
            got = metrics(c, device, image_valid_mask=ivm, ms_ssim=False)
            assert got[5] == 0.0 and np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(got[6]), (H, W, got)
            assert (got[0] == np.inf and got[3] == 1.0) if ivm else np.isfinite(got[0])          # both images masked to zero: identical
        c = dict(textured(H, W))
        c["sil"] = torch.full((H, W), SIL_THRES, dtype=torch.float32)
        got = metrics(c, device, sil_mask=True, image_valid_mask=False, ms_ssim=False)
        assert got[0] == np.inf and got[2] == 0.0 and got[6] == 0.0 and got[3] == 1.0, (H, W, got)                 # nothing passes the strict compare
        c["sil"] = torch.nextafter(c["sil"], torch.ones(()))
        got = metrics(c, device, sil_mask=True, image_valid_mask=False, ms_ssim=False)
        compare_sums(got, textured(H, W), False, False, f"{H}x{W}, silhouette one ulp above the threshold")       # everything passes


def feed(device, ev=None):
    g = golden()
    ev = ev or E.MapEvaluator(56, 40, 12, device=device)
    for f in range(3):
        c = golden_case(g, f)
        for sil_mask, ivm in FLAG_COMBOS:
            ev.add_frame(t(c["im"], device), t(c["depth"], device), t(c["sil"], device), t(c["gt"], device), t(c["gt_depth"], device), SIL_THRES,
                         sil_mask=sil_mask, image_valid_mask=ivm, ms_ssim=False)
    return ev


def check_repeatable(device):
    """two evaluators fed the same frames: bit-identical tables (also with MS-SSIM on)"""
    a, b = feed(device).rows(), feed(device).rows()
    assert a.shape == (12, 8) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    c = textured(177, 201, True)
    r1, r2 = metrics(c, device, sil_mask=True), metrics(c, device, sil_mask=True)
    assert np.isfinite(r1).all() and np.array_equal(r1.view(np.uint64), r2.view(np.uint64))


def golden_distance():
    """how far the golden (the reference's fp32 torch sums) is from the fp64 restatement -> dict of per-quantity maxima; printed"""
    g = golden()
    d = dict(psnr=0.0, l1=0.0, rmse=0.0, ssim=0.0)
    for key, sil_mask, ivm in (("report_progress", False, False), ("eval_sil", True, True), ("eval_plain", False, True)):
        for f in range(3):
            s = restate_sums(golden_case(g, f), sil_mask, ivm)
            d["psnr"] = max(d["psnr"], abs(g[key][f, 0] - s["psnr"]))
            d["rmse"] = max(d["rmse"], abs(g[key][f, 1] - s["depth_l1"]))
            d["l1"] = max(d["l1"], abs(g[key][f, 2] - s["depth_l1"]))
    for f in range(3):
        c = golden_case(g, f)
        d["ssim"] = max(d["ssim"], abs(g["calc_ssim"][f] - ssim_same(*masked_pair(c, False, False))))
    print(f"[eval golden] distance of the golden from the fp64 restatement: {d}")
    return d


def check_golden(device):
    """PSNR / RMSE / L1 in the reference's three modes, calc_ssim and the trajectory error against tests/golden/eval.npz"""
    g, d = golden(), golden_distance()
    assert float(g["sil_thres"]) == SIL_THRES
    for key, sil_mask, ivm in (("report_progress", False, False), ("eval_sil", True, True), ("eval_plain", False, True)):
        for f in range(3):
            c = golden_case(g, f)
            got = metrics(c, device, sil_mask=sil_mask, image_valid_mask=ivm, ssim=True, ms_ssim=False)
            want = g[key][f]
            print(f"[eval golden] {key} frame {f}: got {got[:3]} want {want}")
            assert abs(got[0] - want[0]) <= PSNR_ATOL + d["psnr"], (key, f)
            assert abs(got[1] - want[1]) <= SUM_RTOL * want[1] + d["rmse"] and abs(got[2] - want[2]) <= SUM_RTOL * want[2] + d["l1"], (key, f)
    bound = 16 * worst_textured_e32("ssim")
    for f in range(3):
        c = golden_case(g, f)
        got = metrics(c, device, image_valid_mask=False, ms_ssim=False)[3]
        err32, _ = e32(c, False, False, "ssim")
        print(f"[eval golden] calc_ssim frame {f}: got {got:.9f} want {g['calc_ssim'][f]:.9f}")
        assert abs(got - g["calc_ssim"][f]) <= max(err32, bound) + d["ssim"], f
    check_ate_golden()


def check_ate_golden():
    g = golden()
    gp, ep = g["ate_gt"][:, :3, 3].T.astype(np.float64), g["ate_est"][:, :3, 3].T.astype(np.float64)
    rot, trans, err = E.align(gp, ep)
    assert np.allclose(rot, g["align_rot"], rtol=0, atol=1e-12) and np.allclose(trans, g["align_trans"], rtol=0, atol=1e-12)
    assert np.allclose(err, g["align_error"], rtol=1e-9, atol=1e-14)
    mean, rmse = E.evaluate_ate([torch.from_numpy(m) for m in g["ate_gt"]], list(g["ate_est"]))
    # (the reference's evaluate_ate aligns the float32 arrays in float32: coordinates up to 2.5, a few dozen roundings of 2^-24 relative -> 1e-6)
    assert abs(mean - float(g["ate"])) <= 1e-6 and abs(mean - err.mean()) <= 1e-15 and abs(rmse - np.sqrt(np.mean(g["align_error"] ** 2))) <= 1e-12 and rmse >= mean
    # a known rigid motion without noise is recovered
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(3, 9))
    a = 0.7
    R0 = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rot, trans, err = E.align(pts, R0 @ pts + [[1.0], [2.0], [3.0]])
    assert np.allclose(rot, R0, atol=1e-12) and np.allclose(trans.reshape(3), [1, 2, 3], atol=1e-12) and err.max() < 1e-12


def refused(fn, name, kinds=(ValueError, TypeError)):
    try:
        fn()
    except kinds as e:
        assert name in str(e), (name, str(e))
    else:
        raise AssertionError(f"accepted a bad {name}")


def check_refusals_and_write(device):
    """wrong dtype, device, shape or layout raises and names the argument; MS-SSIM at 160 x 200 and a full table raise; nothing is launched;
    write gives the reference's four files"""
    c = textured(40, 56)
    a = {k: t(v, device) for k, v in c.items()}
    other = "meta"
    call = lambda **kw: E.frame_metrics(**{**dict(im=a["im"], depth=a["depth"], silhouette=a["sil"], gt_im=a["gt"], gt_depth=a["gt_depth"],  # noqa: E731
                                                  sil_thres=SIL_THRES, ms_ssim=False), **kw})
    refused(lambda: call(im=a["im"].double()), "im")
    refused(lambda: call(gt_im=a["gt"].half()), "gt_im")
    refused(lambda: call(depth=a["depth"].t()), "depth")
    refused(lambda: call(depth=a["depth"][:, ::2]), "depth")
    refused(lambda: call(silhouette=torch.empty(40, 56, device=other)), "silhouette")
    refused(lambda: call(gt_depth=a["gt_depth"][:39].contiguous()), "gt_depth")
    refused(lambda: call(gt_im=a["gt"].permute(0, 2, 1)), "gt_im")
    refused(lambda: call(im=a["im"].cpu().numpy()), "im")
    refused(lambda: call(ms_ssim=True), "ms_ssim")
    big = {k: t(v, device) for k, v in textured(160, 200).items()}
    refused(lambda: E.frame_metrics(big["im"], big["depth"], big["sil"], big["gt"], big["gt_depth"], SIL_THRES), "ms_ssim")
    refused(lambda: E.MapEvaluator(56, 40, 0, device=device), "capacity")
    ev = E.MapEvaluator(56, 40, 2, device=device)
    add = lambda e, **kw: e.add_frame(**{**dict(im=a["im"], depth=a["depth"], silhouette=a["sil"], gt_im=a["gt"], gt_depth=a["gt_depth"],  # noqa: E731
                                                sil_thres=SIL_THRES, ms_ssim=False), **kw})
    refused(lambda: add(ev, im=a["im"][:, :39].contiguous()), "im")
    refused(lambda: add(ev, depth=a["depth"].double()), "depth")
    refused(lambda: add(ev, ms_ssim=True), "ms_ssim")
    assert ev.frames == 0 and ev.rows().shape == (0, 8)
    add(ev); add(ev, sil_mask=True)
    before = ev.rows().copy()
    refused(lambda: add(ev), "capacity")
    assert ev.frames == 2 and np.array_equal(ev.rows().view(np.uint64), before.view(np.uint64))
    # the library's own refusals: an error code, a message that names the call, and the row untouched
    import ctypes as C
    from activesplat_amd import _lib
    lib = _lib.get()
    row = torch.full((8,), 7.0, dtype=torch.float64, device=device)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    ptrs = [p(big["im"]), p(big["depth"]), p(big["sil"]), p(big["gt"]), p(big["gt_depth"])]
    assert lib.gs_eval_frame(200, 160, *ptrs, SIL_THRES, E.MS_SSIM, p(row), p(scratch), None) == 1 and b"GS_EVAL_MS_SSIM" in lib.gs_last_error()
    assert lib.gs_eval_frame(0, 160, *ptrs, SIL_THRES, 0, p(row), p(scratch), None) == 1 and b"gs_eval_frame" in lib.gs_last_error()
    assert lib.gs_eval_frame(200, -1, *ptrs, SIL_THRES, 0, p(row), p(scratch), None) == 1
    assert lib.gs_eval_frame(200, 160, *ptrs, SIL_THRES, 16, p(row), p(scratch), None) == 1 and b"flag" in lib.gs_last_error()
    assert lib.gs_eval_frame(200, 160, ptrs[0], None, *ptrs[2:], SIL_THRES, 0, p(row), p(scratch), None) == 1 and b"null pointer" in lib.gs_last_error()
    assert lib.gs_eval_frame(200, 160, *ptrs, SIL_THRES, 0, None, p(scratch), None) == 1
    if device != "cpu":
        torch.cuda.synchronize()
    assert bool((row == 7.0).all())
    lay = _lib.GsEvalLayout()
    assert lib.gs_eval_frame_layout(200, 160, E.SSIM | E.MS_SSIM, C.byref(lay)) == 0 and lay.ms_ssim_defined == 0 and lay.levels == 1
    assert lib.gs_eval_frame_layout(163, 161, E.SSIM | E.MS_SSIM, C.byref(lay)) == 0 and lay.ms_ssim_defined == 1 and lay.levels == 5
    assert list(lay.level_width) == [163, 82, 41, 21, 11] and list(lay.level_height) == [161, 81, 41, 21, 11] and lay.total_bytes % 8 == 0
    assert lib.gs_eval_frame_layout(176, 164, E.MS_SSIM, C.byref(lay)) == 0 and list(lay.level_width) == [176, 88, 44, 22, 11]
    assert lib.gs_eval_frame_layout(0, 4, 0, C.byref(lay)) == 1 and lib.gs_eval_frame_layout(4, 4, 0, None) == 1
    # write: the reference's four files, np.savetxt's format, the MS-SSIM column in ssim.txt
    rows = ev.rows()
    with tempfile.TemporaryDirectory() as d:
        ev.write(os.path.join(d, "eval"))
        assert sorted(os.listdir(os.path.join(d, "eval"))) == ["l1.txt", "psnr.txt", "rmse.txt", "ssim.txt"]
        for name, col in (("psnr.txt", 0), ("rmse.txt", 1), ("l1.txt", 2), ("ssim.txt", 4)):
            assert np.array_equal(np.loadtxt(os.path.join(d, "eval", name)).reshape(-1), rows[:, col], equal_nan=True), name
        assert open(os.path.join(d, "eval", "psnr.txt")).read().split("\n")[0] == "%.18e" % rows[0, 0]
    s = ev.summary()
    assert s["frames"] == 2 and s["avg_psnr"] == float(np.mean(rows[:, 0])) and s["avg_l1"] == float(np.mean(rows[:, 2])) and np.isnan(s["avg_ms_ssim"])
    ev.reset()
    assert ev.frames == 0


# ---- evaluate_map and the mapper hook ----------------------------------------------------------------------------------
def mapper_frames(device, frames=6, W=64, H=64):
    gt = syn.shell_scene(3000, seed=2, W=W, H=H)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    return [dict(fr, gt_w2c=fr["w2c"].astype(np.float32)) for fr in syn.orbit_sequence(gt, frames, W, H, device)]


def run_mapper(device, seq, config, W=64, H=64):
    from activesplat_amd.mapper import SplatMapper
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=len(seq), **config), device=device)
    for fr in seq:
        mp.run(fr)
    return mp


def rows_by_hand(mp, seq, picked, device, **kw):
    out = []
    for i in picked:
        im, depth, sil = E.render_frame(mp.params, mp.cam, i)
        out.append(E.frame_metrics(im.contiguous(), depth.contiguous(), sil.contiguous(), seq[i]["color"].contiguous(), seq[i]["depth"].contiguous(),
                                   mp.cfg["mapping"]["sil_thres"], **kw).cpu().numpy())
    return np.stack(out)


def check_evaluate_map(device):
    """SplatMapper.evaluate over six 64 x 64 frames: the frame selection for eval_every 1 and 2, every row equal to frame_metrics on a separate
    render, a NaN ground-truth pose left out of the trajectory, the four files; and the report_progress hook's table"""
    seq = mapper_frames(device)
    mp = run_mapper(device, seq, dict(map_every=2, mapping_iters=2, report_progress=True, report_global_progress_every=2))
    assert mp.progress_frames == [0, 1, 3, 5] and mp.progress.frames == 4
    prog = mp.progress.rows()
    assert np.isfinite(prog[:, [0, 1, 2, 5, 6]]).all() and np.isnan(prog[:, 3:5]).all() and (prog[:, 0] > 10).all()
    last = rows_by_hand(mp, seq, [5], device, sil_mask=False, image_valid_mask=False, ssim=False, ms_ssim=False)      # nothing moved the map since
    assert np.array_equal(prog[3].view(np.uint64), last[0].view(np.uint64))
    for every, picked in ((1, [0, 1, 2, 3, 4, 5]), (2, [0, 1, 3, 5])):
        res = mp.evaluate(seq, eval_every=every, ms_ssim=False)
        assert res["frames"] == picked and res["rows"].shape == (len(picked), 8)
        want = rows_by_hand(mp, seq, picked, device, sil_mask=False, image_valid_mask=True, ssim=True, ms_ssim=False)
        assert np.array_equal(res["rows"].view(np.uint64), want.view(np.uint64))
        assert np.isfinite(res["rows"][:, [0, 1, 2, 3, 5, 6]]).all() and np.isnan(res["rows"][:, 4]).all()
        assert res["summary"]["frames"] == len(picked) and res["summary"]["avg_psnr"] == float(np.mean(res["rows"][:, 0]))
    print(f"[eval map] rows {res['rows'].tolist()} ate {res['ate']} rmse {res['ate_rmse']}")
    est = [np.eye(4)] + [E._pose_column(mp.params, i).numpy() for i in range(1, 6)]
    gts = [fr["gt_w2c"] for fr in seq]
    assert (res["ate"], res["ate_rmse"]) == E.evaluate_ate(gts, est) and res["ate"] < 1e-6          # the mapper wrote the ground-truth poses
    broken = [dict(fr) for fr in seq]
    broken[2]["gt_w2c"] = np.full((4, 4), np.nan, dtype=np.float32)
    moved = dict(mp.params)
    moved["cam_trans"] = mp.params["cam_trans"].detach().clone()
    moved["cam_trans"][0, :, 2] = 5.0                                      # frame 2's estimate is far off, but its ground truth is NaN: left out
    moved["cam_trans"][0, 0, 4] += 0.25
    r2 = E.evaluate_map(moved, broken, syn.intrinsics(64, 64), np.eye(4), 0.98, 2, True, eval_every=2, ssim=False, ms_ssim=False)
    keep = [0, 1, 3, 4, 5]
    est = [np.eye(4)] + [E._pose_column(moved, i).numpy() for i in keep[1:]]
    assert (r2["ate"], r2["ate_rmse"]) == E.evaluate_ate([gts[i] for i in keep], est) and 0.01 < r2["ate"] < 0.25 < 5.0
    no_gt = [{k: v for k, v in fr.items() if k != "gt_w2c"} for fr in seq]
    assert mp.evaluate(no_gt, eval_every=2, ssim=False, ms_ssim=False)["ate"] is None
    with tempfile.TemporaryDirectory() as d:
        res["evaluator"].write(d)
        assert sorted(os.listdir(d)) == ["l1.txt", "psnr.txt", "rmse.txt", "ssim.txt"]
        assert np.array_equal(np.loadtxt(os.path.join(d, "l1.txt")), res["rows"][:, 2])
    # the silhouette branch of eval: mapping_iters == 0 and no new Gaussians
    r3 = E.evaluate_map(mp.params, seq, syn.intrinsics(64, 64), np.eye(4), 0.98, 0, False, eval_every=2, ms_ssim=False)
    want = rows_by_hand(mp, seq, [0, 1, 3, 5], device, sil_mask=True, image_valid_mask=True, ssim=True, ms_ssim=False)
    assert np.array_equal(r3["rows"].view(np.uint64), want.view(np.uint64)) and not np.array_equal(r3["rows"][:, 2], res["rows"][:, 2])


def check_evaluate_map_ms_ssim(device, W=163, H=161):
    """one 161 x 163 frame with MS-SSIM on, through SplatMapper.evaluate"""
    seq = mapper_frames(device, 1, W, H)
    mp = run_mapper(device, seq, dict(mapping_iters=0), W, H)
    res = mp.evaluate(seq)
    want = rows_by_hand(mp, seq, [0], device)
    print(f"[eval map] 161x163 row {res['rows'][0].tolist()}")
    assert res["rows"].shape == (1, 8) and np.array_equal(res["rows"].view(np.uint64), want.view(np.uint64))
    assert 0.0 < res["rows"][0, 4] <= 1.0 and 0.0 < res["rows"][0, 3] <= 1.0 and res["ate"] == 0.0


def check_mapper_default_is_unchanged(device, deterministic_mapping):
    """report_progress=False (the default) and a mapper without the key build the same map, bit for bit; with the key on, the map is the same too
    (the hook only reads).  Mapping iterations add gradients with float atomics, whose order is fixed only on ONE emulator thread
    (deterministic_mapping); elsewhere the comparison runs with mapping_iters = 0, for the reason completion_cases.check_mapper states."""
    seq = mapper_frames(device, 4)
    base = dict(map_every=2) if deterministic_mapping else dict(mapping_iters=0)
    plain = run_mapper(device, seq, base)
    off = run_mapper(device, seq, dict(base, report_progress=False))
    on = run_mapper(device, seq, dict(base, report_progress=True, report_global_progress_every=2))
    assert plain.progress is None and off.progress is None and plain.cfg["report_progress"] is False and plain.cfg["report_global_progress_every"] == 100
    assert (on.progress_frames == [0, 1, 3]) if deterministic_mapping else (on.progress is None)     # only frames that ran iterations report
    for other in (off, on):
        assert set(plain.params) == set(other.params) and plain.stats["iters"] == other.stats["iters"]
        for k in plain.params:
            assert torch.equal(plain.params[k].detach(), other.params[k].detach()), k
