"""The map-quality evaluation at its own shapes (GPU box): one frame at 256 x 256 (the reference's sensor) and at 640 x 480.
  (a) gs_eval_frame alone (PSNR + depth errors + SSIM + MS-SSIM, images masked by the valid depth: what `eval` asks), and its sums pass alone;
  (b) one fused render of a synthetic map + gs_eval_frame (evaluate.render_frame + MapEvaluator.add_frame: a frame of evaluate_map);
  (c) the same metrics as torch operations on the same device (fp32: masks, calc_psnr, the depth sums, calc_ssim's five depthwise
      convolutions, the 5-scale MS-SSIM with separable valid convolutions and avg_pool2d), no host read inside the timed call;
  (d) the reference's route for MS-SSIM (eval_helpers.py:483): both images copied to the host and the 5-scale evaluation there, 16 threads.
Every figure: WARM (>= 20) untimed calls, then REPEATS (>= 100) calls each between its own pair of events (host clock for (d)); median and
p10 / p90 in milliseconds.  PROFILE=1: only 50 calls of (a) per size, for `rocprofv3 --kernel-trace --stats -- python scripts/eval_time.py`
(the per-launch split).  Environment: REPEATS (100), WARM (20), GAUSSIANS (100 000).  Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import evaluate as E, synthetic as syn  # noqa: E402
from activesplat_amd.camera import setup_camera  # noqa: E402
from tests import eval_cases as ec  # noqa: E402

dev = torch.device("cuda")
REPEATS = max(100, int(os.environ.get("REPEATS", 100)))
WARM = max(20, int(os.environ.get("WARM", 20)))
N = int(os.environ.get("GAUSSIANS", 100_000))
SIZES = ((256, 256), (480, 640))          # (H, W)
THRES = ec.SIL_THRES


def stats(ms):
    ms = sorted(ms)
    return dict(median=round(statistics.median(ms), 4), p10=round(ms[len(ms) // 10], 4), p90=round(ms[(9 * len(ms)) // 10], 4))


def device_ms(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return stats(out)


def host_ms(fn, repeats):
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


W1 = ec.window32()


def torch_metrics(c, w2d, wh, wv):
    """the reference's arithmetic as torch launches on the device, fp32 -> a [6] tensor (no host read)"""
    valid = c["gt_depth"] > 0
    x, y = c["im"] * valid, c["gt"] * valid
    mse = ((x - y) ** 2).view(3, -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    d = torch.abs(c["depth"] - c["gt_depth"]) * valid
    l1 = d.sum() / valid.sum()
    rmse = (torch.sqrt((c["depth"] - c["gt_depth"]) ** 2) * valid).sum() / valid.sum()
    ssim, _ = ec._moments(x[None], y[None], lambda v: F.conv2d(v, w2d, padding=5, groups=3))
    conv = lambda v: F.conv2d(F.conv2d(v, wh, groups=3), wv, groups=3)  # noqa: E731
    a, b, terms = x[None], y[None], []
    for level in range(5):
        s, cs = ec._moments(a, b, conv)
        terms.append((cs if level < 4 else s).mean((0, 2, 3)))
        if level < 4:
            pad = [a.shape[2] % 2, a.shape[3] % 2]
            a, b = F.avg_pool2d(a, 2, padding=pad), F.avg_pool2d(b, 2, padding=pad)
    wgt = torch.tensor(ec.MS_WEIGHTS, device=x.device)[:, None]
    ms = (torch.stack(terms).clamp(min=0) ** wgt).prod(0).mean()
    return torch.stack([psnr, rmse, l1, ssim.mean(), ms, valid.sum().float()])


def host_ms_ssim(c):
    """both images to the host, the 5-scale evaluation there (the published definition, fp32)"""
    valid = c["gt_depth"] > 0
    x, y = (c["im"] * valid).cpu(), (c["gt"] * valid).cpu()
    return ec.ms_value(ec.ms_terms(x, y))


res = {"repeats": REPEATS, "warm": WARM, "gaussians": N, "device": torch.cuda.get_device_name(0), "sizes": {}}
for H, W in SIZES:
    c = {k: v.to(dev).contiguous() for k, v in ec.textured(H, W, True).items()}
    ev = E.MapEvaluator(W, H, 4, device=dev)

    def eval_all():
        ev.frames = 0
        ev.add_frame(c["im"], c["depth"], c["sil"], c["gt"], c["gt_depth"], THRES)

    def eval_sums():
        ev.frames = 0
        ev.add_frame(c["im"], c["depth"], c["sil"], c["gt"], c["gt_depth"], THRES, ssim=False, ms_ssim=False)

    def eval_ssim_only():
        ev.frames = 0
        ev.add_frame(c["im"], c["depth"], c["sil"], c["gt"], c["gt_depth"], THRES, ms_ssim=False)

    if os.environ.get("PROFILE"):
        for _ in range(50):
            eval_all()
        torch.cuda.synchronize()
        continue
    r = {"gs_eval_frame_all": device_ms(eval_all), "gs_eval_frame_psnr_depth_ssim": device_ms(eval_ssim_only), "gs_eval_frame_sums_only": device_ms(eval_sums)}
    eval_all()
    row = ev.rows()[0]
    # (b) render + evaluation
    params = {k: v.to(dev) for k, v in syn.make_params(N, W, H, seed=3).items()}
    params["cam_unnorm_rots"] = torch.tensor([1.0, 0, 0, 0], device=dev).reshape(1, 4, 1).repeat(1, 1, 2).contiguous()
    params["cam_trans"] = torch.zeros(1, 3, 2, device=dev)
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=dev)
    pose7 = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]

    def render_and_eval():
        ev.frames = 0
        im, depth, sil = E.render_frame(params, cam, 0, pose7)
        ev.add_frame(im, depth, sil, c["gt"], c["gt_depth"], THRES)

    def render_only():
        E.render_frame(params, cam, 0, pose7)

    r["render_plus_gs_eval_frame"] = device_ms(render_and_eval)
    r["render_alone"] = device_ms(render_only)
    # (c) torch operations on the device
    w2d = (W1[:, None] @ W1[None, :]).expand(3, 1, 11, 11).contiguous().to(dev)
    wh, wv = W1.reshape(1, 1, 1, 11).expand(3, 1, 1, 11).contiguous().to(dev), W1.reshape(1, 1, 11, 1).expand(3, 1, 11, 1).contiguous().to(dev)
    r["torch_ops_same_device"] = device_ms(lambda: torch_metrics(c, w2d, wh, wv))
    tm = torch_metrics(c, w2d, wh, wv).cpu().numpy()
    # (d) the reference's MS-SSIM route
    torch.set_num_threads(16)
    r["host_ms_ssim_16_threads"] = host_ms(lambda: host_ms_ssim(c), 20)
    r["row"] = [float(f"{v:.10g}") for v in row]
    r["torch_ops_row"] = [float(f"{v:.10g}") for v in tm]
    r["fused_over_torch_ops"] = round(r["gs_eval_frame_all"]["median"] / r["torch_ops_same_device"]["median"], 3)
    res["sizes"][f"{H}x{W}"] = r
print(json.dumps(res))
