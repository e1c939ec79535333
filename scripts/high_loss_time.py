"""The per-frame high-loss look target (GPU box): get_high_loss_samples (src/mapper/splatam/__init__.py:184-252) behind its render.
  (1) device time, by events, of visibility.high_loss_grid + visibility.grid_dbscan(grid, 0, 5, 10) on an H x W frame -> 90 x 90, at 256 x 256 and
      512 x 512: five windows of `CALLS` calls each (default 200), milliseconds per call, median and spread.  The images are a synthetic frame: a
      rendered surface behind the measured one in three blobs (about a fifth of the pixels flagged).
  (2) host wall time of SplatMapper.high_loss_step -- the step run() takes on every frame once a map exists -- with high_loss_target off (the
      render and the mask's torch expression) and on (the render, gs_high_loss_grid, gs_grid_dbscan), on one mapper after its first frame,
      alternating, five windows of `STEPS` steps each (default 50): the time until the calls have returned (enqueue: what run() waits for) and
      the time until the device has finished (a synchronise behind the window); with the flag on also with the pose read after every step
      (the one small copy).  Environment: W, H (default 256), N (Gaussians of the synthetic scene the frames come from, default 20000).
  (3) bytes that cross to the host per frame: the H x W mask a caller had to fetch before, the cluster table afterwards.
Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import synthetic as syn, visibility as VIS  # noqa: E402
from activesplat_amd.mapper import SplatMapper  # noqa: E402

dev = torch.device("cuda")
CALLS, STEPS = int(os.environ.get("CALLS", 200)), int(os.environ.get("STEPS", 50))


def med(v):
    return {"median": round(statistics.median(v), 4), "spread": round(max(v) - min(v), 4), "windows": [round(x, 4) for x in v]}


def frame_images(H, W):
    y, x = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for cy, cx, r in ((0.3, 0.25, 0.16), (0.7, 0.7, 0.2), (0.2, 0.8, 0.08)):
        m |= (y - cy * H) ** 2 + (x - cx * W) ** 2 < (r * min(H, W)) ** 2
    g = np.random.default_rng(0)
    gt = (1.5 + 0.5 * g.random((H, W))).astype(np.float32)
    depth = (gt + np.where(m, 1.0, 0.0) + 0.05 * g.standard_normal((H, W))).astype(np.float32)
    opacity = np.clip(0.9 + 0.08 * g.standard_normal((H, W)), 0, 1).astype(np.float32)
    return tuple(torch.from_numpy(a).to(dev) for a in (depth, opacity, gt))


def device_time(H, W):
    d, o, g = frame_images(H, W)

    def call():
        mask, grid = VIS.high_loss_grid(d, o, g)
        return mask, grid, VIS.grid_dbscan(grid, 0.0, VIS.HIGH_LOSS_EPS, VIS.HIGH_LOSS_MIN_SAMPLES)
    for _ in range(10):
        mask, grid, c = call()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / CALLS)
    return {"size": f"{H}x{W}", "flagged_pixels": int(mask.sum()), "grid_ones": int(grid.sum()), "clusters": int(c.n_clusters),
            "device_ms_per_call": med(out)}


def step_time():
    W, H, N = int(os.environ.get("W", 256)), int(os.environ.get("H", 256)), int(os.environ.get("N", 20000))
    gt = syn.shell_scene(N, seed=2, W=W, H=H)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    frames = list(syn.orbit_sequence(gt, 2, W, H, dev))
    fused = dict(fused_render=True, fused_loss=True, fused_inputs=True, fused_preprocess=True)
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=2, **fused), device=dev)
    mp.run(frames[0])
    fr = frames[1]
    view = SplatMapper._w2c_host(torch.as_tensor(fr["quat"]).reshape(4), torch.as_tensor(fr["position"]).reshape(3))
    # the measured depth of the second frame with a part of it pulled 1 m towards the camera: the map then renders behind it there
    depth = fr["depth"].clone()
    depth[:, H // 4: H // 2, W // 8: W // 2] = (depth[:, H // 4: H // 2, W // 8: W // 2] - 1.0).clamp_min(0.2)

    def window(flag, read):
        mp.cfg["high_loss_target"] = flag
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            mp.high_loss_step(view, depth)
            if read:
                mp.high_loss_samples_pose_c2w
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) / STEPS * 1e3, (t2 - t0) / STEPS * 1e3
    for flag, read in ((False, False), (True, False), (True, True)):
        window(flag, read)
    res = {k: [] for k in ("off_enqueue", "off_done", "on_enqueue", "on_done", "on_read_pose")}
    for _ in range(5):
        e, d = window(False, False); res["off_enqueue"].append(e); res["off_done"].append(d)
        e, d = window(True, False); res["on_enqueue"].append(e); res["on_done"].append(d)
        e, d = window(True, True); res["on_read_pose"].append(d)
    mp.cfg["high_loss_target"] = True
    mp.high_loss_step(view, depth)
    pose = mp.high_loss_samples_pose_c2w
    table = 4 + 4 + 3 * 4 * 256
    return {"size": f"{H}x{W}", "gaussians_in_map": int(mp.params["means3D"].shape[0]), "flagged_pixels": int(mp.high_loss_mask.sum()),
            "grid_ones": int(mp.high_loss_grid.sum()), "pose": pose is not None,
            "host_ms_per_step": {k: med(v) for k, v in res.items()},
            "bytes_to_host_per_frame": {"before_mask_HxW_bool": H * W, "after_total_count_and_256_row_table": table,
                                        "after_tracked_frame_with_pose": table + 64}}


print(json.dumps({"calls_per_window": CALLS, "steps_per_window": STEPS, "device": [device_time(256, 256), device_time(512, 512)],
                  "mapper_step": step_time()}))
