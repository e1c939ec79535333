"""One camera-tracking iteration on two frame sizes -- 256 x 256 with 200 k Gaussians and 640 x 480 with 500 k -- by three paths, and the wall
time of one whole track_frame (40 iterations).  GPU box.  Prints one JSON line per (size, path); median and spread of REPS timed blocks of
ITERS iterations each (wall clock around a synchronised block).

    tracking_iteration  mapping.tracking_iteration: device-pose forward, render, gs_tracking_loss, pose-only backward, gs_tracking_step
    fused_get_loss      get_loss(tracking=True, fused=True, fused_preprocess=True) + backward + torch.optim.Adam on the two camera tensors
    unfused             get_loss(tracking=True) + backward + torch.optim.Adam (two raster passes, transform_to_frame(camera_grad=True))
    track_frame         mapping.track_frame(fused=True), tracking_iters = 40, use_depth_loss_thres off (one round)
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from activesplat_amd import mapping as M  # noqa: E402
from tests import tracking_cases as T  # noqa: E402

ITERS, REPS, WARM = int(os.environ.get("ITERS", 20)), int(os.environ.get("REPS", 5)), int(os.environ.get("WARM", 5))


def timed(step, iters=ITERS, reps=REPS, warm=WARM):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / iters * 1e3)
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), iters=iters, reps=reps)


def main():
    dev = torch.device("cuda")
    only = os.environ.get("ONLY")
    for n, W, H in ((200_000, 256, 256), (500_000, 640, 480)):
        params, curr, variables, t, _truth = T.track_scene(n, W, H, "cuda")
        cfg = M.tracking_config(dict(use_depth_loss_thres=False))
        w = cfg["loss_weights"]
        paths = {}
        state = M.TrackingState(params, W, H)
        state.begin(params, t)
        paths["tracking_iteration"] = lambda: M.tracking_iteration(params, curr, variables, t, cfg, state)
        opt = torch.optim.Adam([{"params": [params["cam_unnorm_rots"]], "lr": 1e-3}, {"params": [params["cam_trans"]], "lr": 4e-3}])

        def torch_step(**flags):
            loss, _v, _ = M.get_loss(params, curr, variables, t, w, cfg["use_sil_for_loss"], cfg["sil_thres"], tracking=True, **flags)
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        paths["fused_get_loss"] = lambda: torch_step(fused=True, fused_preprocess=True)
        paths["unfused"] = lambda: torch_step()
        for path, step in paths.items():
            if only and path != only:
                continue
            print(json.dumps(dict(P=n, W=W, H=H, path=path, **timed(step))), flush=True)
        if not only or only == "track_frame":
            cfg40 = dict(tracking_iters=40, use_depth_loss_thres=False)
            print(json.dumps(dict(P=n, W=W, H=H, path="track_frame", iterations=40,
                                  **timed(lambda: M.track_frame(params, curr, variables, t, cfg40), iters=1, reps=REPS, warm=1))), flush=True)
        del params, curr, variables, state
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
