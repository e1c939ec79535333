"""The frame ingest at the mapper's own shapes (GPU box): what the first per-frame stage costs with `device_ingest` off (the host resizes and
pageable copies of frames.to_mapping_tensors: the code of the parent commit) and on (ingest.FrameIngest: one upload, one gs_frame_ingest launch).
  (1) SplatMapper.run_raw over a synthetic orbit (FRAMES frames, default 20; the shipped schedule: map_every = keyframe_every = 5,
      mapping_iters = 2) for every set-up of SETUPS: source size -> mapping size, densify_downscale_factor.  After one untimed sequence of each
      kind, REPEATS (>= 5) sequences with device_ingest off and on, alternating, a fresh mapper each:
        * host wall time per run_raw call WITHOUT a synchronise, split into map frames (id == 0 or (id + 1) % 5 == 0) and other frames;
        * wall time of the whole sequence, ending in ONE synchronise.
      Milliseconds; median and [min - max] over the repeats.  Both the fused paths of the loop and the reference's call pattern are run
      (FUSED=0: the latter only).
  (2) the gs_frame_ingest launch alone, from device events: ingest.ingest_frame on device tensors between its own pair of events, behind a busy
      kernel long enough for the host to have enqueued all three (so the figure is device time, not the host's enqueue), CALLS (default 100) calls
      after 20 untimed ones; microseconds, median and p10 / p90.  PROFILE=1: only 50 such calls per set-up, for
      `rocprofv3 --kernel-trace --stats -- python scripts/ingest_time.py`.
Environment: FRAMES, REPEATS, CALLS, N (Gaussians of the synthetic scene, default 20000), FUSED.  Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import ingest as IN, synthetic as syn  # noqa: E402
from activesplat_amd.mapper import SplatMapper  # noqa: E402

dev = torch.device("cuda")
FRAMES = int(os.environ.get("FRAMES", 20))
REPEATS = max(5, int(os.environ.get("REPEATS", 5)))
CALLS = int(os.environ.get("CALLS", 100))
N = int(os.environ.get("N", 20000))
#: (source size, mapping size, densify_downscale_factor)
SETUPS = ((256, 256, 1), (256, 256, 2), (512, 256, 1), (512, 256, 2))
FUSED = dict(fused_render=True, fused_loss=True, fused_inputs=True, fused_preprocess=True, fused_adam=True, fused_iteration=True, fused_growth=True)


def med(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def raw_frames(src):
    """the orbit as the simulator would hand it over: uint8 image, metric depth, camera-to-world pose, and the tracker's pose parameters"""
    gt = syn.shell_scene(N, seed=2, W=src, H=src)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    out = []
    for fr in syn.orbit_sequence(gt, FRAMES, src, src, dev):
        image = (fr["color"].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        depth = fr["depth"][0].cpu().numpy()
        out.append((np.ascontiguousarray(image), np.ascontiguousarray(depth), np.linalg.inv(np.asarray(fr["w2c"], dtype=np.float64)), fr["id"],
                    fr["quat"], fr["position"]))
    return out


def sequence(frames, size, fac, on, flags):
    mp = SplatMapper(syn.intrinsics(size, size), size, size, config=dict(step_num=FRAMES, densify_downscale_factor=fac, device_ingest=on, **flags),
                     device=dev)
    every = mp.cfg["map_every"]
    map_ms, other_ms = [], []
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for image, depth, pose, fid, quat, position in frames:
        t0 = time.perf_counter()
        mp.run_raw(image, depth, pose, fid, quat, position)
        (map_ms if fid == 0 or (fid + 1) % every == 0 else other_ms).append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t_start) * 1e3
    return whole, statistics.mean(map_ms), statistics.mean(other_ms), int(mp.params["means3D"].shape[0])


def mapper_times(frames, size, fac, flags):
    for on in (False, True):
        sequence(frames, size, fac, on, flags)
    res = {m: {"whole_sequence_ms": [], "map_frame_host_ms": [], "other_frame_host_ms": []} for m in ("off", "on")}
    gaussians = {}
    for _ in range(REPEATS):
        for on in (False, True):
            whole, a, b, n = sequence(frames, size, fac, on, flags)
            r = res["on" if on else "off"]
            r["whole_sequence_ms"].append(whole)
            r["map_frame_host_ms"].append(a)
            r["other_frame_host_ms"].append(b)
            gaussians["on" if on else "off"] = n
    out = {m: {k: med(v) for k, v in r.items()} for m, r in res.items()}
    off, on = out["off"]["whole_sequence_ms"], out["on"]["whole_sequence_ms"]
    out["gaussians_in_map"] = gaussians
    # "faster" only when the two ranges do not touch
    out["on_faster_than_off_beyond_the_spread"] = bool(on["max"] < off["min"])
    return out


def kernel_time(frames, src, sizes):
    image, depth = torch.from_numpy(frames[0][0]).to(dev), torch.from_numpy(frames[0][1]).to(dev)
    calls = 50 if os.environ.get("PROFILE") else CALLS
    for _ in range(20):
        IN.ingest_frame(image, depth, sizes)
    torch.cuda.synchronize()
    if os.environ.get("PROFILE"):
        for _ in range(calls):
            IN.ingest_frame(image, depth, sizes)
        torch.cuda.synchronize()
        return None
    sleep = getattr(torch.cuda, "_sleep", None)
    us = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if sleep is not None:
            sleep(400_000)                      # (some hundred microseconds of device time in front: the three enqueues below are in by then)
        e0.record()
        IN.ingest_frame(image, depth, sizes)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us = sorted(us)
    return {"median_us": round(statistics.median(us), 2), "p10_us": round(us[len(us) // 10], 2), "p90_us": round(us[(9 * len(us)) // 10], 2),
            "behind_a_busy_kernel": sleep is not None}


res = {"device": torch.cuda.get_device_name(0), "frames": FRAMES, "repeats": REPEATS, "calls": CALLS, "scene_gaussians": N, "setups": []}
by_src = {}
for src, size, fac in SETUPS:
    if src not in by_src:
        by_src[src] = raw_frames(src)
    frames = by_src[src]
    sizes = [(size, size)] + ([(int(size / fac), int(size / fac))] if fac != 1 else [])
    r = {"source": f"{src}x{src}", "mapping": f"{size}x{size}", "densify_downscale_factor": fac,
         "gs_frame_ingest_between_events": kernel_time(frames, src, sizes)}
    if not os.environ.get("PROFILE"):
        kinds = (("fused", FUSED), ("reference_pattern", {})) if int(os.environ.get("FUSED", 1)) else (("reference_pattern", {}),)
        for name, flags in kinds:
            r["run_raw_" + name] = mapper_times(frames, size, fac, flags)
    res["setups"].append(r)
print(json.dumps(res))
