"""The completion / accuracy judge at its own shape (GPU box): 200 000 mesh samples against 128 x 128 frames (scripts/judges/eval_actions.py samples
200 000 points and back-projects every frame of a run).
  (a) gs_cloud_nearest alone, both directions -- samples -> cloud (200 000 queries, 16 384 streamed points) and cloud -> samples -- hipEvents
      around `calls` back-to-back calls of each, five alternating repeats, milliseconds per call; next to each the derived floor
      pairs x 7 lane-operations / 78.6e12 per second (157.3 TF fp32 / 2) and the fraction of it reached;
  (b) gs_completion_row alone and gs_depth_cloud alone, the same way;
  (c) the whole CompletionJudge.add_frame: one frame, then a run of 100 frames, host clock around work that ends in rows();
  (d) the reference's method on this box's host: scipy.spatial.KDTree build + query for both directions (eval_actions.py:36-39) with workers=16,
      per frame, on the same samples and clouds (three frames).
Also the largest differences between (c)'s rows and rows computed from (d)'s distances.  Environment: SAMPLES (default 200 000), SIZE (default 128),
FRAMES (default 100), CALLS (default 200).  Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import judge as J, synthetic as syn  # noqa: E402
from tests import completion_cases as cc  # noqa: E402

dev = torch.device("cuda")
N = int(os.environ.get("SAMPLES", 200_000))
S = int(os.environ.get("SIZE", 128))
FRAMES = int(os.environ.get("FRAMES", 100))
CALLS = int(os.environ.get("CALLS", 200))
LANE_OPS_PER_S = 157.3e12 / 2

K = syn.intrinsics(S, S)
samples_h = cc.room_samples(N, seed=0)
samples = torch.from_numpy(samples_h).to(dev)
poses = [cc.yaw_pose(360.0 * i / FRAMES, [0.2, -0.1, 0.3]) for i in range(FRAMES)]
depths_h = [cc.room_depth(m, S, S) for m in poses]
depths = [torch.from_numpy(d).to(dev) for d in depths_h]
points, valid = J.depth_cloud(depths[0], K, poses[0])
P = int(points.shape[0])


def events(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


out_s = torch.empty(N, dtype=torch.float32, device=dev)
out_p = torch.empty(P, dtype=torch.float32, device=dev)
scratch = J._nearest(samples, None, points, valid, J.NEAREST_ROOT, out_s)
scratch = J._nearest(points, valid, samples, None, J.NEAREST_ROOT, out_p, scratch)
row = torch.zeros(6, dtype=torch.float64, device=dev)
jd = J.CompletionJudge(samples, device=dev)
jd.add_points(points, 0.0, valid)


def fwd():
    J._nearest(samples, None, points, valid, J.NEAREST_ROOT, out_s, scratch)


def bwd():
    J._nearest(points, valid, samples, None, J.NEAREST_ROOT, out_p, scratch)


def reduce_row():
    from activesplat_amd import _lib, rasterizer as R
    _lib.check(_lib.get().gs_completion_row(N, R._ptr(out_s), P, R._ptr(out_p), R._ptr(valid), 0.0, R._ptr(row), R._ptr(jd._row_scratch),
                                            _lib.stream_ptr(dev)))


def cloud():
    J.depth_cloud(depths[0], K, poses[0])


for fn in (fwd, bwd, reduce_row, cloud):
    for _ in range(3):
        fn()
t = {k: [] for k in ("samples_to_cloud", "cloud_to_samples", "row", "depth_cloud")}
for _ in range(5):
    t["samples_to_cloud"].append(events(fwd, CALLS)); t["cloud_to_samples"].append(events(bwd, CALLS))
    t["row"].append(events(reduce_row, CALLS)); t["depth_cloud"].append(events(cloud, CALLS))
floor_ms = N * P * 7 / LANE_OPS_PER_S * 1e3


def frames_ms(n):
    jd.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        jd.add_frame(depths[i % FRAMES], K, poses[i % FRAMES], 0.25 * i)
    rows = jd.rows()
    return (time.perf_counter() - t0) * 1e3, rows


frames_ms(2)
one = [frames_ms(1)[0] for _ in range(5)]
run = []
for _ in range(3):
    ms, rows = frames_ms(FRAMES)
    run.append(ms)

# the reference's method on the host
from scipy.spatial import KDTree  # noqa: E402

host, lo, inf, worst = [], np.ones(N), np.full(N, np.inf), 0.0
s64 = samples_h.astype(np.float64)
for i in range(3):
    pts, ok = J.depth_cloud(depths[i], K, poses[i])
    cloud_h = pts[ok.bool()].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    d, _ = KDTree(cloud_h).query(s64, workers=16)
    a, _ = KDTree(s64).query(cloud_h, workers=16)
    host.append((time.perf_counter() - t0) * 1e3)
    lo, inf = np.minimum(lo, d), np.minimum(inf, d)
    want = np.array([lo.mean(), np.mean(np.float64(lo < 0.05)), inf.mean(), np.mean(np.float64(inf < 0.05)), 0.25 * i, a.mean()])
    worst = max(worst, float(np.max(np.abs(rows[i] - want) / np.maximum(np.abs(want), 1e-300))))

med = {k: statistics.median(v) for k, v in t.items()}
res = {"samples": N, "frame": [S, S], "cloud_points": P, "valid_points": int(valid.sum()), "calls": CALLS,
       **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
       **{f"{k}_median_ms": round(m, 4) for k, m in med.items()},
       "floor_ms_per_direction": round(floor_ms, 4),
       "fraction_of_floor_samples_to_cloud": round(floor_ms / med["samples_to_cloud"], 3),
       "fraction_of_floor_cloud_to_samples": round(floor_ms / med["cloud_to_samples"], 3),
       "add_frame_one_ms": [round(x, 3) for x in one], "add_frame_one_median_ms": round(statistics.median(one), 3),
       "run_frames": FRAMES, "run_ms": [round(x, 2) for x in run], "run_ms_per_frame_median": round(statistics.median(run) / FRAMES, 4),
       "host_kdtree_workers16_ms_per_frame": [round(x, 1) for x in host], "host_kdtree_median_ms": round(statistics.median(host), 1),
       "max_relative_row_difference_device_vs_kdtree_first_3_frames": worst,
       "last_row": [float(f"{v:.9g}") for v in rows[-1]]}
print(json.dumps(res))
