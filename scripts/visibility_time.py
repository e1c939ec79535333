"""The planner's global visibility query over K Voronoi nodes (GPU box): src/visualizer/visualizer.py:991-995 calls get_global_invisibility per
node -- three views, three blocking copies, then get_convexhull_volume, whose first step is sklearn's DBSCAN(eps=5, min_samples=25) on the
pixels with 1 - opacity > 0.8 of the 150 x 360 panorama (src/mapper/__init__.py:8-19).
  (a) the parent commit's way on this library: per node lookaround.global_invisibility_inputs (one fused look_around, two device-to-host
      copies) + DBSCAN on the host (sklearn's if it imports, else the numpy restatement of tests/cluster_cases.py -- the JSON says which);
  (b) visibility.global_invisibility_nodes: one activation, K raster passes of 3 views (the default, bit-identical panoramas), one
      gs_grid_dbscan, one copy;  (b21) the same with nodes_per_pass=21: one raster pass for the 3 K views.
Five alternating repeats of `calls` queries each, host clock around work that ends in a device synchronise (both sides end on the host);
medians and spread in milliseconds per query of K nodes, (a) split into its render + copy and its clustering share.
`--kernel B`: only gs_grid_dbscan on B of the panoramas, 20 calls -- for `rocprofv3 --kernel-trace --stats -- python scripts/visibility_time.py
--kernel B`.  Environment: N (Gaussians of synthetic.shell_scene, default 200 000), K (default 21).  Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import lookaround as LA, synthetic as syn, visibility as VIS  # noqa: E402

dev = torch.device("cuda")
N = int(os.environ.get("N", 200_000))
K = int(os.environ.get("K", 21))
params = {k: v.to(dev) for k, v in syn.shell_scene(N, seed=2, W=LA.LOOK_W, H=LA.LOOK_H).items()}
c2w = np.eye(4)
g = np.random.default_rng(0)
positions = np.stack([0.5 * g.uniform(-1, 1, K), np.ones(K), 0.5 * g.uniform(-1, 1, K)], 1)

if len(sys.argv) > 2 and sys.argv[1] == "--kernel":
    B = int(sys.argv[2])
    opacity = VIS.look_around_nodes(params, c2w, positions[:B]).opacity.contiguous()
    for _ in range(20):
        out = VIS.grid_dbscan(opacity, VIS.GLOBAL_THRESHOLD, VIS.GLOBAL_EPS, VIS.GLOBAL_MIN_SAMPLES, complement=True)
    torch.cuda.synchronize()
    print(json.dumps({"kernel_only": True, "B": B, "calls": 20, "clusters": out.n_clusters.tolist(),
                      "masked": (out.labels > -2).sum(dim=(1, 2)).tolist()}))
    sys.exit(0)

try:
    from sklearn.cluster import DBSCAN

    def cluster(inv):
        pts = np.column_stack(np.where(inv > 0.8))
        return DBSCAN(eps=5, min_samples=25).fit_predict(pts) if len(pts) else np.zeros(0, np.int64)
    host_dbscan = "sklearn"
except ImportError:
    from tests import cluster_cases as cc

    def cluster(inv):
        r = cc.restate(inv, 0.8, 5, 25)
        return r["labels"][r["mask"]]
    host_dbscan = "numpy restatement (tests/cluster_cases.restate)"

split = [0.0, 0.0]


def query_a():
    out = []
    for p in positions:
        t0 = time.perf_counter()
        depth_np, inv_np = LA.global_invisibility_inputs(params, c2w, p)
        t1 = time.perf_counter()
        out.append((depth_np, inv_np, cluster(inv_np)))
        split[0] += t1 - t0
        split[1] += time.perf_counter() - t1
    return out


def query_b():
    return VIS.global_invisibility_nodes(params, c2w, positions)


def query_b21():
    return VIS.global_invisibility_nodes(params, c2w, positions, nodes_per_pass=21)


def window(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


calls_a, calls_b = int(os.environ.get("CALLS_A", 1)), int(os.environ.get("CALLS_B", 20))
for fn in (query_a, query_b, query_b21):
    for _ in range(2):
        fn()
split[:] = [0.0, 0.0]
ta, tb, tc = [], [], []
for _ in range(5):
    ta.append(window(query_a, calls_a)); tb.append(window(query_b, calls_b)); tc.append(window(query_b21, calls_b))
a, b = query_a(), query_b()
same = [int((b[k]["labels"][b[k]["invisibility"] > np.float32(0.8)] != a[k][2]).sum()) if (b[k]["invisibility"] > np.float32(0.8)).sum() == len(a[k][2])
        else "masks differ (atlas rounding)" for k in range(K)]
res = {"gaussians": N, "nodes": K, "host_dbscan": host_dbscan,
       "a_per_node_ms": [round(t, 3) for t in ta], "b_batched_ms": [round(t, 3) for t in tb],
       "a_median_ms": round(statistics.median(ta), 3), "a_spread_ms": round(max(ta) - min(ta), 3),
       "b_median_ms": round(statistics.median(tb), 3), "b_spread_ms": round(max(tb) - min(tb), 3),
       "b21_one_pass_ms": [round(t, 3) for t in tc], "b21_median_ms": round(statistics.median(tc), 3), "b21_spread_ms": round(max(tc) - min(tc), 3),
       "a_render_and_copy_ms_per_query": round(split[0] / (5 * calls_a + 1) * 1e3, 3), "a_host_dbscan_ms_per_query": round(split[1] / (5 * calls_a + 1) * 1e3, 3),
       "masked_pixels_per_node": [int((d["labels"] > -2).sum()) for d in b], "clusters_per_node": [d["n_clusters"] for d in b],
       "labels_differing_from_host_dbscan_per_node": same}
print(json.dumps(res))
