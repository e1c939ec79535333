"""The planner's global visibility query over K Voronoi nodes, finished on the device (GPU box): src/visualizer/visualizer.py:991-995 calls
get_global_invisibility per node and keeps two floats, node['invisibility'] and node['volume'] (src/mapper/__init__.py:8-90).
  (a) visibility.global_invisibility_nodes: renders + gs_grid_dbscan on the device, ONE copy of depth, invisibility and labels of every node --
      the query up to the DBSCAN labels;
  (b) visibility.global_invisibility_scores: the same + gs_cluster_hulls, ONE copy of [K] invisibility, [K] volume, [K] status;
  (c) (a) + the host finish of the loop behind the labels: the numpy restatement of dilate / findContours (tests/hull_cases.py: OpenCV is not a
      dependency) and scipy.spatial.ConvexHull if it imports (else the restated hull -- the JSON says which).
Five alternating repeats of `calls` queries each, host clock around work that ends on the host; medians and spread in milliseconds per query of K
nodes, the bytes that cross to the host per query, and the device time of gs_cluster_hulls alone (hipEvents around 20 calls).
Environment: N (Gaussians of synthetic.shell_scene, default 200 000), K (default 21), SCENE=shell|sphere.  Prints JSON."""
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
from tests import cluster_cases as cc, hull_cases as hc  # noqa: E402

dev = torch.device("cuda")
N = int(os.environ.get("N", 200_000))
K = int(os.environ.get("K", 21))
SCENE = os.environ.get("SCENE", "shell")
if SCENE == "shell":
    params = {k: v.to(dev) for k, v in syn.shell_scene(N, seed=2, W=LA.LOOK_W, H=LA.LOOK_H).items()}
else:                                                    # an opaque sphere with three holes: three compact blobs per panorama
    params = cc.cap_params(dev, 100.0, 10.0, 25.0, n=N, scale=0.15 * (5000 / N) ** 0.5, more_holes=((-120.0, -20.0, 17.0), (10.0, 30.0, 12.0)))
c2w = np.eye(4)
g = np.random.default_rng(0)
positions = np.stack([0.5 * g.uniform(-1, 1, K), np.ones(K), 0.5 * g.uniform(-1, 1, K)], 1)

try:
    from scipy.spatial import ConvexHull

    def hull(pts, scale):
        p = pts * np.array([scale[0], scale[1], 1.0])
        return float(ConvexHull(p).volume) if len(p) >= 4 and np.linalg.matrix_rank(p - p[0]) == 3 else 0.0
    host_hull = "scipy.spatial.ConvexHull"
except ImportError:
    def hull(pts, scale):
        return hc.hull_volume(pts) * scale[0] * scale[1]
    host_hull = "numpy restatement (tests/hull_cases.hull_volume)"
ROWS = hc.ellipse_rows()
SCALE = (np.deg2rad(360 / 360), np.deg2rad(150 / 150))


def finish(d):
    """the loop of get_convexhull_volume behind its DBSCAN line on one node of (a) -> (last_invisibility, last_volume)"""
    inv = vol = 0.0
    for c in range(d["n_clusters"]):
        _, pts, _ = hc.restate_cluster(d["labels"], d["depth"][..., 0], c, ROWS, 15)
        v = hull(pts, SCALE)
        inv += float(d["sum_value"][c]) * v
        vol += v
    return inv, vol


def query_a():
    return VIS.global_invisibility_nodes(params, c2w, positions)


def query_b():
    return VIS.global_invisibility_scores(params, c2w, positions)


def query_c():
    return [finish(d) if d is not None else (0.0, 0.0) for d in query_a()]


def window(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


calls_ab, calls_c = int(os.environ.get("CALLS_AB", 20)), int(os.environ.get("CALLS_C", 1))
for fn in (query_a, query_b):
    for _ in range(2):
        fn()
ta, tb, tc = [], [], []
for _ in range(5):
    ta.append(window(query_a, calls_ab)); tb.append(window(query_b, calls_ab)); tc.append(window(query_c, calls_c))
a, b, c = query_a(), query_b(), query_c()
bytes_a = sum(sum(np.asarray(v).nbytes for v in d.values()) for d in a if d is not None)
bytes_b = b[0].nbytes + b[1].nbytes + 4 * K
# the hull kernels alone
pano = VIS.look_around_nodes(params, c2w, positions)
gd = VIS.grid_dbscan(pano.opacity, VIS.GLOBAL_THRESHOLD, VIS.GLOBAL_EPS, VIS.GLOBAL_MIN_SAMPLES, complement=True)
h = VIS.cluster_hulls(gd.labels, pano.depth, gd)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
e0.record()
for _ in range(20):
    h = VIS.cluster_hulls(gd.labels, pano.depth, gd)
e1.record()
torch.cuda.synchronize()
vol_c, inv_c = np.array([v for _, v in c]), np.array([i for i, _ in c])
res = {"scene": SCENE, "gaussians": N, "nodes": K, "host_hull": host_hull,
       "a_labels_ms": [round(t, 3) for t in ta], "b_scores_ms": [round(t, 3) for t in tb], "c_labels_plus_host_finish_ms": [round(t, 3) for t in tc],
       "a_median_ms": round(statistics.median(ta), 3), "a_spread_ms": round(max(ta) - min(ta), 3),
       "b_median_ms": round(statistics.median(tb), 3), "b_spread_ms": round(max(tb) - min(tb), 3),
       "c_median_ms": round(statistics.median(tc), 3), "c_spread_ms": round(max(tc) - min(tc), 3),
       "bytes_to_host_a_and_c": int(bytes_a), "bytes_to_host_b": int(bytes_b),
       "cluster_hulls_device_ms_per_call": round(e0.elapsed_time(e1) / 20, 4),
       "clusters_per_node": gd.n_clusters.tolist(), "max_contour_points": int(h.n_points.max()), "status": h.status.tolist(),
       "volume_b": [float(f"{v:.6g}") for v in b[1]], "max_rel_volume_difference_b_vs_c": float(np.max(np.abs(b[1] - vol_c) / np.maximum(np.abs(vol_c), 1e-300))),
       "max_rel_invisibility_difference_b_vs_c": float(np.max(np.abs(b[0] - inv_c) / np.maximum(np.abs(inv_c), 1e-300)))}
print(json.dumps(res))
