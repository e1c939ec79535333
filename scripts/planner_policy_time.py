"""The roadmap subregions and the hierarchical choice at the planner's shapes (GPU box): the floor plan of scripts/roadmap_time.py
(tests/roadmap_cases.floor_plan at 128 x 128, seed 3) magnified to SIZE x SIZE (default 256 and 1024), the agent at the roomiest pixel, radius
and cells magnified with it.  On the Roadmap of plan_roadmap:
  (a) every new stage between device events -- node_distances, subregions, nodes_in_horizon, and path_to + shortcut_path of the last node --
      the median of REPEATS runs after one warm-up;
  (b) the whole chain of plan_step(policy=...) behind the roadmap WITHOUT the scores' renders (policy.plan with seeded stand-in scores), wall
      clock around a synchronise;
  (c) baseline 1, the host chain of the same rules: csgraph Dijkstra from every node, scipy's average linkage and fcluster, the line rule in
      Python integers for the horizon flags and the shortcut, wall clock, with the thread pools the environment gives (OMP_NUM_THREADS);
  (d) baseline 2, node_distances as K calls of grid_geodesic -- the only way to D before gs_node_distances; each call reads 4 bytes per
      relaxation round -- wall clock around a synchronise.
The outputs are compared before anything is reported (D three ways, the labels with the restatement and with scipy, the horizon flags, the
shortcut).  Environment: SIZES (default "256,1024"), REPEATS (default 5).  Prints JSON."""
import json
import math
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import policy as PL, roadmap as RM  # noqa: E402
from tests import policy_cases as pc  # noqa: E402
from tests import roadmap_cases as rc  # noqa: E402

dev = torch.device("cuda")
SIZES = [int(s) for s in os.environ.get("SIZES", "256,1024").split(",")]
REPEATS = int(os.environ.get("REPEATS", 5))
BASE, BASE_RADIUS_PX, BASE_CELL, BASE_PX_PER_M = 128, 2.0, 8, 8.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def device_stages(rm, px_per_m, radius_px):
    ms = {}
    D, ms["node_distances"] = timed(lambda: RM.node_distances(rm))
    (labels, count, heights), ms["subregions"] = timed(lambda: RM.subregions(rm, D, px_per_m))
    horizon, ms["nodes_in_horizon"] = timed(lambda: RM.nodes_in_horizon(rm))
    path, ms["path_to_last_node"] = timed(lambda: rm.path_to(rm.K - 1))
    (short, k, safe), ms["shortcut_path"] = timed(lambda: RM.shortcut_path(rm, path, radius_px))
    return ms, dict(D=D, labels=labels, horizon=horizon, path=path, short=short, k=k, safe=safe)


def geodesic_loop(rm):
    """D as the parent commit gets it: one grid_geodesic per node, sampled at the nodes on the device"""
    nodes = rm.node_rc.cpu().numpy()
    r, c = rm.node_rc[:, 0].long(), rm.node_rc[:, 1].long()
    rows = [RM.grid_geodesic(rm.roadmap, (int(a), int(b)))[r, c] for a, b in nodes]
    return torch.stack(rows)


def host_chain(roadmap, dist2, node_rc, agent, path, px_per_m, radius_px):
    t0 = time.perf_counter()
    D = pc.ref_node_distances(roadmap, node_rc)
    t1 = time.perf_counter()
    labels, _ = pc.scipy_labels(pc.ref_C(node_rc, D), 2.0 * px_per_m)
    t2 = time.perf_counter()
    horizon = (pc.ref_clearance(dist2, np.concatenate([np.tile(agent, (len(node_rc), 1)), node_rc], 1)) >= 1).astype(np.uint8)
    t3 = time.perf_counter()
    clear = pc.ref_clearance(dist2, np.concatenate([np.tile(agent, (len(path), 1)), path], 1))
    ok = clear >= math.ceil((1.5 * radius_px) ** 2)
    ok[0] = True
    k = int(np.flatnonzero(ok).max())
    t4 = time.perf_counter()
    ms = dict(node_distances=t1 - t0, subregions=t2 - t1, nodes_in_horizon=t3 - t2, shortcut_path=t4 - t3, total=t4 - t0)
    return {key: v * 1e3 for key, v in ms.items()}, dict(D=D, labels=labels, horizon=horizon, k=k)


def main():
    out = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS, host_threads=os.environ.get("OMP_NUM_THREADS"), sizes={})
    for size in SIZES:
        if size % BASE:
            raise SystemExit(f"SIZES must be multiples of {BASE}")
        f = size // BASE
        radius_px, cell, px_per_m = BASE_RADIUS_PX * f, min(RM.MAX_CELL, BASE_CELL * f), BASE_PX_PER_M * f
        free, unseen = (np.kron(m, np.ones((f, f), np.uint8)) for m in rc.floor_plan(BASE, BASE, seed=3))
        r, c = rc.roomiest_pixel(*rc.floor_plan(BASE, BASE, seed=3))
        agent = (r * f + f // 2, c * f + f // 2)
        maps = types.SimpleNamespace(free_map_binary=rc.t(free, dev), visible_map_binary=rc.t(unseen, dev))
        rm = RM.plan_roadmap(maps, agent, radius_px, cell)
        device_stages(rm, px_per_m, radius_px)
        runs = [device_stages(rm, px_per_m, radius_px) for _ in range(REPEATS)]
        stage_ms = {k: statistics.median(run[0][k] for run in runs) for k in runs[0][0]}
        got = runs[-1][1]
        rng = np.random.RandomState(0)
        inv, vol = rng.rand(rm.K) * 400.0, rng.rand(rm.K)
        chain = lambda: PL.plan(rm, PL.SubregionPolicy(step_px=2.0 * f, radius_px=radius_px), lambda: (inv, vol), px_per_m, radius_px)
        chain()
        whole = [wall(chain)[1] for _ in range(REPEATS)]
        geodesic_loop(rm)
        loops = [wall(lambda: geodesic_loop(rm)) for _ in range(max(1, REPEATS // 2))]
        roadmap, dist2, node_rc, path = rc.n(rm.roadmap), rc.n(rm.dist2), rc.n(rm.node_rc), rc.n(got["path"])
        host_chain(roadmap, dist2, node_rc, agent, path, px_per_m, radius_px)       # (the first run pays for imports and thread pools)
        host_ms, host = host_chain(roadmap, dist2, node_rc, agent, path, px_per_m, radius_px)
        restated, _ = pc.ref_linkage(pc.ref_C(node_rc, host["D"]), 2.0 * px_per_m)
        same = dict(D_scipy=bool(np.array_equal(rc.n(got["D"]), host["D"])), D_geodesic_loop=bool(np.array_equal(rc.n(loops[-1][0]), host["D"])),
                    labels_restated=bool(np.array_equal(rc.n(got["labels"]), restated)), labels_scipy=bool(np.array_equal(rc.n(got["labels"]), host["labels"])),
                    horizon=bool(np.array_equal(rc.n(got["horizon"]), host["horizon"])), shortcut_k=bool(int(got["k"].item()) == host["k"]))
        out["sizes"][str(size)] = dict(agent=agent, radius_px=radius_px, cell=cell, px_per_m=px_per_m, K=rm.K, roadmap_pixels=int(rm.roadmap.sum()),
                                       subregions=int(rc.n(got["labels"]).max(initial=-1)) + 1, rounds_B=rm.rounds[1], path_pixels=len(path),
                                       device_stage_ms=stage_ms, policy_chain_wall_ms=statistics.median(whole),
                                       host_chain_ms=host_ms, geodesic_loop_wall_ms=statistics.median(v for _, v in loops), device_equals_host=same)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
