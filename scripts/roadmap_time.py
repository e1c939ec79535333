"""The planner roadmap at its own shapes (GPU box): one seeded floor plan (tests/roadmap_cases.floor_plan at 128 x 128, seed 3: 52 % of it
traversable) magnified to SIZE x SIZE (default 256 and 1024: factors 2 and 8), the agent at the roomiest pixel, the radius (2 px at 128) and the
cells (8 px at 128) magnified with it -- the same building at two map resolutions.
  (a) every stage of plan_roadmap between device events (the two geodesic fields include their per-round 4-byte reads: the events span them),
      the median of REPEATS runs after one warm-up, with the relaxation round counts;
  (b) plan_roadmap as a whole, wall clock around a synchronise, and its one device-to-host copy of K, the entry and the status alone;
  (c) the same rules as the scipy / numpy chain of the tests on the host (binary_opening, binary_dilation, label, distance_transform_edt with
      its indices in place of the brute-force feature, the numpy roadmap, csgraph Dijkstra twice, the numpy nodes), wall clock, with the
      thread pools the environment gives (OMP_NUM_THREADS); the device's and the host's outputs are compared (dist2, roadmap, fields, nodes).
Environment: SIZES (default "256,1024"), REPEATS (default 5).  Prints JSON."""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import _lib, rasterizer as R, roadmap as RM  # noqa: E402
from scipy import ndimage  # noqa: E402
from tests import roadmap_cases as rc  # noqa: E402

dev = torch.device("cuda")
SIZES = [int(s) for s in os.environ.get("SIZES", "256,1024").split(",")]
REPEATS = int(os.environ.get("REPEATS", 5))
BASE, BASE_RADIUS_PX, BASE_CELL = 128, 2.0, 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def device_stages(free, unseen, agent, RADIUS_PX, CELL):
    ms = {}
    H, W = free.shape
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    trav, ms["traversable_map"] = timed(lambda: RM.traversable_map(free, unseen, agent, status=status[0:1]))
    (dist2, feature), ms["clearance_field"] = timed(lambda: RM.clearance_field(trav))
    roadmap, ms["voronoi_roadmap"] = timed(lambda: RM.voronoi_roadmap(trav, dist2, feature, int(np.ceil(RADIUS_PX ** 2))))
    (field_a, rounds_a), ms["grid_geodesic_A"] = timed(lambda: RM.grid_geodesic(trav, agent, status=status[1:2], return_rounds=True))
    entry = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = RM._scratch(H, W, dev)
    _, ms["roadmap_entry"] = timed(lambda: _lib.check(_lib.get().gs_roadmap_entry(H, W, R._ptr(roadmap), R._ptr(field_a), R._ptr(entry), R._ptr(scratch),
                                                                                  _lib.stream_ptr(dev))))
    (field_b, rounds_b), ms["grid_geodesic_B"] = timed(lambda: RM._geodesic(roadmap, H, W, (-1, -1), entry, status[2:3], None))
    nodes, ms["roadmap_nodes"] = timed(lambda: RM.roadmap_nodes(roadmap, dist2, field_b, CELL))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    small = torch.cat([nodes[3], entry, status]).tolist()
    ms["one_copy"] = (time.perf_counter() - t0) * 1e3
    K = small[0]
    _, ms["trace_path_last_node"] = timed(lambda: RM.trace_path(roadmap, field_b, nodes[0][K - 1], H * W)) if K else (None, 0.0)
    return ms, dict(rounds_A=rounds_a, rounds_B=rounds_b, K=K, traversable=int(trav.sum()), roadmap=int(roadmap.sum()))


def host_chain(free, unseen, agent, RADIUS_PX, CELL):
    t0 = time.perf_counter()
    trav, _ = rc.ref_traversable(free, unseen, agent, 4, 3)
    t1 = time.perf_counter()
    edt, idx = ndimage.distance_transform_edt(np.pad(trav != 0, 1), return_indices=True)
    dist2 = np.rint(edt[1:-1, 1:-1] ** 2).astype(np.int32)
    feature = (np.moveaxis(idx, 0, -1)[1:-1, 1:-1] - 1).astype(np.int16)
    t2 = time.perf_counter()
    roadmap = rc.ref_roadmap(trav, dist2, feature, int(np.ceil(RADIUS_PX ** 2)))
    t3 = time.perf_counter()
    field_a, _ = rc.ref_geodesic(trav, agent)
    er, ec, _ = rc.ref_entry(roadmap, field_a)
    field_b, _ = rc.ref_geodesic(roadmap, (er, ec))
    t4 = time.perf_counter()
    nodes = rc.ref_nodes(roadmap, dist2, field_b, CELL)
    t5 = time.perf_counter()
    ms = dict(traversable_map=t1 - t0, clearance_field=t2 - t1, voronoi_roadmap=t3 - t2, geodesic_A_entry_B=t4 - t3, roadmap_nodes=t5 - t4, total=t5 - t0)
    return {k: v * 1e3 for k, v in ms.items()}, dict(trav=trav, dist2=dist2, field_a=field_a, nodes=nodes)


def main():
    out = dict(device=torch.cuda.get_device_name(0), repeats=REPEATS, host_threads=os.environ.get("OMP_NUM_THREADS"), sizes={})
    for size in SIZES:
        if size % BASE:
            raise SystemExit(f"SIZES must be multiples of {BASE}")
        f = size // BASE
        RADIUS_PX, CELL = BASE_RADIUS_PX * f, min(RM.MAX_CELL, BASE_CELL * f)
        free, unseen = (np.kron(m, np.ones((f, f), np.uint8)) for m in rc.floor_plan(BASE, BASE, seed=3))
        r, c = rc.roomiest_pixel(*rc.floor_plan(BASE, BASE, seed=3))
        agent = (r * f + f // 2, c * f + f // 2)
        dfree, dunseen = rc.t(free, dev), rc.t(unseen, dev)
        maps = types.SimpleNamespace(free_map_binary=dfree, visible_map_binary=dunseen)
        device_stages(dfree, dunseen, agent, RADIUS_PX, CELL)
        runs = [device_stages(dfree, dunseen, agent, RADIUS_PX, CELL) for _ in range(REPEATS)]
        stage_ms = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
        whole = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rm = RM.plan_roadmap(maps, agent, RADIUS_PX, CELL)
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
        host_chain(free, unseen, agent, RADIUS_PX, CELL)                # (the first run pays for imports and thread pools)
        host_ms, host = host_chain(free, unseen, agent, RADIUS_PX, CELL)
        same = dict(trav=bool(np.array_equal(rc.n(rm.trav), host["trav"])), dist2=bool(np.array_equal(rc.n(rm.dist2), host["dist2"])),
                    field_agent=bool(np.array_equal(rc.n(rm.field_agent), host["field_a"])),
                    nodes_with_scipy_tie_rule=bool(np.array_equal(rc.n(rm.node_rc), host["nodes"][0]) and np.array_equal(rc.n(rm.node_field), host["nodes"][2])))
        out["sizes"][str(size)] = dict(agent=agent, radius_px=RADIUS_PX, cell=CELL, counts=runs[0][1], device_stage_ms=stage_ms, device_stage_sum_ms=sum(v for k, v in stage_ms.items() if k != "trace_path_last_node"),
                                       plan_roadmap_wall_ms=statistics.median(whole), host_scipy_chain_ms=host_ms, device_equals_host=same)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
