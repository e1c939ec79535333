"""The simulated agent at a user's shapes (GPU box): agent.navgrid and the closed loop of explore.Explorer.
  (1) agent.navgrid between its own pair of device events at SIZES (256 x 256 and 1024 x 1024 cells over the room's footprint and a margin) on the
      12-triangle room and on the same room with every wall tessellated into QUADS x QUADS quads (default 290: 1 009 200 triangles; the room of
      scripts/mesh_sensor_time.py); CALLS (default 50) calls after 20 untimed ones; milliseconds, median and p10 / p90.  Every call ends in the copy
      of its two counters, so the device is idle when the next call begins: the figure holds the four launches, their enqueue gaps and the scratch
      allocation, not the kernels alone -- those come from `rocprofv3 --kernel-trace --stats -- python scripts/agent_time.py` with PROFILE=1 (20
      calls per set-up, nothing else) and ONLY=<set-up name> (one set-up per profiler run).  With each set-up: D (the length of the tile lists) and
      the longest tile list.
  (2) the numpy restatement of the rule (tests/agent_cases.py: restate) on the 12-triangle room at 64 x 64 cells, host seconds, next to navgrid on the
      same grid, and whether the two grids are equal.  The restatement is the only yardstick there is: no device predecessor, no Habitat.
  (3) the closed loop in the flat room at 256 x 256 frames: ACTIONS (default 150) actions of explore.Explorer (30 degree turns, one 45 degree look
      down in the bootstrap); actions per second of host wall time and the share spent in sensing (MeshSensor.frame), mapping (SplatMapper.run) and
      planning (SplatMapper.plan_step), each bracketed by a device synchronise; the first frame and the first plan are reported apart.
      Left out when PROFILE or ONLY is set.
Environment: CALLS, QUADS, ACTIONS, PROFILE, ONLY.  Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from activesplat_amd import agent as AG, explore as EX, policy as PL, sensor as S, synthetic as syn  # noqa: E402
from activesplat_amd.mapper import SplatMapper  # noqa: E402
import mesh_sensor_time as MT  # noqa: E402

dev = torch.device("cuda")
CALLS = int(os.environ.get("CALLS", 50))
QUADS = int(os.environ.get("QUADS", 290))
ACTIONS = int(os.environ.get("ACTIONS", 150))
PROFILE = os.environ.get("PROFILE", "0") == "1"
ONLY = os.environ.get("ONLY", "")
SIZES = (256, 1024)
FLOOR_Y = MT.ROOM[1][0]


def grid_of(size):
    """size x size cells over the room's footprint (4 m x 6 m) and 0.1 m around it"""
    return dict(origin_xz=(MT.ROOM[0][0] - 0.1, MT.ROOM[2][0] - 0.1), cell=6.2 / size, grid_shape=(size, size), floor_y=FLOOR_Y)


def navgrid_times(scene, size, calls):
    ms, grid = [], None
    for i in range(20 + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        grid = AG.navgrid(scene, **grid_of(size))
        b.record()
        b.synchronize()
        if i >= 20:
            ms.append(a.elapsed_time(b))
    values = torch.bincount(grid.reshape(-1).long(), minlength=4).tolist()
    return {"navgrid_ms": MT.spread(ms), "D": scene.last_navgrid_counts[0], "longest_tile_list": scene.last_navgrid_counts[1], "cells_by_value": values}


def against_restatement(scene, size=64):
    from tests import agent_cases as ac
    kw = grid_of(size)
    t0 = time.perf_counter()
    want = ac.restate(scene.vertices.cpu().numpy(), scene.triangles.cpu().numpy(), kw["origin_xz"], kw["cell"], kw["grid_shape"], floor_y=FLOOR_Y)
    seconds = time.perf_counter() - t0
    ms = []
    for _ in range(10):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = AG.navgrid(scene, **kw)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t1))
    return {"cells": f"{size} x {size}", "triangles": scene.num_triangles, "numpy_restatement_s": round(seconds, 3), "navgrid_host_ms_median": round(statistics.median(ms), 3),
            "equal": bool(np.array_equal(got.cpu().numpy(), want))}


class Clock:
    def __init__(self):
        self.ms = {}

    def wrap(self, obj, name, key):
        inner = getattr(obj, name)

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*a, **kw)
            torch.cuda.synchronize()
            self.ms.setdefault(key, []).append(1e3 * (time.perf_counter() - t0))
            return out
        setattr(obj, name, timed)


def closed_loop(scene, size=256):
    K = syn.intrinsics(size, size, fx=size / 2.0, fy=size / 2.0)
    sensor = S.MeshSensor(scene, K, size, size)
    nav = AG.NavGrid.build(scene, origin_xz=(MT.ROOM[0][0], MT.ROOM[2][0]), cell=0.0625, grid_shape=(96, 64), floor_y=FLOOR_Y)
    start = (0.0, 1.5)
    agent = AG.SimAgent(nav, start, turn_angle=30.0, tilt_angle=45.0)
    mp = SplatMapper(K, size, size, config=dict(step_num=ACTIONS + 2, densify_downscale_factor=2, device_ingest=True), device=dev)
    # the planner's window in the mapper's world (x = x - start x, z = -(z - start z)); the band from 0.1 m above the floor to the head
    plan = dict(world_center=(0.0 - start[0], -(0.0 - start[1])), world_shape=(4.0, 6.0), grid_shape=(64, 96), upper=-1.15, lower=0.25, agent_radius=0.1,
                node_spacing=0.5, scale_modifier=1.0)
    pol = PL.SubregionPolicy(step_px=agent.forward_step * 16.0, radius_px=0.1 * 16.0)
    ex = EX.Explorer(mp, sensor, agent, plan, policy=pol, look_down_steps=1)
    clock = Clock()
    clock.wrap(sensor, "frame", "sensing")
    clock.wrap(mp, "run", "mapping")
    clock.wrap(mp, "plan_step", "planning")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ex.run(ACTIONS)
    torch.cuda.synchronize()
    total = 1e3 * (time.perf_counter() - t0)
    first = {k: round(v[0], 3) for k, v in clock.ms.items()}
    rest = {k: sum(v[1:]) for k, v in clock.ms.items()}
    steady = total - sum(first.values())
    return {"actions": len(out["actions"]), "plans": out["plans"], "nodes": out["nodes"], "arrivals": out["arrivals"], "collisions": out["collisions"],
            "gaussians": int(mp.params["means3D"].shape[0]), "total_ms": round(total, 1), "first_call_ms": first,
            "actions_per_second_without_first_calls": round(1e3 * len(out["actions"]) / steady, 1),
            "share_without_first_calls": {k: round(v / steady, 3) for k, v in rest.items()},
            "per_call_ms_median": {k: round(statistics.median(v[1:]), 3) for k, v in clock.ms.items() if len(v) > 1}}


def main():
    scenes = {"room_12_triangles": 1, f"room_{12 * QUADS * QUADS}_triangles": QUADS}
    scenes = {name: MT.room(n) for name, n in scenes.items() if not ONLY or ONLY.startswith(name)}
    out = {"navgrid": {}}
    for name, scene in scenes.items():
        for size in SIZES:
            if not ONLY or ONLY == f"{name}_{size}x{size}":
                out["navgrid"][f"{name}_{size}x{size}"] = navgrid_times(scene, size, 20 if PROFILE else CALLS)
    if not PROFILE and not ONLY:
        out["against_restatement"] = against_restatement(scenes["room_12_triangles"])
        out["closed_loop_256x256"] = closed_loop(scenes["room_12_triangles"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
