"""The simulated agent: the navigable area of a storey computed from the scene mesh on the device, the simulator's discrete actions on top of it, and
the reference's offline judge replayed without a simulator.

The reference moves its agent with Habitat-sim's `sim.step(action)` on a navmesh (src/dataloader/dataloader.py:237-272) and judges a run by replaying
the recorded `actions.txt` through the simulator (scripts/judges/eval_actions.py).  Habitat-sim does not run on this stack, so:

* `navgrid`        -- the public primitive: uint8 [H, W] on the scene's device, 1 = navigable floor, 0 = void, 2 and 3 = blocked, from
                      `gs_mesh_navgrid` (include/gsplat_hip.h states the rule: every triangle clipped against every cell in fp64, the y range
                      of the clipped polygon sets a floor bit and an obstacle bit);
* `NavGrid`        -- that grid eroded by the agent's radius (`roadmap.clearance_field`), copied to the host once;
* `SimAgent`       -- position, heading and pitch under the reference's action integers (0 stop, 1 move_forward, 2 turn_left, 3 turn_right,
                      4 look_up, 5 look_down); `.X_WV` is the pose `MeshSensor.frame` / `SplatMapper.run_raw` take;
* `save_actions` / `load_actions` / `replay` -- the reference's `actions.txt` (one integer per line);
* `judge_actions`  -- eval_actions.py:96-150 on `MeshSensor` + `judge.CompletionJudge`.

THIS IS A GRID RULE, NOT Recast and NOT Habitat's navmesh, and nothing here was run against Habitat-sim: where the two disagree about a cell, a
recorded `actions.txt` replays to another place.  Not modelled: sliding along obstacles (the reference runs Habitat with `allow_sliding: False`,
so a blocked step simply ends early), stairs and any change of floor height (the feet stay at `floor_y`), agent acceleration, sensor noise.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import rasterizer as R
from . import roadmap as RM
from .sensor import MAX_SIZE, MeshScene

STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT, LOOK_UP, LOOK_DOWN = range(6)       # _DefaultHabitatSimActions, as written to actions.txt
ACTIONS = (STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT, LOOK_UP, LOOK_DOWN)
VOID, FLOOR = 0, 1                                                             # cell values of `navgrid`; 2 and 3 are blocked


def _finite(value, name):
    v = float(value)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {value!r}")
    return v


@torch.no_grad()
def navgrid(scene, origin_xz, cell, grid_shape, floor_y, agent_height=1.5, max_climb=0.2):
    """The navigable area of the storey whose floor is at height `floor_y` of `scene` (a `MeshScene` in the simulator's world frame, y up) ->
    uint8 [H, W] on the scene's device.  `grid_shape` = (H, W); cell (r, c) is the closed square
    [x0 + c cell, x0 + (c + 1) cell] x [z0 + r cell, z0 + (r + 1) cell] with (x0, z0) = `origin_xz`; all scalars are HOST values, taken as fp64.
    A cell is 1 (floor) when some triangle has, inside the cell, a part within `max_climb` of the floor and no triangle has a part between
    `floor_y + max_climb` and `floor_y + agent_height`; 0 where there is neither, 2 or 3 where there is an obstacle (the exact rule:
    include/gsplat_hip.h, gs_mesh_navgrid).  Conservative: a triangle that only touches a cell's border counts for that cell.

    agent_height = 1.5 and max_climb = 0.2 (and `NavGrid.build`'s agent_radius = 0.1) are Habitat's DOCUMENTED agent defaults; they were not
    read from the reference, and the rule is not Habitat's navmesh construction.

    The tile lists are sized like `render_mesh`'s: the call is made with the capacity remembered in `scene.capacities`, the two counters are
    copied to the host (that copy waits for the device, once per call) and the call is repeated with room when the lists did not fit."""
    if not isinstance(scene, MeshScene):
        raise TypeError(f"scene must be a MeshScene, got {type(scene).__name__}")
    R._require_rocm(scene.device)
    H, W = (int(v) for v in grid_shape)
    if not (1 <= W <= MAX_SIZE and 1 <= H <= MAX_SIZE):
        raise ValueError(f"grid size {H} x {W} out of range (1 <= H, W <= {MAX_SIZE})")
    x0, z0 = (_finite(v, "origin_xz") for v in origin_xz)
    cell, floor_y = _finite(cell, "cell"), _finite(floor_y, "floor_y")
    agent_height, max_climb = _finite(agent_height, "agent_height"), _finite(max_climb, "max_climb")
    if cell <= 0.0:
        raise ValueError(f"cell must be positive, got {cell}")
    if max_climb < 0.0 or agent_height <= max_climb:
        raise ValueError(f"need 0 <= max_climb < agent_height, got max_climb {max_climb}, agent_height {agent_height}")
    lib, dev, T = _lib.get(), scene.device, scene.num_triangles
    key = ("navgrid", H, W)
    capacity = int(scene.capacities.get(key, max(4096, 4 * T)))
    grid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)           # (read as unsigned)
    while True:
        layout = _lib.GsMeshLayout()
        _lib.check(lib.gs_mesh_navgrid_layout(T, W, H, capacity, C.byref(layout)))
        scratch = torch.empty(int(layout.total_bytes), dtype=torch.uint8, device=dev)
        _lib.check(lib.gs_mesh_navgrid(scene.num_vertices, R._ptr(scene.vertices) if T else None, T, R._ptr(scene.triangles) if T else None, x0, z0, cell,
                                       floor_y, max_climb, agent_height, W, H, R._ptr(scratch), capacity, R._ptr(grid), R._ptr(counts), _lib.stream_ptr(dev)))
        need, longest = (int(v) & 0xffffffff for v in counts.tolist())         # the one copy that waits for the device
        if need <= capacity:
            break
        if need == 0xffffffff:
            raise RuntimeError("navgrid: the tile lists need 2^32 entries or more")
        capacity = min(0xfffffffe, need + need // 8)
    scene.capacities[key] = capacity
    scene.last_navgrid_counts = (need, longest)
    return grid


class NavGrid:
    """Where the agent's centre may stand: `grid` (uint8 [H, W], device: `navgrid`'s), `dist2` (int32 [H, W], device: the squared distance in
    cells from each floor cell to the nearest cell that is not floor, the image frame counting as one -- `roadmap.clearance_field` of
    grid == 1) and `free` (bool [H, W], HOST): floor cells with dist2 >= ceil((agent_radius / cell)^2), the threshold form of
    `roadmap.voronoi_roadmap`'s min_dist2.  `free` is copied to the host ONCE, in `build`: the scene is static, and the agent's state lives on
    the host because the sensor takes its pose as a host value anyway."""

    def __init__(self, grid, dist2, free, origin_xz, cell, floor_y, agent_radius):
        self.grid, self.dist2, self.free = grid, dist2, free
        self.x0, self.z0 = float(origin_xz[0]), float(origin_xz[1])
        self.cell, self.floor_y, self.agent_radius = float(cell), float(floor_y), float(agent_radius)
        self.H, self.W = int(free.shape[0]), int(free.shape[1])

    @classmethod
    @torch.no_grad()
    def build(cls, scene, origin_xz, cell, grid_shape, floor_y, agent_height=1.5, max_climb=0.2, agent_radius=0.1):
        """`navgrid(...)`, then the clearance field of its floor cells; 1 <= H, W <= roadmap.MAX_SIDE.  agent_radius = 0.1 m: Habitat's
        documented default (see `navgrid`)."""
        agent_radius = _finite(agent_radius, "agent_radius")
        if agent_radius < 0.0:
            raise ValueError(f"agent_radius must not be negative, got {agent_radius}")
        grid = navgrid(scene, origin_xz, cell, grid_shape, floor_y, agent_height, max_climb)
        floor = (grid == FLOOR).to(torch.uint8)
        dist2, _ = RM.clearance_field(floor)
        min_dist2 = int(math.ceil((agent_radius / float(cell)) ** 2))
        free = ((floor != 0) & (dist2 >= min_dist2)).cpu().numpy()             # the one copy to the host
        return cls(grid, dist2, free, origin_xz, cell, floor_y, agent_radius)

    def cell_of(self, x, z):
        """(r, c) of the cell that holds the point: floor((z - z0) / cell), floor((x - x0) / cell); it may lie outside the grid"""
        return int(math.floor((float(z) - self.z0) / self.cell)), int(math.floor((float(x) - self.x0) / self.cell))

    def is_free(self, x, z):
        """may the agent's centre stand at (x, z)?  Outside the grid counts as blocked."""
        r, c = self.cell_of(x, z)
        return 0 <= r < self.H and 0 <= c < self.W and bool(self.free[r, c])


class SimAgent:
    """The simulator's agent on a `NavGrid`.  The defaults are the reference's (config/env/activesplat_pointnav.yaml): 10 degrees per turn, 15
    per tilt, 0.065 m per forward step, the sensor 1.25 m above the feet.

    Heading and pitch are INTEGER COUNTS of turn and tilt steps; the angle is (count * step) modulo 360 degrees, so a full circle returns the
    same pose bits.  `X_WV` is the sensor pose in the convention `MeshSensor.frame` and `SplatMapper.run_raw` take: R = Ry(yaw) Rx(pitch) with
    Ry = [[c, 0, s], [0, 1, 0], [-s, 0, c]], the camera looks along its -z, turn_left increases yaw, look_up increases pitch (about the
    camera's x), position (x, floor_y + sensor_height, z).

    move_forward has NO SLIDING, as the reference's `allow_sliding: False`: with n = ceil(forward_step / (cell / 4)) the candidates
    p + (i / n) forward_step f, i = 1 .. n, f = (-sin yaw, -cos yaw) in (x, z), are tested in order and the agent stops at the last one before
    the first that is not free (`NavGrid.is_free`; it stays where it is when the first is not).  `step` returns whether the whole step was
    made.  The y of the feet stays `floor_y`: stairs are not modelled.  Whether Habitat clamps the pitch was not established: it is NOT
    clamped here.  `actions` is the list of actions so far; `path_length` is the NUMBER of forward actions times `forward_step`: the
    reference counts actions, not displacement (eval_actions.py:103-105)."""

    def __init__(self, nav, position_xz, heading_steps=0, turn_angle=10.0, tilt_angle=15.0, forward_step=0.065, sensor_height=1.25):
        if not isinstance(nav, NavGrid):
            raise TypeError(f"nav must be a NavGrid, got {type(nav).__name__}")
        self.nav = nav
        self.turn_angle, self.tilt_angle = _finite(turn_angle, "turn_angle"), _finite(tilt_angle, "tilt_angle")
        self.forward_step, self.sensor_height = _finite(forward_step, "forward_step"), _finite(sensor_height, "sensor_height")
        if self.forward_step <= 0.0:
            raise ValueError(f"forward_step must be positive, got {forward_step}")
        self.x, self.z = (_finite(v, "position_xz") for v in position_xz)
        if not nav.is_free(self.x, self.z):
            raise ValueError(f"the start position {(self.x, self.z)} (cell {nav.cell_of(self.x, self.z)}) is not free")
        self.heading_steps, self.pitch_steps = int(heading_steps), 0
        self.actions, self.forward_count = [], 0
        self.substeps = max(1, int(math.ceil(self.forward_step / (nav.cell / 4.0))))

    @property
    def yaw(self):
        return math.radians((self.heading_steps * self.turn_angle) % 360.0)

    @property
    def pitch(self):
        return math.radians((self.pitch_steps * self.tilt_angle) % 360.0)

    @property
    def forward(self):
        """f, the unit (x, z) direction a forward step takes"""
        yaw = self.yaw
        return np.array([-math.sin(yaw), -math.cos(yaw)])

    @property
    def position(self):
        """the sensor's world position (x, floor_y + sensor_height, z)"""
        return np.array([self.x, self.nav.floor_y + self.sensor_height, self.z])

    @property
    def X_WV(self):
        c, s = math.cos(self.yaw), math.sin(self.yaw)
        cp, sp = math.cos(self.pitch), math.sin(self.pitch)
        X = np.eye(4)
        X[:3, :3] = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
        X[:3, 3] = self.position
        return X

    @property
    def path_length(self):
        return self.forward_count * self.forward_step

    def step(self, action):
        """one action -> True, or False for a forward step that was cut short (a collision)"""
        action = int(action)
        if action not in ACTIONS:
            raise ValueError(f"unknown action {action} (0 stop, 1 move_forward, 2 turn_left, 3 turn_right, 4 look_up, 5 look_down)")
        done = True
        if action == MOVE_FORWARD:
            f, n = self.forward, self.substeps
            x, z = self.x, self.z
            for i in range(1, n + 1):
                cx, cz = self.x + (i / n) * self.forward_step * f[0], self.z + (i / n) * self.forward_step * f[1]
                if not self.nav.is_free(cx, cz):
                    done = False
                    break
                x, z = cx, cz
            self.x, self.z = x, z
            self.forward_count += 1
        elif action == TURN_LEFT:
            self.heading_steps += 1
        elif action == TURN_RIGHT:
            self.heading_steps -= 1
        elif action == LOOK_UP:
            self.pitch_steps += 1
        elif action == LOOK_DOWN:
            self.pitch_steps -= 1
        self.actions.append(action)
        return done


def save_actions(path, actions):
    """the reference's actions.txt: one integer per line (dataloader.py:262-263)"""
    with open(path, "w") as f:
        for a in actions:
            f.write(f"{int(a)}\n")


def load_actions(path):
    with open(path) as f:
        return [int(line) for line in f.read().split()]


def replay(agent, actions):
    """apply `actions` to `agent` in order -> the list of `step` results"""
    return [agent.step(a) for a in actions]


@torch.no_grad()
def judge_actions(scene, sensor, agent, actions, samples):
    """The reference's offline judge (eval_actions.py:96-150) without a simulator: one frame at the agent's start pose (the reference's initial
    "stop"), then for every action: step, frame.  Each frame is `sensor.frame(agent.X_WV)` (`sensor` a `MeshSensor` on `scene`), folded into a
    `judge.CompletionJudge` over `samples` ([N, 3] float32 on the scene's device, in the SIMULATOR'S world, e.g. `sample_surface(scene, n)`) with
    the path length at that moment.  -> rows [len(actions) + 1, 6] float64 on the host (`judge.COLUMNS`), read back once."""
    from . import judge as J
    if sensor.scene is not scene:
        raise ValueError("sensor must look at `scene`")
    cj = J.CompletionJudge(samples, device=scene.device)

    def look():
        _, depth = sensor.frame(agent.X_WV)
        cj.add_frame(depth, sensor.k4, np.linalg.inv(sensor.w2c(agent.X_WV)), agent.path_length)
    look()
    for a in actions:
        agent.step(a)
        look()
    return cj.rows()
