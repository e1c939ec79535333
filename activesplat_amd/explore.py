"""The episode loop: sense -> map -> plan -> act -> judge, closed over the mesh sensor, the mapper, the planner and the simulated agent.

It mirrors the control flow of the reference's planner node (scripts/nodes/planner_node.py) on this package's stages:

* bootstrap    ceil(360 / turn_angle) turn_left actions (:176-183); the frame after every action goes through `SplatMapper.run_sensor`.  The
               reference's up / down looks, interleaved with those turns (:194-230), are left out.  A level sensor 1.25 m above the floor never
               sees the floor under the agent, and `plan_step` finds no node while the agent's own pixel has not been seen; so
               `look_down_steps = n > 0` (off by default) adds n look_down actions, a second circle and n look_up actions -- a plain
               stand-in for those looks, not a restatement of them;
* plan         `SplatMapper.plan_step(view_c2w, **plan, policy=policy)`; no node (node < 0) ends the episode;
* follow       the rule of :696-699 and :758-771: waypoints up to the last one within one step are dropped; the agent turns towards the next
               waypoint while the heading error exceeds `turn_angle`, else moves forward while the waypoint is farther than one step;
* arrive       within `arrived_steps` x forward_step (1.5 steps, :969) of the last waypoint: a full turn (the look-around), `policy.arrive`, replan;
* collide      a forward action that was cut short: `policy.fail` of the chosen node, replan.

NOT built: escape plans, the line test in front of every step, spline smoothing, the reweighting after exhaustion, the high-connectivity and
rotation-selection branches, periodic replanning while under way.

FRAMES.  The simulator's world has y up (`agent.SimAgent.X_WV`); the mapper's world is the FIRST sensor frame in the camera convention x right,
y down, z forward: p_mapper = sensor.w2c(X0) p_sim (`sim_to_mapper`), the matrix tests/mesh_cases.py uses to carry the judge's samples over.
The planner's top-down maps look along the mapper's +y, so the first pose must be level (asserted).  Waypoints come back through the inverse
(`mapper_to_sim`).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import agent as AG
from . import frames as FR
from . import roadmap as RM


def sim_to_mapper(sensor, X0):
    """4x4: the simulator's world -> the mapper's world, for the first sensor pose X0"""
    return np.asarray(sensor.w2c(X0), dtype=np.float64)


def mapper_to_sim(sensor, X0):
    """4x4: the mapper's world -> the simulator's world"""
    return np.linalg.inv(sim_to_mapper(sensor, X0))


def points_to_sim(sensor, X0, points):
    """points [n, 3] of the mapper's world (array or tensor) -> float64 [n, 3] in the simulator's world, on the host"""
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    m = mapper_to_sim(sensor, X0)
    return p @ m[:3, :3].T + m[:3, 3]


def view_c2w(sensor, X0, X):
    """the camera-to-world matrix, in the mapper's world, of the sensor at pose X (x right, y down, z forward): what `plan_step` takes"""
    return sim_to_mapper(sensor, X0) @ np.linalg.inv(np.asarray(sensor.w2c(X), dtype=np.float64))


def quat_wxyz(rot):
    """(w, x, y, z) of a rotation matrix, w >= 0, from the largest of the four candidates (safe for every angle)"""
    m = np.asarray(rot, dtype=np.float64)
    cand = np.array([1.0 + m[0, 0] + m[1, 1] + m[2, 2], 1.0 + m[0, 0] - m[1, 1] - m[2, 2], 1.0 - m[0, 0] + m[1, 1] - m[2, 2],
                     1.0 - m[0, 0] - m[1, 1] + m[2, 2]])
    k = int(np.argmax(cand))
    s = 2.0 * math.sqrt(max(cand[k], 0.0))
    if k == 0:
        q = np.array([0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s])
    elif k == 1:
        q = np.array([(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s])
    elif k == 2:
        q = np.array([(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s])
    else:
        q = np.array([(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s])
    return (q if q[0] >= 0.0 else -q).astype(np.float32)


class Explorer:
    """One episode of `agent` (an `agent.SimAgent`, at its start pose, level) seen through `sensor` (a `sensor.MeshSensor`) and mapped by `mapper`
    (a `SplatMapper` whose cfg["step_num"] exceeds the number of frames: one per action, and one at the start).
    plan: the keyword arguments of `SplatMapper.plan_step` after the view -- world_center, world_shape, grid_shape, upper, lower, agent_radius,
    node_spacing (and, if wanted, height, scale_modifier, max_clusters) -- in the MAPPER'S world.  policy: a `policy.SubregionPolicy` or None
    (the greedy choice).  bootstrap_turns: None for the full circle, ceil(360 / turn_angle).  look_down_steps: see the module's text."""

    def __init__(self, mapper, sensor, agent, plan, policy=None, bootstrap_turns=None, arrived_steps=1.5, look_down_steps=0):
        if not isinstance(agent, AG.SimAgent):
            raise TypeError(f"agent must be a SimAgent, got {type(agent).__name__}")
        if agent.pitch_steps != 0:
            raise ValueError("the first pose must be level: the planner's maps look along the first camera's y axis")
        self.mapper, self.sensor, self.agent, self.plan, self.policy = mapper, sensor, agent, dict(plan), policy
        self.full_turn = int(math.ceil(360.0 / agent.turn_angle))
        self.bootstrap_turns = self.full_turn if bootstrap_turns is None else int(bootstrap_turns)
        self.look_down_steps = int(look_down_steps)
        self.arrived = float(arrived_steps) * agent.forward_step
        self.X0 = agent.X_WV
        assert abs(self.X0[1, 1] - 1.0) < 1e-12, "the first pose must be level"
        self._first = None
        self.frame_id = 0
        self.positions, self.results = [], []
        self.plans = self.arrivals = self.collisions = 0
        self.nodes = []

    @property
    def bootstrap_actions(self):
        """the number of actions the bootstrap takes"""
        return self.bootstrap_turns * (2 if self.look_down_steps > 0 else 1) + 2 * max(self.look_down_steps, 0)

    # -- frames ---------------------------------------------------------------------------------------------------------------------------
    def agent_rc(self):
        """the planner's pixel (r, c) that shows the agent"""
        p = sim_to_mapper(self.sensor, self.X0) @ np.append(self.agent.position, 1.0)
        world = {k: self.plan[k] for k in ("world_center", "world_shape", "grid_shape")}
        return np.rint(RM.world_to_pixel((p[0], p[2]), height=float(self.plan.get("height", 1000.0)), **world)).astype(np.int64)

    def _sense(self):
        X = self.agent.X_WV
        gt_w2c, self._first = FR.gt_w2c_from_pose(X, self._first)
        self.mapper.run_sensor(self.sensor, X, self.frame_id, quat_wxyz(gt_w2c[:3, :3]), gt_w2c[:3, 3])
        self.frame_id += 1
        self.positions.append((self.agent.x, self.agent.z))

    def _act(self, action):
        done = self.agent.step(action)
        self.results.append(done)
        self._sense()
        if self.policy is not None:
            self.policy.visit(self.agent_rc())
        return done

    def _turn_round(self, turns, budget):
        for _ in range(turns):
            if len(self.agent.actions) >= budget:
                return
            self._act(AG.TURN_LEFT)

    # -- the loop -------------------------------------------------------------------------------------------------------------------------
    def _plan(self):
        view = torch.tensor(view_c2w(self.sensor, self.X0, self.agent.X_WV), dtype=torch.float32)
        out = self.mapper.plan_step(view, policy=self.policy, **self.plan)
        self.plans += 1
        self.nodes.append(int(out["node"]))
        if out["node"] < 0:
            return None, None
        way = points_to_sim(self.sensor, self.X0, out["waypoints"])[:, [0, 2]]
        node_rc = out["roadmap"].node_rc[int(out["node"])].cpu().numpy()
        return way, node_rc

    def heading_error(self, target_xz):
        """degrees in (-180, 180] by which the yaw has to grow (turn_left) for the agent to face `target_xz`"""
        dx, dz = float(target_xz[0]) - self.agent.x, float(target_xz[1]) - self.agent.z
        want = math.degrees(math.atan2(-dx, -dz))                              # f = (-sin yaw, -cos yaw)
        have = (self.agent.heading_steps * self.agent.turn_angle) % 360.0
        return (want - have + 180.0) % 360.0 - 180.0

    def run(self, max_actions):
        """-> dict(actions, positions float64 [len(actions) + 1, 2] (simulator x, z; the start first), completed (one bool per action), plans,
        nodes (the node of every plan), arrivals, collisions, judge (the rows of `mapper.judge`, one per frame, or None)).  `max_actions` counts every action,
        the bootstrap's included."""
        budget = int(max_actions)
        agent, step = self.agent, self.agent.forward_step
        if self.frame_id == 0:
            self._sense()
            if self.policy is not None:
                self.policy.visit(self.agent_rc())
            self._turn_round(self.bootstrap_turns, budget)
            if self.look_down_steps > 0:
                for action, count in ((AG.LOOK_DOWN, self.look_down_steps), (AG.TURN_LEFT, self.bootstrap_turns), (AG.LOOK_UP, self.look_down_steps)):
                    for _ in range(count):
                        if len(agent.actions) < budget:
                            self._act(action)
        way = node_rc = None
        while len(agent.actions) < budget:
            if way is None:
                way, node_rc = self._plan()
                if way is None:
                    break
            here = np.array([agent.x, agent.z])
            if len(way) == 0 or np.linalg.norm(way[-1] - here) <= self.arrived:
                self.arrivals += 1
                self._turn_round(self.full_turn, budget)
                if self.policy is not None:
                    self.policy.arrive(self.agent_rc())
                way = None
                continue
            near = np.nonzero(np.linalg.norm(way - here, axis=1) <= step)[0]
            if len(near):
                way = way[int(near[-1]) + 1:]
            if len(way) == 0:
                continue                                                        # (the arrival test above takes it from here)
            err = self.heading_error(way[0])
            if err > agent.turn_angle:
                self._act(AG.TURN_LEFT)
            elif err < -agent.turn_angle:
                self._act(AG.TURN_RIGHT)
            elif not self._act(AG.MOVE_FORWARD):
                self.collisions += 1
                if self.policy is not None:
                    self.policy.fail(node_rc)
                way = None
        judge = getattr(self.mapper, "judge", None)
        return dict(actions=list(agent.actions), positions=np.asarray(self.positions, dtype=np.float64).reshape(-1, 2), completed=list(self.results),
                    plans=self.plans, nodes=list(self.nodes), arrivals=self.arrivals, collisions=self.collisions,
                    judge=judge.rows() if judge is not None else None)
