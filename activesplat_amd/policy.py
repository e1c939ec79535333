"""The reference's hierarchical target choice, restated on the grid roadmap: integer node scores built from flags
(scripts/nodes/planner_node.py:46-61, :1128-1215) and the stateful subregion policy that picks the next node (:249-463).

Host logic over K-sized arrays: the maps, the all-pairs distances and the clustering stay on the device (roadmap.node_distances,
roadmap.subregions, roadmap.nodes_in_horizon); what arrives here are a few K-sized copies, never a map.  Pixels are (r, c); lengths are
in pixels.  `plan` runs the stages in the reference's order on a Roadmap (`SplatMapper.plan_step(policy=...)` calls it).

Restated for the reference's INITIAL flag weights only.  NOT built, on purpose: the reweighting after every node has been visited and the
random choice that goes with it (:1150-1164, :453-457); escape plans (`get_escape_plan`) and the movement-failure handling; spline
interpolation of the chosen path; manual planning.  Where the reference runs a safe Dijkstra path from a candidate to the remembered far
target (:414-429) this takes the roadmap distance D / 12 between the two nodes.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import roadmap as RM

#: NODES_FLAGS_WEIGHT_INIT (planner_node.py:54-61); REAL_OPACITY_INVISIBILITY weighs the separate invisibility score
NODE_WEIGHTS = dict(unarrived=20, in_horizon=10, invisibility=2, volume=1, real_invisibility=1, fail=-60)


def _host(x, dtype=None):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x) if dtype is None else np.asarray(x, dtype=dtype)


def _scaled(values):
    """ceil(10 v / max v) as int32, the maximum by np.nanmax; a zero or NaN maximum (or no node) gives 0 instead of the reference's division
    warning; a NaN value gives 0"""
    values = _host(values, np.float64)
    if values.size == 0 or np.isnan(values).all():
        return np.zeros(values.shape, np.int32)
    top = np.nanmax(values)
    if not (top != 0.0 and math.isfinite(top)):
        return np.zeros(values.shape, np.int32)
    return np.nan_to_num(np.ceil(values / top * 10.0), nan=0.0).astype(np.int32)


def node_scores(invisibility, volume, unarrived, in_horizon, fail, weights=NODE_WEIGHTS):
    """planner_node.py:1201-1215 -> (score int32 [K], invisibility_score int32 [K]):
    score = 20 unarrived + 10 in_horizon + 2 ceil(10 inv / max inv) + 1 ceil(10 vol / max vol) - 60 fail, invisibility_score = ceil(inv).
    `invisibility`, `volume`: the two floats per node of `global_invisibility_scores`; the three flags: 0 / 1 per node
    (`SubregionPolicy.flags`, `roadmap.nodes_in_horizon`)."""
    inv = _host(invisibility, np.float64)
    flag = lambda x: _host(x).astype(np.int32).reshape(inv.shape)
    score = (weights["unarrived"] * flag(unarrived) + weights["in_horizon"] * flag(in_horizon) + weights["invisibility"] * _scaled(inv)
             + weights["volume"] * _scaled(volume).reshape(inv.shape) + weights["fail"] * flag(fail))
    return score.astype(np.int32), (weights["real_invisibility"] * np.nan_to_num(np.ceil(inv), nan=0.0)).astype(np.int32)


def _nearest(points, nodes):
    """the distance from each node [K, 2] to the nearest of `points` [n, 2]; +inf without points"""
    if len(points) == 0:
        return np.full(len(nodes), np.inf)
    d = nodes[:, None, :].astype(np.float64) - np.asarray(points, np.float64)[None, :, :]
    return np.sqrt((d * d).sum(-1)).min(1)


class SubregionPolicy:
    """The state the choice carries from one planning step to the next (planner_node.py): the visited agent positions
    (`__topdown_translation_array`), the selected positions (`__position_selected_vertices`: where the agent stood when it arrived at a
    target), the failed nodes (`__fail_vertices_nodes`) and `use_global_plan`.

    step_px: the agent's step in pixels; radius_px: its radius; arrived_steps: `__step_num_as_arrived` (config planner.step_num_as_arrived,
    1.5 in every dataset of the reference); visited_steps: `__step_num_as_visited` (10 or 15 there) -- None: the arrived radius serves both;
    too_far_steps: `__step_num_as_too_far`; subregion_threshold: the 250 of :277."""

    def __init__(self, step_px, radius_px, arrived_steps=1.5, too_far_steps=200, subregion_threshold=250, visited_steps=None):
        self.step_px, self.radius_px = float(step_px), float(radius_px)
        self.arrived_px = self.step_px * float(arrived_steps)
        self.visited_px = self.arrived_px if visited_steps is None else self.step_px * float(visited_steps)
        self.too_far_px = float(too_far_steps) * self.step_px
        self.subregion_threshold = subregion_threshold
        self.visited = np.zeros((0, 2), np.float64)
        self.selected = np.zeros((0, 2), np.float64)
        self.failed = np.zeros((0, 2), np.float64)
        self.use_global_plan = False
        self.last = {}

    def visit(self, rc):
        """the agent stands at pixel `rc`"""
        self.visited = np.vstack([self.visited, np.asarray(rc, np.float64).reshape(1, 2)])

    def arrive(self, rc):
        """the agent has arrived at a chosen target and stands at `rc`"""
        self.selected = np.vstack([self.selected, np.asarray(rc, np.float64).reshape(1, 2)])

    def fail(self, rc):
        """no path to the node at `rc` could be found"""
        self.failed = np.vstack([self.failed, np.asarray(rc, np.float64).reshape(1, 2)])

    def flags(self, node_rc):
        """-> (unarrived, fail) int32 [K]: farther than visited_px from every visited position; within radius_px of a failed node"""
        nodes = _host(node_rc, np.float64).reshape(-1, 2)
        return (_nearest(self.visited, nodes) > self.visited_px).astype(np.int32), (_nearest(self.failed, nodes) <= self.radius_px).astype(np.int32)

    def choose(self, rm, D_labels, scores, invisibility_scores, path_length_px):
        """planner_node.py:262-463 for the initial weights -> the node's index, or -1 (and `use_global_plan` is raised for the next call).
        rm: the Roadmap (its `agent_rc` and `node_rc`); D_labels: the pair (D [K, K] of `node_distances`, labels [K] of `subregions`);
        scores, invisibility_scores: `node_scores`'; path_length_px [K]: the length of the way from the agent to each node, NaN where there
        is none.  What was decided is left in `self.last` (plan, current and chosen subregion, candidates, far)."""
        D, labels = D_labels
        D, labels = _host(D, np.int64), _host(labels, np.int64)
        scores, inv = _host(scores, np.int64).copy(), _host(invisibility_scores, np.int64).copy()
        length = _host(path_length_px, np.float64)
        nodes = _host(rm.node_rc, np.float64).reshape(-1, 2)
        K = len(nodes)
        self.last = dict(plan=None, current=-1, subregion=-1, candidates=np.zeros(0, np.int64), far=-1)
        if K == 0:
            self.use_global_plan = True
            return -1
        agent = np.asarray(rm.agent_rc, np.float64)
        to_agent = np.sqrt(((nodes - agent) ** 2).sum(1))
        current = int(labels[int(np.argmin(to_agent))])
        member = labels == current
        # the current subregion: a node near a selected position scores 0 and counts as arrived; a score <= 0 takes the invisibility score away
        arrived = member & (_nearest(self.selected, nodes) < self.visited_px)
        local_scores = scores.copy()
        local_scores[arrived] = 0
        inv[member & (local_scores <= 0)] = 0
        go_global = bool(arrived[member].all()) or int(inv[member].max()) < self.subregion_threshold
        if self.use_global_plan or go_global:
            self.use_global_plan = False
            # the subregion with the best node outside the current one, not arrived, reachable; labels are numbered by their smallest member,
            # so label order is the reference's dictionary order and np.argmax takes its first maximum
            counted = ~member & ~(_nearest(self.selected, nodes) < self.arrived_px) & ~np.isnan(length)
            best = np.zeros(int(labels.max()) + 1, np.int64)
            np.maximum.at(best, labels[counted], np.maximum(scores[counted], 0))
            chosen = int(np.argmax(best))
            candidates, cand_scores, plan = np.flatnonzero(labels == chosen), scores, "global"
        else:
            chosen, candidates, cand_scores, plan = current, np.flatnonzero(member), local_scores, "local"
        self.last.update(plan=plan, current=current, subregion=chosen, candidates=candidates)
        length = np.where(to_agent < self.arrived_px, np.nan, length)       # (:372: nodes the agent stands on are skipped)
        far, level_scores = -1, cand_scores[candidates]
        for level in range(int(level_scores.max()), int(level_scores.min()) - 1, -1):
            at = candidates[level_scores == level]
            if len(at) == 0 or np.isnan(length[at]).all():
                continue
            if far >= 0:
                near = at[length[at] < self.too_far_px]                      # (NaN compares false)
                if len(near) == 0:
                    continue
                to_far = np.where(D[near, far] >= 2 ** 31 - 1, np.nan, D[near, far] / 12.0)
                if not (to_far < length[far]).any():
                    continue
                return int(near[int(np.nanargmin(to_far))])
            k = int(at[int(np.nanargmin(length[at]))])
            if length[k] > self.too_far_px:
                far = k
                self.last["far"] = far
                continue
            return k
        if far < 0:
            self.use_global_plan = True
        return far


@torch.no_grad()
def plan(rm, policy, invisibility_scores, px_per_m, radius_px):
    """One choice on a Roadmap with nodes, in the reference's order: `node_distances` -> `subregions` -> `nodes_in_horizon` ->
    `invisibility_scores()` (a callable -> the (invisibility [K], volume [K]) of `global_invisibility_scores`) -> `node_scores` ->
    `policy.choose` -> `path_to` -> `shortcut_path`.  The agent's pixel is recorded as visited.  The way to a node is measured along the
    roadmap (`node_path_length` / 12 pixels; every node of a Roadmap is reachable).  One K-sized copy of the labels, the horizon flags and
    the path lengths, then the copies `path_to` and `shortcut_path` make.
    -> dict(invisibility, volume, subregions int32 [K] (host), scores int32 [K] (host), distances (D, device), node (-1: none), path_rc,
    shortcut_rc, safe (device))"""
    K, dev = rm.K, rm.node_rc.device
    policy.visit(rm.agent_rc)
    D = RM.node_distances(rm)
    labels, _, _ = RM.subregions(rm, D, px_per_m)
    horizon = RM.nodes_in_horizon(rm)
    inv, vol = invisibility_scores()
    small = torch.cat([labels.to(torch.int64), horizon.to(torch.int64), rm.node_path_length()]).cpu().numpy()
    labels_h, horizon_h, length = small[:K].astype(np.int32), small[K:2 * K], small[2 * K:] / 12.0
    unarrived, fail = policy.flags(rm.node_rc)
    scores, inv_scores = node_scores(inv, vol, unarrived, horizon_h, fail)
    node = policy.choose(rm, (D, labels_h), scores, inv_scores, length)
    empty = torch.zeros(0, 2, dtype=torch.int32, device=dev)
    out = dict(invisibility=inv, volume=vol, subregions=labels_h, scores=scores, distances=D, node=node, path_rc=empty, shortcut_rc=empty,
               safe=torch.zeros((), dtype=torch.uint8, device=dev))
    if node >= 0:
        path = rm.path_to(node)
        short, _, safe = RM.shortcut_path(rm, path, radius_px)
        out.update(path_rc=path, shortcut_rc=short, safe=safe)
    return out
