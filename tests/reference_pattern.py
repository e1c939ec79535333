"""TEST INFRASTRUCTURE: the reference's step-by-step call patterns, kept ONLY as the comparison baseline of the fused product paths.

* densify_stepwise / prune_stepwise: clone -> cat -> split -> cat -> remove -> cull -> remove on the product's own surgery primitives
  (optim.build_index / gather_rows / cat_params_to_optimizer / remove_points), the order of src/mapper/splatam/utils/slam_external.py:171-247 --
  what the fused event (optim.densify / prune_gaussians: one classification, one index, one gather per tensor) must reproduce row for row.
* remove_points_torch / prune_torch / densify_torch: the same events (slam_external.py:143-247) restated in PURE torch -- boolean indexing and
  torch.cat on plain tensor dicts of parameters, both Adam moments and the four statistics, no call into the library -- the independent
  reference of tests/mapstep_cases.py (densify_stepwise shares build_index / gather_rows with the product and cannot see their faults).
* keyframe_overlap_torch: the per-keyframe scoring loop of utils/keyframe_selection.py:62-86 in torch ops, against gs_keyframe_overlap.

Nothing under activesplat_amd/ imports this module."""
import torch

from activesplat_amd import optim as O
from activesplat_amd.mapping import build_rotation


def _too_big(params, variables, factor):
    return torch.exp(params["log_scales"]).max(dim=1).values > factor * variables["scene_radius"]


def prune_stepwise(params, variables, optimizer, iter, prune_dict):
    if iter > prune_dict["stop_after"]:
        return params, variables
    if iter >= prune_dict["start_after"] and iter % prune_dict["prune_every"] == 0:
        thr = prune_dict["final_removal_opacity_threshold"] if iter == prune_dict["stop_after"] else prune_dict["removal_opacity_threshold"]
        gone = (torch.sigmoid(params["logit_opacities"]) < thr).squeeze(-1)
        if iter >= prune_dict["remove_big_after"]:
            gone = gone | _too_big(params, variables, 0.1)
        params, variables = O.remove_points(gone, params, variables, optimizer)
    if iter > 0 and iter % prune_dict["reset_opacities_every"] == 0 and prune_dict["reset_opacities"]:
        params = O.update_params_and_optimizer({"logit_opacities": O.inverse_sigmoid(torch.ones_like(params["logit_opacities"]) * 0.01)}, params, optimizer)
    return params, variables


def densify_stepwise(params, variables, optimizer, iter, densify_dict, samples=None):
    """Same signature and results as optim.densify(..., samples=...); without `samples` the split offsets come from torch.normal."""
    if iter > densify_dict["stop_after"]:
        return params, variables
    variables = O.accumulate_mean2d_gradient(variables)
    if iter >= densify_dict["start_after"] and iter % densify_dict["densify_every"] == 0:
        names = [k for k in params if k not in O._SKIP]
        dev = params["means3D"].device
        thresh, n_into = densify_dict["grad_thresh"], densify_dict["num_to_split_into"]
        score = variables["means2D_gradient_accum"] / variables["denom"]
        score[score.isnan()] = 0.0
        limit = 0.01 * variables["scene_radius"]
        # 1. clone the small ones that moved: rows appended behind the originals
        clones = O.build_index((score >= thresh) & (torch.exp(params["log_scales"]).max(dim=1).values <= limit))
        ts = variables.get("timestep")
        if ts is not None:
            ts = torch.cat((ts, O.gather_rows(ts, clones)))
        params = O.cat_params_to_optimizer({k: O.gather_rows(params[k], clones) for k in names}, params, optimizer)
        # 2. split the large ones (clones carry no score): n_into children each, offset by N(0, scale) in the parent's frame, scale / (0.8 n)
        total = params["means3D"].shape[0]
        score_all = torch.zeros(total, device=dev)
        score_all[: score.shape[0]] = score
        parents_mask = (score_all >= thresh) & (torch.exp(params["log_scales"]).max(dim=1).values > limit)
        parents = O.build_index(parents_mask).repeat(n_into)
        kids = {k: O.gather_rows(params[k], parents) for k in names}
        sigma = torch.exp(kids["log_scales"])
        sigma = sigma.repeat(1, 3) if sigma.shape[1] == 1 else sigma
        if samples is None:
            samples = torch.normal(mean=torch.zeros_like(sigma), std=sigma)
        kids["means3D"] = kids["means3D"] + (build_rotation(kids["unnorm_rotations"]) * samples.to(dev).unsqueeze(1)).sum(dim=-1)
        kids["log_scales"] = torch.log(torch.exp(kids["log_scales"]) / (0.8 * n_into))
        if ts is not None:
            ts = torch.cat((ts, O.gather_rows(ts, parents)))
        params = O.cat_params_to_optimizer(kids, params, optimizer)
        total = params["means3D"].shape[0]
        for k in ("means2D_gradient_accum", "denom", "max_2D_radius"):
            variables[k] = torch.zeros(total, device=dev)
        if ts is not None:
            variables["timestep"] = ts
        # 3. the split parents leave; 4. faint and oversized Gaussians leave
        params, variables = O.remove_points(torch.cat((parents_mask, torch.zeros(parents.numel(), dtype=torch.bool, device=dev))), params, variables, optimizer)
        thr = densify_dict["final_removal_opacity_threshold"] if iter == densify_dict["stop_after"] else densify_dict["removal_opacity_threshold"]
        gone = (torch.sigmoid(params["logit_opacities"]) < thr).squeeze(-1)
        if iter >= densify_dict["remove_big_after"]:
            gone = gone | _too_big(params, variables, 0.1)
        params, variables = O.remove_points(gone, params, variables, optimizer)
    if iter > 0 and iter % densify_dict["reset_opacities_every"] == 0 and densify_dict.get("reset_opacities", False):
        params = O.update_params_and_optimizer({"logit_opacities": O.inverse_sigmoid(torch.ones_like(params["logit_opacities"]) * 0.01)}, params, optimizer)
    return params, variables


# ---- pure torch: no optimizer object, no library call.  params / exp_avg / exp_avg_sq: dicts name -> tensor; stats: dict of the four statistics ----
STATS = ("means2D_gradient_accum", "denom", "max_2D_radius", "timestep")


def _rotation_matrices(q):
    """[n,4] (w,x,y,z), normalised here -> [n,3,3] (slam_helpers.py:41-60)."""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def remove_points_torch(to_remove, params, exp_avg, exp_avg_sq, stats):
    keep = ~to_remove
    return ({k: v[keep] for k, v in params.items()}, {k: v[keep] for k, v in exp_avg.items()}, {k: v[keep] for k, v in exp_avg_sq.items()},
            {k: v[keep] for k, v in stats.items()})


def _cull_mask(params, scene_radius, thr, remove_big):
    gone = (torch.sigmoid(params["logit_opacities"]) < thr).squeeze(-1)
    if remove_big:
        gone = gone | (torch.exp(params["log_scales"]).max(dim=1).values > 0.1 * scene_radius)
    return gone


def prune_torch(params, exp_avg, exp_avg_sq, stats, scene_radius, thr, remove_big):
    """The removal half of prune_gaussians (slam_external.py:171-185) -> (params, exp_avg, exp_avg_sq, stats, fired)."""
    gone = _cull_mask(params, scene_radius, thr, remove_big)
    big = torch.exp(params["log_scales"]).max(dim=1).values > 0.1 * scene_radius
    faint = (torch.sigmoid(params["logit_opacities"]) < thr).squeeze(-1)
    fired = dict(opacity_cull=int(faint.sum()), too_big_cull=int((big & ~faint).sum()) if remove_big else 0)
    return remove_points_torch(gone, params, exp_avg, exp_avg_sq, stats) + (fired,)


def densify_torch(params, exp_avg, exp_avg_sq, stats, scene_radius, grad_thresh, n_into, thr, remove_big, samples):
    """The densify event (slam_external.py:204-243) on statistics that already hold this iteration's share: clone -> cat -> split -> cat ->
    the parents leave -> cull.  samples [n_into * split parents, 3]: the N(0, scale) offsets, indexed like the un-culled list of children
    (block c = child c of every split parent, parents ascending).  Appended rows start with zero moments and zero statistics, and inherit the
    parent's timestep (optim.py's module docstring: the reference leaves that case undefined).
    -> (params, exp_avg, exp_avg_sq, stats, fired); fired counts how often each branch decided."""
    n0 = params["means3D"].shape[0]
    dev = params["means3D"].device
    score = stats["means2D_gradient_accum"] / stats["denom"]
    undefined = score.isnan()
    score = torch.where(undefined, torch.zeros_like(score), score)
    limit = 0.01 * scene_radius
    smax = torch.exp(params["log_scales"]).max(dim=1).values
    hot = score >= grad_thresh
    to_clone, to_split = hot & (smax <= limit), hot & (smax > limit)

    def append(d, rows, zero):
        return {k: torch.cat((v, torch.zeros_like(rows[k]) if zero else rows[k]), dim=0) for k, v in d.items()}
    clones = {k: v[to_clone] for k, v in params.items()}
    ts = torch.cat((stats["timestep"], stats["timestep"][to_clone]))
    params, exp_avg, exp_avg_sq = append(params, clones, False), append(exp_avg, clones, True), append(exp_avg_sq, clones, True)
    n_clone = int(to_clone.sum())
    split_all = torch.cat((to_split, torch.zeros(n_clone, dtype=torch.bool, device=dev)))           # (clones carry no score: never split)
    kids = {k: v[split_all].repeat(n_into, 1) for k, v in params.items()}
    n_kids = kids["means3D"].shape[0]
    assert samples.shape[0] == n_kids
    f32, f64 = kids["means3D"].dtype, torch.float64              # (the children's values: formed in float64, rounded once)
    kids["means3D"] = (kids["means3D"].to(f64) + torch.bmm(_rotation_matrices(kids["unnorm_rotations"].to(f64)),
                                                           samples.to(dev).to(f64).unsqueeze(-1)).squeeze(-1)).to(f32)
    kids["log_scales"] = torch.log(torch.exp(kids["log_scales"].to(f64)) / (0.8 * n_into)).to(f32)
    ts = torch.cat((ts, ts[split_all].repeat(n_into)))
    params, exp_avg, exp_avg_sq = append(params, kids, False), append(exp_avg, kids, True), append(exp_avg_sq, kids, True)
    total = params["means3D"].shape[0]
    stats = {k: (ts if k == "timestep" else torch.zeros(total, dtype=v.dtype, device=dev)) for k, v in stats.items()}
    parents_gone = torch.cat((split_all, torch.zeros(n_kids, dtype=torch.bool, device=dev)))
    params, exp_avg, exp_avg_sq, stats = remove_points_torch(parents_gone, params, exp_avg, exp_avg_sq, stats)
    n_orig = n0 - int(to_split.sum())
    gone = _cull_mask(params, scene_radius, thr, remove_big)
    faint = (torch.sigmoid(params["logit_opacities"]) < thr).squeeze(-1)
    big = torch.exp(params["log_scales"]).max(dim=1).values > 0.1 * scene_radius
    fired = dict(clone=n_clone, split=int(to_split.sum()), undefined_score=int(undefined.sum()), opacity_cull=int(faint.sum()),
                 too_big_original=int((big & ~faint)[:n_orig].sum()) if remove_big else 0,
                 too_big_child=int((big & ~faint)[n_orig + n_clone:].sum()) if remove_big else 0,
                 rows_before_children=int((~gone)[:n_orig + n_clone].sum()))
    return remove_points_torch(gone, params, exp_avg, exp_avg_sq, stats) + (fired,)


def keyframe_overlap_torch(pts, keyframe_list, intrinsics, width, height, edge=20):
    """-> per keyframe: number of the world points `pts` [n,3] that project inside its image shrunk by `edge` pixels, at positive depth."""
    counts = []
    for kf in keyframe_list:
        w2c = kf["est_w2c"]
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        pix = cam @ intrinsics.T
        z = pix[:, 2:] + 1e-5
        u, v = (pix / z)[:, 0], (pix / z)[:, 1]
        counts.append(int(((u < width - edge) & (u > edge) & (v < height - edge) & (v > edge) & (z[:, 0] > 0)).sum()))
    return counts
