"""The planner's top-down map camera on the HIP path (GPU box): src/visualizer/visualizer.py:923-937 renders the map TWICE per GUI tick through a
camera 1000 m up (:1577-1601) with scale_modifier 0.01 -- the height-cut "free map" with opacity colours and the visible map -- both
forward-only.  Second part ("one_tick_from_parameters"): one tick = both boolean maps from the map's PARAMETERS, (a) the composition a port of
visualizer.py:923-965 makes on this library -- clone, cut_gaussian_by_height, torch activations, two renders, byte / grey / threshold in torch
on the device -- against (b) topdown.topdown_maps, one fused pass: five alternating repeats of 60 ticks between device events each, medians
and spread, and the raster stages of both.  (Every kernel (a) launches is instruction-for-instruction the parent commit's.)  Prints JSON: per-render and per-tick milliseconds, per-stage hipEvent averages, and the blend forward with the few-tile
(producer / consumer) kernel forced on for this 437 / 529-tile view against the plain streams kernel (which the 257..768-tile band uses)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import GaussianRasterizer, _lib, rasterizer as R  # noqa: E402
from tests import parity_cases as pc  # noqa: E402

dev = torch.device("cuda")
N = int(os.environ.get("N", 1_000_000))
lib = _lib.get()
out = {"gaussians": N}
for W, H in ((360, 300), (368, 368)):
    rs, rv = pc.topdown_scene(N, dev, W=W, H=H)
    rs = rs._replace(debug=False)
    white = rs._replace(bg=torch.ones(3, device=dev))
    m2d = torch.zeros(N, 3, device=dev)
    # the free map: Gaussians between the agent's foot and head (here: half of them), coloured by opacity (GaussianColorType.Opacity)
    keep = rv["means3D"][:, 1] > -0.7
    free = {k: v[keep].contiguous() for k, v in rv.items()}
    free["colors_precomp"] = free["opacities"].expand(-1, 3).contiguous()
    m2f = torch.zeros(free["means3D"].shape[0], 3, device=dev)

    def tick():
        with torch.no_grad():
            GaussianRasterizer(raster_settings=rs)(means2D=m2f, **free)
            GaussianRasterizer(raster_settings=white)(means2D=m2d, **rv)

    def one():
        with torch.no_grad():
            return GaussianRasterizer(raster_settings=white)(means2D=m2d, **rv)

    def bench(fn, n=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    res = {"tiles": ((W + 15) // 16) * ((H + 15) // 16)}
    res["visible_map_ms"] = round(bench(one), 4)
    res["tick_two_renders_ms"] = round(bench(tick), 4)
    col, radii, depth, op = one()
    res["D"] = int(R.last_stats["num_rendered"]); res["max_tile_list"] = int(R.last_stats["max_tile_instances"])
    res["visible"] = int((radii > 0).sum()); res["radii_values"] = sorted(int(v) for v in torch.unique(radii).tolist())
    res["opacity_mean"] = round(float(op.mean()), 4)
    for name, knob in (("plain_streams_kernel", 256), ("few_tile_pc_kernel_forced", 4096)):
        _lib.check(lib.gs_set_half_quadrants(knob))
        try:
            lib.gs_profile_enable(1)
            for _ in range(20):
                one()
            torch.cuda.synchronize()
            res["stages_us_" + name] = {k: round(ms / c * 1e3, 1) for k, (ms, c) in _lib.profile_collect().items() if c}
            lib.gs_profile_enable(0)
            res["ms_" + name] = round(bench(one), 4)
            c2 = one()[0]
            res["same_image_" + name] = bool(torch.equal(c2, col))
        finally:
            _lib.check(lib.gs_set_half_quadrants(256))
    out[f"{W}x{H}"] = res


def one_tick_from_parameters(W, H, reps=5, ticks=60):
    import statistics
    import torch.nn.functional as F
    from activesplat_amd import io as IO, topdown as TD
    from tests import topdown_cases as tc
    params = tc.scene_params(N, W, H, dev)
    upper, lower = tc.BAND
    cam = TD.topdown_camera(tc.CENTRE, tc.EXTENT, (W, H), device=dev)
    black = cam._replace(bg=torch.zeros(3, device=dev))
    m2d = torch.zeros(N, 3, device=dev)

    def activate(p):
        ls = p["log_scales"]
        return dict(means3D=p["means3D"], colors_precomp=p["rgb_colors"], rotations=F.normalize(p["unnorm_rotations"]),
                    opacities=torch.sigmoid(p["logit_opacities"]), scales=torch.exp(torch.tile(ls, (1, 3)) if ls.shape[1] == 1 else ls))

    def tick_a():
        with torch.no_grad():
            p = IO.cut_gaussian_by_height({k: v.clone() for k, v in params.items()}, upper, lower)
            free = activate(p)
            opacity = GaussianRasterizer(raster_settings=black)(means2D=torch.zeros_like(free["means3D"]), **free)[3]
            color = GaussianRasterizer(raster_settings=cam)(means2D=m2d, **activate(params))[0]
            free_bin = (opacity[0] <= 0.4).to(torch.uint8)
            rgb = (color.clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(1, 2, 0).contiguous()
            return opacity[0], free_bin, rgb, (TD.rgb_to_grey_u8(rgb) == 255).to(torch.uint8)

    def tick_b():
        return TD.topdown_maps(params, cam, upper, lower)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ticks):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ticks

    for fn in (tick_a, tick_b):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):                                  # alternating: both see the same neighbours on a shared host
        ta.append(window(tick_a)); tb.append(window(tick_b))
    res = {"composition_ms": [round(t, 4) for t in ta], "fused_ms": [round(t, 4) for t in tb],
           "composition_median_ms": round(statistics.median(ta), 4), "composition_spread_ms": round(max(ta) - min(ta), 4),
           "fused_median_ms": round(statistics.median(tb), 4), "fused_spread_ms": round(max(tb) - min(tb), 4)}
    res["fused_wins_by_more_than_the_spread"] = bool(statistics.median(ta) - statistics.median(tb) > max(ta) - min(ta))
    for name, fn in (("composition", tick_a), ("fused", tick_b)):
        lib.gs_profile_enable(1)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        st = {k: (ms, c) for k, (ms, c) in _lib.profile_collect().items() if c}
        lib.gs_profile_enable(0)
        res["stages_us_per_tick_" + name] = {k: round(ms / 20 * 1e3, 1) for k, (ms, c) in st.items()}
        res["raster_us_per_tick_" + name] = round(sum(ms for ms, _ in st.values()) / 20 * 1e3, 1)
    a, b = tick_a(), tick_b()
    res["differing_pixels_composition_vs_fused"] = [int((x != y).reshape(H * W, -1).any(1).sum()) for x, y in zip(a, b)]
    return res


out["one_tick_from_parameters"] = {f"{W}x{H}": one_tick_from_parameters(W, H) for W, H in ((360, 300), (368, 368))}
print(json.dumps(out))
