"""ignore_outlier_depth_loss on the fused paths, timed on two frame sizes -- 256 x 256 with 200 k Gaussians and 640 x 480 with 500 k.  GPU box.

    python scripts/outlier_times.py            -> profiles/outlier_loss.txt

The driver starts one child process per (size, section), each under a time limit of its own, and stops at the first child that fails or runs
out of time (nothing more is started on the device after that).  Inside a child the variants of a section are timed ALTERNATELY: ROUNDS rounds,
in each round one block per variant; a block is as many calls as fill about WINDOW seconds (calibrated per variant after WARM untimed calls),
wall clock around the block, which ends in a device synchronise.  One JSON line per variant: median, minimum and maximum of its blocks, ms per
call.  All learning rates are zero, so the poses and the map -- and with them the work per call -- stay what they are from block to block.

    median     gs_depth_error_median alone at a grid of G workgroups per pass (G = 1: a single workgroup; `chosen`: the library's G(n)).
               One call = a memset, three histogram passes and the pick
    tracking   one tracking iteration: mapping.tracking_iteration with the option off and on, and the only route the option had before:
               mapping.track_frame(fused=False) with the option (TRACK_ITERS iterations per call, reported per iteration)
    mapping    one mapping iteration: mapping.mapping_iteration with the option off and on, and the route the option had before:
               get_loss(fused=True, fused_preprocess=True, ignore_outlier_depth_loss=True) with the torch loss, backward, optimizer.step()
    growth     mapping.grow_rows (gs_grow_gaussians: the same select, mask, compaction, rows, and the call's one host read of the counts) on a
               frame of that size, no map.  Timed call by call with device events (timed_by_events); a block's figure is the median of its calls
"""
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((200_000, 256, 256), (500_000, 640, 480))
SECTIONS = ("median", "tracking", "mapping", "growth")
GROWTH_CALLS = 200                                 # event-timed calls per block of the growth section
GRIDS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
CHILD_LIMIT = 420                                  # seconds per child
WINDOW, ROUNDS, WARM = float(os.environ.get("WINDOW", 0.3)), int(os.environ.get("ROUNDS", 5)), int(os.environ.get("WARM", 5))
TRACK_ITERS = 50                                   # iterations of one track_frame(fused=False) call
ZERO_LRS = dict(means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0, logit_opacities=0.0, log_scales=0.0, cam_unnorm_rots=0.0, cam_trans=0.0)


def timed_alternately(variants, per_call=None):
    """variants: {name: step}.  -> {name: dict(ms_median, ms_min, ms_max, calls_per_block, blocks)}; per_call[name]: iterations inside one call."""
    import torch
    per_call = per_call or {}
    calls = {}
    for name, step in variants.items():
        for _ in range(WARM):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        calls[name] = max(3, min(20000, int(math.ceil(WINDOW / max((time.perf_counter() - t0) / 3, 1e-7)))))
    ts = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, step in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                step()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) / (calls[name] * per_call.get(name, 1)) * 1e3)
    return {name: dict(ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), calls_per_block=calls[name],
                       blocks=len(v)) for name, v in ts.items()}


def timed_by_events(variants, calls=GROWTH_CALLS):
    """As timed_alternately, for calls that end in a host read: a pair of device events around every call, a block = the median of `calls`."""
    import torch
    for step in variants.values():
        for _ in range(WARM):
            step()
    ts = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, step in variants.items():
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
            for a, b in pairs:
                a.record()
                step()
                b.record()
            torch.cuda.synchronize()
            ts[name].append(statistics.median(a.elapsed_time(b) for a, b in pairs))
    return {name: dict(ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), calls_per_block=calls,
                       blocks=len(v)) for name, v in ts.items()}


def growth_step(W, H):
    """-> a call of mapping.grow_rows on depth_pair's frame: a silhouette with ~9 % below the threshold, a camera at the origin."""
    import numpy as np
    import torch
    from activesplat_amd import mapping as M
    from activesplat_amd import synthetic as syn
    g = torch.Generator().manual_seed(5)
    d, gt = [x[0].cuda() for x in depth_pair(H, W)]
    sil = (1.0 - 0.6 * torch.rand(H, W, generator=g) ** 2).cuda()
    color = torch.rand(3, H, W, generator=g).cuda()
    K = syn.intrinsics(W, H)
    return lambda: M.grow_rows(d, sil, gt, color, K, np.eye(4), 0.5, "isotropic")


def depth_pair(H, W, seed=0):
    """rendered and measured depth [1,H,W]: the render within 2 % of the measurement, a sixteenth of the pixels off by +-(0.5 .. 2.0), a block
    without measurement."""
    import torch
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(1, H, W, generator=g) * 3 + 0.5
    d = gt + 0.02 * torch.randn(1, H, W, generator=g)
    displace(d, g)
    gt[0, : H // 3, : W // 2] = 0.0
    return d, gt


def displace(depth, gen):
    import torch
    n = depth.numel()
    idx = torch.randperm(n, generator=gen)[: n // 16]
    depth.view(-1)[idx] += (0.5 + 1.5 * torch.rand(idx.numel(), generator=gen)) * (torch.randint(0, 2, (idx.numel(),), generator=gen).float() * 2 - 1)


def scene(n, W, H):
    """A map of n Gaussians, frame 2 of 4 rendered at a pose a little off the camera column's as its colour and depth target, a sixteenth of the
    measured depths displaced by +-(0.5 .. 2.0)."""
    import numpy as np
    import torch
    from activesplat_amd import mapping as M
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    t, T = 2, 4
    params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in syn.make_params(n, W, H, seed=3).items()}
    rots = torch.tensor([1.0, 0.0, 0.0, 0.0]).reshape(1, 4, 1).repeat(1, 1, T)
    trans = torch.zeros(1, 3, T)
    rots[0, :, t] = torch.tensor([0.99985, 0.01, 0.015, -0.005])
    trans[0, :, t] = torch.tensor([0.03, -0.02, 0.05])
    params["cam_unnorm_rots"], params["cam_trans"] = torch.nn.Parameter(rots.cuda()), torch.nn.Parameter(trans.cuda())
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device="cuda")
    variables = {k: torch.zeros(n, device="cuda") for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
    _, (im, _r, depth, _s, _dsq) = M.tracking_render(params, dict(cam=cam), variables, t)
    measured = depth.cpu().clone()
    displace(measured, torch.Generator().manual_seed(91))
    curr = dict(cam=cam, id=t, im=im.clone(), depth=measured.cuda(), w2c=torch.eye(4, device="cuda"))
    with torch.no_grad():
        params["cam_unnorm_rots"][0, :, t] = torch.tensor([1.1, 0.017, 0.011, 0.003])
        params["cam_trans"][0, :, t] = torch.tensor([0.045, -0.032, 0.07])
        variables["max_2D_radius"].zero_()
    return params, curr, variables, t


def child(section, n, W, H):
    import ctypes as C
    import torch
    from activesplat_amd import _lib
    from activesplat_amd import mapping as M
    from activesplat_amd import optim as O
    assert torch.cuda.is_available(), "outlier_times: needs the GPU"
    lib = _lib.get()

    def say(results, **kw):
        for name, r in results.items():
            print(json.dumps(dict(section=section, P=n, W=W, H=H, path=name, **kw.get(name, {}), **r)), flush=True)
    if section == "median":
        d, g = [x.cuda() for x in depth_pair(H, W)]
        want = ((g - d).abs() * (g > 0)).median()
        st = _lib.stream_ptr(d.device)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        auto = int(lib.gs_depth_error_median_workgroups(W, H))
        variants, extra = {}, {}
        for grid in GRIDS + (0,):
            out = torch.empty(1, device="cuda")
            scratch = torch.empty(int(lib.gs_depth_error_median_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda")
            name = f"gs_depth_error_median G={grid or auto}" + ("" if grid else " (chosen)")
            variants[name] = (lambda grid=grid, out=out, scratch=scratch:
                              _lib.check(lib.gs_depth_error_median_grid(W, H, p(d), p(g), p(scratch), p(out), grid, st)))
            variants[name]()
            assert torch.equal(out.cpu().view(torch.int32), want.cpu().reshape(1).view(torch.int32)), (grid, float(out), float(want))
            extra[name] = dict(grid=grid or auto, chosen=not grid)
        say(timed_alternately(variants), **extra)
        return
    if section == "growth":
        name, step = "grow_rows (gs_grow_gaussians)", growth_step(W, H)
        rows, n_cand = step()
        say(timed_by_events({name: step}), **{name: dict(candidates=n_cand, rows=int(rows["means3D"].shape[0]))})
        return
    params, curr, variables, t = scene(n, W, H)
    if section == "tracking":
        variants = {}
        for option in (False, True):
            cfg = M.tracking_config(dict(use_depth_loss_thres=False, ignore_outlier_depth_loss=option, lrs=ZERO_LRS))
            state = M.TrackingState(params, W, H)
            state.begin(params, t)
            variants[f"tracking_iteration, option {'on' if option else 'off'}"] = \
                (lambda cfg=cfg, state=state: M.tracking_iteration(params, curr, variables, t, cfg, state))
        ref_cfg = dict(use_depth_loss_thres=False, ignore_outlier_depth_loss=True, lrs=ZERO_LRS, tracking_iters=TRACK_ITERS)
        ref = f"track_frame(fused=False), option on, per iteration of {TRACK_ITERS}"
        variants[ref] = lambda: M.track_frame(params, curr, variables, t, ref_cfg, fused=False)
        say(timed_alternately(variants, {ref: TRACK_ITERS}))
        return
    w = dict(im=0.5, depth=1.0)
    opt = O.initialize_optimizer(params, ZERO_LRS)
    variants = {f"mapping_iteration, option {'on' if option else 'off'}":
                (lambda option=option: M.mapping_iteration(params, curr, variables, t, w, opt, ignore_outlier_depth_loss=option)) for option in (False, True)}

    def torch_loss():
        loss, _v, _ = M.get_loss(params, curr, variables, t, w, fused=True, fused_preprocess=True, ignore_outlier_depth_loss=True)
        loss.backward()
        with torch.no_grad():
            opt.step()
            opt.zero_grad(set_to_none=True)
    variants["get_loss(fused_preprocess=True) with the torch loss, option on"] = torch_loss
    say(timed_alternately(variants))


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1], *[int(v) for v in sys.argv[2:5]])
        return
    rows = []
    for n, W, H in SIZES:
        for section in SECTIONS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), section, str(n), str(W), str(H)], stdout=subprocess.PIPE, text=True,
                                   timeout=CHILD_LIMIT)
            except subprocess.TimeoutExpired:
                sys.exit(f"outlier_times: {section} at {W} x {H} ran out of its {CHILD_LIMIT} s: stopping")
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                sys.exit(f"outlier_times: {section} at {W} x {H} ended with status {r.returncode}: stopping")
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    lines = ["ignore_outlier_depth_loss on the fused paths (scripts/outlier_times.py; MI355X).  ms per call: median [min .. max] of "
             f"{ROUNDS} blocks per variant, the variants of a section timed alternately, a block = the given number of calls (about {WINDOW} s), "
             "wall clock around a block that ends in a device synchronise; learning rates zero.", ""]
    for n, W, H in SIZES:
        lines.append(f"{W} x {H}, {n} Gaussians")
        for r in rows:
            if (r["P"], r["W"], r["H"]) == (n, W, H):
                lines.append(f"  {r['section']:9s} {r['path']:68s} {r['ms_median']:8.4f} [{r['ms_min']:.4f} .. {r['ms_max']:.4f}]  x{r['calls_per_block']}")
        lines.append("")
    out = os.path.join(ROOT, os.environ.get("OUT", os.path.join("profiles", "outlier_loss.txt")))
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
