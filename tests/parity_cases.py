"""Parity cases shared by the host-emulated kernel tests (CPU) and the GPU tests: each case builds a
settings tuple + rendervars, runs the product path and the fp32 C oracle on identical inputs, and
checks: integer artefacts bit-exact (radii, tile rects, tile counts, scan offsets, sorted keys, sorted
ids incl. index tie-break, tile ranges, n_contrib), images within the stated fp32 tolerance
(atol 1e-5 + rtol 1e-4; >= 99.9 % of pixels, the rest are alpha = 1/255 /
T = 1e-4 threshold flips caused by exp() ULP differences, each bounded by one alpha*colour step),
gradients vs the fp64 oracle (rtol 1e-3, atol 1e-6 |g|_inf on >= 99.5 % of elements and relative
L2 error < 1e-3)."""
import numpy as np
import torch

from tests import util

FWD_RTOL, FWD_ATOL = 1e-4, 1e-5
GRAD_RTOL = 1e-3


def build_case(name, device):
    W, H, N, kw, mutate = 96, 80, 2500, {}, None
    if name == "basic":
        pass
    elif name == "ragged_image":            # 50x37: partial tiles on both edges
        W, H, N = 50, 37, 800
    elif name == "tiny_lookaround":         # the reference's 120x150 visibility views
        W, H, N = 120, 150, 1500
    elif name == "lookaround_intrinsics":   # the planner's 120 x 150 view: hfov 120, vfov 150 -> fx = 34.6, fy = 20.1, cx = 59, cy = 74
        from activesplat_amd.lookaround import look_around_k
        W, H, N = 120, 150, 4000
        kw = dict(K=look_around_k(), w2c=util.pose(0.4, (0.05, -0.02, 0.2)), bg=(1.0, 1.0, 1.0))
    elif name == "posed_white_bg":
        kw = dict(w2c=util.pose(0.25, (0.1, -0.05, 0.3)), bg=(1.0, 1.0, 1.0))
    elif name == "scale_modifier":
        kw = dict(scale_modifier=0.37, bg=(0.2, 0.1, 0.4))
    elif name == "scale_modifier_001":      # the planner's scale_modifier (visualizer.py:935-936) on an ordinary view: every splat shrinks to the low-pass footprint
        N, kw = 4000, dict(scale_modifier=0.01, bg=(0.1, 0.0, 0.2))
    elif name in ("topdown_1000m", "topdown_1000m_white"):
        # the planner's top-down map camera (src/visualizer/visualizer.py:923-937,1577-1601 through splatam.py:413-434): 1000 m above the scene,
        # focal length 2e4 px, far = 100 (no far cull: everything is ~1000 deep), scale_modifier 0.01; black background (the depth / silhouette
        # pass and the "free map") and white (the colour pass)
        return topdown_scene(20000, device, bg=(1.0, 1.0, 1.0) if name.endswith("white") else (0.0, 0.0, 0.0))
    elif name == "behind_camera":           # about half the Gaussians are near-culled
        kw = dict(w2c=util.pose(0.0, (0.0, 0.0, -2.0)))
    elif name == "all_culled":              # D == 0
        kw = dict(w2c=util.pose(0.0, (0.0, 0.0, -100.0)), bg=(0.3, 0.6, 0.9))
    elif name == "huge_gaussians":          # few Gaussians covering hundreds of tiles each
        N, kw = 40, dict(scale_jitter=0.1)
        mutate = lambda rv: rv.update(scales=rv["scales"] * 60.0)  # noqa: E731
    elif name == "dense_overdraw":          # early termination (T < 1e-4) everywhere
        W, H, N = 48, 48, 6000
        mutate = lambda rv: rv.update(opacities=rv["opacities"] * 0.5 + 0.5)  # noqa: E731
    elif name == "mixed_sizes":
        # depth bands of quadrant-covering splats between bands of small ones, all faint (no saturation): list chunks of ~15 and of 64 hit
        # records in turn -> the blend kernels' compacted staging closes rounds early AND splits chunks (blend.hip)
        W, H, N = 64, 64, 6000

        def mutate(rv):
            z = rv["means3D"][:, 2:3]
            big = (torch.floor(z * 6.0).long() % 2 == 0)
            rv.update(scales=torch.where(big, rv["scales"] * 25.0, rv["scales"]), opacities=rv["opacities"] * 0.04)
    elif name == "merge_tiles":             # ~5k instances per tile: chunk sort + LDS rank-merge (8192 variant)
        W, H, N = 48, 48, 20000
        mutate = lambda rv: rv.update(opacities=rv["opacities"] * 0.05)  # noqa: E731
    elif name == "merge_tiles_large":       # ~12k instances per tile: 16384 variant
        W, H, N = 48, 48, 48000
        mutate = lambda rv: rv.update(opacities=rv["opacities"] * 0.02)  # noqa: E731
    elif name == "merge_passes":            # > 16384 instances per tile: 4096-key runs + pairwise merge passes through global memory (3 passes)
        W, H, N = 32, 32, 40000
        mutate = lambda rv: rv.update(opacities=rv["opacities"] * 0.02)  # noqa: E731
    elif name == "merge_passes_even":       # > 32768 per tile: 4 passes (the run sort starts in the other buffer), ragged last runs
        W, H, N = 32, 32, 75000
        mutate = lambda rv: rv.update(opacities=rv["opacities"] * 0.01)  # noqa: E731
    elif name in ("bucket_lists", "bucket_lists_long", "crowded_depth", "crowded_depth_long", "bucket_lists_big", "crowded_depth_big"):
        # tile lists of ~3.5 k / ~4.6 k keys (one bucket-sort workgroup per tile, 8 / 10 keys per thread); "crowded": every depth but a
        # few outliers inside 1e-4 of each other, so one bin of the bucket sort holds the whole list -> its comparison-network branch
        # (one run / two runs + merge)
        # "_big": ~8-10 k keys per tile: the 1024-thread instantiation of the bucket sort (eleven keys per thread; crowded: its network branch,
        # a run of 8192 + the rest + a rank merge)
        W, H, N = 48, 48, {"bucket_lists": 14000, "bucket_lists_long": 18000, "crowded_depth": 11000, "crowded_depth_long": 15500,
                           "bucket_lists_big": 34000, "crowded_depth_big": 30000}[name]

        def mutate(rv, crowded=name.startswith("crowded")):
            upd = dict(opacities=rv["opacities"] * 0.05)
            if crowded:
                g = torch.Generator().manual_seed(7)
                m = rv["means3D"]
                znew = 2.0 + 1e-4 * torch.rand(m.shape[0], generator=g).to(m.device)
                znew[:3] = 0.6; znew[3:6] = 3.9
                upd["means3D"] = (m * (znew / m[:, 2])[:, None]).contiguous()
            rv.update(upd)
    elif name == "equal_depth":             # every Gaussian at exactly the same view depth: the keys differ in the id only (index tie-break);
        W, H, N = 48, 48, 9000              # the bucket sort sees zero depth span (one bin) -> comparison-network branch

        def mutate(rv):
            m = rv["means3D"]
            rv.update(means3D=(m * (2.0 / m[:, 2])[:, None]).contiguous(), opacities=rv["opacities"] * 0.05)
    elif name == "many_tiles":              # 2064x1104 px = 129 x 69 = 8901 tiles > 8192: no LDS tile histogram -> radix path
        W, H, N = 2064, 1104, 3000
    elif name == "low_opacity":             # many Gaussians below the 1/255 threshold
        mutate = lambda rv: rv.update(opacities=rv["opacities"] * 0.02)  # noqa: E731
    elif name == "one_gaussian":
        N = 1
    elif name == "not_multiple_of_block":
        N = 257
    elif name in ("sh0", "sh1", "sh2", "sh3"):
        kw = dict(sh_degree=int(name[2]), w2c=util.pose(-0.15, (0.05, 0.0, 0.1)))
    elif name == "sh3_half_culled":         # half of the Gaussians near-culled: their SH rows are not fetched in the backward
        N, kw = 1500, dict(sh_degree=3, w2c=util.pose(0.0, (0.0, 0.0, -2.0)))
    elif name == "sh2_ragged":              # 1003 = 31*32 + 11 rows of 27 floats: partial slab, scalar tail of the 16 B copies
        N, kw = 1003, dict(sh_degree=2, w2c=util.pose(0.1, (0.0, 0.05, 0.1)))
    elif name == "cov3d_precomp":
        pass
    elif name in ("nonfinite_geometry", "nonfinite_appearance", "nonfinite_sh"):
        # Parameters a diverged Adam step can produce (the reference guards poses only: src/mapper/splatam/__init__.py:514-515; NaN depth pixels are
        # masked in the loss, splatam.py:221-231 -- nothing guards the Gaussians).  Geometry: NaN / inf means, inf / zero / NaN / negative scales,
        # zero and NaN quaternions, view depth exactly at the 0.2 near cull, a scale of 1e4 (radius ~ 1e6 px).  Appearance: NaN opacity, NaN colour
        # (one channel), opacity above 1 and below 0.  Rule: a Gaussian whose screen-space record holds a NaN or an infinity is
        # culled (radius 0, zero gradients); finite out-of-range values are taken as they are.
        W, H, N = 160, 120, 3000
        if name == "nonfinite_sh":
            kw = dict(sh_degree=3)

        def mutate(rv, name=name):
            nan, inf = float("nan"), float("inf")
            m, sc, q = rv["means3D"].clone(), rv["scales"].clone(), rv["rotations"].clone()
            m[0, 0] = nan; m[1, 1] = nan; m[2, 2] = nan; m[3] = nan
            m[10, 0] = inf; m[11, 1] = -inf; m[12, 2] = inf; m[13, 2] = -inf; m[14] = inf
            sc[20, 0] = inf; sc[21] = inf; sc[30, 1] = 0.0; sc[31] = 0.0; sc[40, 2] = nan; sc[41] = nan; sc[50, 0] = -sc[50, 0]; sc[51] = -sc[51]
            q[60] = 0.0; q[61] = 0.0; q[70, 0] = nan; q[71] = nan
            m[80:90, 2] = 0.2                                 # exactly the near-cull depth (culled: p_view.z <= 0.2)
            m[90:92, 2] = 0.20000002                          # the next float above it (kept)
            sc[95:98] = 1.0e4
            upd = dict(means3D=m, scales=sc, rotations=q)
            if name != "nonfinite_geometry":
                o = rv["opacities"].clone()
                o[100] = nan; o[101] = nan; o[102] = 2.0; o[103] = -0.5
                upd["opacities"] = o
                if "colors_precomp" in rv:
                    c = rv["colors_precomp"].clone()
                    c[110, 1] = nan; c[111] = nan
                    upd["colors_precomp"] = c
                else:
                    sh = rv["shs"].clone()
                    sh[110, 0, 1] = nan; sh[111, 5, :] = nan      # a DC coefficient, a degree-2 coefficient of all channels
                    upd["shs"] = sh
            rv.update(upd)
    else:
        raise KeyError(name)
    rs, rv = util.scene(N, W, H, seed=abs(hash(name)) % 1000 if False else sum(map(ord, name)), device=device, **kw)
    if mutate:
        mutate(rv)
    if name == "cov3d_precomp":
        from oracle.dense_torch import build_cov3d
        S = build_cov3d(rv["scales"].cpu(), rv["rotations"].cpu(), 1.0)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()
        rv.pop("scales"); rv.pop("rotations")
        rv["cov3D_precomp"] = cov.to(device)
    return rs, rv


def topdown_camera(W=360, H=300, scene_w=18.0, scene_h=15.0, centre=(0.3, -0.2), height=1000.0, bg=(0.0, 0.0, 0.0), device="cpu", scale_modifier=0.01):
    """The settings get_topdown_cam + render_o3d_image hand the rasteriser (visualizer.py:1577-1601): camera `height` metres up the -y axis
    looking along +y, fov from the scene's extent, principal point at the integer image centre, near 0.01 / far 100."""
    from activesplat_amd.camera import setup_camera
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float64)
    c2w[:3, 3] = [centre[0], -height, centre[1]]
    fx, fy = W / (scene_w / height), H / (scene_h / height)          # fov2focal(2 atan(extent / 2h), pixels)
    K = np.array([[fx, 0.0, W // 2], [0.0, fy, H // 2], [0.0, 0.0, 1.0]])
    return setup_camera(W, H, K, np.linalg.inv(c2w), near=0.01, far=100, scale_modifier=scale_modifier, bg=bg, device=device)


def topdown_scene(N, device, seed=12, bg=(0.0, 0.0, 0.0), W=360, H=300):
    """A room-scale map (18 m x 15 m footprint, heights -1.6 .. 0.2 m in the mapper's y-down world frame, splats of 1-8 cm) under the
    top-down camera; a tenth of it lies outside the footprint."""
    g = torch.Generator().manual_seed(seed)
    xz = (torch.rand(N, 2, generator=g) - 0.5) * torch.tensor([20.0, 16.5])
    y = -1.6 + 1.8 * torch.rand(N, 1, generator=g)
    means = torch.cat([xz[:, :1], y, xz[:, 1:]], 1)
    scales = torch.exp(torch.log(torch.tensor(0.03)) + 0.5 * torch.randn(N, 3, generator=g))
    rv = dict(means3D=means.float(), rotations=torch.nn.functional.normalize(torch.randn(N, 4, generator=g)),
              opacities=torch.sigmoid(torch.randn(N, 1, generator=g) + 1.0), scales=scales.float(), colors_precomp=torch.rand(N, 3, generator=g))
    rs = topdown_camera(W, H, bg=bg, device=device)._replace(debug=True)
    return rs, {k: v.to(device).contiguous() for k, v in rv.items()}


BIG_TILE_CASES = ["merge_tiles", "merge_tiles_large", "merge_passes", "merge_passes_even", "bucket_lists", "bucket_lists_long", "crowded_depth",
                  "crowded_depth_long", "equal_depth", "bucket_lists_big", "crowded_depth_big"]
CASES = ["basic", "ragged_image", "tiny_lookaround", "lookaround_intrinsics", "posed_white_bg", "scale_modifier", "scale_modifier_001", "topdown_1000m",
         "topdown_1000m_white", "behind_camera", "all_culled",
         "huge_gaussians", "dense_overdraw", "mixed_sizes", "low_opacity", "one_gaussian", "not_multiple_of_block", "sh0", "sh1", "sh2",
         "sh3", "sh2_ragged", "sh3_half_culled", "cov3d_precomp"]
#: inputs with NaN / inf / out-of-range parameters (culled; images and gradients stay finite -- the ordinary checks apply)
NONFINITE_CASES = ["nonfinite_geometry", "nonfinite_appearance", "nonfinite_sh"]
CASES += NONFINITE_CASES


def set_sort_path(path):
    """path: 'auto' | 'tile_lds' | 'radix' -- forces the binning path of the library under test."""
    from activesplat_amd import _lib
    _lib.check(_lib.get().gs_set_sort_path({"auto": 0, "tile_lds": 1, "radix": 2}[path]))


def check_whole_quadrants_on_small_images(device, oracle32, oracle64):
    """Images of at most 256 tiles are blended by half-quadrant wavefronts (default), so the small parity cases all run that way: here
    the same cases with whole quadrants (what larger images use), and both must agree with each other bit for bit in the forward."""
    from activesplat_amd import _lib
    lib = _lib.get()
    try:
        for name in ("basic", "ragged_image", "posed_white_bg", "dense_overdraw", "mixed_sizes", "huge_gaussians", "sh3", "merge_tiles", "not_multiple_of_block"):
            rs, rv = build_case(name, device)
            _lib.check(lib.gs_set_half_quadrants(256))
            halves = util.run_product(rs, rv)
            _lib.check(lib.gs_set_half_quadrants(0))
            got, _ = check_forward(rs, rv, oracle32)
            for k in ("color", "depth", "opacity"):
                assert np.array_equal(got[k], halves[k]), (name, k)
            if name in ("basic", "ragged_image", "dense_overdraw", "mixed_sizes", "sh3"):
                check_backward(rs, rv, oracle64, oracle32=oracle32)
    finally:
        _lib.check(lib.gs_set_half_quadrants(256))


def check_raw_parameter_mode(device, n=500):
    """mapping.get_loss(fused_preprocess=True) -- the rasteriser's per-Gaussian kernels take the mapper's PARAMETERS and do the frame transform
    + activations themselves (gs_preprocess_forward_raw / gs_render_backward_raw) -- against the activation kernels in front of the rasteriser
    (fused_inputs) and the reference's torch ops: loss, statistics, gradients; isotropic and anisotropic maps; and, over two keyframes, the
    in-kernel accumulation into .grad against autograd's."""
    from activesplat_amd import mapping as M
    from tests.test_parallel import _scene
    for iso in (False, True):
        out = []
        for mode in ("torch", "kernels", "raw", "raw_acc"):
            params, kfs = _scene(n=n, device=device)
            if iso:
                params["log_scales"] = torch.nn.Parameter(params["log_scales"].detach()[:, :1].clone())
            nn_ = params["means3D"].shape[0]
            variables = {k: torch.zeros(nn_, device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
            flags = dict(torch=dict(), kernels=dict(fused=True, fused_loss=True, fused_inputs=True),
                         raw=dict(fused=True, fused_loss=True, fused_preprocess=True),
                         raw_acc=dict(fused=True, fused_loss=True, fused_preprocess=True, accumulate_grads=True))[mode]
            total = 0.0
            for t in (1, 2):                               # two keyframes: gradients accumulate
                loss, variables, _ = M.get_loss(params, kfs[t], variables, t, dict(im=0.5, depth=1.0), **flags)
                loss.backward()
                total += float(loss.detach())
            out.append((total, {k: v.grad.clone() for k, v in params.items() if v.grad is not None}, variables["max_2D_radius"].clone(),
                        variables["seen"].clone()))
        for o in out[1:]:
            assert abs(out[0][0] - o[0]) < 4e-6 * abs(out[0][0]), (iso, out[0][0], o[0])
            # (the activations are not bit-identical between torch, activate.hip and the contraction-free per-Gaussian kernels: a radius --
            # ceil(3 sigma) -- may flip by one for a Gaussian on the boundary, which also moves `seen` for radius 0 <-> 1)
            dr = (out[0][2] - o[2]).abs()
            assert float(dr.max()) <= 1.0 and float((dr > 0).float().mean()) < 5e-4, (iso, float(dr.max()), int((dr > 0).sum()))
            assert float((out[0][3] != o[3]).float().mean()) < 5e-4, int((out[0][3] != o[3]).sum())
            for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
                a, b = out[0][1][k], o[1][k]
                assert a.shape == b.shape, (k, a.shape, b.shape)
                if iso and k == "unnorm_rotations":          # equal scales: the rotation does not matter, its gradient is rounding noise
                    assert float((a - b).norm()) < 1e-5 * float(out[0][1]["means3D"].norm()), (k, float((a - b).norm()))
                    continue
                assert float((a - b).norm() / a.norm()) < 3e-4, (iso, k, float((a - b).norm() / a.norm()))


def check_raw_parameter_mode_nonfinite(device, n=600):
    """The non-finite rule in the mapper's own call (get_loss from the PARAMETERS: the frame transform and the activations run inside the per-Gaussian
    kernels): NaN / inf means, log scales of +inf (exp -> inf) and -inf (exp -> 0: finite, kept), NaN and +inf logits (sigmoid(+inf) = 1: finite, kept),
    a zero quaternion (F.normalize's eps keeps it zero: finite, kept) and a NaN quaternion, a NaN colour.  Every path -- activation kernels + plain rasteriser, raw-parameter rasteriser, the
    same with in-kernel accumulation, the Adam step inside the backward -- culls the same rows: finite loss, finite gradients, zero gradient and
    `seen` = False for the culled rows, and the parameters of every OTHER row step as they do without the bad rows' presence being felt."""
    from activesplat_amd import mapping as M, optim as O
    from tests.test_parallel import _scene
    nan, inf = float("nan"), float("inf")
    bad = [3, 4, 5, 10, 20, 21, 31, 40]
    kept = [11, 22, 30]
    lrs = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)

    def scene():
        params, kfs = _scene(n=n, device=device)
        with torch.no_grad():
            params["means3D"][3, 0] = nan; params["means3D"][4, 2] = inf; params["means3D"][5] = -inf
            params["log_scales"][10, 1] = inf; params["log_scales"][11, 1] = -inf
            params["logit_opacities"][20] = nan; params["logit_opacities"][21] = -nan; params["logit_opacities"][22] = inf
            params["unnorm_rotations"][30] = 0.0; params["unnorm_rotations"][31, 2] = nan
            params["rgb_colors"][40, 1] = nan
        return params, kfs
    outs = {}
    for mode in ("kernels", "raw", "raw_acc", "raw_adam"):
        params, kfs = scene()
        variables = {k: torch.zeros(n, device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
        opt = O.initialize_optimizer(params, lrs)
        flags = dict(kernels=dict(fused=True, fused_loss=True, fused_inputs=True), raw=dict(fused=True, fused_loss=True, fused_preprocess=True),
                     raw_acc=dict(fused=True, fused_loss=True, fused_preprocess=True, accumulate_grads=True),
                     raw_adam=dict(fused=True, fused_loss=True, fused_preprocess=True, fused_adam=opt))[mode]
        before = {k: v.detach().clone() for k, v in params.items()}
        loss, variables, _ = M.get_loss(params, kfs[1], variables, 1, dict(im=0.5, depth=1.0), **flags)
        loss.backward()
        assert bool(torch.isfinite(loss)), (mode, float(loss))
        seen = variables["seen"]
        assert not bool(seen[bad].any()), (mode, seen[bad].tolist())
        assert bool(torch.isfinite(variables["means2D"].grad).all()) and float(variables["means2D"].grad[bad].abs().max()) == 0.0, mode
        if mode == "raw_adam":
            for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
                rows = [i for i in range(n) if i not in bad and i not in kept]
                assert bool(torch.isfinite(params[k].detach()[rows]).all()), (mode, k)
                # a culled row is stepped with a zero gradient: first step, zero moments -> the parameter does not move (a NaN stays the NaN it was)
                a, b = params[k].detach()[bad], before[k][bad]
                assert bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()), (mode, k)
        else:
            good = torch.ones(n, dtype=torch.bool, device=params["means3D"].device)
            good[bad] = False
            for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
                g = params[k].grad
                assert g is not None and bool(torch.isfinite(g[good]).all()), (mode, k)
                if mode != "kernels":
                    # (the separate activation kernels -- like the reference's torch activations -- chain the rasteriser's ZERO gradient of a culled
                    # row through the derivative of a NaN activation: 0 x NaN.  The raw-parameter kernels write the culled row's zero directly)
                    assert bool(torch.isfinite(g).all()) and float(g[bad].abs().max()) == 0.0, (mode, k, g[bad])
            outs[mode] = (float(loss.detach()), {k: params[k].grad[good].clone() for k in lrs if params[k].grad is not None})
    for mode in ("raw", "raw_acc"):
        assert abs(outs["kernels"][0] - outs[mode][0]) < 4e-6 * abs(outs["kernels"][0]), (mode, outs["kernels"][0], outs[mode][0])
        for k in ("means3D", "rgb_colors", "logit_opacities", "log_scales"):
            a, b = outs["kernels"][1][k], outs[mode][1][k]
            assert float((a - b).norm() / a.norm()) < 3e-4, (mode, k, float((a - b).norm() / a.norm()))


def check_loss_masks_nonfinite_depth(device, n=500):
    """The mapping loss masks pixels without a valid depth measurement (splatam.py:221-231: `depth > 0` and the rendered values not NaN).  A NaN / inf /
    negative / zero ground-truth depth pixel must count exactly like a missing one (0) in the fused loss (csrc/loss.hip) -- value and every
    gradient identical to the bit of the same call with those pixels zeroed, everything finite.  (The reference's torch ops give the masked pixels
    a 0 x sign(NaN) = NaN gradient there; the fused kernels select.)"""
    from activesplat_amd import mapping as M
    from tests.test_parallel import _scene
    out = []
    for variant in ("zeroed", "nonfinite"):
        params, kfs = _scene(n=n, device=device)
        kf = dict(kfs[1])
        d = kf["depth"].clone()
        H, W = d.shape[-2:]
        d[0, 0:3, :] = 0.0 if variant == "zeroed" else float("nan")
        d[0, 5, : W // 2] = 0.0 if variant == "zeroed" else float("-inf")
        d[0, 7, 1::2] = 0.0 if variant == "zeroed" else -1.5
        d[0, H - 1, :] = 0.0
        kf["depth"] = d
        nn_ = params["means3D"].shape[0]
        variables = {k: torch.zeros(nn_, device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
        loss, variables, _ = M.get_loss(params, kf, variables, 1, dict(im=0.5, depth=1.0), fused=True, fused_loss=True, fused_inputs=True)
        loss.backward()
        assert bool(torch.isfinite(loss)), (variant, float(loss))
        grads = {k: v.grad.clone() for k, v in params.items() if v.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values()), variant
        out.append((float(loss.detach()), grads))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        a, b = out[0][1][k], out[1][1][k]
        assert float((a - b).norm()) <= 2e-5 * float(a.norm()), k          # (device: the atomic sums' order; emulated kernels: equal)


def check_raw_parameter_mode_sh(device, n=400, W=64, H=48):
    """The same with 16-coefficient SH rows (configs[2]'s loop): render_rgbd_raw(shs=...) against fused_rendervar + render_rgbd(shs=...)."""
    from activesplat_amd import mapping as M, rasterizer as R
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    p = syn.make_params(n, W, H, seed=5, sh_degree=3)
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, sh_degree=3)
    pose = [0.9950042, 0.0, 0.0998334, 0.0, 0.03, -0.02, 0.05]
    g = torch.Generator().manual_seed(2)
    dLc, dLd = torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)
    out = []
    for raw in (False, True):
        prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
        if raw:
            m2d = torch.empty_like(prm["means3D"], requires_grad=True)
            im, radius, depth, sil, dsq = R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"],
                                                            pose, shs=prm["shs"])
        else:
            rv = M.fused_rendervar(dict(prm, rgb_colors=prm["shs"]), 0, pose)
            rv.pop("colors_precomp")
            m2d = rv["means2D"]
            im, radius, depth, sil, dsq = R.render_rgbd(cam, shs=prm["shs"], **rv)
        ((im * dLc).sum() + (depth * dLd).sum()).backward()
        out.append((im.detach().clone(), depth.detach().clone(), radius.clone(), {k: v.grad.clone() for k, v in prm.items() if v.grad is not None},
                    m2d.grad.clone()))
    a, b = out
    dr = (a[2] - b[2]).abs()
    assert int(dr.max()) <= 1 and float((dr > 0).float().mean()) < 5e-4, (int(dr.max()), int((dr > 0).sum()))      # (see above: boundary radii)
    # images: equal up to the activations' rounding, except where it flips an alpha >= 1/255 / T >= 1e-4 test of a pixel (bounded, rare)
    for x, y, tol in ((a[0], b[0], 5e-5), (a[1], b[1], 5e-4)):
        d = (x - y).abs()
        assert float((d > tol).float().mean()) < 1e-3 and float(d.max()) < 0.02 * max(1.0, float(y.abs().max())), (float(d.max()), int((d > tol).sum()))
    for k in ("means3D", "shs", "unnorm_rotations", "logit_opacities", "log_scales"):
        assert float((a[3][k] - b[3][k]).norm() / a[3][k].norm()) < 3e-4, (k, float((a[3][k] - b[3][k]).norm() / a[3][k].norm()))
    assert float((a[4] - b[4]).norm() / a[4].norm()) < 3e-4


def _depth_ties_cover(prm_means, pose, rv_means, radius, d, W, H, tol):
    """True when every pixel of `d` above `tol` lies in the footprints of a pair of Gaussians whose view depths are within four ulps in fp32 (or ordered the other
    way in fp64): the depth order of such a pair is not decided in fp32, the two entries evaluate the frame transform with different roundings, and either order is a
    valid rendering (scripts/exp/fuzz_raw_diag.py prints the pairs).  -> (all covered, covered pixels, differing pixels, largest difference OUTSIDE the pairs' footprints)."""
    from activesplat_amd import synthetic as syn
    K = syn.intrinsics(W, H)
    z32 = rv_means[:, 2].cpu()
    px = (rv_means[:, 0] / rv_means[:, 2] * K[0][0] + K[0][2]).cpu(); py = (rv_means[:, 1] / rv_means[:, 2] * K[1][1] + K[1][2]).cpu()
    q = torch.tensor(pose[:4], dtype=torch.float64); t = torch.tensor(pose[4:], dtype=torch.float64)
    w, x, y, z = q / q.norm()
    Rm = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)
    z64 = (prm_means.double().cpu() @ Rm.T + t)[:, 2]
    order = torch.argsort(z32, stable=True)
    zs, zz = z32[order], z64[order]
    near = torch.nonzero((zz[1:] < zz[:-1]) | ((zs[1:] - zs[:-1]) <= 4 * torch.finfo(torch.float32).eps * zs[1:].abs()))[:, 0]
    ra = radius.cpu().float()
    ys, xs = torch.nonzero(d.cpu() > tol, as_tuple=True)
    covered = torch.zeros(len(ys), dtype=torch.bool)
    for j in near.tolist():
        i0, i1 = int(order[j]), int(order[j + 1])
        if ra[i0] > 0 and ra[i1] > 0:
            both = torch.ones(len(ys), dtype=torch.bool)
            for i in (i0, i1):
                both &= ((xs - px[i]).abs() <= ra[i] + 1) & ((ys - py[i]).abs() <= ra[i] + 1)
            covered |= both
    rest = d.cpu()[ys[~covered], xs[~covered]]
    return bool(covered.all()), int(covered.sum()), len(ys), (float(rest.max()) if len(rest) else 0.0)


def check_raw_entry_random_draw(seed, device, rows_detail=False):
    """One draw of the raw-parameter sweep (scripts/exp/fuzz_raw.py; profiles/r05_fuzz_raw.txt): render_rgbd_raw (frame transform + activations inside the per-Gaussian
    kernels, gradients w.r.t. the PARAMETERS) against fused_rendervar + render_rgbd on a random map (50..40 000 Gaussians, colours or 16 SH rows, isotropic or
    anisotropic), image size (both sides of the few-tile / chained-kernel thresholds) and pose.  Radii within one on a handful of boundary Gaussians; images equal up to
    bounded threshold flips; parameter gradients within 3e-4 relative L2 without the two worst rows.
    -> "ok" | "depth tie" (the two entries blend a pair of splats whose view depths are within four fp32 ulps in different orders and every differing pixel lies in the
    pair's footprints: both are valid fp32 renderings, the gradients are not compared) | ("rows", key, row, relative difference) (two rows carry more than 3e-3 of
    the norm: one per-pixel alpha = 1/255 decision)."""
    from activesplat_amd import mapping as M, rasterizer as R
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    r = np.random.RandomState(seed)
    n = int(r.choice([int(r.randint(50, 2000)), int(r.randint(2000, 40000))]))
    W, H = (int(r.randint(24, 200)), int(r.randint(24, 160))) if seed % 3 else (int(r.randint(272, 420)), int(r.randint(256, 330)))
    sh, iso = seed % 4 == 0, bool(seed % 2)
    p = syn.make_params(n, W, H, seed=seed, sh_degree=3 if sh else None)
    if sh:
        p.pop("rgb_colors", None)
    if iso:
        p["log_scales"] = p["log_scales"][:, :1].contiguous()
    p["log_scales"] = p["log_scales"] + float(r.uniform(-0.5, 1.2))
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, sh_degree=3 if sh else 0)
    a = float(r.uniform(-0.4, 0.4))
    pose = [float(np.cos(a / 2)), 0.0, float(np.sin(a / 2)), 0.0, float(r.uniform(-0.2, 0.2)), float(r.uniform(-0.1, 0.1)), float(r.uniform(-0.8, 0.4))]
    g = torch.Generator().manual_seed(seed)
    dLc, dLd = torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)
    out = []
    for raw in (False, True):
        prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
        col = dict(shs=prm["shs"]) if sh else dict(colors_precomp=prm["rgb_colors"])
        if raw:
            m2d = torch.empty_like(prm["means3D"], requires_grad=True)
            im, radius, depth, sil, dsq = R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], pose, **col)
        else:
            rv = M.fused_rendervar(dict(prm, rgb_colors=prm["shs"]) if sh else prm, 0, pose)
            rv.pop("colors_precomp")
            m2d = rv["means2D"]
            tm = rv["means3D"].detach().clone()
            im, radius, depth, sil, dsq = R.render_rgbd(cam, **col, **rv)
        ((im * dLc).sum() + (depth * dLd).sum()).backward()
        out.append((im.detach(), depth.detach(), radius.clone(), {k: v.grad.double() for k, v in prm.items() if v.grad is not None}, m2d.grad.double()))
    x, y = out
    dr = (x[2] - y[2]).abs()
    assert int(dr.max()) <= 1 and float((dr > 0).float().mean()) < 2e-3 + 2.0 / n, ("radii", int(dr.max()), int((dr > 0).sum()))
    for u, v, tol, nm in ((x[0], y[0], 5e-5, "colour"), (x[1], y[1], 5e-4, "depth")):
        d = (u - v).abs()
        if not (float((d > tol).float().mean()) < 2e-3 and float(d.max()) < 0.03 * max(1.0, float(v.abs().max()))):
            # a depth tie may come with the ordinary alpha = 1/255 threshold flips elsewhere in the image (seeds 4385 / 4668 of the round-6 soak: one and two
            # pixels of 4e-4 .. 2.4e-3 next to 60 / 63 tie pixels): what the pairs' footprints do not cover must meet the bound a scene without a tie meets
            ok, c, m, rest = _depth_ties_cover(p["means3D"], pose, tm, x[2], d.amax(0), W, H, tol)
            assert c > 0 and (m - c) / float(H * W) < 2e-3 and rest < 0.03 * max(1.0, float(v.abs().max())), \
                (nm, float(d.max()), int((d > tol).sum()), "pixels in depth-tie footprints: %d of %d, largest difference outside them %.2e" % (c, m, rest))
            return "depth tie"
    verdict = "ok"
    for k in x[3]:
        if iso and k == "unnorm_rotations":                 # equal scales: the rotation's gradient is rounding noise
            continue
        e2 = ((x[3][k] - y[3][k]).reshape(n, -1) ** 2).sum(1)
        nr = float(x[3][k].norm().clamp_min(1e-30))
        rest = float((e2.sum() - e2.sort().values[-2:].sum()).clamp_min(0).sqrt()) if n > 8 else 0.0
        if not rest < 3e-4 * nr:
            # a depth tie SMALL enough for the images to pass the bound above (seeds 8395 / 8572 of the round-6 soak: 15 / 11 pixels, at most 1.8e-3 / 5.6e-3)
            # still reorders the pair for every Gaussian blended behind it there -- more than two rows move (3.4e-4 / 4.5e-4 of the norm without the two
            # worst): the same verdict as above when the pairs' footprints cover every differing pixel
            d = (x[0] - y[0]).abs().amax(0)
            ok, c, m, _ = _depth_ties_cover(p["means3D"], pose, tm, x[2], d, W, H, 5e-5)
            assert ok and c > 0 and rest < 3e-3 * nr, (k, rest / nr, float(e2.sum().sqrt()) / nr, "pixels in depth-tie footprints: %d of %d" % (c, m))
            return "depth tie"
        if not float(e2.sum().sqrt()) < 3e-3 * nr and verdict == "ok":
            w = int(e2.argmax())
            verdict = ("rows", k, w, round(float(e2.sum().sqrt()) / nr, 5))
            if rows_detail:                                 # the one pixel inside that Gaussian's footprint where the two forward images differ
                K = syn.intrinsics(W, H)
                cx, cy = float(tm[w, 0] / tm[w, 2] * K[0][0] + K[0][2]), float(tm[w, 1] / tm[w, 2] * K[1][1] + K[1][2])
                dd = (x[0] - y[0]).abs().amax(0)
                rr = int(x[2][w]) + 1
                x0, x1, y0, y1 = max(0, int(cx) - rr), min(W, int(cx) + rr + 2), max(0, int(cy) - rr), min(H, int(cy) + rr + 2)
                box = dd[y0:y1, x0:x1]
                top = torch.topk(box.flatten(), min(5, box.numel()))
                print("   seed", seed, k, "row", w, "radius", int(x[2][w]), "centre (%.1f, %.1f); largest colour differences inside its footprint:" % (cx, cy),
                      [(x0 + int(i) % (x1 - x0), y0 + int(i) // (x1 - x0), "%.2e" % float(v)) for v, i in zip(top.values, top.indices)],
                      "; median over the image %.2e, maximum %.2e" % (float(dd.median()), float(dd.max())),
                      "\n      activation kernels:", x[3][k][w].tolist(), "\n      raw entry:         ", y[3][k][w].tolist())
    return verdict


def _classify_loss_call_difference(p, q, t, kf, cam, W, H, dev):
    """Why the two calls' gradients differ by more than rounding: the two renders (inputs one ulp apart: torch activations in front of the plain render / activations inside
    the raw entry's kernels) are compared.  -> ("L1 kink", flips): sign(im - gt), the gradient of the reference's L1 colour term, differs at a pixel-channel -- one flip moves
    dL/dC there by 2 * 0.5 * 0.8 / (3 H W) for every Gaussian blended at the pixel;  ("depth L1 kink", flips): the same for sign(depth - gt) of the masked depth term
    (2 / number of masked pixels);  ("depth tie", n): every pixel that differs by more than 5e-5 lies in the footprints of a
    pair of splats whose view depths are within four fp32 ulps (parity_cases._depth_ties_cover) -- through the SSIM window every Gaussian around sees another dL/dC;  else None."""
    from activesplat_amd import mapping as M, rasterizer as R
    with torch.no_grad():
        prm = {k: v.clone().to(dev) for k, v in p.items()}
        prm["cam_unnorm_rots"] = q.reshape(1, 4, 1).clone().to(dev); prm["cam_trans"] = t.reshape(1, 3, 1).clone().to(dev)
        rv0 = M.transformed_params2rendervar(prm, M.transform_to_frame(prm, 0, gaussians_grad=False, camera_grad=False))
        pose7 = torch.cat([torch.nn.functional.normalize(q, dim=0), t]).tolist()
        a = R.render_rgbd(cam, **{k: v.detach() for k, v in rv0.items()})
        b = R.render_rgbd_raw(cam, prm["means3D"], torch.empty_like(prm["means3D"]), prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], pose7,
                              colors_precomp=prm["rgb_colors"])
    flips = [(int(c), int(x_), int(y_), "%.1e / %.1e" % (float(a[0][c, y_, x_] - kf["im"][c, y_, x_]), float(b[0][c, y_, x_] - kf["im"][c, y_, x_])))
             for c, y_, x_ in torch.nonzero(torch.sign(a[0] - kf["im"]) != torch.sign(b[0] - kf["im"]))[:4]]
    if flips:
        return "L1 kink", flips
    msk = kf["depth"] > 0
    flips = [(int(x_), int(y_), "%.1e / %.1e" % (float(a[2][0, y_, x_] - kf["depth"][0, y_, x_]), float(b[2][0, y_, x_] - kf["depth"][0, y_, x_])))
             for _, y_, x_ in torch.nonzero((torch.sign(a[2] - kf["depth"]) != torch.sign(b[2] - kf["depth"])) & msk)[:4]]
    if flips:
        return "depth L1 kink", flips
    d = (a[0] - b[0]).abs().amax(0)
    if int((d > 5e-5).sum()):
        ok, c, m, _ = _depth_ties_cover(p["means3D"], pose7, rv0["means3D"].detach(), a[1], d, W, H, 5e-5)
        if ok:
            return "depth tie", "%d pixels differ by more than 5e-5 (max %.1e), all in the footprints of depth-tied pairs" % (m, float(d.max()))
        return None, "%d pixels differ by more than 5e-5 (max %.1e), %d of them in depth-tie footprints" % (m, float(d.max()), c)
    return None, "images equal to 5e-5"


def check_get_loss_random_draw(seed, device):
    """One draw of the loss-call sweep (scripts/exp/fuzz_get_loss.py; profiles/r05_fuzz_get_loss.txt): get_loss as the reference runs it (torch activations -> two raster
    passes through the drop-in GaussianRasterizer -> masked depth L1 + L1 + SSIM in torch; src/mapper/splatam/__init__.py get_loss) against the fully fused form of the same
    call (fused=True, fused_loss=True, fused_preprocess=True: raw-parameter single-pass RGB-D render + gs_mapping_loss) on a random map, ragged image size, pose, random
    targets and a band without depth: loss (2e-5), loss parts (5e-5), seen / max_2D_radius, gradients of the five per-Gaussian parameters (3e-4 relative L2 without the two
    worst rows).  `means2D.grad` differs by design (the fused pass carries the depth term too) and is not compared.
    -> "ok" | (class, key, relative difference, detail) when the two renders differ by a discrete event that _classify_loss_call_difference names | ("rows", ...)."""
    from activesplat_amd import mapping as M
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    dev = device
    r = np.random.RandomState(seed)
    n = int(r.choice([int(r.randint(50, 2000)), int(r.randint(2000, 30000))]))
    W, H = (int(r.randint(24, 200)), int(r.randint(24, 160))) if seed % 3 else (int(r.randint(272, 420)), int(r.randint(256, 330)))
    iso = bool(seed % 2)
    p = syn.make_params(n, W, H, seed=seed)
    if iso:
        p["log_scales"] = p["log_scales"][:, :1].contiguous()
    p["log_scales"] = p["log_scales"] + float(r.uniform(0.0, 1.5))                      # larger splats: a silhouette above 0.99 somewhere
    a = float(r.uniform(-0.3, 0.3))
    q = torch.tensor([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0], dtype=torch.float32)
    t = torch.tensor([r.uniform(-0.2, 0.2), r.uniform(-0.1, 0.1), r.uniform(-0.6, 0.3)], dtype=torch.float32)
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=dev)
    g = torch.Generator().manual_seed(seed)
    kf = dict(cam=cam, id=0, im=torch.rand(3, H, W, generator=g).to(dev), depth=(torch.rand(1, H, W, generator=g) * 3 + 0.5).to(dev), w2c=torch.eye(4, device=dev))
    kf["depth"][0, : H // 7] = 0.0                                                      # a band without depth: the loss' depth mask
    out = []
    for fused in (False, True):
        prm = {k: torch.nn.Parameter(v.clone().to(dev)) for k, v in p.items()}
        prm["cam_unnorm_rots"] = torch.nn.Parameter(q.reshape(1, 4, 1).clone().to(dev))
        prm["cam_trans"] = torch.nn.Parameter(t.reshape(1, 3, 1).clone().to(dev))
        var = {k: torch.zeros(n, device=dev) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
        kw = dict(fused=True, fused_loss=True, fused_preprocess=True) if fused else {}
        loss, var, parts = M.get_loss(prm, kf, var, 0, dict(im=0.5, depth=1.0), **kw)
        loss.backward(M.unit_gradient(loss)) if fused else loss.backward()
        out.append((float(loss.detach()), {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in parts.items()},
                    {k: v.grad.double() for k, v in prm.items() if v.grad is not None and not k.startswith("cam_")}, var["seen"].clone(), var["max_2D_radius"].clone()))
    x, y = out
    verdict = "ok"
    for k in x[2]:
        if iso and k == "unnorm_rotations":
            continue
        e2 = ((x[2][k] - y[2][k]).reshape(n, -1) ** 2).sum(1)
        nr = float(x[2][k].norm().clamp_min(1e-30))
        rest = float((e2.sum() - e2.sort().values[-2:].sum()).clamp_min(0).sqrt()) if n > 8 else 0.0
        if not rest < 3e-4 * nr:
            why, detail = _classify_loss_call_difference(p, q, t, kf, cam, W, H, dev)
            assert why, (k, rest / nr, float(e2.sum().sqrt()) / nr, detail)
            return (why, k, round(rest / nr, 6), detail)
        if not float(e2.sum().sqrt()) < 3e-3 * nr and verdict == "ok":
            verdict = ("rows", k, int(e2.argmax()), round(float(e2.sum().sqrt()) / nr, 5))
    assert abs(x[0] - y[0]) <= 2e-5 * abs(x[0]) + 1e-7, ("loss", x[0], y[0])
    for k in x[1]:
        assert abs(x[1][k] - y[1][k]) <= 5e-5 * abs(x[1][k]) + 1e-7, ("part", k, x[1][k], y[1][k])
    assert int((x[3] != y[3]).sum()) <= 1 + n // 2000 and float((x[4] - y[4]).abs().max()) <= 1.0, ("seen / max radius", int((x[3] != y[3]).sum()), float((x[4] - y[4]).abs().max()))
    return verdict


def check_adam_inside_the_backward(device, n=600, W=64, H=48, steps=3, exact=True, seed=6, pose=None, visible=(0.2, 0.95)):
    """render_rgbd_raw(adam=optimizer) -- the Adam step of the five per-Gaussian tensors inside the per-Gaussian backward kernel
    (gs_render_backward_raw_adam) -- against backward + GaussianAdam.step() (whose arithmetic the golden adam.npz fixture pins): parameters,
    both moments, step counters and means2D.grad after every one of `steps` iterations; colours / 16-coefficient SH rows, anisotropic /
    isotropic maps; about a third of the Gaussians behind the camera (zero gradient: moments decay, parameters still move).
    exact=True (the emulated build on ONE host thread, where the blend backward's atomic sums have a fixed order): BIT for bit.
    exact=False (the device: two runs of the atomics sum in different orders, and Adam turns a gradient at rounding-noise level into a
    step of +-lr): the first moments within 5e-5 relative L2 (the bar the chained / one-walker comparisons of two atomic orders use is
    2e-5 per step), the second within 1e-4, and the parameters equal within 1e-6 of their scale on all but 0.1 % of the elements."""
    from activesplat_amd import optim as O, rasterizer as R
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    pose = pose or [0.9950042, 0.0, 0.0998334, 0.0, 0.03, -0.02, -1.2]
    g = torch.Generator().manual_seed(4)
    dLc, dLd = torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)
    for sh, iso in ((False, False), (False, True), (True, False)):
        p0 = syn.make_params(n, W, H, seed=seed, sh_degree=3 if sh else None)
        if sh:
            p0.pop("rgb_colors")
        if iso:
            p0["log_scales"] = p0["log_scales"][:, :1].contiguous()
        cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, sh_degree=3 if sh else 0)
        lrs = dict(means3D=1e-3, rgb_colors=2.5e-3, shs=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3)
        runs = []
        for fused in (False, True):
            prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p0.items()}
            opt = O.initialize_optimizer(prm, {k: lrs[k] for k in prm})
            hist = []
            for it in range(steps):
                m2d = torch.empty_like(prm["means3D"], requires_grad=True)
                col = dict(shs=prm["shs"]) if sh else dict(colors_precomp=prm["rgb_colors"])
                im, radius, depth, sil, dsq = R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"],
                                                                prm["unnorm_rotations"], pose, adam=opt if fused else None, **col)
                ((im * dLc).sum() + (depth * dLd).sum()).backward()
                if fused:
                    assert all(v.grad is None for v in prm.values())
                opt.step()                                  # (fused: nothing holds a gradient -- a no-op)
                opt.zero_grad(set_to_none=True)
                hist.append(({k: v.detach().clone() for k, v in prm.items()},
                             {k: (opt.state[v]["exp_avg"].clone(), opt.state[v]["exp_avg_sq"].clone(), int(opt.state[v]["step"])) for k, v in prm.items()},
                             m2d.grad.clone(), int((radius > 0).sum())))
            runs.append(hist)
        for it, (a, b) in enumerate(zip(*runs)):
            assert visible[0] * n < a[3] < visible[1] * n, a[3]
            rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))  # noqa: E731
            if exact:
                assert torch.equal(a[2], b[2]), ("means2D.grad", sh, iso, it)
            else:
                assert rel(a[2], b[2]) < 5e-5, ("means2D.grad", sh, iso, it, rel(a[2], b[2]))
            for k in a[0]:
                assert a[1][k][2] == b[1][k][2] == it + 1, (k, sh, iso, it)
                if exact:
                    assert torch.equal(a[0][k], b[0][k]), (k, sh, iso, it, float((a[0][k] - b[0][k]).abs().max()))
                    assert torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1]), (k, sh, iso, it)
                    continue
                if iso and k == "unnorm_rotations":          # equal scales: the rotation's gradient is rounding noise, which Adam amplifies to +-lr
                    continue
                assert rel(a[1][k][0], b[1][k][0]) < 5e-5 and rel(a[1][k][1], b[1][k][1]) < 1e-4, (k, sh, iso, it, rel(a[1][k][0], b[1][k][0]), rel(a[1][k][1], b[1][k][1]))
                d = (a[0][k] - b[0][k]).abs()
                assert float((d > 1e-6 * float(b[0][k].abs().max())).float().mean()) < 1e-3, (k, sh, iso, it, float(d.max()))


def check_adam_backward_guards(device, n=400, W=64, H=48):
    """The in-kernel optimiser step is applied at most once per render and never silently: a second backward through the same graph is
    refused; the stepped parameters' version counters move, so a graph that saved them before the step fails in ITS backward; a launch that fails
    leaves step counters and moments in step."""
    from activesplat_amd import _lib, optim as O, rasterizer as R
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    pose = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    p0 = syn.make_params(n, W, H, seed=2)
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device)
    prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p0.items()}
    opt = O.initialize_optimizer(prm, {k: 1e-3 for k in prm})

    def render():
        m2d = torch.empty_like(prm["means3D"], requires_grad=True)
        return R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], pose, adam=opt,
                                 colors_precomp=prm["rgb_colors"])
    im = render()[0]
    reg = (prm["means3D"] ** 2).sum()                       # another branch that saved the parameter before the step
    v0 = prm["means3D"]._version
    before = prm["means3D"].detach().clone()
    im.sum().backward(retain_graph=True)
    assert prm["means3D"]._version > v0 and not torch.equal(before, prm["means3D"].detach())
    steps = {k: int(opt.state[v]["step"]) for k, v in prm.items()}
    assert set(steps.values()) == {1}
    after = prm["means3D"].detach().clone()
    try:
        im.sum().backward()
        raise AssertionError("a second backward through a stepped render must be refused")
    except RuntimeError as e:
        assert "already applied its optimiser step" in str(e) or "modified by an inplace operation" in str(e), e
    assert torch.equal(after, prm["means3D"].detach()) and {k: int(opt.state[v]["step"]) for k, v in prm.items()} == steps
    try:
        reg.backward()
        raise AssertionError("a graph that saved the parameters before the in-kernel step must not differentiate through stepped values silently")
    except RuntimeError as e:
        assert "modified by an inplace operation" in str(e), e
    # a failing launch: the step counters are rolled back
    im = render()[0]
    real = _lib.check

    def failing(code):
        raise RuntimeError("injected launch failure")
    _lib.check = failing
    try:
        try:
            im.sum().backward()
            raise AssertionError("the injected failure must surface")
        except RuntimeError as e:
            assert "injected launch failure" in str(e)
    finally:
        _lib.check = real
    assert {k: int(opt.state[v]["step"]) for k, v in prm.items()} == steps
    im = render()[0]
    im.sum().backward()
    assert set(int(opt.state[v]["step"]) for v in prm.values()) == {2}
    # a refusal BEFORE the launch (entry 1 of the five already holds a gradient): no counter moves -- not even entry 0's -- and the SAME graph can
    # be retried once the cause is gone
    im = render()[0]
    prm["logit_opacities"].grad = torch.zeros_like(prm["logit_opacities"])
    try:
        im.sum().backward(retain_graph=True)
        raise AssertionError("a parameter that already holds a gradient must be refused")
    except RuntimeError as e:
        assert "already holds a gradient" in str(e), e
    assert set(int(opt.state[v]["step"]) for v in prm.values()) == {2}
    prm["logit_opacities"].grad = None
    im.sum().backward()
    assert set(int(opt.state[v]["step"]) for v in prm.values()) == {3}


class poisoned_empty:
    """Every float tensor torch.empty / empty_like hands out inside the block is filled with NaN: a row the product path allocates uninitialised
    and then does not write shows up as NaN instead of as whatever the allocator's block held before."""

    def __enter__(self):
        self.real = (torch.empty, torch.empty_like)

        def poison(fn):
            def f(*a, **k):
                t = fn(*a, **k)
                if t.is_floating_point() and t.numel():
                    t.detach().fill_(float("nan"))
                return t
            return f
        torch.empty, torch.empty_like = poison(self.real[0]), poison(self.real[1])
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self.real
        return False


def check_unrendered_rows_are_written(device, n=512, W=64, H=48):
    """Keyframe batches (raw parameters, gradients added into .grad in the kernel): a wavefront none of whose Gaussians was rendered leaves the
    per-Gaussian backward early -- and must still write its rows of dL/dmeans2D, which is not accumulated and which the host allocates
    uninitialised (256 / 256 unseen rows were NaN in a NaN-prefilled buffer).  Rows n/2.. lie behind the camera; colours and SH rows;
    every float allocation of the call is poisoned with NaN."""
    from activesplat_amd import mapping as M
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    for sh in (False, True):
        p0 = syn.make_params(n, W, H, seed=4)
        p0["means3D"][n // 2:, 2] = -p0["means3D"][n // 2:, 2]                   # whole wavefronts of unseen Gaussians
        if sh:
            g = torch.Generator().manual_seed(8)
            shs = 0.2 * torch.randn(n, 16, 3, generator=g)
            shs[:, 0, :] = (p0.pop("rgb_colors") - 0.5) / 0.28209479177387814
            p0["shs"] = shs
        cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device, sh_degree=3 if sh else 0)
        prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p0.items()}
        prm["cam_unnorm_rots"] = torch.nn.Parameter(torch.tensor([1.0, 0, 0, 0], device=device).reshape(1, 4, 1))
        prm["cam_trans"] = torch.nn.Parameter(torch.zeros(1, 3, 1, device=device))
        var = {k: torch.zeros(n, device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
        tim, tdepth = syn.make_targets(W, H)
        kf = dict(cam=cam, im=tim.to(device), depth=tdepth.to(device), id=0, w2c=torch.eye(4, device=device))
        for step in range(2):                                   # step 0 creates the .grad tensors, step 1 accumulates into them (acc = 1: the gated path)
            with poisoned_empty():
                loss, var, _ = M.get_loss(prm, kf, var, 0, dict(im=0.5, depth=1.0), fused=True, fused_loss=True, fused_inputs=True, fused_preprocess=True,
                                          pose7=[1.0, 0, 0, 0, 0, 0, 0], accumulate_grads=True)
                loss.backward()
            g2 = var["means2D"].grad
            assert g2 is not None and bool(torch.isfinite(g2).all()), (sh, step, int((~torch.isfinite(g2)).any(dim=1).sum()))
            seen = var["seen"]
            assert int(seen[n // 2:].sum()) == 0 and int(seen[:n // 2].sum()) > 0
            assert float(g2[n // 2:].abs().max()) == 0.0 and float(g2[:n // 2].abs().max()) > 0.0
            for k, v in prm.items():
                if not k.startswith("cam_"):
                    assert v.grad is not None and bool(torch.isfinite(v.grad).all()), (k, sh, step)
                    assert float(v.grad[n // 2:].abs().max()) == 0.0, (k, sh, step)


def check_unrendered_rows_of_dense_gradients(device):
    """The dense gradient outputs of the drop-in call and of the raw-parameter entry (nothing accumulated): with every float allocation of the call
    poisoned with NaN (the Python twin of the front-end allocates through torch.empty) every gradient is finite and the row of a Gaussian the frame did
    not render is exactly zero in every output.  Colours, 16- and 9-coefficient SH rows, a precomputed covariance, ragged Gaussian counts, a scene none
    of whose Gaussians is rendered, whole wavefronts of unrendered rows as well as scattered ones, images on both sides of the few-tile threshold."""
    from activesplat_amd import rasterizer as R
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    was = R.use_frontend
    R.use_frontend = False
    try:
        for name, n_over in (("basic", None), ("sh3", None), ("sh2_ragged", None), ("cov3d_precomp", None), ("all_culled", None), ("one_gaussian", None),
                             ("basic", 511), ("basic", 513), ("sh3", 1025), ("mixed_sizes", None)):
            rs, rv = build_case(name, device)
            if n_over:
                rv = {k: v[:n_over].contiguous() for k, v in rv.items()}
            n = rv["means3D"].shape[0]
            if name != "all_culled" and n > 8:
                rv = {k: v.clone() for k, v in rv.items()}
                rv["means3D"][n // 3:n // 3 + min(200, n // 4), 2] = -1.0
            H, W = int(rs.image_height), int(rs.image_width)
            dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(11))
            with poisoned_empty():
                res = util.run_product(rs, rv, dL)
            dead = res["radii"] <= 0
            assert name == "all_culled" or dead.any() or n <= 8, (name, "no unrendered row in the case")
            for k, g in res["grads"].items():
                assert np.isfinite(g).all(), (name, n_over, k, int((~np.isfinite(g)).sum()))
                assert not dead.any() or float(np.abs(g[dead]).max()) == 0.0, (name, n_over, k)
        for iso, (W, H), n in ((False, (64, 48), 700), (True, (64, 48), 700), (False, (288, 272), 3000)):
            p = syn.make_params(n, W, H, seed=21)
            if iso:
                p["log_scales"] = p["log_scales"][:, :1].contiguous()
            p["means3D"][n // 2:n // 2 + 150, 2] = -p["means3D"][n // 2:n // 2 + 150, 2]
            cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device)
            g = torch.Generator().manual_seed(5)
            dLc, dLd = torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)
            prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p.items()}
            with poisoned_empty():
                m2d = torch.empty_like(prm["means3D"], requires_grad=True)
                im, radius, depth, sil, dsq = R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"],
                                                                [1.0, 0, 0, 0, 0, 0, 0], colors_precomp=prm["rgb_colors"])
                ((im * dLc).sum() + (depth * dLd).sum()).backward()
            dead = radius.cpu() <= 0
            assert bool(dead.any()) and not bool(dead.all())
            for k, gk in dict({k: v.grad.cpu() for k, v in prm.items()}, means2D=m2d.grad.cpu()).items():
                assert bool(torch.isfinite(gk).all()), (iso, W, k)
                assert float(gk[dead].abs().max()) == 0.0, (iso, W, k)
    finally:
        R.use_frontend = was


def check_mapping_iteration_without_autograd(device, n=500, exact=True):
    """mapping.mapping_iteration (the iteration's four library calls issued directly) against get_loss(fused..., fused_adam=) + backward + step +
    zero_grad through autograd: parameters, moments, loss, means2D.grad, seen, max_2D_radius after three iterations on three keyframes;
    anisotropic and isotropic maps.  exact: bit for bit (emulated kernels on one host thread); else to the order of the atomic sums."""
    from activesplat_amd import mapping as M, optim as O
    from tests.test_parallel import _scene
    lrs = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)
    for iso in (False, True):
        outs = []
        for direct in (False, True):
            params, kfs = _scene(n=n, device=device)
            if iso:
                params["log_scales"] = torch.nn.Parameter(params["log_scales"].detach()[:, :1].clone())
            nn_ = params["means3D"].shape[0]
            var = {k: torch.zeros(nn_, device=device) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
            opt = O.initialize_optimizer(params, lrs)
            for it in range(3):
                kf = kfs[it]
                if direct:
                    loss, var, parts = M.mapping_iteration(params, kf, var, kf["id"], dict(im=0.5, depth=1.0), opt)
                    assert all(p.grad is None for p in params.values())
                else:
                    loss, var, parts = M.get_loss(params, kf, var, kf["id"], dict(im=0.5, depth=1.0), fused=True, fused_loss=True, fused_preprocess=True,
                                                  fused_adam=opt)
                    loss.backward(M.unit_gradient(loss))
                    with torch.no_grad():
                        opt.step(); opt.zero_grad(set_to_none=True)
            outs.append(({k: v.detach().clone() for k, v in params.items()},
                         {k: (opt.state[v]["exp_avg"].clone(), int(opt.state[v]["step"])) for k, v in params.items() if v in opt.state and len(opt.state[v])},
                         var["means2D"].grad.clone(), var["seen"].clone(), var["max_2D_radius"].clone(), float(loss.detach()), float(parts["im"])))
        a, b = outs
        assert abs(a[5] - b[5]) <= (0.0 if exact else 1e-6 * abs(a[5])) and abs(a[6] - b[6]) <= (0.0 if exact else 1e-6 * abs(a[6]))
        assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
        for k in a[1]:
            assert a[1][k][1] == b[1][k][1] == 3, k
        if exact:
            assert torch.equal(a[2], b[2])
            assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and all(torch.equal(a[1][k][0], b[1][k][0]) for k in a[1])
        else:
            rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))  # noqa: E731
            assert rel(a[2], b[2]) < 5e-5
            for k in a[1]:
                if iso and k == "unnorm_rotations":
                    continue
                assert rel(a[1][k][0], b[1][k][0]) < 5e-5, (k, rel(a[1][k][0], b[1][k][0]))


def check_few_tile_backward_segments(device, oracle64, oracle32=None, N=20000, W=64, H=48, seed=41):
    """Images of at most 256 tiles: the backward walks every quadrant's list in 3 (default), 2 or 1 segments on as many wavefronts, the
    front ones resuming from the per-pixel state the forward recorded (every 256th list position up to 4096, powers of two beyond).  A scene
    of faint splats whose quadrants reach ~1-4 k list positions deep, so that cuts at thirds exist: forward outputs identical for every
    setting, gradients equal to the one-walker kernel's up to the order of the sums, the fp64 oracle, and the fused RGB-D variant."""
    from activesplat_amd import _lib
    lib = _lib.get()
    rs, rv = util.scene(N, W, H, seed=seed, device=device, scale_jitter=0.4)
    rs = rs._replace(debug=False)
    rv["opacities"] = (rv["opacities"] * 0.03).clamp(0, 1)
    rv["scales"] = rv["scales"] * 2.0
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3))
    try:
        _lib.check(lib.gs_set_backward_segments(1))
        ref = util.run_product(rs, rv, dL)
        art = util.artefacts()
        deep = int(art["n_contrib"].max())
        assert deep >= 3 * 256, deep                              # deep enough for two cuts
        assert int(util.LAST["bl"].segments) == 1                 # (not the segmented forward of very long lists: it records nothing)
        for segs in (2, 3):
            _lib.check(lib.gs_set_backward_segments(segs))
            got = util.run_product(rs, rv, dL)
            for k in ("color", "depth", "opacity", "radii"):
                assert np.array_equal(got[k], ref[k]), (segs, k)
            for k, g in got["grads"].items():
                r = ref["grads"][k]
                assert np.isfinite(g).all(), (segs, k)
                assert np.linalg.norm(g.astype(np.float64) - r) <= 3e-5 * max(np.linalg.norm(r), 1e-30), (segs, k, np.linalg.norm(g - r) / np.linalg.norm(r))
        check_backward(rs._replace(debug=True), rv, oracle64, seed=3, oracle32=oracle32)
        # the fused RGB-D backward (depth gradient through the same segments): three segments against one walker
        from activesplat_amd import rasterizer as R
        g = torch.Generator().manual_seed(5)
        dLc, dLd = torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)
        both = []
        for segs in (1, 3):
            _lib.check(lib.gs_set_backward_segments(segs))
            inp = {k: v.detach().clone().requires_grad_(True) for k, v in rv.items()}
            m2d = torch.zeros(N, 3, device=device, requires_grad=True)
            color, radii, depth, sil, dsq = R.render_rgbd(rs, means2D=m2d, **inp)
            ((color * dLc).sum() + (depth * dLd).sum()).backward()
            both.append({**{k: v.grad.detach().double() for k, v in inp.items()}, "means2D": m2d.grad.detach().double()})
        for k in both[0]:
            assert float((both[1][k] - both[0][k]).norm() / both[0][k].norm().clamp_min(1e-30)) <= 3e-5, k
        if N <= 30000:
            check_fused_rgbd(rs, rv, oracle64)
    finally:
        _lib.check(lib.gs_set_backward_segments(3))


def check_chained_backward(device, oracle64, N=5000, W=288, H=272, oracle32=None, seed=33):
    """Images of more than 768 tiles walk every quadrant's list in three chained pieces (gs_set_backward_chain): here the threshold is
    lowered so that a 306-tile image takes that path, with splats large and faint enough for walks of several 64-record chunks; against
    the one-walker kernel (forward identical, gradients equal up to the order of the atomic sums) and against the fp64 oracle."""
    from activesplat_amd import _lib
    lib = _lib.get()
    rs, rv = util.scene(N, W, H, seed=seed, device=device, scale_jitter=0.5)
    rs = rs._replace(debug=False)
    rv["opacities"] = (rv["opacities"] * 0.15).clamp(0, 1)
    rv["scales"] = rv["scales"] * 3.0
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(7))
    try:
        _lib.check(lib.gs_set_backward_chain(1, -1))
        ref = util.run_product(rs, rv, dL)
        _lib.check(lib.gs_set_backward_chain(3, 256))
        got = util.run_product(rs, rv, dL)
        for k in ("color", "depth", "opacity", "radii"):
            assert np.array_equal(got[k], ref[k]), k
        for k, g in got["grads"].items():
            r = ref["grads"][k]
            assert np.isfinite(g).all(), k
            assert np.linalg.norm(g.astype(np.float64) - r) <= 2e-5 * max(np.linalg.norm(r), 1e-30), (k, np.linalg.norm(g - r) / np.linalg.norm(r))
        check_backward(rs._replace(debug=True), rv, oracle64, seed=7, oracle32=oracle32)
    finally:
        _lib.check(lib.gs_set_backward_chain(3, -1))


def check_chained_backward_fails_safe(device, N=5000, W=288, H=272, seed=33):
    """VERDICT r4 item 6.  (a) ordered tickets on / off give the same gradients (the arithmetic per pixel is the same sequence); (b) a wait that
    runs out (provoked: gs_set_backward_chain_polls(-2)) raises the host-visible status word: the next render raises, chaining is off afterwards
    and the frame rendered again is right; nothing hangs."""
    from activesplat_amd import _lib
    lib = _lib.get()
    rs, rv = util.scene(N, W, H, seed=seed, device=device, scale_jitter=0.5)
    rs = rs._replace(debug=False)
    rv["opacities"] = (rv["opacities"] * 0.15).clamp(0, 1)
    rv["scales"] = rv["scales"] * 3.0
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(7))
    sync = (lambda: torch.cuda.synchronize()) if device != "cpu" else (lambda: None)
    try:
        _lib.check(lib.gs_set_backward_chain(3, 256)); _lib.check(lib.gs_set_backward_chain_tickets(0))
        plain = util.run_product(rs, rv, dL)
        _lib.check(lib.gs_set_backward_chain_tickets(1))
        tick = util.run_product(rs, rv, dL)
        tick2 = util.run_product(rs, rv, dL)                      # (a second launch: the last drawer put the counters back)
        for k, g in tick["grads"].items():
            for other in (plain, tick2):
                r = other["grads"][k]
                assert np.isfinite(g).all() and np.linalg.norm(g.astype(np.float64) - r) <= 2e-5 * max(np.linalg.norm(r), 1e-30), k
        # (b) the timeout path
        _lib.poll_async_status()
        _lib.check(lib.gs_set_backward_chain_polls(-2))
        bad = util.run_product(rs, rv, dL)
        sync()
        assert not all(np.isfinite(g).all() for g in bad["grads"].values())      # NaN state went through the pieces behind the first
        # (c) the host has not looked yet (the backward is asynchronous: it learns of the event in front of the NEXT render) -- optimiser steps
        # enqueued behind the failed backward must leave parameters and moments alone: the separate step ...
        from activesplat_amd import optim as O, rasterizer as R
        from activesplat_amd import synthetic as syn
        w = torch.nn.Parameter(torch.randn(1001, 3, generator=torch.Generator().manual_seed(1)).to(device))
        o1 = O.initialize_optimizer({"means3D": w}, {"means3D": 1e-2})
        w.grad = torch.full_like(w, float("nan"))
        w0 = w.detach().clone()
        o1.step(); sync()
        assert torch.equal(w0, w.detach()) and float(o1.state[w]["exp_avg"].abs().max()) == 0.0, "Adam stepped on the gradients of a timed-out backward"
        # ... and the step INSIDE a backward whose own blend times out (same launch sequence: nobody could have intervened)
        p0 = syn.make_params(N, W, H, seed=seed)
        prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in p0.items()}
        o2 = O.initialize_optimizer(prm, {k: 1e-2 for k in prm})
        m2d = torch.empty_like(prm["means3D"], requires_grad=True)
        _lib._status[0] = 0                                      # (this render's poll must pass: the event under test is the one its OWN backward raises)
        im = R.render_rgbd_raw(rs, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"],
                               [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], adam=o2, colors_precomp=prm["rgb_colors"])[0]
        im.backward(dL.to(device)); sync()
        for k, v in prm.items():
            assert torch.equal(v.detach().cpu(), p0[k]), k
            assert float(o2.state[v]["exp_avg"].abs().max()) == 0.0 and float(o2.state[v]["exp_avg_sq"].abs().max()) == 0.0, k
        assert float(m2d.grad.abs().max()) == 0.0
        try:
            util.run_product(rs, rv, dL)
            raise AssertionError("the render after a timed-out chained backward must raise")
        except RuntimeError as e:
            assert "timed out" in str(e) and "SKIPPED" in str(e), e
        # reported and cleared: steps run again
        w.grad = torch.ones_like(w)
        o1.step(); sync()
        assert not torch.equal(w0, w.detach())
        _lib.check(lib.gs_set_backward_chain_polls(-1))
        again = util.run_product(rs, rv, dL)                       # chaining is off now (one walker per quadrant): finite and equal
        sync()
        _lib.poll_async_status()
        for k, g in again["grads"].items():
            r = plain["grads"][k]
            assert np.isfinite(g).all() and np.linalg.norm(g.astype(np.float64) - r) <= 2e-5 * max(np.linalg.norm(r), 1e-30), k
    finally:
        _lib.check(lib.gs_set_backward_chain_polls(-1)); _lib.check(lib.gs_set_backward_chain_tickets(0))
        _lib.check(lib.gs_set_backward_chain(3, -1))
        if _lib._status is not None:
            _lib._status[0] = 0


#: tally of check_backward's fp32 escape hatch over the session (printed by tests/conftest.py); "decisions": how often the third tier -- the
#: comparison against the oracles run with the other decision at a PROVEN alpha = 1/255 threshold pixel -- decided
HATCH = {"keys_checked": 0, "fired": 0, "where": [], "decisions": 0, "decision_where": []}

#: relative half-width of the window around 1/255 inside which a visibility decision may legitimately differ between two fp32 evaluation orders
#: of alpha = o exp(power): the per-Gaussian record (pixel mean, conic) is fp32, so `power` carries an absolute error of a few 1e-6 at the rim of a footprint
#: -- and more where the exponent's terms are large (threshold_gaussians widens the window of such a pixel to 4 (eps / 2) x the sum of the terms' magnitudes)
THRESHOLD_WINDOW = 1e-5


def threshold_gaussians(f64, idx, W, H, window=THRESHOLD_WINDOW):
    """Those of the Gaussians `idx` that own a pixel whose alpha -- fp64, from the fp64 oracle's per-Gaussian record `f64` -- lies within `window`
    (relative) of the 1/255 visibility threshold: a pixel that one arithmetic blends and another skips (one alpha = 1/255 step of gradient apart).
    -> list of (gaussian, x, y, 255 alpha - 1)."""
    xy, co, radii = f64["xy"], f64["conic_opacity"], f64["radii"]
    out = []
    for i in idx:
        i = int(i); rad = int(radii[i])
        if rad <= 0:
            continue
        x0, x1 = max(0, int(xy[i, 0]) - rad - 1), min(W, int(xy[i, 0]) + rad + 2)
        y0, y1 = max(0, int(xy[i, 1]) - rad - 1), min(H, int(xy[i, 1]) + rad + 2)
        if x1 <= x0 or y1 <= y0:
            continue
        px, py = np.meshgrid(np.arange(x0, x1, dtype=np.float64), np.arange(y0, y1, dtype=np.float64))
        dx, dy = xy[i, 0] - px, xy[i, 1] - py
        power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
        a255 = np.where(power > 0, 0.0, np.minimum(0.99, co[i, 3] * np.exp(np.minimum(power, 0.0)))) * 255.0 - 1.0
        # the window of a pixel: `window`, or -- where that is more -- what an fp32 evaluation of the exponent can be off by THERE: its three terms are
        # formed and added in ~4 roundings of quantities bounded by S = |a| dx^2 / 2 + |c| dy^2 / 2 + |b dx dy|, i.e. |d power| <= 4 (eps / 2) S, and
        # d alpha / alpha = d power.  (Round 6, seed 142045 of the sweeps: a radius-61 splat with terms of 22 + 36 + 55 at the pixel, 255 alpha - 1 =
        # +1.06e-5 -- the kernel skips it, both oracles blend it, 94-97 % of three tensors' error in that one row; the fixed 1e-5 window missed it by 6 %.)
        S = 0.5 * np.abs(co[i, 0]) * dx * dx + 0.5 * np.abs(co[i, 2]) * dy * dy + np.abs(co[i, 1] * dx * dy)
        win = np.maximum(window, 4.0 * 0.5 * 1.1920929e-07 * S)
        ratio = np.abs(a255) / win
        j = int(np.argmin(ratio))
        if ratio.flat[j] < 1.0:
            out.append((i, int(px.flat[j]), int(py.flat[j]), float(a255.flat[j])))
    return out


def alpha255_at(rec, i, x, y):
    """255 alpha - 1 of Gaussian i at pixel (x, y), evaluated in fp64 from the per-Gaussian record of an oracle's forward (`rec`: the fp64 oracle's, or the
    fp32 oracle's -- the record both fp32 evaluations share)."""
    xy, co = np.asarray(rec["xy"], np.float64), np.asarray(rec["conic_opacity"], np.float64)
    dx, dy = xy[i, 0] - float(x), xy[i, 1] - float(y)
    power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
    return (0.0 if power > 0 else min(0.99, co[i, 3] * np.exp(min(power, 0.0)))) * 255.0 - 1.0


#: margin by which the oracle's threshold factor of a proven Gaussian is moved past its alpha (relative): above the few 1e-6 by which two fp32
#: evaluation orders of alpha differ, below the 1e-5 window of the proof
DECISION_MARGIN = 5e-6


def decision_aware(k, g, f64, W, H, rerun, oracle64, oracle32, min_frac=None, top=3):
    """Third tier of the gradient rule: the DECISION-MATCHED comparison.  `g` [P, ...] is one gradient tensor of the kernel that
    failed both the fp64 bar and the fp32-oracle rule.  Among the `top` Gaussians that carry most of its squared error, those that provably own a pixel
    at the alpha = 1/255 threshold (threshold_gaussians) are candidates for "the kernel's arithmetic took the other decision there".  For every
    non-empty subset of them the two oracles are run AGAIN with the visibility threshold of exactly those Gaussians moved past their alpha
    (gso_set_threshold_scale: by the distance of alpha to the threshold plus 5e-6) -- the same algorithm with the kernel's decision at those
    pixels -- and the WHOLE tensor is judged by tiers 1 and 2 against those references: nothing is excluded, and the side effects of the flipped pixel
    on every other Gaussian that blends there (their transmittance and behind-colour change by alpha = 1/255) are part of the reference.
    `rerun(oracle) -> {key: gradient}` repeats the caller's oracle run.  Returns True when a subset passes (tallied), False otherwise."""
    import itertools
    P = g.shape[0]
    key = k.split(" ")[0]                                     # ("means3D (fused RGB-D)" -> the oracle's key)
    r = np.asarray(rerun.base64[key], np.float64).reshape(g.shape)
    e = ((g.astype(np.float64) - r).reshape(P, -1) ** 2).sum(1)
    worst = np.argsort(-e)[:top]
    proven = threshold_gaussians(f64, worst, W, H)
    # ... or at the threshold by the fp32 ORACLE's record -- the pixel mean and conic that both fp32 evaluations (oracle and kernel) start from.  The fp64
    # record's pixel mean may sit 3e-5 px away from it (a projection in fp32 at depth 0.5), which moves alpha by 3e-5: seed 210541 of the round-6 soak,
    # Gaussian 23255 at pixel (179, 9): fp64 -3.04e-5, the fp32 oracle's arithmetic -1.8e-7 (skips), the kernel's +4.2e-7 (blends).
    f32 = getattr(rerun, "fwd32", None)
    # a candidate = (Gaussian, pixel, 255 alpha - 1 by the proving record, the decision to impose on BOTH oracles: +1 skip / -1 blend).  Proven by the fp64
    # record: the other decision than that oracle's own.  Proven by the fp32 record only: either one -- the fp32 oracle's own decision there is a matter
    # of its last bits (fp64 arithmetic on its record says +2.8e-7 where its fp32 arithmetic says -1.8e-7), so both are tried.
    options = [[(i, x, y, d, 1 if d >= 0 else -1)] for i, x, y, d in proven]
    if f32 is not None:
        have = {i for i, _, _, _ in proven}
        options += [[(i, x, y, d, 1), (i, x, y, d, -1)] for i, x, y, d in threshold_gaussians(f32, worst, W, H) if i not in have]
    # a decision an earlier tensor of the same backward was matched with is tried first: the flipped pixel moves T and the behind-colour of every Gaussian
    # blended there, and in a tensor like dL/dopacity the threshold's owner itself (alpha = 1/255) need not be among the rows that carry the error (seed
    # 400746 of the emulated sweep: means3D matched through Gaussian 67 at pixel (7, 31); the five opacity rows that differ are the Gaussians behind it)
    known = list(getattr(rerun, "decided", []))
    if not options and not known:
        return False
    subsets = known + [c for n in range(len(options), 0, -1) for grp in itertools.combinations(options, n) for c in itertools.product(*grp)]
    try:
        # The decision is imposed through the Gaussian's threshold, i.e. on every pixel of it whose alpha lies between the threshold and the moved one:
        # a Gaussian with TWO pixels within the margin (seed 400746 of the emulated sweep: Gaussian 67 at (7, 31), -8.5e-7, where the kernel blends, and
        # at (33, 29), where it skips like the oracles) needs a move that stops between them -- the narrower margins are tried after the default one.
        for combo5, margin in [(c, m) for c in subsets for m in (DECISION_MARGIN, 1e-6, 2.5e-7)]:
            combo = [(i, x, y, d) for i, x, y, d, _ in combo5]
            scale = np.ones(P)
            for i, x, y, d, mode in combo5:
                # past whichever of the two oracles' alphas lies further in the imposed direction
                ds = [alpha255_at(f64, i, x, y)] + ([alpha255_at(f32, i, x, y)] if f32 is not None else [])
                scale[i] = 1.0 + (max(ds) + margin if mode > 0 else min(ds) - margin)
            oracle64.set_threshold_scale(scale); oracle32.set_threshold_scale(scale)
            r2 = np.asarray(rerun(oracle64)[key], np.float64).reshape(g.shape)
            o2 = np.asarray(rerun(oracle32)[key], np.float64).reshape(g.shape)
            nr = max(np.linalg.norm(r2), 1e-30); gmax = float(np.abs(r2).max())
            rel, rel32 = np.linalg.norm(g - r2) / nr, np.linalg.norm(o2 - r2) / nr
            ok = rel < 1e-3 or rel <= 1.5 * rel32 + 1e-6
            if min_frac is not None:
                frac, frac32 = util.close_frac(g, r2, GRAD_RTOL, 1e-6 * gmax), util.close_frac(o2, r2, GRAD_RTOL, 1e-6 * gmax)
                ok = ok and (frac >= min_frac or (1.0 - frac) <= 1.5 * (1.0 - frac32) + 1e-3)
            if ok:
                if hasattr(rerun, "decided") and tuple(combo5) not in rerun.decided:
                    rerun.decided.append(tuple(combo5))
                HATCH["decisions"] += 1
                HATCH["decision_where"].append((k, [(i, x, y, d) for i, x, y, d in combo], float(rel), float(rel32)))
                print(f"decision-matched comparison for {k}: with the oracle's decision flipped at {[(i, (x, y), f'{d:+.1e}') for i, x, y, d in combo]} "
                      f"(Gaussian, pixel, 255 alpha - 1): rel {rel:.3e}, fp32 oracle {rel32:.3e}")
                return True
        return False
    finally:
        oracle64.set_threshold_scale(None); oracle32.set_threshold_scale(None)


class _Rerun:
    """callable that repeats an oracle run for decision_aware; `base64`: the fp64 oracle's gradients of the undisturbed run"""

    def __init__(self, fn, base64, fwd32=None):
        self.fn, self.base64, self.fwd32 = fn, base64, fwd32        # fwd32: the fp32 oracle's forward (its per-Gaussian record), if the caller has it
        self.decided = []                                            # decisions earlier tensors of this backward were matched with

    def __call__(self, oracle):
        return self.fn(oracle)


def check_forward(rs, rv, oracle32, exact_float=False, oracle64=None):
    """oracle64 (the sweeps of scripts/exp only): an image that misses the tolerance against the fp32 oracle is judged like a gradient of tier 2 --
    against the fp64 oracle, where it must be no further out than the fp32 oracle itself is.  (Strongly anisotropic splats: the quadratic form of
    the exponent is a difference of large products, and two fp32 evaluation orders of it differ by more than the tolerance -- on such scenes the
    kernel is usually CLOSER to fp64 than the fp32 oracle, `scripts/exp/fwd_hard.py`.)  The suite's calls do not pass it: there the bar is the plain one."""
    got = util.run_product(rs, rv)
    art = util.artefacts()
    ref = util.run_oracle(oracle32, rs, rv)
    # ---- integer artefacts: bit-exact ----
    assert got["D"] == ref["D"]
    assert np.array_equal(got["radii"], ref["radii"])
    live = ref["radii"] > 0
    assert np.array_equal(art["tiles_touched"], ref["tiles_touched"])
    assert np.array_equal(art["rect"][live], ref["rect"][live])
    if art["offsets"] is not None:                     # radix-sort path only
        assert np.array_equal(art["offsets"], ref["offsets"])
    else:
        assert np.array_equal(art["pairs_ids"], art["point_list"])
    assert np.array_equal(art["keys_sorted"], ref["keys_sorted"])
    assert np.array_equal(art["point_list"], ref["ids_sorted"])
    rg = art["ranges"].copy()
    rg[rg[:, 0] == rg[:, 1]] = 0                       # an empty tile is [s,s) on the scan path, [0,0) in the oracle
    assert np.array_equal(rg, ref["ranges"])
    # per-Gaussian floats produced by the contraction-free TU are bit-exact too
    assert np.array_equal(art["geom"][live, 0:2], ref["xy"][live])
    assert np.array_equal(art["geom"][live, 9], ref["depth"][live])
    assert np.array_equal(art["geom"][live][:, [2, 3, 4, 5]], ref["conic_opacity"][live])
    # ---- images ----
    for k_got, k_ref in (("color", "color"), ("depth", "out_depth"), ("opacity", "opacity")):
        a, b = got[k_got], ref[k_ref]
        assert np.isfinite(a).all() and np.isfinite(b).all(), k_got        # (non-finite inputs are culled: DESIGN.md section 2)
        if exact_float:
            assert np.array_equal(a, b), k_got
        else:
            scale = max(1.0, float(np.abs(b).max()))
            # >= 99.9 % of the values inside the tolerance; on tiny images (a few hundred pixels) two pixels' worth of
            # alpha = 1/255 / T = 1e-4 threshold flips are allowed instead (each bounded by the 0.02 limit below)
            n_bad = int(round((1.0 - util.close_frac(a, b, FWD_RTOL, FWD_ATOL * scale)) * a.size))
            allowed = max(0.001 * a.size, 6 if k_got == "color" else 2)
            if n_bad > allowed and oracle64 is not None:
                ref64 = util.run_oracle(oracle64, rs, rv) if "_ref64" not in got else got["_ref64"]
                got["_ref64"] = ref64
                c = np.asarray(ref64[k_ref], np.float64).reshape(a.shape)
                bad_k = int(round((1.0 - util.close_frac(a, c, FWD_RTOL, FWD_ATOL * scale)) * a.size))
                bad_o = int(round((1.0 - util.close_frac(b, c, FWD_RTOL, FWD_ATOL * scale)) * a.size))
                HATCH["forward_fired"] = HATCH.get("forward_fired", 0) + 1
                assert bad_k <= 1.5 * bad_o + allowed, (k_got, n_bad, bad_k, bad_o, a.size)
            else:
                assert n_bad <= allowed, (k_got, n_bad, a.size)
            assert np.abs(a - b).max() <= 0.02 * scale, k_got
    # PSNR >= 60 dB; an image of a few hundred pixels is exempt (one threshold-flipped pixel of 0.02 in 500 pixels is 58 dB --
    # those are bounded by the per-value checks above)
    assert got["color"].size < 3 * 4096 or util.psnr(got["color"], ref["color"]) >= 60.0, util.psnr(got["color"], ref["color"])
    nc_equal = np.mean(art["n_contrib"] == ref["n_contrib"])
    assert nc_equal == 1.0 if exact_float else nc_equal >= 0.999
    return got, ref


def check_backward(rs, rv, oracle64, seed=0, min_frac=0.995, oracle32=None):
    """Gradients vs the fp64 oracle at the stated fp32 tolerance.  With `oracle32`, a key that misses the tolerance is still
    accepted when the fp32 ORACLE misses it by as much (ill-conditioned scenes: the limit is the arithmetic, not the kernel):
    the kernel's error must then stay within 1.5x the fp32 oracle's own error against fp64.  Third tier (decision_aware): when the miss sits in at
    most three Gaussians that provably own a pixel whose alpha is within 1e-5 of the 1/255 visibility threshold (one arithmetic blends it, another
    skips it), the oracles are run again with the OTHER decision at those pixels and the whole tensor is judged by the first two tiers against them."""
    H, W = int(rs.image_height), int(rs.image_width)
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed))
    got = util.run_product(rs, rv, dL)
    ref = util.run_oracle(oracle64, rs, rv, dL)
    ref32 = None
    decided = []                                                # decisions the third tier matched earlier tensors of this backward with (decision_aware)
    for k, g in got["grads"].items():
        r = ref["grads"][k].reshape(g.shape)
        gmax = float(np.abs(r).max())
        if gmax == 0.0:
            assert np.abs(g).max() == 0.0, k
            continue
        assert np.isfinite(g).all(), k
        frac = util.close_frac(g, r, GRAD_RTOL, 1e-6 * gmax)
        rel = np.linalg.norm(g.astype(np.float64) - r) / np.linalg.norm(r)
        HATCH["keys_checked"] += 1
        # (a tensor of fewer than 400 elements -- scenes of 1 ... 130 Gaussians in the random sweeps -- cannot express 99.5 %: one element is
        # more than 0.5 % of it.  There the bar is "at most two elements outside the tolerance"; the relative L2 bar is unchanged)
        if g.size < 400 and round((1.0 - frac) * g.size) <= 2:
            frac = max(frac, min_frac)
        if (frac < min_frac or rel >= 1e-3) and oracle32 is not None:
            # logged: how often the stated tolerance is missed and the fp32-oracle comparison decides instead (conftest prints the tally)
            HATCH["fired"] += 1
            HATCH["where"].append((k, float(rel), float(frac), int(g.shape[0])))
            print(f"check_backward: fp32 escape hatch for {k}: rel {rel:.3e}, frac {frac:.5f} (P = {g.shape[0]})")
            ref32 = util.run_oracle(oracle32, rs, rv, dL) if ref32 is None else ref32
            o = ref32["grads"][k].reshape(g.shape).astype(np.float64)
            rel32 = np.linalg.norm(o - r) / np.linalg.norm(r)
            frac32 = util.close_frac(o, r, GRAD_RTOL, 1e-6 * gmax)
            if not (rel <= 1.5 * rel32 + 1e-6 and (1.0 - frac) <= 1.5 * (1.0 - frac32) + 1e-3):
                rerun = _Rerun(lambda orc: util.run_oracle(orc, rs, rv, dL)["grads"], ref["grads"], fwd32=ref32)
                rerun.decided = decided
                assert decision_aware(k, g, ref, W, H, rerun, oracle64, oracle32, min_frac=min_frac), (k, rel, rel32, frac, frac32)
            continue
        assert frac >= min_frac, (k, frac)
        assert rel < 1e-3, (k, rel)
    return got, ref


def check_fused_rgbd(rs, rv, oracle64, seed=0, oracle32=None):
    """rasterizer.render_rgbd (one pass) vs (a) the two reference-style passes of the same library and
    (b) the fp64 oracle with a depth gradient.  With `oracle32` (the random sweeps of scripts/exp: scenes of tens of thousands of Gaussians)
    a gradient that misses the 1e-3 bar against fp64 is judged against the fp32 oracle's own error, as in check_backward, and -- third tier -- against
    the oracles run with the other decision at proven alpha = 1/255 threshold pixels (decision_aware)."""
    from activesplat_amd import rasterizer as R
    H, W = int(rs.image_height), int(rs.image_width)
    dev = rv["means3D"].device
    g = torch.Generator().manual_seed(seed)
    dLc = torch.randn(3, H, W, generator=g).to(dev)
    dLd = torch.randn(1, H, W, generator=g).to(dev)
    P = rv["means3D"].shape[0]

    def leaves():
        inp = {k: v.detach().clone().requires_grad_(True) for k, v in rv.items()}
        return inp, torch.zeros(P, 3, device=dev, requires_grad=True)
    # (1) fused
    inp, m2d = leaves()
    color, radii, depth, sil, dsq = R.render_rgbd(rs, means2D=m2d, **inp)
    ((color * dLc).sum() + (depth * dLd).sum()).backward()
    gf = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    gf["means2D"] = m2d.grad.detach().cpu().numpy()
    # (2) two passes, the second with colours [z_cam, 1, z_cam^2] built from means3D (viewmatrix row-vector convention)
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731

    def two_passes():
        """-> (c1, r1, c2, {key: (gradient of the colour pass, gradient of the depth pass)}): the two passes' gradients SEPARATELY -- their sum is
        what the fused pass must reproduce, the sum of their norms is the scale its rounding is measured against"""
        inp2, m2a = leaves()
        m2b = torch.zeros(P, 3, device=dev, requires_grad=True)
        c1, r1, _, _ = R.GaussianRasterizer(raster_settings=rs)(means2D=m2a, **inp2)
        V = rs.viewmatrix.reshape(4, 4).to(dev)
        z = inp2["means3D"] @ V[:3, 2] + V[3, 2]
        second = {k: v for k, v in inp2.items() if k not in ("colors_precomp", "shs")}
        c2, _, _, _ = R.GaussianRasterizer(raster_settings=rs._replace(bg=torch.zeros(3, device=dev)))(
            means2D=m2b, colors_precomp=torch.stack([z, torch.ones_like(z), z * z], 1), **second)
        leaves2 = list(inp2.items()) + [("means2D", m2a)]
        g_col = torch.autograd.grad((c1 * dLc).sum(), [v for _, v in leaves2], allow_unused=True)
        leaves3 = [(k, v) for k, v in inp2.items() if k not in ("colors_precomp", "shs")] + [("means2D", m2b)]
        g_dep = dict(zip([k for k, _ in leaves3], torch.autograd.grad((c2[0:1] * dLd).sum(), [v for _, v in leaves3], allow_unused=True)))
        out = {}
        for (k, _), gc_ in zip(leaves2, g_col):
            a_ = np.zeros(gf[k].shape, np.float64) if gc_ is None else n(gc_).astype(np.float64)
            gd_ = g_dep.get(k)
            out[k] = (a_, np.zeros(gf[k].shape, np.float64) if gd_ is None else n(gd_).astype(np.float64))
        return c1, r1, c2, out
    c1, r1, c2, parts = two_passes()
    assert np.array_equal(n(radii), n(r1))
    if R.last_stats.get("max_tile_instances", 0) >= 8192 and not np.array_equal(n(color), n(c1)):
        # (tile lists of 8192 and more in a small image take the SEGMENTED forward, whose segments add their sums with atomics: two renders
        # of one scene agree to the last bits only)
        assert np.abs(n(color) - n(c1)).max() <= 2e-6 * max(1.0, float(np.abs(n(c1)).max()))
    else:
        np.testing.assert_array_equal(n(color), n(c1))
    for a, b, name in ((depth[0], c2[0], "depth"), (sil[0], c2[1], "silhouette"), (dsq[0], c2[2], "depth_sq")):
        sc = max(1.0, float(n(b).max()))
        assert close_frac(n(a), n(b), 1e-5, 2e-6 * sc) > 0.9999, name
    for k in gf:
        a_, b_ = parts[k]
        d_ = (gf[k].astype(np.float64) - (a_ + b_)).reshape(P, -1) if P else np.zeros((0, 1))
        e2 = (d_ ** 2).sum(1)
        scale = max(np.linalg.norm(a_) + np.linalg.norm(b_), 1e-30)
        # 1e-4 of the two parts' magnitudes for the tensor WITHOUT its two worst rows, 1e-3 with them.  The device's atomics sum in a different order
        # every run, and one kind of Gaussian carries a run-to-run spread of up to 2e-4 of the whole tensor all by itself: a screen-filling splat
        # centred far outside the image (raw moments with pixel offsets of hundreds, combinations that nearly cancel in the chain to the 3-D
        # parameters) -- seeds 130378, 142132, 150586 of the round-5 sweeps; `scripts/exp/rgbd_variance.py`: 99-100 % of the spread in ONE Gaussian,
        # two runs of the SAME formulation 5e-5 ... 2e-4 apart.  A wrong term in the fused pass would show in every row.
        worst = np.sort(e2)[-2:].sum() if P > 8 else 0.0
        assert np.sqrt(max(e2.sum() - worst, 0.0)) < 1e-4 * scale, (k, float(np.sqrt(e2.sum())) / scale)
        assert np.sqrt(e2.sum()) < 1e-3 * scale, (k, float(np.sqrt(e2.sum())) / scale)
    # (3) fp64 oracle
    ref = util.run_oracle(oracle64, rs, rv)
    go = oracle64.backward(ref, dLc.cpu().numpy(), dLd.cpu().numpy())
    go32 = None
    decided = []                                                # (see check_backward)
    for k, gq in gf.items():
        r = go[k].reshape(gq.shape)
        rel = np.linalg.norm(gq.astype(np.float64) - r) / max(np.linalg.norm(r), 1e-30)
        HATCH["keys_checked"] += 1
        if rel >= 1e-3 and oracle32 is not None:
            HATCH["fired"] += 1
            HATCH["where"].append((k + " (fused RGB-D)", float(rel), 1.0, int(gq.shape[0])))
            if go32 is None:
                fwd32 = util.run_oracle(oracle32, rs, rv)
                go32 = oracle32.backward(fwd32, dLc.cpu().numpy(), dLd.cpu().numpy())
            o = go32[k].reshape(gq.shape).astype(np.float64)
            rel32 = np.linalg.norm(o - r) / max(np.linalg.norm(r), 1e-30)
            if not rel <= 1.5 * rel32 + 1e-6:
                rerun = _Rerun(lambda orc: orc.backward(util.run_oracle(orc, rs, rv), dLc.cpu().numpy(), dLd.cpu().numpy()), go, fwd32=fwd32)
                rerun.decided = decided
                assert decision_aware(k + " (fused RGB-D)", gq, ref, W, H, rerun, oracle64, oracle32), (k, rel, rel32)
            continue
        assert rel < 1e-3, (k, rel)
    sc = max(1.0, float(ref["depth_sq"].max()))
    assert close_frac(n(dsq), ref["depth_sq"], FWD_RTOL, FWD_ATOL * sc) >= 0.999


def close_frac(a, b, rtol, atol):
    return util.close_frac(a, b, rtol, atol)


def check_optimistic_launch(device, N=20000):
    """The binning workspace of frame k is sized from frame k-1 and the render enqueued before the counters are read:
    a hit (same view again) and a miss (a view with 10x the instances, re-launched with exact sizes after the
    capacity-clamped first attempt) must both reproduce the exactly-sized launch bit for bit."""
    from activesplat_amd import GaussianRasterizer, rasterizer as R
    rs_far, rv = util.scene(N, 96, 80, seed=11, device=device, w2c=util.pose(0.0, (0.0, 0.0, -3.3)))     # most of the scene behind the camera
    rs_near, _ = util.scene(N, 96, 80, seed=11, device=device)
    m2d = torch.zeros(N, 3, device=device)
    run = lambda rs: [t.clone() for t in GaussianRasterizer(raster_settings=rs)(means2D=m2d, **rv)]  # noqa: E731
    R.optimistic = False
    try:
        exact_far, exact_near = run(rs_far), run(rs_near)
        d_far = R.last_stats["num_rendered"]
    finally:
        R.optimistic = True
    R._capacity.clear()
    R.last_stats.pop("optimistic_hits", None); R.last_stats.pop("optimistic_misses", None)
    a = run(rs_far)                       # no guess yet: exact
    b = run(rs_far)                       # hit
    assert R.last_stats.get("optimistic_hits", 0) == 1 and R.last_stats.get("optimistic_misses", 0) == 0
    d_near_guess = R._capacity[(N, 96, 80, rv["means3D"].device.index)][0]
    c = run(rs_near)                      # miss: D grows far beyond 1.25 x
    assert R.last_stats["num_rendered"] > d_near_guess and R.last_stats["optimistic_misses"] == 1
    d = run(rs_near)                      # hit at the grown capacity
    e = run(rs_far)                       # hit with a much larger capacity than needed
    assert R.last_stats["optimistic_hits"] == 3
    for got, ref in ((a, exact_far), (b, exact_far), (c, exact_near), (d, exact_near), (e, exact_far)):
        for x, y in zip(got, ref):
            assert torch.equal(x, y)
    # gradients through an optimistic hit
    rv_g = {k: v.clone().requires_grad_(True) for k, v in rv.items()}
    GaussianRasterizer(raster_settings=rs_near)(means2D=m2d, **rv_g)[0].sum().backward()
    R.optimistic = False
    try:
        rv_h = {k: v.clone().requires_grad_(True) for k, v in rv.items()}
        GaussianRasterizer(raster_settings=rs_near)(means2D=m2d, **rv_h)[0].sum().backward()
    finally:
        R.optimistic = True
    for k in rv_g:
        if rv_g[k].grad is not None:
            a, b = rv_g[k].grad.double(), rv_h[k].grad.double()     # two runs of the atomics: sums in a different order
            assert float((a - b).norm() / b.norm().clamp_min(1e-30)) < 1e-5, k


def check_optimistic_tile_list_growth(device):
    """An optimistic launch whose TILE-LIST capacity is too small: frame 1 has lists under one sort chunk (2048), frame 2 --
    same (P, W, H) key -- lists of several thousand, so the optimistic attempt sorts only the first chunk(s) of every tile
    and leaves the tail of point_list unwritten.  The attempt must neither fault (garbage ids are not Gaussian indices)
    nor leak into the result: the exact re-launch reproduces the exactly-sized render bit for bit."""
    from activesplat_amd import GaussianRasterizer, rasterizer as R
    N, W, H = 20000, 48, 48
    rs_far, rv = util.scene(N, W, H, seed=5, device=device, w2c=util.pose(0.0, (0.0, 0.0, -3.4)))
    rs_near, _ = util.scene(N, W, H, seed=5, device=device)
    rv["opacities"] = rv["opacities"] * 0.05
    m2d = torch.zeros(N, 3, device=device)
    run = lambda rs: [t.clone() for t in GaussianRasterizer(raster_settings=rs)(means2D=m2d, **rv)]  # noqa: E731
    R.optimistic = False
    try:
        exact_far = run(rs_far); far_tile = R.last_stats["max_tile_instances"]
        exact_near = run(rs_near); near_tile = R.last_stats["max_tile_instances"]
    finally:
        R.optimistic = True
    assert 0 < far_tile < 1500 and near_tile > 2 * 2048, (far_tile, near_tile)
    R._capacity.clear()
    R.last_stats.pop("optimistic_hits", None); R.last_stats.pop("optimistic_misses", None)
    a = run(rs_far)
    # what the caching allocator hands to the optimistic attempt's point_list: make it look like anything but Gaussian ids
    junk = torch.full((int(R.last_stats["num_rendered"] * 16 + 65536),), 0x7F7F7F7F, dtype=torch.int32, device=device)
    del junk
    b = run(rs_near)
    assert R.last_stats.get("optimistic_misses", 0) == 1
    c = run(rs_near)
    assert R.last_stats.get("optimistic_hits", 0) == 1
    for got, ref in ((a, exact_far), (b, exact_near), (c, exact_near)):
        for x, y in zip(got, ref):
            assert torch.equal(x, y)


def check_segmented_forward(device, oracle32):
    """Few tiles, long lists: the tile lists are composited in parallel segments (GsBinLayout.segments > 1).  Against the
    oracle like every other case, and against the one-workgroup-per-tile walk of the same library."""
    from activesplat_amd import _lib, rasterizer as R
    lib = _lib.get()
    rs, rv = build_case("merge_tiles_large", device)                 # 48 x 48: 9 tiles of ~12 k records
    got, ref = check_forward(rs, rv, oracle32)
    assert int(util.LAST["bl"].segments) > 1
    seg = util.artefacts()
    _lib.check(lib.gs_set_forward_segments(0))
    try:
        one = util.run_product(rs, rv)
        assert int(util.LAST["bl"].segments) == 1
        art = util.artefacts()
    finally:
        _lib.check(lib.gs_set_forward_segments(1))
    for k in ("color", "depth", "opacity"):
        assert np.abs(got[k] - one[k]).max() <= 2e-5 * max(1.0, float(np.abs(one[k]).max())), k
    assert np.mean(seg["n_contrib"] == art["n_contrib"]) >= 0.999
    assert np.abs(seg["final_T"] - art["final_T"]).max() <= 1e-6
    # the backward consumes the segmented forward's final_T / n_contrib
    dL = torch.randn(3, int(rs.image_height), int(rs.image_width), generator=torch.Generator().manual_seed(0))
    a = util.run_product(rs, rv, dL)["grads"]
    _lib.check(lib.gs_set_forward_segments(0))
    try:
        b = util.run_product(rs, rv, dL)["grads"]
    finally:
        _lib.check(lib.gs_set_forward_segments(1))
    for k in a:
        den = np.linalg.norm(b[k])
        if den > 0:
            assert np.linalg.norm(a[k] - b[k]) / den < 1e-4, k


def check_render_views_leaves_the_capacity_table_alone(device, N=2000, W=48, H=40):
    """render_views launches at exact size outside the capacity table (the atlas picks its segment count from the capacities, so a stored
    guess would make a panorama depend on the call history): R._capacity and the hit / miss counters are what they were before the call,
    the call twice gives the same bits, and the three views are those of three single-view exact-size calls: bit for bit in the view whose
    atlas slot starts at column 0 and in every view's radii.  The other views are NOT bit-identical to a single-view render, before this helper
    existed or after: a pixel's x is offset by its view's slot, so fp32 rounds pixel - mean differently (measured here on the emulated
    kernels, the same figures with and without the shared launch helper: colour up to 1.4e-6, depth 7.2e-6, opacity 1.6e-6 apart).  They
    are held to the bound that tests/test_lookaround.py (batched against batched=False) and cluster_cases.check_look_around_nodes already
    pin for exactly this difference: atol 1e-5, depth atol 2e-5 / rtol 1e-5."""
    from activesplat_amd import GaussianRasterizer, rasterizer as R
    views = [util.scene(N, W, H, seed=4, device=device, w2c=util.pose(yaw, t))[0] for yaw, t in ((0.0, (0.0, 0.0, 0.0)), (0.35, (0.1, 0.0, 0.2)),
                                                                                                  (-0.4, (-0.2, 0.05, 0.4)))]
    _, rv = util.scene(N, W, H, seed=4, device=device)
    was = R.optimistic
    try:
        R.optimistic = False
        single = [[t.clone() for t in GaussianRasterizer(raster_settings=rs)(means2D=None, **rv)] for rs in views]
        R.optimistic = True
        R._capacity.clear()
        R._capacity[("sentinel",)] = (7, 9)
        R.last_stats["optimistic_hits"], R.last_stats["optimistic_misses"] = 5, 3
        with torch.no_grad():
            got = R.render_views(views, **rv)
            again = R.render_views(views, **rv)
        assert R._capacity == {("sentinel",): (7, 9)}, R._capacity
        assert (R.last_stats["optimistic_hits"], R.last_stats["optimistic_misses"]) == (5, 3)
        assert R.last_stats["P"] == N and R.last_stats["num_rendered"] > 0
        worst = 0.0
        for v, (g, a, ref) in enumerate(zip(got, again, single)):
            assert g[0].shape == (3, H, W) and g[1].shape == (N,)
            for x, y in zip(g, a):
                assert torch.equal(x, y), v                      # (no dependence on the call history)
            worst = max([worst] + [float((x.float() - y.float()).abs().max()) for x, y in zip(g, ref)])
        print(f"[render_views] largest difference between a view of the atlas and its single-view render: {worst:.3e}")
        for v, (g, ref) in enumerate(zip(got, single)):
            assert torch.equal(g[1], ref[1]) and int((ref[1] > 0).sum()) > 0, v           # radii: every view, exactly
            if v == 0:
                assert all(torch.equal(x, y) for x, y in zip(g, ref))
            else:
                assert torch.allclose(g[0], ref[0], atol=1e-5) and torch.allclose(g[3], ref[3], atol=1e-5), v
                assert torch.allclose(g[2], ref[2], atol=2e-5, rtol=1e-5), v
    finally:
        R.optimistic = was
        R._capacity.clear()
        R.last_stats.pop("optimistic_hits", None); R.last_stats.pop("optimistic_misses", None)


def check_raw_inputs_by_name(device, N=500, W=48, H=40):
    """render_rgbd_raw (autograd) and the direct entry (render_rgbd_raw_direct + backward_direct, what mapping_iteration calls) are the same
    launches: equal outputs, equal dL/dmeans2D.  And the three exclusions of the raw inputs still raise with their messages."""
    import pytest
    from activesplat_amd import rasterizer as R
    from activesplat_amd import synthetic as syn
    from activesplat_amd.camera import setup_camera
    p = {k: v.to(device) for k, v in syn.make_params(N, W, H, seed=9).items()}
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device)
    pose = [0.9950042, 0.0, 0.0998334, 0.0, 0.03, -0.02, 0.05]
    g = torch.Generator().manual_seed(4)
    dLc, dLd = torch.randn(3, H, W, generator=g).to(device), torch.randn(1, H, W, generator=g).to(device)
    args = (p["means3D"], p["logit_opacities"], p["log_scales"], p["unnorm_rotations"])
    iso = int(p["log_scales"].shape[1]) == 1
    m2d = torch.empty_like(p["means3D"], requires_grad=True)
    a = R.render_rgbd_raw(cam, args[0], m2d, *args[1:], pose, colors_precomp=p["rgb_colors"])
    ((a[0] * dLc).sum() + (a[2] * dLd).sum()).backward()
    with torch.no_grad():
        ctx, b = R.render_rgbd_raw_direct(cam, args[0], torch.empty_like(p["means3D"]), *args[1:], R.RawInputs(pose, iso), colors_precomp=p["rgb_colors"])
        d_m2d = R.backward_direct(ctx, dLc, dLd)[1]
    assert int((a[1] > 0).sum()) > N // 4
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    print(f"[raw inputs] |dL/dmeans2D| autograd - direct: {float((m2d.grad - d_m2d).abs().max()):.3e} of {float(d_m2d.abs().max()):.3e}")
    if device == "cpu":
        assert torch.equal(m2d.grad, d_m2d)
    else:                                                            # (two runs of the device's atomics: sums in a different order)
        assert float((m2d.grad.double() - d_m2d.double()).norm() / d_m2d.double().norm().clamp_min(1e-30)) < 1e-5
    raw = lambda **kw: R.render_rgbd_raw(cam, args[0], torch.empty_like(p["means3D"]), *args[1:], pose, colors_precomp=p["rgb_colors"], **kw)  # noqa: E731
    camera = (torch.tensor(pose[:4], device=device, requires_grad=True), torch.tensor(pose[4:], device=device, requires_grad=True))
    with pytest.raises(Exception, match="adam= and accumulate_grads= exclude each other"):
        raw(adam=object(), accumulate_grads=True)
    with pytest.raises(Exception, match="adam= and a differentiable camera exclude each other"):
        raw(adam=object(), camera=camera)
    with pytest.raises(Exception, match=r"gaussians_grad=False is the pose-only backward: it needs camera=\(cam_rot, cam_trans\)"):
        raw(gaussians_grad=False)
