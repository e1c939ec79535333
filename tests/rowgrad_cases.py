"""The per-Gaussian backward (csrc/preprocess_bwd.hip) ROW BY ROW at its rare branches, shared by the host-emulated kernel tests
(tests/test_rowgrad.py) and the device tests (tests/test_gpu_rowgrad.py).

parity_cases.check_backward judges a whole gradient tensor (99.5 % of the elements, relative L2 below 1e-3).  A mistake of the per-Gaussian
chain is confined to the rows that take one branch -- the frustum clamp, an SH channel clamped at 0, a culled row inside a live wavefront, a
coefficient loop predicated for a degree below 3 -- and in the generated scenes each of those is taken by far fewer than 0.5 % of the rows.  The
scenes here make such a class the MAJORITY of the visible rows (asserted from the fp64 reference), and every visible row is judged on its own.

Scenes keep the blend out of the row error: splats sit one or two to a tile (exact_lists' placement) or reach into the image from outside it
with few neighbours, opacity is at most 0.5 (no pixel reaches the alpha = 0.99 clamp, no walk reaches T < 1e-4 -- asserted), lists are short,
and no Gaussian owns a pixel with |255 alpha - 1| < 1e-4 (asserted with parity_cases.threshold_gaussians; a splat that does is dimmed by 3 %
when the scene is built, until none is left).

Rule (check_rows), for every visible row i, gradient tensor k and component c, with g_64 the fp64 oracle's row and g_32 the fp32 oracle's:

    |g_kernel - g_64|  <=  min( 2 |g_32 - g_64| + FLOOR ||g_64[i]||_inf ,  CAP ||g_64[i]||_inf )

a row whose fp64 gradient is zero is exactly zero in the kernel, and so is every row of a Gaussian that was not rendered, in every tensor.  The
factor 2 is the mirror rule of DESIGN section 6; the reference for the error is the fp32 ORACLE (operation for operation the kernel's chain),
never the kernel.  No row is excused and there is no second tier.

FLOOR and CAP are measured on the two oracles alone (test_rowgrad.test_fp32_oracle_alone_sets_floor_and_cap re-measures them on every run):
the largest per-row relative error max_c |g_32 - g_64| / ||g_64[i]||_inf of the fp32 oracle over all scenes, entry points and tensors here is
MEASURED_ORACLE32_ROW_ERROR; FLOOR is twice that, rounded up to one significant digit.  CAP starts at the project's 1e-3 and is 10 FLOOR
where the fp32 oracle alone stays inside that on every scene (profiles/README.md, "Per-Gaussian backward, row by row", states which).

Raw-parameter entry points (render_rgbd_raw: activations and the frame transform inside the kernel): the oracles take the ACTIVATED inputs,
formed from the fp32 parameters in the oracle's own precision, and their row gradients are chained to the parameters by torch autograd in that
precision (fp64 for g_64, fp32 for g_32).  The camera-pose gradient is a sum over the rows: it is held to the sum of the rows' bounds, each
row's share taken from the same two chains.  The Adam-in-the-backward entry writes no gradient: after ONE step from zero moments the first
moment is (1 - beta1) g, so the row gradient is read back from it (one fp32 rounding, 6e-8 of the element), and on the emulated kernels
parameters and both moments also equal backward + GaussianAdam.step() bit for bit."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from activesplat_amd import mapping as M
from activesplat_amd import optim as O
from activesplat_amd import rasterizer as R
from tests import parity_cases as pc
from tests import projection_cases as prc
from tests import util

W, H = 160, 128                     # 10 x 8 tiles; fx = fy = 80, tan(fov) = 1 and 0.8: clamp limits 1.3 and 1.04
GX, GY = W // 16, H // 16
FX, CX, CY = W / 2.0, W / 2.0 - 1.0, H / 2.0 - 1.0
LIMX, LIMY = 1.3 * 1.0, 1.3 * 0.8

#: largest per-row relative error of the fp32 oracle against the fp64 oracle over every scene / entry point / tensor of this module (CPU, the
#: oracles alone; test_fp32_oracle_alone_sets_floor_and_cap prints the current value and holds it to FLOOR / 2)
MEASURED_ORACLE32_ROW_ERROR = 6.3e-4
#: 2 x MEASURED_ORACLE32_ROW_ERROR, rounded up to one significant digit
FLOOR = 2e-3
#: cap on a row's relative error: the project's 1e-3.  (10 x FLOOR would not be tighter, so the starting point stands -- and since FLOOR exceeds
#: it, the cap is what binds on every row: a visible row is within 1e-3 of its own largest fp64 component, or the test fails.)
CAP = 1e-3
# (isotropic maps: equal scales make the rotation irrelevant, its exact gradient is zero and the kernel's is the rounding noise of terms of the
# size of the row's log-scale gradient -- both are sums of dL/dM R s: check_rows holds it to CAP x that row's log-scale gradient)
#: no Gaussian of a scene owns a pixel with |255 alpha - 1| below this
THRESHOLD_WINDOW = 1e-4


def _unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q)).tolist()


POSE7 = _unit([math.cos(0.06), 0.03, math.sin(0.06), -0.02]) + [0.05, -0.03, 0.1]


class Scene:
    def __init__(self, name, rs, rv, kind, meta=None):
        self.name, self.rs, self.rv, self.kind, self.meta = name, rs, rv, kind, meta or {}
        self.P = int(rv["means3D"].shape[0])
        self.raw = None            # raw-parameter scenes: dict(params, iso)


# ---- placement ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *s):
    return torch.rand(*s, generator=g, dtype=torch.float64)


def _randn(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float64)


def _in_tiles(tiles, g):
    """exact_lists' placement: pixel centres 5 .. 11 px inside the tile -> (u, v)"""
    t = torch.as_tensor(tiles)
    n = t.shape[0]
    return 16.0 * (t % GX).double() + 5.0 + 6.0 * _rand(g, n), 16.0 * (t // GX).double() + 5.0 + 6.0 * _rand(g, n)


def _means(u, v, z):
    return torch.stack([(u - CX) / FX * z, (v - CY) / FX * z, z], 1)


def _small_splats(tiles, g, lo=0.5, hi=1.5):
    """Splats of lo .. hi px per axis centred in the given tiles (radius at most 5 px: a splat stays in its tile or just touches a neighbour)"""
    u, v = _in_tiles(tiles, g)
    n = u.shape[0]
    z = 0.5 + 3.5 * _rand(g, n)
    scales = (z / FX)[:, None] * (lo + (hi - lo) * _rand(g, n, 3))
    rot = F.normalize(_randn(g, n, 4))
    return dict(means3D=_means(u, v, z), scales=scales, rotations=rot, opacities=(0.1 + 0.4 * _rand(g, n))[:, None])


def _behind(n, g):
    """Finite Gaussians behind the camera (culled by the near plane)"""
    z = -(0.5 + 3.0 * _rand(g, n))
    m = torch.stack([(_rand(g, n) - 0.5) * 2.0, (_rand(g, n) - 0.5) * 2.0, z], 1)
    return dict(means3D=m, scales=0.02 + 0.05 * _rand(g, n, 3), rotations=F.normalize(_randn(g, n, 4)), opacities=(0.1 + 0.4 * _rand(g, n))[:, None])


def _cat(parts, g, shuffle=True):
    rv = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    n = rv["means3D"].shape[0]
    perm = torch.randperm(n, generator=g) if shuffle else torch.arange(n)
    return {k: v[perm].float().contiguous() for k, v in rv.items()}, perm


def _near_axis_rot(g, n, jitter=0.1):
    q = torch.zeros(n, 4, dtype=torch.float64)
    q[:, 0] = 1.0
    return F.normalize(q + jitter * _randn(g, n, 4))


def _clamped_splats(axis, n, g, ratios=None):
    """n splats whose centre lies beyond 1.3 tan(fov) on `axis` ('x', 'y' or 'xy') and whose footprint reaches back into the image: long on the
    clamped axis (the image edge sits at ~1.6 sigma), 2 .. 3.5 px on the other, so that one tile row (x) / column (y) holds one group of them.
    ratios: explicit |t / tz| on the clamped axis (rows near the limit)."""
    i = torch.arange(n)
    side = torch.where(_rand(g, n) < 0.5, -1.0, 1.0).double()
    z = 0.5 + 3.0 * _rand(g, n)
    if axis == "x":
        r = (LIMX + 0.02 + 0.4 * _rand(g, n)) if ratios is None else torch.as_tensor(ratios, dtype=torch.float64)
        rx = side * r
        ry = (16.0 * (i % GY).double() + 8.0 + 3.0 * (2 * _rand(g, n) - 1) - CY) / FX
        long_px = (r - 1.0).clamp_min(0.3) * FX / 1.6
        sig = torch.stack([long_px, 2.0 + 1.5 * _rand(g, n)], 1)
    elif axis == "y":
        r = (LIMY + 0.02 + 0.3 * _rand(g, n)) if ratios is None else torch.as_tensor(ratios, dtype=torch.float64)
        ry = side * r
        rx = (16.0 * (i % GX).double() + 8.0 + 3.0 * (2 * _rand(g, n) - 1) - CX) / FX
        long_px = (r - 0.8).clamp_min(0.24) * FX / 1.6
        sig = torch.stack([2.0 + 1.5 * _rand(g, n), long_px], 1)
    else:
        side2 = torch.where(_rand(g, n) < 0.5, -1.0, 1.0).double()
        ax, ay = LIMX + 0.02 + 0.25 * _rand(g, n), LIMY + 0.02 + 0.2 * _rand(g, n)
        rx, ry = side * ax, side2 * ay
        d = torch.maximum((ax - 1.0) * FX, (ay - 0.8) * FX) / 1.5
        sig = d[:, None] * (0.9 + 0.2 * _rand(g, n, 2))
    means = torch.stack([rx * z, ry * z, z], 1)
    scales = torch.stack([sig[:, 0] * z / FX, sig[:, 1] * z / FX, 0.3 * torch.minimum(sig[:, 0], sig[:, 1]) * z / FX], 1)
    hi = 0.3 if axis == "xy" else 0.5
    return dict(means3D=means, scales=scales, rotations=_near_axis_rot(g, n), opacities=(0.1 + (hi - 0.1) * _rand(g, n))[:, None])


_O32 = []


def _oracle32():
    if not _O32:
        from oracle.gs_oracle import Oracle
        _O32.append(Oracle("f32"))
    return _O32[0]


def _settle(rs, rv, oracle64):
    """Dim (by 3 %, repeatedly) every Gaussian that owns a pixel with |255 alpha - 1| < THRESHOLD_WINDOW until none does: a row that needs
    excusing means the scene is wrong.  -> rv (deterministic: the oracle alone decides)"""
    rv = dict(rv)
    for _ in range(12):
        hits = []
        for o in (oracle64, _oracle32()):
            f = util.run_oracle(o, rs, rv)
            hits += pc.threshold_gaussians(f, np.nonzero(f["radii"] > 0)[0], W, H, window=THRESHOLD_WINDOW)
        if not hits:
            return rv
        o = rv["opacities"].clone()
        o[sorted({h[0] for h in hits})] *= 0.97
        rv["opacities"] = o
    raise AssertionError("threshold pixels left after 12 rounds")


_SCENES = {}
SCENES = ["clamp_x", "clamp_y", "clamp_xy", "sh_clamped_deg0", "sh_clamped_deg1", "sh_clamped_deg2", "sh_clamped_deg3", "needle_rows"]
#: sparse_live: P % 256 in {1, 63, 65}
SPARSE_P = [513, 575, 577]


def _colors(g, n):
    return torch.rand(n, 3, generator=g)


def _rs(sh_degree=None):
    rs, _ = util.scene(1, W, H, device="cpu", sh_degree=sh_degree)
    return rs


def _clamp_scene(name, oracle64, exact):
    axis = name.split("_")[1]
    g = _gen({"x": 101, "y": 102, "xy": 103}[axis])
    near = [1.0 + s * d for d in (1e-4, 3e-4, 9e-4) for s in (-1.0, 1.0)]            # within 1e-3 (relative) of the limit, both sides
    parts = []
    if axis in ("x", "xy"):
        parts += [_clamped_splats("x", 96 if axis == "x" else 12, g), _clamped_splats("x", 12, g, ratios=[LIMX * r for r in near] * 2)]
    if axis in ("y", "xy"):
        parts += [_clamped_splats("y", 100 if axis == "y" else 10, g), _clamped_splats("y", 12, g, ratios=[LIMY * r for r in near] * 2)]
    if axis == "xy":
        parts.append(_clamped_splats("xy", 120, g))
    interior = [t for t in range(GX * GY) if 3 <= t % GX <= 6 and 2 <= t // GX <= 5]
    parts += [_small_splats(interior * (1 if axis == "xy" else 2), g), _behind(80, g)]
    rv, _ = _cat(parts, g)
    named = {}
    if exact and axis == "x":
        # the comparison is strict: a row exactly AT the limit (tx / tz = 1.3f with tz = 1, an identity view) is unclamped, one ulp above is clamped
        at, above = np.float32(1.3), np.nextafter(np.float32(1.3), np.float32(2.0))
        e = _clamped_splats("x", 4, g, ratios=[1.3] * 4)
        m = e["means3D"].float()
        m[:, 2] = 1.0
        m[:, 0] = torch.tensor([at, -at, above, -above])
        m[:, 1] = torch.tensor([-0.5, -0.1, 0.2, 0.6])
        e["scales"] = e["scales"] / e["means3D"][:, 2:3]
        P0 = rv["means3D"].shape[0]
        rv = {k: torch.cat([rv[k], (m if k == "means3D" else e[k].float())], 0).contiguous() for k in rv}
        named = {"at_limit": [P0, P0 + 1], "one_ulp_over": [P0 + 2, P0 + 3]}
    rv["colors_precomp"] = _colors(g, rv["means3D"].shape[0])
    rs = _rs()
    return Scene(name, rs, _settle(rs, rv, oracle64), "clamp", dict(axis=axis, named=named))


def _sh_scene(name, oracle64, width):
    deg = int(name[-1])
    g = _gen(200 + deg)
    tiles = list(range(GX * GY)) * 2
    rv, _ = _cat([_small_splats(tiles, g), _behind(60, g)], g)
    n = rv["means3D"].shape[0]
    Mw = (deg + 1) ** 2 if width == "own" else 16
    # DC term: colour = 0.5 + C0 dc + (higher orders); row i gets i % 4 channels well below zero, the others well above
    i = torch.arange(n)
    neg = torch.stack([(i % 4) > ((c + i // 4) % 3) for c in range(3)], 1)
    mag = 0.25 + 0.35 * torch.rand(n, 3, generator=g)
    target = torch.where(neg, -mag, mag)
    shs = 0.05 * torch.randn(n, Mw, 3, generator=g)
    shs[:, 0, :] = (target - 0.5) / 0.28209479177387814
    nb = (deg + 1) ** 2
    if Mw > nb:
        # coefficients above the degree are not part of the function: every eighth row holds NaN / inf there, and nothing may read them (with
        # finite values a loop bound of M instead of nb changes no output: the basis functions above the degree are zero)
        shs[::8, nb:, :] = float("nan")
        shs[4::8, nb:, 1] = float("inf")
    rv["shs"] = shs.contiguous()
    rs = _rs(sh_degree=deg)
    return Scene(name, rs, _settle(rs, rv, oracle64), "sh", dict(deg=deg, width=Mw))


def _needle_scene(oracle64):
    """projection_cases.needle_scene's shapes (one axis 100 .. 1000 times the other two, randomly oriented), one needle per tile and short
    enough to stay there (2.5 .. 5 px along the needle, the other two axes far below the 0.3 px low-pass), with forty ordinary splats between
    them.  (A needle longer than a tile does not keep the blend out of its row: the pixel mean's gradient is conic x first moments, which
    cancels by L^2 / 0.3 for a needle of L px, and the blend sums those moments in fp32 -- on a 9 .. 35 px variant of this scene single rows
    of means2D / means3D sat at 1.6e-3 .. 2.4e-3 of fp64 and moved by 1e-3 with the order of the blend's atomic sums.)"""
    g = _gen(301)
    s = _small_splats(list(range(GX * GY)), g)
    n = s["means3D"].shape[0]
    z = s["means3D"][:, 2]
    long_px = 2.5 + 2.5 * _rand(g, n)
    aniso = torch.exp(math.log(100.0) + _rand(g, n) * math.log(10.0))
    sc = (long_px / aniso)[:, None] * (0.9 + 0.2 * _rand(g, n, 3))
    sc[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = long_px
    s["scales"] = sc * (z / FX)[:, None]
    rv, _ = _cat([s, _small_splats(list(range(0, GX * GY, 2)), g), _behind(90, g)], g)
    rv["colors_precomp"] = _colors(g, rv["means3D"].shape[0])
    rs = _rs()
    return Scene("needle_rows", rs, _settle(rs, rv, oracle64), "needle")


def _to_raw(rv, g, iso=False):
    """The mapper's parameters whose activations under POSE7 are (up to fp32 rounding) the rendervars rv."""
    q = torch.tensor(POSE7[:4], dtype=torch.float64)
    t = torch.tensor(POSE7[4:], dtype=torch.float64)
    Rm = M.build_rotation(q[None])[0]
    n = rv["means3D"].shape[0]
    rot = rv["rotations"].double()
    if not iso:
        rot = M.quat_mult((q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64)).expand(n, 4), rot)
    o = rv["opacities"].double()
    p = dict(means3D=(rv["means3D"].double() - t) @ Rm, unnorm_rotations=rot * (0.5 + 1.5 * _rand(g, n))[:, None],
             logit_opacities=torch.log(o / (1 - o)), log_scales=torch.log(rv["scales"].double()[:, :1] if iso else rv["scales"].double()))
    p = {k: v.float().contiguous() for k, v in p.items()}
    if "shs" in rv:
        p["shs"] = rv["shs"].clone()
    else:
        p["rgb_colors"] = rv["colors_precomp"].clone()
    return p


def _sparse_scene(P, iso, oracle64):
    """Raw-parameter entry: ONE visible row per wavefront of 64 at a varying lane, wavefront 2 entirely culled, the last wavefront partial
    (P % 256 in {1, 63, 65}); the culled rows are behind the camera, and some of them carry NaN / inf / zero-quaternion parameters."""
    g = _gen(400 + P + (1 if iso else 0))
    waves = (P + 63) // 64
    live = []
    for w in range(waves):
        if w == 2:
            continue
        rows = min(64, P - 64 * w)
        live.append(64 * w + min((11 * w + 5) % 64, rows - 1))
    tiles = [(7 * j + 3) % (GX * GY) for j in range(len(live))]
    vis = _small_splats(tiles, g, lo=0.8, hi=1.6)
    if iso:
        vis["scales"] = vis["scales"][:, :1].expand(-1, 3).clone()
    back = _behind(P - len(live), g)
    rv = {}
    lm = torch.zeros(P, dtype=torch.bool)
    lm[live] = True
    for k in vis:
        a = torch.empty(P, vis[k].shape[1], dtype=torch.float64)
        a[lm], a[~lm] = vis[k], back[k]
        rv[k] = a.float().contiguous()
    rv["colors_precomp"] = _colors(g, P)
    rs = _rs()
    rv = _settle(rs, rv, oracle64)
    sc = Scene(f"sparse_live_{P}_{'iso' if iso else 'aniso'}", rs, rv, "sparse", dict(live=live, P=P))
    prm = _to_raw(rv, g, iso=iso)
    # poison culled rows (none of them a lone visible row): wavefronts 0, 1 (beside a live lane), 2 (the culled wavefront) and the last one
    nan, inf = float("nan"), float("inf")
    dead = [i for i in range(P) if not lm[i]]
    pick = lambda w, j: [i for i in dead if i // 64 == w][j]  # noqa: E731
    bad = {}
    prm["means3D"][pick(0, 0), 1] = nan; bad[pick(0, 0)] = "nan mean"
    prm["log_scales"][pick(0, 1), 0] = inf; bad[pick(0, 1)] = "inf log-scale"
    prm["logit_opacities"][pick(1, 0)] = nan; bad[pick(1, 0)] = "nan logit"
    prm["unnorm_rotations"][pick(1, 1), 2] = nan; bad[pick(1, 1)] = "nan quaternion"
    prm["unnorm_rotations"][pick(1, 2)] = 0.0; bad[pick(1, 2)] = "zero quaternion"
    prm["means3D"][pick(2, 0), 2] = inf; bad[pick(2, 0)] = "inf mean"
    prm["log_scales"][pick(2, 1), 0] = nan; bad[pick(2, 1)] = "nan log-scale"
    prm["unnorm_rotations"][pick(2, 2)] = 0.0; bad[pick(2, 2)] = "zero quaternion"
    prm["unnorm_rotations"][pick(2, 3)] = inf; bad[pick(2, 3)] = "inf quaternion"
    if P - 64 * (waves - 1) > 1:
        prm["log_scales"][dead[-1], 0] = inf; bad[dead[-1]] = "inf log-scale"
    sc.raw = dict(params=prm, iso=iso)
    sc.meta["bad"] = bad
    return sc


def scene(name, oracle64, exact=True, width="own"):
    """-> the cached Scene `name`.  exact (clamp_x): with the rows exactly at the limit and one ulp above (drop-in entry points: an identity view
    keeps tx / tz exact; the raw-parameter entry's frame transform does not).  width (SH scenes): 'own' = (deg + 1)^2 coefficients per row (the
    any-width instantiation), 16 = rows of 16 with the degree below 3 predicated away (the 16-coefficient instantiation)."""
    key = (name, exact if name == "clamp_x" else True, width if name.startswith("sh_") else "own")
    if key not in _SCENES:
        if name.startswith("clamp_"):
            _SCENES[key] = _clamp_scene(name, oracle64, key[1])
        elif name.startswith("sh_"):
            _SCENES[key] = _sh_scene(name, oracle64, width)
        elif name == "needle_rows":
            _SCENES[key] = _needle_scene(oracle64)
        else:
            raise KeyError(name)
    return _SCENES[key]


def sparse_scene(P, iso, oracle64):
    key = ("sparse", P, iso)
    if key not in _SCENES:
        _SCENES[key] = _sparse_scene(P, iso, oracle64)
    return _SCENES[key]


def raw_of(sc):
    """-> dict(params, iso) of a scene for the raw-parameter entry points (the scene's rendervars moved to the world frame of POSE7)"""
    if sc.raw is None:
        sc.raw = dict(params=_to_raw(sc.rv, _gen(77)), iso=False)
    return sc.raw


# ---- references --------------------------------------------------------------------------------------------------------------------------------
def upstream():
    """dL/dcolour [3, H, W], dL/ddepth [1, H, W]: a constant per channel plus noise of half its size.  (Under pure noise a row's gradient is what
    is left of pixel terms that cancel, and the fp32 ORACLE's rows sit at up to 3e-3 of fp64 on ordinary splats: the bar would measure the
    upstream image, not the chain.)"""
    g = _gen(9)
    c = torch.tensor([1.0, -0.7, 0.5]).reshape(3, 1, 1)
    return c * (1.0 + 0.5 * torch.randn(3, H, W, generator=g)), 0.5 * (1.0 + 0.5 * torch.randn(1, H, W, generator=g))


def _cov3d(rv):
    """R S S^T R^T (fp64, rounded to the fp32 input the entry point takes), upper triangle"""
    q = rv["rotations"].double()
    Rm = M.build_rotation(q)
    Mm = Rm * rv["scales"].double()[:, None, :]
    S = Mm @ Mm.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float().contiguous()


def cov_inputs(sc):
    if "cov" not in sc.meta:
        rv = {k: v for k, v in sc.rv.items() if k not in ("scales", "rotations")}
        rv["cov3D_precomp"] = _cov3d(sc.rv)
        sc.meta["cov"] = rv
    return sc.meta["cov"]


def _chain(prm, iso, dtype):
    """transform_to_frame(camera_grad=True) + transformed_params2rendervar in `dtype`, the camera pair as leaves -> (leaves, (q, t), rendervars)"""
    d = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in prm.items()}
    q = torch.tensor(POSE7[:4], dtype=dtype, requires_grad=True)
    t = torch.tensor(POSE7[4:], dtype=dtype, requires_grad=True)
    n = d["means3D"].shape[0]
    means = d["means3D"] @ M.build_rotation(q[None])[0].T + t
    if iso:
        rot, sc = F.normalize(d["unnorm_rotations"]), torch.exp(d["log_scales"]).repeat(1, 3)
    else:
        rot, sc = F.normalize(M.quat_mult(q.expand(n, 4), F.normalize(d["unnorm_rotations"]))), torch.exp(d["log_scales"])
    return d, (q, t), dict(means3D=means, rotations=rot, opacities=torch.sigmoid(d["logit_opacities"]), scales=sc)


RAW_KEYS = {"means3D": "means3D", "rotations": "unnorm_rotations", "opacities": "logit_opacities", "scales": "log_scales"}


def _raw_forward(oracle, sc):
    """The oracle's forward on the activations of the scene's parameters, formed in the oracle's precision -> (forward, activations, dtype)"""
    raw = raw_of(sc)
    prm, iso = raw["params"], raw["iso"]
    dtype = torch.float64 if oracle.real == np.float64 else torch.float32
    with torch.no_grad():
        _d, _p, act_all = _chain(prm, iso, dtype)
    rv = {k: v.detach() for k, v in act_all.items()}
    rv["shs" if "shs" in prm else "colors_precomp"] = prm["shs" if "shs" in prm else "rgb_colors"]
    return util.run_oracle(oracle, sc.rs, rv), act_all, dtype


def _settle_raw(sc, oracle64, oracle32):
    """_settle for the raw-parameter form of a scene (its activations are the rendervars up to rounding, which may move a rim pixel into the
    window): the logit of a Gaussian that owns a threshold pixel in either oracle's forward drops by 0.03."""
    if sc.meta.get("raw_settled"):
        return
    prm = raw_of(sc)["params"]
    for _ in range(12):
        hits = []
        for o in (oracle64, oracle32):
            f = _raw_forward(o, sc)[0]
            hits += pc.threshold_gaussians(f, np.nonzero(f["radii"] > 0)[0], W, H, window=THRESHOLD_WINDOW)
        if not hits:
            sc.meta["raw_settled"] = True
            return
        prm["logit_opacities"][sorted({h[0] for h in hits})] -= 0.03
    raise AssertionError("threshold pixels left after 12 rounds")


def _raw_reference(oracle, sc, depth):
    raw = raw_of(sc)
    prm, iso = raw["params"], raw["iso"]
    f, act_all, dtype = _raw_forward(oracle, sc)
    col = "shs" if "shs" in prm else "colors_precomp"
    dLc, dLd = upstream()
    g = oracle.backward(f, dLc.numpy(), dLd.numpy() if depth else None)
    vis = np.nonzero(f["radii"] > 0)[0]
    ix = torch.as_tensor(vis)
    # the chain on the VISIBLE rows alone (a culled row may hold NaN parameters: 0 x NaN would reach the pose gradient through the sums)
    d, (q, t), act = _chain({k: v[ix] for k, v in prm.items() if k in RAW_KEYS.values()}, iso, dtype)
    up = {k: torch.as_tensor(np.asarray(g[k]).reshape(act_all[k].shape)[vis]).to(dtype) for k in act}
    rows = sum((act[k] * up[k]).sum(1) for k in act)                              # L_i of every visible row
    leaves = [d[RAW_KEYS[k]] for k in act]
    grads = torch.autograd.grad(rows.sum(), leaves, retain_graph=True)
    out = {}
    for k, gr in zip(list(act), grads):
        out[RAW_KEYS[k]] = np.zeros(tuple(prm[RAW_KEYS[k]].shape), np.float64)
        out[RAW_KEYS[k]][vis] = gr.detach().double().numpy()
    out["shs" if col == "shs" else "rgb_colors"] = np.asarray(g[col], np.float64)
    out["means2D"] = np.asarray(g["means2D"], np.float64)
    # every row's share of the pose gradient: d L_i / d (q, t)
    eye = torch.eye(len(vis), dtype=dtype)
    jq, jt = torch.autograd.grad(rows, [q, t], grad_outputs=eye, is_grads_batched=True)
    out["_pose_rows"] = np.concatenate([jq.double().numpy(), jt.double().numpy()], 1)          # [visible, 7]
    return f, out


def _rv_reference(oracle, sc, rv, depth):
    dLc, dLd = upstream()
    f = util.run_oracle(oracle, sc.rs, rv)
    g = oracle.backward(f, dLc.numpy(), dLd.numpy() if depth else None)
    return f, {k: np.asarray(g[k], np.float64) for k in list(rv) + ["means2D"]}


_REFS = {}


def reference(sc, entry, depth, oracle64, oracle32):
    """entry: 'sr' (scale + rotation), 'cov' (cov3D_precomp), 'raw' (parameters) -> dict(f64, g64, g32, visible); computed once per scene."""
    key = (sc.name, id(sc), entry, depth)
    if key not in _REFS:
        if entry == "raw":
            _settle_raw(sc, oracle64, oracle32)
            f64, g64 = _raw_reference(oracle64, sc, depth)
            f32, g32 = _raw_reference(oracle32, sc, depth)
        else:
            rv = sc.rv if entry == "sr" else cov_inputs(sc)
            f64, g64 = _rv_reference(oracle64, sc, rv, depth)
            f32, g32 = _rv_reference(oracle32, sc, rv, depth)
        vis = f64["radii"] > 0
        assert np.array_equal(vis, f32["radii"] > 0), (sc.name, entry, "the two oracles disagree on visibility: move the splat")
        _REFS[key] = dict(f64=f64, f32=f32, g64=g64, g32=g32, visible=vis, iso=bool(entry == "raw" and raw_of(sc)["iso"]))
        assert_scene(sc, _REFS[key], entry)
    return _REFS[key]


# ---- what a scene is built to hold, from the fp64 reference ------------------------------------------------------------------------------------
def classes(sc, ref):
    """-> a label per row (the class of the branch it takes), from the fp64 oracle's forward and the fp64 inputs"""
    f = ref["f64"]
    P = sc.P
    lab = np.array(["plain"] * P, dtype=object)
    if sc.kind == "clamp":
        m = np.asarray(f["_ctx"]["means3D"], np.float64)                            # (identity view: the camera-frame mean)
        rx, ry = np.abs(m[:, 0] / m[:, 2]), np.abs(m[:, 1] / m[:, 2])
        cx_, cy_ = rx > LIMX, ry > LIMY
        lab[cx_ & ~cy_], lab[~cx_ & cy_], lab[cx_ & cy_] = "clamped-x", "clamped-y", "clamped-xy"
        nearx, neary = np.abs(rx / LIMX - 1) < 1e-3, np.abs(ry / LIMY - 1) < 1e-3
        for i in np.nonzero(nearx | neary)[0]:
            lab[i] = lab[i] + " (near the limit)"
        for name, rows in sc.meta.get("named", {}).items():
            for i in rows:
                lab[i] = f"{lab[i]} [{name}]"
    elif sc.kind == "sh":
        n = np.asarray(f["clamped"]).astype(bool).sum(1)
        lab = np.array([f"{int(k)} channels clamped" for k in n], dtype=object)
    elif sc.kind == "sparse":
        lab = np.array([f"lane {i % 64} of wavefront {i // 64}" for i in range(P)], dtype=object)
    elif sc.kind == "needle":
        s = sc.rv["scales"].double().numpy()
        a = s.max(1) / np.sort(s, 1)[:, 1]
        lab = np.array([f"anisotropy {('>= 300' if x >= 300 else '>= 90' if x >= 90 else '< 90')}" for x in a], dtype=object)
    return lab


def assert_scene(sc, ref, entry):
    """The scene holds what it was built for (class majorities), and the blend stays out of the row error: no alpha at the 0.99 clamp, no
    walk at the T stop, short lists, no threshold pixel -- all from the oracles alone."""
    f, vis = ref["f64"], ref["visible"]
    nv = int(vis.sum())
    lab = classes(sc, ref)
    co = np.asarray(f["conic_opacity"])
    assert co[vis, 3].max() <= 0.5 + 1e-6, (sc.name, co[vis, 3].max())
    assert float(np.asarray(f["final_T"]).min()) > 1e-2, (sc.name, float(np.asarray(f["final_T"]).min()))
    n = f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0].astype(np.int64)
    assert n.max() <= 64, (sc.name, int(n.max()))
    for fw in (ref["f64"], ref["f32"]):
        hits = pc.threshold_gaussians(fw, np.nonzero(vis)[0], W, H, window=THRESHOLD_WINDOW)
        assert not hits, (sc.name, entry, hits[:4])
    if sc.kind == "clamp":
        axis = sc.meta["axis"]
        frac = np.mean([l.split(" ")[0] == "clamped-" + axis for l in lab[vis]])
        assert frac >= 0.6, (sc.name, frac, nv)
        near = [l for l in lab[vis] if "near the limit" in l]
        assert sum(l.startswith("clamped") for l in near) >= 3 and sum(l.startswith("plain") for l in near) >= 3, (sc.name, near)
        if entry != "raw":
            for name, rows in sc.meta["named"].items():
                assert all(vis[i] for i in rows), (sc.name, name)
                assert all(lab[i].startswith("plain" if name == "at_limit" else "clamped-x") for i in rows), (sc.name, name, [lab[i] for i in rows])
    elif sc.kind == "sh":
        k = np.asarray(f["clamped"]).astype(bool).sum(1)[vis]
        assert np.mean(k >= 1) >= 0.5, (sc.name, np.mean(k >= 1))
        assert all((k == c).sum() >= 10 for c in (1, 2, 3)), (sc.name, [(int(c), int((k == c).sum())) for c in range(4)])
        assert np.array_equal(np.asarray(ref["f32"]["clamped"]), np.asarray(f["clamped"])), sc.name
        if entry != "raw":
            pre = prc._np(prc.reference(sc.rs, sc.rv)["rgb_pre"])[vis]
            assert np.abs(pre).min() > 1e-3, (sc.name, np.abs(pre).min())            # no channel sits at the clamp itself
    elif sc.kind == "sparse":
        live = sc.meta["live"]
        assert sorted(np.nonzero(vis)[0].tolist()) == sorted(live), (sc.name, np.nonzero(vis)[0].tolist(), live)
        per_wave = np.bincount(np.nonzero(vis)[0] // 64, minlength=(sc.P + 63) // 64)
        assert per_wave[2] == 0 and (np.delete(per_wave, 2) == 1).all() and sc.P % 256 in (1, 63, 65), (sc.name, per_wave)
    elif sc.kind == "needle":
        frac = np.mean([not l.endswith("< 90") for l in lab[vis]])
        assert frac >= 0.6 and nv >= 100, (sc.name, frac, nv)
    assert 200 <= sc.P <= 600 and (nv >= 100 or sc.kind == "sparse"), (sc.name, sc.P, nv)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------
REPORT = []          # (label, tensor, worst ratio, class of that row): the tests print it; the device log shows margins


def oracle_row_error(ref):
    """Largest per-row relative error of the fp32 oracle against the fp64 oracle over the visible rows of every tensor -> (value, tensor, row)"""
    worst = (0.0, None, -1)
    vis = np.nonzero(ref["visible"])[0]
    for k, r in ref["g64"].items():
        if k.startswith("_") or (k == "unnorm_rotations" and ref.get("iso")):
            continue
        r64 = np.asarray(r, np.float64).reshape(r.shape[0], -1)[vis]
        r32 = np.asarray(ref["g32"][k], np.float64).reshape(r.shape[0], -1)[vis]
        scale = np.abs(r64).max(1)
        ok = scale > 0
        if not ok.any():
            continue
        e = np.abs(r32 - r64).max(1)[ok] / scale[ok]
        j = int(np.argmax(e))
        if e[j] > worst[0]:
            worst = (float(e[j]), k, int(vis[ok][j]))
    return worst


def check_rows(label, sc, ref, got, radii=None, skip=(), iso_rotation=False):
    """got: {tensor: array [P, ...]} of the kernel.  Every visible row against the rule at the top; every other row exactly zero."""
    vis = ref["visible"]
    if radii is not None:
        assert np.array_equal(np.asarray(radii) > 0, vis), (label, "visibility differs from the oracles'", np.nonzero((np.asarray(radii) > 0) != vis)[0][:8])
    lab = classes(sc, ref)
    P = sc.P
    for k, g in got.items():
        if k in skip:
            continue
        G = np.asarray(g, np.float64).reshape(P, -1)
        R64 = np.asarray(ref["g64"][k], np.float64).reshape(P, -1)
        R32 = np.asarray(ref["g32"][k], np.float64).reshape(P, -1)
        assert np.isfinite(G).all(), (label, k, "non-finite gradient in rows", np.nonzero(~np.isfinite(G).all(1))[0][:8].tolist())
        dead = np.nonzero(~vis & (np.abs(G).max(1) != 0))[0]
        assert dead.size == 0, (label, k, "rows of Gaussians that were not rendered must be exactly zero", dead[:8].tolist(), G[dead[:2]].tolist())
        if iso_rotation and k == "unnorm_rotations":
            scale = np.abs(np.asarray(ref["g64"]["log_scales"], np.float64).reshape(P, -1)).max(1)
            ratio = np.abs(G).max(1)[vis] / (CAP * scale[vis])
            j = int(np.argmax(ratio))
            REPORT.append((label, k + " (isotropic: noise)", float(ratio[j]), lab[np.nonzero(vis)[0][j]]))
            print(f"[rowgrad] {label:44s} {k:18s} isotropic map, rounding noise only: largest |g| / (CAP x the row's log-scale gradient) {ratio[j]:.2e}")
            assert ratio[j] <= 1.0, (label, k, float(ratio[j]))
            continue
        scale = np.abs(R64).max(1)
        zero = vis & (scale == 0)
        assert (np.abs(G[zero]) == 0).all(), (label, k, "rows with a zero fp64 gradient must be exactly zero", np.nonzero(zero & (np.abs(G).max(1) != 0))[0][:8])
        rows = np.nonzero(vis & (scale > 0))[0]
        if rows.size == 0:
            continue
        e_k, e_32 = np.abs(G - R64)[rows], np.abs(R32 - R64)[rows]
        s = scale[rows][:, None]
        bound = np.minimum(2.0 * e_32 + FLOOR * s, CAP * s)
        ratio = (e_k / bound).max(1)
        j = int(np.argmax(ratio))
        REPORT.append((label, k, float(ratio[j]), lab[rows[j]]))
        print(f"[rowgrad] {label:44s} {k:18s} worst row {rows[j]:4d} ratio {ratio[j]:.3f} ({lab[rows[j]]}); rel. error {float((e_k[j] / s[j]).max()):.2e}, "
              f"fp32 oracle {float((e_32[j] / s[j]).max()):.2e}")
        if ratio[j] > 1.0:
            bad = rows[ratio > 1.0]
            raise AssertionError(f"{label}: {k}: {bad.size} of {rows.size} rows outside the per-row bound, worst row {rows[j]} ({lab[rows[j]]}): ratio {ratio[j]:.3f}, "
                                 f"kernel {G[rows[j]].tolist()} fp64 {R64[rows[j]].tolist()} fp32 oracle {R32[rows[j]].tolist()}; classes of the failing rows: "
                                 f"{sorted(set(lab[bad]))}")


def check_pose(label, sc, ref, got7):
    """The pose gradient (dq [4], dt [3]) against the sum of the fp64 rows' shares; bound: the sum of the rows' bounds."""
    c64, c32 = ref["g64"]["_pose_rows"], ref["g32"]["_pose_rows"]
    s = np.abs(c64).max(1, keepdims=True)
    bound = np.minimum(2.0 * np.abs(c32 - c64) + FLOOR * s, CAP * s).sum(0)
    err = np.abs(np.asarray(got7, np.float64) - c64.sum(0))
    ratio = err / bound
    j = int(np.argmax(ratio))
    REPORT.append((label, "pose", float(ratio[j]), f"component {j}"))
    print(f"[rowgrad] {label:44s} {'pose':18s} worst component {j} ratio {ratio[j]:.3f}; error {err[j]:.2e} of {np.abs(c64.sum(0))[j]:.2e} (sum of row shares' magnitudes "
          f"{np.abs(c64).sum(0)[j]:.2e})")
    assert np.isfinite(got7).all() and ratio[j] <= 1.0, (label, "pose", ratio.tolist())


# ---- the entry points --------------------------------------------------------------------------------------------------------------------------
class _NoBackwardCtx(R._DirectCtx):
    """A forward that was NOT told a backward follows (no input requires grad): it saves no SH Jacobian, the backward recomputes it."""
    needs_input_grad = (False,) * len(R._DirectCtx.needs_input_grad)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def run_dropin(sc, device, rv=None, fused=False, saved_jacobian=True):
    """GaussianRasterizer (fused: render_rgbd, colour AND depth gradient) on rendervars -> (gradients, radii).  saved_jacobian=False: the same
    library calls with a forward that was not told a backward follows (_RasterizeGaussians.forward / _backward on a direct context)."""
    rv = sc.rv if rv is None else rv
    rs = sc.rs._replace(bg=sc.rs.bg.to(device), viewmatrix=sc.rs.viewmatrix.to(device), projmatrix=sc.rs.projmatrix.to(device), campos=sc.rs.campos.to(device))
    dLc, dLd = (t.to(device) for t in upstream())
    inp = {k: v.detach().clone().to(device).requires_grad_(saved_jacobian) for k, v in rv.items()}
    m2d = torch.zeros(sc.P, 3, device=device, requires_grad=saved_jacobian)
    if saved_jacobian:
        if fused:
            color, radii, depth, _s, _q = R.render_rgbd(rs, means2D=m2d, **inp)
            ((color * dLc).sum() + (depth * dLd).sum()).backward()
        else:
            color, radii, _d, _o = R.GaussianRasterizer(raster_settings=rs)(means2D=m2d, **inp)
            (color * dLc).sum().backward()
        g = {k: _np(v.grad) for k, v in inp.items()}
        g["means2D"] = _np(m2d.grad)
        return g, _np(radii)
    ctx = _NoBackwardCtx()
    i = inp.get
    out = R._RasterizeGaussians.forward(ctx, i("means3D"), m2d, i("shs"), i("colors_precomp"), i("opacities"), i("scales"), i("rotations"), i("cov3D_precomp"), rs, fused)
    assert ctx.sh_jac == 0
    t = R._RasterizeGaussians._backward(ctx, dLc, dLd if fused else None)
    names = ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
    return {k: _np(v) for k, v in zip(names, t) if v is not None}, _np(out[1])


def _params(sc, device):
    raw = raw_of(sc)
    return {k: torch.nn.Parameter(v.clone().to(device)) for k, v in raw["params"].items()}, raw["iso"]


def _cols(prm):
    return dict(shs=prm["shs"]) if "shs" in prm else dict(colors_precomp=prm["rgb_colors"])


def _rs_on(sc, device):
    rs = sc.rs
    return rs._replace(bg=rs.bg.to(device), viewmatrix=rs.viewmatrix.to(device), projmatrix=rs.projmatrix.to(device), campos=rs.campos.to(device))


def run_raw(sc, device, accumulate=False, saved_jacobian=True):
    """render_rgbd_raw -> (parameter gradients + means2D, radii).  accumulate: the backward ADDS into zero-filled .grad tensors (the gated path)."""
    prm, _iso = _params(sc, device)
    rs = _rs_on(sc, device)
    dLc, dLd = (t.to(device) for t in upstream())
    m2d = torch.empty(sc.P, 3, device=device, requires_grad=saved_jacobian)
    if not saved_jacobian:
        ctx = _NoBackwardCtx()
        out = R._RasterizeGaussians.forward(ctx, prm["means3D"].detach(), m2d, prm["shs"].detach() if "shs" in prm else None,
                                            prm["rgb_colors"].detach() if "rgb_colors" in prm else None, prm["logit_opacities"].detach(), prm["log_scales"].detach(),
                                            prm["unnorm_rotations"].detach(), None, rs, True, R.RawInputs(POSE7, _iso))
        assert ctx.sh_jac == 0
        t = R._RasterizeGaussians._backward(ctx, dLc, dLd)
        names = ("means3D", "means2D", "shs", "rgb_colors", "logit_opacities", "log_scales", "unnorm_rotations")
        return {k: _np(v) for k, v in zip(names, t) if v is not None}, _np(out[1])
    if accumulate:
        for k, v in prm.items():
            v.grad = torch.zeros_like(v)
    color, radii, depth, _s, _q = R.render_rgbd_raw(rs, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], POSE7,
                                                    accumulate_grads=accumulate, **_cols(prm))
    ((color * dLc).sum() + (depth * dLd).sum()).backward()
    g = {k: _np(v.grad) for k, v in prm.items()}
    g["means2D"] = _np(m2d.grad)
    return g, _np(radii)


LRS = dict(means3D=1e-3, rgb_colors=2.5e-3, shs=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3)


def run_adam(sc, device, exact):
    """render_rgbd_raw(adam=): ONE step from zero moments.  -> (row gradients read back from the first moment, means2D included, radii); exact:
    parameters and both moments equal backward + GaussianAdam.step() bit for bit, row by row."""
    rs = _rs_on(sc, device)
    dLc, dLd = (t.to(device) for t in upstream())
    res = []
    for fused in (True, False) if exact else (True,):
        prm, _iso = _params(sc, device)
        opt = O.initialize_optimizer(prm, {k: LRS[k] for k in prm})
        m2d = torch.empty(sc.P, 3, device=device, requires_grad=True)
        color, radii, depth, _s, _q = R.render_rgbd_raw(rs, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], POSE7,
                                                        adam=opt if fused else None, **_cols(prm))
        ((color * dLc).sum() + (depth * dLd).sum()).backward()
        opt.step()
        res.append((prm, {k: (opt.state[v]["exp_avg"], opt.state[v]["exp_avg_sq"]) for k, v in prm.items()}, m2d.grad, radii))
    prm, st, m2d, radii = res[0]
    b1 = 0.9
    g = {k: _np(st[k][0]).astype(np.float64) / (1.0 - b1) for k in prm}
    g["means2D"] = _np(m2d)
    before = raw_of(sc)["params"]
    vis = _np(radii) > 0
    for k in prm:
        # a Gaussian that was not rendered steps with a zero gradient from zero moments: nothing moves (a NaN stays the NaN it was)
        a, b = _np(prm[k])[~vis], before[k].numpy()[~vis]
        assert ((a == b) | (np.isnan(a) & np.isnan(b))).all(), (sc.name, k)
        assert (_np(st[k][0])[~vis] == 0).all() and (_np(st[k][1])[~vis] == 0).all(), (sc.name, k)
    if exact:
        prm2, st2, m2d2, _ = res[1]
        assert torch.equal(m2d, m2d2)
        for k in prm:
            same = lambda a, b: bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())  # noqa: E731
            rows = lambda a, b: np.nonzero(~_np((a == b) | (torch.isnan(a) & torch.isnan(b))).reshape(sc.P, -1).all(1))[0][:8].tolist()  # noqa: E731
            assert same(prm[k].detach(), prm2[k].detach()), (sc.name, k, "parameters", rows(prm[k].detach(), prm2[k].detach()))
            assert same(st[k][0], st2[k][0]) and same(st[k][1], st2[k][1]), (sc.name, k, "moments", rows(st[k][0], st2[k][0]))
    return g, _np(radii)


def run_pose(sc, device, pose_only):
    """render_rgbd_raw(camera=): mode 1 (parameter rows + pose) or mode 2 (gaussians_grad=False: dmeans2D and the pose only)
    -> (gradients, pose gradient [7], radii)"""
    prm, _iso = _params(sc, device)
    rs = _rs_on(sc, device)
    dLc, dLd = (t.to(device) for t in upstream())
    q = torch.tensor(POSE7[:4], dtype=torch.float32, device=device, requires_grad=True)
    t = torch.tensor(POSE7[4:], dtype=torch.float32, device=device, requires_grad=True)
    m2d = torch.empty(sc.P, 3, device=device, requires_grad=True)
    color, radii, depth, _s, _q = R.render_rgbd_raw(rs, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], None,
                                                    camera=(q, t), gaussians_grad=not pose_only, **_cols(prm))
    ((color * dLc).sum() + (depth * dLd).sum()).backward()
    if pose_only:
        assert all(v.grad is None for v in prm.values()), sc.name
        g = {}
    else:
        g = {k: _np(v.grad) for k, v in prm.items()}
    g["means2D"] = _np(m2d.grad)
    return g, np.concatenate([_np(q.grad), _np(t.grad)]), _np(radii)


# ---- one scene through every entry point that reaches a distinct instantiation -----------------------------------------------------------------
def check_cov3d(name, device, oracle64, oracle32, width="own"):
    """The drop-in call with cov3D_precomp (render_rgbd: colour and depth gradient) on one scene"""
    sc = scene(name, oracle64, exact=True, width=width)
    tag = f"{name}" + (f"/M={sc.meta['width']}" if sc.kind == "sh" else "")
    refc = reference(sc, "cov", True, oracle64, oracle32)
    for sj in (True, False) if sc.kind == "sh" else (True,):
        g, radii = run_dropin(sc, device, rv=cov_inputs(sc), fused=True, saved_jacobian=sj)
        check_rows(f"{tag} cov3D_precomp" + ("" if sj else " (recompute)"), sc, refc, g, radii)


def check_scene(name, device, oracle64, oracle32, exact_adam=False, width="own", cov3d=True):
    """A clamp / SH / needle scene: the drop-in call (scale + rotation; SH scenes with the saved Jacobian and with the recompute branch), the
    cov3D_precomp call (cov3d), and -- colours, or 16-coefficient rows at degree 3 -- the raw-parameter entry, the Adam step inside it, pose
    modes 1 and 2."""
    sc = scene(name, oracle64, exact=True, width=width)
    tag = f"{name}" + (f"/M={sc.meta['width']}" if sc.kind == "sh" else "")
    jac = (True, False) if sc.kind == "sh" else (True,)
    ref = reference(sc, "sr", False, oracle64, oracle32)
    for sj in jac:
        g, radii = run_dropin(sc, device, saved_jacobian=sj)
        check_rows(f"{tag} drop-in" + ("" if sj else " (recompute)"), sc, ref, g, radii)
    if cov3d:
        check_cov3d(name, device, oracle64, oracle32, width=width)
    if sc.kind == "sh" and not (sc.meta["deg"] == 3 and sc.meta["width"] == 16):
        return
    rsc = scene(name, oracle64, exact=False, width=width)
    refr = reference(rsc, "raw", True, oracle64, oracle32)
    for sj in jac:
        g, radii = run_raw(rsc, device, saved_jacobian=sj)
        check_rows(f"{tag} raw" + ("" if sj else " (recompute)"), rsc, refr, g, radii)
    g, radii = run_adam(rsc, device, exact_adam)
    check_rows(f"{tag} raw adam", rsc, refr, g, radii)
    for pose_only in (False, True):
        g, pose, radii = run_pose(rsc, device, pose_only)
        check_rows(f"{tag} raw pose mode {2 if pose_only else 1}", rsc, refr, g, radii)
        check_pose(f"{tag} raw pose mode {2 if pose_only else 1}", rsc, refr, pose)


def check_sparse(P, iso, device, oracle64, oracle32, exact_adam=False):
    """sparse_live: the raw-parameter entry, its accumulating (gated) form, the Adam step, pose modes 1 and 2."""
    sc = sparse_scene(P, iso, oracle64)
    ref = reference(sc, "raw", True, oracle64, oracle32)
    tag = sc.name
    for acc in (False, True):
        g, radii = run_raw(sc, device, accumulate=acc)
        check_rows(f"{tag} raw" + (" accumulate" if acc else ""), sc, ref, g, radii, iso_rotation=iso)
    g, radii = run_adam(sc, device, exact_adam)
    check_rows(f"{tag} raw adam", sc, ref, g, radii, iso_rotation=iso)
    for pose_only in (False, True):
        g, pose, radii = run_pose(sc, device, pose_only)
        check_rows(f"{tag} raw pose mode {2 if pose_only else 1}", sc, ref, g, radii, iso_rotation=iso)
        check_pose(f"{tag} raw pose mode {2 if pose_only else 1}", sc, ref, pose)


def all_references(oracle64, oracle32):
    """Every (scene, entry) reference of this module -> [(label, ref)]: what FLOOR and CAP are measured on."""
    out = []
    for name in SCENES:
        widths = ("own", 16) if name.startswith("sh_") and not name.endswith("3") else ("own",)
        for w in widths:
            sc = scene(name, oracle64, width=w)
            out.append((f"{name}/{w} sr", reference(sc, "sr", False, oracle64, oracle32)))
            out.append((f"{name}/{w} cov", reference(sc, "cov", True, oracle64, oracle32)))
            if not name.startswith("sh_") or name.endswith("3"):
                rsc = scene(name, oracle64, exact=False, width=w)
                out.append((f"{name}/{w} raw", reference(rsc, "raw", True, oracle64, oracle32)))
    for P in SPARSE_P:
        for iso in (False, True):
            out.append((f"sparse_live_{P}_{iso} raw", reference(sparse_scene(P, iso, oracle64), "raw", True, oracle64, oracle32)))
    return out
