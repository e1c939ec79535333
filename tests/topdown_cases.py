"""Shared checks of the planner's top-down maps (activesplat_amd/topdown.py): run on the host-emulated kernels by tests/test_topdown.py and on the
MI355X by tests/test_gpu_topdown.py.

The reference for every comparison is the fp32 oracle run THE REFERENCE'S WAY (visualizer.py:923-965): activate the parameters in torch
(sigmoid, exp, F.normalize, as transformed_params2rendervar does) -> cut by height -> compact -> oracle forward of the subset -> opacity <= 0.4;
oracle forward of everything on white -> bytes -> grey -> == 255.

Tolerances (none of them comes from the code under test):
* floats: the project's image tolerance, rtol 1e-4 / atol 1e-5 (tests/parity_cases.py: FWD_RTOL, FWD_ATOL) with its rule for the pixels whose
  alpha = 1/255 or T = 1e-4 decision flips -- at least 99.9 % of the values inside the tolerance, none further out than 0.02;
* bytes: a byte may differ from the oracle's by at most 1, and only where the oracle's colour x 255 lies within 255 x (atol + rtol |colour|) of
  an integer -- a colour that moves by the tolerance moves colour x 255 by 255 times as much, and only next to an integer can that change
  the truncation;
* boolean maps: equal to the oracle's except at PROVABLY AMBIGUOUS pixels -- free map: the oracle's opacity within the tolerance of 0.4;
  visible map: a touched pixel (oracle opacity > 0) where moving the oracle's colour by -/+ the tolerance flips grey == 255 (grey is
  monotone in every channel, so the two extreme colours decide).  An untouched pixel is never exempt: its colour is exactly 1 x bg on both
  sides.  The ambiguous pixels are counted and capped at 0.2 % of the image per map.
"""
import numpy as np
import torch

from activesplat_amd import io as IO
from activesplat_amd import rasterizer as R
from activesplat_amd import topdown as TD
from tests import parity_cases as pc
from tests import util

RTOL, ATOL = pc.FWD_RTOL, pc.FWD_ATOL
CAP = 0.002                     # ambiguous pixels per map, fraction of the image
BAND = (0.1, 1.3)               # upper (agent head) <= -y <= lower (agent foot - adjust): the band of the counts in the issue
CENTRE, EXTENT = (0.3, -0.2), (18.0, 15.0)


def params_of(rv, iso=False, quat_scale=1.7):
    """The mapper's parameters whose activations are (up to rounding) the render variables `rv` of parity_cases.topdown_scene: logit
    opacities, log scales ([P, 1] when iso: the first column), unnormalised quaternions."""
    ls = torch.log(rv["scales"])
    return dict(means3D=rv["means3D"].clone(), rgb_colors=rv["colors_precomp"].clone(), unnorm_rotations=(rv["rotations"] * quat_scale).contiguous(),
                logit_opacities=torch.logit(rv["opacities"].clamp(1e-6, 1 - 1e-6)).contiguous(), log_scales=(ls[:, :1] if iso else ls).contiguous())


def scene_params(N, W, H, device, iso=False, seed=12):
    _rs, rv = pc.topdown_scene(N, "cpu", seed=seed, W=W, H=H)
    return {k: v.to(device) for k, v in params_of(rv, iso).items()}


def camera(W, H, device):
    return TD.topdown_camera(CENTRE, EXTENT, (W, H), device=device)._replace(debug=True)


def grey_rule_params(device, n=160, seed=5):
    """Isolated, faint, near-white splats: touched pixels whose bytes sit at 250-254 in ONE channel -- the off-diagonal cases of the grey
    formula ((255,255,251) and (254,255,255) are still "unseen", (255,254,255) and (255,255,250) are not)."""
    g = torch.Generator().manual_seed(seed)
    xz = (torch.rand(n, 2, generator=g) - 0.5) * torch.tensor([17.0, 14.0]) + torch.tensor(CENTRE)
    y = -1.0 + 0.5 * torch.rand(n, 1, generator=g)
    palette = torch.tensor([[1.0, 1.0, 0.3], [0.3, 1.0, 1.0], [1.0, 0.3, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.6, 1.0]])
    col = palette[torch.randint(0, len(palette), (n,), generator=g)]
    opac = 0.006 + 0.05 * torch.rand(n, 1, generator=g)
    p = dict(means3D=torch.cat([xz[:, :1], y, xz[:, 1:]], 1).float().contiguous(), rgb_colors=col.contiguous(),
             unnorm_rotations=torch.randn(n, 4, generator=g), logit_opacities=torch.logit(opac), log_scales=torch.log(torch.full((n, 3), 0.03)))
    return {k: v.to(device) for k, v in p.items()}


# ---- the reference, run the reference's way ---------------------------------------------------------------------------------------------

def activate(params):
    """transformed_params2rendervar (slam_helpers.py:124-139) in the world frame."""
    ls = params["log_scales"].detach().cpu()
    if ls.shape[1] == 1:
        ls = torch.tile(ls, (1, 3))
    return dict(means3D=params["means3D"].detach().cpu().float(), colors_precomp=params["rgb_colors"].detach().cpu().float(),
                rotations=torch.nn.functional.normalize(params["unnorm_rotations"].detach().cpu().float()),
                opacities=torch.sigmoid(params["logit_opacities"].detach().cpu().float()), scales=torch.exp(ls.float()))


def in_band(means3D, upper, lower):
    """complement of __cut_gaussian_by_height (visualizer.py:2277-2286), fp32"""
    y = -means3D[:, 1].float()
    return ~torch.logical_or(y < np.float32(upper), y > np.float32(lower))


def to_bytes(color_chw):
    """[3, H, W] float32 -> [H, W, 3] uint8: clamp to [0, 1], x 255, truncate"""
    c = np.clip(np.asarray(color_chw, np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return np.ascontiguousarray(c.astype(np.uint8).transpose(1, 2, 0))


def oracle_maps(oracle32, params, cam, upper, lower):
    rs_cpu = cam._replace(bg=cam.bg.cpu(), viewmatrix=cam.viewmatrix.cpu(), projmatrix=cam.projmatrix.cpu(), campos=cam.campos.cpu())
    rv = activate(params)
    keep = in_band(rv["means3D"], upper, lower)
    H, W = int(cam.image_height), int(cam.image_width)
    full = util.run_oracle(oracle32, rs_cpu, rv)
    if int(keep.sum()) > 0:
        sub = util.run_oracle(oracle32, rs_cpu, {k: v[keep].contiguous() for k, v in rv.items()})
        free_opacity = np.asarray(sub["opacity"], np.float32).reshape(H, W)
    else:
        free_opacity = np.zeros((H, W), np.float32)
    color = np.asarray(full["color"], np.float32).reshape(3, H, W)
    rgb = to_bytes(color)
    return dict(free_opacity=free_opacity, free_map_binary=(free_opacity <= np.float32(0.4)).astype(np.uint8), color=color, visible_rgb=rgb,
                visible_map_binary=(TD.rgb_to_grey_u8(rgb) == 255).astype(np.uint8), touched=np.asarray(full["opacity"]).reshape(H, W) > 0,
                full=full, keep=keep)


def ambiguous_free(ref):
    o = ref["free_opacity"].astype(np.float64)
    return np.abs(o - 0.4) <= ATOL + RTOL * np.abs(o)


def ambiguous_visible(ref):
    c = ref["color"].astype(np.float64)
    tol = ATOL + RTOL * np.abs(c)
    lo = TD.rgb_to_grey_u8(to_bytes((c - tol).astype(np.float32))) == 255
    hi = TD.rgb_to_grey_u8(to_bytes((c + tol).astype(np.float32))) == 255
    return ref["touched"] & (lo != hi)


def run(params, cam, upper, lower):
    with R.capture() as state:
        m = TD.topdown_maps(params, cam, upper, lower)
    got = {k: getattr(m, k).cpu().numpy() for k in m._fields}
    got["state"] = state
    return got


def check_against_oracle(got, ref, label, need_free=True, need_unseen=True):
    """items 1-3 of the issue; prints the figures before it asserts"""
    H, W = ref["free_opacity"].shape
    npix = H * W
    for k in ("free_opacity", "free_map_binary", "visible_rgb", "visible_map_binary"):
        assert np.isfinite(got[k].astype(np.float64)).all(), k
    # 1. floats
    a, b = got["free_opacity"], ref["free_opacity"]
    n_bad = int(round((1.0 - util.close_frac(a, b, RTOL, ATOL)) * a.size))
    max_err = float(np.abs(a.astype(np.float64) - b).max())
    d = got["visible_rgb"].astype(np.int32) - ref["visible_rgb"].astype(np.int32)
    c255 = ref["color"].astype(np.float64).transpose(1, 2, 0) * 255.0
    near_int = np.abs(c255 - np.round(c255)) <= 255.0 * (ATOL + RTOL * np.abs(c255 / 255.0))
    n_byte = int((d != 0).sum())
    n_byte_unexplained = int(((d != 0) & ~near_int).sum())
    # 2. boolean maps
    amb_f, amb_v = ambiguous_free(ref), ambiguous_visible(ref)
    mis_f = got["free_map_binary"] != ref["free_map_binary"]
    mis_v = got["visible_map_binary"] != ref["visible_map_binary"]
    free_frac, unseen_frac = float(ref["free_map_binary"].mean()), float(ref["visible_map_binary"].mean())
    print(f"[topdown {label}] {W}x{H}: free_opacity outside tolerance {n_bad}/{npix} (max err {max_err:.2e}); bytes differing {n_byte} "
          f"(max {int(np.abs(d).max())}, not next to an integer {n_byte_unexplained}); free map: {free_frac * 100:.1f} % free, ambiguous "
          f"{int(amb_f.sum())}, mismatches {int(mis_f.sum())} (outside the ambiguous set {int((mis_f & ~amb_f).sum())}); visible map: "
          f"{unseen_frac * 100:.1f} % unseen, ambiguous {int(amb_v.sum())}, mismatches {int(mis_v.sum())} (outside {int((mis_v & ~amb_v).sum())}); "
          f"cap {int(CAP * npix)}")
    assert n_bad <= 0.001 * a.size and max_err <= 0.02, (n_bad, max_err)
    assert int(np.abs(d).max()) <= 1 and n_byte_unexplained == 0, (int(np.abs(d).max()), n_byte_unexplained)
    assert int(amb_f.sum()) <= CAP * npix and int(amb_v.sum()) <= CAP * npix, (int(amb_f.sum()), int(amb_v.sum()))
    assert not (mis_f & ~amb_f).any(), int((mis_f & ~amb_f).sum())
    assert not (mis_v & ~amb_v).any(), int((mis_v & ~amb_v).sum())
    # 3. both values of a map must occur in a scene that is used for it
    if need_free:
        assert 0.0 < free_frac < 1.0, free_frac
    if need_unseen:
        assert 0.0 < unseen_frac < 1.0, unseen_frac
    return dict(n_bad=n_bad, bytes=n_byte, amb_free=int(amb_f.sum()), amb_vis=int(amb_v.sum()))


def check_scene(device, oracle32, N, W, H, iso=False, need_free=True, need_unseen=True, band=BAND):
    params = scene_params(N, W, H, device, iso)
    cam = camera(W, H, device)
    ref = oracle_maps(oracle32, params, cam, *band)
    got = run(params, cam, *band)
    return check_against_oracle(got, ref, f"N={N} {'iso' if iso else 'aniso'}", need_free, need_unseen)


def check_grey_rule(device, oracle32, W=360, H=300):
    """item 4: touched pixels on both sides of the grey formula's off-diagonal cases, shown by the oracle, reproduced by the kernel"""
    params = grey_rule_params(device)
    cam = camera(W, H, device)
    ref = oracle_maps(oracle32, params, cam, *BAND)
    rgb, t = ref["visible_rgb"].astype(np.int32), ref["touched"]
    all255 = (rgb == 255).all(-1)
    unseen = ref["visible_map_binary"] == 1
    n_unseen_not_white = int((t & unseen & ~all255).sum())
    one_off = (rgb.sum(-1) >= 3 * 255 - 5) & ~all255              # one channel a few steps below 255
    n_seen_nearly_white = int((t & ~unseen & one_off).sum())
    print(f"[topdown grey rule] touched {int(t.sum())}; unseen although not (255,255,255): {n_unseen_not_white}; seen although within 5 steps of "
          f"white: {n_seen_nearly_white}")
    assert n_unseen_not_white > 0 and n_seen_nearly_white > 0
    got = run(params, cam, *BAND)
    check_against_oracle(got, ref, "grey rule", need_free=False, need_unseen=True)
    # and on the kernel's OWN bytes the map is the formula, pixel for pixel
    assert np.array_equal(got["visible_map_binary"], (TD.rgb_to_grey_u8(got["visible_rgb"]) == 255).astype(np.uint8))
    assert int(((got["visible_map_binary"] == 1) & ~(got["visible_rgb"] == 255).all(-1)).sum()) > 0


GREY_TABLE = [((254, 255, 255), 255), ((255, 255, 251), 255), ((255, 254, 255), 254), ((253, 255, 255), 254), ((255, 255, 250), 254),
              ((255, 255, 255), 255), ((0, 0, 0), 0)]


def check_band_edges(device, oracle32, W=120, H=150, N=3000):
    """item 5"""
    params = scene_params(N, W, H, device)
    cam = camera(W, H, device)
    upper, lower = np.float32(0.25), np.float32(1.125)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))          # noqa: E731
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))         # noqa: E731
    # eight opaque probes under distinct pixels, everything else far outside the band: -y exactly on the two edges (in), one ulp outside (out)
    m = params["means3D"].clone()
    m[:, 1] = 5.0                                                           # -y = -5: below `upper`
    probes = [(-float(upper), True), (-float(lower), True), (-float(dn(upper)), False), (-float(up(lower)), False),
              (-float(up(upper)), True), (-float(dn(lower)), True), (float("nan"), False), (-0.5, True)]
    fx, fy = W / (EXTENT[0] / 1000.0), H / (EXTENT[1] / 1000.0)
    pix = []
    for j, (y, _inside) in enumerate(probes):
        px, py = 10 + 12 * j, 20 + 14 * j
        # (camera x = world x - cx, camera y = -(world z - cz), depth 1000 + y; pixel = f x / depth + W // 2 - 0.5: the centre of pixel (px, py))
        depth = 1000.0 + (y if y == y else 0.0)
        m[j, 0] = CENTRE[0] + (px + 0.5 - W // 2) * depth / fx
        m[j, 2] = CENTRE[1] - (py + 0.5 - H // 2) * depth / fy
        m[j, 1] = y
        pix.append((py, px))
    params["means3D"] = m.contiguous()
    params["logit_opacities"] = params["logit_opacities"].clone()
    params["logit_opacities"][:len(probes)] = 4.0
    got = run(params, cam, float(upper), float(lower))
    ref = oracle_maps(oracle32, params, cam, float(upper), float(lower))
    assert np.array_equal(in_band(m.cpu(), upper, lower)[:len(probes)].numpy(), np.array([p[1] or p[0] != p[0] for p in probes]))
    for (py, px), (y, inside) in zip(pix, probes):
        o = float(got["free_opacity"][py, px])
        print(f"[topdown band edge] -y = {-y!r}: free_opacity {o:.4f} (oracle {float(ref['free_opacity'][py, px]):.4f}), expected {'in' if inside else 'out'}")
        assert (o > 0.5) == inside, (y, o)
    check_against_oracle(got, ref, "band edges", need_free=True, need_unseen=True)
    # an empty band: nothing is composited into the free map
    params = scene_params(N, W, H, device)
    got = run(params, cam, 50.0, 60.0)
    assert (got["free_opacity"] == 0).all() and (got["free_map_binary"] == 1).all()
    assert (got["visible_map_binary"] == 0).any()                          # (the visible map does not depend on the band)
    # a band that holds everything: the free map is the opacity of the full render
    got = run(params, cam, -1.0e9, 1.0e9)
    ref = oracle_maps(oracle32, params, cam, -1.0e9, 1.0e9)
    assert bool(ref["keep"].all())
    full_opacity = np.asarray(ref["full"]["opacity"], np.float32).reshape(H, W)
    assert np.array_equal(ref["free_opacity"], full_opacity)
    check_against_oracle(got, ref, "band = everything", need_free=True, need_unseen=True)
    # and it equals the opacity of the product's own full render, bit for bit
    prod = util.run_product(cam, library_activation(params))
    n_diff = int((prod["opacity"].reshape(H, W) != got["free_opacity"]).sum())
    print(f"[topdown band = everything] pixels differing from the product's full-render opacity: {n_diff}")
    assert n_diff == 0


def check_nonfinite(device, W=120, H=150):
    """item 5: the NaN / inf rows of the existing nonfinite_* inputs leave all four outputs finite"""
    _rs, rv = pc.build_case("nonfinite_appearance", "cpu")
    # the case's Gaussians sit in front of ITS camera: move them under the top-down one (x, z in the footprint, y in and around the band)
    g = torch.Generator().manual_seed(3)
    Pn = rv["means3D"].shape[0]
    good = torch.cat([(torch.rand(Pn, 1, generator=g) - 0.5) * 16.0 + CENTRE[0], -1.6 + 1.8 * torch.rand(Pn, 1, generator=g),
                      (torch.rand(Pn, 1, generator=g) - 0.5) * 13.0 + CENTRE[1]], 1)
    bad = ~torch.isfinite(rv["means3D"])
    rv["means3D"] = torch.where(bad, rv["means3D"], good).contiguous()
    params = params_of(rv)
    for k, src in (("logit_opacities", "opacities"), ("log_scales", "scales")):       # keep the case's non-finite / out-of-range rows non-finite
        params[k] = torch.where(torch.isfinite(params[k]), params[k], torch.full_like(params[k], float("nan")))
    params = {k: v.to(device) for k, v in params.items()}
    n_bad_rows = int((~torch.isfinite(torch.cat([v.reshape(Pn, -1).cpu() for v in params.values()], 1))).any(1).sum())
    assert n_bad_rows >= 20, n_bad_rows
    got = run(params, camera(W, H, device), *BAND)
    for k in ("free_opacity", "free_map_binary", "visible_rgb", "visible_map_binary"):
        assert np.isfinite(got[k].astype(np.float64)).all(), k
    assert set(np.unique(got["free_map_binary"])) <= {0, 1} and set(np.unique(got["visible_map_binary"])) <= {0, 1}
    assert (got["free_opacity"] >= 0).all() and (got["free_opacity"] <= 1).all()
    assert (got["free_opacity"] > 0).any() and (got["visible_map_binary"] == 0).any()
    print(f"[topdown nonfinite] rows with a non-finite parameter {n_bad_rows}/{Pn}; touched pixels {(got['visible_map_binary'] == 0).sum()}")


def check_integer_artefacts(device, oracle32, N, W, H, iso=False):
    """item 6: radii, rects, counts, sorted ids and ranges of the banded per-Gaussian stage, bit-identical to the fp32 oracle of the FULL scene
    (inputs: the library's own activations of the parameters -- the kernels' __expf / sigmoid are not torch's to the bit)"""
    params = scene_params(N, W, H, device, iso)
    cam = camera(W, H, device)
    got = run(params, cam, *BAND)
    util.LAST.clear(); util.LAST.update(got["state"])
    art = util.artefacts()
    rv = library_activation(params)
    ref = util.run_oracle(oracle32, cam, rv)
    live = ref["radii"] > 0
    assert int(got["state"]["D"]) == ref["D"] and ref["D"] > 0
    assert np.array_equal(got["state"]["radii"].cpu().numpy(), ref["radii"])
    assert np.array_equal(art["tiles_touched"], ref["tiles_touched"])
    assert np.array_equal(art["rect"][live], ref["rect"][live])
    assert art["offsets"] is None                                          # (top-down grids are on the tile-binning path)
    assert np.array_equal(art["keys_sorted"], ref["keys_sorted"])
    assert np.array_equal(art["point_list"], ref["ids_sorted"])
    rg = art["ranges"].copy()
    rg[rg[:, 0] == rg[:, 1]] = 0
    assert np.array_equal(rg, ref["ranges"])
    # the per-Gaussian floats too; the opacity carries the band bit as its sign and nothing else
    assert np.array_equal(art["geom"][live, 0:2], ref["xy"][live]) and np.array_equal(art["geom"][live, 9], ref["depth"][live])
    # (the conic comes from scales / rotations activated inside the per-Gaussian kernel, the oracle's from the activation kernel's: two translation
    # units, one built without FMA contraction -- equal to the last bits only on the emulator; the integer artefacts above do not notice)
    assert np.allclose(art["geom"][live][:, [2, 3, 4]], ref["conic_opacity"][live][:, :3], rtol=1e-4, atol=1e-7)
    assert np.allclose(np.abs(art["geom"][live, 5]), ref["conic_opacity"][live][:, 3], rtol=1e-6, atol=0)
    band = in_band(params["means3D"].cpu(), *BAND).numpy()
    assert np.array_equal(np.signbit(art["geom"][live, 5]), band[live])
    assert 0 < int(band[live].sum()) < int(live.sum())
    print(f"[topdown artefacts] N={N} {W}x{H}: D={ref['D']}, {int(live.sum())} visible, {int(band[live].sum())} of them in band: bit-identical")


def library_activation(params):
    """render variables from the parameters through the LIBRARY's activation kernel (activate.hip: the formulas of the raw-parameter
    per-Gaussian kernels, identity pose)"""
    return _activate_forward(params)


def _activate_forward(params):
    import ctypes as C
    from activesplat_amd import _lib
    lib = _lib.get()
    dev = params["means3D"].device
    P = int(params["means3D"].shape[0])
    iso = 1 if params["log_scales"].shape[1] == 1 else 0
    out = dict(means3D=torch.empty(P, 3, device=dev), rotations=torch.empty(P, 4, device=dev), opacities=torch.empty(P, 1, device=dev),
               scales=torch.empty(P, 3, device=dev))
    pose = (C.c_float * 7)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    _lib.check(lib.gs_activate_forward(P, iso, pose, R._ptr(params["means3D"]), R._ptr(params["unnorm_rotations"]), R._ptr(params["logit_opacities"]),
                                       R._ptr(params["log_scales"]), R._ptr(out["means3D"]), R._ptr(out["rotations"]), R._ptr(out["opacities"]),
                                       R._ptr(out["scales"]), R._stream(dev)))
    out["colors_precomp"] = params["rgb_colors"]
    return out


def _composition(params, cam, how):
    """what topdown_maps replaces, on the same library: cut_gaussian_by_height, then two rasteriser calls -> (free opacity [H, W], colour [3, H, W])
    how = "activated": the library's activation kernel (activate.hip) + GaussianRasterizer, the call a port of visualizer.py makes;
    how = "raw"      : render_rgbd_raw, the rasteriser call that activates inside its per-Gaussian kernel (SplatMapper.render_rgbd's)"""
    H, W = int(cam.image_height), int(cam.image_width)
    cut = IO.cut_gaussian_by_height({k: v.clone() for k, v in params.items()}, *BAND)
    if how == "activated":
        sub = util.run_product(cam, _activate_forward(cut))["opacity"]
        full = util.run_product(cam, _activate_forward(params))["color"]
    else:
        ident = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]

        def raw(p):
            with torch.no_grad():
                return R.render_rgbd_raw(cam, p["means3D"], torch.empty(0, device=p["means3D"].device), p["logit_opacities"], p["log_scales"],
                                         p["unnorm_rotations"], ident, colors_precomp=p["rgb_colors"])
        sub, full = raw(cut)[3].cpu().numpy(), raw(params)[0].cpu().numpy()
    return sub.reshape(H, W), full.reshape(3, H, W), int(cut["means3D"].shape[0])


def _differing_pixels(got, free_opacity, color):
    rgb = to_bytes(color)
    return dict(free_opacity=int((free_opacity != got["free_opacity"]).sum()),
                free_map_binary=int(((free_opacity <= np.float32(0.4)).astype(np.uint8) != got["free_map_binary"]).sum()),
                visible_rgb=int((rgb != got["visible_rgb"]).any(-1).sum()),
                visible_map_binary=int(((TD.rgb_to_grey_u8(rgb) == 255).astype(np.uint8) != got["visible_map_binary"]).sum()))


def check_equivalence(device, N, W, H, iso=False):
    """item 7: topdown_maps against what it replaces ON THE SAME LIBRARY -- cut_gaussian_by_height, two rasteriser calls, thresholds on the host.
    The number of differing pixels per output is reported and must be 0: same per-entry arithmetic in the same order."""
    params = scene_params(N, W, H, device, iso)
    cam = camera(W, H, device)
    got = run(params, cam, *BAND)
    out = {}
    for how in ("raw", "activated"):
        free_opacity, color, n_band = _composition(params, cam, how)
        out[how] = _differing_pixels(got, free_opacity, color)
        print(f"[topdown equivalence, {how}] N={N} {W}x{H} {'iso' if iso else 'aniso'}: in band {n_band}/{N}; differing pixels {out[how]}")
        if how == "activated":
            # On the device the activation kernel (activate.hip, built with FMA contraction) and the per-Gaussian kernel (preprocess.hip, built
            # without: the bit-level spec) round the normalised quaternion and the frame transform differently in the last bit, so this
            # composition's INPUTS to the raster pass are not the fused call's to the bit; its opacity can then differ in the last bits of a few
            # pixels (measured on the MI355X: 0-2 of 108 000 - 135 424; on the emulator, one set of flags, 0).  The blend is not the cause: the
            # "raw" composition, which activates inside the same per-Gaussian kernel, must give 0.  What is asserted here is the project's
            # float tolerance.
            assert np.allclose(free_opacity, got["free_opacity"], rtol=RTOL, atol=ATOL)
    assert all(v == 0 for v in out["raw"].values()), out
    return out


def check_mapper(device, frames=3, W=64, H=48):
    """item 8: SplatMapper.topdown_maps after a few mapped frames of the synthetic sequence -- the same tensors as topdown_maps on the
    mapper's parameters, and both map values occur in both maps"""
    from activesplat_amd import synthetic as syn
    from activesplat_amd.mapper import SplatMapper
    gt = syn.shell_scene(3000, seed=2, W=W, H=H)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=frames), device=device)
    for fr in syn.orbit_sequence(gt, frames, W, H, device):
        mp.run(fr)
    m3 = mp.params["means3D"].detach()
    centre = (float(m3[:, 0].mean()), float(m3[:, 2].mean()))
    ext = (2.2 * float((m3[:, 0] - centre[0]).abs().max()), 2.2 * float((m3[:, 2] - centre[1]).abs().max()))
    upper, lower = float((-m3[:, 1]).quantile(0.3)), float((-m3[:, 1]).quantile(0.8))
    got = mp.topdown_maps(centre, ext, (120, 150), upper, lower)
    want = TD.topdown_maps(mp.params, TD.topdown_camera(centre, ext, (120, 150), device=device), upper, lower)
    for k in got._fields:
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert got.free_opacity.shape == (150, 120) and got.visible_rgb.shape == (150, 120, 3)
    ff, uf = float(got.free_map_binary.float().mean()), float(got.visible_map_binary.float().mean())
    print(f"[topdown mapper] {m3.shape[0]} Gaussians after {frames} frames: {ff * 100:.1f} % free, {uf * 100:.1f} % unseen")
    assert 0.0 < ff < 1.0 and 0.0 < uf < 1.0


def check_optimistic_launch(device, N=3000, W=120, H=150, raise_log_scales=8.0):
    """The twin of parity_cases.check_optimistic_launch for the top-down route: a tick's binning workspace is sized from the previous tick of its
    (P, W, H) stream.  An exact launch, a hit, a miss (the same map with its log scales raised by 8: 4 490 -> 60 429 tile instances on
    the emulated kernels against a stored guess of 9 708, re-launched with exact sizes), a hit at the grown capacity and a hit with a much larger capacity than needed must all reproduce the
    exactly-sized maps bit for bit, and the route counts its hits and misses like the rasteriser's own."""
    params = scene_params(N, W, H, device)
    cam = camera(W, H, device)
    small = lambda: TD.topdown_maps(params, cam, *BAND)                                  # noqa: E731
    big = dict(params, log_scales=params["log_scales"] + raise_log_scales)
    large = lambda: TD.topdown_maps(big, cam, *BAND)                                     # noqa: E731
    was = R.optimistic
    try:
        R.optimistic = False
        exact_small, exact_large = small(), large()
        R.optimistic = True
        R._capacity.clear()
        R.last_stats.pop("optimistic_hits", None); R.last_stats.pop("optimistic_misses", None)
        got = [small(), small()]                 # no guess yet: exact; then a hit
        assert R.last_stats.get("optimistic_hits", 0) == 1 and R.last_stats.get("optimistic_misses", 0) == 0
        d_guess = R._capacity[("topdown", N, W, H, params["means3D"].device.index)][0]
        got.append(large())                      # miss: D grows far beyond 1.25 x + 4096
        print(f"[topdown optimistic] stored guess {d_guess}, tile instances of the large tick {R.last_stats['num_rendered']}")
        assert R.last_stats["num_rendered"] > d_guess and R.last_stats["optimistic_misses"] == 1
        got += [large(), small()]                # hit at the grown capacity; hit with a much larger capacity than needed
        assert R.last_stats["optimistic_hits"] == 3 and R.last_stats["optimistic_misses"] == 1
        for step, (m, ref) in enumerate(zip(got, (exact_small, exact_small, exact_large, exact_large, exact_small))):
            for k in m._fields:
                assert torch.equal(getattr(m, k), getattr(ref, k)), (step, k)
        assert not torch.equal(exact_small.visible_rgb, exact_large.visible_rgb)
    finally:
        R.optimistic = was
        R._capacity.clear()
