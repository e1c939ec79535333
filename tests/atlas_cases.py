"""The multi-view atlas render (GsCamera.num_views > 1, gs_atlas_layout, rasterizer.render_views) VIEW BY VIEW against the oracles, shared by the
host-emulated kernel tests (tests/test_atlas.py) and the device tests (tests/test_gpu_atlas.py).

The atlas is the path under every planner decision (look_around, look_around_nodes and what is built on them) and has code of its own in the
per-Gaussian kernels (the view index of a block, the per-view matrices and camera centre, the rect clamped to the view's columns and moved
to its slot, the slot offset added to the pixel mean in fp32), in what binning and blend see (one image of V gxv tile columns) and on the host.
The older atlas tests compare it with the product's own single-view renders under allclose or a share rule; a wrong view index, a rect that
leaks into the neighbouring slot or a padding row that becomes visible fits inside those.

REFERENCES, per view v, from that view's settings alone: the fp32 and the fp64 oracle (util.run_oracle), and R64_v = blendpix_cases.replay (fp64)
of the fp64 oracle's record with the x of every row moved by

    delta_i = fl32(x32_i + 16 gxv v) - (x32_i + 16 gxv v),                  x32 = the fp32 oracle's pixel x (never the kernel's record)

which is all that the slot does to a view (include/gsplat_hip.h, "THE SLOT RULE"): the differences between a view of the atlas and its
single-view render -- the alpha >= 1/255 decisions that flip in late slots included -- are predicted pixel by pixel instead of tolerated.

RULES.  No pixel, no row and no view is excused and there is no second tier.  rows = virtual P / V.
  integer artefacts, exact: radii and tile counts of rows [v rows, v rows + P) are the fp32 oracle's of view v, the padding rows behind them hold
    0 and 0; the rect of a live row is the oracle's with both x bounds moved by v gxv; D is the sum of the views' D; the list of atlas tile
    (ty, v gxv + tx) is the oracle's sorted list of view v's tile (tx, ty) with v rows added to every id (depth ties as
    parity_cases.check_forward takes them: in the oracle's order, by index -- equal view depths do occur, 2 of 255 rows in `pairs_255`);
    n_contrib at every pixel is the shifted replay's.
  record, live rows, bit for bit: x == fl32(x32 + 16 gxv v), y, conic, opacity and depth the fp32 oracle's (what parity_cases.check_forward
    compares for one view); colours that were handed in are equal too.
  pixels, every value of colour, depth and opacity as returned and of final T from the image state:
    |o_k - R64_v| <= min(2 |o_32 - o_64| + FLOOR_F A_p, cap_of(FLOOR_F, n_pairs) A_p);  a pixel nothing contributes to is exactly bg, 0, 0, T = 1.
o_32 / o_64: the two oracles' images of the view; A_p, n_pairs: the shifted replay's.  FLOOR_F, cap_of, the two windows and the 3 % dimming step
are blendpix_cases' own, unchanged; test_atlas.test_fp32_oracle_alone_stays_under_half_the_floor measures the fp32 oracle's largest
|o_32 - o_64| / A_p over every case here and holds it to FLOOR_F / 2.  The only other figure is SETTLE_CAP: settling (a Gaussian that owns a
pixel inside either window on the shifted replay of any view is dimmed by 3 % until none is left) may touch fewer than 5 % of a scene, asserted
from the references alone.

profiles/README.md, "Atlas, view by view", holds the measured figures."""
import numpy as np
import torch

from activesplat_amd import lookaround as LA
from activesplat_amd import rasterizer as R
from activesplat_amd import synthetic as syn
from activesplat_amd import visibility as VIS
from activesplat_amd.camera import setup_camera
from tests import blendpix_cases as bp
from tests import cluster_cases as cc
from tests import parity_cases as pc
from tests import rowgrad_cases as rg
from tests import util

SETTLE_CAP = 0.05
#: the factor on blendpix's two windows that makes the alpha window parity_cases.THRESHOLD_WINDOW: for the oracles' own, unshifted records (_settle)
OWN_WIDEN = pc.THRESHOLD_WINDOW / bp.ALPHA_WINDOW
OUTPUTS = ("color", "depth", "opacity", "final_T")

#: name -> (V, W, H, P); P of `segmented` is what blendpix_cases._segmented_parts makes
CASES = dict(pano3=(3, 120, 150, 1500), pano63=(63, 120, 150, 1500), pairs_255=(2, 48, 40, 255), pairs_256=(2, 48, 40, 256),
             pairs_257=(2, 48, 40, 257), strip64=(64, 40, 40, 800), sh48=(3, 64, 48, 600), sh4=(2, 64, 48, 300), cov=(3, 64, 48, 600),
             edges=(3, 120, 150, 300), empty_view=(3, 64, 48, 400), tall_radix=(64, 40, 704, 3000), segmented=(2, 48, 40, 8300))
NAMES = list(CASES)


class Case:
    """cams: the V settings on the host; rv: the inputs on the host -- or params: the mapper's parameters, activated by the kernels of the
    device under test exactly as look_around activates them (the panoramas of look_around are then the very atlas that is judged)."""

    def __init__(self, name, cams, rv=None, params=None):
        self.name, self.cams, self.rv, self.params = name, cams, rv, params
        self.V, self.W, self.H = len(cams), int(cams[0].image_width), int(cams[0].image_height)
        self.gxv = (self.W + 15) // 16
        self.bg = tuple(float(b) for b in cams[0].bg.reshape(-1).tolist())
        self.dimmed = set()

    def inputs(self, device):
        """-> the keyword tensors of render_views on `device`"""
        if self.params is None:
            return {k: v.to(device) for k, v in self.rv.items()}
        rv = LA._world_rendervar({k: v.to(device) for k, v in self.params.items()})
        rv.pop("means2D")
        return rv

    def dim(self, hits):
        hits = sorted(hits)
        self.dimmed |= set(hits)
        if self.params is None:
            o = self.rv["opacities"].clone()
            o[hits] *= 0.97
            self.rv = dict(self.rv, opacities=o)
        else:
            # the same 3 % on the activated opacity, taken in the parameter: logit(0.97 sigmoid(l))
            logit = self.params["logit_opacities"].clone()
            o = 0.97 * torch.sigmoid(logit[hits].double())
            logit[hits] = torch.log(o / (1.0 - o)).float()
            self.params = dict(self.params, logit_opacities=logit)


def _cam(W, H, w2c, bg=(0.0, 0.0, 0.0), sh_degree=0, fx=None):
    return setup_camera(W, H, syn.intrinsics(W, H, fx=fx), w2c, device="cpu", bg=bg, sh_degree=sh_degree)


def _look_cams(poses):
    k3 = LA.look_around_k()
    return [setup_camera(LA.LOOK_W, LA.LOOK_H, k3, np.linalg.inv(LA.rot_axis(np.asarray(p, np.float64), "y", np.deg2rad(LA.LOOK_HFOV_DEG * i))), LA.VIZ_NEAR,
                         LA.VIZ_FAR, device="cpu", bg=(1.0, 1.0, 1.0)) for p in poses for i in range(int(360 / LA.LOOK_HFOV_DEG))]


def _activated(p):
    return {k: v.contiguous() for k, v in syn.activate(p).items()}


def _ring(V, W, H, bg=(0.0, 0.0, 0.0), step=0.02, fx=None):
    return [_cam(W, H, util.pose(yaw=2 * np.pi * v / V, t=(step * v, 0.0, 0.0)), bg=bg, fx=fx) for v in range(V)]


def _to_world(part, w2c):
    """Splats laid out in a camera's frame (blendpix_cases._splats) -> the world frame of that camera's pose (rotations about y only)"""
    Rm, t = torch.as_tensor(w2c[:3, :3]), torch.as_tensor(w2c[:3, 3])
    out = dict(part)
    out["means3D"] = (part["means3D"] - t) @ Rm                                   # R^T (c - t), row vectors
    return out


def _edge_parts(g, W, H, n, n_fill):
    """In one camera's frame: n round splats of 20 .. 60 px radius (3 sigma; most of them near 20 -- the number of rim pixels a splat has near
    alpha = 1/255 grows with sigma^2, and settling may touch 5 % of the scene), five in twelve with their mean up to one radius outside the
    left edge, five in twelve outside the right edge, the rest within one radius inside either edge; and n_fill splats of 2 .. 4 px all over
    the view"""
    rad = 20.0 + 40.0 * bp._rand(g, n) ** 3
    f = bp._rand(g, n)
    side = torch.arange(n) % 12
    u = torch.where(side < 5, -f * rad, torch.where(side < 10, (W - 1.0) + f * rad, torch.where(side < 11, f * rad, (W - 1.0) - f * rad)))
    v = 10.0 + (H - 20.0) * bp._rand(g, n)
    sp = bp._splats(g, W, H, u, v, bp._depths(g, n, 1.0, 2.5), rad / 3.0, 0.1 + 0.4 * bp._rand(g, n))
    fill = bp._field(g, W, H, (0.0, 0.0, float(W), float(H)), n_fill, (2.0, 4.0), (0.1, 0.6), z=(2.5, 4.0))
    out = {k: torch.cat([sp[k], fill[k]], 0) for k in sp}
    s = out["scales"][:, :1]
    out["scales"] = torch.cat([s, s, s], 1)                                       # spheres: no orientation to carry between the views' frames
    return out


def _join(parts, g):
    rv = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    perm = torch.randperm(rv["means3D"].shape[0], generator=g)
    return {k: v[perm].float().contiguous() for k, v in rv.items()}


def _build(name):
    V, W, H, P = CASES[name]
    if name in ("pano3", "pano63"):
        # the planner's calls: look_around at cluster_cases.base_pose, look_around_nodes over 21 nodes spread as node_positions spreads them
        params = cc.shell_params("cpu", n=P)
        poses = [cc.base_pose()] if name == "pano3" else [VIS.node_pose(cc.base_pose(), p) for p in cc.node_positions(21)]
        return Case(name, _look_cams(poses), params=params)
    if name.startswith("pairs_"):
        rv = util.scene(P, W, H, seed=4)[1]
        return Case(name, [_cam(W, H, util.pose(0.0)), _cam(W, H, util.pose(0.35, (0.1, 0.0, 0.2)))], rv={k: v.contiguous() for k, v in rv.items()})
    if name in ("strip64", "tall_radix"):
        rv = _activated(syn.shell_scene(P, seed=2, W=W, H=H))
        fx = None
        if name == "tall_radix":
            # a focal length of 100 px (a view of 23 x 148 degrees; at the W / 2 = 20 px of the other cases the 704 rows would span 173 degrees
            # and the fp32 oracle alone is 1.4e-2 of A_p off at a splat near the pole).  Splats of 1.5 px (smaller ones move the fp32 oracle itself past half the floor: the alpha of a 1 px splat at row 700 feels the rounding of its centre): the number of a splat's rim pixels
            # near alpha = 1/255 grows with its area, and the settling of 64 views of 28160 pixels may touch 5 % of the scene
            fx = 100.0
            rv["scales"] = (0.3 * rv["scales"]).contiguous()
        else:
            rv["scales"] = (0.7 * rv["scales"]).contiguous()                       # (the same, for 64 views of 800 splats)
        return Case(name, _ring(V, W, H, bg=(1.0, 1.0, 1.0), fx=fx), rv=rv)
    if name in ("sh48", "sh4"):
        deg = 3 if name == "sh48" else 1
        rv = _activated(syn.make_params(P, W, H, seed=11, sh_degree=3))
        rv["shs"] = rv["shs"][:, :(deg + 1) ** 2].contiguous()
        spots = [(0.0, (0.0, 0.0, 0.0)), (0.3, (0.6, -0.3, 0.3)), (-0.3, (-0.7, 0.4, 0.5))][:V]
        return Case(name, [_cam(W, H, util.pose(y, t), bg=(0.2, 0.3, 0.1), sh_degree=deg) for y, t in spots], rv=rv)
    if name == "cov":
        rv = _activated(syn.make_params(P, W, H, seed=12))
        cov = dict(means3D=rv["means3D"], opacities=rv["opacities"], colors_precomp=rv["colors_precomp"], cov3D_precomp=rg._cov3d(rv))
        return Case(name, [_cam(W, H, util.pose(y, t)) for y, t in ((0.0, (0.0, 0.0, 0.0)), (0.35, (0.1, 0.0, 0.2)), (-0.4, (-0.2, 0.05, 0.4)))], rv=cov)
    if name == "edges":
        g = bp._gen(sum(map(ord, name)))
        w2cs = [util.pose(2 * np.pi * v / V) for v in range(V)]
        return Case(name, [_cam(W, H, w, bg=(0.3, 0.1, 0.7)) for w in w2cs], rv=_join([_to_world(_edge_parts(g, W, H, 24, P // V - 24), w) for w in w2cs], g))
    if name == "empty_view":
        rv = util.scene(P, W, H, seed=5)[1]
        return Case(name, [_cam(W, H, w, bg=(0.3, 0.1, 0.7)) for w in (util.pose(0.0), util.pose(np.pi), util.pose(np.pi, (0.1, 0.0, -0.1)))],
                    rv={k: v.contiguous() for k, v in rv.items()})
    if name == "segmented":
        g = bp._gen(sum(map(ord, name)))
        return Case(name, [_cam(W, H, util.pose(0.0)), _cam(W, H, util.pose(0.0, (0.02, -0.01, 0.0)))], rv=bp._cat(bp._segmented_parts(g, W, H, 16.0, 16.0), g))
    raise KeyError(name)


# ---- references ----------------------------------------------------------------------------------------------------------------------------
def _shifted(f, x32, off):
    """An oracle's forward with the slot's rounding put on its x: delta = fl32(x32 + off) - (x32 + off)"""
    x32 = np.asarray(x32, np.float32)
    delta = (x32 + np.float32(off)).astype(np.float32).astype(np.float64) - (x32.astype(np.float64) + float(off))
    rec = dict(f)
    xy = np.asarray(f["xy"], np.float64).copy()
    xy[:, 0] += delta
    rec["xy"] = xy
    return rec


def _oracles(case, rv, o64, o32):
    out = []
    for v, cam in enumerate(case.cams):
        f64, f32 = util.run_oracle(o64, cam, rv), util.run_oracle(o32, cam, rv)
        off = 16 * case.gxv * v
        x32 = np.asarray(f32["xy"], np.float32)[:, 0]
        out.append(dict(f64=f64, f32=f32, off=off, s64=_shifted(f64, x32, off), s32=_shifted(f32, x32, off)))
    return out


def _wide_window_rows(rec, window):
    """The rows for which parity_cases.threshold_gaussians can say more than the replay's own alpha window: it tests the same alpha of the same
    record against `window`, widened to 4 (eps / 2) S where the exponent's terms are large.  S <= (|a| / 2 + |c| / 2 + |b|) (radius + 2)^2 over
    the box it scans; a row whose bound stays under `window` is left to the replay."""
    co, rad = np.abs(np.asarray(rec["conic_opacity"], np.float64)), np.asarray(rec["radii"], np.float64)
    s_max = (0.5 * co[:, 0] + 0.5 * co[:, 2] + co[:, 1]) * (rad + 2.0) ** 2
    return np.nonzero((rad > 0) & (4.0 * 0.5 * 1.1920929e-07 * s_max >= window))[0]


def _oracles_differ(r):
    """The two oracles' own images of a view differ in n_contrib or by more than half the floor somewhere (A_p: the shifted replay's)"""
    if not np.array_equal(r["f32"]["n_contrib"], r["f64"]["n_contrib"]):
        return True
    _, A = bp.replay_images(r["rp"])
    o32, o64 = _images(r["f32"]), _images(r["f64"])
    return any((np.abs(o32[k] - o64[k]) > 0.5 * bp.FLOOR_F * A[k]).any() for k in OUTPUTS)


def _settle(case, device, o64, o32):
    """blendpix_cases._settle over the views: the windows are evaluated on the SHIFTED records (the fp64 one 1.05 x as wide, then the fp32 one
    once that is clean) -- and on the oracles' own, unshifted records as well: the rule's 2 |o_32 - o_64| is taken between the two oracles'
    images of the view, and in a late slot a pixel can sit at a threshold of the unshifted record while the shifted one is 4e-4 (relative)
    away from it (before this, the two oracles took different decisions at one pixel each of `pano63`, `strip64` and `tall_radix`).  Only the
    views in which the two oracles do differ -- in n_contrib, or by more than FLOOR_F / 2 of A_p -- are looked at this way.  There the
    two oracles only have to agree with each other, so the windows are parity_cases.THRESHOLD_WINDOW wide, the project's figure for two fp32
    evaluation orders of one alpha; the full blendpix windows would also dim away every flip that the shifted reference is there to predict"""
    for _ in range(40):
        rv = {k: v.cpu() for k, v in case.inputs(device).items()}
        views = _oracles(case, rv, o64, o32)
        hits = set()
        for keys, widen in ((("s64", "f64"), 1.05), (("s32", "f32"), 1.0)):
            for r in views:
                for key in keys:
                    if key[0] == "f" and (r["off"] == 0 or not _oracles_differ(r)):
                        continue                                                   # (slot 0: the shifted record is the oracle's own)
                    rec = r[key]
                    rp = bp.replay(rec, case.W, case.H, case.bg, widen=widen * (1.0 if key[0] == "s" else OWN_WIDEN))
                    hits |= {h[0] for h in rp.alpha_margin} | {h[0] for h in rp.stop_margin}
                    if key[0] == "s":
                        hits |= {h[0] for h in pc.threshold_gaussians(rec, _wide_window_rows(rec, widen * bp.ALPHA_WINDOW), case.W, case.H, window=widen * bp.ALPHA_WINDOW)}
                    if key == "s64":
                        r["rp"] = rp                                               # (the windows only fill the margin lists: this is THE shifted replay)
            if hits:
                break
        if not hits:
            return rv, views
        case.dim(hits)
    raise AssertionError((case.name, "threshold pixels left after 40 rounds"))


_REFS = {}


def reference(name, device, o64, o32):
    """-> (case, ref) once per (case, device): the settled case and, per view, the two oracles' forwards, the shifted replay `rp` and the number
    of pixels whose n_contrib the shift moves (`flips`)"""
    key = (name, str(device))
    if key not in _REFS:
        case = _build(name)
        rv, views = _settle(case, device, o64, o32)
        for v, r in enumerate(views):
            f64, f32 = r["f64"], r["f32"]
            for k in ("radii", "rect", "tiles_touched", "ranges", "ids_sorted"):
                assert np.array_equal(f64[k], f32[k]), (name, v, k, "the two oracles disagree on an integer artefact: move the scene")
            assert not r["rp"].alpha_margin and not r["rp"].stop_margin, (name, v)
            r["flips"] = int((r["rp"].n_contrib != np.asarray(f64["n_contrib"], np.int64)).sum())
        P = int(rv["means3D"].shape[0])
        assert len(case.dimmed) < SETTLE_CAP * P, (name, "settling dimmed", len(case.dimmed), "of", P)
        ref = dict(rv=rv, views=views, P=P, flips=sum(r["flips"] for r in views), dimmed=len(case.dimmed))
        ref["oracle32_error"] = oracle_pixel_error(case, ref)
        print(f"[atlas] {name}: V {case.V}, {case.W} x {case.H}, P {P}; D per view {[int(r['f32']['D']) for r in views][:8]}{' ...' if case.V > 8 else ''}; "
              f"predicted flips {ref['flips']}; dimmed Gaussians {ref['dimmed']}; fp32 oracle alone {ref['oracle32_error'][0]:.3e} of A_p ({ref['oracle32_error'][1]})")
        _REFS[key] = (case, ref)
    return _REFS[key]


def _images(f):
    return dict(color=np.asarray(f["color"], np.float64), depth=np.asarray(f["out_depth"], np.float64), opacity=np.asarray(f["opacity"], np.float64),
                final_T=np.asarray(f["final_T"], np.float64)[None])


def oracle_pixel_error(case, ref):
    """The fp32 oracle's largest |o_32 - o_64| / A_p over every view, pixel and output -> (value, (view, output)); the oracles alone"""
    worst = (0.0, None)
    for v, r in enumerate(ref["views"]):
        _, A = bp.replay_images(r["rp"])
        o32, o64 = _images(r["f32"]), _images(r["f64"])
        for k in OUTPUTS:
            m = A[k] > 0
            if m.any():
                worst = max(worst, (float((np.abs(o32[k] - o64[k])[m] / A[k][m]).max()), (v, k)))
    return worst


# ---- what a case is there for: asserted from the oracles ---------------------------------------------------------------------------------------
def assert_case(case, ref):
    name, views = case.name, ref["views"]
    V, W, H, P = CASES[name]
    assert (case.V, case.W, case.H) == (V, W, H) and ref["P"] == P, (name, ref["P"])
    live = [np.asarray(r["f32"]["radii"]) > 0 for r in views]
    if name != "empty_view":
        assert all(m.any() for m in live), (name, "every view sees something")
    if name.startswith("pano"):
        assert W % 16 == 8 and case.bg == (1.0, 1.0, 1.0)
    if name == "pano63":
        assert V * case.gxv * ((H + 15) // 16) == 5040
        assert ref["flips"] >= 1, (name, "the shifted and the unshifted replay agree on n_contrib everywhere: the predicted flips do not exist")
    if name.startswith("pairs_"):
        assert W % 16 == 0 and (-P) % 256 == {255: 1, 256: 0, 257: 255}[P]
    if name == "strip64":
        assert V == 64 and V * case.gxv * ((H + 15) // 16) == 576
    if name in ("sh48", "sh4"):
        M = int(ref["rv"]["shs"].shape[1])
        assert M == (16 if name == "sh48" else 4) and int(case.cams[0].sh_degree) == (3 if name == "sh48" else 1)
        pos = [c.campos.numpy() for c in case.cams]
        assert all(np.abs(pos[a] - pos[b]).max() > 0.3 for a in range(V) for b in range(a)), (name, "views at different positions")
        rgb = [np.asarray(r["f32"]["rgb"]) for r in views]
        differ = np.zeros(P, bool)
        for a in range(V):
            for b in range(a):
                differ |= live[a] & live[b] & (rgb[a] != rgb[b]).any(1)
        assert differ.sum() > 0.5 * P, (name, "colours that differ between the views", int(differ.sum()), P)
        if name == "sh48":
            clamped = np.zeros(P, bool)
            for v, r in enumerate(views):
                clamped |= live[v] & (np.asarray(r["f32"]["clamped"]) != 0).any(1)
            assert clamped.sum() >= 0.01 * P, (name, "rows with a clamped channel", int(clamped.sum()))
    if name == "cov":
        assert "cov3D_precomp" in ref["rv"] and "scales" not in ref["rv"]
    if name == "edges":
        left = right = outside = 0
        for v, r in enumerate(views):
            f = r["f32"]
            x, rad, rect = np.asarray(f["xy"], np.float64)[:, 0], np.asarray(f["radii"], np.float64), np.asarray(f["rect"])
            left += int((live[v] & (x - rad < 0) & (rect[:, 0] == 0)).sum())
            right += int((live[v] & (x + rad + 15.0 >= 16.0 * (case.gxv + 1)) & (rect[:, 2] == case.gxv)).sum())
            outside += int((live[v] & ((x < -0.5) | (x > W - 0.5))).sum())
            assert (rad[live[v]] >= 20).sum() >= 30, (name, v, "splats of 20 px and more")
        assert left >= 30 and right >= 30 and outside >= 10, (name, left, right, outside)
    if name == "empty_view":
        assert int(views[0]["f32"]["D"]) > 0 and int(views[1]["f32"]["D"]) == 0 and int(views[2]["f32"]["D"]) == 0
    if name == "tall_radix":
        assert V * case.gxv * ((H + 15) // 16) == 8448
    if name == "segmented":
        assert max(int(r["rp"].list_len.max()) for r in views) > 8192


# ---- the run -------------------------------------------------------------------------------------------------------------------------------
def _on(cam, device):
    return cam._replace(bg=cam.bg.to(device), viewmatrix=cam.viewmatrix.to(device), projmatrix=cam.projmatrix.to(device), campos=cam.campos.to(device))


def run(case, device, settings_on_device=False, as_list=False, expect_D=None):
    """render_views of the case inside a capture -> dict(color, depth, opacity [., H, AW] tensors, stride, state, art[, views: the list form])"""
    cams = [_on(c, device) for c in case.cams] if settings_on_device else case.cams
    with R.capture() as state:
        out = R.render_views(cams, return_atlas=not as_list, **case.inputs(device))
    # (D first: the decoding below indexes with the tile lists, and a frame with a rect in the wrong slot has other lists)
    assert expect_D is None or int(state["D"]) == expect_D, (case.name, "D is not the sum of the views' D", int(state["D"]), expect_D)
    util.LAST.clear(); util.LAST.update(state)
    got = dict(state=state, art=util.artefacts(), stride=int(state["view_stride"]), rows=int(state["rows_per_view"]))
    if as_list:
        got["views"] = out
    else:
        got.update(color=out[0], depth=out[1], opacity=out[2])
        assert out[3] == got["stride"]
    return got


REPORT = {}          # case -> dict(oracle32_error, kernel_error, flips, dimmed): the tests print it


def check_integers(case, ref, got):
    name, V, gxv, P = case.name, case.V, case.gxv, ref["P"]
    st, art, rows = got["state"], got["art"], got["rows"]
    Pv = int(st["P"])
    assert rows * V == Pv and rows == -(-P // 256) * 256 and int(st["W"]) == V * got["stride"] and got["stride"] == 16 * gxv, (name, rows, Pv, got["stride"])
    radii = st["radii"].cpu().numpy()
    gy = (case.H + 15) // 16
    assert int(st["D"]) == sum(int(r["f32"]["D"]) for r in ref["views"]), (name, "D", int(st["D"]))
    lists = []
    for v, r in enumerate(ref["views"]):
        f = r["f32"]
        own, pad = slice(v * rows, v * rows + P), slice(v * rows + P, (v + 1) * rows)
        assert np.array_equal(radii[own], f["radii"]), (name, v, "radii")
        assert np.array_equal(art["tiles_touched"][own], f["tiles_touched"]), (name, v, "tiles_touched")
        assert not radii[pad].any() and not art["tiles_touched"][pad].any(), (name, v, "a padding row is visible")
        live = np.asarray(f["radii"]) > 0
        want = np.asarray(f["rect"]).astype(np.int32) + np.array([v * gxv, 0, v * gxv, 0], np.int32)
        assert np.array_equal(art["rect"][own][live], want[live]), (name, v, "rect", np.nonzero((art["rect"][own] != want).any(1) & live)[0][:4].tolist())
        lists.append((np.asarray(f["ranges"]).astype(np.int64), np.asarray(f["ids_sorted"]).astype(np.int64) + v * rows))
    ranges, plist = art["ranges"].astype(np.int64), art["point_list"].astype(np.int64)
    at = 0
    for ty in range(gy):
        for v in range(V):
            rg_, ids = lists[v]
            for tx in range(gxv):
                s, e = rg_[ty * gxv + tx]
                a, b = ranges[ty * V * gxv + v * gxv + tx]
                assert b - a == e - s and (a == at or e == s), (name, "tile range", v, tx, ty, (int(a), int(b)), at, int(e - s))
                if e > s and not np.array_equal(plist[a:b], ids[s:e]):
                    raise AssertionError(f"{name}: the list of atlas tile ({ty}, {v * gxv + tx}) is not view {v}'s list of tile ({tx}, {ty}) + {v * rows}")
                at += int(e - s)
    assert at == int(st["D"]), (name, at)


def check_record(case, ref, got):
    name, P, rows = case.name, ref["P"], got["rows"]
    geom = got["art"]["geom"]
    for v, r in enumerate(ref["views"]):
        f = r["f32"]
        live = np.asarray(f["radii"]) > 0
        g = geom[v * rows:v * rows + P][live]
        xy = np.asarray(f["xy"], np.float32)[live]
        x = (xy[:, 0] + np.float32(r["off"])).astype(np.float32)
        assert np.array_equal(g[:, 0], x), (name, v, "record x is not fl32(x32 + 16 gxv v)", int((g[:, 0] != x).sum()))
        assert np.array_equal(g[:, 1], xy[:, 1]), (name, v, "record y")
        assert np.array_equal(g[:, 9], np.asarray(f["depth"], np.float32)[live]), (name, v, "record depth")
        assert np.array_equal(g[:, 2:6], np.asarray(f["conic_opacity"], np.float32)[live]), (name, v, "record conic / opacity")
        if "colors_precomp" in ref["rv"]:
            assert np.array_equal(g[:, 6:9], ref["rv"]["colors_precomp"].numpy()[live]), (name, v, "record colour")


def check_pixels(case, ref, got):
    name, W, H, S = case.name, case.W, case.H, got["stride"]
    art = got["art"]
    bg = np.asarray(case.bg, np.float64)
    worst_all = 0.0
    for v, r in enumerate(ref["views"]):
        rp = r["rp"]
        cols = slice(v * S, v * S + W)
        nc = art["n_contrib"][:, cols].astype(np.int64)
        bad = np.argwhere(nc != rp.n_contrib)
        if bad.size:
            y, x = bad[0]
            raise AssertionError(f"{name} view {v}: n_contrib differs from the shifted replay at {len(bad)} pixels, first ({x}, {y}): kernel {int(nc[y, x])}, "
                                 f"replay {int(rp.n_contrib[y, x])} (unshifted fp64 oracle {int(r['f64']['n_contrib'][y, x])})")
        k_img = dict(color=got["color"][:, :, cols], depth=got["depth"][:, :, cols], opacity=got["opacity"][:, :, cols])
        k_img = {k: t.cpu().numpy().astype(np.float64) for k, t in k_img.items()}
        k_img["final_T"] = art["final_T"][None, :, cols].astype(np.float64)
        R64, A = bp.replay_images(rp)
        o32, o64 = _images(r["f32"]), _images(r["f64"])
        cap = bp.cap_of(bp.FLOOR_F, rp.n_pairs)[None]
        un = ~rp.touched
        for k in OUTPUTS:
            g = k_img[k]
            assert np.isfinite(g).all(), (name, v, k)
            exact = dict(color=np.float32(bg).astype(np.float64).reshape(3, 1), depth=0.0, opacity=0.0, final_T=1.0)[k]
            assert (g[:, un] == exact).all(), (name, v, k, "a pixel nothing contributes to must be exactly bg / 0 / 0 / T = 1")
            err, e32 = np.abs(g - R64[k]), np.abs(o32[k] - o64[k])
            bound = np.where(un[None], np.inf, np.minimum(2.0 * e32 + bp.FLOOR_F * A[k], cap * A[k]))
            ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
            c, y, x = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            worst_all = max(worst_all, float((err / np.where(A[k] > 0, A[k], np.inf)).max()))
            if ratio[c, y, x] > 1.0:
                raise AssertionError(f"{name} view {v}: {k}: {int((ratio > 1.0).sum())} values outside the per-pixel bound, worst pixel ({x}, {y}) channel {c} "
                                     f"({bp.pixel_classes(rp, x, y)}): ratio {ratio[c, y, x]:.3f}, kernel {g[c, y, x]!r} shifted replay {R64[k][c, y, x]!r} "
                                     f"fp64 oracle {o64[k][c, y, x]!r} fp32 oracle {o32[k][c, y, x]!r}")
    REPORT[name] = dict(oracle32_error=ref["oracle32_error"][0], kernel_error=worst_all, flips=ref["flips"], dimmed=ref["dimmed"])
    print(f"[atlas] {name}: kernel's worst error {worst_all:.3e} of A_p (floor {bp.FLOOR_F:g}); fp32 oracle alone {ref['oracle32_error'][0]:.3e}; "
          f"predicted flips {ref['flips']}; dimmed Gaussians {ref['dimmed']}")


_GOT = {}


def check_case(name, device, o64, o32):
    """One case: what it is there for (from the oracles), then integers, record and every pixel of every view -> (case, ref, got)"""
    case, ref = reference(name, device, o64, o32)
    assert_case(case, ref)
    got = run(case, device, expect_D=sum(int(r["f32"]["D"]) for r in ref["views"]))
    bl = got["state"]["bl"]
    if name == "tall_radix":
        assert int(bl.path) == 2, int(bl.path)
    elif name == "segmented":
        assert int(bl.segments) > 1, int(bl.segments)
    else:
        assert int(bl.path) == 1, int(bl.path)
    if name == "empty_view":
        for v in (1, 2):
            t = got["art"]["ranges"].reshape((case.H + 15) // 16, case.V * case.gxv, 2)[:, v * case.gxv:(v + 1) * case.gxv]
            assert (t[..., 0] == t[..., 1]).all(), (name, v, "tile ranges of an empty view")
    check_integers(case, ref, got)
    check_record(case, ref, got)
    check_pixels(case, ref, got)
    _GOT[(name, str(device))] = got
    return case, ref, got


# ---- further checks --------------------------------------------------------------------------------------------------------------------------
def _judged(name, device, o64, o32):
    key = (name, str(device))
    if key not in _GOT:
        check_case(name, device, o64, o32)
    case, ref = _REFS[key]
    return case, ref, _GOT[key]


def check_settings_on_host_and_device(name, device, o64, o32):
    """All settings tensors on the host (one packed upload) and all on the device (stacked there): bit-identical atlases"""
    case, _ref, got = _judged(name, device, o64, o32)
    assert all(not c.viewmatrix.is_cuda for c in case.cams)
    dev = run(case, device, settings_on_device=True)
    for k in ("color", "depth", "opacity"):
        assert torch.equal(got[k], dev[k]), (name, k)
    for k in ("final_T", "n_contrib", "point_list", "ranges", "tiles_touched"):
        assert np.array_equal(got["art"][k], dev["art"][k]), (name, k)
    live = got["art"]["tiles_touched"] > 0                                         # (a culled row's record is never written)
    assert np.array_equal(got["art"]["geom"][live], dev["art"]["geom"][live]) and np.array_equal(got["art"]["rect"][live], dev["art"]["rect"][live]), name


def check_list_form(name, device, o64, o32):
    """The list form hands out views of ONE atlas tensor per output: view v is its columns [v stride, v stride + W), equal to the atlas that
    return_atlas=True returns, and its radii are the artefact rows [v rows, v rows + P)"""
    case, ref, got = _judged(name, device, o64, o32)
    lst = run(case, device, as_list=True)
    S, rows, P = lst["stride"], lst["rows"], ref["P"]
    assert len(lst["views"]) == case.V
    base = [t._base if t._base is not None else t for t in lst["views"][0]]
    for v, (color, radii, depth, opacity) in enumerate(lst["views"]):
        for t, b, k in ((color, base[0], "color"), (depth, base[2], "depth"), (opacity, base[3], "opacity")):
            assert t._base is b and tuple(b.shape[1:]) == (case.H, case.V * S) and t.storage_offset() == v * S and t.shape[2] == case.W, (name, v, k)
            assert t.stride() == b.stride(), (name, v, k)
            assert torch.equal(t, got[k][:, :, v * S:v * S + case.W]), (name, v, k)
        assert radii._base is base[1] and radii.storage_offset() == v * rows and radii.shape == (P,), (name, v)
        assert radii.data_ptr() == lst["state"]["radii"].data_ptr() + 4 * v * rows and torch.equal(radii, lst["state"]["radii"][v * rows:v * rows + P]), (name, v)


def _gather(got, n, views):
    cols = torch.cat([torch.arange(v * got["stride"], v * got["stride"] + LA.LOOK_W) for v in range(n * views)]).to(got["color"].device)
    return got["opacity"][0][:, cols], got["depth"][0][:, cols], (torch.clamp(got["color"][:, :, cols], min=0, max=1.0) * 255).byte()


def check_look_around(device, o64, o32):
    """look_around gathers exactly the columns of the atlas judged as `pano3`"""
    case, _ref, got = _judged("pano3", device, o64, o32)
    pano = LA.look_around({k: v.to(device) for k, v in case.params.items()}, cc.base_pose())
    op, dp, im = _gather(got, 1, 3)
    assert pano["opacity"].shape == (150, 360) and torch.equal(pano["opacity"], op)
    assert torch.equal(pano["depth"], dp.unsqueeze(-1)) and torch.equal(pano["rgb"], im.permute(1, 2, 0))


def check_look_around_nodes(device, o64, o32):
    """look_around_nodes(nodes_per_pass=21) over 21 nodes gathers exactly the columns of the atlas judged as `pano63`"""
    case, _ref, got = _judged("pano63", device, o64, o32)
    pano = VIS.look_around_nodes({k: v.to(device) for k, v in case.params.items()}, cc.base_pose(), cc.node_positions(21), nodes_per_pass=21)
    assert all(pano.valid) and pano.opacity.shape == (21, 150, 360)
    op, dp, im = _gather(got, 21, 3)
    assert torch.equal(pano.opacity, op.view(150, 21, 360).permute(1, 0, 2))
    assert torch.equal(pano.depth, dp.view(150, 21, 360).permute(1, 0, 2).unsqueeze(-1))
    assert torch.equal(pano.rgb, im.view(3, 150, 21, 360).permute(2, 1, 3, 0))
