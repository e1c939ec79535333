"""The per-Gaussian stage against the fp64 published-form reference (oracle/dense_torch.project_dense): ONE comparison rule, used by the
CPU tests (tests/test_projection_fp64.py: the fp32 oracle twin, the emulated kernels) and the GPU tests (tests/test_gpu_projection_fp64.py:
the HIP kernels).

Every bit-exact parity test holds the kernel's per-Gaussian records against oracle/gs_oracle.c in fp32, which evaluates the same
(factorised) formula operation for operation.  This rule compares them with an INDEPENDENT evaluation in fp64 in the published order
(T Sigma T^T, k00 k11 - k01^2), so a mistake the kernel and its twin share (a clamp limit, the lambda floor, the ceil, the rect's +15, an
SH constant) is caught.

The tolerances are the per-Gaussian first-order fp32 bounds that project_dense returns with each quantity (its docstring; u = 2^-24):
a sum of n terms rounds by at most n u of the sum of the terms' magnitudes, a product or a quotient by u of its value, and each step's
bound carries the bounds of its operands forward to first order.  None is taken from the product's output.  Per quantity:

  * depth tz: 4 u of |m2 px| + |m6 py| + |m10 pz| + |m14| (3 products, 3 sums);
  * pixel mean: the clip-space rows to 4 u of their terms' magnitudes, the division by hw + 1e-7 and the viewport map
    ((ndc + 1) W - 1) / 2 with 1.5 u of (|ndc| + 1) W;
  * the 2-D covariance entries: J to 4-6 u (plus the depth's error where tz is close to the near plane), T = J W to 3 u of |J||W|,
    M = R diag(s) to 6 u of |R||s| (|R| with every difference inside R turned into a sum), A = T M and K = A A^T each to 3 u of the
    magnitudes, the errors of the factors carried forward; for a given Sigma, K = T Sigma T^T to 7 u of |T||Sigma||T|^T;
  * x = mid^2 - det: 2 mid dmid + ddet + 3 u (mid^2 + k00 k11 + k01^2) -- dx = kappa u (mid^2 + det) of the issue with the entry errors
    written out (kappa ~ 2 x 33 + 3 for scale + rotation input); sqrt(max(0.1, x)) moves by min(sqrt(dx), dx / (2 sqrt(x))): the
    cancellation of mid^2 - det for a large, near-isotropic splat puts up to sqrt(kappa u) mid on lambda, which is why the radius
    bound is per Gaussian.  d(3 sqrt(lambda)) = 3 dlambda / (2 sqrt(lambda)) + 2 u (3 sqrt(lambda));
  * rect edge arguments (px -+ r [+ 15]) / 16: the pixel mean's bound / 16 plus 3 u of (|px| + r + 15) / 16;
  * conic: relative Frobenius error |dK|_F / lambda_min (an inverse perturbed by dK) + 3 u (k00 k11 + k01^2) / det (the determinant's
    own rounding in the published order) + 4 u;
  * SH colour: (19 + number of basis functions) u of sum_k |B_k c_k| + 0.5, |B_k| evaluated without cancellation (sh_basis_abs).

The oracle twin stays inside these bounds with a wide margin (test_projection_fp64 prints the largest error / bound ratio of each
quantity); they are first order, so the rule applies them with no further factor.

Rule (compare()):
  * Visibility: radius > 0 agrees, except at a PROVEN boundary: |tz - 0.2| within its bound, a rect whose area can be 0 or not within
    the bounds of its edges and radius, or a published determinant within its bound of 0.  Those are counted.
  * Radius: equal; +-1 only where 3 sqrt(lambda) lies within its bound of an integer (counted).
  * Rect: every edge equal to the fp64 rect recomputed with the PRODUCT's radius (so a radius that legitimately moved by one moves the
    rect with it); +-1 only where that edge's argument lies within its bound of an integer (counted).  tiles_touched = the rect's area.
  * Pixel mean and depth: within their bounds.  Conic: within its relative Frobenius bound; the maximum and 99.9th percentile of the
    relative Frobenius error are reported.  Opacity: the input (or within the bound of an activated input).
  * SH colour: |rgb - max(c + 0.5, 0)| within the bound (so a clamped 0 agrees with c + 0.5 <= 0 except within the bound).
  * The counted exceptions are printed and may not exceed EXCEPTION_FRAC of the visible Gaussians (+ EXCEPTION_SLACK).  Anything else
    fails the test.
"""
import numpy as np
import torch

from oracle.dense_torch import U32, project_dense, rect_from
from tests import util

EXCEPTION_FRAC = 1e-3       # boundary exceptions allowed, as a fraction of the visible Gaussians
EXCEPTION_SLACK = 2         # ... plus this many on any scene (a few-hundred-Gaussian scene may hold one boundary splat)


def _np(t):
    return None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))


def reference(rs, rv, **kw):
    """project_dense on the inputs of a rendervar dict (fp32 tensors, promoted), on the inputs' device."""
    g = rv.get
    return project_dense(util.cam_dict(rs), g("means3D"), g("opacities"), colors=g("colors_precomp"), shs=g("shs"), scales=g("scales"),
                         rotations=g("rotations"), cov3D_precomp=g("cov3D_precomp"), **kw)


def records_from_oracle(o):
    """oracle/gs_oracle.py preprocess()/forward() output -> the record dict compare() takes"""
    co = o["conic_opacity"]
    return dict(radii=o["radii"], xy=o["xy"], conic=co[:, :3], opacity=co[:, 3], rgb=o["rgb"], depth=o["depth"], rect=o["rect"],
                tiles_touched=o["tiles_touched"], cov2d=o["cov2d"])


def records_from_artefacts(art, radii):
    """util.artefacts() of a debug forward + its radii -> the record dict (geom: x, y, conic a b c, opacity, rgb, depth, extents)"""
    g = art["geom"]
    return dict(radii=np.asarray(radii), xy=g[:, 0:2], conic=g[:, 2:5], opacity=g[:, 5], rgb=g[:, 6:9], depth=g[:, 9], rect=art["rect"],
                tiles_touched=art["tiles_touched"])


def _tl(a, hi):
    return np.minimum(np.clip(np.trunc(np.clip(a, -1048576, 1048576)), 0, None), hi).astype(np.int64)


def conic_rel_frobenius(conic, ref_conic):
    a, b = np.asarray(conic, np.float64), np.asarray(ref_conic, np.float64)
    w = np.array([1.0, 2.0, 1.0])                      # the off-diagonal entry counts twice in the 2 x 2 matrix
    return np.sqrt(((a - b) ** 2 * w).sum(1) / (b ** 2 * w).sum(1))


def compare(got, ref, label, rgb="given", opacity="given", cap=True, verbose=True):
    """got: the product's per-Gaussian records (records_from_*), ref: project_dense(...).  rgb: "given" (colours passed through: equal),
    "sh" (the SH rule) or None (not compared); opacity: "given" (equal) or "bound" (ref['opacity_err']).  Returns the statistics."""
    R = {k: _np(v) for k, v in ref.items() if k not in ("W", "H")}
    W, H = ref["W"], ref["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    hi = np.array([gx, gy, gx, gy])
    rad = np.asarray(got["radii"]).astype(np.int64)
    gv, rvis = rad > 0, R["visible"]
    P = rad.shape[0]
    st = dict(label=label, P=P, visible=int(rvis.sum()), vis_exc=0, radius_exc=0, rect_exc=0, near=0, area=0, det=0)
    # ---- visibility ----
    v, ve = R["v"], R["v_err"]
    r_lo, r_hi = np.ceil(v - ve), np.ceil(v + ve)                  # every radius an fp32 evaluation can produce
    pix = torch.from_numpy(R["xy"]); pe = torch.from_numpy(R["xy_err"])
    _, a_lo, e_lo = (_np(t) for t in rect_from(pix, pe, torch.from_numpy(r_lo), W, H))
    _, a_hi, e_hi = (_np(t) for t in rect_from(pix, pe, torch.from_numpy(r_hi), W, H))
    lo_edge = np.concatenate([_tl(a_hi[:, :2] - e_hi[:, :2], hi[:2]), _tl(a_lo[:, 2:] - e_lo[:, 2:], hi[2:])], 1)   # smallest x0 y0 x1 y1
    hi_edge = np.concatenate([_tl(a_lo[:, :2] + e_lo[:, :2], hi[:2]), _tl(a_hi[:, 2:] + e_hi[:, 2:], hi[2:])], 1)   # largest
    area_min = np.clip(lo_edge[:, 2] - hi_edge[:, 0], 0, None) * np.clip(lo_edge[:, 3] - hi_edge[:, 1], 0, None)
    area_max = (hi_edge[:, 2] - lo_edge[:, 0]) * (hi_edge[:, 3] - lo_edge[:, 1])
    near_b = np.abs(R["near"]) <= R["depth_err"]
    det_b = R["det"] <= R["det_err"]
    area_b = (area_min <= 0) & (area_max > 0)
    bad = np.nonzero(gv != rvis)[0]
    for i in bad:
        if near_b[i]:
            st["near"] += 1
        elif R["near"][i] > 0 and det_b[i]:
            st["det"] += 1
        elif R["near"][i] > 0 and area_b[i]:
            st["area"] += 1
        else:
            raise AssertionError(f"{label}: Gaussian {i}: product radius {rad[i]}, fp64 visible={bool(rvis[i])} (tz-0.2={R['near'][i]:.3e} "
                                 f"+-{R['depth_err'][i]:.1e}, det={R['det'][i]:.3e} +-{R['det_err'][i]:.1e}, area in [{area_min[i]}, "
                                 f"{area_max[i]}], 3sqrt(lam)={v[i]:.6f} +-{ve[i]:.1e})")
    st["vis_exc"] = len(bad)
    both = gv & rvis
    ix = np.nonzero(both)[0]
    # ---- radius ----
    d = rad[ix] - R["rf"][ix]
    ok = (d == 0) | ((np.abs(d) == 1) & (rad[ix] >= r_lo[ix]) & (rad[ix] <= r_hi[ix]))
    if not ok.all():
        j = ix[~ok][0]
        raise AssertionError(f"{label}: {int((~ok).sum())} radii off, e.g. Gaussian {j}: {rad[j]} vs fp64 {R['rf'][j]} "
                             f"(3sqrt(lam)={v[j]:.7f} +-{ve[j]:.2e})")
    st["radius_exc"] = int((d != 0).sum())
    # ---- rect, against the fp64 rect recomputed with the product's radius ----
    rect_p, args_p, err_p = (_np(t) for t in rect_from(pix[ix], pe[ix], torch.from_numpy(rad[ix]), W, H))
    grect = np.asarray(got["rect"])[ix].astype(np.int64)
    dr = grect - rect_p
    allowed = (grect >= _tl(args_p - err_p, hi)) & (grect <= _tl(args_p + err_p, hi)) & (np.abs(dr) <= 1)
    ok = (dr == 0) | allowed
    if not ok.all():
        k = np.nonzero(~ok.all(1))[0][0]
        j = ix[k]
        raise AssertionError(f"{label}: {int((~ok.all(1)).sum())} rects off, e.g. Gaussian {j}: {grect[k].tolist()} vs fp64 {rect_p[k].tolist()} "
                             f"(arguments {args_p[k].tolist()} +-{err_p[k].max():.1e}, radius {rad[j]})")
    st["rect_exc"] = int((dr != 0).any(1).sum())
    tt = np.asarray(got["tiles_touched"]).astype(np.int64)
    assert (tt[~gv] == 0).all(), label
    assert np.array_equal(tt[ix], (grect[:, 2] - grect[:, 0]) * (grect[:, 3] - grect[:, 1])), label
    # ---- pixel mean, depth ----
    for k, ek in (("xy", "xy_err"), ("depth", "depth_err")):
        a = np.asarray(got[k])[ix].astype(np.float64)
        e = np.abs(a - R[k][ix]) / R[ek][ix]
        st[f"{k}_ratio"] = float(e.max()) if e.size else 0.0
        assert st[f"{k}_ratio"] <= 1.0, (label, k, st[f"{k}_ratio"], ix[np.unravel_index(np.argmax(e), e.shape)[0]])
    # ---- the 2-D covariance entries, where the product reports them (the oracle): the bound lambda's is built from ----
    if "cov2d" in got:
        e = np.abs(np.asarray(got["cov2d"])[ix].astype(np.float64) - R["cov2d"][ix]) / R["cov2d_err"][ix]
        st["cov2d_ratio"] = float(e.max()) if e.size else 0.0
        assert st["cov2d_ratio"] <= 1.0, (label, "cov2d", st["cov2d_ratio"])
    # ---- conic ----
    rel = conic_rel_frobenius(np.asarray(got["conic"])[ix], R["conic"][ix])
    ratio = rel / R["conic_bound"][ix]
    st.update(conic_max=float(rel.max()) if rel.size else 0.0, conic_p999=float(np.percentile(rel, 99.9)) if rel.size else 0.0,
              conic_ratio=float(ratio.max()) if rel.size else 0.0)
    if rel.size and ratio.max() > 1.0:
        j = ix[np.argmax(ratio)]
        raise AssertionError(f"{label}: conic of Gaussian {j} off by {rel.max():.3e} relative (bound {R['conic_bound'][j]:.3e}): "
                             f"{np.asarray(got['conic'])[j].tolist()} vs fp64 {R['conic'][j].tolist()}")
    # ---- opacity ----
    o = np.asarray(got["opacity"])[ix].astype(np.float64)
    if opacity == "given":
        assert np.array_equal(o, R["opacity"][ix]), label
    else:
        e = np.abs(o - R["opacity"][ix]) / R["opacity_err"][ix]
        st["opacity_ratio"] = float(e.max()) if e.size else 0.0
        assert st["opacity_ratio"] <= 1.0, (label, "opacity", st["opacity_ratio"])
    # ---- colour ----
    if rgb == "given":
        assert np.array_equal(np.asarray(got["rgb"])[ix].astype(np.float64), R["rgb"][ix]), label
    elif rgb == "sh":
        c = np.asarray(got["rgb"])[ix].astype(np.float64)
        err = np.abs(c - np.maximum(R["rgb_pre"][ix], 0.0))
        ratio = err / R["rgb_err"][ix]
        st["rgb_ratio"] = float(ratio.max()) if ratio.size else 0.0
        st["rgb_p999"] = float(np.percentile(ratio, 99.9)) if ratio.size else 0.0
        if ratio.size and ratio.max() > 1.0:
            k = np.unravel_index(np.argmax(ratio), ratio.shape)
            j = ix[k[0]]
            raise AssertionError(f"{label}: SH colour of Gaussian {j} channel {k[1]}: {c[k]:.8f} vs fp64 max({R['rgb_pre'][j, k[1]]:.8f}, 0) "
                                 f"(bound {R['rgb_err'][j, k[1]]:.2e})")
        zero = c == 0.0
        assert (R["rgb_pre"][ix][zero] <= R["rgb_err"][ix][zero]).all(), label
    n_exc = st["vis_exc"] + st["radius_exc"] + st["rect_exc"]
    st["exceptions"] = n_exc
    st["cap"] = int(EXCEPTION_FRAC * st["visible"]) + EXCEPTION_SLACK
    if verbose:
        print(f"[projection_fp64] {label}: P={P} visible={st['visible']} boundary exceptions: visibility {st['vis_exc']} (near {st['near']}, "
              f"area {st['area']}, det {st['det']}), radius {st['radius_exc']}, rect {st['rect_exc']} (cap {st['cap']}); conic rel. Frobenius "
              f"max {st['conic_max']:.2e} p99.9 {st['conic_p999']:.2e} (largest error/bound {st['conic_ratio']:.3f}); xy error/bound "
              f"{st['xy_ratio']:.3f}, depth {st['depth_ratio']:.3f}" + (f", cov2D entries {st['cov2d_ratio']:.3f}" if "cov2d_ratio" in st else "")
              + (f"; SH colour error/bound max {st['rgb_ratio']:.3f} p99.9 {st['rgb_p999']:.3f}"
                 if rgb == "sh" else ""))
    if cap:
        assert n_exc <= st["cap"], (label, st)
    return st


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def _rv(means, scales, seed, device, sh_degree=None):
    g = torch.Generator().manual_seed(seed)
    N = means.shape[0]
    rv = dict(means3D=means.float(), scales=scales.float(), rotations=torch.nn.functional.normalize(torch.randn(N, 4, generator=g)),
              opacities=torch.sigmoid(torch.randn(N, 1, generator=g) + 1.0))
    if sh_degree is None:
        rv["colors_precomp"] = torch.rand(N, 3, generator=g)
    else:
        rv["shs"] = 0.3 * torch.randn(N, 16, 3, generator=g)
    return {k: v.to(device).contiguous() for k, v in rv.items()}


def offscreen_scene(N, device, W=128, H=96, seed=5, sh_degree=None):
    """Splats whose mean lies outside the +-1.3 tan(fov) cone (the EWA clamp is active), in x, in y or in both, whose footprint still
    reaches the image; a third of them between 1.3 tanfovy and 1.3 tanfovx vertically (tanfovx = 1, tanfovy = 0.75), where a clamp
    limit taken from the wrong axis would differ."""
    rs, _ = util.scene(1, W, H, device=device, sh_degree=sh_degree)
    g = torch.Generator().manual_seed(seed)
    z = 0.5 + 3.0 * torch.rand(N, generator=g)
    k = torch.randint(0, 3, (N,), generator=g)
    sgn = lambda: torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
    rx = torch.where(k == 0, sgn() * (1.32 + 0.6 * torch.rand(N, generator=g)), (torch.rand(N, generator=g) - 0.5) * 1.6)
    ry = torch.where(k == 1, sgn() * (0.99 + 0.29 * torch.rand(N, generator=g)),
                     torch.where(k == 2, sgn() * (1.0 + 0.6 * torch.rand(N, generator=g)), (torch.rand(N, generator=g) - 0.5) * 1.2))
    rx = torch.where(k == 2, sgn() * (1.32 + 0.4 * torch.rand(N, generator=g)), rx)
    means = torch.stack([rx * z, ry * z, z], 1)
    s = z[:, None] * torch.exp(torch.log(torch.tensor(0.25)) + 0.8 * torch.randn(N, 3, generator=g))
    return rs, _rv(means, s, seed, device, sh_degree)


def near_plane_scene(N, device, W=128, H=96, seed=6):
    """Splats at view depths 0.19 .. 0.25 (the near cull at 0.2, J = f / tz at its largest): ordinary and strongly anisotropic shapes."""
    rs, _ = util.scene(1, W, H, device=device)
    g = torch.Generator().manual_seed(seed)
    z = 0.19 + 0.06 * torch.rand(N, generator=g)
    means = torch.stack([(torch.rand(N, generator=g) - 0.5) * 1.6 * z, (torch.rand(N, generator=g) - 0.5) * 1.2 * z, z], 1)
    s = 0.002 * torch.exp(1.2 * torch.randn(N, 3, generator=g))
    return rs, _rv(means, s, seed, device)


def needle_scene(N, device, W=128, H=96, seed=7, near=True, sh_degree=None):
    """Needles: one axis 100 .. 5000 times the other two (anisotropy above 2 000 for a third of them), randomly oriented; near=True puts
    them at view depths 0.21 .. 0.6, right in front of the near plane (radii of thousands of pixels), else 0.5 .. 4."""
    rs, _ = util.scene(1, W, H, device=device, sh_degree=sh_degree)
    g = torch.Generator().manual_seed(seed)
    z = (0.21 + 0.39 * torch.rand(N, generator=g)) if near else (0.5 + 3.5 * torch.rand(N, generator=g))
    means = torch.stack([(torch.rand(N, generator=g) - 0.5) * 2.0 * z, (torch.rand(N, generator=g) - 0.5) * 1.5 * z, z], 1)
    s = (z / 64.0)[:, None] * torch.exp(0.3 * torch.randn(N, 3, generator=g)) * 0.3
    ax = torch.randint(0, 3, (N,), generator=g)
    s[torch.arange(N), ax] *= torch.exp(torch.log(torch.tensor(100.0)) + torch.rand(N, generator=g) * float(np.log(50.0)))
    return rs, _rv(means, s, seed, device, sh_degree)


def hard_sweep(seeds, device):
    """fuzz_scenes.hard_scene at s = 1.2 for the given seeds"""
    from tests import fuzz_scenes
    return [(f"hard_{s}", *fuzz_scenes.hard_scene(s, device, 1.2)) for s in seeds]
