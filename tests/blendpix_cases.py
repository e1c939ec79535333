"""The blend kernels (csrc/blend.hip) PIXEL BY PIXEL and ROW BY ROW at their rare branches, shared by the host-emulated kernel tests
(tests/test_blendpix.py) and the device tests (tests/test_gpu_blendpix.py).

parity_cases.check_forward lets 0.1 % of an image's values miss the tolerance and check_backward judges a whole gradient tensor; the scenes of
rowgrad_cases keep the blend out of their rows on purpose.  A mistake in a blend branch -- the alpha = 0.99 clamp (the gradient passes through,
T takes the clamped value), a walk that stops at T (1 - alpha) < 1e-4 and leaves entries behind, the rim of a footprint near alpha = 1/255,
the T x background term, a backward walker that resumes from a state the forward recorded, a chained piece -- is confined to the pixels and
rows that take the branch.  The scenes here make such a class a large share of the image (asserted from the replay), and every pixel and
every rendered row is judged on its own.

THE REPLAY (replay()) is the tests' own plain reference of the operation: an fp64 numpy evaluation of the forward and backward blend, tile
by tile and vectorised over the tile's pixels, from an oracle's per-Gaussian record (xy, conic_opacity, rgb, depth) and its sorted tile lists
(ranges, ids_sorted), over the N = 6 channels [r, g, b, z, 1, z^2] with background [bg, 0, 0, 0].  It yields every pixel's outputs with their
absolute sums A_p = sum |c w| + T |bg|, final T, n_contrib, stop position and classes, and for every Gaussian the net and the ABSOLUTE sum S
(sum over pixels of |term|) of its contributions to dL/dopacity, dL/dfeature, dL/dxy, dL/dconic and dL/dz.  test_blendpix holds the replay to
the fp64 oracle (forward equal, net sums within 1e-10 S).  A row's own magnitude is the wrong scale for its error: a row is a sum over
50 .. 600 pixels of signed terms and about 1 % of the rows cancel to below 1 % of their terms; S is what the rounding of the sum scales with.

RULES.  No pixel and no row is excused and there is no second tier.

  forward, every value of colour, depth, opacity, depth^2 and final T:   |o_k - o_64| <= min(2 |o_32 - o_64| + FLOOR_F A_p, CAP_p A_p)
  n_contrib equal at every pixel; a pixel nothing contributes to is exactly bg, 0, 0, 0 and T = 1
  backward, every rendered row i and component:                          |g_k - g_64| <= min(2 |g_32 - g_64| + FLOOR_B s_i, CAP_i s_i)
  rows of Gaussians that were not rendered are exactly zero

o_64 / g_64: the fp64 oracle; o_32 / g_32: the fp32 oracle (never the kernel).  s_i = the largest S over the row's components for
colors_precomp, opacities and means2D (in the binding's units: dL/dxy x (W / 2, H / 2)); for cov3D_precomp s_i = ||g_64[i]||_inf kappa_i with
kappa_i = max_c S_conic / max_c |dconic_64| >= 1.  means3D, scales and rotations of the same scenes go through the unchanged
parity_cases.check_backward.  FLOOR = 2 x the fp32 oracle's own largest error in these units over every pass/fail scene, entry and tensor
(MEASURED_*; test_blendpix.test_fp32_oracle_alone_sets_floors re-measures it on every run), rounded up to one significant digit;
CAP = 10 FLOOR + n 2^-24, n the number of contributing pairs of the pixel / contributing pixels of the row (the worst case of adding n fp32
terms in any order, which is what the device's atomics do), never above the project's 1e-3.

SETTLING (deterministic, from both oracles' records): a Gaussian that owns a pixel with alpha within 1e-4 (relative) of 1/255, or a visible
step with T (1 - alpha) within 1e-3 (relative) of 1e-4, is dimmed by 3 % until none is left; the two oracles must then agree on n_contrib at
every pixel.  (Two clamped entries in a row give 0.01 x 0.01, the stop threshold itself: the clamp scene holds one clamped splat per tile.)

profiles/README.md, "Blend, pixel by pixel",
holds the measured floors and the margins on the device."""
import ctypes as C
import math

import numpy as np
import torch

from activesplat_amd import _lib
from activesplat_amd import rasterizer as R
from tests import output_grad_cases as og
from tests import parity_cases as pc
from tests import rowgrad_cases as rg
from tests import util

ALPHA_MIN = 1.0 / 255.0
T_MIN = 1e-4
#: the fp32 oracle's largest error against the fp64 oracle over every pass/fail scene, entry and output / tensor, in the rule's units
#: (|o_32 - o_64| / A_p and |g_32 - g_64| / s_i); CPU, the oracles alone -- test_fp32_oracle_alone_sets_floors prints the current values
#: and holds them to these records within 10 % (another libm moves them by less; a generator change by more)
MEASURED_ORACLE32_PIXEL_ERROR = 5.77e-5       # many/stop, colour, a rim pixel
MEASURED_ORACLE32_ROW_ERROR = 2.62e-4         # many/stop, cov3D_precomp, a row of 6 pixels deep in walks that stop
#: 2 x MEASURED, rounded up to one significant digit
FLOOR_F = 2e-4
FLOOR_B = 6e-4
CAP_MAX = 1e-3                       # the project's bar
ALPHA_WINDOW = 1e-4                  # no pixel has alpha within this (relative) of 1/255 ...
STOP_WINDOW = 1e-3                   # ... and no visible step has T (1 - alpha) within this (relative) of 1e-4

OUTPUTS = ("color", "depth", "opacity", "depth_sq", "final_T")
#: GaussianRasterizer (colour) / render_rgbd (colour + depth) / depth + silhouette (OUT = 1: keeps the list segments) / all four (OUT = 2: one walker)
ENTRIES = ("color", "rgbd", "dos", "all")
EVERYTHING = ("depth", "silhouette", "depth_sq")


def cap_of(floor, n):
    return np.minimum(10.0 * floor + np.asarray(n, np.float64) * 2.0 ** -24, CAP_MAX)


# ---- the replay ----------------------------------------------------------------------------------------------------------------------------
class Replay:
    """What replay() returns.  Images are [., H, W]; per-Gaussian arrays are [P, .]; pairs are counted, not stored."""


def _tile_pixels(t, gx, W, H):
    x0, y0 = 16 * (t % gx), 16 * (t // gx)
    xs, ys = np.arange(x0, min(x0 + 16, W)), np.arange(y0, min(y0 + 16, H))
    px, py = np.meshgrid(xs, ys)
    return px.reshape(-1), py.reshape(-1)


def replay(rec, W, H, bg, dL=None, cuts=None, widen=1.0):
    """rec: an oracle's forward (its record and tile lists).  bg [3].  dL: None (forward and classes only) or dict(color [3, H, W], depth,
    opacity, depth_sq [1, H, W] or None).  cuts: None or a function (wmax) -> list position of the first recorded cut of a quadrant whose
    deepest contributor is wmax (0: none) -- classifies the pairs past it.  widen: factor on the two threshold windows (settling).  All arithmetic in fp64, in the oracle's order of operations."""
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    xy, co, rgb, z = f8(rec["xy"]), f8(rec["conic_opacity"]), f8(rec["rgb"]), f8(rec["depth"])
    ranges, ids_all = np.asarray(rec["ranges"]).astype(np.int64), np.asarray(rec["ids_sorted"]).astype(np.int64)
    radii = np.asarray(rec["radii"])
    P = xy.shape[0]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    feat = np.concatenate([rgb, z[:, None], np.ones((P, 1)), (z * z)[:, None]], 1)                      # [P, 6]
    bg6 = np.concatenate([f8(bg).reshape(3), np.zeros(3)])
    out = Replay()
    out.W, out.H, out.P = W, H, P
    out.img = np.zeros((6, H, W)); out.A = np.zeros((6, H, W))
    out.final_T = np.ones((H, W)); out.n_contrib = np.zeros((H, W), np.int64); out.n_pairs = np.zeros((H, W), np.int64)
    out.stop_pos = np.full((H, W), -1, np.int64)             # list position (0-based) of the entry the pixel stopped AT, -1: it never stopped
    out.behind_stop = np.zeros((H, W), np.int64)             # entries of the list behind that position
    out.list_len = np.zeros((H, W), np.int64)
    out.clamped_px = np.zeros((H, W), bool); out.rim_px = np.zeros((H, W), bool); out.past_cut_px = np.zeros((H, W), bool)
    out.T_at_cut = np.full((H, W), np.nan)
    out.stopped_before_cut = np.zeros((H, W), bool)
    out.pairs = dict(contributing=0, clamped=0, rim=0, box=0, box_skipped=0, past_cut=0)
    out.alpha_margin = []                                    # (gaussian, x, y, 255 alpha - 1) inside ALPHA_WINDOW
    out.stop_margin = []                                     # (gaussian, x, y, T (1 - alpha) / 1e-4 - 1) inside STOP_WINDOW
    out.rows = dict(pixels=np.zeros(P, np.int64), clamped=np.zeros(P, np.int64), rim=np.zeros(P, np.int64), stopped=np.zeros(P, np.int64),
                    background=np.zeros(P, np.int64), past_cut=np.zeros(P, np.int64))
    back = dL is not None
    if back:
        zero = np.zeros((1, H, W))
        d6 = np.concatenate([f8(dL["color"]).reshape(3, H, W)] + [zero if dL.get(k) is None else f8(dL[k]).reshape(1, H, W) for k in ("depth", "opacity", "depth_sq")], 0)
        names = dict(dop=1, dfeat=6, dxy=2, dconic=3)
        out.net = {k: np.zeros((P, n)) for k, n in names.items()}
        out.S = {k: np.zeros((P, n)) for k, n in names.items()}
    for t in range(gx * gy):
        s, e = ranges[t]
        px, py = _tile_pixels(t, gx, W, H)
        n = int(e - s)
        out.list_len[py, px] = n
        if n == 0:
            out.img[:, py, px] = bg6[:, None]; out.A[:, py, px] = np.abs(bg6)[:, None]
            continue
        ids = ids_all[s:e]
        dx, dy = xy[ids, 0][:, None] - px[None, :], xy[ids, 1][:, None] - py[None, :]
        a_, b_, c_, op = (co[ids, k][:, None] for k in range(4))
        power = -0.5 * (a_ * dx * dx + c_ * dy * dy) - b_ * dx * dy
        G = np.exp(np.minimum(power, 0.0))
        raw = op * G
        alpha = np.minimum(0.99, raw)
        hit = (power <= 0) & (alpha >= ALPHA_MIN)
        near = (power <= 0) & (np.abs(255.0 * alpha - 1.0) < widen * ALPHA_WINDOW)
        T_after = np.cumprod(np.where(hit, 1.0 - alpha, 1.0), 0)
        T_before = np.concatenate([np.ones((1, px.size)), T_after[:-1]], 0)
        stops = hit & (T_after < T_MIN)
        stopped = stops.any(0)
        pos = np.where(stopped, stops.argmax(0), n)
        k_ = np.arange(n)[:, None]
        ok = hit & (k_ < pos[None, :])
        seen = hit & (k_ <= pos[None, :])                     # the visible steps, the stopping one included
        edge = seen & (np.abs(T_after / T_MIN - 1.0) < widen * STOP_WINDOW)
        for arr, sink in ((near & (k_ <= pos[None, :]), out.alpha_margin), (edge, out.stop_margin)):
            for j, p in zip(*np.nonzero(arr)):
                sink.append((int(ids[j]), int(px[p]), int(py[p]), float(255.0 * alpha[j, p] - 1.0 if sink is out.alpha_margin else T_after[j, p] / T_MIN - 1.0)))
        w = np.where(ok, alpha * T_before, 0.0)
        Tf = np.where(stopped, T_before[np.minimum(pos, n - 1), np.arange(px.size)], T_after[-1])
        last = np.where(ok.any(0), n - ok[::-1].argmax(0), 0)
        fw = feat[ids]                                        # [n, 6]
        out.img[:, py, px] = fw.T @ w + bg6[:, None] * Tf[None, :]
        out.A[:, py, px] = np.abs(fw).T @ w + np.abs(bg6)[:, None] * Tf[None, :]
        out.final_T[py, px], out.n_contrib[py, px], out.n_pairs[py, px] = Tf, last, ok.sum(0)
        out.stop_pos[py, px] = np.where(stopped, pos, -1)
        out.behind_stop[py, px] = np.where(stopped, n - 1 - pos, 0)
        clamped, rim = ok & (raw > 0.99), ok & (alpha < 1.5 * ALPHA_MIN)
        out.clamped_px[py, px], out.rim_px[py, px] = clamped.any(0), rim.any(0)
        # box candidates: the pairs of a pixel inside the splat's square of `radius` pixels (what the binning lists the splat for); skipped: no hit
        rad = radii[ids].astype(np.float64)[:, None]
        box = (np.abs(dx) <= rad) & (np.abs(dy) <= rad) & (k_ <= pos[None, :])
        past = np.zeros_like(ok)
        if cuts is not None:
            qid = (py % 16 // 8) * 2 + (px % 16 // 8)
            for q in range(4):
                m = qid == q
                if not m.any() or last[m].max() == 0:
                    continue
                cut = int(cuts(int(last[m].max())))
                if cut <= 0 or cut >= last[m].max():
                    continue
                past[:, m] = ok[:, m] & (k_ >= cut)
                cols = np.nonzero(m)[0]
                res = last[cols] > cut                         # the pixel contributes past the cut: the front walker resumes it from the recorded state
                out.past_cut_px[py[cols], px[cols]] = res
                out.T_at_cut[py[cols[res]], px[cols[res]]] = T_before[cut, cols[res]]
                out.stopped_before_cut[py[cols], px[cols]] = stopped[cols] & (pos[cols] < cut)
        P_ = out.pairs
        P_["contributing"] += int(ok.sum()); P_["clamped"] += int(clamped.sum()); P_["rim"] += int(rim.sum()); P_["past_cut"] += int(past.sum())
        P_["box"] += int(box.sum()); P_["box_skipped"] += int((box & ~hit).sum())
        bgw = (Tf > 0.2) & (Tf < 0.9) & (np.abs(bg6).max() > 0)
        rw = out.rows
        rw["pixels"][ids] += ok.sum(1); rw["clamped"][ids] += clamped.sum(1); rw["rim"][ids] += rim.sum(1)
        rw["stopped"][ids] += (ok & stopped[None, :]).sum(1); rw["background"][ids] += (ok & bgw[None, :]).sum(1); rw["past_cut"][ids] += past.sum(1)
        if not back:
            continue
        dpx = d6[:, py, px]                                   # [6, m]
        cdot = fw @ dpx                                       # [n, m]: c_j . dL
        wc = w * cdot
        behind = np.cumsum(wc[::-1], 0)[::-1] - wc + (Tf * (bg6 @ dpx))[None, :]          # sum_{k > j} w_k c_k . dL + T_final bg . dL
        one_m = np.where(ok, 1.0 - alpha, 1.0)
        dalpha = np.where(ok, T_before * cdot - behind / one_m, 0.0)
        dG = op * dalpha
        gdx, gdy = G * dx, G * dy
        terms = dict(dop=[G * dalpha], dxy=[dG * (-gdx * a_ - gdy * b_), dG * (-gdy * c_ - gdx * b_)],
                     dconic=[-0.5 * gdx * dx * dG, -gdx * dy * dG, -0.5 * gdy * dy * dG], dfeat=[w * dpx[ch][None, :] for ch in range(6)])
        for k, comps in terms.items():
            for c, v in enumerate(comps):
                v = np.where(ok, v, 0.0)
                out.net[k][ids, c] += v.sum(1)
                out.S[k][ids, c] += np.abs(v).sum(1)
    out.touched = out.n_contrib > 0
    if back:
        # dL/dz: z is channel 3's colour and z^2 channel 5's
        out.net["dz"] = (out.net["dfeat"][:, 3] + 2.0 * z * out.net["dfeat"][:, 5])[:, None]
        out.S["dz"] = (out.S["dfeat"][:, 3] + 2.0 * np.abs(z) * out.S["dfeat"][:, 5])[:, None]
    return out


def pixel_classes(rp, x, y):
    """-> the classes of one pixel, for a failure message"""
    c = []
    if not rp.touched[y, x]:
        c.append("untouched")
    if rp.clamped_px[y, x]:
        c.append("clamped")
    if rp.stop_pos[y, x] >= 0:
        c.append(f"stopped at list position {int(rp.stop_pos[y, x])} ({int(rp.behind_stop[y, x])} entries behind)")
    if rp.rim_px[y, x]:
        c.append("rim")
    if rp.touched[y, x] and 0.2 < rp.final_T[y, x] < 0.9:
        c.append("background-weighted")
    if rp.past_cut_px[y, x]:
        c.append("past-the-cut")
    return ", ".join(c) if c else "plain"


def row_classes(rp, i):
    """-> the classes of one Gaussian's contributing pairs with their shares, for a failure message"""
    n = max(int(rp.rows["pixels"][i]), 1)
    c = [f"{k} {100.0 * rp.rows[k][i] / n:.0f} %" for k in ("clamped", "stopped", "rim", "background", "past_cut") if rp.rows[k][i]]
    return (", ".join(c) if c else "plain") + f" of {int(rp.rows['pixels'][i])} pixels"


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, name, W, H, bg, rv, report_only=False):
        self.name, self.W, self.H, self.rv, self.report_only = name, W, H, rv, report_only
        self.bg = tuple(float(np.float32(b)) for b in bg)                   # (the settings hold it in fp32)
        self.P = int(rv["means3D"].shape[0])
        self.rs = util.scene(1, W, H, device="cpu", bg=bg)[0]._replace(debug=False)
        self.meta = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *s):
    return torch.rand(*s, generator=g, dtype=torch.float64)


def _splats(g, W, H, u, v, z, sigma, op):
    """Isotropic splats of `sigma` pixels centred on the pixels (u, v) at depth z (the camera of util.scene: fx = fy = W / 2; a camera-frame point (x, y, z) lands on the pixel
    (fx x / z + W / 2 - 1.5, fy y / z + H / 2 - 1.5))"""
    u, v, z, sigma, op = (torch.as_tensor(a, dtype=torch.float64) for a in (u, v, z, sigma, op))
    n = u.shape[0]
    fx, cx, cy = W / 2.0, W / 2.0 - 1.5, H / 2.0 - 1.5
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fx * z, z], 1)
    # flat discs facing the camera, turned about the view axis: off the optical axis a sphere's footprint is stretched by the perspective, a disc's
    # is not, and the footprint is `sigma` pixels (plus the 0.3 low-pass) everywhere in the image
    half = math.pi * _rand(g, n)
    rot = torch.stack([torch.cos(half), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.sin(half)], 1)
    s = sigma * z / fx
    return dict(means3D=means, scales=torch.stack([s, s * (0.9 + 0.1 * _rand(g, n)), 1e-3 * s], 1), rotations=rot, opacities=op[:, None].clone(), colors_precomp=_rand(g, n, 3))


def _depths(g, n, lo, hi):
    """n distinct depths on an even grid in (lo, hi), shuffled: both oracles and the kernels sort by the fp32 depth, and two depths an ulp apart
    may sort differently in the fp64 oracle's record"""
    return lo + (hi - lo) * (torch.randperm(n, generator=g).double() + 0.5) / n


def _cat(parts, g):
    rv = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    zs = rv["means3D"][:, 2].float().double().sort().values
    assert float((zs[1:] - zs[:-1]).min()) > 2e-6, "two splats at (nearly) one depth"
    perm = torch.randperm(rv["means3D"].shape[0], generator=g)
    return {k: v[perm].float().contiguous() for k, v in rv.items()}


def _field(g, W, H, box, n, sigma, op, z=(1.0, 4.0)):
    """n splats with centres uniform in the pixel box (x0, y0, x1, y1); sigma, op: (lo, hi) or a function of the centre (u, v)"""
    x0, y0, x1, y1 = box
    u, v = x0 + (x1 - x0) * _rand(g, n), y0 + (y1 - y0) * _rand(g, n)
    pick = lambda a: a(u, v) if callable(a) else a[0] + (a[1] - a[0]) * _rand(g, n)  # noqa: E731
    return _splats(g, W, H, u, v, _depths(g, n, z[0], z[1]), pick(sigma), pick(op))


def _clamp_parts(g, W, H, tiles):
    """One splat of 2 .. 2.2 px per tile, centred on the tile's pixel (8, 8): its square of 3 sigma stays inside the tile, so no pixel sees two
    clamped entries in a row (0.01 x 0.01 is the stop threshold itself).  raw alpha = opacity x G exceeds 0.99 out to r = sigma sqrt(2 ln(opacity
    / 0.99)), and a footprint reaches alpha = 1/255 at r^2 larger by 11.06 sigma^2 whatever the opacity: for the clamped pairs to be the MAJORITY
    of a footprint the opacity has to be far above 1 (the drop-in entry points take any opacity; at opacity <= 1 only r < 0.1 sigma is clamped).
    Seven tiles in eight hold an opacity of 1000 .. 4000, every eighth one of 0.995 .. 1.  Behind them (T = 0.01: the clamped value) lie
    a few ordinary splats of 2 .. 3 px."""
    gx = (W + 15) // 16
    t = torch.as_tensor(tiles)
    n = t.shape[0]
    op = torch.where(torch.arange(n) % 8 == 7, 0.995 + 0.005 * _rand(g, n), torch.exp(math.log(1000.0) + math.log(4.0) * _rand(g, n)))
    front = _splats(g, W, H, 16.0 * (t % gx) + 8.0, 16.0 * (t // gx) + 8.0, _depths(g, n, 1.0, 2.0), 2.0 + 0.2 * _rand(g, n), op)
    x0, y0 = 16.0 * float((t % gx).min()), 16.0 * float((t // gx).min())
    x1, y1 = 16.0 * float((t % gx).max()) + 16.0, 16.0 * float((t // gx).max()) + 16.0
    return [front, _field(g, W, H, (x0, y0, x1, y1), n // 4, (2.0, 3.0), (0.1, 0.5), z=(3.0, 4.0))]


def _stop_parts(g, W, H, box, hole_tile):
    """A field of 2.2 .. 3.2 px splats of opacity 0.9 .. 0.99 over `box` whose density rises from 0.12 per pixel on the left to 0.24 on the right
    (tile lists of ~100 .. 250 entries): a walk stops a little past the middle of its list, between list positions ~50 and ~150, and leaves the
    rest behind.  (Opaque and small: a walk's steps in log T are large and a splat is seen by few stopped pixels, so that dimming a splat to move one
    step out of the window around T = 1e-4 moves fewer than one other in -- with 4 .. 6 px splats the settling does not end.)  In `hole_tile` (outside the field) one
    quadrant holds a stack of four 0.2 px splats (0.58 px with the low-pass) of opacity 0.95 .. 0.99 on every pixel but one: 63 pixels stop, the
    64th sees only tails and never does.  (The tile in the image's top left corner: alpha of so small and opaque a splat moves by 4e-5 (1 - alpha)
    with the fp32 rounding of a centre near x = 150, sixteen times less near x = 10.)"""
    x0, y0, x1, y1 = box
    n = int(0.165 * (x1 - x0) * (y1 - y0))
    u = x0 + (x1 - x0) * (torch.sqrt(1.0 + 3.0 * _rand(g, n)) - 1.0)
    field = _splats(g, W, H, u, y0 + (y1 - y0) * _rand(g, n), _depths(g, n, 1.0, 4.0), 2.2 + _rand(g, n), 0.9 + 0.09 * _rand(g, n))
    gx = (W + 15) // 16
    qx, qy = 16 * (hole_tile % gx) + 8, 16 * (hole_tile // gx)              # quadrant 1 of the tile: pixels (8 .. 15, 0 .. 7)
    pts = [(qx + i, qy + j) for j in range(8) for i in range(8) if (i, j) != (3, 4)]
    # (0.15, 0.1) px off the pixel centres: dL/dxy of a splat is proportional to its offset from the pixel, and a splat that contributes to the
    # one pixel it sits on would hold nothing but the fp32 rounding of its own centre
    u = torch.tensor([p[0] for p in pts] * 4, dtype=torch.float64) + 0.15
    v = torch.tensor([p[1] for p in pts] * 4, dtype=torch.float64) + 0.1
    stack = _splats(g, W, H, u, v, _depths(g, u.shape[0], 0.5, 0.9), torch.full_like(u, 0.2), 0.95 + 0.04 * _rand(g, u.shape[0]))
    return [field, stack], (qx + 3, qy + 4)


def _background_parts(g, W, H, box):
    """Faint 2 .. 4 px splats, about four to a pixel: most touched pixels end at 0.2 < T < 0.9 and the T x background term carries a large part
    of the colour; the tiles outside `box` stay untouched."""
    x0, y0, x1, y1 = box
    n = int(0.06 * (x1 - x0) * (y1 - y0))
    return [_field(g, W, H, box, n, (2.0, 4.0), (0.05, 0.35))]


def _grid_field(g, W, H, box, rho, sigma, op, z):
    """rho splats per pixel on a jittered grid over `box` (far less pixel-to-pixel spread of the optical depth than uniform random centres)"""
    x0, y0, x1, y1 = box
    step = 1.0 / math.sqrt(rho)
    nx, ny = int((x1 - x0) / step), int((y1 - y0) / step)
    i = torch.arange(nx * ny)
    n = nx * ny
    u = x0 + ((i % nx).double() + 0.2 + 0.6 * _rand(g, n)) * step
    v = y0 + ((i // nx).double() + 0.2 + 0.6 * _rand(g, n)) * step
    return _splats(g, W, H, u, v, _depths(g, n, z[0], z[1]), sigma[0] + (sigma[1] - sigma[0]) * _rand(g, n), op[0] + (op[1] - op[0]) * _rand(g, n))


def _resumed_parts(g, W, H, x0, y0):
    """A block of 4 x 2 tiles at (x0, y0), front to back: a sheet of 4 px splats of opacity 0.3, ~70 to a tile list (T = 0.33); two 0.2 px
    splats (0.58 px with the low-pass) of opacity 1.2 on every pixel of four pixel rows, (0.15, 0.1) px off the pixel -- alpha is clamped
    there, 0.33 x 0.01 x 0.01 stops those 256 pixels inside the first 230 list positions, and their neighbour rows see a quarter of it --; a
    field of 4 px splats of opacity 0.047, 0.25 to the pixel (another 1.2 nats: final T ~ 0.1).  Tile lists of 450 .. 700 entries that
    contribute to their end: the first cut of a quadrant's walk is list position 256, where T is 0.05 .. 0.4, and the front walkers of the
    few-tile backward resume every other pixel from the state recorded there."""
    box = (x0 - 13.0, y0 - 13.0, x0 + 64.0 + 13.0, y0 + 32.0 + 13.0)
    sheet = _grid_field(g, W, H, box, 0.04, (3.9, 4.1), (0.29, 0.31), z=(0.2, 0.45))
    field = _grid_field(g, W, H, box, 0.25, (3.9, 4.1), (0.044, 0.050), z=(1.5, 4.0))
    pts = [(x0 + i + 0.15, y0 + 6.0 + j + 0.1) for j in range(4) for i in range(64)] * 2
    u, v = (torch.tensor([p[k] for p in pts], dtype=torch.float64) for k in (0, 1))
    patch = _splats(g, W, H, u, v, _depths(g, u.shape[0], 0.5, 1.0), torch.full_like(u, 0.2), torch.full_like(u, 1.2))
    return [sheet, field, patch]


def _segmented_parts(g, W, H, x0, y0):
    """8300 splats of 0.5 px and opacity 0.03 in ONE tile: its list of more than 8192 entries makes gs_bin_layout cut list segments (the streams
    forward with SEG 1 / 2); a pixel sees a few hundred of them and ends at T ~ 0.04."""
    return [_field(g, W, H, (x0 + 1.0, y0 + 1.0, x0 + 15.0, y0 + 15.0), 8300, (0.5, 0.5), (0.028, 0.032))]


def _build(name):
    """-> Scene (before settling)"""
    fam, _, kind = name.partition("/")
    if fam == "few":
        W, H = 160, 128
        g = _gen(sum(map(ord, name)))
        if kind == "clamp":
            return Scene(name, W, H, (0.0, 0.0, 0.0), _cat(_clamp_parts(g, W, H, list(range(80))), g))
        if kind == "stop":
            parts, hole = _stop_parts(g, W, H, (42.0, 0.0, 160.0, 128.0), hole_tile=0)
            sc = Scene(name, W, H, (0.0, 0.0, 0.0), _cat(parts, g))
            sc.meta["hole"] = hole
            return sc
        if kind == "rim":
            # opacity 0.006 .. 0.02: alpha >= 1/255 only in the core of a footprint, and a large share of what contributes lies below 1.5/255
            return Scene(name, W, H, (0.0, 0.0, 0.0), _cat([_field(g, W, H, (0.0, 0.0, 160.0, 128.0), 3000, (2.0, 4.0), (0.006, 0.02))], g))
        if kind in ("background_white", "background_colour"):
            bg = (1.0, 1.0, 1.0) if kind.endswith("white") else (0.3, 0.1, 0.7)
            return Scene(name, W, H, bg, _cat(_background_parts(g, W, H, (0.0, 0.0, 120.0, 100.0)), g))
        if kind == "resumed":
            return Scene(name, W, H, (0.0, 0.0, 0.0), _cat(_resumed_parts(g, W, H, 16.0, 16.0), g))
        if kind == "segmented":
            return Scene(name, W, H, (0.0, 0.0, 0.0), _cat(_segmented_parts(g, W, H, 64.0, 48.0), g))
        if kind == "deep_saturated":
            # two tiles under 1.0 splats to the pixel whose walks end near T = 1e-4 after ~1700 entries: an fp32 limit (the fp32 oracle alone is 1e-3 of
            # S off at single rows), report-only
            return Scene(name, W, H, (0.0, 0.0, 0.0), _cat([_field(g, W, H, (64.0 - 13.0, 48.0 - 13.0, 96.0 + 13.0, 64.0 + 13.0), 2436, (3.8, 4.2), (0.07, 0.11))], g),
                         report_only=True)
        if kind == "background_ragged":
            W, H = 150, 117
            return Scene(name, W, H, (0.3, 0.1, 0.7), _cat(_background_parts(g, W, H, (40.0, 0.0, 150.0, 117.0)), g))
    if fam == "many":
        W, H = 265, 250                                                      # 17 x 16 = 272 tiles, ragged: the streams forward, the one-walker backward
        g = _gen(sum(map(ord, name)) + 7)
        if kind == "stop":
            parts, hole = _stop_parts(g, W, H, (130.0, 120.0, 265.0, 250.0), hole_tile=0)
            sc = Scene(name, W, H, (0.0, 0.0, 0.0), _cat(parts, g))
            sc.meta["hole"] = hole
            return sc
        if kind == "background":
            return Scene(name, W, H, (0.3, 0.1, 0.7), _cat(_background_parts(g, W, H, (40.0, 30.0, 265.0, 250.0)), g))
        if kind == "resumed":
            return Scene(name, W, H, (0.0, 0.0, 0.0), _cat(_resumed_parts(g, W, H, 16.0, 16.0), g))
    raise KeyError(name)


FEW = ["few/clamp", "few/stop", "few/rim", "few/background_white", "few/background_colour", "few/background_ragged", "few/resumed"]
MANY = ["many/stop", "many/background"]
CHAINED = ["many/resumed"]
SEGMENTED = ["few/segmented"]
PASS_FAIL = FEW + MANY + CHAINED + SEGMENTED
REPORT_ONLY = ["few/deep_saturated"]

_O32_ = []


def _O32():
    if not _O32_:
        from oracle.gs_oracle import Oracle
        _O32_.append(Oracle("f32"))
    return _O32_[0]


def _rs_on(sc, device):
    rs = sc.rs
    return rs._replace(bg=rs.bg.to(device), viewmatrix=rs.viewmatrix.to(device), projmatrix=rs.projmatrix.to(device), campos=rs.campos.to(device))

_SCENES = {}


def _settle(sc, oracle64):
    """Dim (by 3 %, repeatedly) every Gaussian that owns a pixel at the alpha = 1/255 threshold (pc.threshold_gaussians and the replay's own
    window) or a visible step at the T = 1e-4 threshold, in either oracle's record, until none is left."""
    rv = dict(sc.rv)

    def hits_of(o, widen):
        f = util.run_oracle(o, sc.rs, rv)
        rp = replay(f, sc.W, sc.H, sc.bg, widen=widen)
        return ({h[0] for h in pc.threshold_gaussians(f, np.nonzero(f["radii"] > 0)[0], sc.W, sc.H, window=widen * ALPHA_WINDOW)}
                | {h[0] for h in rp.alpha_margin} | {h[0] for h in rp.stop_margin})
    for _ in range(40):
        # the loop looks at the fp64 record with windows 1.05 x as wide (the fp32 record differs from it by 1e-6 of alpha and T, a hundredth of
        # the windows), the fp32 record is looked at once it is clean
        hits = hits_of(oracle64, 1.05)
        hits = hits or hits_of(_O32(), 1.0)
        if not hits:
            sc.rv = rv
            return
        o_ = rv["opacities"].clone()
        o_[sorted(hits)] *= 0.97
        rv["opacities"] = o_
    raise AssertionError((sc.name, "threshold pixels left after 40 rounds"))


def scene(name, oracle64):
    if name not in _SCENES:
        sc = _build(name)
        _settle(sc, oracle64)
        _SCENES[name] = sc
    return _SCENES[name]


def upstream(sc):
    """dL/d(colour, depth, opacity, depth^2) = randn, as the issue's probe"""
    g = _gen(1000 + sc.W)
    return dict(color=torch.randn(3, sc.H, sc.W, generator=g), depth=torch.randn(1, sc.H, sc.W, generator=g), opacity=torch.randn(1, sc.H, sc.W, generator=g),
                depth_sq=torch.randn(1, sc.H, sc.W, generator=g))


def _dl_of(sc, entry):
    full = upstream(sc)
    keep = dict(color=("color",), rgbd=("color", "depth"), dos=("color", "depth", "opacity"), all=("color", "depth", "opacity", "depth_sq"))[entry]
    return {k: (v if k in keep else None) for k, v in full.items()}


def recorded_cut(wmax, segments=3):
    """List position of the first cut of a quadrant's walk wmax deep, as the few-tile backward with `segments` walkers takes it: the recorded
    position (every 256th up to 4096) nearest to wmax / segments, 0 below half the first.  (The references are built without a kernel library;
    check_few holds this to the library's gs_recorded_cut.)"""
    target = int(wmax) // segments
    assert target <= 4096 + 128
    pos = 0 if target < 128 else 256 * min(max((target + 128) // 256, 1), 16)
    return pos if pos < wmax else 0


def assert_recorded_cut():
    pos, lvl = C.c_uint32(0), C.c_int32(0)
    lib = _lib.get()
    lib.gs_recorded_cut.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    for segments in (3, 2):
        for wmax in range(1, 1200, 7):
            _lib.check(lib.gs_recorded_cut(wmax // segments, C.byref(pos), C.byref(lvl)))
            assert recorded_cut(wmax, segments) == (int(pos.value) if pos.value < wmax else 0), (wmax, segments)


# ---- references --------------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _grads(oracle, sc, rv, entry, f):
    n = lambda t: None if t is None else t.numpy()  # noqa: E731
    dL = _dl_of(sc, entry)
    if entry in ("all", "dos"):
        assert "cov3D_precomp" not in rv
        g = og.reference(oracle, sc.rs, rv, dL)
    else:
        g = oracle.backward(f, n(dL["color"]), n(dL["depth"]))
    return {k: np.asarray(v, np.float64) for k, v in g.items() if not isinstance(v, dict)}


def reference(sc, entry, oracle64, oracle32, cov=False):
    """-> dict(f64, f32, rp (the replay on the fp64 record, with this entry's upstream gradients), g64, g32, visible); once per (scene, entry)"""
    key = (sc.name, entry, cov)
    if key not in _REFS:
        rv = rg.cov_inputs(sc) if cov else sc.rv
        fkey = (sc.name, "fwd", cov)
        if fkey not in _REFS:
            f64, f32 = util.run_oracle(oracle64, sc.rs, rv), util.run_oracle(oracle32, sc.rs, rv)
            assert np.array_equal(f64["radii"] > 0, f32["radii"] > 0), (sc.name, "the two oracles disagree on visibility: move the splat")
            assert np.array_equal(f64["n_contrib"], f32["n_contrib"]), (sc.name, "the two oracles disagree on n_contrib: the scene is wrong, move it",
                                                                       np.argwhere(f64["n_contrib"] != f32["n_contrib"])[:4].tolist())
            _REFS[fkey] = (f64, f32)
        f64, f32 = _REFS[fkey]
        rp = replay(f64, sc.W, sc.H, sc.bg, dL=_dl_of(sc, entry), cuts=recorded_cut if sc.name == "few/resumed" else None)
        _REFS[key] = dict(f64=f64, f32=f32, rp=rp, g64=_grads(oracle64, sc, rv, entry, f64), g32=_grads(oracle32, sc, rv, entry, f32), visible=f64["radii"] > 0)
    return _REFS[key]


def images_of(f):
    """An oracle's forward -> the five covered outputs"""
    return dict(color=np.asarray(f["color"], np.float64), depth=np.asarray(f["out_depth"], np.float64), opacity=np.asarray(f["opacity"], np.float64),
                depth_sq=np.asarray(f["depth_sq"], np.float64), final_T=np.asarray(f["final_T"], np.float64)[None])


def replay_images(rp):
    """The replay's outputs and absolute sums A_p in the same layout (final T = 1 - sum w: its absolute sum is sum w + T = 1)"""
    img = dict(color=rp.img[0:3], depth=rp.img[3:4], opacity=1.0 - rp.final_T[None], depth_sq=rp.img[5:6], final_T=rp.final_T[None])
    A = dict(color=rp.A[0:3], depth=rp.A[3:4], opacity=rp.A[4:5], depth_sq=rp.A[5:6], final_T=np.ones_like(rp.final_T)[None])
    return img, A


def row_scales(sc, ref, cov=False):
    """s_i of the rule for every tensor judged row by row -> {tensor: [P]}"""
    rp = ref["rp"]
    half = np.array([0.5 * sc.W, 0.5 * sc.H])
    s = dict(colors_precomp=rp.S["dfeat"][:, :3].max(1), opacities=rp.S["dop"][:, 0], means2D=(rp.S["dxy"] * half).max(1))
    if cov:
        den = np.abs(rp.net["dconic"]).max(1)
        kappa = np.where(den > 0, rp.S["dconic"].max(1) / np.where(den > 0, den, 1.0), 1.0)
        s["cov3D_precomp"] = np.abs(ref["g64"]["cov3D_precomp"]).max(1) * np.maximum(kappa, 1.0)
    return s


# ---- what a scene is built to hold: asserted from the replay -------------------------------------------------------------------------------------
def assert_scene(sc, ref):
    rp = ref["rp"]
    kind = sc.name.split("/")[1]
    t = rp.touched
    p = rp.pairs
    info = dict(P=sc.P, longest_list=int(rp.list_len.max()), touched=int(t.sum()), stopped=int((rp.stop_pos >= 0).sum()), **p)
    print(f"[blendpix] scene {sc.name}: {info}")
    assert not rp.alpha_margin and not rp.stop_margin, (sc.name, rp.alpha_margin[:3], rp.stop_margin[:3])
    assert sc.P <= (10000 if kind == "segmented" else 4000), (sc.name, sc.P)
    stopped = rp.stop_pos >= 0
    if stopped.any() and kind != "resumed":
        assert rp.list_len[stopped].max() <= 256, (sc.name, "lists of at most 256 entries where pixels stop", int(rp.list_len[stopped].max()))
    if kind == "clamp":
        front = ref["visible"] & (np.asarray(ref["f64"]["depth"]) < 2.5)                  # the layer of one splat per tile (the few behind it are ordinary)
        assert front.sum() == 80 and float(np.asarray(ref["f64"]["conic_opacity"])[front, 3].min()) >= 0.995 * 0.97 ** 3, sc.name      # (0.995 and up; settling may dim by 3 % steps)
        assert p["clamped"] >= 0.5 * p["contributing"], (sc.name, p)
    elif kind == "stop":
        assert stopped.sum() >= 0.5 * t.sum(), (sc.name, int(stopped.sum()), int(t.sum()))
        have = set(np.unique(rp.stop_pos[stopped]).tolist())
        assert {63, 64, 65, 127, 128, 129} <= have, (sc.name, "stop positions on both sides of 64 and 128", sorted(have & set(range(60, 70)) | have & set(range(124, 133))))
        assert (rp.behind_stop[stopped] >= 64).sum() >= 0.25 * stopped.sum(), (sc.name, "entries behind the stop")
        x, y = sc.meta["hole"]
        q = (slice(y // 8 * 8, y // 8 * 8 + 8), slice(x // 8 * 8, x // 8 * 8 + 8))
        assert t[q].all() and (~stopped[q]).sum() == 1 and not stopped[y, x], (sc.name, "one quadrant with a single pixel that never stops", int((~stopped[q]).sum()))
    elif kind == "rim":
        op = np.asarray(ref["f64"]["conic_opacity"])[ref["visible"], 3]
        assert 0.006 * 0.97 ** 3 <= op.min() and op.max() <= 0.02, (sc.name, op.min(), op.max())
        assert p["box_skipped"] >= 0.5 * p["box"] and p["rim"] >= 0.1 * p["contributing"], (sc.name, p)
    elif kind == "resumed":
        deep = (rp.list_len >= 400) & t
        n_tiles = int(deep.sum()) / 256.0
        assert 6 <= n_tiles <= 12 and rp.list_len.max() <= 800, (sc.name, n_tiles, int(rp.list_len.max()))
        assert rp.final_T[deep & ~stopped].min() >= 1e-2, (sc.name, float(rp.final_T[deep & ~stopped].min()))
        assert (deep & stopped).sum() >= 0.1 * deep.sum(), (sc.name, int((deep & stopped).sum()), int(deep.sum()))
        if sc.name.startswith("few/"):
            assert (rp.past_cut_px & deep).sum() >= 0.5 * deep.sum(), (sc.name, int((rp.past_cut_px & deep).sum()), int(deep.sum()))
            tc = rp.T_at_cut[rp.past_cut_px & deep]
            assert tc.min() >= 1e-2 and tc.max() <= 0.5, (sc.name, float(tc.min()), float(tc.max()))
            assert (rp.stopped_before_cut & deep).sum() >= 0.1 * deep.sum(), (sc.name, int((rp.stopped_before_cut & deep).sum()))
    elif kind == "segmented":
        assert rp.list_len.max() >= 8192 and rp.final_T.min() >= 1e-2 and not stopped.any(), (sc.name, int(rp.list_len.max()), float(rp.final_T.min()))
        busy = rp.list_len >= 8192
        assert 100 <= np.median(rp.n_pairs[busy]) <= 600, (sc.name, float(np.median(rp.n_pairs[busy])))
    elif kind.startswith("background"):
        mid = t & (rp.final_T > 0.2) & (rp.final_T < 0.9)
        assert mid.sum() >= 0.5 * t.sum(), (sc.name, int(mid.sum()), int(t.sum()))
        gx = (sc.W + 15) // 16
        untouched_tiles = [k for k in range(gx * ((sc.H + 15) // 16)) if not t[16 * (k // gx):16 * (k // gx) + 16, 16 * (k % gx):16 * (k % gx) + 16].any()]
        assert untouched_tiles and (~t).sum() >= 256, (sc.name, "untouched tiles")
        assert max(sc.bg) > 0
    return info


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------------
REPORT = []          # (label, output / tensor, worst ratio, class): the tests print it; the device log shows the margins


def oracle_pixel_error(ref):
    """The fp32 oracle's largest |o_32 - o_64| / A_p over every pixel and output -> (value, output)"""
    o64, A = replay_images(ref["rp"])
    o32 = images_of(ref["f32"])
    worst = (0.0, None)
    for k in OUTPUTS:
        m = A[k] > 0
        if m.any():
            e = float((np.abs(o32[k] - o64[k])[m] / A[k][m]).max())
            worst = max(worst, (e, k))
    return worst


def oracle_row_error(sc, ref, cov=False):
    """The fp32 oracle's largest |g_32 - g_64| / s_i over the rendered rows of every tensor judged by rows -> (value, tensor, row)"""
    worst = (0.0, None, -1)
    for k, s in row_scales(sc, ref, cov).items():
        rows = np.nonzero(ref["visible"] & (s > 0))[0]
        if rows.size == 0:
            continue
        e = np.abs(ref["g32"][k].reshape(sc.P, -1) - ref["g64"][k].reshape(sc.P, -1))[rows].max(1) / s[rows]
        j = int(np.argmax(e))
        worst = max(worst, (float(e[j]), k, int(rows[j])))
    return worst


def check_pixels(label, sc, ref, got):
    """got: dict of the kernel's color [3, H, W], depth, opacity, depth_sq, final_T [1, H, W] (absent: not produced by this entry) and n_contrib"""
    rp = ref["rp"]
    bad = np.argwhere(np.asarray(got["n_contrib"], np.int64) != rp.n_contrib)
    if bad.size:
        y, x = bad[0]
        raise AssertionError(f"{label}: n_contrib differs at {len(bad)} pixels, first ({x}, {y}): kernel {int(got['n_contrib'][y, x])}, fp64 {int(rp.n_contrib[y, x])}; "
                             f"classes of the failing pixels: {sorted({pixel_classes(rp, int(b[1]), int(b[0])).split(' at ')[0] for b in bad[:200]})}")
    o64, A = replay_images(rp)
    o32 = images_of(ref["f32"])
    cap = cap_of(FLOOR_F, rp.n_pairs)[None]
    bg = np.asarray(sc.bg, np.float64)
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g = np.asarray(got[k], np.float64).reshape(o64[k].shape)
        assert np.isfinite(g).all(), (label, k)
        exact = dict(color=bg.reshape(3, 1), depth=0.0, opacity=0.0, depth_sq=0.0, final_T=1.0)[k]
        un = ~rp.touched
        assert (g[:, un] == np.broadcast_to(np.float32(exact), g[:, un].shape if k != "color" else (3, int(un.sum())))).all(), (label, k, "a pixel nothing contributes to must be exactly bg / 0 / T = 1")
        err, e32 = np.abs(g - o64[k]), np.abs(o32[k] - o64[k])
        bound = np.minimum(2.0 * e32 + FLOOR_F * A[k], cap * A[k])
        bound = np.where(un[None], np.inf, bound)                  # (judged exactly above)
        ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
        c, y, x = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        REPORT.append((label, k, float(ratio[c, y, x]), pixel_classes(rp, x, y)))
        print(f"[blendpix] {label:44s} {k:9s} worst pixel ({x:3d}, {y:3d}) ratio {ratio[c, y, x]:.3f} ({pixel_classes(rp, x, y)}); error {err[c, y, x]:.2e} of A {A[k][c, y, x]:.2e}, "
              f"fp32 oracle {e32[c, y, x]:.2e}")
        if ratio[c, y, x] > 1.0:
            where = np.argwhere(ratio > 1.0)
            raise AssertionError(f"{label}: {k}: {len(where)} values outside the per-pixel bound, worst pixel ({x}, {y}) channel {c} ({pixel_classes(rp, x, y)}): ratio "
                                 f"{ratio[c, y, x]:.3f}, kernel {g[c, y, x]!r} fp64 {o64[k][c, y, x]!r} fp32 oracle {o32[k][c, y, x]!r}; classes of the failing pixels: "
                                 f"{sorted({pixel_classes(rp, int(b[2]), int(b[1])).split(' at ')[0] for b in where[:200]})}")


def check_rows(label, sc, ref, got, cov=False):
    """got: {tensor: [P, .]} of the kernel.  colors_precomp, opacities, means2D (cov: and cov3D_precomp) row by row against the rule."""
    rp, vis = ref["rp"], ref["visible"]
    cap = cap_of(FLOOR_B, rp.rows["pixels"])
    for k, s in row_scales(sc, ref, cov).items():
        G = np.asarray(got[k], np.float64).reshape(sc.P, -1)
        R64, R32 = ref["g64"][k].reshape(sc.P, -1), ref["g32"][k].reshape(sc.P, -1)
        assert np.isfinite(G).all(), (label, k, "non-finite gradient in rows", np.nonzero(~np.isfinite(G).all(1))[0][:8].tolist())
        live = vis & (rp.rows["pixels"] > 0)
        dead = np.nonzero(~live & (np.abs(G).max(1) != 0))[0]
        assert dead.size == 0, (label, k, "rows of Gaussians that were not rendered must be exactly zero", dead[:8].tolist())
        rows = np.nonzero(live & (s > 0))[0]
        if rows.size == 0:
            continue
        e_k, e_32 = np.abs(G - R64)[rows], np.abs(R32 - R64)[rows]
        s_ = s[rows][:, None]
        bound = np.minimum(2.0 * e_32 + FLOOR_B * s_, cap[rows][:, None] * s_)
        ratio = (e_k / bound).max(1)
        j = int(np.argmax(ratio))
        REPORT.append((label, k, float(ratio[j]), row_classes(rp, rows[j])))
        print(f"[blendpix] {label:44s} {k:14s} worst row {rows[j]:4d} ratio {ratio[j]:.3f} ({row_classes(rp, rows[j])}); error {float(e_k[j].max() / s_[j]):.2e} of S, "
              f"fp32 oracle {float(e_32[j].max() / s_[j]):.2e}")
        if ratio[j] > 1.0:
            bad = rows[ratio > 1.0]
            raise AssertionError(f"{label}: {k}: {bad.size} of {rows.size} rows outside the per-row bound, worst row {rows[j]} ({row_classes(rp, rows[j])}): ratio {ratio[j]:.3f}, "
                                 f"kernel {G[rows[j]].tolist()} fp64 {R64[rows[j]].tolist()} fp32 oracle {R32[rows[j]].tolist()}, S {float(s[rows[j]]):.3e}; classes of the failing "
                                 f"rows: {[row_classes(rp, int(b)) for b in bad[:6]]}")


# ---- the entry points --------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def run_entry(sc, entry, device, rv=None):
    """One forward + backward of the kernel through `entry` -> (images incl. final_T and n_contrib, gradients)"""
    rv = sc.rv if rv is None else rv
    rs = _rs_on(sc, device)
    dL = {k: (None if v is None else v.to(device)) for k, v in _dl_of(sc, entry).items()}
    inp, m2d = og.leaves({k: v.to(device) for k, v in rv.items()})
    with R.capture() as state:
        if entry == "color":
            color, _r, depth, opacity = R.GaussianRasterizer(raster_settings=rs)(means2D=m2d, **inp)
            images = dict(color=color, depth=depth, opacity=opacity)
        else:
            color, _r, depth, opacity, dsq = R.render_rgbd(rs, means2D=m2d, differentiable_outputs=dict(all=EVERYTHING, dos=("depth", "silhouette"), rgbd=("depth",))[entry], **inp)
            images = dict(color=color, depth=depth, opacity=opacity, depth_sq=dsq)
    util.LAST.clear(); util.LAST.update(state)
    art = util.artefacts()
    og.loss_of(images, dL).backward()
    got = {k: _np(v) for k, v in images.items()}
    got["final_T"], got["n_contrib"] = art["final_T"][None], art["n_contrib"]
    return got, og.collect(inp, m2d)


def check_scene(name, device, oracle64, oracle32, entries=ENTRIES, knob=""):
    """One scene through the entries: every pixel and every rendered row against the rules (a report-only scene prints its ratios)."""
    sc = scene(name, oracle64)
    for entry in entries:
        ref = reference(sc, entry, oracle64, oracle32)
        assert_scene(sc, ref)
        got, grads = run_entry(sc, entry, device)
        label = f"{name} {entry}{knob}"
        check_pixels(label, sc, ref, got)
        check_rows(label, sc, ref, grads)


def check_cov(name, device, oracle64, oracle32):
    """The cov3D_precomp entry (render_rgbd, colour and depth gradient): dL/dconic reaches cov3D_precomp alone"""
    sc = scene(name, oracle64)
    ref = reference(sc, "rgbd", oracle64, oracle32, cov=True)
    got, grads = run_entry(sc, "rgbd", device, rv=rg.cov_inputs(sc))
    check_pixels(f"{name} rgbd cov3D_precomp", sc, ref, got)
    check_rows(f"{name} rgbd cov3D_precomp", sc, ref, grads, cov=True)


def tensor_rule(name, device, oracle64, oracle32):
    """means3D, scales and rotations of a scene: the unchanged parity_cases.check_backward"""
    sc = scene(name, oracle64)
    rs = _rs_on(sc, device)._replace(debug=True)
    pc.check_backward(rs, {k: v.to(device) for k, v in sc.rv.items()}, oracle64, seed=3, oracle32=oracle32)


def check_few(name, device, oracle64, oracle32):
    """A few-tile scene: the pc forward and the few-tile backward with three, two and one list segments (the knob is restored)."""
    lib = _lib.get()
    assert_recorded_cut()
    try:
        for segs in (3, 2, 1):
            _lib.check(lib.gs_set_backward_segments(segs))
            check_scene(name, device, oracle64, oracle32, entries=ENTRIES if segs == 3 else ("rgbd", "dos"), knob=f" segments={segs}")
        _lib.check(lib.gs_set_backward_segments(3))
        check_cov(name, device, oracle64, oracle32)
        tensor_rule(name, device, oracle64, oracle32)
    finally:
        _lib.check(lib.gs_set_backward_segments(3))


def check_chained(name, pieces, device, oracle64, oracle32):
    """The resumed scene in the 272-tile image with the chain threshold lowered to 256 tiles: every quadrant's walk in `pieces` chained pieces,
    each taking over (T, S) from the piece behind it (the knob is restored)."""
    lib = _lib.get()
    try:
        _lib.check(lib.gs_set_backward_chain(pieces, 256))
        check_scene(name, device, oracle64, oracle32, knob=f" chain={pieces}")
        tensor_rule(name, device, oracle64, oracle32)
    finally:
        _lib.check(lib.gs_set_backward_chain(3, -1))


def check_report_only(name, device, oracle64, oracle32):
    """A scene outside the rules' regime: its ratios against the same bounds are printed; it is judged by pc.check_forward / check_backward alone."""
    sc = scene(name, oracle64)
    ref = reference(sc, "rgbd", oracle64, oracle32)
    got, grads = run_entry(sc, "rgbd", device)
    for fn, arg in ((check_pixels, got), (check_rows, grads)):
        try:
            fn(f"{name} rgbd (report only)", sc, ref, arg)
        except AssertionError as e:
            print(f"[blendpix] report only: {str(e)[:300]}")
    rs = _rs_on(sc, device)._replace(debug=True)
    rv = {k: v.to(device) for k, v in sc.rv.items()}
    pc.check_forward(rs, rv, oracle32)
    pc.check_backward(rs, rv, oracle64, seed=3, oracle32=oracle32)


def check_segmented(name, device, oracle64, oracle32):
    """The tile list of more than 8192 entries: the forward in list segments (asserted from the binning layout of the run)"""
    check_scene(name, device, oracle64, oracle32)
    assert int(util.LAST["bl"].segments) > 1, int(util.LAST["bl"].segments)


def check_many(name, device, oracle64, oracle32):
    """A many-tile scene (272 tiles): the streams forward and the one-walker backward."""
    check_scene(name, device, oracle64, oracle32)
    check_cov(name, device, oracle64, oracle32)
    tensor_rule(name, device, oracle64, oracle32)


def all_references(oracle64, oracle32):
    """Every (scene, entry) reference of the pass/fail scenes -> [(label, scene, ref, cov)]: what the floors are measured on"""
    out = []
    for name in PASS_FAIL:
        sc = scene(name, oracle64)
        for entry in ENTRIES:
            out.append((f"{name} {entry}", sc, reference(sc, entry, oracle64, oracle32), False))
        if name not in SEGMENTED:
            out.append((f"{name} rgbd cov", sc, reference(sc, "rgbd", oracle64, oracle32, cov=True), True))
    return out
