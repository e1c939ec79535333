"""The C++ autograd front-end of the drop-in call (activesplat_amd/csrc/torch_frontend.cpp) against its Python twin (rasterizer._RasterizeGaussians):
the shared cases of tests/test_frontend.py (the twin on the host-emulated kernels), tests/test_gpu_frontend.py (both routes on the device) and
tests/test_gpu_frontend_concurrency.py (streams, threads, evictions; device only).

Two references, neither of them the code under test: the fp32 / fp64 oracles (parity_cases.check_forward / check_backward, output_grad_cases.compare,
unchanged) and the CANONICAL CALL of a case -- the Python twin on `x.detach().to(float32).contiguous().clone()` leaves of the same values, inside
capture(), with the capacity table cleared in front of it (an exact launch).

Bars.  Forward outputs and the integer artefacts: bit equality (every scene here is walked by one workgroup per tile list: `bl.segments <= 1` is
asserted).  Gradients: on the emulated build (one host thread, a fixed order of the sums) bit equality; on the device the bar check_chained_backward
uses between two orders of the atomic sums, relative L2 <= 2e-5 (BAR).  A leaf handed in as `leaf[P,1].expand(P,3)` receives the row sum of the
[P,3] gradient, which autograd forms in fp32 with two additions per row: each addition rounds by at most 2^-24 of its result, and both results are
bounded by sum_j |g_j|, so the bar there is BAR + 2 * 2^-24 * ||sum_j |g_j||| / ||ref|| against the fp64 row sum of the canonical gradient."""
import contextlib
import threading

import numpy as np
import torch

from activesplat_amd import rasterizer as R
from tests import output_grad_cases as og
from tests import parity_cases as pc
from tests import util
from tests.regime_cases import INTEGER_ARTEFACTS

BAR = 2e-5
SCENES = ("plain", "sh3", "cov3d", "tiles306")
SEEDS = dict(plain=3, sh3=13, cov3d=17, tiles306=21)
FORMS = ("slice", "transposed", "fp64", "offset")
#: (scene, input) pairs of section A: every input of the call on the smallest scene that has it
INPUTS = [("plain", "means3D"), ("plain", "opacities"), ("plain", "scales"), ("plain", "rotations"), ("plain", "colors_precomp"), ("sh3", "shs"),
          ("cov3d", "cov3D_precomp")]
#: the largest relative L2 seen against the canonical gradients, per section of the cases (printed by every comparison)
MAXREL = {"A": 0.0, "B": 0.0, "C": 0.0}


def scene(name, device):
    """plain: 12 tiles (few-tile forward, three-walker backward); sh3 / cov3d: 30 tiles, SH rows / precomputed covariances; tiles306: the streams
    forward and the plain backward."""
    if name == "plain":
        return og.scene("plain", device)
    if name == "sh3":
        return pc.build_case("sh3", device)
    if name == "cov3d":
        return pc.build_case("cov3d_precomp", device)
    if name == "tiles306":
        return util.scene(3000, 288, 272, seed=21, device=device)
    raise KeyError(name)


def colour_grad(rs, seed, device):
    return og.image_grads(rs, seed, device, which=("color",))


def _stats():
    return R.last_stats.get("optimistic_hits", 0), R.last_stats.get("optimistic_misses", 0)


@contextlib.contextmanager
def route(frontend):
    """`R.use_frontend = frontend` for the block, set and put back by ONE thread: the flag is global to the process, so the worker threads of
    check_two_threads run inside their test thread's block and never touch it themselves (render(..., set_route=False))."""
    old = R.use_frontend
    R.use_frontend = frontend
    try:
        yield
    finally:
        R.use_frontend = old


def leaves_the_route_alone(check):
    """A section C check ends with `R.use_frontend` as it found it: the tests that follow in the session keep the route they rely on."""
    import functools

    @functools.wraps(check)
    def checked(*args, **kw):
        entry = R.use_frontend
        try:
            return check(*args, **kw)
        finally:
            assert R.use_frontend is entry, (check.__name__, entry, R.use_frontend)
    return checked


def render(rs, args, m2d, frontend, capture=True, entry="dropin", outputs=None, set_route=True):
    """One call through the C++ front-end (frontend=True) or the Python twin -> (output tensors by name, capture state, (hits, misses) it counted).
    set_route=False: the caller's thread has set the route for all of its workers (route()); the flag must then already be `frontend`."""
    before = _stats()
    if not set_route:
        assert R.use_frontend is frontend, (R.use_frontend, frontend)
    with (route(frontend) if set_route else contextlib.nullcontext()):
        with (R.capture() if capture else contextlib.nullcontext({})) as state:
            if entry == "dropin":
                color, radii, depth, opacity = R.GaussianRasterizer(rs, differentiable_outputs=outputs or ())(means2D=m2d, **args)
                depth_sq = None
            else:
                kw = {} if outputs is None else dict(differentiable_outputs=outputs)
                color, radii, depth, opacity, depth_sq = R.render_rgbd(rs, means2D=m2d, **kw, **args)
    if color.grad_fn is not None and color.device.type == "cuda":
        # the route asked for is the route taken: the twin is never used silently in the front-end's place (nor the other way round)
        assert ("_RasterizeGaussians" in color.grad_fn.name()) == (not frontend), (frontend, color.grad_fn.name())
    after = _stats()
    return dict(color=color, radii=radii, depth=depth, opacity=opacity, depth_sq=depth_sq), dict(state), (after[0] - before[0], after[1] - before[1])


def host(out):
    return {k: v.detach().cpu().numpy() for k, v in out.items() if v is not None}


def decode(state):
    """The integer artefacts of a captured forward (util.artefacts), and that one workgroup walked every tile list."""
    assert int(state["bl"].segments) <= 1, int(state["bl"].segments)
    if state["P"] == 0:
        return None
    util.LAST.clear(); util.LAST.update(state)
    art = util.artefacts()
    return {k: art[k] for k in INTEGER_ARTEFACTS + ("path",)}


def canonical_leaves(rv, requires=True):
    inp = {k: v.detach().to(torch.float32).contiguous().clone().requires_grad_(requires) for k, v in rv.items()}
    return inp, torch.zeros(rv["means3D"].shape[0], 3, device=rv["means3D"].device, requires_grad=requires)


_CANON = {}


def canonical(tag, rs, rv, seed):
    """The canonical call of (rs, rv) with the loss <dL/dcolor(seed), color>, computed once per (tag, device) and kept on the host."""
    key = (tag, str(rv["means3D"].device))
    if key not in _CANON:
        R._capacity.clear()
        inp, m2d = canonical_leaves(rv)
        out, state, _ = render(rs, inp, m2d, frontend=False)
        art = decode(state)
        og.loss_of(out, colour_grad(rs, seed, m2d.device)).backward()
        _CANON[key] = dict(out=host(out), art=art, grads=og.collect(inp, m2d), D=int(state["D"]))
        for v in _CANON[key]["out"].values():
            v.setflags(write=False)
    return _CANON[key]


def canonical_scene(name, device):
    rs, rv = scene(name, device)
    return rs, rv, canonical(name, rs, rv, SEEDS[name])


def same_forward(out, can, what):
    for k in ("color", "depth", "opacity", "radii"):
        assert np.array_equal(out[k], can["out"][k]), (what, k)


def same_artefacts(art, can, what):
    if can["art"] is None:
        assert art is None, what
        return
    live = can["out"]["radii"] > 0
    for k in INTEGER_ARTEFACTS:
        a, b = (art[k][live], can["art"][k][live]) if k == "rect" else (art[k], can["art"][k])      # (a culled row's rectangle is not defined)
        assert np.array_equal(a, b), (what, k)
    assert art["path"] == can["art"]["path"], what


def rel_l2(g, r):
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64).reshape(np.shape(g))
    nr = float(np.linalg.norm(r))
    return float(np.linalg.norm(g - r)) / nr if nr > 0.0 else (0.0 if not np.abs(g).any() else float("inf"))


def grads_close(got, ref, exact, what, section, bar=BAR, scale=1.0):
    """Every gradient of `got` against scale x `ref`: bit for bit on the emulated build, within `bar` relative L2 on the device."""
    for k, g in got.items():
        r = np.asarray(ref[k]).reshape(g.shape) * np.float32(scale)
        assert np.isfinite(g).all(), (what, k)
        e = rel_l2(g, r)
        MAXREL[section] = max(MAXREL[section], e)
        print(f"frontend {section} {what} {k}: rel {e:.3e} (largest of section {section} so far {MAXREL[section]:.3e})")
        if exact:
            assert np.array_equal(g, r), (what, k, e)
        else:
            assert e <= bar, (what, k, e)


# ---- A. tensor forms ----------------------------------------------------------------------------------------------------------------------------
def as_form(x, form):
    """x in one of the input forms -> (leaf, the tensor handed to the call, leaf.grad -> dL/d(handed values), leaf.grad -> the elements beside them)."""
    x = x.detach()
    nothing = lambda g: g.reshape(-1)[:0]  # noqa: E731
    if form == "plain":
        leaf = x.clone().requires_grad_(True)
        return leaf, leaf, (lambda g: g), nothing
    if form == "slice":                                        # a column slice of a wider tensor
        wide = torch.zeros(*x.shape[:-1], x.shape[-1] + 2, dtype=x.dtype, device=x.device)
        wide[..., 1:-1] = x
        leaf = wide.requires_grad_(True)
        arg = leaf[..., 1:-1]
        assert not arg.is_contiguous() or x.shape[0] < 2
        return leaf, arg, (lambda g: g[..., 1:-1]), (lambda g: torch.cat([g[..., :1], g[..., -1:]], -1).reshape(-1))
    if form == "transposed":                                   # the leaf itself lives in a transposed storage
        leaf = x.transpose(0, -1).contiguous().transpose(0, -1).detach().requires_grad_(True)
        assert leaf.shape == x.shape and (not leaf.is_contiguous() or x.shape[-1] == 1 or x.shape[0] < 2)      # ([P,1]: only in the mixed call)
        return leaf, leaf, (lambda g: g), nothing
    if form == "fp64":
        leaf = x.double().requires_grad_(True)
        return leaf, leaf, (lambda g: g), nothing
    if form == "offset":                                       # contiguous, but one element into its storage: not 16-byte aligned
        buf = torch.zeros(x.numel() + 1, dtype=x.dtype, device=x.device)
        buf[1:] = x.reshape(-1)
        leaf = buf.requires_grad_(True)
        arg = leaf[1:].view(x.shape)
        assert arg.is_contiguous() and (arg.data_ptr() % 16 != 0 or x.numel() == 0)
        return leaf, arg, (lambda g: g[1:].view(x.shape)), (lambda g: g[:1])
    raise KeyError(form)


def settings_form(rs, which):
    """The settings with one tensor in another form: "view" the non-contiguous [1,4,4] transpose setup_camera's arithmetic produces, "proj" in fp64,
    "bg" on the host."""
    if "view" in which:
        v = rs.viewmatrix.reshape(4, 4).t().contiguous().unsqueeze(0).transpose(1, 2)
        assert not v.is_contiguous() and torch.equal(v.reshape(16), rs.viewmatrix.reshape(16))
        rs = rs._replace(viewmatrix=v)
    if "proj" in which:
        rs = rs._replace(projmatrix=rs.projmatrix.double())
    if "bg" in which:
        rs = rs._replace(bg=rs.bg.cpu())
    return rs


MIXED = dict(means3D="slice", opacities="offset", scales="transposed", rotations="fp64", colors_precomp="slice", shs="fp64", cov3D_precomp="offset")


def run_forms(rs, rv, forms, frontend, seed, capture=True):
    """The call with rv[k] in forms.get(k, "plain") and the colour loss of `seed` -> (outputs, artefacts, gradients of the handed values, hits / misses);
    asserts what holds of every leaf whatever the reference: .grad has the leaf's shape and dtype, is zero beside the handed values, and an fp64
    leaf's gradient is an fp32 number converted exactly."""
    made = {k: as_form(v, forms.get(k, "plain")) for k, v in rv.items()}
    m2d = torch.zeros(rv["means3D"].shape[0], 3, device=rv["means3D"].device, requires_grad=True)
    out, state, stats = render(rs, {k: m[1] for k, m in made.items()}, m2d, frontend, capture=capture)
    art = decode(state) if capture else None
    og.loss_of(out, colour_grad(rs, seed, m2d.device)).backward()
    grads = {"means2D": m2d.grad.detach().cpu().numpy()}
    for k, (leaf, _arg, pick, beside) in made.items():
        g = leaf.grad
        assert g is not None and g.shape == leaf.shape and g.dtype == leaf.dtype, (k, forms.get(k))
        assert not bool(beside(g).any()), (k, forms.get(k))
        if g.dtype == torch.float64:
            assert torch.equal(g.float().double(), g), k
        grads[k] = pick(g).detach().cpu().numpy()
    return host(out), art, grads, stats


def check_against_canonical(rs, rv, can, forms, frontend, seed, what, section, capture=True):
    out, art, grads, stats = run_forms(rs, rv, forms, frontend, seed, capture=capture)
    same_forward(out, can, what)
    if capture:
        same_artefacts(art, can, what)
    grads_close(grads, can["grads"], rv["means3D"].device.type == "cpu", what, section)
    return stats


def check_input_forms(name, key, device, frontend):
    """rv[key] in every one of FORMS, the other inputs plain.  A [P,1] input (opacities) has no transposed form that differs from the plain
    one -- strides (1, P) with a last dimension of one count as contiguous --, so that form is left out for it: its non-contiguous form is the slice."""
    rs, rv, can = canonical_scene(name, device)
    for form in FORMS:
        if form == "transposed" and rv[key].shape[-1] == 1:
            continue
        check_against_canonical(rs, rv, can, {key: form}, frontend, SEEDS[name], f"{name} {key} {form} frontend={frontend}", "A")


def check_all_forms_together(name, device, frontend):
    """Every input in a form of its own, and the three settings forms, in one call."""
    rs, rv, can = canonical_scene(name, device)
    check_against_canonical(settings_form(rs, ("view", "proj", "bg")), rv, can, MIXED, frontend, SEEDS[name], f"{name} mixed frontend={frontend}", "A")


def check_settings_forms(name, device, frontend):
    rs, rv, can = canonical_scene(name, device)
    for which in ("view", "proj", "bg"):
        check_against_canonical(settings_form(rs, (which,)), rv, can, {}, frontend, SEEDS[name], f"{name} settings {which} frontend={frontend}", "A")


def check_expanded_scales(device, frontend):
    """scales = leaf[P,1].expand(P,3): the leaf receives the row sum of the [P,3] gradient."""
    rs, rv = scene("plain", device)
    iso = rv["scales"][:, :1].contiguous()
    rv = dict(rv, scales=iso.expand(-1, 3))
    can = canonical("plain iso", rs, rv, SEEDS["plain"])
    leaf = iso.clone().requires_grad_(True)
    inp, m2d = canonical_leaves({k: v for k, v in rv.items() if k != "scales"})
    out, state, _ = render(rs, dict(inp, scales=leaf.expand(-1, 3)), m2d, frontend)
    art = decode(state)
    og.loss_of(out, colour_grad(rs, SEEDS["plain"], m2d.device)).backward()
    what = f"plain expanded scales frontend={frontend}"
    same_forward(host(out), can, what)
    same_artefacts(art, can, what)
    exact = rv["means3D"].device.type == "cpu"
    grads_close(og.collect(inp, m2d), {k: v for k, v in can["grads"].items() if k != "scales"}, exact, what, "A")
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype
    g3 = np.asarray(can["grads"]["scales"], np.float64)
    ref = g3.sum(1, keepdims=True)
    two_additions = 2.0 * 2.0 ** -24 * float(np.linalg.norm(np.abs(g3).sum(1))) / float(np.linalg.norm(ref))
    e = rel_l2(leaf.grad.detach().cpu().numpy(), ref)
    print(f"frontend A {what} scales: rel {e:.3e}, two fp32 additions per row allow {two_additions:.3e}")
    assert e <= (0.0 if exact else BAR) + two_additions, (what, e, two_additions)


def check_scene_against_the_oracles(name, device, frontend, oracle32, oracle64):
    """The scene through parity_cases.check_forward / check_backward, unchanged, on the route under test: "equal to the twin" is tied to the oracles."""
    rs, rv = scene(name, device)
    old = R.use_frontend
    R.use_frontend = frontend
    try:
        pc.check_forward(rs, rv, oracle32)
        assert int(util.LAST["bl"].segments) <= 1
        pc.check_backward(rs, rv, oracle64, seed=SEEDS[name], oracle32=oracle32)
    finally:
        R.use_frontend = old


# ---- B. what autograd asks of the backward ------------------------------------------------------------------------------------------------------
def _colour_key(rv):
    return "shs" if "shs" in rv else "colors_precomp"


def check_requires_grad_subset(name, which, device, frontend):
    """Only `which` ("means3D", "colour", "means2D") requires grad: the other leaves keep .grad None, the one matches the all-leaves call."""
    rs, rv, can = canonical_scene(name, device)
    inp, m2d = canonical_leaves(rv, requires=False)
    wanted = _colour_key(rv) if which == "colour" else which
    (m2d if wanted == "means2D" else inp[wanted]).requires_grad_(True)
    out, state, _ = render(rs, inp, m2d, frontend)
    what = f"{name} only {wanted} frontend={frontend}"
    same_forward(host(out), can, what)
    same_artefacts(decode(state), can, what)
    assert out["color"].requires_grad and not (out["radii"].requires_grad or out["depth"].requires_grad or out["opacity"].requires_grad)
    og.loss_of(out, colour_grad(rs, SEEDS[name], m2d.device)).backward()
    leaves = dict(inp, means2D=m2d)
    for k, v in leaves.items():
        assert (v.grad is None) == (k != wanted), (what, k)
    grads_close({wanted: leaves[wanted].grad.detach().cpu().numpy()}, can["grads"], rv["means3D"].device.type == "cpu", what, "B")


def check_no_gradient_wanted(name, device, frontend):
    """No input requires grad / torch.no_grad(): the same outputs, none of them part of a graph."""
    rs, rv, can = canonical_scene(name, device)
    for mode in ("no input requires grad", "torch.no_grad()"):
        inp, m2d = canonical_leaves(rv, requires=mode == "torch.no_grad()")
        with (torch.no_grad() if mode == "torch.no_grad()" else contextlib.nullcontext()):
            out, state, _ = render(rs, inp, m2d, frontend)
        what = f"{name} {mode} frontend={frontend}"
        same_forward(host(out), can, what)
        same_artefacts(decode(state), can, what)
        for k, v in out.items():
            assert v is None or (not v.requires_grad and v.grad_fn is None), (what, k)


def check_colour_left_alone(which, device, frontend, oracle64, oracle32):
    """The loss reads one image output and leaves `color` alone, so the colour gradient reaches the backward undefined: render_rgbd with a loss on
    depth ("depth"), the drop-in call with differentiable_outputs=("opacity",) and a loss on opacity ("opacity").  Against the two-pass fp64 oracle."""
    rs, rv = scene("plain", device)
    rs = rs._replace(debug=False)
    dL = og.image_grads(rs, og.SEEDS["plain"], device, which=(which,))
    assert dL["color"] is None
    inp, m2d = og.leaves(rv)
    if which == "depth":
        out, _, _ = render(rs, inp, m2d, frontend, capture=False, entry="rgbd")
        assert out["depth"].requires_grad and not out["opacity"].requires_grad
    else:
        out, _, _ = render(rs, inp, m2d, frontend, capture=False, outputs=("opacity",))
        assert out["opacity"].requires_grad and not out["depth"].requires_grad
    og.loss_of({k: out[k] for k in ("color", "depth", "opacity")}, dL).backward()
    got = og.collect(inp, m2d)
    assert np.abs(got["colors_precomp"]).max() == 0.0            # no colour term in this loss
    assert np.abs(got["means3D"]).max() > 0.0
    ref = og.reference(oracle64, rs, rv, dL)
    og.compare(got, ref, lambda: og.reference(oracle32, rs, rv, dL), f"colour left alone, loss on {which}, frontend={frontend}")


def check_second_backward(name, device, frontend):
    """backward(retain_graph=True) twice through one graph: the first finds the gradient records zero-filled by the forward, the second must not."""
    rs, rv, can = canonical_scene(name, device)
    exact = rv["means3D"].device.type == "cpu"
    inp, m2d = canonical_leaves(rv)
    out, _, _ = render(rs, inp, m2d, frontend)
    loss = og.loss_of(out, colour_grad(rs, SEEDS[name], m2d.device))
    loss.backward(retain_graph=True)
    first = {k: g.copy() for k, g in og.collect(inp, m2d).items()}       # (on the host the arrays share the memory .grad accumulates into)
    grads_close(first, can["grads"], exact, f"{name} first backward frontend={frontend}", "B")
    loss.backward()
    second = og.collect(inp, m2d)
    grads_close(second, first, exact, f"{name} second backward frontend={frontend}", "B", bar=2 * BAR, scale=2.0)


def check_hit_and_miss(name, device, frontend, oracle64=None, oracle32=None, capture=True):
    """An exact launch fills the capacity table; the second render is an optimistic hit (the backward finds the point list inside the workspace);
    the same (P, W, H) with scale_modifier 4 outgrows the stored guess: a miss, rendered again at exact size (the point list is a tensor of its own).
    capture=False: the same calls outside a capture() block."""
    rs, rv, can = canonical_scene(name, device)
    rs4 = rs._replace(scale_modifier=4.0)
    can4 = canonical(name + " x4", rs4, rv, SEEDS[name])
    P, W, H = rv["means3D"].shape[0], int(rs.image_width), int(rs.image_height)
    tag = f"{name} frontend={frontend} capture={capture}"
    R._capacity.clear()
    inp, m2d = canonical_leaves(rv, requires=False)
    out, state, stats = render(rs, inp, m2d, frontend, capture=capture)
    assert stats == (0, 0), stats
    same_forward(host(out), can, tag + " exact")
    guess = R._capacity[(P, W, H, rv["means3D"].device.index)]
    assert can["D"] <= guess[0]
    stats = check_against_canonical(rs, rv, can, {}, frontend, SEEDS[name], tag + " hit", "B", capture=capture)
    assert stats == (1, 0), stats
    if oracle64 is not None:
        old, before = R.use_frontend, _stats()
        R.use_frontend = frontend
        try:
            pc.check_backward(rs, rv, oracle64, seed=SEEDS[name], oracle32=oracle32)
        finally:
            R.use_frontend = old
        assert (_stats()[0] - before[0], _stats()[1] - before[1]) == (1, 0)      # (check_backward's own render was a hit too)
    stats = check_against_canonical(rs4, rv, can4, {}, frontend, SEEDS[name], tag + " miss", "B", capture=capture)
    assert stats == (0, 1), stats
    assert R.last_stats["num_rendered"] == can4["D"] and (can4["D"] > guess[0] or R.last_stats["max_tile_instances"] > guess[1]), (can4["D"], guess)
    if name == "tiles306":
        assert can4["D"] > guess[0], (can4["D"], guess)           # (here it is the pair count itself that outgrows the guess)


def check_p_edges(which, device, frontend):
    """P = 0, P = 1 (a visible Gaussian), and every Gaussian culled (D = 0), each with its backward."""
    rs, rv, can = canonical_scene("plain", device)
    if which == "P0":
        rv = {k: v[:0] for k, v in rv.items()}
    elif which == "P1":
        i = int(np.nonzero(can["out"]["radii"] > 0)[0][0])
        rv = {k: v[i:i + 1] for k, v in rv.items()}
    else:
        rv = dict(rv, means3D=rv["means3D"] * torch.tensor([1.0, 1.0, -1.0], device=rv["means3D"].device))
    can = canonical("plain " + which, rs, rv, SEEDS["plain"])
    out, art, grads, _ = run_forms(rs, rv, {}, frontend, SEEDS["plain"])
    what = f"plain {which} frontend={frontend}"
    same_forward(out, can, what)
    same_artefacts(art, can, what)
    grads_close(grads, can["grads"], rv["means3D"].device.type == "cpu", what, "B")
    for k, g in grads.items():
        assert g.shape[0] == rv["means3D"].shape[0], (what, k)
    if which == "P1":
        assert out["radii"][0] > 0 and np.abs(grads["means3D"]).max() > 0.0
    if which == "culled":
        assert can["D"] == 0 and not out["radii"].any() and not out["opacity"].any()
        for k, g in grads.items():
            assert np.isfinite(g).all() and not g.any(), (what, k)


# ---- C. streams, threads, evictions (device only) -----------------------------------------------------------------------------------------------
def _forward_backward(rs, rv, seed, frontend):
    """One forward + backward with fresh leaves on the current stream, on the route the caller's route() block has set -> (output tensors,
    leaves); nothing is read back."""
    inp, m2d = canonical_leaves(rv)
    out, _, _ = render(rs, inp, m2d, frontend, capture=False, set_route=False)
    og.loss_of(out, colour_grad(rs, seed, m2d.device)).backward()
    return out, (inp, m2d)


def _check_runs(runs, can, exact, what):
    for i, (out, (inp, m2d)) in enumerate(runs):
        same_forward(host(out), can, f"{what} #{i}")
        grads_close(og.collect(inp, m2d), can["grads"], exact, f"{what} #{i}", "C")


@leaves_the_route_alone
def check_two_side_streams(device, frontend):
    """Scene X on one side stream and scene Y on another, enqueued alternately four times each without a synchronisation in between; every
    backward is started from under the OTHER stream's context (autograd runs it on the stream of its forward)."""
    X, Y = canonical_scene("plain", device), canonical_scene("sh3", device)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dL = {name: colour_grad(case[0], SEEDS[name], device) for name, case in (("plain", X), ("sh3", Y))}
    torch.cuda.synchronize()
    pending = []
    for _ in range(4):
        for (rs, rv, _can), name, st in ((X, "plain", s1), (Y, "sh3", s2)):
            with torch.cuda.stream(st):
                inp, m2d = canonical_leaves(rv)
                out, _, _ = render(rs, inp, m2d, frontend, capture=False)
                loss = og.loss_of(out, dL[name])
            pending.append((name, st, out, (inp, m2d), loss))
    for name, st, _out, _leaves, loss in pending:
        with torch.cuda.stream(s2 if st is s1 else s1):
            loss.backward()
    torch.cuda.synchronize()
    for name, can in (("plain", X[2]), ("sh3", Y[2])):
        _check_runs([(o, l) for n, _s, o, l, _ in pending if n == name], can, False, f"{name} side stream frontend={frontend}")


@leaves_the_route_alone
def check_two_threads(device, frontend, side_stream):
    """Two Python threads of this process, each rendering its own scene eight times, forward and backward; side_stream: the second thread works on
    a stream of its own, else both share the default stream."""
    X, Y = canonical_scene("plain", device), canonical_scene("sh3", device)
    side = torch.cuda.Stream() if side_stream else None
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(name, case, stream):
        try:
            rs, rv, _can = case
            with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
                results[name] = [_forward_backward(rs, rv, SEEDS[name], frontend) for _ in range(8)]
        except BaseException as e:                                # noqa: BLE001  (raised again on the test's thread)
            errors.append((name, e))

    threads = [threading.Thread(target=work, args=("plain", X, None)), threading.Thread(target=work, args=("sh3", Y, side))]
    with route(frontend):                                         # (set once, here: the workers only read the flag)
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    for name, can in (("plain", X[2]), ("sh3", Y[2])):
        _check_runs(results[name], can, False, f"{name} thread side_stream={side_stream} frontend={frontend}")


def _hip_runtime():
    """The HIP runtime this process has loaded (the one torch brought), for hipStreamCreate: torch hands out streams from a pool of 32."""
    import ctypes
    import os
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    assert os.path.exists(path), f"{path}: torch's own HIP runtime not found (any other copy would be a second runtime in this process)"
    return ctypes.CDLL(path)


@leaves_the_route_alone
def check_stream_table_eviction(device, frontend):
    """One render on each of 66 fresh streams (the per-thread tables of counter pairs hold 64, so with the default stream's entry three are
    evicted on the way), then again on the first of them and on the default stream: the outputs are what they were.  WHICH entries went is not
    observable from here (the C++ table evicts an arbitrary one, the twin's its oldest): the case shows that renders stay bit-equal whatever was
    evicted, not that a particular stream's pair was recycled."""
    import ctypes
    rs, rv, can = canonical_scene("plain", device)
    inp, m2d = canonical_leaves(rv, requires=False)
    hip = _hip_runtime()
    hip.hipStreamCreate.argtypes, hip.hipStreamDestroy.argtypes = [ctypes.POINTER(ctypes.c_void_p)], [ctypes.c_void_p]
    handles = []
    try:
        for _ in range(66):
            h = ctypes.c_void_p()
            assert hip.hipStreamCreate(ctypes.byref(h)) == 0
            handles.append(h.value)
        assert len(set(handles)) == 66
        streams = [torch.cuda.ExternalStream(h) for h in handles]
        default = host(render(rs, inp, m2d, frontend, capture=False)[0])
        same_forward(default, can, f"default stream frontend={frontend}")
        torch.cuda.synchronize()
        for i, st in enumerate(streams + [streams[0]]):
            with torch.cuda.stream(st):
                out = host(render(rs, inp, m2d, frontend, capture=False)[0])
            same_forward(out, can, f"stream {i} of 66 frontend={frontend}")
        same_forward(host(render(rs, inp, m2d, frontend, capture=False)[0]), can, f"default stream after 66 streams frontend={frontend}")
    finally:
        torch.cuda.synchronize()
        out = default = None
        torch.cuda.empty_cache()                                  # (the allocator's cached blocks of these streams go back before the streams do)
        for h in handles:
            hip.hipStreamDestroy(h)


@leaves_the_route_alone
def check_layout_table_eviction(device, frontend):
    """Renders at 66 distinct (P, W, H) -- the first P = 1..66 rows of one scene; the layout tables hold 64 -- then the first again."""
    rs, rv, _can = canonical_scene("plain", device)

    def rows(p):
        inp, m2d = canonical_leaves({k: v[:p] for k, v in rv.items()}, requires=False)
        return host(render(rs, inp, m2d, frontend, capture=False)[0])
    first = {p: rows(p) for p in range(1, 67)}
    for p in (1, 2, 66):
        again = rows(p)
        for k in ("color", "depth", "opacity", "radii"):
            assert np.array_equal(again[k], first[p][k]), (p, k, frontend)
    # ... and each is the render of its rows: the twin, with its tables emptied, on three of them
    R._layouts.clear(); R._capacity.clear()
    for p in (1, 33, 66):
        inp, m2d = canonical_leaves({k: v[:p] for k, v in rv.items()}, requires=False)
        ref = host(render(rs, inp, m2d, False, capture=False)[0])
        for k in ("color", "depth", "opacity", "radii"):
            assert np.array_equal(first[p][k], ref[k]), (p, k, frontend)
