"""Shared cases of the kernels that write the map's parameters and statistics on every iteration -- adam.hip (gs_adam_step, gs_adam_step_multi,
GaussianAdam), rows.hip (gs_pack_columns / gs_adam_rows / gs_unpack_columns), the statistics kernels of stats.hip (gs_visibility_stats,
gs_accumulate_grad2d) and gs_keyframe_overlap (grow.hip) -- against references restated HERE in float64 or exact integer torch.  No reference
calls the library.  Run twice: tests/test_optimstep_fp64.py on the host-emulated kernels, tests/test_gpu_optimstep_fp64.py on the device.

The one-step Adam rule (adam_bounds).  u = 2^-24, T = 2^-126 (the smallest normal fp32: a result below it may be rounded to a subnormal or
flushed to zero, either way by less than T).  adam_elem evaluates, every operation rounded to fp32 and none contracted,

    m' = m + c1 (g - m)                 c1 = fl(1 - b1)
    v' = b2 v + (c2 g) g                b2 = fl(beta2), c2 = fl(1 - b2)
    den = sqrt(v') k + e                k = fl(1 / sqrt(1 - beta2^t)), e = fl(eps)
    p' = p - s (m' / den)               s = fl(lr / (1 - beta1^t))

and the float64 reference evaluates torch's single-tensor formula on the float64 images of the same fp32 inputs with the constants formed in
double.  To first order in u, with every constant off by at most u of itself and every operation by at most u of its result:

    E_m = u (3 |c1 (g - m)| + |m'|) + 4 T        the difference, the product with a rounded constant (3 u of the product), the sum (u of m')
    E_v = u (2 b2 v + 3 c2 g^2 + v') + 4 T       b2 v: constant and product; (c2 g) g: constant and two products; the sum.  4 T: g^2 and v
                                                 underflow (|g| < 1e-19), and so may the stored moments
    d_sqrt = sqrt(v') - sqrt(max(v' - E_v, 0))   how far the root moves when v' moves by E_v (exact, no linearisation: v' may be 0)
    E_den = k d_sqrt + 3 u k sqrt(v') + u e + u den      the root's rounding, k's and the product's; e's rounding; the sum
    E_upd = E_m s / den + |upd| (E_den / den + 3 u)      upd = s m' / den: the quotient, s's rounding, the product
    E_p = E_upd + u |p'| + 4 T                   u |p'| is at least half an ulp of p': the rounding of the final subtraction

For p = 0 the subtraction is exact and |p'| = |upd|: E_p is then a bound RELATIVE TO THE UPDATE (about 10 u of it where nothing cancels), which
is what an rtol on a parameter of size 1 never was.  SAFETY = 2 multiplies all three bounds: it covers the second-order terms dropped above and
a square root or division that is faithfully (one ulp = 2 u) rather than correctly rounded.  It is not fitted: the fp32 torch mirror of the
same operation sequence on the CPU must lie inside the bound on every input set (test_adam_rule_holds_for_the_fp32_mirror), and the worst
error / E of kernel and mirror is printed (profiles/README.md holds the figures).  What a bound cannot see -- a constant rounded twice, two
operations swapped: an ulp -- is held by check_adam_bits_equal_mirror: the step equals the sequence above in numpy float32 bit for bit.

Every check prints the figures it asserts on and appends them to REPORT."""
import ctypes as C
import math

import numpy as np
import torch

REPORT = []
U = 2.0 ** -24            # unit roundoff of float32
TINY = 2.0 ** -126        # smallest normal float32
SAFETY = 2.0              # see the module docstring
B1, B2 = 0.9, 0.999


def _say(section, **kw):
    REPORT.append(dict(section=section, **kw))
    print(section, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _lib():
    from activesplat_amd import _lib as L
    return L, L.get()


def _stream(device):
    from activesplat_amd import _lib as L
    return L.stream_ptr(torch.device(device))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


# =====================================================================================================================================
# 1. One Adam step against float64
# =====================================================================================================================================
def adam_reference64(p, g, m, v, lr, eps, step, b1=B1, b2=B2):
    """torch.optim.Adam's single-tensor step (no weight decay, no amsgrad) in float64 -> m', v', update, p - update, denominator."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m1 = m + (1.0 - b1) * (g - m)                   # exp_avg.lerp_(grad, 1 - beta1)
    v1 = b2 * v + (1.0 - b2) * g * g                # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    den = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    return m1, v1, upd, p - upd, den


def adam_bounds(p, g, m, v, lr, eps, step, b1=B1, b2=B2):
    """-> (E_m, E_v, E_p) of the module docstring, float64, WITHOUT the safety factor."""
    m1, v1, upd, p1, den = adam_reference64(p, g, m, v, lr, eps, step, b1, b2)
    g, m, v = g.double(), m.double(), v.double()
    k, s = 1.0 / math.sqrt(1.0 - b2 ** step), lr / (1.0 - b1 ** step)
    e_m = U * (3 * ((1 - b1) * (g - m)).abs() + m1.abs()) + 4 * TINY
    e_v = U * (2 * b2 * v + 3 * (1 - b2) * g * g + v1) + 4 * TINY
    sq = v1.sqrt()
    d_sqrt = sq - (v1 - e_v).clamp_min(0).sqrt()
    e_den = k * d_sqrt + 3 * U * k * sq + U * eps + U * den
    e_upd = e_m * s / den + upd.abs() * (e_den / den + 3 * U)
    e_p = e_upd + U * p1.abs() + 4 * TINY
    return e_m, e_v, e_p


def adam_mirror32(p, g, m, v, lr, eps, step, b1=B1, b2=B2):
    """adam_elem's operation sequence in fp32 torch on the CPU (element-wise ops, no contraction); constants rounded once from double."""
    f = lambda x: torch.tensor(x, dtype=torch.float64).float()  # noqa: E731
    c1, b2f, c2 = f(1.0 - b1), f(b2), f(1.0 - b2)
    s, k, e = f(lr / (1.0 - b1 ** step)), f(1.0 / math.sqrt(1.0 - b2 ** step)), f(eps)
    m1 = m + c1 * (g - m)
    v1 = b2f * v + (c2 * g) * g
    den = v1.sqrt() * k + e
    return p - s * (m1 / den), m1, v1


def adam_ratios(before, after, lr, eps, step, where=None):
    """worst |kernel - float64| / E per quantity (E without the safety factor) over the elements of `where` (default: all)."""
    p, g, m, v = before
    m1, v1, _, p1, _ = adam_reference64(p, g, m, v, lr, eps, step)
    e_m, e_v, e_p = adam_bounds(p, g, m, v, lr, eps, step)
    out = {}
    for name, got, ref, e in (("p", after[0], p1, e_p), ("m", after[1], m1, e_m), ("v", after[2], v1, e_v)):
        r = (got.double() - ref).abs() / e
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)      # a NaN where the reference is finite is a miss
        if where is not None:
            r = r[where]
        out[name] = float(r.max()) if r.numel() else 0.0
    return out


def assert_adam_rule(tag, before, after, lr, eps, step, where=None):
    r = adam_ratios(before, after, lr, eps, step, where)
    _say("adam", case=tag, n=int(before[0].numel()), step=step, p=r["p"], m=r["m"], v=r["v"])
    for q in ("p", "m", "v"):
        assert r[q] <= SAFETY, f"{tag}: {q} misses the one-step rule: error / bound = {r[q]:.3f} > {SAFETY}"
    return r


ADAM_SETS = ("p0", "p1e3", "fresh", "g0", "logg_eps15", "logg_eps8", "lr0")
ADAM_STEPS = (1, 2, 10, 1000, 100000)


def _log_uniform(n, lo, hi, g):
    return 10.0 ** (math.log10(lo) + (math.log10(hi) - math.log10(lo)) * torch.rand(n, generator=g, dtype=torch.float64))


def adam_inputs(kind, n, seed=0):
    """-> (p, g, m, v) fp32 CPU, lr, eps.  Moments of a run in progress unless the set says otherwise: m ~ 0.3 of the gradient scale, v its
    square."""
    gen = torch.Generator().manual_seed(97 * seed + 13 * ADAM_SETS.index(kind) + n % 1009)
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)  # noqa: E731
    lr, eps = 1e-3, 1e-15
    scale = _log_uniform(n, 1e-4, 1.0, gen)
    g, p = rn() * scale, rn()
    m, v = 0.3 * rn() * scale, scale * scale * (0.1 + torch.rand(n, generator=gen, dtype=torch.float64))
    if kind == "p0":
        p = torch.zeros(n, dtype=torch.float64)
    elif kind == "p1e3":
        p = 1e3 * (1 + torch.rand(n, generator=gen, dtype=torch.float64)) * torch.sign(rn())
    elif kind == "fresh":
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    elif kind == "g0":
        g = torch.zeros(n, dtype=torch.float64)
    elif kind in ("logg_eps15", "logg_eps8"):
        mag = _log_uniform(n, 1e-25, 1e4, gen)
        g = mag * torch.sign(rn())
        m, v = 0.3 * rn() * mag, mag * mag * (0.1 + torch.rand(n, generator=gen, dtype=torch.float64))
        eps = 1e-15 if kind == "logg_eps15" else 1e-8
    elif kind == "lr0":
        lr = 0.0
    return (p.float(), g.float(), m.float(), v.float()), lr, eps


def run_adam(device, api, before, lr, eps, step):
    """One step through gs_adam_step ('single') or gs_adam_step_multi ('multi') -> (p, m, v) on the CPU."""
    L, lib = _lib()
    p, g, m, v = [t.clone().to(device) for t in before]
    n = p.numel()
    if api == "single":
        L.check(lib.gs_adam_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr, B1, B2, eps, step, _stream(device)))
    else:
        arr = (L.GsAdamTensor * 1)(L.GsAdamTensor(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr, B1, B2, eps, step, 0))
        L.check(lib.gs_adam_step_multi(1, arr, _stream(device)))
    return p.cpu(), m.cpu(), v.cpu()


def check_adam_mirror(kind):
    """The guard of the rule: the fp32 mirror lies inside the bound on every input set and step count (CPU only, no kernel)."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step in ADAM_STEPS:
        before, lr, eps = adam_inputs(kind, 20011)
        r = adam_ratios(before, adam_mirror32(*before, lr, eps, step), lr, eps, step)
        worst = {q: max(worst[q], r[q]) for q in worst}
    _say("adam-mirror", set=kind, p=worst["p"], m=worst["m"], v=worst["v"])
    assert max(worst.values()) <= SAFETY, f"the fp32 mirror leaves the one-step bound on {kind}: {worst}"


def check_adam_set(device, kind, n=4099):
    for step in ADAM_STEPS:
        before, lr, eps = adam_inputs(kind, n)
        a, b = run_adam(device, "single", before, lr, eps, step), run_adam(device, "multi", before, lr, eps, step)
        assert all(_same_bits(x, y) for x, y in zip(a, b)), f"{kind} step {step}: gs_adam_step and gs_adam_step_multi differ"
        assert_adam_rule(f"{kind}", before, a, lr, eps, step)
        if kind == "lr0":
            assert _same_bits(a[0], before[0]), "lr = 0 moved a parameter"
            assert not torch.equal(a[1], before[2]) and not torch.equal(a[2], before[3]), "lr = 0: the moments must still advance"
        if kind == "p0":                         # the update itself: p' = -upd, and the bound is relative to it (module docstring)
            _, _, upd, _, _ = adam_reference64(*before, lr, eps, step)
            e_p = adam_bounds(*before, lr, eps, step)[2]
            rel = (e_p / upd.abs().clamp_min(1e-300))
            assert float(rel.median()) < 16 * U, f"the p = 0 bound is not a relative bound on the update: median E_p / |upd| = {float(rel.median()):.2e}"


def adam_mirror32_numpy(p, g, m, v, lr, eps, step, b1=B1, b2=B2):
    """adam_elem's operation sequence in numpy float32: one correctly rounded IEEE operation per line, constants rounded once from double."""
    f = np.float32
    p, g, m, v = (t.numpy() for t in (p, g, m, v))
    c1, b2f, c2 = f(1.0 - b1), f(b2), f(1.0 - b2)
    s, k, e = f(lr / (1.0 - b1 ** step)), f(1.0 / math.sqrt(1.0 - b2 ** step)), f(eps)
    with np.errstate(all="ignore"):
        d = g - m
        m1 = m + c1 * d
        v1 = b2f * v + (c2 * g) * g
        den = np.sqrt(v1) * k + e
        p1 = p - s * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return torch.from_numpy(p1), torch.from_numpy(m1), torch.from_numpy(v1)


def check_adam_bits_equal_mirror(device, kind, n=4099):
    """The header's arithmetic to the bit: adam_elem is contraction-free IEEE fp32 (correctly rounded +, *, /, sqrt) on constants that are formed
    in double and rounded ONCE, so it equals that sequence in numpy float32 bit for bit -- which no bound can ask: a constant rounded twice
    ((float)lr / (float)bc1) or a reordered sum moves the result by an ulp, well inside any first-order bound.  (numpy, not torch: torch's fp32
    square root on the CPU is not correctly rounded -- sqrt(0.002058513928204775f) comes out one ulp low -- which the rule's SAFETY absorbs and a
    bit comparison cannot.)  Compared on the elements none of whose intermediates comes near the subnormals (there the device may flush where
    the host rounds): all of them, except on the two log-uniform sets."""
    for step in ADAM_STEPS:
        before, lr, eps = adam_inputs(kind, n)
        p, g, m, v = before
        got = run_adam(device, "multi", before, lr, eps, step)
        want = adam_mirror32_numpy(p, g, m, v, lr, eps, step)
        m1, v1, upd, _, _ = adam_reference64(p, g, m, v, lr, eps, step)
        g64, m64, v64 = g.double(), m.double(), v.double()
        inter = [g64, m64, v64, g64 - m64, (g64 - m64) * (1 - B1), m1, B2 * v64, (1 - B2) * g64, (1 - B2) * g64 ** 2, v1, upd]
        clear = torch.ones(n, dtype=torch.bool)
        for x in inter:
            clear &= (x == 0) | (x.abs() >= 2.0 ** -100)
        frac = float(clear.float().mean())
        assert (frac > 0.5) if kind.startswith("logg") else (frac == 1.0), f"{kind}: only {frac:.2%} of the elements stay clear of the subnormals"
        for name, a, b in zip("pmv", got, want):
            diff = _bits(a)[clear] != _bits(b)[clear]
            assert not bool(diff.any()), f"{kind} step {step}: {int(diff.sum())} elements of {name} differ from the fp32 sequence in their bits"


def check_adam_evolution(device, steps=30, n=2051):
    """30 consecutive steps; at every step the reference restarts from the kernel's own fp32 state."""
    (p, g, m, v), lr, eps = adam_inputs("fresh", n, seed=3)
    gen = torch.Generator().manual_seed(5)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step in range(1, steps + 1):
        g = (torch.randn(n, generator=gen, dtype=torch.float64) * _log_uniform(n, 1e-6, 1e1, gen)).float()
        after = run_adam(device, "multi", (p, g, m, v), lr, eps, step)
        r = adam_ratios((p, g, m, v), after, lr, eps, step)
        worst = {q: max(worst[q], r[q]) for q in worst}
        p, m, v = after
    _say("adam-evolution", steps=steps, p=worst["p"], m=worst["m"], v=worst["v"])
    assert max(worst.values()) <= SAFETY, f"a step of the evolution misses the rule: {worst}"


def check_adam_nonfinite(device):
    """A NaN and a +-inf gradient in the middle of a float4: only that element's p, m, v become non-finite."""
    (p, g, m, v), lr, eps = adam_inputs("p0", 16, seed=9)
    bad = [5, 9, 14]
    g[5], g[9], g[14] = float("nan"), float("inf"), float("-inf")
    ok = torch.ones(16, dtype=torch.bool); ok[bad] = False
    for api in ("single", "multi"):
        after = run_adam(device, api, (p, g, m, v), lr, eps, 7)
        for t in after:
            assert not torch.isfinite(t[bad]).any(), "a non-finite gradient left a finite parameter or moment"
            assert torch.isfinite(t[ok]).all(), "a non-finite gradient reached a neighbour"
        assert_adam_rule(f"nonfinite/{api}", (p, g, m, v), after, lr, eps, 7, where=ok)


# sizes at which launch_adam / launch_adam_multi change path: n >> 2 float4 pieces, workgroups of 256 lanes, at most 2048 workgroups, so one
# grid pass covers 2048 * 1024 elements; the multi kernel takes a second piece per trip at i + 2048 * 256 float4; the tail n & 3 goes to the
# tensor's first workgroup; n * 28 > 256 MiB (n >= 9 586 981) is the non-temporal instantiation.  (2048 * 1024 + 7 is added to the issue's
# list: the first size at which lane 0 really has a second piece.)
_PASS = 2048 * 1024
ADAM_SIZES = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, _PASS - 1, _PASS + 3, _PASS + 7, 2 * _PASS + 1027, 4 * _PASS + 5)
ADAM_STREAM_SIZES = (9586980, 9586981)
assert ADAM_STREAM_SIZES[0] * 28 <= (256 << 20) < ADAM_STREAM_SIZES[1] * 28


def check_adam_size(device, n):
    before, lr, eps = adam_inputs("logg_eps15" if n % 2 else "p0", max(n, 1), seed=n % 7)
    before = tuple(t[:n].contiguous() for t in before)
    step = 3
    a, b = run_adam(device, "single", before, lr, eps, step), run_adam(device, "multi", before, lr, eps, step)
    assert all(_same_bits(x, y) for x, y in zip(a, b)), f"n = {n}: gs_adam_step and gs_adam_step_multi differ"
    if n:
        assert_adam_rule(f"size {n}", before, a, lr, eps, step)


def multi_sizes(big):
    """19 tensors -> three launches of at most eight; empty tensors at positions 0, 8 and 18.  Tensor 11 has lanes with a second 16-byte piece
    per trip while its launch holds other tensors' workgroups (the piece's stride is the TENSOR's workgroup count, not the grid's); big: tensor 14
    takes a second trip as well."""
    s = [0, 1027, 1, 2, 3, 4, 5, 1023, 0, 1024, 1025, _PASS + 7, 7, 1027, 2 * _PASS + 1027 if big else 2051, 6, 257, 1029, 0]
    assert len(s) == 19 and s[0] == s[8] == s[18] == 0
    return s


def check_adam_multi(device, big):
    L, lib = _lib()
    sizes = multi_sizes(big)
    GUARD = 8
    offs, total = [], GUARD
    for n in sizes:
        offs.append(total)                                    # every tensor starts 16-byte aligned, at least GUARD floats behind the last
        total += (n + 3) // 4 * 4 + GUARD
    sentinel = torch.tensor([-7.25, 3.5e10, float("nan"), 1e-30]).repeat(total // 4 + 1)[:total]
    buf = {q: sentinel.clone() for q in "pgmv"}
    hyper, before = [], []
    for i, (n, o) in enumerate(zip(sizes, offs)):
        t, _, _ = adam_inputs(ADAM_SETS[i % 6], max(n, 1), seed=i)
        lr, eps, step = (1e-4, 2.5e-3, 1e-3, 5e-2)[i % 4], (1e-15, 1e-8)[i % 2], (1, 2, 10, 1000, 100000)[i % 5]
        hyper.append((lr, eps, step))
        before.append(tuple(x[:n].contiguous() for x in t))
        for q, x in zip("pgmv", t):
            buf[q][o:o + n] = x[:n]
    dev = {q: buf[q].clone().to(device) for q in "pgmv"}
    assert all(dev[q].data_ptr() % 16 == 0 for q in "pgmv")
    arr = (L.GsAdamTensor * 19)()
    for i, (n, o) in enumerate(zip(sizes, offs)):
        lr, eps, step = hyper[i]
        ptr = [dev[q].data_ptr() + 4 * o if n else None for q in "pgmv"]
        arr[i] = L.GsAdamTensor(n, ptr[0], ptr[1], ptr[2], ptr[3], lr, B1, B2, eps, step, 0)
    L.check(lib.gs_adam_step_multi(19, arr, _stream(device)))
    out = {q: dev[q].cpu() for q in "pgmv"}
    touched = torch.zeros(total, dtype=torch.bool)
    for i, (n, o) in enumerate(zip(sizes, offs)):
        touched[o:o + n] = True
        if not n:
            continue
        lr, eps, step = hyper[i]
        got = tuple(out[q][o:o + n] for q in "pmv")
        one = run_adam(device, "single", before[i], lr, eps, step)
        assert all(_same_bits(x, y) for x, y in zip(got, one)), f"tensor {i} (n = {n}): the batched step differs from gs_adam_step"
        assert_adam_rule(f"multi[{i}]", before[i], got, lr, eps, step)
    for q in "pmv":
        assert torch.equal(_bits(out[q])[~touched], _bits(buf[q])[~touched]), f"a guard element of {q} changed"
    assert torch.equal(_bits(out["g"]), _bits(buf["g"])), "the gradients changed"


API_LRS = dict(means3D=1e-4, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3, cam_unnorm_rots=0.0, cam_trans=0.0)


def check_gaussian_adam_api(device, n=1031):
    """GaussianAdam against torch.optim.Adam on float64 copies, five steps, the reference's seven groups.  At every step a float64 torch.optim.Adam
    is loaded with the kernel's own state before the step and takes ONE step; the one-step rule applies to what it leaves."""
    from activesplat_amd import optim as O
    gen = torch.Generator().manual_seed(11)
    shapes = dict(means3D=(n, 3), rgb_colors=(n, 3), unnorm_rotations=(n, 4), logit_opacities=(n, 1), log_scales=(n, 1),
                  cam_unnorm_rots=(1, 4, 2), cam_trans=(1, 3, 2))
    params = {k: torch.nn.Parameter(torch.randn(*s, generator=gen).to(device)) for k, s in shapes.items()}
    opt = O.initialize_optimizer(params, API_LRS)
    late = "log_scales"                                       # a gradient only from step 3 on: its own counter starts at 1 then
    for it in range(1, 6):
        state0 = {}
        for k, p in params.items():
            has = not k.startswith("cam_") and (k != late or it >= 3)
            p.grad = (torch.randn(*shapes[k], generator=gen) * 10.0 ** (it - 4)).to(device) if has else None
            st = opt.state.get(p)
            state0[k] = (p.detach().cpu().clone(), None if st is None else st["exp_avg"].cpu().clone(), None if st is None else st["exp_avg_sq"].cpu().clone(),
                         0 if st is None else int(st["step"]))
        opt.step()
        for k, p in params.items():
            p0, m0, v0, t0 = state0[k]
            if p.grad is None:
                assert p not in opt.state, f"{k}: state created for a parameter without a gradient"
                assert _same_bits(p.detach(), p0)
                continue
            st = opt.state[p]
            want_step = it if k != late else it - 2
            assert int(st["step"]) == want_step == t0 + 1, f"{k}: step counter {st['step']} at iteration {it}"
            g = p.grad.cpu()
            q = torch.nn.Parameter(p0.double())
            ref = torch.optim.Adam([{"params": [q], "lr": API_LRS[k]}], lr=0.0, eps=1e-15)
            if t0:
                ref.state[q] = dict(step=torch.tensor(float(t0)), exp_avg=m0.double(), exp_avg_sq=v0.double())
            q.grad = g.double()
            ref.step()
            m0 = torch.zeros_like(p0) if m0 is None else m0
            v0 = torch.zeros_like(p0) if v0 is None else v0
            e_m, e_v, e_p = adam_bounds(p0, g, m0, v0, API_LRS[k], 1e-15, want_step)
            for name, got, want, e in (("p", p.detach().cpu(), q.detach(), e_p), ("m", st["exp_avg"].cpu(), ref.state[q]["exp_avg"], e_m),
                                       ("v", st["exp_avg_sq"].cpu(), ref.state[q]["exp_avg_sq"], e_v)):
                r = float(((got.double() - want).abs() / e).max())
                _say("adam-api", key=k, it=it, quantity=name, ratio=r)
                assert r <= SAFETY, f"GaussianAdam {k} iteration {it}: {name} error / bound = {r:.3f}"


# =====================================================================================================================================
# 2. The alignment contract
# =====================================================================================================================================
def _offset_view(n, device, fill):
    """a contiguous fp32 tensor of n elements whose storage starts one element (4 bytes) behind a 16-byte boundary"""
    base = torch.full((n + 8,), float(fill), device=device)
    assert base.data_ptr() % 16 == 0
    return base, base[1:1 + n]


def check_adam_refuses_misaligned(device):
    """gs_adam_step / gs_adam_step_multi refuse (GS_EINVAL, message with the tensor index) before any launch: every tensor of the call keeps its
    values.  No misaligned launch is made: only the refusal is tested."""
    L, lib = _lib()
    n = 37
    for which in range(4):
        ts = [torch.full((n,), 1.0 + i, device=device) for i in range(4)]
        base, view = _offset_view(n, device, 1.0 + which)
        ts[which] = view
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        rc = lib.gs_adam_step(n, ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), 1e-3, B1, B2, 1e-15, 1, _stream(device))
        assert rc == 1 and "tensor 0" in lib.gs_last_error().decode() and "16-byte" in lib.gs_last_error().decode()
        # batched: two good tensors in front (one launch's worth would step them if the check came late), the bad one at index 9 (second launch)
        good = [[torch.full((n,), 1.0 + i, device=device) for i in range(4)] for _ in range(10)]
        good[9] = ts
        arr = (L.GsAdamTensor * 10)(*[L.GsAdamTensor(n, *[x.data_ptr() for x in t], 1e-3, B1, B2, 1e-15, 1, 0) for t in good])
        rc = lib.gs_adam_step_multi(10, arr, _stream(device))
        assert rc == 1 and "tensor 9" in lib.gs_last_error().decode(), lib.gs_last_error().decode()
        for t in good:
            for i, x in enumerate(t):
                assert bool((x == 1.0 + i).all()), "a refused call changed a tensor"
    # an empty misaligned tensor is nobody's business
    base, view = _offset_view(4, device, 0.0)
    assert lib.gs_adam_step(0, view.data_ptr(), view.data_ptr(), view.data_ptr(), view.data_ptr(), 1e-3, B1, B2, 1e-15, 1, _stream(device)) == 0


def check_gaussian_adam_refuses_misaligned(device):
    """GaussianAdam.step() raises through _lib.check; parameters, moments and step counters of EVERY tensor of the call are as before."""
    from activesplat_amd import optim as O
    n = 41
    a = torch.nn.Parameter(torch.full((n, 3), 2.0, device=device))
    base, view = _offset_view(3 * n, device, 3.0)
    b = view.view(n, 3).detach().requires_grad_(True)
    c = torch.nn.Parameter(torch.full((n, 1), 4.0, device=device))
    assert b.is_contiguous() and b.data_ptr() % 16 == 4
    opt = O.GaussianAdam([{"params": [a], "lr": 1e-2}, {"params": [b], "lr": 1e-2}, {"params": [c], "lr": 1e-2}], lr=0.0, eps=1e-15)
    a.grad, c.grad = torch.ones_like(a), torch.ones_like(c)
    opt.step()                                               # a and c have state and counter 1; b has none yet
    m_a, v_a = opt.state[a]["exp_avg"].clone(), opt.state[a]["exp_avg_sq"].clone()
    pa, pc = a.detach().clone(), c.detach().clone()
    b.grad = torch.ones(n, 3, device=device)
    try:
        opt.step()
    except Exception as e:                                   # noqa: BLE001  (_lib.check raises a plain Exception with the library's message)
        assert "tensor 1" in str(e) and "16-byte" in str(e), str(e)
    else:
        raise AssertionError("GaussianAdam.step() accepted a parameter at an odd element offset")
    assert int(opt.state[a]["step"]) == 1 and int(opt.state[c]["step"]) == 1, "a refused step advanced a counter"
    assert b not in opt.state or int(opt.state[b]["step"]) == 0
    assert _same_bits(a.detach(), pa) and _same_bits(c.detach(), pc) and bool((b.detach() == 3.0).all())
    assert _same_bits(opt.state[a]["exp_avg"], m_a) and _same_bits(opt.state[a]["exp_avg_sq"], v_a)
    b.grad = None
    opt.step()                                               # the optimiser goes on: a and c take their second step
    assert int(opt.state[a]["step"]) == 2 and int(opt.state[c]["step"]) == 2 and not _same_bits(a.detach(), pa)


def check_backward_adam_refuses_misaligned(device, n=300, W=64, H=48):
    """gs_render_backward_raw_adam makes 16-byte accesses to the rotation rows (and the SH rows) of parameter and moments: a moment tensor at an odd
    element offset is refused (tensor 3 of the five descriptors) before the backward launches anything; counters, parameters and moments stay."""
    from activesplat_amd import optim as O, rasterizer as R, synthetic as syn
    from activesplat_amd.camera import setup_camera
    pose = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    cam = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device)
    prm = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in syn.make_params(n, W, H, seed=2).items()}
    opt = O.initialize_optimizer(prm, {k: 1e-3 for k in prm})

    def render():
        m2d = torch.empty_like(prm["means3D"], requires_grad=True)
        return R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], pose, adam=opt,
                                 colors_precomp=prm["rgb_colors"])
    render()[0].sum().backward()                                          # step 1: the state exists
    st = opt.state[prm["unnorm_rotations"]]
    base, view = _offset_view(4 * n, device, 0.0)
    st["exp_avg"] = view.view(n, 4).copy_(st["exp_avg"])
    assert st["exp_avg"].is_contiguous() and st["exp_avg"].data_ptr() % 16 == 4
    snap = {k: (v.detach().clone(), opt.state[v]["exp_avg"].clone(), opt.state[v]["exp_avg_sq"].clone(), int(opt.state[v]["step"])) for k, v in prm.items()
            if v in opt.state}
    assert {s[3] for s in snap.values()} == {1}
    im = render()[0]
    try:
        im.sum().backward()
    except Exception as e:                                   # noqa: BLE001
        assert "tensor 3" in str(e) and "16-byte" in str(e), str(e)
    else:
        raise AssertionError("the backward with the optimiser step accepted rotation moments at an odd element offset")
    for k, (p0, m0, v0, t0) in snap.items():
        s1 = opt.state[prm[k]]
        assert int(s1["step"]) == t0, f"{k}: a refused step advanced the counter"
        assert _same_bits(prm[k].detach(), p0) and _same_bits(s1["exp_avg"], m0) and _same_bits(s1["exp_avg_sq"], v0), f"{k} changed"


# =====================================================================================================================================
# 3. gs_pack_columns / gs_adam_rows / gs_unpack_columns
# =====================================================================================================================================
ROW_WIDTHS = ((3, 3, 4, 1, 3), (3, 3, 4, 1, 1), (3, 48, 4, 1, 3), (16,), (17,), (64,), (1,) * 8, (8,) * 8)
ROWS_NARROW, ROWS_WIDE = (1, 255, 256, 257), (63, 64, 65)
ROWS_NARROW_BIG, ROWS_WIDE_BIG = 4096 * 256 + 300, 4096 * 64 + 70          # the second trip of the row-block loop (at most 4096 workgroups)


def row_counts(widths):
    return ROWS_NARROW if sum(widths) <= 16 else ROWS_WIDE


def check_row_index_rule():
    """rows_kernel takes the row of element j of a key of width w as (int)((j + 0.5f) * (1.0f / w)): equal to j // w for every width the call
    admits and every j of a block (256 rows x 16 floats, 64 rows x 64 floats: j < 256 * 64 covers both).  A change of ROWS / GMAX has to face this."""
    j = np.arange(256 * 64, dtype=np.int64)
    bad = 0
    for w in range(1, 65):
        iw = np.float32(1.0) / np.float32(w)
        row = ((j.astype(np.float32) + np.float32(0.5)) * iw).astype(np.int32)
        bad += int((row != j // w).sum())
    assert bad == 0, f"{bad} (j, w) pairs where the float row index is not j // w"


def _row_array(L, widths, p=None, m=None, v=None, g=None, hyper=None):
    K = len(widths)
    arr = (L.GsRowTensor * K)()
    ptr = lambda ts, k: None if ts is None or ts[k] is None else ts[k].data_ptr()  # noqa: E731
    for k, w in enumerate(widths):
        lr, eps, step = hyper[k] if hyper else (0.0, 1e-15, 1)
        arr[k] = L.GsRowTensor(ptr(p, k), ptr(m, k), ptr(v, k), ptr(g, k), lr, B1, B2, eps, w, step)
    return arr


def _alloc(n_floats, device, offset1, fill=None, gen=None):
    """n_floats fp32 on `device` (random, or `fill`); offset1: a view one element behind a 16-byte boundary (rows.hip takes any 4-byte-aligned pointer)"""
    src = torch.full((n_floats + 5,), float(fill)) if fill is not None else torch.randn(n_floats + 5, generator=gen)
    base = src.to(device)
    view = base[1:1 + n_floats] if offset1 else base[:n_floats]
    assert view.data_ptr() % 16 == (4 if offset1 and n_floats else 0) or not n_floats
    return view


def check_rows_pack_unpack(device, widths, n, offset1=False):
    L, lib = _lib()
    K, G = len(widths), sum(widths)
    gen = torch.Generator().manual_seed(1000 * G + n)
    n_padded = n + 37
    null_key = K // 2 if K > 1 else None                                  # a key without a gradient packs as zero columns
    grads = [None if k == null_key else _alloc(n * w, device, offset1, gen=gen).view(n, w) for k, w in enumerate(widths)]
    flat = _alloc(n_padded * G, device, offset1, fill=float("nan")).view(n_padded, G)
    L.check(lib.gs_pack_columns(K, _row_array(L, widths, g=grads), n, n_padded, flat.data_ptr(), _stream(device)))
    want = torch.cat([torch.zeros(n, w) if g is None else g.cpu() for g, w in zip(grads, widths)], dim=1)
    want = torch.cat([want, torch.zeros(n_padded - n, G)])
    assert _same_bits(flat, want), f"pack {widths} n = {n}"
    # n = 0 with padding: all zeros
    flat0 = _alloc(5 * G, device, offset1, fill=float("nan")).view(5, G)
    L.check(lib.gs_pack_columns(K, _row_array(L, widths, g=grads), 0, 5, flat0.data_ptr(), _stream(device)))
    assert _same_bits(flat0, torch.zeros(5, G)), f"pack {widths} n = 0"
    # unpack: every key equals its column block; the guard rows behind every tensor stay
    GUARD = 3
    src = _alloc(n * G, device, offset1, gen=gen).view(n, G)
    params = [_alloc((n + GUARD) * w, device, offset1, fill=-5.5).view(n + GUARD, w) for w in widths]
    L.check(lib.gs_unpack_columns(K, _row_array(L, widths, p=params), n, src.data_ptr(), _stream(device)))
    off = 0
    for p, w in zip(params, widths):
        assert _same_bits(p[:n], src[:, off:off + w].contiguous()), f"unpack {widths} n = {n}"
        assert bool((p[n:] == -5.5).all()), "unpack wrote behind row n"
        off += w


def rows_windows(n):
    """(row_lo, n_valid, n_rows) of the issue; the tensors hold enough rows for every window (check_rows_adam), and the last window is clamped
    for n < 3 (it is (n - 3, 3, 256) from n = 3 on)."""
    return ((0, n, n), (257, 300, 512), (5, 0, 64), (max(n - 3, 0), min(3, n), 256))


def check_rows_adam(device, widths, n, offset1=False, windows=None):
    L, lib = _lib()
    K, G = len(widths), sum(widths)
    windows = windows or rows_windows(n)
    # rows of every tensor: row_lo + n_rows of every window fits (a kernel that stepped the shard's padding rows would change rows of the
    # tensors, which the test then sees, instead of writing behind them), two more rows behind
    N = max([n] + [lo + rows for lo, _, rows in windows]) + 2
    gen = torch.Generator().manual_seed(77 * G + n)
    hyper = [((1e-4, 2.5e-3, 1e-3, 5e-2)[k % 4], (1e-15, 1e-8)[k % 2], (1, 2, 10, 1000, 100000)[k % 5]) for k in range(K)]
    for row_lo, n_valid, n_rows in windows:
        p0 = [torch.randn(N, w, generator=gen) for w in widths]
        m0 = [0.1 * torch.randn(N, w, generator=gen) for w in widths]
        v0 = [0.01 * torch.rand(N, w, generator=gen) for w in widths]
        shard0 = torch.randn(n_rows, G, generator=gen) * 10.0 ** torch.randint(-6, 2, (n_rows, 1), generator=gen).float()
        dev = lambda ts: [_alloc(N * w, device, offset1, fill=0.0).view(N, w).copy_(t.to(device)) for t, w in zip(ts, widths)]  # noqa: E731
        p, m, v = dev(p0), dev(m0), dev(v0)
        shard = _alloc(n_rows * G, device, offset1, fill=0.0).view(n_rows, G).copy_(shard0.to(device))
        out = _alloc(n_rows * G, device, offset1, fill=float("nan")).view(n_rows, G)
        arr = _row_array(L, widths, p=p, m=m, v=v, hyper=hyper)
        L.check(lib.gs_adam_rows(K, arr, row_lo, n_valid, n_rows, shard.data_ptr(), out.data_ptr(), _stream(device)))
        # out_shard = NULL is accepted and changes nothing about the step
        p2, m2, v2 = dev(p0), dev(m0), dev(v0)
        L.check(lib.gs_adam_rows(K, _row_array(L, widths, p=p2, m=m2, v=v2, hyper=hyper), row_lo, n_valid, n_rows, shard.data_ptr(), None, _stream(device)))
        sl = slice(row_lo, row_lo + n_valid)
        inside = torch.zeros(N, dtype=torch.bool); inside[sl] = True
        off, want_out = 0, torch.zeros(n_rows, G)
        tag = f"rows {widths} n={n} window=({row_lo},{n_valid},{n_rows})"
        for k, w in enumerate(widths):
            lr, eps, step = hyper[k]
            pk, mk, vk = p[k].cpu(), m[k].cpu(), v[k].cpu()
            assert _same_bits(pk, p2[k]) and _same_bits(mk, m2[k]) and _same_bits(vk, v2[k]), tag + ": out_shard = NULL changes the step"
            for got, was, q in ((pk, p0[k], "p"), (mk, m0[k], "m"), (vk, v0[k], "v")):
                assert torch.equal(_bits(got)[~inside], _bits(was)[~inside]), tag + f": key {k}: a row of {q} outside the window changed"
            if n_valid:
                before = tuple(t.reshape(-1).contiguous() for t in (p0[k][sl], shard0[:n_valid, off:off + w], m0[k][sl], v0[k][sl]))
                one = run_adam(device, "multi", before, lr, eps, step)
                got = (pk[sl].reshape(-1), mk[sl].reshape(-1), vk[sl].reshape(-1))
                assert all(_same_bits(x, y) for x, y in zip(got, one)), tag + f": key {k} differs from gs_adam_step_multi on those rows"
                r = adam_ratios(before, got, lr, eps, step)
                assert max(r.values()) <= SAFETY, tag + f": key {k} misses the one-step rule: {r}"
                want_out[:n_valid, off:off + w] = pk[sl]
            off += w
        assert _same_bits(out, want_out), tag + ": out_shard is not the updated rows followed by zero rows"


def check_rows_refusals(device):
    L, lib = _lib()
    t = lambda n, w: torch.zeros(n, w, device=device)  # noqa: E731
    flat = torch.zeros(16, 80, device=device)

    def pack(widths, n, n_padded):
        return lib.gs_pack_columns(len(widths), _row_array(L, widths, g=[t(max(n, 1), max(w, 1)) for w in widths]), n, n_padded, flat.data_ptr(), _stream(device))
    assert pack((64, 1), 4, 4) == 1, "G = 65 accepted"
    assert pack((1,) * 9, 4, 4) == 1, "nine keys accepted"
    assert pack((3, 0, 4), 4, 4) == 1, "width 0 accepted"
    assert pack((3, 4), 4, 3) == 1, "n_padded < n accepted"
    assert pack((3, 4), 4, 4) == 0
    widths = (3, 4)
    p, m, v = ([t(8, w) for w in widths] for _ in range(3))
    arr = _row_array(L, widths, p=p, m=m, v=v)
    assert lib.gs_adam_rows(2, arr, 0, 5, 4, flat.data_ptr(), None, _stream(device)) == 1, "n_rows < n_valid accepted"
    assert lib.gs_adam_rows(2, arr, 0, 4, 4, flat.data_ptr(), None, _stream(device)) == 0


# =====================================================================================================================================
# 4. Statistics and keyframe scoring
# =====================================================================================================================================
STATS_P = (0, 1, 255, 256, 257, 2 ** 20 + 3)


def check_visibility_stats(device, P):
    """seen = radius > 0 and max_2D_radius = fmaxf(max_2D_radius, radius), exact; a NaN already in max_2D_radius is REPLACED by the radius (fmaxf
    returns the operand that is a number; torch.maximum would keep the NaN)."""
    L, lib = _lib()
    gen = torch.Generator().manual_seed(P + 1)
    radii = torch.randint(-50, 400, (P,), generator=gen, dtype=torch.int32)
    special = torch.tensor([0, 1, 2 ** 24, -1, -2 ** 24, 2 ** 24 - 1, 0, 7], dtype=torch.int32)
    radii[: min(P, 8)] = special[: min(P, 8)]
    mx0 = (torch.rand(P, generator=gen) * 300 - 20).float()
    if P > 12:
        mx0[8:11] = float("nan")
        radii[9] = 0; radii[10] = -3
    want_seen = radii > 0
    rf = radii.double()                                                  # |radius| <= 2^24: exact in fp32 as well
    want_mx = torch.where(torch.isnan(mx0), rf.float(), torch.maximum(mx0, rf.float()))
    r_d, s = radii.to(device), _stream(device)
    for seen_null, mx_null in ((False, False), (True, False), (False, True)):
        seen = torch.full((P,), 7, dtype=torch.uint8, device=device)
        mx = mx0.clone().to(device)
        L.check(lib.gs_visibility_stats(P, r_d.data_ptr() if P else None, None if seen_null else seen.data_ptr(), None if mx_null else mx.data_ptr(), s))
        assert torch.equal(seen.cpu(), torch.full((P,), 7, dtype=torch.uint8) if seen_null else want_seen.to(torch.uint8)), "seen"
        assert _same_bits(mx, mx0 if mx_null else want_mx), "max_2D_radius"
    if P:
        assert lib.gs_visibility_stats(P, None, None, None, s) == 1


def check_fused_visibility_nan_rule(device):
    """The fused raw entry writes max_2D_radius by the same rule: a NaN in it is replaced by the radius of this render."""
    from activesplat_amd import rasterizer as R, synthetic as syn
    from activesplat_amd.camera import setup_camera
    W, H, n = 64, 48, 300
    p = {k: v.to(device).contiguous() for k, v in syn.make_params(n, W, H, seed=5).items()}
    rs = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=device)
    mx0 = torch.rand(n) * 30
    mx0[::3] = float("nan")
    mx, seen = mx0.clone().to(device), torch.zeros(n, dtype=torch.bool, device=device)
    out = R.render_rgbd_raw(rs, p["means3D"], torch.zeros_like(p["means3D"]), p["logit_opacities"], p["log_scales"], p["unnorm_rotations"],
                            [1.0, 0, 0, 0, 0, 0, 0], colors_precomp=p["rgb_colors"], visibility=(mx, seen))
    radii = out[1].cpu()
    assert int((radii > 0).sum()) > n // 4, "the scene of this test is not visible"
    assert torch.equal(seen.cpu(), radii > 0)
    assert _same_bits(mx, torch.where(torch.isnan(mx0), radii.float(), torch.maximum(mx0, radii.float())))


# accumulator rule: acc' = fl(acc + fl(sqrt(fl(gx^2 + gy^2)))).  gx^2 + gy^2 is off by at most 2 u of itself (each product u, the sum u; one
# contraction into an FMA only removes a rounding), the root halves that and adds its own u: 2 u ||g||.  The sum adds half an ulp of acc'.  One
# square may underflow by less than T: the root moves by at most T / ||g||.  ACCUM_C = 2 x SAFETY, in units of u.
ACCUM_C = 2 * SAFETY


def _ulp32(x):
    """ulp of the fp32 binade that holds |x| (float64 tensor in, float64 out); 2^-149 below the normals"""
    _, e = torch.frexp(x.abs().clamp_min(TINY))
    return torch.ldexp(torch.ones_like(x), e - 24)


def check_accumulate_grad2d(device, P):
    L, lib = _lib()
    gen = torch.Generator().manual_seed(3 * P + 2)
    mag = _log_uniform(P, 1e-18, 1e15, gen)
    ang = torch.rand(P, generator=gen, dtype=torch.float64) * 2 * math.pi
    grad = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang), torch.full((P,), float("nan"), dtype=torch.float64)], dim=1).float()
    seen = torch.rand(P, generator=gen) < 0.6
    acc0 = _log_uniform(P, 1e-20, 1e3, gen).float()
    den0 = torch.randint(0, 50, (P,), generator=gen).float()
    acc, den = acc0.clone().to(device), den0.clone().to(device)
    g_d, s_d = grad.to(device), seen.to(device)
    L.check(lib.gs_accumulate_grad2d(P, g_d.data_ptr() if P else None, s_d.data_ptr() if P else None, acc.data_ptr() if P else None,
                                     den.data_ptr() if P else None, _stream(device)))
    acc, den = acc.cpu(), den.cpu()
    assert torch.equal(den, den0 + seen.float()), "denom"
    assert torch.equal(_bits(acc)[~seen], _bits(acc0)[~seen]), "an unseen row changed"
    norm = (grad[:, 0].double() ** 2 + grad[:, 1].double() ** 2).sqrt()
    want = acc0.double() + norm
    bound = _ulp32(want) / 2 + ACCUM_C * U * norm + SAFETY * TINY / norm.clamp_min(1e-30)
    ratio = ((acc.double() - want).abs() / bound)[seen]
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _say("accumulate_grad2d", P=P, worst=worst)
    assert worst <= 1.0, f"accumulator error / bound = {worst:.3f} (a NaN from the third column shows as inf)"


# keyframe overlap: first-order bounds on the kernel's fp32 u, v, pz (a sum of n terms rounds by at most n u of the terms' magnitudes --
# products and sums, contracted or not -- a quotient by u of its value, the operands' bounds carried forward), times SAFETY.
OVERLAP_NPTS = (0, 1, 255, 256, 257, 100_003)
OVERLAP_KF = (1, 3, 64)


def overlap_inputs(n_pts, n_kf, seed=0):
    """world points in front of, behind and (about 1 %) within 1e-4 of the camera plane of keyframe 0, some NaN; w2c: small rotations about y
    and translations; intrinsics with skew 0."""
    gen = torch.Generator().manual_seed(31 * n_pts + n_kf + seed)
    pts = torch.rand(n_pts, 3, generator=gen, dtype=torch.float64) * torch.tensor([6.0, 4.0, 6.0]) - torch.tensor([3.0, 2.0, 2.0])
    w2c = torch.zeros(n_kf, 4, 4, dtype=torch.float64)
    for k in range(n_kf):
        a = 0.0 if k == 0 else float(torch.rand(1, generator=gen) - 0.5) * 1.2
        w2c[k] = torch.tensor([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]], dtype=torch.float64)
        if k:
            w2c[k, :3, 3] = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 0.8
    if n_pts >= 200:
        near = torch.arange(0, n_pts, 97)
        pts[near, 2] = (torch.rand(near.numel(), generator=gen, dtype=torch.float64) - 0.5) * 2e-4      # pz of keyframe 0 within 1e-4 of 0
        pts[torch.arange(5, n_pts, 501)] = float("nan")
        pts[torch.arange(6, n_pts, 1001), 1] = float("nan")
    return pts.float(), w2c.float()


def overlap_reference(pts, w2c, K, W, H, edge):
    """-> sure [n_kf], ambiguous [n_kf] (int64) from a float64 projection of the fp32 inputs."""
    P, M, Kd = pts.double(), w2c.double(), torch.tensor(K, dtype=torch.float64).reshape(3, 3)
    k32 = Kd.float().double()
    X = P[None, :, :]                                                     # [1, n, 3]
    cam, e_cam = [], []
    for r in range(3):
        terms = M[:, None, r, :3] * X                                     # [kf, n, 3]
        cam.append(terms.sum(-1) + M[:, None, r, 3])
        e_cam.append(4 * U * (terms.abs().sum(-1) + M[:, None, r, 3].abs()))
    img, e_img = [], []
    for r in range(3):
        terms = torch.stack([k32[r, c] * cam[c] for c in range(3)], -1)
        img.append(terms.sum(-1))
        e_img.append(sum(k32[r, c].abs() * e_cam[c] for c in range(3)) + 4 * U * terms.abs().sum(-1))
    pz = img[2] + 1e-5
    e_pz = e_img[2] + U * pz.abs() + U * 1e-5
    u, v = img[0] / pz, img[1] / pz
    e_u = (e_img[0] + u.abs() * e_pz) / pz.abs() + U * u.abs()
    e_v = (e_img[1] + v.abs() * e_pz) / pz.abs() + U * v.abs()
    e_u, e_v, e_pz = SAFETY * e_u, SAFETY * e_v, SAFETY * e_pz
    lo, hi_u, hi_v = float(edge), float(W - edge), float(H - edge)
    inside = (u < hi_u) & (u > lo) & (v < hi_v) & (v > lo) & (pz > 0)
    amb = ((u - lo).abs() <= e_u) | ((u - hi_u).abs() <= e_u) | ((v - lo).abs() <= e_v) | ((v - hi_v).abs() <= e_v) | (pz.abs() <= e_pz)
    return (inside & ~amb).sum(1), amb.sum(1), amb


def check_keyframe_overlap(device, n_pts, n_kf, edge=20, W=640, H=480):
    L, lib = _lib()
    pts, w2c = overlap_inputs(n_pts, n_kf)
    K = [500.0, 0.0, 319.5, 0.0, 480.0, 239.5, 0.0, 0.0, 1.0]
    sure, amb, amb_mask = overlap_reference(pts, w2c, K, W, H, edge)
    pairs = max(n_pts * n_kf, 1)
    frac = float(amb.sum()) / pairs
    if n_pts >= 255:
        assert frac <= 0.005, f"{frac:.4%} of the (point, keyframe) pairs are ambiguous: the inputs of this test do not decide enough"
    counts = torch.full((n_kf,), 0xFFFFFF, dtype=torch.int32, device=device)
    p_d, m_d = pts.to(device), w2c.contiguous().to(device)
    k9 = (C.c_float * 9)(*K)
    L.check(lib.gs_keyframe_overlap(n_pts, p_d.data_ptr() if n_pts else None, n_kf, m_d.data_ptr(), k9, W, H, edge, counts.data_ptr(), _stream(device)))
    got = counts.cpu().long()
    _say("keyframe_overlap", n_pts=n_pts, n_kf=n_kf, edge=edge, W=W, ambiguous=int(amb.sum()), ambiguous_frac=frac, counted=int(got.sum()), sure=int(sure.sum()))
    assert bool(((got >= sure) & (got <= sure + amb)).all()), f"counts {got.tolist()} outside [sure, sure + ambiguous] = {sure.tolist()} + {amb.tolist()}"
    if W - edge <= edge:
        assert int(got.sum()) == 0 and int(sure.sum()) == 0
    elif n_pts >= 255 and W >= 640:
        assert int(sure[0]) > n_pts // 20, "keyframe 0 sees too few points for this test to mean anything"
    return got
