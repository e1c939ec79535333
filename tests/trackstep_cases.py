"""Shared cases of the tracking tail -- gs_tracking_step (tracking_step_kernel, activate.hip), the pose-gradient finish it shares with bundle
adjustment (pose_grad_finish_block, gs_common.h), the per-workgroup pose rows (pose_grad_accumulate / pose_grad_block_row) and the loss rows
(tracking_loss_kernel's rows, tracking_loss_reduce) -- against references restated HERE: torch / numpy float64, or numpy float32 where the
kernel's fp32 sequence is held to the bit.  No reference calls the library or activesplat_amd.mapping.  Run twice: tests/test_trackstep_fp64.py
on the host-emulated kernels, tests/test_gpu_trackstep_fp64.py on the device.  Every input is a synthetic row buffer or a few thousand
Gaussians: no rasteriser is involved.  u = 2^-24 throughout.

A. Row reduction and the dL/dR -> dL/dq chain.  Two ways in: (1) gs_tracking_step with injected pose rows (the finish at the device column, then
   F.normalize's Jacobian; the gradient is read from the moments of step 1: state[0:7] = fl(c1 grad), c1 = fl32(1 - 0.9), so grad = state / c1
   to within u relative, and state[7:14] = fl(c2 fl(grad^2)) gives the sign-free part again); (2) gs_activate_backward_pose on an isotropic map
   with integer means3D / g_means3D in [-8, 8]: every product and fp32 partial sum is exact, so the rows and the t[16] the finish sees are
   known integers (pose_grad_finish_kernel at a host pose; dL_dpose7 is read directly).  The injected rows hold dyadic values (integers in
   +-2^12, / 2^6): their fp64 sums are exact in any order, so no reference depends on the reduction order, and every row and slice has its own
   random values: a row added twice, skipped or swapped changes the sum.
     Tier 1, against the chain at the kernel's own normalised column.  normalize_pose_column is ((a^2 + b^2) + c^2) + d^2, sqrtf, division by
   max(norm, 1e-12f), nothing contracted: numpy float32 repeats it to the bit.  The reference is float64 autograd through build_rotation at that
   column, then the Jacobian (G - u (u.G)) / n, or G / 1e-12 below the clamp.  The kernel does all of that in double and rounds ONCE, so
       |grad_k - ref_k| <= u |ref_k|  (the output rounding)  +  u |ref_k|  (the read-out through the moment; entry (2) has none)  +  2^-45 S,
   S = (max |t[12:16]| + 8 max |dR| / |q|) / n the size of the terms a component is formed from (|q| = the norm of the quaternion the finish
   receives, n = the column's norm, or 1e-12 on the clamp branch; entry (2): no n).  2^-45 S: the double chain and the float64 reference are
   each under a hundred operations of relative error 2^-53 on terms no larger than ~1.4 S: 2 x 100 x 1.4 x 2^-53 < 2^-45.  A component that
   cancels to near zero is held to 2^-45 S, i.e. to the last bit of the LARGEST term: any wrong coefficient shows.
     Tier 2, against the pure float64 chain from the fp32 column (float64 F.normalize -> build_rotation -> autograd): bound C u S, C = 64,
   counted from the roundings of normalize_pose_column.  The four squares (u each) and three adds (u each) of positive terms leave the sum of
   squares within 4 u, the root within 2 u + u of its own rounding = 3 u (the norm n), each quotient within 3 u + u = 4 u: the computed column
   is u~ = u + du, |du|_2 <= 4 u, and n~ = n (1 + 3 u).  With f(q) = <dR, R(q / |q|)> = q^T M q / q^T q, |M|_2 <= sqrt(3) |dR|_F <= 5.2 D
   (D = max |dR|), the gradient G_R = 2 (M - f) q has |G_R|_2 <= lambda_max - lambda_min <= 10.4 D and the Hessian 2 (M - f) - 2 (q G_R^T +
   G_R q^T) has norm <= 20.8 D + 41.6 D = 62.4 D; |G|_2 <= 10.4 D + 2 T (T = max |t[12:16]|) <= 2 (8 D + T).  To first order:
       the norm in the Jacobian:            3 u |ref|              <= 3 u x 2 S        =  6 u S
       du in the projector u (u.G):         2 x 4 u |G| / n        <= 8 u x 2 S        = 16 u S
       du in G_R:                           4 u x 62.4 D / n       <= 4 u x 7.8 S      = 31.2 u S
       tier 1 itself:                                                                     2 u S
   together 55.2 u S, rounded up to the next power of two for the second-order terms.  (On the clamp branch the column is divided by fl32(1e-12),
   off by 0.67 u, once: fewer roundings, same bound.)  This tier catches a wrong normalisation; tier 1 everything behind it.
     The all-zero column has no finite reference: its expected outcome is what the same chain gives in fp32 torch (NaN where that is NaN).

B. Per-Gaussian shares (pose_grad_accumulate) and the workgroup row (pose_grad_block_row): gs_activate_backward_pose on an anisotropic map
   with ONE live row (every other row: zero gradients, NaN means, NaN or zero quaternions -- the header promises they add nothing), in both
   pose_only modes.  Reference: float64 autograd of R(q/|q|) w + t and normalize(quat_mult(q_cam, normalize(q_i))).  Rule (check_activate's):
   error / scale of the kernel <= max(2 x that of an fp32 torch mirror of the same formula, 1e-6) for the worst case and <= max(2 x, 8 u) for
   the mean over the cases; scale = max(largest |ref|, |g_rot| / max(|q_i|, 1), |g_mean| |w|) (the rotation share is L(u_i)^T (g - r (r.g)) /
   |q_cam (x) u_i| with |u_i| = 1: it does not grow with 1 / |q_i| for a small q_i, so the term scale stated for the PARAMETER gradient,
   |g_rot| / |q_i|, is used only where it is the smaller one).  The translation components are the live row's g_means3D to the bit.  Dense
   cases (every row live) are held per component against the float64 sum, scale = the sum of the rows' term scales (quaternion) or of the
   |g_means3D| (translation), floor 8 u, the mirror summing fp32 shares in fp32 in index order.

C. Loss rows.  Injected rows on the grid 2^-10 (magnitudes 1e-3 .. 1e4, all distinct; fp64 sums exact): wd = fl(fl32(S0) w_depth), wc =
   fl(fl32(S1) w_im), loss = fl(wd + wc) in numpy float32, to the bit in state[22:25] and history_row[0:3].  Real rows of gs_tracking_loss: row r
   against the float64 sum over its own 256 pixels, bound (6 + 3 + 1) u sum |terms| (six butterfly levels, three adds of the four wave sums, the
   term's own rounding).  The colour term adds its three channels inside the thread first, two more roundings, so its worst case is 12 u; the
   10 u stated for both is asserted for both: random roundings of up to 768 terms stay far below either (worst row: 0.2 of it).

D. The Adam step.  The kernel's sequence (torch's foreach order), every operation rounded to fp32, none contracted:
       m' = m + c1 (g - m)        v1 = v b2        v' = v1 + c2 (g g)        den = sqrt(v') / k + e        p' = p + s (m' / den)
   c1 = fl(1 - 0.9), b2 = fl(0.999), c2 = fl(1 - 0.999), k = fl(sqrt(1 - 0.999^t)), e = fl(1e-8), s = fl(-(lr / (1 - 0.9^t))), formed in double
   and rounded once.  Held to the bit in numpy float32 wherever the gradient is exact (translation: always; quaternion: a column (c, 0, 0, 0),
   c a power of two).  Elsewhere the one-step rule of optimstep_cases.py, re-derived for this order -- the division by a rounded k costs what
   the product with a rounded 1 / k costs there (constant, root, quotient: 3 u), every other term is the same:
       E_m = u (3 |c1 (g - m)| + |m'|) + 4 T + c1 E_g
       E_v = u (2 b2 v + 3 c2 g^2 + v') + 4 T + c2 (2 |g| E_g + E_g^2)
       E_den = d_sqrt / k + 3 u sqrt(v') / k + u e + u den,   d_sqrt = sqrt(v') - sqrt(max(v' - E_v, 0))
       E_p = E_m |s| / den + |upd| (E_den / den + 3 u) + u |p'| + 4 T
   with E_g the gradient's own allowance from A (tier 1 without the read-out: u |g| + 2^-45 S) taken to first order through the step (exactly,
   for g^2), T = 2^-126 and SAFETY = 2 on all three as there.  Not fitted: the numpy float32 mirror fed the float64 gradient rounded to fp32
   must lie inside on the same input sets (check_adam_evolution with kernel=False).

E. The candidate rule (strict <, start fl32(1e20): the first minimum wins, a NaN never does) replayed on the host from the history rows.

Not covered, deliberately: pose_grad_finish_dev_kernel (reached only through a render: tracking_cases.check_device_pose_matches_host_pose holds
it to the host-pose finish) and the skip branch of the step (chain_failed: needs a provoked walk timeout).

Every check prints the figures it asserts on and appends them to REPORT (profiles/README.md holds the device's)."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

REPORT = []
U = 2.0 ** -24            # unit roundoff of float32
TINY = 2.0 ** -126        # smallest normal float32
SAFETY = 2.0              # of the one-step Adam rule (optimstep_cases.py)
SLACK = 2.0 ** -45        # fp64 slack of tier 1, in units of S (module docstring)
C_TIER2 = 64.0            # counted in the module docstring
B1, B2, EPS = 0.9, 0.999, 1e-8
f32 = np.float32


def _say(section, **kw):
    REPORT.append(dict(section=section, **kw))
    print(section, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _L():
    from activesplat_amd import _lib as L
    return L, L.get()


def _stream(device):
    from activesplat_amd import _lib as L
    return L.stream_ptr(torch.device(device))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_bits_or_nan(a, b):
    """the same bits, or a NaN in both (a NaN's payload and sign are not the kernel's to keep)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and _same_bits(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


CANARY = (-7.25, 3.5e10, 1e-30, 77.0)


def _canary(n):
    return torch.tensor(CANARY, dtype=torch.float32).repeat(n // 4 + 1)[:n].clone()


# =====================================================================================================================================
# The references
# =====================================================================================================================================
def normalize_column32(x):
    """normalize_pose_column in numpy float32 -> (u[4], norm): one correctly rounded IEEE operation per step, in the kernel's order."""
    a, b, c, d = (f32(v) for v in x)
    with np.errstate(all="ignore"):
        norm = np.sqrt(((a * a + b * b) + c * c) + d * d)
        n = max(norm, f32(1e-12))
        u = np.array([a / n, b / n, c / n, d / n], dtype=np.float32)
    assert norm.dtype == np.float32
    return u, norm


def _rotation(q):
    """quat_to_rot's formula (w first), row-major [9]; any dtype."""
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1)


def _build_rotation(q):
    """slam_external.py's build_rotation: the formula at q / |q| (plain square root of the sum of squares, no clamp)."""
    return _rotation(q / torch.sqrt((q * q).sum(-1, keepdim=True)))


def _quat_mult(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def finish_reference64(q, t16):
    """pose_grad_finish_block's result in float64: q = the quaternion the finish receives (float64 [4]), t16 = the exact column sums (float64
    [16]: dL/dt, dL/dR row-major, the rotation term) -> [7] = dL/d(qw..qz) by autograd through build_rotation, + the rotation term as is; dL/dt."""
    x = q.clone().requires_grad_(True)
    (t16[3:12] * _build_rotation(x)).sum().backward()
    return torch.cat([x.grad + t16[12:16], t16[0:3]])


def _scale(t16, nq, den):
    return (float(t16[12:16].abs().max()) + 8.0 * float(t16[3:12].abs().max()) / nq) / den


def step_gradient_tier1(col, t16):
    """-> (grad[7] float64, S): the step's gradient evaluated in float64 at the fp32 normalised column the kernel forms."""
    u32, n32 = normalize_column32(col)
    u, n = torch.tensor(u32.astype(np.float64)), float(n32)
    G = finish_reference64(u, t16)
    den = n if n >= 1e-12 else 1e-12
    gq = (G[:4] - u * (u * G[:4]).sum()) / n if n >= 1e-12 else G[:4] / 1e-12
    return torch.cat([gq, G[4:]]), _scale(t16, float(u.norm()), den)


def step_gradient_tier2(col, t16):
    """-> grad[7]: float64 autograd from the fp32 column through F.normalize and build_rotation."""
    x = torch.tensor(np.asarray(col, dtype=np.float32).astype(np.float64), requires_grad=True)
    uq = F.normalize(x, dim=0)
    ((t16[3:12] * _build_rotation(uq)).sum() + (t16[12:16] * uq).sum()).backward()
    return torch.cat([x.grad, t16[0:3]])


def step_gradient_fp32_torch(col, t16):
    """The same chain in fp32 torch autograd: the expected outcome of the all-zero column."""
    x = torch.tensor(np.asarray(col, dtype=np.float32), requires_grad=True)
    t = t16.float()
    uq = F.normalize(x, dim=0)
    ((t[3:12] * _build_rotation(uq)).sum() + (t[12:16] * uq).sum()).backward()
    return torch.cat([x.grad, t[0:3]])


def adam_constants(lr_rot, lr_trans, step):
    """gs_tracking_step's constants: formed in double, rounded once."""
    bc1, bc2 = 1.0 - math.pow(B1, float(step)), 1.0 - math.pow(B2, float(step))
    return dict(c1=f32(1.0 - B1), b2=f32(B2), c2=f32(1.0 - B2), k=f32(math.pow(bc2, 0.5)), e=f32(EPS),
                s=np.array([f32(-(lr_rot / bc1))] * 4 + [f32(-(lr_trans / bc1))] * 3, dtype=np.float32))


def adam_mirror32(p, g, m, v, lr_rot, lr_trans, step):
    """The kernel's sequence on float32 numpy arrays [7] -> p', m', v'."""
    c = adam_constants(lr_rot, lr_trans, step)
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = m + c["c1"] * (g - m)
        v1 = v * c["b2"]
        v1 = v1 + c["c2"] * (g * g)
        den = np.sqrt(v1) / c["k"] + c["e"]
        p1 = p + c["s"] * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def adam_reference64(p, g, m, v, lr_rot, lr_trans, step):
    """torch.optim.Adam's single-tensor step in float64 (numpy) -> m', v', upd, p', den, |s|."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    s = np.array([lr_rot / bc1] * 4 + [lr_trans / bc1] * 3)
    m1 = m + (1.0 - B1) * (g - m)
    v1 = B2 * v + (1.0 - B2) * g * g
    den = np.sqrt(v1) / math.sqrt(bc2) + EPS
    upd = s * m1 / den
    return m1, v1, upd, p - upd, den, s


def adam_bounds(p, g, m, v, e_g, lr_rot, lr_trans, step):
    """-> (E_m, E_v, E_p) of the module docstring (float64 [7], without SAFETY); e_g = the allowance of the gradient itself."""
    m1, v1, upd, p1, den, s = adam_reference64(p, g, m, v, lr_rot, lr_trans, step)
    g, m, v = (np.asarray(a, dtype=np.float64) for a in (g, m, v))
    k = math.sqrt(1.0 - B2 ** step)
    e_m = U * (3 * np.abs((1 - B1) * (g - m)) + np.abs(m1)) + 4 * TINY + (1 - B1) * e_g
    e_v = U * (2 * B2 * v + 3 * (1 - B2) * g * g + v1) + 4 * TINY + (1 - B2) * (2 * np.abs(g) * e_g + e_g * e_g)
    sq = np.sqrt(v1)
    d_sqrt = sq - np.sqrt(np.maximum(v1 - e_v, 0.0))
    e_den = d_sqrt / k + 3 * U * sq / k + U * EPS + U * den
    e_p = e_m * s / den + np.abs(upd) * (e_den / den + 3 * U) + U * np.abs(p1) + 4 * TINY
    return e_m, e_v, e_p


def adam_ratios(before, after, e_g, lr_rot, lr_trans, step):
    """worst |got - float64| / E per quantity over the seven values; before = (p, g64, m, v), after = (p', m', v')."""
    p, g, m, v = before
    m1, v1, _, p1, _, _ = adam_reference64(p, g, m, v, lr_rot, lr_trans, step)
    e_m, e_v, e_p = adam_bounds(p, g, m, v, e_g, lr_rot, lr_trans, step)
    out = {}
    for name, got, ref, e in (("p", after[0], p1, e_p), ("m", after[1], m1, e_m), ("v", after[2], v1, e_v)):
        r = np.abs(np.asarray(got, dtype=np.float64) - ref) / e
        out[name] = float(np.where(np.isnan(r), np.inf, r).max())
    return out


# =====================================================================================================================================
# Driving the kernels
# =====================================================================================================================================
MARGIN = 16


class Track:
    """cam_unnorm_rots [1,4,T] and cam_trans [1,3,T] inside canary margins, and the 32-float state, on `device`."""

    def __init__(self, device, rots, trans, t):
        L, lib = _L()
        self.L, self.lib, self.dev, self.t, self.T = L, lib, torch.device(device), t, int(rots.shape[-1])
        T = self.T
        self.rbuf, self.tbuf = _canary(4 * T + 2 * MARGIN), _canary(3 * T + 2 * MARGIN)
        self.rbuf[MARGIN:MARGIN + 4 * T] = rots.reshape(-1).float()
        self.tbuf[MARGIN:MARGIN + 3 * T] = trans.reshape(-1).float()
        self.r0, self.t0 = self.rbuf.clone(), self.tbuf.clone()
        self.rbuf, self.tbuf = self.rbuf.to(self.dev), self.tbuf.to(self.dev)
        assert int(lib.gs_tracking_state_bytes()) >= 32 * 4
        self.state = _canary(int(lib.gs_tracking_state_bytes()) // 4).to(self.dev)
        self.hist = torch.full((10,), float("nan"), device=self.dev)
        self.st = _stream(device)

    def _ptrs(self):
        return self.rbuf.data_ptr() + 4 * MARGIN, self.tbuf.data_ptr() + 4 * MARGIN

    def begin(self):
        r, t = self._ptrs()
        self.L.check(self.lib.gs_tracking_begin(r, t, self.T, self.t, self.state.data_ptr(), self.st))

    def step(self, P, pose_rows, W, H, loss_rows, w_im, w_depth, lr_rot, lr_trans, k, history=True):
        r, t = self._ptrs()
        self.L.check(self.lib.gs_tracking_step(P, pose_rows.data_ptr(), W, H, loss_rows.data_ptr(), w_im, w_depth, r, t, self.T, self.t,
                                               lr_rot, lr_trans, k, self.state.data_ptr(), self.hist.data_ptr() if history else None, self.st))
        return self.hist.cpu() if history else None

    def column(self):
        """the seven values of column t as they stand in memory (float32 CPU)."""
        T, t = self.T, self.t
        r, tr = self.rbuf.cpu()[MARGIN:MARGIN + 4 * T].view(4, T), self.tbuf.cpu()[MARGIN:MARGIN + 3 * T].view(3, T)
        return torch.cat([r[:, t], tr[:, t]])

    def assert_rest_untouched(self):
        """every other column and both margins of both tensors hold their first bits."""
        T, t = self.T, self.t
        for buf, first, rows in ((self.rbuf, self.r0, 4), (self.tbuf, self.t0, 3)):
            keep = torch.ones(rows * T + 2 * MARGIN, dtype=torch.bool)
            keep[MARGIN + t:MARGIN + rows * T:T] = False
            assert int((~keep).sum()) == rows
            assert torch.equal(_bits(buf)[keep], _bits(first)[keep]), "the step wrote outside its column"


def pose_scratch(device, rows):
    """rows [nrows,16] float32 -> (P-independent) scratch of gs_pose_grad_scratch_bytes with NaN behind the last row."""
    _, lib = _L()
    nrows = int(rows.shape[0])
    buf = torch.full((int(lib.gs_pose_grad_scratch_bytes(256 * nrows)) // 4,), float("nan"))
    assert buf.numel() >= 16 * nrows
    buf[:16 * nrows] = rows.reshape(-1)
    return buf.to(device)


def dyadic_rows(nrows, seed, scale=64.0, top=4096):
    """[nrows,16] float32: integers in +-top over `scale`; their float64 sums are exact in any order."""
    g = torch.Generator().manual_seed(7919 * seed + nrows)
    return (torch.randint(-top, top + 1, (nrows, 16), generator=g).double() / scale).float()


def one_loss_row(device, d=1.0, c=1.0):
    """the loss rows of a 16 x 16 image: one row {depth sum, colour sum}."""
    _, lib = _L()
    buf = torch.full((int(lib.gs_tracking_loss_scratch_bytes(16, 16)) // 4,), float("nan"))
    buf[0], buf[1] = d, c
    return buf.to(device)


def nrows_of(P):
    return (P + 255) // 256


# =====================================================================================================================================
# A. Row reduction and the dL/dR -> dL/dq chain
# =====================================================================================================================================
STEP_P = (1, 256, 257, 3840, 4096, 4097, 8192, 8193, 65537)          # 1, 1, 2, 15, 16, 17, 32, 33, 257 rows
_GEN = np.array([0.3, -1.2, 0.5, 0.8])
_F1E12 = float(f32(1e-12))
COLUMNS = {
    "identity x 1.7": (1.7, 0.0, 0.0, 0.0),
    "general": tuple(_GEN),
    "general 2": (-0.7, 0.4, 1.9, -0.2),
    "norm 1e-3": tuple(_GEN / np.linalg.norm(_GEN) * 1e-3),
    "norm 1e3": tuple(_GEN / np.linalg.norm(_GEN) * 1e3),
    "turn about x": (0.0, 1.3, 0.0, 0.0),
    "turn about y": (0.0, 0.0, 3.0, 0.0),
    "turn about z": (0.0, 0.0, 0.0, 0.7),
    "near identity": (0.9994, 0.02, -0.021, 0.019),
    "norm 1e-15, w only": (1e-15, 0.0, 0.0, 0.0),
    "norm 1e-15, general": tuple(_GEN / np.linalg.norm(_GEN) * 1e-15),
    "norm fl32(1e-12): below the double 1e-12, clamped": (_F1E12, 0.0, 0.0, 0.0),
    "norm one ulp above fl32(1e-12): not clamped": (float(np.nextafter(f32(1e-12), f32(1))), 0.0, 0.0, 0.0),
}
LR_ROT, LR_TRANS = 1e-3, 4e-3


def first_step(device, P, col, rows, T=3, t=1):
    """gs_tracking_begin + step 1 on the injected rows -> (grad read from the first moments, grad^2 from the second, state) float64 / CPU."""
    rots, trans = torch.zeros(1, 4, T), torch.zeros(1, 3, T)
    rots[0, :, t] = torch.tensor(np.asarray(col, dtype=np.float32))
    rots[0, 0, [i for i in range(T) if i != t]] = 1.0
    trk = Track(device, rots, trans, t)
    trk.begin()
    trk.step(P, pose_scratch(device, rows), 16, 16, one_loss_row(device), 0.5, 1.0, LR_ROT, LR_TRANS, 1)
    st = trk.state.cpu()
    trk.assert_rest_untouched()
    c = adam_constants(LR_ROT, LR_TRANS, 1)
    return st[0:7].double() / float(c["c1"]), st[7:14].double() / float(c["c2"]), st


def check_finish_through_step(device, P):
    nrows = nrows_of(P)
    worst = dict(tier1=0.0, tier2=0.0, square=0.0)
    where = dict(tier1="", tier2="")
    for name, col in COLUMNS.items():
        for seed in (0, 1):
            rows = dyadic_rows(nrows, seed)
            t16 = rows.double().sum(0)
            got, got_sq, _ = first_step(device, P, col, rows)
            ref1, S = step_gradient_tier1(col, t16)
            ref2 = step_gradient_tier2(col, t16)
            assert torch.isfinite(got).all() and torch.isfinite(ref1).all() and torch.isfinite(ref2).all(), (name, got, ref1, ref2)
            # the translation: the exact sums (integers / 64 below 2^24 / 64: fp32 holds them), read through the moment: u relative
            assert torch.equal(ref1[4:], t16[0:3]) and bool(((got - ref1).abs() <= U * ref1.abs())[4:].all()), (name, P, got[4:], t16[0:3])
            r1 = float(((got - ref1).abs() / (2 * U * ref1.abs() + SLACK * S))[:4].max())
            r2 = float(((got - ref2).abs() / (C_TIER2 * U * S))[:4].max())
            # the second moment: fl(c2 fl(g^2)) against (m / c1)^2 -- three roundings against two: 4 u + O(u^2), where g^2 stays normal
            sq = got * got
            ok = (sq < 1e37) & (sq > 1e-30)
            rs = float(((got_sq - sq).abs() / ((4 * U + 16 * U * U) * sq))[ok].max()) if bool(ok.any()) else 0.0
            for key, r in (("tier1", r1), ("tier2", r2)):
                if r > worst[key]:
                    worst[key], where[key] = r, f"{name}/seed {seed}"
            worst["square"] = max(worst["square"], rs)
    _say("finish/step", P=P, rows=nrows, tier1=worst["tier1"], tier1_at=where["tier1"], tier2=worst["tier2"], tier2_at=where["tier2"],
         square=worst["square"])
    assert worst["tier1"] <= 1, f"tier 1 (the chain at the kernel's own column): error / bound = {worst['tier1']:.3f} at {where['tier1']}"
    assert worst["tier2"] <= 1, f"tier 2 (float64 from the fp32 column): error / bound = {worst['tier2']:.3f} at {where['tier2']}"
    assert worst["square"] <= 1, f"second moments against the squares of the first: {worst['square']:.3f}"
    return worst


def check_zero_column(device, P=4097):
    """The all-zero column: whatever the fp32 torch chain gives, NaN where that gives NaN."""
    rows = dyadic_rows(nrows_of(P), 5)
    t16 = rows.double().sum(0)
    got, _, st = first_step(device, P, (0.0, 0.0, 0.0, 0.0), rows)
    want = step_gradient_fp32_torch((0.0, 0.0, 0.0, 0.0), t16).double()
    _say("finish/zero-column", kernel=str([float(x) for x in got]), fp32_torch=str([float(x) for x in want]))
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (got, want)
    fin = ~torch.isnan(want)
    assert bool(((got - want).abs() <= U * want.abs())[fin].all()), (got, want)          # (read through the moment: u relative)


def unit32(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).astype(np.float32)


UNIT_POSES = {
    "identity": unit32((1, 0, 0, 0)), "general": unit32(_GEN), "general 2": unit32((-0.7, 0.4, 1.9, -0.2)),
    "turn about x": unit32((0, 1, 0, 0)), "turn about y": unit32((0, 0, 1, 0)), "turn about z": unit32((0, 0, 0, -1)),
    "near identity": unit32((0.9994, 0.02, -0.021, 0.019)),
}
ACT_P = (1, 256, 257, 4097, 8193, 65537)


def run_backward_pose(device, iso, pose7, means, rots, g_means, g_rots, pose_only):
    """gs_activate_backward_pose -> dL_dpose7 (CPU); the scratch is NaN-filled in front of the call."""
    L, lib = _L()
    P = int(means.shape[0])
    dev = torch.device(device)
    on = lambda x: None if x is None else x.contiguous().to(dev)  # noqa: E731
    means, rots, g_means, g_rots = on(means), on(rots), on(g_means), on(g_rots)
    pscr = torch.full((int(lib.gs_pose_grad_scratch_bytes(P)) // 4,), float("nan"), device=dev)
    out = torch.full((7,), float("nan"), device=dev)
    pose = (C.c_float * 7)(*[float(x) for x in pose7])
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    if pose_only:
        extra = [None] * 6
        keep = []
    else:
        keep = [torch.rand(P, 1).to(dev), torch.rand(P, 3).to(dev), torch.empty(P, 3, device=dev), torch.empty(P, 4, device=dev),
                torch.empty(P, 1, device=dev), torch.empty(P, 1 if iso else 3, device=dev)]
        extra = [x.data_ptr() for x in keep]
    L.check(lib.gs_activate_backward_pose(P, iso, pose, ptr(means), ptr(rots), extra[0], extra[1], ptr(g_means), ptr(g_rots), None, None,
                                          extra[2], extra[3], extra[4], extra[5], 0, 1 if pose_only else 0, out.data_ptr(), pscr.data_ptr(),
                                          _stream(device)))
    rows = pscr.cpu()[:16 * nrows_of(P)].view(-1, 16)
    return out.cpu(), rows


def check_finish_through_activate(device, P):
    """Entry (2): an isotropic map with integer means and mean gradients: the rows are exact integers."""
    worst, at = 0.0, ""
    for seed in (0, 1):
        g = torch.Generator().manual_seed(101 * seed + P)
        means = torch.randint(-8, 9, (P, 3), generator=g).float()
        gm = torch.randint(-8, 9, (P, 3), generator=g).float()
        rots = torch.randn(P, 4, generator=g)
        t16 = torch.zeros(16, dtype=torch.float64)
        t16[0:3] = gm.double().sum(0)
        t16[3:12] = (gm.double()[:, :, None] * means.double()[:, None, :]).sum(0).reshape(9)
        for name, q in UNIT_POSES.items():
            pose7 = list(q) + [0.25, -0.5, 0.125]
            got, rows = run_backward_pose(device, 1, pose7, means, rots, gm, None, True)
            # the rows themselves: exact integer sums of each workgroup's 256 Gaussians
            for r in range(rows.shape[0]):
                a, b = gm.double()[256 * r:256 * r + 256], means.double()[256 * r:256 * r + 256]
                want = torch.cat([a.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(9), torch.zeros(4, dtype=torch.float64)])
                assert torch.equal(rows[r].double(), want), (P, name, r, rows[r], want)
            qd = torch.tensor(q.astype(np.float64))
            ref = finish_reference64(qd, t16)
            S = _scale(t16, float(qd.norm()), 1.0)
            assert torch.equal(got[4:].double(), t16[0:3]), (P, name, got[4:], t16[0:3])
            r1 = float(((got.double() - ref).abs() / (U * ref.abs() + SLACK * S))[:4].max()) if S > 0 else float((got[:4] != 0).any())
            if r1 > worst:
                worst, at = r1, f"{name}/seed {seed}"
    _say("finish/activate", P=P, rows=nrows_of(P), tier1=worst, at=at)
    assert worst <= 1, f"pose_grad_finish_kernel at a host pose: error / bound = {worst:.3f} at {at}"
    return worst


# =====================================================================================================================================
# B. Per-Gaussian shares and the workgroup row
# =====================================================================================================================================
SHARE_P = (1, 257, 4097)
SHARE_KINDS = ("plain", "zero_q", "tiny_q", "parallel", "far")


def share_chain(qc, tr, w, q, gm, gr, iso):
    """sum over the rows of g_mean . (R(q_cam / |q_cam|) w + t) + g_rot . normalize(quat_mult(q_cam, normalize(q_i))); qc [P,4], tr [P,3]: one
    copy of the pose per row, so that autograd returns every row's own share.  Any dtype."""
    R = _build_rotation(qc).reshape(-1, 3, 3)
    L = (((R @ w[:, :, None])[:, :, 0] + tr) * gm).sum()
    if not iso:
        L = L + (F.normalize(_quat_mult(qc, F.normalize(q, dim=1)), dim=1) * gr).sum()
    return L


def shares(pose7, w, q, gm, gr, iso, dtype):
    """-> [P,7] every row's share of dL_dpose7 in `dtype` (autograd of share_chain on the `dtype` images of the fp32 inputs)."""
    P = w.shape[0]
    p = torch.tensor(np.asarray(pose7, dtype=np.float32)).to(dtype)
    qc, tr = p[:4].expand(P, 4).clone().requires_grad_(True), p[4:].expand(P, 3).clone().requires_grad_(True)
    share_chain(qc, tr, w.to(dtype), q.to(dtype), gm.to(dtype), gr.to(dtype), iso).backward()
    return torch.cat([qc.grad, tr.grad], dim=1)


def live_row(kind, pose7, seed):
    """-> (w, q, g_mean, g_rot) float32 of one live Gaussian."""
    g = torch.Generator().manual_seed(seed)
    w, q = torch.randn(3, generator=g) * 2, torch.randn(4, generator=g)
    gm, gr = torch.randn(3, generator=g), torch.randn(4, generator=g)
    if kind == "zero_q":
        q = torch.zeros(4)
    elif kind == "tiny_q":
        q = q / q.norm() * 1e-15
    elif kind == "parallel":        # upstream parallel to the activated rotation: the projection g - r (r.g) cancels
        qc = torch.tensor(np.asarray(pose7[:4], dtype=np.float32))
        gr = F.normalize(_quat_mult(qc, F.normalize(q, dim=0)), dim=0) * 1.75
    elif kind == "far":
        w, gm = w / w.norm() * 1e3, gm * 1e-4
    return w, q, gm, gr


def check_single_share(device, P):
    positions = sorted({p for p in (0, 63, 64, 255, 256, P - 1) if p < P})
    poses = [list(UNIT_POSES["general"]) + [0.1, -0.2, 0.3], list(UNIT_POSES["near identity"]) + [-1.5, 0.25, 2.0]]
    ek, em, at = [], [], []
    case = 0
    for i, pos in enumerate(positions):
        for kind in ("plain", SHARE_KINDS[1 + (i + P) % 4]) + (SHARE_KINDS[1:] if pos == positions[-1] else ()):
            pose7 = poses[case % 2]
            case += 1
            w, q, gm, gr = live_row(kind, pose7, 1000 * P + 10 * pos + SHARE_KINDS.index(kind))
            means, rots = torch.full((P, 3), float("nan")), torch.full((P, 4), float("nan"))
            rots[::2] = 0.0                                              # dead rows: NaN means; NaN or zero quaternions
            g_means, g_rots = torch.zeros(P, 3), torch.zeros(P, 4)
            means[pos], rots[pos], g_means[pos], g_rots[pos] = w, q, gm, gr
            ref = shares(pose7, w[None], q[None], gm[None], gr[None], 0, torch.float64)[0]
            mir = shares(pose7, w[None], q[None], gm[None], gr[None], 0, torch.float32)[0].double()
            qn = float(q.double().norm())
            scale = max(float(ref[:4].abs().max()), float(gr.double().norm()) / max(qn, 1.0) if qn > 0 else 0.0,
                        float(gm.double().norm() * w.double().norm()))
            assert scale > 0 and torch.isfinite(ref).all() and torch.isfinite(mir).all(), (kind, ref, mir)
            outs = []
            for pose_only in (1, 0):
                got, rows = run_backward_pose(device, 0, pose7, means, rots, g_means, g_rots, pose_only)
                assert torch.isfinite(got).all(), (P, pos, kind, pose_only, got)
                assert torch.equal(got[4:], gm), (P, pos, kind, pose_only, got[4:], gm)           # dL/dt: the live row's g_means3D, to the bit
                live = rows[pos // 256]
                dead = torch.cat([rows[:pos // 256], rows[pos // 256 + 1:]])
                assert torch.count_nonzero(dead) == 0 and torch.isfinite(live).all(), (P, pos, kind, "a dead row reached a workgroup's sums")
                outs.append(got)
            assert _same_bits(outs[0], outs[1]), (P, pos, kind, "pose_only changes the pose gradient")
            ek.append(float((outs[0][:4].double() - ref[:4]).abs().max()) / scale)
            em.append(float((mir[:4] - ref[:4]).abs().max()) / scale)
            at.append(f"{kind}@{pos}")
    kw, mw, km, mm = max(ek), max(em), sum(ek) / len(ek), sum(em) / len(em)
    _say("share/single", P=P, cases=len(ek), kernel_worst=kw, kernel_worst_at=at[ek.index(kw)], mirror_worst=mw, kernel_mean=km, mirror_mean=mm)
    assert kw <= max(2 * mw, 1e-6), f"worst share: kernel {kw:.3e} at {at[ek.index(kw)]} against the fp32 mirror's {mw:.3e}"
    assert km <= max(2 * mm, 8 * U), f"mean over the cases: kernel {km:.3e} against the fp32 mirror's {mm:.3e}"


DENSE = [(4097, 0), (4097, 1), (8193, 0), (8193, 1)]


def check_dense_shares(device, P, iso):
    g = torch.Generator().manual_seed(17 * P + iso)
    w, q = torch.randn(P, 3, generator=g) * 2, torch.randn(P, 4, generator=g) * torch.exp(torch.rand(P, 1, generator=g) * 4 - 2)
    gm, gr = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g)
    worst_k, worst_m = 0.0, 0.0
    for name in ("general", "near identity", "turn about y"):
        pose7 = list(UNIT_POSES[name]) + [0.1, -0.2, 0.3]
        s64 = shares(pose7, w, q, gm, gr, iso, torch.float64)
        # a component's scale: the sum of the rows' term scales (check_single_share's), whatever the shares themselves cancel to
        rot = torch.zeros(P, dtype=torch.float64) if iso else gr.double().norm(dim=1) / q.double().norm(dim=1).clamp_min(1.0)
        sq = float((rot + gm.double().norm(dim=1) * w.double().norm(dim=1)).sum())
        ref, scale = s64.sum(0), torch.cat([torch.full((4,), sq, dtype=torch.float64), gm.double().abs().sum(0)])
        s32 = shares(pose7, w, q, gm, gr, iso, torch.float32).numpy()
        mir = torch.tensor(np.cumsum(s32, axis=0, dtype=np.float32)[-1].astype(np.float64))       # fp32 shares added in fp32 in index order
        got = [run_backward_pose(device, iso, pose7, w, q, gm, gr, po)[0] for po in (1, 0)]
        assert _same_bits(got[0], got[1]), (P, iso, name, "pose_only changes the pose gradient")
        ek, em = float(((got[0].double() - ref).abs() / scale).max()), float(((mir - ref).abs() / scale).max())
        _say("share/dense", P=P, iso=iso, pose=name, kernel=ek, mirror=em)
        worst_k, worst_m = max(worst_k, ek), max(worst_m, em)
        assert ek <= max(2 * em, 8 * U), f"{name}: kernel {ek:.3e} of the sum of the term scales against the fp32 mirror's {em:.3e}"
    return worst_k, worst_m


# =====================================================================================================================================
# C. Loss rows
# =====================================================================================================================================
LOSS_ROW_IMAGES = ((16, 16), (255, 256), (256, 256), (257, 256), (513, 256))       # (W, H): 1, 255, 256, 257, 513 rows
LOSS_WEIGHTS = ((0.5, 1.0), (0.3, 0.7))                                                # (w_im, w_depth); the second pair's products round


def grid_loss_rows(nrows, seed):
    """[nrows,2] float32 on the grid 2^-10, magnitudes 1e-3 .. 1e4 (log-uniform), all distinct."""
    rng = np.random.default_rng(seed)
    k = np.floor(2.0 ** rng.uniform(0.0, math.log2(1e4 * 1024), 2 * nrows)).astype(np.int64)
    k.sort()
    for i in range(1, k.size):
        k[i] = max(k[i], k[i - 1] + 1)
    rng.shuffle(k)
    assert k.min() >= 1 and k.max() < 2 ** 24 and np.unique(k).size == k.size
    return torch.tensor(k.reshape(nrows, 2).astype(np.float64) / 1024.0).float()


def weighted32(S0, S1, w_im, w_depth):
    """tracking_loss_reduce's tail in numpy float32 from the exact sums -> [loss, depth, im]."""
    wd, wc = f32(S0) * f32(w_depth), f32(S1) * f32(w_im)
    out = np.array([wd + wc, wd, wc])
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def loss_scratch(device, W, H, rows):
    _, lib = _L()
    nrows = (W * H + 255) // 256
    nbytes = int(lib.gs_tracking_loss_scratch_bytes(W, H))
    assert 8 * nrows <= nbytes < 8 * nrows + 256, (W, H, nbytes)          # one row of two floats per workgroup of the image, rounded up to 256 bytes
    buf = torch.full((nbytes // 4,), float("nan"))
    if rows is not None:
        assert rows.shape == (nrows, 2)
        buf[:2 * nrows] = rows.reshape(-1)
    return buf.to(device)


def check_injected_loss_rows(device, W, H):
    nrows = (W * H + 255) // 256
    some_inexact = False
    for seed in (0, 1):
        rows = grid_loss_rows(nrows, 31 * seed + nrows)
        S = rows.double().sum(0)
        assert float(S[0]) * 1024 == round(float(S[0]) * 1024)            # (the float64 sums are exact)
        some_inexact |= float(f32(float(S[0]))) != float(S[0])
        for w_im, w_depth in LOSS_WEIGHTS:
            want = weighted32(float(S[0]), float(S[1]), w_im, w_depth)
            trk = Track(device, torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1), torch.zeros(1, 3, 1), 0)
            trk.begin()
            hist = trk.step(1, pose_scratch(device, dyadic_rows(1, 3)), W, H, loss_scratch(device, W, H, rows), w_im, w_depth, LR_ROT, LR_TRANS, 1)
            st = trk.state.cpu()
            assert _same_bits(st[22:25], want), (W, H, seed, w_im, st[22:25].tolist(), want.tolist())
            assert _same_bits(hist[0:3], want), (W, H, seed, w_im, hist[0:3].tolist(), want.tolist())
    _say("loss/injected", image=f"{W}x{H}", rows=nrows, sums_beyond_fp32=int(some_inexact))
    assert some_inexact or nrows < 255


REAL_LOSS_IMAGES = ((1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 257), (5, 7), (67, 45))   # (W, H)
SIL_THRES = 0.99


def check_real_loss_rows(device, W, H):
    from tests import tracking_cases as TC                                 # (the inputs with their special pixels only)
    L, lib = _L()
    npix, nrows = W * H, (W * H + 255) // 256
    worst = dict(depth=0.0, im=0.0)
    for use_sil, plain in ((1, 0), (0, 0), (1, 1)):
        ins = TC.loss_inputs(W, H, "cpu", seed=W + H)
        if plain:                                                        # no special pixel: every pixel is in both sums (the small images' depth rows)
            g = torch.Generator().manual_seed(W * H)
            ins[2], ins[4] = torch.rand(1, H, W, generator=g) * 3 + 0.5, torch.rand(1, H, W, generator=g) * 3 + 0.5
            ins[3], ins[5] = ins[2] * ins[2] + 0.05, torch.ones(1, H, W)
        im, gt, depth, dsq, gtd, sil = ins
        for w_im, w_depth in LOSS_WEIGHTS:
            d = [x.contiguous().to(device) for x in ins]
            grads = torch.empty(4, H, W, device=device)
            scratch = loss_scratch(device, W, H, None)
            out = torch.full((3,), float("nan"), device=device)
            L.check(lib.gs_tracking_loss(W, H, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                         d[5].data_ptr() if use_sil else None, use_sil, SIL_THRES, w_im, w_depth, grads[:3].data_ptr(),
                                         grads[3:].data_ptr(), scratch.data_ptr(), out.data_ptr(), _stream(device)))
            rows = scratch.cpu()
            assert torch.isnan(rows[2 * nrows:]).all(), "a row behind the image's last workgroup was written"
            rows = rows[:2 * nrows].view(nrows, 2)
            # float64 terms of the fp32 inputs, pixel by pixel
            m = (gtd > 0) & ~torch.isnan(depth) & ~torch.isnan(dsq - depth * depth)
            if use_sil:
                m = m & (sil > f32(SIL_THRES).item())
            m = m.view(-1)
            td = torch.where(m, (gtd.double() - depth.double()).abs().view(-1), torch.zeros(npix, dtype=torch.float64))
            tc = (gt.double() - im.double()).abs().view(3, npix).sum(0)
            tc = torch.where(m, tc, torch.zeros_like(tc)) if use_sil else tc
            for r in range(nrows):
                sd, sc = td[256 * r:256 * r + 256].sum(), tc[256 * r:256 * r + 256].sum()       # (non-negative terms: sum |terms| = the sum)
                ed = abs(float(rows[r, 0]) - float(sd)) / max(10 * U * float(sd), 1e-300)
                ec = abs(float(rows[r, 1]) - float(sc)) / max(10 * U * float(sc), 1e-300)
                if float(sd) == 0:
                    assert float(rows[r, 0]) == 0
                    ed = 0.0
                worst["depth"], worst["im"] = max(worst["depth"], ed), max(worst["im"], ec)
            # the step reduces the same rows to the same bits
            trk = Track(device, torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1), torch.zeros(1, 3, 1), 0)
            trk.begin()
            hist = trk.step(1, pose_scratch(device, dyadic_rows(1, 3)), W, H, scratch, w_im, w_depth, LR_ROT, LR_TRANS, 1)
            assert _same_bits(trk.state.cpu()[22:25], out) and _same_bits(hist[0:3], out), (W, H, use_sil, trk.state.cpu()[22:25], out.cpu())
            S = rows.double().sum(0)                                     # (a dozen fp32 values of one size: exact in float64 in any order)
            assert _same_bits(out, weighted32(float(S[0]), float(S[1]), w_im, w_depth)), (W, H, use_sil, out.cpu(), S)
    _say("loss/real", image=f"{W}x{H}", rows=nrows, depth=worst["depth"], im=worst["im"])
    assert worst["depth"] <= 1, f"a depth row misses (6 + 3 + 1) u of its terms: {worst['depth']:.3f}"
    assert worst["im"] <= 1, f"a colour row misses (6 + 3 + 1) u of its terms: {worst['im']:.3f}"


# =====================================================================================================================================
# D. The Adam step on the pose
# =====================================================================================================================================
def _translation_rows(k, nrows, seed):
    """dyadic rows whose translation columns sum to small, large, zero and 2^-70 gradients as the steps go."""
    rows = dyadic_rows(nrows, 100 * seed + k)
    kind = (k + 4 * seed) % 7                                            # seed 1: the 2^-70 gradient meets the fresh state of step 1
    if kind == 3:
        rows[:, 0:3] = 0.0                                               # a zero gradient
    elif kind == 5:
        rows[:, 0:3] = 0.0
        rows[0, 0], rows[0, 1], rows[nrows - 1, 2] = 2.0 ** -70, -(2.0 ** -70), 2.0 ** -70     # g^2 = 2^-140 underflows
    elif k % 3 == 0:
        rows[:, 0:3] = rows[:, 0:3] / 4096.0                             # small
    return rows


def check_translation_bits(device, P=4097, steps=30):
    """Components 4..6 of p, m, v equal the numpy float32 sequence at every step; the quaternion moves in the same run."""
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        T, t = 3, 1
        rots, trans = torch.randn(1, 4, T, generator=g), torch.randn(1, 3, T, generator=g)
        trk = Track(device, rots, trans, t)
        trk.begin()
        p = trk.column().numpy()
        m, v = np.zeros(7, dtype=np.float32), np.zeros(7, dtype=np.float32)
        q0 = p[:4].copy()
        for k in range(1, steps + 1):
            rows = _translation_rows(k, nrows_of(P), seed)
            grad = np.zeros(7, dtype=np.float32)
            grad[4:] = rows.double().sum(0)[0:3].numpy()                  # exact, and fp32 holds it
            assert np.array_equal(grad[4:].astype(np.float64), rows.double().sum(0)[0:3].numpy())
            trk.step(P, pose_scratch(device, rows), 16, 16, one_loss_row(device), 0.5, 1.0, LR_ROT, LR_TRANS, k)
            p, m, v = adam_mirror32(p, grad, m, v, LR_ROT, LR_TRANS, k)
            st, col = trk.state.cpu(), trk.column()
            for name, got, want in (("p", col[4:], p[4:]), ("m", st[4:7], m[4:]), ("v", st[11:14], v[4:])):
                assert _same_bits(got, torch.from_numpy(np.ascontiguousarray(want))), (seed, k, name, got.tolist(), want.tolist())
            assert bool((st[25:32] == 0).all())
        assert not np.array_equal(trk.column().numpy()[:4], q0) and bool(torch.isfinite(trk.column()).all())
        trk.assert_rest_untouched()


def check_quaternion_bits(device, P=4097):
    """Column (c, 0, 0, 0), c a power of two: u = (1, 0, 0, 0), the gradient of step 1 is exact -- grad[0] = 0, grad[k] = (2 (dR_a - dR_b) +
    t[12 + k]) / c -- and all seven values follow the fp32 sequence to the bit; lr_rot != lr_trans."""
    lr_rot, lr_trans = 2e-3, 5e-4
    for c in (0.125, 1.0, 32.0):
        for seed in (0, 1):
            rows = dyadic_rows(nrows_of(P), 11 + seed, top=512)
            t = rows.double().sum(0)
            dR = t[3:12]
            gq = torch.stack([torch.zeros((), dtype=torch.float64), 2 * (dR[7] - dR[5]) + t[13], 2 * (dR[2] - dR[6]) + t[14],
                              2 * (dR[3] - dR[1]) + t[15]])
            gq[1:] = gq[1:] / c
            grad = torch.cat([gq, t[0:3]])
            assert torch.equal(grad.float().double(), grad)               # fp32 holds the exact gradient
            ref2 = step_gradient_tier2((c, 0.0, 0.0, 0.0), t)
            assert float((ref2 - grad).abs().max()) <= 1e-12 * float(grad.abs().max())      # (the closed form is the chain's)
            T, tt = 2, 1
            rots, trans = torch.zeros(1, 4, T), torch.tensor([[[0.5, -1.25], [2.0, 0.75], [-3.0, 1.5]]])
            rots[0, 0, :] = c
            trk = Track(device, rots, trans, tt)
            trk.begin()
            p0 = trk.column().numpy()
            trk.step(P, pose_scratch(device, rows), 16, 16, one_loss_row(device), 0.5, 1.0, lr_rot, lr_trans, 1)
            p, m, v = adam_mirror32(p0, grad.float().numpy(), np.zeros(7, dtype=np.float32), np.zeros(7, dtype=np.float32), lr_rot, lr_trans, 1)
            st = trk.state.cpu()
            for name, got, want in (("p", trk.column(), p), ("m", st[0:7], m), ("v", st[7:14], v)):
                assert _same_bits(got, torch.from_numpy(np.ascontiguousarray(want))), (c, seed, name, got.tolist(), want.tolist())
            assert float(st[0]) == 0 and float(st[7]) == 0 and trk.column()[0] == c
            trk.assert_rest_untouched()


EVOLUTION_COLUMNS = ("general", "near identity", "norm 1e-3", "turn about y", "norm 1e3")


def _evolution_rows(k, nrows, seed):
    rows = dyadic_rows(nrows, 1000 * seed + k)
    if k % 5 == 0:
        rows = rows / 1024.0                                             # (small and large steps)
    return rows


def _gradient_with_allowance(col, t16):
    """-> (float64 gradient at the kernel's own normalised column, E_g = u |g| + 2^-45 S; the translation is exact)."""
    g, S = step_gradient_tier1(col, t16)
    e_g = U * g.abs() + SLACK * S
    e_g[4:] = 0.0
    return g.numpy(), e_g.numpy()


def check_adam_evolution(device, name, P=4097, steps=30, kernel=True):
    """30 steps from a general column; at every step the float64 reference restarts from the previous fp32 state (the kernel's, or the mirror's
    with kernel=False: the guard of the rule, which runs no kernel)."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for seed in (0, 1):
        T, t = 2, 0
        rots, trans = torch.zeros(1, 4, T), torch.tensor([[[0.5, -1.25], [2.0, 0.75], [-3.0, 1.5]]])
        rots[0, :, t] = torch.tensor(np.asarray(COLUMNS[name], dtype=np.float32))
        rots[0, 0, 1] = 1.0
        if kernel:
            trk = Track(device, rots, trans, t)
            trk.begin()
            p = trk.column().numpy()
        else:
            p = torch.cat([rots[0, :, t], trans[0, :, t]]).numpy()
        m, v = np.zeros(7, dtype=np.float32), np.zeros(7, dtype=np.float32)
        for k in range(1, steps + 1):
            rows = _evolution_rows(k, nrows_of(P), seed)
            g64, e_g = _gradient_with_allowance(p[:4], rows.double().sum(0))
            if kernel:
                trk.step(P, pose_scratch(device, rows), 16, 16, one_loss_row(device), 0.5, 1.0, LR_ROT, LR_TRANS, k)
                st = trk.state.cpu().numpy()
                after = (trk.column().numpy(), st[0:7].copy(), st[7:14].copy())
            else:
                after = adam_mirror32(p, g64.astype(np.float32), m, v, LR_ROT, LR_TRANS, k)
            r = adam_ratios((p, g64, m, v), after, e_g, LR_ROT, LR_TRANS, k)
            worst = {q: max(worst[q], r[q]) for q in worst}
            p, m, v = after
        assert np.isfinite(p).all()
    _say("adam-evolution" if kernel else "adam-mirror", column=name, steps=steps, p=worst["p"], m=worst["m"], v=worst["v"])
    assert max(worst.values()) <= SAFETY, f"{'a step of the evolution' if kernel else 'the fp32 mirror'} misses the one-step rule on {name}: {worst}"
    return worst


LAYOUTS = ((1, 0), (2, 0), (2, 1), (5, 0), (5, 4))                      # (num_frames, time_idx)


def check_layout(device, T, t, P=257, steps=3):
    g = torch.Generator().manual_seed(10 * T + t)
    rots, trans = torch.randn(1, 4, T, generator=g), torch.randn(1, 3, T, generator=g)
    trk = Track(device, rots, trans, t)
    trk.begin()
    st = trk.state.cpu()
    assert bool((st[0:14] == 0).all()) and float(st[14]) == float(f32(1e20)) and bool((st[25:32] == 0).all())
    assert _same_bits(st[15:22], torch.cat([rots[0, :, t], trans[0, :, t]])) and _same_bits(st[15:22], trk.column())
    assert _same_bits(st[32:], _canary(st.numel())[32:])
    trk.assert_rest_untouched()
    before = trk.column()
    for k in range(1, steps + 1):
        hist = trk.step(P, pose_scratch(device, dyadic_rows(nrows_of(P), k)), 16, 16, one_loss_row(device), 0.5, 1.0, LR_ROT, LR_TRANS, k)
        trk.assert_rest_untouched()
        st = trk.state.cpu()
        assert bool((st[25:32] == 0).all()) and _same_bits(st[32:], _canary(st.numel())[32:])
        assert _same_bits(hist[3:10], trk.column())
    assert not bool((trk.column() == before).any()), "a value of the column did not move"


# =====================================================================================================================================
# E. Candidate rule and bookkeeping
# =====================================================================================================================================
INF, NAN = float("inf"), float("nan")
LOSS_SEQUENCES = {
    "ties, nan, inf": (5.0, 3.0, 3.0, NAN, 4.0, 2.0, 2.0, INF, 1.0),
    "first loss 1e20f": (float(f32(1e20)), 2e20, 1e30, INF, 3e20),
    "all nan": (NAN, NAN, NAN, NAN),
}


def check_candidate_rule(device, name, P=300):
    losses = LOSS_SEQUENCES[name]
    T, t = 3, 2
    g = torch.Generator().manual_seed(5)
    rots, trans = torch.randn(1, 4, T, generator=g), torch.randn(1, 3, T, generator=g)
    runs = {}
    for history in (True, False):
        trk = Track(device, rots, trans, t)
        trk.begin()
        first = trk.column()
        best, cand, best_k = f32(1e20), first, None
        states = []
        for k, loss in enumerate(losses, 1):
            hist = trk.step(P, pose_scratch(device, dyadic_rows(nrows_of(P), k)), 16, 16, one_loss_row(device, loss, 0.0), 1.0, 1.0,
                            LR_ROT, LR_TRANS, k, history=history)
            st = trk.state.cpu()
            states.append(st.clone())
            if not history:
                continue
            assert _same_bits(hist[3:10], trk.column()), (name, k)
            want = torch.tensor([loss, loss, 0.0])
            assert _same_bits_or_nan(hist[0:3], want) and _same_bits_or_nan(st[22:25], want), (name, k, hist[0:3], st[22:25])
            if f32(float(hist[0])) < best:                               # SplaTAM's rule: strict <, from float(1e20)
                best, cand, best_k = f32(float(hist[0])), hist[3:10].clone(), k
            assert float(st[14]) == float(best) and _same_bits(st[15:22], cand), (name, k, best_k, st[14:22], cand)
            assert float(st[25]) == 0
        runs[history] = states
        if history:
            if name == "ties, nan, inf":
                assert best_k == 9 and float(best) == 1.0
            else:
                assert best_k is None and _same_bits(trk.state.cpu()[15:22], first) and float(trk.state.cpu()[14]) == float(f32(1e20))
            if name == "ties, nan, inf":                                 # the replay step by step: 1, 2, 2, 2, 2, 6, 6, 6, 9
                mins = [float(s[14]) for s in states]
                assert mins == [5.0, 3.0, 3.0, 3.0, 3.0, 2.0, 2.0, 2.0, 1.0], mins
                assert _same_bits(states[2][15:22], states[1][15:22]) and _same_bits(states[6][15:22], states[5][15:22]), "a tie replaced the earlier step"
                assert _same_bits(states[3][15:22], states[1][15:22]) and _same_bits(states[7][15:22], states[5][15:22]), "a NaN or inf loss won"
    for a, b in zip(runs[True], runs[False]):
        assert _same_bits_or_nan(a, b), "a NULL history_row changes the state"
    _say("candidate", sequence=name, steps=len(losses))
