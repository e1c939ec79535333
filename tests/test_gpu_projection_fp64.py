"""GPU (-m gpu): the HIP per-Gaussian kernels' debug-forward records (util.artefacts()'s geom -- pixel mean, conic, opacity, colour, depth --
with radii, rects and tile counts) against the fp64 published-form reference (oracle/dense_torch.project_dense, evaluated in float64 on the
device) under the one rule of tests/projection_cases.py.  Each test prints its boundary-exception counts and its conic (and colour) error
percentiles."""
import numpy as np
import pytest
import torch

from activesplat_amd import rasterizer as R
from activesplat_amd import synthetic as syn
from activesplat_amd.camera import setup_camera
from oracle.dense_torch import U32, project_dense
from tests import fuzz_scenes, parity_cases as pc, projection_cases as prc, util

pytestmark = pytest.mark.gpu

HARD_SEEDS = list(range(330000, 330012))


def _check(rs, rv, label):
    got = util.run_product(rs, rv)
    rec = prc.records_from_artefacts(util.artefacts(), got["radii"])
    return prc.compare(rec, prc.reference(rs, rv), f"hip {label}", rgb="sh" if "shs" in rv else "given")


def test_projection_fp64_configs1(hip):
    """configs[1]: 500 k Gaussians, 640 x 480, colours given"""
    _check(*util.scene(500_000, 640, 480, seed=0, device=hip), "configs1")


def test_projection_fp64_configs2_sh3(hip):
    """configs[2]: 2 M Gaussians, 640 x 480, SH degree 3 -- the per-Gaussian SH colour included"""
    st = _check(*util.scene(2_000_000, 640, 480, seed=0, device=hip, sh_degree=3), "configs2")
    assert "rgb_ratio" in st


def test_projection_fp64_topdown_1m(hip):
    """the planner's top-down camera (1000 m up, focal length 2e4 px, scale_modifier 0.01) over 1 M Gaussians: low-pass-dominated splats"""
    _check(*pc.topdown_scene(1_000_000, hip), "topdown_1m")


@pytest.mark.parametrize("case", ["cov3d_precomp", "posed_white_bg"])
def test_projection_fp64_cases(hip, case):
    _check(*pc.build_case(case, hip), case)


@pytest.mark.parametrize("seed", HARD_SEEDS + [s for s, _ in fuzz_scenes.FLAGGED_R06_HARD])
def test_projection_fp64_hard_sweep(hip, seed):
    """the s = 1.2 anisotropic sweep (needles above 2 000 : 1; odd seeds in front of the near plane) and the scenes it flagged"""
    _check(*fuzz_scenes.hard_scene(seed, hip, 1.2), f"hard_{seed}")


@pytest.mark.parametrize("scene", ["offscreen_clamp", "near_plane"])
def test_projection_fp64_named_scenes(hip, scene):
    rs, rv = prc.offscreen_scene(20000, hip, W=320, H=240) if scene == "offscreen_clamp" else prc.near_plane_scene(20000, hip, W=320, H=240)
    _check(rs, rv, scene)


def _raw_reference(rs, p, pose7, iso, dev):
    """transform_to_frame + the activations in fp64 (slam_helpers.py:252-304,124-139), on the fp32 parameters and the fp32 pose the kernel
    receives, then project_dense.  The kernel evaluates the frame transform and the activations in fp32 (exp and the sigmoid through
    __expf): their bounds enter project_dense as input errors -- the means to 8 u of |R||p| + |t|, the scales to (4 + 1.5 |log s|) u
    relative, the unit quaternion to 8 u per component, the opacity to (4 + 1.5 |logit|) u of itself + 2 u."""
    from activesplat_amd.mapping import quat_mult
    d = lambda t: t.detach().to(dev, torch.float64)  # noqa: E731
    q32 = torch.tensor(np.asarray(pose7[:4], np.float32), dtype=torch.float64, device=dev)
    t32 = torch.tensor(np.asarray(pose7[4:], np.float32), dtype=torch.float64, device=dev)
    r, x, y, z = q32.tolist()
    Rc = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                       [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                       [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64, device=dev)
    m = d(p["means3D"])
    means = m @ Rc.T + t32
    means_err = 8 * U32 * (m.abs() @ Rc.abs().T + t32.abs())
    uq = torch.nn.functional.normalize(d(p["unnorm_rotations"]))
    rot = uq if iso else torch.nn.functional.normalize(quat_mult(q32.expand_as(uq), uq))
    ls = d(p["log_scales"])
    scales = torch.exp(ls).expand(-1, 3) if iso else torch.exp(ls)
    lo = d(p["logit_opacities"]).reshape(-1)
    op = torch.sigmoid(lo)
    op_err = (4 + 1.5 * lo.abs()) * U32 * op + 2 * U32
    ref = project_dense(util.cam_dict(rs), means, op, colors=d(p["rgb_colors"]), scales=scales, rotations=rot, means_err=means_err,
                            scale_rel=float((4 + 1.5 * ls.abs().max()) * U32), rot_err=8 * U32, opacity_err=op_err)
    return ref


@pytest.mark.parametrize("iso", [False, True], ids=["anisotropic", "isotropic"])
def test_projection_fp64_raw_parameter_entry(hip, iso):
    """render_rgbd_raw: the frame transform and the activations run inside the per-Gaussian kernel -- the path every tracking and mapping
    iteration takes.  Geometric fields: pixel mean, conic, opacity, depth, radius, rect."""
    W, H, n = 320, 240, 100_000
    p = syn.make_params(n, W, H, seed=41)
    if iso:
        p["log_scales"] = p["log_scales"][:, :1].contiguous()
    p["log_scales"] = p["log_scales"] + 0.4
    rs = setup_camera(W, H, syn.intrinsics(W, H), np.eye(4), device=hip)
    a = 0.3
    pose7 = [float(np.cos(a / 2)), 0.0, float(np.sin(a / 2)), 0.0, 0.12, -0.05, 0.3]
    prm = {k: v.to(hip).contiguous() for k, v in p.items()}
    m2d = torch.zeros_like(prm["means3D"])
    with R.capture() as state:
        out = R.render_rgbd_raw(rs, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"], pose7,
                                colors_precomp=prm["rgb_colors"])
    util.LAST.clear(); util.LAST.update(state)
    rec = prc.records_from_artefacts(util.artefacts(), out[1].cpu().numpy())
    ref = _raw_reference(rs, p, pose7, iso, hip)
    st = prc.compare(rec, ref, f"hip raw entry {'isotropic' if iso else 'anisotropic'}", rgb=None, opacity="bound")
    assert st["visible"] > 0.5 * n
