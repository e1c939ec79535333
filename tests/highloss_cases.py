"""Shared checks of the per-frame high-loss look target (activesplat_amd/visibility.py: high_loss_grid, high_loss_target,
target_from_high_loss_clusters; gs_high_loss_grid; SplatMapper(high_loss_target=True)): run on the host-emulated kernels by
tests/test_highloss.py and on the MI355X by tests/test_gpu_highloss.py.

References
* `pixel_rule`: src/mapper/splatam/__init__.py:212-215 in numpy float32, operation for operation.
* `resize_int`: the integer resize rule of include/gsplat_hip.h in numpy int64.  tests/test_highloss.py compares it with `frames.resize_linear`,
  the project's float64 restatement of cv2's sampling convention, on every mask of every case here.
* `cluster_cases.restate`: the labelling rule of gs_grid_dbscan in numpy.  tests/golden/make_highloss_golden.py ran it against
  sklearn.cluster.DBSCAN(eps=5, min_samples=10).fit_predict(np.column_stack(np.where(grid > 0))) on the grid of every case here and stored the
  grids and sklearn's labels in tests/golden/highloss.npz; tests/test_highloss.py compares the two again from the fixture.
* `restate_target`: src/mapper/splatam/__init__.py:219-250 op for op on a grid, with the restated labels.

Tolerances: none.  Masks and grids are compared bit for bit; the 4 x 4 pose with np.array_equal, because the call and the restatement run the same
numpy operations on the same integers.
"""
import os

import numpy as np
import torch

from activesplat_amd import lookaround as LA
from activesplat_amd import synthetic as syn
from activesplat_amd import visibility as VIS
from tests import cluster_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "highloss.npz")

#: (name, source H, source W, grid H, grid W).  The sizes are read as rows x columns; the non-square ones also run transposed, so that either
#: reading of "7 x 5 -> 11 x 9" is covered
RESIZE_CASES = (("up", 7, 5, 11, 9), ("up_t", 5, 7, 9, 11), ("mixed", 37, 53, 90, 90), ("mixed_t", 53, 37, 90, 90), ("s40x48", 40, 48, 90, 90),
                ("s48x40", 48, 40, 90, 90), ("s150x120", 150, 120, 90, 90), ("s120x150", 120, 150, 90, 90), ("s256", 256, 256, 90, 90),
                ("identity", 90, 90, 90, 90))
#: the masks of every resize case: random at three densities, and blobs that touch each image edge
MASK_KINDS = ("random10", "random50", "random90", "blobs")
MIN_TIE_SHARE = 0.01


# ---- the rules, restated ----------------------------------------------------------------------------------------------------------------

def pixel_rule(depth, opacity, gt, depth_err_thres=0.3, opacity_thres=0.8):
    depth, opacity, gt = (np.asarray(a, np.float32) for a in (depth, opacity, gt))
    with np.errstate(invalid="ignore"):
        depth_diff = np.abs(depth - gt)
        depth_error = depth_diff * (gt > 0).astype(np.float32)
        return (depth > gt) & (depth_error > np.float32(depth_err_thres)) & (opacity > np.float32(opacity_thres))


def _axis(n_dst, n_src):
    d = np.arange(n_dst, dtype=np.int64)
    den = 2 * n_dst
    num = (2 * d + 1) * n_src - n_dst
    i0 = num // den                                      # (numpy's // floors towards -inf)
    w1 = num - i0 * den
    return np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1), den - w1, w1, den


def resize_int(mask, grid_w, grid_h):
    """-> (grid float32 [grid_h, grid_w] of 0 / 1, ties bool: the pixels whose bilinear value is exactly one half)"""
    m = np.asarray(mask).astype(np.int64)
    y0, y1, wy0, wy1, den_y = _axis(grid_h, m.shape[0])
    x0, x1, wx0, wx1, den_x = _axis(grid_w, m.shape[1])
    S = (m[y0][:, x0] * wy0[:, None] * wx0[None, :] + m[y0][:, x1] * wy0[:, None] * wx1[None, :]
         + m[y1][:, x0] * wy1[:, None] * wx0[None, :] + m[y1][:, x1] * wy1[:, None] * wx1[None, :])
    return (2 * S >= den_x * den_y).astype(np.float32), 2 * S == den_x * den_y


def restate_target(grid, view_c2w, cluster_invisibility_threshold=25, hfov=90, vfov=90):
    """src/mapper/splatam/__init__.py:219-250 on the resized mask (`grid`: 0 / 1) -> (pose or None, restated clustering or None)"""
    high_loss_samples_pose_c2w = None
    non_presence_depth_mask_np = np.asarray(grid).astype(np.uint8)
    non_presence_depth_points = np.column_stack(np.where(non_presence_depth_mask_np > 0))
    if len(non_presence_depth_points) == 0:
        return None, None
    r = None
    if np.sum(non_presence_depth_mask_np) > 20:
        r = cc.restate(non_presence_depth_mask_np.astype(np.float32), 0.0, 5, 10)
        cluster_centers, cluster_invisibilities = [], []
        for cluster in range(r["n_clusters"]):
            rows, cols = np.where(r["labels"] == cluster)
            points = np.column_stack([rows, cols])
            center = points.mean(axis=0)
            invisibility_sum = np.sum(non_presence_depth_mask_np[points[:, 0], points[:, 1]])
            if invisibility_sum > cluster_invisibility_threshold:
                cluster_centers.append(center)
                cluster_invisibilities.append(invisibility_sum)
        if len(cluster_invisibilities) > 0:
            max_area_center = cluster_centers[int(np.argmax(cluster_invisibilities))]
            center_vec = np.array([max_area_center[1] / non_presence_depth_mask_np.shape[1] * hfov - hfov / 2,
                                   max_area_center[0] / non_presence_depth_mask_np.shape[0] * vfov - vfov / 2])
            horizontal_angle = np.deg2rad(center_vec[0])
            vertical_angle = np.deg2rad(center_vec[1])
            if np.abs(horizontal_angle) > np.deg2rad(5) or np.abs(vertical_angle) > np.deg2rad(5):
                high_loss_samples_pose_c2w = LA.rot_axis(view_c2w, "y", horizontal_angle)
                high_loss_samples_pose_c2w = LA.rot_axis(high_loss_samples_pose_c2w, "x", vertical_angle)
    return high_loss_samples_pose_c2w, r


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------

def case_mask(name, kind):
    _, H, W, _, _ = next(c for c in RESIZE_CASES if c[0] == name)
    g = np.random.default_rng(1000 * H + 10 * W + MASK_KINDS.index(kind))
    if kind.startswith("random"):
        return g.random((H, W)) < int(kind[6:]) / 100
    # blobs: a thresholded smooth field, and a run of ones along a part of each edge
    f = cc._blur(g.standard_normal((H + 8, W + 8)), max(1.0, min(H, W) / 12))[4:-4, 4:-4]
    m = f > 0.3 * f.std()
    m[0, : max(1, W // 3)] = True
    m[-1, W // 2:] = True
    m[H // 4: max(H // 4 + 1, H // 2), 0] = True
    m[: max(1, H // 3), -1] = True
    return m


def images_of(mask, device=None):
    """depth, opacity and gt images ([H, W] float32) whose pixel rule gives `mask`: the render 1 m behind the measured 1.5 m, opacity 0.9"""
    mask = np.asarray(mask, bool)
    depth = np.where(mask, np.float32(2.5), np.float32(1.5)).astype(np.float32)
    opacity = np.full(mask.shape, 0.9, np.float32)
    gt = np.full(mask.shape, 1.5, np.float32)
    if device is None:
        return depth, opacity, gt
    return tuple(torch.from_numpy(a).to(device) for a in (depth, opacity, gt))


_REF = {}


def resize_reference(name, kind):
    """(mask, grid, ties) of one resize case: computed once per process and shared"""
    if (name, kind) not in _REF:
        _, H, W, gh, gw = next(c for c in RESIZE_CASES if c[0] == name)
        m = case_mask(name, kind)
        grid, ties = resize_int(m, gw, gh)
        for a in (m, grid, ties):
            a.setflags(write=False)
        _REF[(name, kind)] = (m, grid, ties)
    return _REF[(name, kind)]


def assert_ties_are_exercised():
    """the issue's condition on the case set, asserted on the restatement: at least 1 % of all grid pixels at an exact tie"""
    ties = sum(int(resize_reference(n, k)[2].sum()) for n, *_ in RESIZE_CASES for k in MASK_KINDS)
    pixels = sum(gh * gw for _, _, _, gh, gw in RESIZE_CASES) * len(MASK_KINDS)
    print(f"exact ties: {ties} of {pixels} grid pixels = {ties / pixels:.2%}")
    assert ties >= MIN_TIE_SHARE * pixels, (ties, pixels)


def block(rows, cols, shape=(90, 90)):
    m = np.zeros(shape, bool)
    m[rows[0]:rows[1], cols[0]:cols[1]] = True
    return m


def decision_masks():
    """name -> (90 x 90 mask, cluster threshold, what the reference returns: 'none' or 'pose')"""
    d = {}
    d["nothing"] = (np.zeros((90, 90), bool), 25, "none")
    d["gate20"] = (block((10, 14), (10, 15)), 15, "none")                          # 4 x 5 = 20 ones: not > 20
    m = block((10, 14), (10, 15)); m[14, 10] = True
    d["gate21"] = (m, 15, "pose")                                                  # 21 ones: clustered, one cluster of 21 > 15
    d["count25"] = (block((10, 15), (10, 15)), 25, "none")                         # a cluster of exactly 25: not > 25
    m = block((10, 15), (10, 15)); m[15, 10] = True
    d["count26"] = (m, 25, "pose")
    d["equal"] = (block((60, 66), (60, 66)) | block((10, 16), (70, 76)), 25, "pose")      # two clusters of 36: number 0 (rows 10-15) wins
    d["centre5"] = (block((42, 49), (47, 54)), 25, "none")                         # centre (45, 50): 5 degrees exactly
    d["centre6"] = (block((42, 49), (48, 55)), 25, "pose")                         # centre (45, 51)
    d["vertical"] = (block((60, 67), (42, 49)), 25, "pose")                        # centre (63, 45): only the vertical angle
    d["three"] = (block((5, 11), (5, 11)) | block((40, 48), (60, 68)) | block((70, 76), (10, 17)), 25, "pose")
    return d


def view_pose():
    c2w = np.eye(4)
    c2w[:3, 3] = [0.3, -0.1, 0.2]
    return LA.rot_axis(c2w, "y", 0.4)


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(GOLDEN) as z:
            _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN


def golden_grids():
    """every grid whose clustering the fixture records: name -> grid (0 / 1 float32), rebuilt here from the cases"""
    out = {f"{n}_{k}": resize_reference(n, k)[1] for n, *_ in RESIZE_CASES for k in MASK_KINDS}
    out.update({f"decision_{n}": m.astype(np.float32) for n, (m, _, _) in decision_masks().items()})
    return out


def golden_labels(key, shape):
    """(the fixture's grid as bool, sklearn's labels in the convention of cluster_cases: -2 unmasked, -1 noise, else the cluster number)"""
    H, W = shape
    m = np.unpackbits(golden()[key + "_grid"])[:H * W].reshape(H, W).astype(bool)
    out = np.full((H, W), -2, np.int32)
    out[m] = golden()[key + "_sklearn"].astype(np.int32)
    return m, out


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------

def pixel_images():
    """37 x 53 images in which each of the three conditions alone decides some pixels, with the special values the issue lists"""
    H, W = 37, 53
    g = np.random.default_rng(3753)
    gt = np.full((H, W), 0.0625, np.float32)
    t = np.float32(0.3)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
    # depth - gt is exact here (multiples of 2^-25 in [0.25, 0.5)): the error is exactly the float below 0.3f, 0.3f, the float above it
    depth = (np.float32(0.0625) + g.choice(np.array([below, t, above], np.float32), (H, W))).astype(np.float32)
    assert set(np.unique(np.abs(depth - gt))) == {below, t, above}
    o = np.float32(0.8)
    opacity = g.choice(np.array([np.nextafter(o, np.float32(0)), o, np.nextafter(o, np.float32(1)), np.float32(0.95)], np.float32), (H, W))
    # rows 20-: free errors around the other two conditions
    gt[20:] = (0.5 + 2 * g.random((H - 20, W))).astype(np.float32)
    depth[20:] = (gt[20:] + g.choice(np.array([-1.0, -0.2, 0.0, 0.2, 1.0], np.float32), (H - 20, W))).astype(np.float32)     # depth <= gt in places
    gt[30, :10], depth[30, :10] = 0.0, 2.0               # unmeasured: the error is multiplied by 0
    gt[30, 10:20], depth[30, 10:20] = -1.0, 2.0          # below 0
    gt[31, :10] = np.nan
    depth[31, 10:20] = np.nan
    depth[31, 20:30] = np.inf                            # over a measured pixel: flagged when the opacity allows
    depth[32, :10], gt[32, :10] = np.inf, 0.0            # inf * 0 = NaN: 0
    depth[32, 10:20], gt[32, 10:20] = np.inf, np.inf
    opacity[33, :20] = np.nan
    depth[33, :20], gt[33, :20] = 3.0, 1.0
    opacity[34], depth[34], gt[34] = 0.95, 3.0, 1.0      # a row that is flagged whatever the draw
    return depth, opacity, gt


def check_pixel_rule(device):
    from activesplat_amd import _lib
    depth, opacity, gt = pixel_images()
    want = pixel_rule(depth, opacity, gt)
    with np.errstate(invalid="ignore"):
        a, b, c = depth > gt, np.abs(depth - gt) * (gt > 0) > np.float32(0.3), opacity > np.float32(0.8)
    # each condition alone decides some pixels
    assert (~a & b & c).any() and (a & ~b & c).any() and (a & b & ~c).any() and want.any()
    assert not want[30, :20].any() and not want[31, :20].any() and want[31, 20:30].any() and not want[32, :20].any() and not want[33, :20].any()
    d, o, g = (torch.from_numpy(x).to(device) for x in (depth, opacity, gt))
    mask, grid = VIS.high_loss_grid(d, o, g)
    assert mask.dtype == torch.bool and mask.shape == (37, 53) and grid.dtype == torch.float32 and grid.shape == (90, 90)
    # SplatMapper.high_loss_samples_mask's expression on the same tensors
    d3, o3, g3 = d.unsqueeze(0), o.unsqueeze(0), g.unsqueeze(0)
    err = (d3 - g3).abs() * (g3 > 0)
    torch_mask = ((d3 > g3) & (err > 0.3) & (o3 > 0.8))[0]
    print(f"pixel rule: {int(want.sum())} of {want.size} flagged")
    assert torch.equal(mask, torch_mask)
    assert np.array_equal(mask.cpu().numpy(), want)
    assert np.array_equal(grid.cpu().numpy(), resize_int(want, 90, 90)[0])
    # the [1, H, W] form, strided inputs, and a null mask_full: the same grid
    wide = torch.zeros(3, 37, 2 * 53, device=device)
    wide[0, :, ::2], wide[1, :, ::2], wide[2, :, ::2] = d, o, g
    mask2, grid2 = VIS.high_loss_grid(wide[0:1, :, ::2], wide[1:2, :, ::2], wide[2:3, :, ::2])
    assert torch.equal(mask2, mask) and torch.equal(grid2, grid)
    grid3 = torch.full((90, 90), 7.0, device=device)
    lib = _lib.get()
    _lib.check(lib.gs_high_loss_grid(53, 37, d.data_ptr(), o.data_ptr(), g.data_ptr(), 0.3, 0.8, 90, 90, None, grid3.data_ptr(), _lib.stream_ptr(d.device)))
    assert torch.equal(grid3, grid)


def check_resize(device, name):
    _, H, W, gh, gw = next(c for c in RESIZE_CASES if c[0] == name)
    for kind in MASK_KINDS:
        m, want, ties = resize_reference(name, kind)
        mask, grid = VIS.high_loss_grid(*images_of(m, device), hfov=gw, vfov=gh)
        print(f"{name} {kind}: {H} x {W} -> {gh} x {gw}, {int(m.sum())} ones -> {int(want.sum())}, {int(ties.sum())} exact ties")
        assert np.array_equal(mask.cpu().numpy(), m), (name, kind)
        got = grid.cpu().numpy()
        assert got.shape == (gh, gw) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, kind, int((got != want).sum()))
        if name == "identity":
            assert np.array_equal(got, m.astype(np.float32))


def check_decision(device, name):
    m, thr, kind = decision_masks()[name]
    c2w = view_pose()
    want, r = restate_target(m.astype(np.float32), c2w, thr)
    assert {"none": want is None, "pose": want is not None}[kind], name
    if name == "gate21":
        assert int(m.sum()) == 21 and r["n_clusters"] == 1 and r["count"][0] == 21
    if name in ("count25", "count26"):
        assert r["n_clusters"] == 1 and r["count"][0] == int(name[5:])
    if name == "equal":
        assert r["n_clusters"] == 2 and r["count"][0] == r["count"][1] == 36 and r["root"][0] == 10 * 90 + 70
    if name == "centre5":
        assert r["sum_col"][0] / r["count"][0] / 90 * 90 - 90 / 2 == 5.0 and r["sum_row"][0] / r["count"][0] == 45.0
    if name == "vertical":
        assert r["sum_col"][0] / r["count"][0] == 45.0
    pose, mask, grid = VIS.high_loss_target(c2w, *images_of(m, device), cluster_invisibility_threshold=thr)
    assert np.array_equal(mask.cpu().numpy(), m) and np.array_equal(grid.cpu().numpy(), m.astype(np.float32))      # (90 x 90: the resize is the identity)
    assert (pose is None) == (want is None), name
    if want is not None:
        assert np.array_equal(pose, want), name
    if name == "equal":                                  # turned towards the cluster with the lower number, the one at rows 10-15
        turned = LA.rot_axis(LA.rot_axis(c2w, "y", np.deg2rad(72.5 / 90 * 90 - 90 / 2)), "x", np.deg2rad(12.5 / 90 * 90 - 90 / 2))
        assert np.array_equal(pose, turned)
    if name == "three":
        assert r["n_clusters"] == 3
        again, _, _ = VIS.high_loss_target(c2w, *images_of(m, device), cluster_invisibility_threshold=thr, max_clusters=1)
        assert np.array_equal(again, pose)
        # the largest of the three (64 pixels) is cluster 1: behind the first row of the table
        assert int(np.argmax(r["count"])) == 1


def _refused(call, text):
    from activesplat_amd import _lib
    try:
        call()
    except Exception as e:
        assert "gs_high_loss_grid" in str(e) and text in str(e), str(e)
        assert text.encode() in _lib.get().gs_last_error()
    else:
        raise AssertionError(f"accepted: {text}")


def check_refusals(device):
    from activesplat_amd import _lib
    lib = _lib.get()
    d, o, g = images_of(block((2, 5), (2, 5), (12, 16)), device)
    _refused(lambda: VIS.high_loss_grid(d, o, g, hfov=300, vfov=300), "grid size out of range")
    _refused(lambda: VIS.high_loss_grid(d, o, g, hfov=0), "grid size out of range")
    _refused(lambda: VIS.high_loss_grid(d, o, g, vfov=4097, hfov=1), "grid size out of range")
    grid = torch.full((90, 90), 7.0, device=device)
    mask = torch.full((12, 16), 7, dtype=torch.uint8, device=device)
    st = _lib.stream_ptr(d.device)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(width=16, height=12, depth=d.data_ptr(), opacity=o.data_ptr(), gt=g.data_ptr(), dt=0.3, ot=0.8,
                                                       gw=90, gh=90, mask=mask.data_ptr(), grid=grid.data_ptr(), stream=st).items()]
    for kw, text in ((dict(dt=float("nan")), "thresholds"), (dict(ot=float("nan")), "thresholds"), (dict(dt=-0.1), "thresholds"), (dict(ot=float("inf")), "thresholds"),
                     (dict(grid=None), "null pointer"), (dict(depth=None), "null pointer"), (dict(gt=None), "null pointer"), (dict(opacity=None), "null pointer"),
                     (dict(width=0), "image size out of range"), (dict(height=16385), "image size out of range"), (dict(gw=0), "grid size out of range"),
                     (dict(gw=300, gh=300), "grid size out of range")):
        assert lib.gs_high_loss_grid(*args(**kw)) == 1, kw               # GS_EINVAL
        assert text.encode() in lib.gs_last_error() and b"gs_high_loss_grid" in lib.gs_last_error(), (kw, lib.gs_last_error())
    # nothing was launched: the outputs still hold what they held
    assert bool((grid == 7.0).all()) and bool((mask == 7).all())
    assert lib.gs_high_loss_grid(*args()) == 0
    assert np.array_equal(mask.cpu().numpy(), block((2, 5), (2, 5), (12, 16)).astype(np.uint8))
    for bad in (torch.zeros(2, 12, 16, device=device), torch.zeros(16, device=device)):
        try:
            VIS.high_loss_grid(bad, bad, bad)
        except ValueError as e:
            assert "[H, W] or [1, H, W]" in str(e)
        else:
            raise AssertionError("high_loss_grid accepted a tensor that is not an image")


def check_repeatable(device):
    m, _, _ = resize_reference("s150x120", "blobs")
    imgs = images_of(m, device)
    a, b = VIS.high_loss_grid(*imgs), VIS.high_loss_grid(*imgs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    c2w = view_pose()
    p, q = VIS.high_loss_target(c2w, *imgs), VIS.high_loss_target(c2w, *imgs)
    assert (p[0] is None) == (q[0] is None) and (p[0] is None or np.array_equal(p[0], q[0]))


# ---- the mapper -----------------------------------------------------------------------------------------------------------------------------

def _sphere(n, seed, radius, scale, keep=None):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    if keep is not None:
        d = d[keep(d)]
    m = d.shape[0]
    return dict(means3D=(radius * d).contiguous(), rgb_colors=torch.rand(m, 3, generator=g), unnorm_rotations=torch.randn(m, 4, generator=g),
                logit_opacities=torch.full((m, 1), 6.0), log_scales=torch.log(torch.full((m, 3), scale)))


def mapper_scenes():
    """The room the first frame sees -- a dense opaque sphere of radius 3 m around the camera -- and the same room with a patch of opaque
    Gaussians 1 m in front of that surface (radius 2 m, a cap of 20 degrees half angle: about a sixth of a 64 x 48 view of 90 degrees, 30 degrees
    to the side of the first frame's axis -- the side the orbit turns to -- and 6 degrees off it vertically).  From the second frame on the sensor measures the patch; the map, built from the
    first frame, still renders the wall 1 m behind it -- the pixels get_high_loss_samples flags (rendered depth > measured depth)."""
    wall = _sphere(12000, 3, 3.0, 0.12)
    yaw, pitch = np.deg2rad(-30.0), np.deg2rad(6.0)
    axis = torch.tensor([np.sin(yaw) * np.cos(pitch), np.sin(pitch), np.cos(yaw) * np.cos(pitch)], dtype=torch.float32)
    patch = _sphere(40000, 4, 2.0, 0.06, keep=lambda d: (d @ axis) > np.cos(np.deg2rad(20.0)))
    return wall, {k: torch.cat([wall[k], patch[k]]) for k in wall}


def check_mapper(device, frames=3, W=64, H=48):
    """SplatMapper(high_loss_target=True) over a 64 x 48 orbit: see mapper_scenes.  The pose equals target_from_high_loss_clusters on the
    restatement of the mapper's own render; the mask equals high_loss_samples_mask on that render; and a mapper that runs the same frames with
    the flag off ends with bit-identical parameters (the step reads the map, it never writes it).  The second mapper takes over a copy of the
    first one's state after frame 0, so that both start from one map (the blend's backward sums floats in an order that differs from run to run on
    the device)."""
    import copy
    from activesplat_amd.mapper import SplatMapper
    wall, wall_and_patch = mapper_scenes()
    first = list(syn.orbit_sequence(wall, 1, W, H, device))
    later = list(syn.orbit_sequence(wall_and_patch, frames, W, H, device))[1:]
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=frames, high_loss_target=True), device=device)
    assert mp.high_loss_samples_pose_c2w is None
    mp.run(first[0])
    assert mp.high_loss_samples_pose_c2w is None and mp.high_loss_mask is None and mp.high_loss_grid is None     # no map existed before frame 0
    off = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=frames), device=device)
    assert not off.cfg["high_loss_target"]
    off.params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in mp.params.items()}
    off.variables = {k: (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in mp.variables.items()}
    off.keyframe_list, off.selected_keyframes = list(mp.keyframe_list), list(mp.selected_keyframes)
    off.gt_w2c_all_frames, off._pose_host = list(mp.gt_w2c_all_frames), dict(mp._pose_host)
    assert frames < mp.cfg["map_every"]                  # (no frame behind frame 0 maps: neither mapper needs its optimiser again)
    poses = 0
    for fr in later:
        mp.run(fr)
        off.run(fr)
        assert mp._high_loss_pending is not None         # run() left the answer on the device
        view = SplatMapper._w2c_host(torch.as_tensor(fr["quat"]).reshape(4), torch.as_tensor(fr["position"]).reshape(3))
        _, depth, opacity = mp.render_rgbd(view)
        want_mask = pixel_rule(depth[0].cpu().numpy(), opacity[0].cpu().numpy(), fr["depth"][0].cpu().numpy())
        want_grid, _ = resize_int(want_mask, 90, 90)
        r = cc.restate(want_grid, 0.0, 5, 10)
        c2w = np.linalg.inv(view.numpy().astype(np.float64))
        want = VIS.target_from_high_loss_clusters(c2w, float(want_grid.sum()), r["count"], r["sum_row"], r["sum_col"], 25)
        restated, _ = restate_target(want_grid, c2w)
        got = mp.high_loss_samples_pose_c2w
        print(f"[high-loss mapper] frame {fr['id']}: {int(want_mask.sum())} of {W * H} pixels flagged, {int(want_grid.sum())} grid pixels, "
              f"{r['n_clusters']} clusters {list(r['count'])}, pose {'yes' if got is not None else 'none'}")
        assert want is not None and restated is not None and np.array_equal(want, restated)
        assert got is not None and np.array_equal(got, want)
        assert mp._high_loss_pending is None and mp.high_loss_samples_pose_c2w is got        # kept for the frame
        assert W * H / 12 < int(want_mask.sum()) < W * H / 3
        assert np.array_equal(mp.high_loss_mask.cpu().numpy(), want_mask) and np.array_equal(mp.high_loss_grid.cpu().numpy(), want_grid)
        assert torch.equal(mp.high_loss_mask, mp.high_loss_samples_mask(view, fr["depth"]))
        assert torch.equal(mp.high_loss_mask, off.high_loss_mask) and off.high_loss_samples_pose_c2w is None and off.high_loss_grid is None
        poses += 1
    assert poses == frames - 1
    assert sorted(mp.params) == sorted(off.params)
    for k in mp.params:
        assert torch.equal(mp.params[k].detach(), off.params[k].detach()), k


def check_mapper_tracked(device, W=64, H=48):
    """a TRACKED frame (tracking.use_gt_poses=False): the view is the pose the tracker left in the camera parameters, a device tensor -- it
    travels to the host in the property's one copy, and the answer is the restatement's at that pose"""
    from activesplat_amd.mapper import SplatMapper
    wall, wall_and_patch = mapper_scenes()
    seq = list(syn.orbit_sequence(wall, 1, W, H, device)) + list(syn.orbit_sequence(wall_and_patch, 2, W, H, device))[1:]
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=2, high_loss_target=True, tracking=dict(use_gt_poses=False, tracking_iters=2)),
                     device=device)
    for fr in seq:
        mp.run(fr)
    w2c_host, w2c_dev, _ = mp._high_loss_pending
    assert w2c_host is None and torch.equal(w2c_dev, mp._w2c(1))
    _, depth, opacity = mp.render_rgbd(w2c_dev)
    want_mask = pixel_rule(depth[0].cpu().numpy(), opacity[0].cpu().numpy(), seq[1]["depth"][0].cpu().numpy())
    want, _ = restate_target(resize_int(want_mask, 90, 90)[0], np.linalg.inv(w2c_dev.cpu().numpy().astype(np.float64)))
    got = mp.high_loss_samples_pose_c2w
    assert np.array_equal(mp.high_loss_mask.cpu().numpy(), want_mask)
    assert want is not None and got is not None and np.array_equal(got, want)
