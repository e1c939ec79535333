"""Shared checks of the on-device cluster hull volumes (activesplat_amd/visibility.py cluster_hulls / global_invisibility_scores, gs_cluster_hulls):
run on the host-emulated kernels by tests/test_hull.py and on the MI355X by tests/test_gpu_hull.py.

References
* `restate` below: the rule a-f of include/gsplat_hip.h (gs_cluster_hulls) in numpy -- dilation by shifted ORs, the border following as a Python
  loop, an incremental hull in fp64 with the header's determinant, the two sums in fp64.
* tests/golden/hull.npz, written by tests/golden/make_hull_golden.py: for every case of this file scipy.spatial.ConvexHull(points).volume
  (scipy 1.15.3) of every cluster that keeps 4 points off one plane, on the restated contour's points in the reference's radian units; for the
  three `global` cases also what the reference's own get_convexhull_volume (src/mapper/__init__.py:8-90) returned and the hull volumes it
  computed, with cv2 replaced by a stub that offers getStructuringElement, dilate, findContours and contourArea through this file's restatement:
  its DBSCAN (sklearn), its loop, its z == 15 skip, its scaling, its ConvexHull and its two sums are the reference's own.  OpenCV itself was
  never run: the dilation and border rules restate its documented behaviour, pinned here by the known answers of tests/test_hull.py.
* the depth images are polynomials of the pixel coordinates evaluated in fp64 with + and * only, so every machine rebuilds the same fp32 bits.

Tolerances (none of them comes from the code under test)
* contour points, n_points, status: exact.
* volume, sum_volume against scipy: rtol 1e-9, atol 1e-12 (both sides fp64; the CPU prototype of the rule measured 7e-14, the margin covers
  another order of operations).  Clusters without 4 points off one plane: exactly 0.
* sum_invisibility: relative cluster_cases.SUM_RTOL = 1e-5 (the per-cluster invisibility sum is gs_grid_dbscan's fp32 one).
"""
import os

import numpy as np
import torch

from activesplat_amd import visibility as VIS
from tests import cluster_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hull.npz")
VOL_RTOL, VOL_ATOL = 1e-9, 1e-12
SUM_RTOL = cc.SUM_RTOL
SKIP = 15.0
DIRS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))
OVERFLOW, NONFINITE, TRUNCATED, FACES = 1, 2, 4, 8

# ---- the rule, restated -----------------------------------------------------------------------------------------------------------------


def ellipse_rows(kh=15, kw=15):
    """getStructuringElement(MORPH_ELLIPSE, (kw, kh)) as the issue restates it, independent of visibility.ellipse_footprint -> list of kh ints"""
    r, c = kh // 2, kw // 2
    rows = []
    for i in range(kh):
        dy = i - r
        dx = int(round(c * np.sqrt((r * r - dy * dy) / (r * r)))) if r else 0          # (OpenCV: inv_r2 = 0 for r = 0)
        rows.append(sum(1 << j for j in range(max(c - dx, 0), min(c + dx + 1, kw))))
    return rows


def dilate(mask, rows, kw):
    """dil(y, x) = OR of mask(y + i - ay, x + j - ax) over the set cells, 0 outside the image"""
    kh = len(rows)
    ay, ax = kh // 2, kw // 2
    out = np.zeros(mask.shape, bool)
    for i, r in enumerate(rows):
        for j in range(kw):
            if (int(r) >> j) & 1:
                out |= cc._shift(mask.astype(bool), i - ay, j - ax, False)
    return out


def trace(dil):
    """the outer border of the component of the first set pixel, CHAIN_APPROX_SIMPLE -> list of (x, y)"""
    H, W = dil.shape
    flat = np.flatnonzero(dil)
    if not len(flat):
        return []
    y0, x0 = divmod(int(flat[0]), W)

    def at(x, y):
        return 0 <= x < W and 0 <= y < H and bool(dil[y, x])
    s = 4
    while True:
        s = (s - 1) & 7
        if at(x0 + DIRS[s][0], y0 + DIRS[s][1]):
            break
        if s == 4:
            return [(x0, y0)]
    x1, y1 = x0 + DIRS[s][0], y0 + DIRS[s][1]
    out, px, py, prev = [], x0, y0, s ^ 4
    for _ in range(4 * H * W + 8):
        sp = s
        for _k in range(8):
            sp = (sp + 1) & 7
            qx, qy = px + DIRS[sp][0], py + DIRS[sp][1]
            if at(qx, qy):
                break
        else:
            raise AssertionError("a border pixel without a set neighbour")
        if sp != prev:
            out.append((px, py))
            prev = sp
        if (qx, qy) == (x0, y0) and (px, py) == (x1, y1):
            return out
        px, py, s = qx, qy, (sp + 4) & 7
    raise AssertionError("the border following did not close")


def orient(a, b, c, d):
    """det [b - a; c - a; d - a], the header's expression in fp64 (numpy never contracts); every argument [3] or [n, 3]"""
    a, b, c, d = (np.asarray(v, np.float64) for v in (a, b, c, d))
    bx, by, bz = (b - a)[..., 0], (b - a)[..., 1], (b - a)[..., 2]
    cx, cy, cz = (c - a)[..., 0], (c - a)[..., 1], (c - a)[..., 2]
    dx, dy, dz = (d - a)[..., 0], (d - a)[..., 1], (d - a)[..., 2]
    return (bx * (cy * dz - cz * dy) - by * (cx * dz - cz * dx)) + bz * (cx * dy - cy * dx)


def hull_volume(pts):
    """incremental hull of pts [n, 3] fp64 (pixel units) -> volume; 0 without four points off one plane"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    if n < 4:
        return 0.0
    P0 = pts[0]
    i1 = next((i for i in range(n) if (pts[i] != P0).any()), None)
    if i1 is None:
        return 0.0
    i2 = next((i for i in range(n) if np.any(np.cross(pts[i1] - P0, pts[i] - P0) != 0)), None)
    if i2 is None:
        return 0.0
    d = orient(P0, pts[i1], pts[i2], pts)
    nz = np.flatnonzero(d != 0)
    if not len(nz):
        return 0.0
    i3 = int(nz[0])
    if d[i3] > 0:
        i1, i2 = i2, i1
    faces = [(0, i1, i2), (i1, 0, i3), (i2, i1, i3), (0, i2, i3)]
    for ip in range(1, n):
        if ip in (i1, i2, i3):
            continue
        F = np.array(faces)
        vis = orient(pts[F[:, 0]], pts[F[:, 1]], pts[F[:, 2]], pts[ip]) > 0
        if not vis.any():
            continue
        edges = [(f[e], f[(e + 1) % 3]) for f, v in zip(faces, vis) if v for e in range(3)]
        have = set(edges)
        faces = [f for f, v in zip(faces, vis) if not v] + [(u, v, ip) for u, v in edges if (v, u) not in have]
        assert len(faces) <= 2 * n - 4
    F = np.array(faces)
    return float(orient(P0, pts[F[:, 0]], pts[F[:, 1]], pts[F[:, 2]]).sum() / 6.0)


def restate_cluster(labels, depth, c, rows, kw, skip=SKIP, max_points=1024):
    """a-d for one cluster -> (the whole contour [(x, y)], the kept ones of its first max_points points [n, 3] fp64 in pixel units, whether one
    of those had a depth that is not finite)"""
    contour = trace(dilate(labels == c, rows, kw))
    stored = contour[:max_points]
    z = np.array([depth[y, x] for x, y in stored], np.float32)
    finite = np.isfinite(z)
    keep = finite & (z != np.float32(skip))
    pts = np.array([(x, y, float(zz)) for (x, y), zz, k in zip(stored, z, keep) if k], np.float64).reshape(-1, 3)
    return contour, pts, bool((~finite).any())


def restate(labels, depth, n_clusters, sum_value, max_clusters=256, rows=None, kw=15, skip=SKIP, x_scale=None, y_scale=None, max_points=1024):
    """a-f for ONE image -> dict(volume [M] fp64, n_points [M], contours (list of [(x, y)]), points (list of [n, 3]), sum_volume,
    sum_invisibility, status)"""
    H, W = labels.shape
    rows = ellipse_rows() if rows is None else rows
    xs = np.deg2rad(360 / W) if x_scale is None else x_scale
    ys = np.deg2rad(150 / H) if y_scale is None else y_scale
    M = max_clusters
    m = min(int(n_clusters), M)
    volume, n_points, contours, points = np.zeros(M), np.zeros(M, np.int64), [], []
    status = TRUNCATED if n_clusters > M else 0
    for c in range(m):
        contour, pts, nonfinite = restate_cluster(labels, depth, c, rows, kw, skip, max_points)
        n_points[c] = len(contour)
        contours.append(contour[:max_points])
        points.append(pts)
        status |= NONFINITE if nonfinite else 0
        if len(contour) > max_points:
            status |= OVERFLOW
        else:
            volume[c] = hull_volume(pts) * (xs * ys)
    sv = np.asarray(sum_value, np.float64)
    return dict(volume=volume, n_points=n_points, contours=contours, points=points, status=status, sum_volume=float(np.sum(volume[:m])),
                sum_invisibility=float(sum(sv[c] * volume[c] for c in range(m))))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def poly_depth(H, W, kind="smooth"):
    """fp32 [H, W]: a curved surface from + and * in fp64 (the same bits on every machine) with a bump per 16 columns and 12 rows, so that the
    contour of a blob a few dozen pixels wide is far from one plane.  `zero`: 3 subtracted and clamped at 0 (a z = 0 plateau); `fifteen`:
    a patch of 6 x 4 pixels at exactly the skipped value in every 16 x 12 cell"""
    y, x = np.indices((H, W)).astype(np.float64)
    u, v = x / W, y / H
    tx, ty = (x % 16) / 16, (y % 12) / 12
    z = 1.5 + 2.0 * u * u + 1.25 * v + 0.75 * u * v + 1.5 * tx * (1 - tx) + 1.0 * ty * (1 - ty)
    if kind == "zero":
        z = np.maximum(z - 3.0, 0.0)
    elif kind == "fifteen":
        z = np.where((x % 16 >= 5) & (x % 16 <= 10) & (y % 12 >= 4) & (y % 12 <= 7), 15.0, z)
    else:
        assert kind == "smooth"
    return z.astype(np.float32)


GLOBAL_DEPTH = {0: "smooth", 1: "zero", 2: "fifteen"}


def blocks(*cols, H=24, W=40):
    """labels with one 7 x 7 block (rows 4-10) per entry of cols, numbered in order"""
    lab = np.full((H, W), -2, np.int32)
    for c, x in enumerate(cols):
        lab[4:11, x:x + 7] = c
    return lab


def plus():
    lab = np.full((24, 40), -2, np.int32)
    lab[4, 1:8] = 0
    lab[1:8, 4] = 0
    return lab


def _case(labels, depth, n=None, M=4, rows=None, kw=15, max_points=1024, depth_base=None):
    """depth_base: the padded array that depth is the [:, :, 3:43] view of (the device test rebuilds that strided view)"""
    labels = labels if labels.ndim == 3 else labels[None]
    depth = depth if depth.ndim == 3 else depth[None]
    n = [int(l.max()) + 1 if (l >= 0).any() else 0 for l in labels] if n is None else n
    # the per-cluster invisibility sums the call multiplies with: positive fp32 values that differ per cluster
    sv = np.array([[np.float32(10.5 + 3.25 * c + b) if c < min(n[b], M) else 0 for c in range(M)] for b in range(len(labels))], np.float32)
    return dict(labels=labels, depth=depth, n=np.array(n, np.int32), sum_value=sv, M=M, rows=rows, kw=kw, max_points=max_points, depth_base=depth_base)


def small_cases():
    """the hand-made 24 x 40 cases: name -> case"""
    d = poly_depth(24, 40)
    corner = np.full((24, 40), -2, np.int32)
    corner[0, 0] = 0
    pixel = np.full((24, 40), -2, np.int32)
    pixel[15, 15] = 0
    overlap = blocks(4, 16)
    out = dict(corner=_case(corner, d), whole=_case(np.zeros((24, 40), np.int32), d), overlap=_case(overlap, d),
               plus1x1=_case(plus(), d, rows=[1], kw=1), pixel1515=_case(pixel, d))
    # B = 3: a strided depth view, an image without clusters, an image with more clusters than the table has rows
    wide = np.stack([np.pad(poly_depth(24, 40) + np.float32(b), ((0, 0), (3, 5)), constant_values=99.0) for b in range(3)])
    out["batch3"] = _case(np.stack([overlap, np.full((24, 40), -2, np.int32), blocks(2, 14, 28)]), wide[:, :, 3:43], n=[2, 0, 3], M=2, depth_base=wide)
    out["constant"] = _case(overlap, np.full((24, 40), 2.0, np.float32))
    out["plane"] = _case(overlap, (0.5 * np.indices((24, 40))[1] + 1.0).astype(np.float32))
    few = np.full((24, 40), np.float32(SKIP))
    contour0 = trace(dilate(overlap == 0, ellipse_rows(), 15))
    for x, y in contour0[:3]:
        few[y, x] = d[y, x]
    out["few"] = _case(overlap, few)
    nan = d.copy()
    nan[contour0[2][1], contour0[2][0]] = np.nan
    out["nan"] = _case(overlap, nan)
    out["overflow"] = _case(overlap, d, max_points=8)
    return out


ZERO_VOLUME = ("constant", "plane", "few", "overflow")


def global_case(seed):
    """one `global` random case of cluster_cases with its synthetic depth -> (values fp32 [150, 360], restated clustering, depth)"""
    values, r = cc.reference("global", seed)
    return values, r, poly_depth(150, 360, GLOBAL_DEPTH[seed])


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(GOLDEN) as z:
            _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN


def golden_contours(key, b, c):
    g = golden()
    off = g[key + "_offsets"]
    M = g[key + "_scipy"].shape[1]
    i = b * M + c
    return [tuple(p) for p in g[key + "_contours"][off[i]:off[i + 1]].astype(int).tolist()]


_REF = {}


def reference(name):
    """the restatement of one small case, per image; computed once per process"""
    if name not in _REF:
        k = small_cases()[name]
        _REF[name] = (k, [restate(k["labels"][b], k["depth"][b], k["n"][b], k["sum_value"][b], k["M"], k["rows"], k["kw"], max_points=k["max_points"])
                          for b in range(len(k["labels"]))])
    return _REF[name]


def reference_global(seed):
    key = f"global_{seed}"
    if key not in _REF:
        values, r, depth = global_case(seed)
        _REF[key] = (values, r, depth, restate(r["labels"], depth, r["n_clusters"], r["sum_value"], 256))
    return _REF[key]


# ---- running the device and comparing -------------------------------------------------------------------------------------------------------

def clusters_of(device, n, sum_value):
    """a GridClusters that carries what cluster_hulls reads: n_clusters and sum_value"""
    return VIS.GridClusters(None, torch.from_numpy(np.asarray(n, np.int32)).to(device), None, None, None, None,
                            torch.from_numpy(np.asarray(sum_value, np.float32)).to(device), None)


def run_case(device, k):
    if k["depth_base"] is not None:
        depth = torch.from_numpy(k["depth_base"]).to(device)[:, :, 3:43]
        assert not depth.is_contiguous() and depth.stride() == (24 * 48, 48, 1)
    else:
        depth = torch.from_numpy(k["depth"]).to(device)
    fp = None if k["rows"] is None else np.array(k["rows"], np.uint32)
    h = VIS.cluster_hulls(torch.from_numpy(k["labels"]).to(device), depth, clusters_of(device, k["n"], k["sum_value"]), footprint=fp,
                          kw=None if fp is None else k["kw"], max_points=k["max_points"], contours=True)
    return {f: getattr(h, f).cpu().numpy() for f in h._fields}


def compare(got, ref, b, key, what, sum_value=None):
    """image b of a device result against its restatement (integers exact) and against the fixture's scipy volumes"""
    g = {f: v[b] for f, v in got.items()}
    M = g["volume"].shape[0]
    m = len(ref["contours"])
    assert np.array_equal(g["n_points"], ref["n_points"][:M]), (what, g["n_points"][:m + 1], ref["n_points"][:m + 1])
    assert int(g["status"]) == ref["status"], (what, int(g["status"]), ref["status"])
    for c in range(m):
        n = len(ref["contours"][c])
        assert [tuple(p) for p in g["contour_xy"][c, :n].tolist()] == ref["contours"][c], (what, c)
        assert (g["contour_xy"][c, n:] == 0).all(), (what, c)
    scipy_volume = golden()[key + "_scipy"][b]
    err = np.abs(g["volume"] - scipy_volume)
    rel = err / np.maximum(np.abs(scipy_volume), 1e-300)
    print(f"{what}: {m} clusters, points {ref['n_points'][:m].tolist()}, status {ref['status']}, volume {g['sum_volume']:.6e}, "
          f"max relative error against scipy {rel[scipy_volume != 0].max() if (scipy_volume != 0).any() else 0:.2e}")
    assert (err <= VOL_ATOL + VOL_RTOL * np.abs(scipy_volume)).all(), (what, g["volume"][:m], scipy_volume[:m])
    assert (g["volume"][m:] == 0).all() and (g["n_points"][m:] == 0).all(), what
    assert abs(g["sum_volume"] - scipy_volume[:m].sum()) <= VOL_ATOL + VOL_RTOL * abs(scipy_volume[:m].sum()), what
    sv = ref["sum_invisibility"]
    assert abs(g["sum_invisibility"] - sv) <= SUM_RTOL * abs(sv), (what, g["sum_invisibility"], sv)


def check_small(device, name):
    k, refs = reference(name)
    got = run_case(device, k)
    for b, ref in enumerate(refs):
        compare(got, ref, b, name, f"{name}[{b}]")
        if name in ZERO_VOLUME:
            assert (got["volume"][b] == 0).all() and got["sum_volume"][b] == 0 and got["sum_invisibility"][b] == 0, name
    if name == "overflow":
        assert (got["status"] & OVERFLOW).all() and (refs[0]["n_points"][:2] > 8).all()
    if name == "nan":
        assert got["status"][0] == NONFINITE and got["volume"][0, 0] > 0
    if name == "batch3":
        assert got["status"].tolist() == [0, 0, TRUNCATED] and got["sum_volume"][1] == 0 and (got["n_points"][1] == 0).all()
    if name == "plus1x1":
        assert refs[0]["contours"][0] == PLUS_CONTOUR


RECTANGLE_CONTOUR = [(2, 1), (2, 3), (5, 3), (5, 1)]
PLUS_CONTOUR = [(4, 1), (4, 3), (3, 4), (1, 4), (3, 4), (4, 5), (4, 7), (4, 5), (5, 4), (7, 4), (5, 4), (4, 3)]
PIXEL1515_HEAD = [(15, 8), (14, 9), (11, 9), (9, 11), (9, 12), (8, 13), (8, 17), (9, 18)]
PIXEL1515_TAIL = [(21, 11), (19, 9), (16, 9)]


def check_global(device, seed):
    """grid_dbscan + cluster_hulls on one 150 x 360 random field with its synthetic depth, against the restatement, scipy's volumes and what the
    reference's get_convexhull_volume returned"""
    values, r, depth, ref = reference_global(seed)
    key = f"global_{seed}"
    g = VIS.grid_dbscan(torch.from_numpy(np.array(values)).to(device), 0.8, 5, 25, complement=True)
    h = VIS.cluster_hulls(g.labels, torch.from_numpy(depth).to(device).unsqueeze(-1), g, contours=True)
    got = {f: getattr(h, f).cpu().numpy()[None] for f in h._fields}
    assert np.array_equal(g.labels.cpu().numpy(), r["labels"])
    compare(got, ref, 0, key, key)
    last_invisibility, last_volume = golden()[key + "_ref"]
    assert abs(got["sum_volume"][0] - last_volume) <= VOL_ATOL + VOL_RTOL * abs(last_volume), (key, got["sum_volume"][0], last_volume)
    assert abs(got["sum_invisibility"][0] - last_invisibility) <= SUM_RTOL * abs(last_invisibility), (key, got["sum_invisibility"][0], last_invisibility)
    assert got["status"][0] == 0


def check_refusals(device):
    from activesplat_amd import _lib
    lib = _lib.get()
    k = small_cases()["overlap"]
    lab, dep = torch.from_numpy(k["labels"]).to(device), torch.from_numpy(k["depth"]).to(device)
    cl = clusters_of(device, k["n"], k["sum_value"])
    for kw, text in ((dict(max_points=3), "max_points"), (dict(max_points=4097), "max_points"), (dict(footprint=np.ones(4, np.uint32), kw=1), "odd kh and kw"),
                     (dict(footprint=np.ones(17, np.uint32), kw=1), "odd kh and kw"), (dict(footprint=np.ones(3, np.uint32), kw=2), "odd kh and kw"),
                     (dict(footprint=np.array([1, 8, 1], np.uint32), kw=3), "beyond kw"), (dict(x_scale=float("nan")), "finite")):
        try:
            VIS.cluster_hulls(lab, dep, cl, **kw)
        except Exception as e:
            assert text in str(e) and "gs_cluster_hulls" in str(e), (kw, str(e))
            assert text.encode() in lib.gs_last_error()
        else:
            raise AssertionError(f"cluster_hulls accepted {list(kw)}")
    with np.testing.assert_raises(ValueError):
        VIS.cluster_hulls(lab, dep[:, :10], cl)
    fp = np.ones(1, np.uint32)
    assert lib.gs_cluster_hulls(1, 24, 40, None, None, 40, 960, None, None, 4, fp.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint32)), 1, 1, 15.0, 1.0, 1.0, 64,
                                None, None, None, None, None, None, None, None) == 1                                         # GS_EINVAL
    assert b"gs_cluster_hulls" in lib.gs_last_error()
    # the entry point itself with ONE argument wrong at a time: the same call with nothing wrong is taken first
    B, H, W, M, P = 1, 24, 40, 4, 64
    layout = _lib.GsHullLayout()
    assert lib.gs_cluster_hulls_layout(B, H, W, M, P, _lib.C.byref(layout)) == 0
    ws = torch.zeros(int(layout.total_bytes) + 8, dtype=torch.uint8, device=device)
    assert ws.data_ptr() % 8 == 0
    out = dict(volume=torch.zeros(B, M, dtype=torch.float64, device=device), n_points=torch.zeros(B, M, dtype=torch.int32, device=device),
               sum_volume=torch.zeros(B, dtype=torch.float64, device=device), sum_invisibility=torch.zeros(B, dtype=torch.float64, device=device),
               status=torch.zeros(B, dtype=torch.int32, device=device))
    good = dict(labels=lab.data_ptr(), depth=dep.data_ptr(), row_stride=W, image_stride=H * W, n_clusters=cl.n_clusters.data_ptr(),
                sum_value=cl.sum_value.data_ptr(), workspace=ws.data_ptr(), contour_xy=None, **{f: t.data_ptr() for f, t in out.items()})
    assert lab.shape == (B, H, W) and dep.shape == (B, H, W) and dep.is_contiguous() and cl.sum_value.shape == (B, M)

    def call(**wrong):
        a = dict(good, **wrong)
        return lib.gs_cluster_hulls(B, H, W, a["labels"], a["depth"], a["row_stride"], a["image_stride"], a["n_clusters"], a["sum_value"], M,
                                    fp.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint32)), 1, 1, 15.0, 1.0, 1.0, P, a["workspace"], a["volume"],
                                    a["n_points"], a["contour_xy"], a["sum_volume"], a["sum_invisibility"], a["status"], _lib.stream_ptr(lab.device))
    assert call() == 0
    wrongs = [dict(row_stride=W - 1), dict(image_stride=-1), dict(workspace=ws.data_ptr() + 4)]
    wrongs += [{f: None} for f in ("labels", "depth", "n_clusters", "sum_value", "workspace", "volume", "n_points", "sum_volume", "sum_invisibility", "status")]
    for wrong in wrongs:
        assert call(**wrong) == 1, wrong                                                                                     # GS_EINVAL
        assert b"gs_cluster_hulls: null pointer" in lib.gs_last_error(), wrong
    assert call() == 0


def check_repeatable(device):
    values, r, depth, _ = reference_global(0)
    v = torch.from_numpy(np.stack([values, values[::-1].copy()])).to(device)
    d = torch.from_numpy(np.stack([depth, depth[::-1].copy()])).to(device)
    g = VIS.grid_dbscan(v, 0.8, 5, 25, complement=True)
    a, b = VIS.cluster_hulls(g.labels, d, g, contours=True), VIS.cluster_hulls(g.labels, d, g, contours=True)
    for f in a._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f           # (bit-identical, the fp64 volumes and sums included)
    assert float(a.sum_volume.min()) > 0


# ---- the query --------------------------------------------------------------------------------------------------------------------------

def score_scene(device):
    """an opaque sphere of Gaussians around the nodes with three holes: every panorama has three blobs of invisibility whose dilated borders lie
    on the sphere, at depths that vary with the node's position (a sparse shell gives one cluster over the whole panorama, whose four corner
    points span no volume)"""
    return cc.cap_params(device, 100.0, 10.0, 25.0, n=5000, scale=0.15, more_holes=((-120.0, -20.0, 17.0), (10.0, 30.0, 12.0)))


def check_scores(device, K, zero_at=None):
    """global_invisibility_scores against the restatement applied to what global_invisibility_nodes returns on the same device"""
    params = score_scene(device)
    c2w = cc.base_pose()
    pos = cc.node_positions(K, zero_at=zero_at)
    inv, vol = VIS.global_invisibility_scores(params, c2w, pos)
    nodes = VIS.global_invisibility_nodes(params, c2w, pos)
    assert inv.shape == (K,) and vol.shape == (K,) and inv.dtype == np.float64 and vol.dtype == np.float64
    seen = 0
    for k, d in enumerate(nodes):
        if d is None:
            assert k == zero_at and inv[k] == 0 and vol[k] == 0
            continue
        ref = restate(d["labels"], d["depth"][..., 0], d["n_clusters"], d["sum_value"])
        seen += int((ref["volume"] > 0).sum())
        print(f"scores K={K} node {k}: {d['n_clusters']} clusters, volume {vol[k]:.6e} (restated {ref['sum_volume']:.6e}), invisibility {inv[k]:.6e} "
              f"(restated {ref['sum_invisibility']:.6e})")
        assert ref["status"] == 0
        assert abs(vol[k] - ref["sum_volume"]) <= VOL_ATOL + VOL_RTOL * abs(ref["sum_volume"]), (k, vol[k], ref["sum_volume"])
        assert abs(inv[k] - ref["sum_invisibility"]) <= SUM_RTOL * abs(ref["sum_invisibility"]), (k, inv[k], ref["sum_invisibility"])
    assert seen > 0, "no cluster with a volume in any panorama: the scene does not exercise the query"
    return params, c2w, pos


def check_scores_raise_when_truncated(device):
    params = score_scene(device)
    try:
        VIS.global_invisibility_scores(params, cc.base_pose(), cc.node_positions(2), max_clusters=1)
    except RuntimeError as e:
        assert "truncated" in str(e)
    else:
        raise AssertionError("a panorama with more clusters than the table has rows was scored silently")


def check_mapper(device, frames=2, W=64, H=48):
    """SplatMapper.global_invisibility_scores after a few mapped frames: the module's function on the mapper's parameters"""
    from activesplat_amd import synthetic as syn
    from activesplat_amd.mapper import SplatMapper
    gt = syn.shell_scene(3000, seed=2, W=W, H=H)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=frames), device=device)
    for fr in syn.orbit_sequence(gt, frames, W, H, device):
        mp.run(fr)
    c2w, pos = cc.base_pose(), cc.node_positions(2)
    got, want = mp.global_invisibility_scores(c2w, pos), VIS.global_invisibility_scores(mp.params, c2w, pos)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    print(f"[hull mapper] {mp.params['means3D'].shape[0]} Gaussians: invisibility {got[0]}, volume {got[1]}")
    # two mapped frames cover a few percent of a panorama: its one cluster dilates to the whole image, whose four corners lie at depth 0 and span no
    # volume.  So that the method is also compared on scores that are not 0, the same mapper then holds the sphere with three holes.
    assert (got[1] == 0).all()
    mp.params = score_scene(device)
    got, want = mp.global_invisibility_scores(c2w, pos, max_clusters=8), VIS.global_invisibility_scores(mp.params, c2w, pos, max_clusters=8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[1] > 0).all() and (got[0] > 0).all()
