"""Generate tests/golden/hull.npz: scipy's hull volumes for every case of tests/hull_cases.py, and what the reference's own
get_convexhull_volume returns for the three 150 x 360 `global` cases.

Run only where scipy, sklearn and the reference are present:   python tests/golden/make_hull_golden.py
The reference's files never travel: src/mapper/__init__.py is IMPORTED here with sys.modules['cv2'] set to a stub, and only numbers are written.
The stub offers getStructuringElement, dilate, findContours, contourArea and the three constants the function names, all through the numpy
restatement of tests/hull_cases.py (OpenCV is not on this machine: its rules are restated, not run).  Everything else the function does is
its own: sklearn's DBSCAN, its loop over the clusters, its z == 15 skip, its scaling to radians, scipy.spatial.ConvexHull, its two sums.

Per case `key`:  key_scipy     fp64 [B, M]: ConvexHull(points in the reference's units).volume per cluster; 0 for a cluster without 4 points off
                               one plane, for a contour over max_points and beyond the clusters
                 key_contours  int16 [n, 2], key_offsets int64 [B * M + 1]: the (first max_points) contour points (x, y) of every cluster
                 key_ref       fp64 [2]: (last_invisibility, last_volume) of get_convexhull_volume -- the `global` cases only
                 key_ref_volumes fp64 [n_clusters]: the hull.volume the reference computed per cluster (by sklearn's label)
Conditions asserted here for the `global` cases: every cluster's dilation is ONE 8-connected component (so that the contour the stub returns is
the reference's max(contours, key=contourArea)), and every cluster keeps at least 4 points off one plane with a coordinate matrix of rank 3
(so that the reference takes neither its random jitter nor its QhullError branch).
"""
import importlib.util
import os
import sys
import types

import numpy as np
from scipy import ndimage
from scipy.spatial import ConvexHull

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import hull_cases as hc  # noqa: E402

REFERENCE = "/root/reference/src/mapper/__init__.py"
STATE = {}


def stub_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.MORPH_ELLIPSE, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE = 2, 0, 2

    def getStructuringElement(shape, ksize):
        assert shape == cv2.MORPH_ELLIPSE
        kw, kh = ksize
        return np.array([[(r >> j) & 1 for j in range(kw)] for r in hc.ellipse_rows(kh, kw)], np.uint8)

    def dilate(mask, kernel, iterations=1):
        assert iterations == 1 and mask.dtype == np.uint8
        ys, xs = np.nonzero(mask)
        STATE["cluster"] = int(STATE["labels"][ys[0], xs[0]])
        rows = [sum(int(v) << j for j, v in enumerate(row)) for row in kernel]
        out = hc.dilate(mask > 0, rows, kernel.shape[1])
        assert ndimage.label(out, structure=np.ones((3, 3)))[1] == 1, "a cluster dilated to more than one component"
        return (out * 255).astype(np.uint8)

    def findContours(image, mode, method):
        assert mode == cv2.RETR_EXTERNAL and method == cv2.CHAIN_APPROX_SIMPLE
        contour = hc.trace(image > 0)
        STATE["contours"][STATE["cluster"]] = contour
        return (np.array(contour, np.int32).reshape(-1, 1, 2),), None

    def contourArea(contour):
        p = contour.reshape(-1, 2).astype(np.float64)
        return 0.5 * abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))

    cv2.getStructuringElement, cv2.dilate, cv2.findContours, cv2.contourArea = getStructuringElement, dilate, findContours, contourArea
    return cv2


def reference_module():
    sys.modules["cv2"] = stub_cv2()
    spec = importlib.util.spec_from_file_location("reference_mapper", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def recording_hull(points):
        p = np.asarray(points, np.float64)
        assert len(p) >= 4 and np.linalg.matrix_rank(p) == 3 and np.linalg.matrix_rank(p - p[0]) == 3, "a cluster without 4 points off one plane"
        hull = ConvexHull(points)
        STATE["volumes"][STATE["cluster"]] = hull.volume
        return hull
    mod.ConvexHull = recording_hull
    return mod


def scipy_volume(pts, xs, ys):
    """ConvexHull(...).volume of restated points [n, 3] (pixel units) in the reference's units; 0 without 4 points off one plane"""
    if len(pts) < 4 or np.linalg.matrix_rank(pts - pts[0]) < 3:
        return 0.0
    return float(ConvexHull(pts * np.array([xs, ys, 1.0])).volume)


def add(out, key, refs, M, W, H, max_points=1024):
    xs, ys = np.deg2rad(360 / W), np.deg2rad(150 / H)
    vol = np.zeros((len(refs), M))
    contours, offsets = [], [0]
    for b, ref in enumerate(refs):
        for c in range(M):
            pts = ref["contours"][c] if c < len(ref["contours"]) else []
            contours += pts
            offsets.append(len(contours))
            if c < len(ref["contours"]) and ref["n_points"][c] <= max_points:
                vol[b, c] = scipy_volume(ref["points"][c], xs, ys)
                mine = ref["volume"][c]
                assert abs(mine - vol[b, c]) <= hc.VOL_ATOL + hc.VOL_RTOL * abs(vol[b, c]), f"{key}[{b}] cluster {c}: restated {mine!r}, scipy {vol[b, c]!r}"
        print(f"{key}[{b}]: status {ref['status']}, points {ref['n_points'][:len(ref['contours'])].tolist()}, scipy volumes {vol[b][:len(ref['contours'])]}")
    out[key + "_scipy"] = vol
    out[key + "_contours"] = np.array(contours, np.int16).reshape(-1, 2)
    out[key + "_offsets"] = np.array(offsets, np.int64)


def main():
    out = {}
    for name, k in hc.small_cases().items():
        _, refs = hc.reference(name)
        add(out, name, refs, k["M"], 40, 24, k["max_points"])
        if name in hc.ZERO_VOLUME:
            assert (out[name + "_scipy"] == 0).all(), name
        else:
            assert all((out[name + "_scipy"][b][:min(k["n"][b], k["M"])] > 0).all() for b in range(len(refs))), name
    ref_mod = reference_module()
    for seed in hc.cc.SEEDS:
        key = f"global_{seed}"
        values, r, depth, ref = hc.reference_global(seed)
        add(out, key, [ref], 256, 360, 150)
        STATE.update(labels=r["labels"], contours={}, volumes={})
        inv = np.float32(1) - values
        last_invisibility, last_volume = ref_mod.get_convexhull_volume(depth[..., None], inv, np.eye(3))
        n = r["n_clusters"]
        assert sorted(STATE["volumes"]) == list(range(n)) and sorted(STATE["contours"]) == list(range(n)), (key, sorted(STATE["volumes"]), n)
        for c in range(n):
            assert STATE["contours"][c] == ref["contours"][c]
            assert STATE["volumes"][c] == out[key + "_scipy"][0, c], (key, c)
        z = np.concatenate([p[:, 2] for p in ref["points"]])
        kept, emitted = sum(len(p) for p in ref["points"]), int(ref["n_points"].sum())
        print(f"{key}: {n} clusters, reference returned ({last_invisibility!r}, {last_volume!r}); restated sums ({ref['sum_invisibility']!r}, "
              f"{ref['sum_volume']!r}); {emitted - kept} of {emitted} points skipped at z == 15, {int((z == 0).sum())} points on the z = 0 plateau")
        if hc.GLOBAL_DEPTH[seed] == "zero":
            assert (z == 0).sum() >= 10, "no z = 0 plateau under the contours"
        if hc.GLOBAL_DEPTH[seed] == "fifteen":
            assert emitted - kept >= 10, "no contour point at the skipped depth"
        assert abs(last_volume - ref["sum_volume"]) <= hc.VOL_ATOL + hc.VOL_RTOL * abs(last_volume)
        assert abs(last_invisibility - ref["sum_invisibility"]) <= hc.SUM_RTOL * abs(last_invisibility)
        out[key + "_ref"] = np.array([last_invisibility, last_volume], np.float64)
        out[key + "_ref_volumes"] = np.array([STATE["volumes"][c] for c in range(n)], np.float64)
    path = os.path.join(HERE, "hull.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
