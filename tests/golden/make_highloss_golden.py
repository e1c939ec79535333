"""Generate tests/golden/highloss.npz: sklearn's DBSCAN labels for the grid of every case of tests/highloss_cases.py.

Run only where sklearn is present:   python tests/golden/make_highloss_golden.py
The reference's own method (get_high_loss_samples, src/mapper/splatam/__init__.py:184-252) cannot be imported: its module needs cv2, and the
method itself calls cv2.resize.  What is recorded is the line of that method that the kernels replace,
    DBSCAN(eps=5, min_samples=10).fit_predict(np.column_stack(np.where(grid > 0)))
on the grids the integer resize rule (highloss_cases.resize_int) gives for the resize cases, and on the 90 x 90 masks of the decision cases.
The fixture holds only masks and labels.

Per grid `key`:  key_grid     the grid's ones, np.packbits of the row-major [grid_h, grid_w] booleans
                 key_sklearn  int16, one per grid pixel that is 1 (-1 noise)
Every grid is also run through cluster_cases.restate here, and the script stops if a single label differs from sklearn's.
"""
import os
import sys

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import cluster_cases as cc  # noqa: E402
from tests import highloss_cases as hc  # noqa: E402


def main():
    out = {}
    for key, grid in hc.golden_grids().items():
        pts = np.column_stack(np.where(grid > 0))
        sk = DBSCAN(eps=5, min_samples=10).fit_predict(pts) if len(pts) else np.zeros(0, np.int64)
        r = cc.restate(grid, 0.0, 5, 10)
        assert np.array_equal(r["mask"], grid > 0)
        assert np.array_equal(r["labels"][r["mask"]], sk), f"{key}: the restatement differs from sklearn at {int((r['labels'][r['mask']] != sk).sum())} pixels"
        assert sk.max(initial=-1) < 32767
        out[key + "_grid"] = np.packbits(grid > 0)
        out[key + "_sklearn"] = sk.astype(np.int16)
        print(f"{key}: {grid.shape}, {len(pts)} ones, {r['n_clusters']} clusters, {int((r['labels'] == -1).sum())} noise")
    hc.assert_ties_are_exercised()
    path = os.path.join(HERE, "highloss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
