"""Generate tests/golden/cluster.npz: sklearn's DBSCAN labels for every case of tests/cluster_cases.py, and what the reference's own
get_invisibility_clusters returns for the 75 x 180 cases.

Run only where sklearn and the reference are present:   python tests/golden/make_cluster_golden.py
The reference's files never travel: src/mapper/__init__.py is IMPORTED here (with a stub for the absent cv2, which the function used does not
call), and only its inputs' masks and its outputs are written.

Per case `key`:  key_mask     the mask, np.packbits of the row-major [H, W] booleans
                 key_sklearn  int16: DBSCAN(eps, min_samples).fit_predict(np.column_stack(np.where(mask))) (-1 noise), one per masked pixel
                 key_values   fp32 [H, W], for the images up to 33 x 70 (the larger ones are rebuilt from their seed, see cluster_cases.py)
                 key_ref_centers [n, 2] fp64, key_ref_sums [n] fp32   get_invisibility_clusters(values, 30) -- the `local` cases only
Every case is also run through cluster_cases.restate here, and the script stops if a single label differs from sklearn's.
"""
import importlib.util
import os
import sys
import types

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import cluster_cases as cc  # noqa: E402

REFERENCE = "/root/reference/src/mapper/__init__.py"


def reference_module():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_mapper", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sklearn_labels(mask, eps, min_samples):
    pts = np.column_stack(np.where(mask))
    return DBSCAN(eps=eps, min_samples=min_samples).fit_predict(pts) if len(pts) else np.zeros(0, np.int64)


def add(out, key, values, thr, eps, ms, comp, keep_values):
    r = cc.restate(values, thr, eps, ms, comp)
    mask = r["mask"]
    sk = sklearn_labels(mask, eps, ms)
    assert np.array_equal(r["labels"][mask], sk), f"{key}: the restatement differs from sklearn at {int((r['labels'][mask] != sk).sum())} pixels"
    assert sk.max(initial=-1) < 32767
    out[key + "_mask"] = np.packbits(mask)
    out[key + "_sklearn"] = sk.astype(np.int16)
    if keep_values:
        out[key + "_values"] = values
    print(f"{key}: {values.shape}, {int(mask.sum())} masked, {r['n_clusters']} clusters, {int(((r['labels'] >= 0) & ~r['core']).sum())} border "
          f"({int(r['contested'].sum())} contested), {int((r['labels'] == -1).sum())} noise")
    return r


def main():
    out = {}
    for col in (15, 16, 13):
        add(out, f"contested_{col}", cc.mask_values(cc.contested_mask(col)), 0.8, 5, 25, False, True)
    add(out, "serpentine", cc.mask_values(cc.serpentine_mask(), complement=True), 0.8, 5, 25, True, False)
    ref = reference_module()
    for name, H, W, thr, eps, ms, comp in cc.RANDOM_CASES:
        rs = []
        for seed in cc.SEEDS:
            values = cc.random_case(name, seed)[0]
            key = f"{name}_{seed}"
            rs.append(add(out, key, values, thr, eps, ms, comp, values.size <= cc.VALUES_STORED_UP_TO))
            if name == "local":
                centers, sums = ref.get_invisibility_clusters(values, 30)
                out[key + "_ref_centers"] = np.asarray(centers, np.float64).reshape(-1, 2)
                out[key + "_ref_sums"] = np.asarray(sums, np.float32)
                print(f"  get_invisibility_clusters: {len(sums)} clusters over the threshold")
        cc.assert_case_set_is_hard(name, rs)
    path = os.path.join(HERE, "cluster.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
