"""Generate tests/golden/subregions.npz: the labels the reference's own get_subregions (src/planner/planner.py:530-574) returns for every case
of tests/policy_cases.SUBREGION_CASES.

Run only where networkx and the reference are present:   python tests/golden/make_subregions_golden.py
The reference's files never travel: src/planner/planner.py is IMPORTED here, with stubs for the absent cv2 (its annotations name cv2.Mat),
rospy and utils (start_timing / end_timing), none of which get_subregions calls; only the inputs and its labels are written.

get_subregions is fed a COMPLETE networkx graph on the nodes whose edge (i, j) weighs D[i][j] / 12 (no edge where D is unreachable) -- D being
shortest path lengths already, its all-pairs Dijkstra returns them -- the node pixels as the vertices, and meter_per_pixel = 1 / px_per_m.
A single node cannot be linked (scipy refuses an empty distance matrix, and so does get_subregions): its one label is written as 1.

Per case `key`:  key_node_rc   int32 [K, 2]
                 key_D         int32 [K, K]: scipy's Dijkstra on the roadmap mask (policy_cases.ref_node_distances), INT32_MAX = unreachable
                 key_px_per_m  fp64
                 key_labels    int32 [K]: get_subregions' cluster numbers (fcluster's, from 1), node by node
Every case is also run through policy_cases.ref_linkage and scipy here, and the script stops if a single label differs.
"""
import importlib.util
import os
import sys
import types

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import policy_cases as pc  # noqa: E402

REFERENCE = "/root/reference/src/planner/planner.py"


def reference_module():
    cv2 = types.ModuleType("cv2")
    cv2.Mat = np.ndarray
    utils = types.ModuleType("utils")
    utils.start_timing = utils.end_timing = lambda *a, **k: None
    sys.modules.setdefault("cv2", cv2)
    sys.modules.setdefault("rospy", types.ModuleType("rospy"))
    sys.modules.setdefault("utils", utils)
    spec = importlib.util.spec_from_file_location("reference_planner", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_labels(ref, node_rc, D, px_per_m):
    K = len(node_rc)
    if K == 1:
        return np.ones(1, np.int32)
    g = nx.Graph()
    g.add_nodes_from(range(K))
    for i in range(K):
        for j in range(i + 1, K):
            if D[i, j] != pc.INF:
                g.add_edge(i, j, weight=float(D[i, j]) / 12.0)
    sub, _ = ref.get_subregions(g, np.arange(K), node_rc.astype(np.float64), 1.0 / px_per_m)
    return np.array([sub[k] for k in range(K)], np.int32)


def main():
    ref = reference_module()
    out = {}
    for key, *_ in pc.SUBREGION_CASES:
        cs = pc.subregion_case(key)
        labels = reference_labels(ref, cs.node_rc, cs.D, cs.px_per_m)
        assert np.array_equal(pc.canonical(labels), cs.labels), f"{key}: the restatement differs from get_subregions"
        assert np.array_equal(pc.canonical(labels), cs.sp_labels), f"{key}: scipy differs from get_subregions"
        out[key + "_node_rc"], out[key + "_D"] = cs.node_rc.astype(np.int32), cs.D.astype(np.int32)
        out[key + "_px_per_m"], out[key + "_labels"] = np.float64(cs.px_per_m), labels
        print(f"{key}: K {len(cs.node_rc)}, {int(labels.max())} subregions, t {cs.t} px, unreachable pairs {int((cs.D == pc.INF).sum()) // 2}")
    path = os.path.join(HERE, "subregions.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
