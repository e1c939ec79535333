"""CPU (host-emulated kernels): the on-device grid DBSCAN and the node look-arounds (activesplat_amd/visibility.py, gs_grid_dbscan).  The
checks, their references and tolerances: tests/cluster_cases.py.  The same checks run on the MI355X in tests/test_gpu_cluster.py."""
import numpy as np
import pytest
import torch

from tests import cluster_cases as cc


def test_the_restatement_gives_sklearns_labels_for_every_case_of_the_fixture():
    """the rule of include/gsplat_hip.h, in numpy, against sklearn.cluster.DBSCAN's labels recorded by tests/golden/make_cluster_golden.py"""
    for col in (15, 16, 13):
        r = cc.restate(cc.mask_values(cc.contested_mask(col)), 0.8, 5, 25)
        assert np.array_equal(r["mask"], cc.golden_mask(f"contested_{col}", 24, 40))
        assert np.array_equal(r["labels"], cc.golden_labels(f"contested_{col}", 24, 40))
    r = cc.restate(cc.mask_values(cc.serpentine_mask(), complement=True), 0.8, 5, 25, True)
    assert np.array_equal(r["mask"], cc.golden_mask("serpentine", 150, 360)) and np.array_equal(r["labels"], cc.golden_labels("serpentine", 150, 360))
    assert r["n_clusters"] == 1 and r["count"][0] == 28200
    for name, H, W, *_ in cc.RANDOM_CASES:
        for seed in cc.SEEDS:
            _, r = cc.reference(name, seed)
            assert np.array_equal(r["labels"], cc.golden_labels(f"{name}_{seed}", H, W)), (name, seed)


def test_the_restated_cluster_table_is_what_the_references_get_invisibility_clusters_returned():
    """src/mapper/__init__.py:92-117 on the 75 x 180 cases (recorded in the fixture): the clusters over the threshold in ascending number, their
    centres points.mean(axis=0) exactly (integer sums divided in fp64), their fp32 numpy sums to the tolerance of the sums"""
    for seed in cc.SEEDS:
        _, r = cc.reference("local", seed)
        centers, sums = cc.golden()[f"local_{seed}_ref_centers"], cc.golden()[f"local_{seed}_ref_sums"]
        keep = [c for c in range(r["n_clusters"]) if np.float32(r["sum_value"][c]) > 30]
        assert len(keep) == len(sums) > 0
        mine = np.array([[r["sum_row"][c] / r["count"][c], r["sum_col"][c] / r["count"][c]] for c in keep])
        assert np.array_equal(mine, centers)
        assert np.allclose(r["sum_value"][keep], sums.astype(np.float64), rtol=cc.SUM_RTOL, atol=0)


def test_grid_dbscan_has_no_cpu_fallback():
    from activesplat_amd import _lib
    from activesplat_amd import visibility as VIS
    _lib.unload_for_tests()
    import os
    have = os.path.exists(_lib.LIB_PATH)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VIS.grid_dbscan(torch.zeros(24, 40), 0.5, 5, 10)             # (with the HIP library built: host tensors are refused; without: the loader raises)
    assert have or _lib._lib is None


def test_emulated_contested_border_takes_the_smallest_cluster_number(emu):
    cc.check_contested(emu)


def test_emulated_serpentine_is_one_cluster(emu):
    cc.check_serpentine(emu)


@pytest.mark.parametrize("name", [c[0] for c in cc.RANDOM_CASES])
def test_emulated_random_fields_match_the_restatement(emu, name):
    cc.check_random(emu, name)


def test_emulated_small_sizes(emu):
    cc.check_small_sizes(emu)


def test_emulated_nonfinite_values(emu):
    cc.check_nonfinite(emu)


def test_emulated_truncated_table(emu):
    cc.check_truncated(emu)


def test_emulated_refusals(emu):
    cc.check_refusals(emu, batch64=False)


def test_emulated_two_calls_are_bit_identical(emu):
    cc.check_repeatable(emu)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_emulated_look_around_nodes_equal_per_node_look_around(emu, K):
    cc.check_look_around_nodes(emu, K)


def test_emulated_look_around_nodes_in_one_pass(emu):
    cc.check_look_around_nodes(emu, 5, nodes_per_pass=21)
    from activesplat_amd import visibility as VIS
    with pytest.raises(ValueError, match="nodes_per_pass"):
        VIS.look_around_nodes(cc.shell_params(emu), cc.base_pose(), cc.node_positions(2), nodes_per_pass=22)


@pytest.mark.parametrize("K,nodes_per_pass", [(3, None), (2, 21)])
def test_emulated_global_invisibility_nodes_is_the_two_calls(emu, K, nodes_per_pass):
    cc.check_global_nodes(emu, K, nodes_per_pass)


@pytest.mark.parametrize("name", [s[0] for s in cc.LOCAL_SCENES])
def test_emulated_local_invisibility_target(emu, name):
    cc.check_local_target(emu, name)


def test_emulated_mapper_methods(emu):
    cc.check_mapper(emu)
