"""CPU (host-emulated kernels): the per-frame high-loss look target (activesplat_amd/visibility.py: high_loss_grid, high_loss_target;
gs_high_loss_grid; SplatMapper(high_loss_target=True)).  The checks and their references: tests/highloss_cases.py.  The same checks run on the
MI355X in tests/test_gpu_highloss.py."""
import numpy as np
import pytest
import torch

from activesplat_amd import frames as FR
from tests import cluster_cases as cc
from tests import highloss_cases as hc


def test_the_integer_resize_is_the_float64_bilinear_resize_on_every_pixel_of_every_case():
    """the integer rule of include/gsplat_hip.h, in numpy, against frames.resize_linear (cv2's sampling convention in float64, rounded half up) --
    exact ties included, and the case set holds enough of them"""
    for name, H, W, gh, gw in hc.RESIZE_CASES:
        for kind in hc.MASK_KINDS:
            m, grid, ties = hc.resize_reference(name, kind)
            assert m.shape == (H, W) and grid.shape == (gh, gw)
            want = FR.resize_linear(m.astype(np.uint8), gw, gh)
            assert set(np.unique(want)) <= {0, 1}
            assert np.array_equal(grid, want.astype(np.float32)), (name, kind, int((grid != want).sum()))
            if kind == "blobs" and min(H, W) >= 37:
                assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    assert not hc.resize_reference("mixed", "random50")[2].any()             # 37 x 53 -> 90 x 90 has no ties
    hc.assert_ties_are_exercised()


def test_the_restated_labels_are_sklearns_for_every_grid_of_the_fixture():
    """cluster_cases.restate on the grids of the cases against sklearn.cluster.DBSCAN(eps=5, min_samples=10)'s labels recorded by
    tests/golden/make_highloss_golden.py"""
    grids = hc.golden_grids()
    assert len(grids) == len(hc.RESIZE_CASES) * len(hc.MASK_KINDS) + len(hc.decision_masks())
    for key, grid in grids.items():
        m, labels = hc.golden_labels(key, grid.shape)
        assert np.array_equal(m, grid > 0), f"{key}: the rebuilt grid is not the fixture's"
        assert np.array_equal(cc.restate(grid, 0.0, 5, 10)["labels"], labels), key


def test_the_host_half_follows_the_references_lines():
    """target_from_high_loss_clusters against the op-for-op restatement of src/mapper/splatam/__init__.py:219-250, on the decision grids (no kernel)"""
    from activesplat_amd import visibility as VIS
    c2w = hc.view_pose()
    for name, (m, thr, kind) in hc.decision_masks().items():
        grid = m.astype(np.float32)
        want, _ = hc.restate_target(grid, c2w, thr)
        r = cc.restate(grid, 0.0, 5, 10)
        got = VIS.target_from_high_loss_clusters(c2w, float(grid.sum()), r["count"], r["sum_row"], r["sum_col"], thr)
        assert (want is None) == (got is None) == (kind == "none"), name
        assert want is None or np.array_equal(got, want), name


def test_high_loss_grid_has_no_cpu_fallback():
    import os
    from activesplat_amd import _lib
    from activesplat_amd import visibility as VIS
    _lib.unload_for_tests()
    have = os.path.exists(_lib.LIB_PATH)
    z = torch.zeros(12, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VIS.high_loss_grid(z, z, z)                      # (with the HIP library built: host tensors are refused; without: the loader raises)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VIS.high_loss_target(np.eye(4), z, z, z)
    assert have or _lib._lib is None


def test_emulated_pixel_rule(emu):
    hc.check_pixel_rule(emu)


@pytest.mark.parametrize("name", [c[0] for c in hc.RESIZE_CASES])
def test_emulated_resize_matches_the_restatement(emu, name):
    hc.check_resize(emu, name)


@pytest.mark.parametrize("name", list(hc.decision_masks()))
def test_emulated_decisions(emu, name):
    hc.check_decision(emu, name)


def test_emulated_refusals(emu):
    hc.check_refusals(emu)


def test_emulated_two_calls_are_bit_identical(emu):
    hc.check_repeatable(emu)


def test_emulated_mapper(emu):
    hc.check_mapper(emu)


def test_emulated_mapper_tracked_frame(emu):
    hc.check_mapper_tracked(emu)
