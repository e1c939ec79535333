"""GPU (-m gpu): the per-frame high-loss look target on the MI355X -- the checks of tests/highloss_cases.py (references stated there) on the real
kernels.  Nothing here reads sklearn or the reference: the numpy restatement and tests/golden/highloss.npz do."""
import numpy as np
import pytest
import torch

from tests import cluster_cases as cc
from tests import highloss_cases as hc

pytestmark = pytest.mark.gpu


def test_pixel_rule(hip):
    hc.check_pixel_rule(hip)


@pytest.mark.parametrize("name", [c[0] for c in hc.RESIZE_CASES])
def test_resize_matches_the_restatement(hip, name):
    hc.check_resize(hip, name)


def test_grids_cluster_to_the_fixtures_sklearn_labels(hip):
    """high_loss_grid + grid_dbscan on three resize cases: the device's labels are the ones sklearn gave for the same grid"""
    from activesplat_amd import visibility as VIS
    for name, kind in (("s40x48", "random10"), ("s150x120", "blobs"), ("mixed", "blobs")):
        m, want, _ = hc.resize_reference(name, kind)
        _, grid = VIS.high_loss_grid(*hc.images_of(m, hip))
        fixture_grid, labels = hc.golden_labels(f"{name}_{kind}", want.shape)
        assert np.array_equal(grid.cpu().numpy() > 0, fixture_grid)
        assert np.array_equal(VIS.grid_dbscan(grid, 0.0, 5, 10).labels.cpu().numpy(), labels)


@pytest.mark.parametrize("name", list(hc.decision_masks()))
def test_decisions(hip, name):
    hc.check_decision(hip, name)


def test_refusals(hip):
    hc.check_refusals(hip)
    from activesplat_amd import visibility as VIS
    z = torch.zeros(12, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VIS.high_loss_grid(z, z, z)                      # host tensors


def test_two_calls_are_bit_identical(hip):
    hc.check_repeatable(hip)


def test_mapper(hip):
    hc.check_mapper(hip)


def test_mapper_tracked_frame(hip):
    hc.check_mapper_tracked(hip)
