"""GPU (-m gpu): the planner's top-down free / visible maps on the MI355X -- the checks of tests/topdown_cases.py (their tolerances and where they
come from are stated there) on the real kernels, at the sizes of the issue."""
import pytest

from tests import topdown_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,W,H,iso,need_unseen", [(20000, 360, 300, False, True), (20000, 360, 300, True, True), (200000, 360, 300, False, False),
                                                    (20000, 368, 368, False, True), (20000, 368, 368, True, True), (20000, 256, 240, False, True),
                                                    (5000, 120, 150, False, True), (5000, 120, 150, True, True), (5000, 122, 150, False, True)])
def test_topdown_maps_match_the_oracle_run_the_references_way(hip, oracle32, N, W, H, iso, need_unseen):
    tc.check_scene(hip, oracle32, N, W, H, iso=iso, need_unseen=need_unseen)


def test_topdown_grey_rule_scene(hip, oracle32):
    tc.check_grey_rule(hip, oracle32)


def test_topdown_band_edges(hip, oracle32):
    tc.check_band_edges(hip, oracle32)


def test_topdown_nonfinite_parameters_leave_finite_maps(hip):
    tc.check_nonfinite(hip)


@pytest.mark.parametrize("N,W,H,iso", [(20000, 360, 300, False), (20000, 368, 368, True), (5000, 120, 150, False)])
def test_topdown_integer_artefacts_are_the_oracles(hip, oracle32, N, W, H, iso):
    tc.check_integer_artefacts(hip, oracle32, N, W, H, iso=iso)


@pytest.mark.parametrize("N,W,H,iso", [(20000, 360, 300, False), (200000, 360, 300, False), (20000, 368, 368, True), (20000, 256, 240, False),
                                       (5000, 120, 150, True), (5000, 122, 150, False)])
def test_topdown_maps_equal_the_two_pass_composition(hip, N, W, H, iso):
    tc.check_equivalence(hip, N, W, H, iso=iso)


def test_topdown_maps_twice_on_one_stream_take_the_optimistic_launch(hip):
    """the second tick of a (P, W, H) stream is enqueued behind the counting kernels with the first tick's capacities: same maps"""
    import torch
    from activesplat_amd import topdown as TD
    params = tc.scene_params(20000, 360, 300, hip)
    cam = tc.camera(360, 300, hip)
    a = TD.topdown_maps(params, cam, *tc.BAND)
    b = TD.topdown_maps(params, cam, *tc.BAND)
    for k in a._fields:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_mapper_topdown_maps(hip):
    tc.check_mapper(hip)


def test_topdown_optimistic_launch_hits_and_misses_reproduce_the_exact_maps(hip):
    tc.check_optimistic_launch(hip)
