"""GPU (-m gpu): the on-device grid DBSCAN and the node look-arounds on the MI355X -- the checks of tests/cluster_cases.py (references and
tolerances are stated there) on the real kernels.  Nothing here reads sklearn or the reference: the fixture and the numpy restatement do."""
import pytest

from tests import cluster_cases as cc

pytestmark = pytest.mark.gpu


def test_contested_border_takes_the_smallest_cluster_number(hip):
    cc.check_contested(hip)


def test_serpentine_is_one_cluster(hip):
    cc.check_serpentine(hip)


@pytest.mark.parametrize("name", [c[0] for c in cc.RANDOM_CASES])
def test_random_fields_match_the_restatement(hip, name):
    cc.check_random(hip, name)


def test_small_sizes(hip):
    cc.check_small_sizes(hip)


def test_nonfinite_values(hip):
    cc.check_nonfinite(hip)


def test_truncated_table(hip):
    cc.check_truncated(hip)


def test_refusals_and_the_largest_required_batch(hip):
    cc.check_refusals(hip)


def test_two_calls_are_bit_identical(hip):
    cc.check_repeatable(hip)


@pytest.mark.parametrize("K", [1, 2, 21, 22])
def test_look_around_nodes_equal_per_node_look_around(hip, K):
    """the issue's cap for every value, at the call's default; the figures measured at 63 slots in one pass and what follows from them:
    cluster_cases.check_look_around_nodes"""
    cc.check_look_around_nodes(hip, K)


@pytest.mark.parametrize("K", [21, 22])
def test_look_around_nodes_in_passes_of_21(hip, K):
    """nodes_per_pass=21: K = 21 fills one raster pass (63 atlas slots), K = 22 starts a second"""
    cc.check_look_around_nodes(hip, K, nodes_per_pass=21)


@pytest.mark.parametrize("K,nodes_per_pass", [(2, None), (5, None), (2, 21), (5, 21)])
def test_global_invisibility_nodes_is_the_two_calls(hip, K, nodes_per_pass):
    cc.check_global_nodes(hip, K, nodes_per_pass)


@pytest.mark.parametrize("name", [s[0] for s in cc.LOCAL_SCENES])
def test_local_invisibility_target(hip, name):
    cc.check_local_target(hip, name)


def test_mapper_methods(hip):
    cc.check_mapper(hip)
