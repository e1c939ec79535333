"""CPU (host-emulated kernels): the on-device cluster hull volumes (activesplat_amd/visibility.py cluster_hulls / global_invisibility_scores,
gs_cluster_hulls).  The checks, their references and tolerances: tests/hull_cases.py.  The same checks run on the MI355X in tests/test_gpu_hull.py."""
import numpy as np
import pytest
import torch

from tests import hull_cases as hc


def _labels(H, W, pixels):
    m = np.zeros((H, W), bool)
    for x, y in pixels:
        m[y, x] = True
    return m


def test_the_trace_gives_the_known_answers():
    """OpenCV's published output for a rectangle, a single pixel, a 1-pixel-wide plus (points repeat) and the 15 x 15 ellipse around one pixel"""
    rect = _labels(8, 10, [(x, y) for x in range(2, 6) for y in range(1, 4)])
    assert hc.trace(rect) == hc.RECTANGLE_CONTOUR
    assert hc.trace(_labels(8, 10, [(3, 5)])) == [(3, 5)]
    assert hc.trace(np.zeros((8, 10), bool)) == []
    assert hc.trace(hc.plus() == 0) == hc.PLUS_CONTOUR
    assert hc.trace(hc.dilate(hc.plus() == 0, [1], 1)) == hc.PLUS_CONTOUR
    ellipse = hc.trace(hc.dilate(_labels(24, 40, [(15, 15)]), hc.ellipse_rows(), 15))
    assert len(ellipse) == 22 and ellipse[:8] == hc.PIXEL1515_HEAD and ellipse[-3:] == hc.PIXEL1515_TAIL


def test_the_ellipse_footprint_is_the_stated_one():
    from activesplat_amd import visibility as VIS
    half = [7, 7, 7, 6, 6, 5, 4, 0]
    rows = hc.ellipse_rows()
    for i in range(15):
        h = half[abs(i - 7)]
        assert rows[i] == sum(1 << j for j in range(7 - h, 7 + h + 1))
    assert VIS.ellipse_footprint().tolist() == rows and VIS.ellipse_footprint().dtype == np.uint32
    for kh, kw in ((1, 1), (3, 5), (7, 3), (1, 9), (9, 1)):
        assert VIS.ellipse_footprint(kh, kw).tolist() == hc.ellipse_rows(kh, kw)
    with pytest.raises(ValueError):
        VIS.ellipse_footprint(4, 3)


def test_the_dilation_clips_at_the_border_and_is_not_symmetrised():
    corner = hc.dilate(_labels(24, 40, [(0, 0)]), hc.ellipse_rows(), 15)
    assert corner[0, :8].all() and not corner[0, 8] and corner[:8, 0].all() and not corner[8, 0] and int(corner.sum()) == 50     # rows of 8, 8, 8, 7, 7, 6, 5, 1
    # dil(y, x) = OR mask(y + i - ay, x + j - ax): the cell (0, 0) of a 3 x 3 footprint reads the pixel up and left, so the set pixel moves down and right
    moved = hc.dilate(_labels(8, 10, [(4, 4)]), [1, 0, 0], 3)
    assert int(moved.sum()) == 1 and moved[5, 5]


def test_the_restated_hull_is_scipys_on_every_case_of_the_fixture():
    """scipy.spatial.ConvexHull(...).volume recorded by tests/golden/make_hull_golden.py; the contours are the recorded ones"""
    worst = 0.0
    for name, k in hc.small_cases().items():
        _, refs = hc.reference(name)
        for b, ref in enumerate(refs):
            want = hc.golden()[name + "_scipy"][b]
            assert np.allclose(ref["volume"], want, rtol=hc.VOL_RTOL, atol=hc.VOL_ATOL), (name, b)
            assert (want[:len(ref["contours"])] > 0).all() or name in hc.ZERO_VOLUME
            worst = max(worst, float(np.max(np.abs(ref["volume"] - want) / np.maximum(want, 1e-300))))
            for c, contour in enumerate(ref["contours"]):
                assert contour == hc.golden_contours(name, b, c), (name, b, c)
    print(f"restated hull against scipy, small cases: max relative error {worst:.2e}")


@pytest.mark.parametrize("seed", hc.cc.SEEDS)
def test_the_restatement_gives_what_the_references_get_convexhull_volume_returned(seed):
    """src/mapper/__init__.py:8-90 on the 150 x 360 cases (recorded in the fixture): its per-cluster hull volumes and its two sums"""
    _, r, depth, ref = hc.reference_global(seed)
    key = f"global_{seed}"
    g = hc.golden()
    n = r["n_clusters"]
    assert len(g[key + "_ref_volumes"]) == n and np.array_equal(g[key + "_ref_volumes"], g[key + "_scipy"][0, :n])
    assert np.allclose(ref["volume"][:n], g[key + "_ref_volumes"], rtol=hc.VOL_RTOL, atol=hc.VOL_ATOL) and (g[key + "_ref_volumes"] > 0).all()
    for c in range(n):
        assert ref["contours"][c] == hc.golden_contours(key, 0, c)
    last_invisibility, last_volume = g[key + "_ref"]
    assert abs(ref["sum_volume"] - last_volume) <= hc.VOL_ATOL + hc.VOL_RTOL * last_volume
    assert abs(ref["sum_invisibility"] - last_invisibility) <= hc.SUM_RTOL * last_invisibility
    z = np.concatenate([p[:, 2] for p in ref["points"]])
    if hc.GLOBAL_DEPTH[seed] == "zero":
        assert (z == 0).sum() >= 10
    if hc.GLOBAL_DEPTH[seed] == "fifteen":
        assert int(ref["n_points"].sum()) - len(z) >= 10


def test_cluster_hulls_has_no_cpu_fallback():
    import os
    from activesplat_amd import _lib
    from activesplat_amd import visibility as VIS
    _lib.unload_for_tests()
    have = os.path.exists(_lib.LIB_PATH)
    k = hc.small_cases()["overlap"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VIS.cluster_hulls(torch.from_numpy(k["labels"]), torch.from_numpy(k["depth"]), hc.clusters_of("cpu", k["n"], k["sum_value"]))
    assert have or _lib._lib is None


@pytest.mark.parametrize("name", list(hc.small_cases()))
def test_emulated_small_cases(emu, name):
    hc.check_small(emu, name)


@pytest.mark.parametrize("seed", hc.cc.SEEDS)
def test_emulated_global_fields_match_scipy_and_the_reference(emu, seed):
    hc.check_global(emu, seed)


def test_emulated_refusals(emu):
    hc.check_refusals(emu)


def test_emulated_two_calls_are_bit_identical(emu):
    hc.check_repeatable(emu)


@pytest.mark.parametrize("K,zero_at", [(2, None), (5, 2)])
def test_emulated_global_invisibility_scores(emu, K, zero_at):
    hc.check_scores(emu, K, zero_at)


def test_emulated_scores_raise_when_the_cluster_table_is_too_small(emu):
    hc.check_scores_raise_when_truncated(emu)


def test_emulated_mapper_method(emu):
    hc.check_mapper(emu)
