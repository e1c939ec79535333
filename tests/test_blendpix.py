"""The blend kernels pixel by pixel and row by row at their rare branches, on the host-emulated kernels (tests/blendpix_cases.py; the device
twin is tests/test_gpu_blendpix.py)."""
import numpy as np
import pytest

from tests import blendpix_cases as bp
from tests.pose_cases import one_openmp_thread


@pytest.mark.parametrize("name", bp.PASS_FAIL)
def test_replay_equals_the_fp64_oracle(oracle64, oracle32, name):
    """The replay is the tests' own reference: its forward equals the fp64 oracle's images, final T and n_contrib, and the net sums of its
    per-pixel contributions equal the oracle's blend-native gradients within 1e-10 of their absolute sums S (colour alone, colour + depth, and
    all four outputs through output_grad_cases.reference).  The scene's class shares are asserted on the way."""
    sc = bp.scene(name, oracle64)
    half = np.array([0.5 * sc.W, 0.5 * sc.H])
    for entry in bp.ENTRIES:
        ref = bp.reference(sc, entry, oracle64, oracle32)
        bp.assert_scene(sc, ref)
        rp, f, g = ref["rp"], ref["f64"], ref["g64"]
        assert np.array_equal(rp.n_contrib, f["n_contrib"]), name
        img, _A = bp.replay_images(rp)
        for k, v in bp.images_of(f).items():
            assert np.abs(img[k] - v).max() <= 1e-13 * max(1.0, np.abs(v).max()), (name, k, np.abs(img[k] - v).max())
        pairs = [("opacities", rp.net["dop"], rp.S["dop"]), ("colors_precomp", rp.net["dfeat"][:, :3], rp.S["dfeat"][:, :3]),
                 ("means2D", rp.net["dxy"] * half, rp.S["dxy"] * half)]
        if entry in ("color", "rgbd"):
            pairs += [("_dfeat", rp.net["dfeat"][:, :3], rp.S["dfeat"][:, :3]), ("_dxy", rp.net["dxy"], rp.S["dxy"]), ("_dconic", rp.net["dconic"], rp.S["dconic"])]
        for k, net, S in pairs:
            o = g[k].reshape(sc.P, -1)[:, :net.shape[1]]
            err = np.abs(net - o)
            assert (err <= 1e-10 * S).all(), (name, entry, k, float((err / np.where(S > 0, S, 1.0)).max()))
            assert (S >= np.abs(net) * (1 - 1e-12)).all(), (name, entry, k)


def test_fp32_oracle_alone_sets_floors(oracle64, oracle32):
    """The floors come from the two oracles alone: the fp32 oracle's largest error in the rules' units over every pass/fail scene, entry and
    output / tensor is printed (blendpix_cases.MEASURED_* record it) and each FLOOR must be at least twice it, so a generator change that moves
    it shows here.  The kernels are not involved."""
    worst_f, worst_b = (0.0, None), (0.0, None)
    for label, sc, ref, cov in bp.all_references(oracle64, oracle32):
        e, k = bp.oracle_pixel_error(ref)
        eb, kb, row = bp.oracle_row_error(sc, ref, cov)
        print(f"[blendpix] fp32 oracle alone: {label:40s} pixels {e:.3e} ({k}); rows {eb:.3e} ({kb}, row {row}: {bp.row_classes(ref['rp'], row)})")
        worst_f, worst_b = max(worst_f, (e, label)), max(worst_b, (eb, label))
    print(f"[blendpix] fp32 oracle alone: largest per-pixel error {worst_f[0]:.3e} ({worst_f[1]}), FLOOR_F {bp.FLOOR_F:g}; largest per-row error {worst_b[0]:.3e} "
          f"({worst_b[1]}), FLOOR_B {bp.FLOOR_B:g}")
    assert abs(worst_f[0] / bp.MEASURED_ORACLE32_PIXEL_ERROR - 1.0) <= 0.1 and abs(worst_b[0] / bp.MEASURED_ORACLE32_ROW_ERROR - 1.0) <= 0.1, (worst_f, worst_b)
    assert 2.0 * bp.MEASURED_ORACLE32_PIXEL_ERROR <= bp.FLOOR_F < bp.CAP_MAX and 2.0 * bp.MEASURED_ORACLE32_ROW_ERROR <= bp.FLOOR_B < bp.CAP_MAX
    assert 2.0 * worst_f[0] <= bp.FLOOR_F, worst_f
    assert 2.0 * worst_b[0] <= bp.FLOOR_B, worst_b


@pytest.mark.parametrize("name", bp.FEW)
def test_few_tile(emu, oracle64, oracle32, name):
    with one_openmp_thread():
        bp.check_few(name, emu, oracle64, oracle32)


@pytest.mark.parametrize("name", bp.MANY)
def test_many_tile(emu, oracle64, oracle32, name):
    with one_openmp_thread():
        bp.check_many(name, emu, oracle64, oracle32)


def test_segmented(emu, oracle64, oracle32):
    with one_openmp_thread():
        bp.check_segmented("few/segmented", emu, oracle64, oracle32)


@pytest.mark.parametrize("pieces", [3, 2])
def test_resumed_chained(emu, oracle64, oracle32, pieces):
    with one_openmp_thread():
        bp.check_chained("many/resumed", pieces, emu, oracle64, oracle32)


def test_deep_saturated_report_only(emu, oracle64, oracle32):
    with one_openmp_thread():
        bp.check_report_only("few/deep_saturated", emu, oracle64, oracle32)
