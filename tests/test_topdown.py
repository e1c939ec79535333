"""CPU (host-emulated kernels): the planner's top-down free / visible maps in one fused raster pass (activesplat_amd/topdown.py,
gs_preprocess_forward_topdown + gs_render_forward_topdown) against the fp32 oracle run the reference's way.  The checks, their tolerances and
where they come from: tests/topdown_cases.py.  The same checks run on the MI355X in tests/test_gpu_topdown.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import topdown_cases as tc


def test_grey_is_opencv_fixed_point_rgb2gray_not_all_three_bytes_255():
    from activesplat_amd import topdown as TD
    for rgb, grey in tc.GREY_TABLE:
        assert int(TD.rgb_to_grey_u8(np.array(rgb, np.uint8))) == grey, rgb
        assert int(TD.rgb_to_grey_u8(torch.tensor(rgb, dtype=torch.uint8))) == grey, rgb
    # a pure grey keeps its value: the three coefficients sum to 2^14
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(TD.rgb_to_grey_u8(np.stack([v, v, v], -1)), v)


def test_topdown_camera_is_the_parity_cases_camera():
    """the product's topdown_camera restates get_topdown_cam exactly as the helper the topdown_1000m parity cases have used so far"""
    from activesplat_amd import topdown as TD
    from tests import parity_cases as pc
    for W, H in ((360, 300), (368, 368), (120, 150)):
        a = TD.topdown_camera(tc.CENTRE, tc.EXTENT, (W, H), device="cpu")
        b = pc.topdown_camera(W, H, bg=(1.0, 1.0, 1.0))
        for f in ("image_height", "image_width", "tanfovx", "tanfovy", "scale_modifier", "sh_degree"):
            assert getattr(a, f) == getattr(b, f), f
        for f in ("bg", "viewmatrix", "projmatrix", "campos"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_topdown_maps_has_no_cpu_fallback_and_checks_its_arguments(emu_lib_path):
    from activesplat_amd import _lib
    from activesplat_amd import topdown as TD
    _lib.unload_for_tests()
    params = tc.scene_params(100, 120, 150, "cpu")
    cam = tc.camera(120, 150, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TD.topdown_maps(params, cam, *tc.BAND)
    from tests import util
    undo = util.use_emulated_kernels(emu_lib_path)
    try:
        with pytest.raises(ValueError, match="NaN"):
            TD.topdown_maps(params, cam, float("nan"), 1.0)
        with pytest.raises(ValueError, match="log_scales"):
            TD.topdown_maps(dict(params, log_scales=params["log_scales"][:, :2].contiguous()), cam, *tc.BAND)
        lib = _lib.get()
        assert lib.gs_render_forward_topdown(None, 0, 0, 0, None, None, None, None, None, None, None, None, None) == 1                      # GS_EINVAL
        assert b"gs_render_forward_topdown" in lib.gs_last_error()
        assert lib.gs_preprocess_forward_topdown(None, 0, None, None, None, None, None, 0, C.c_float(0.0), C.c_float(1.0), None, None, None, None,
                                                 None, None) == 1                      # GS_EINVAL
        # an empty map renders: everything free, everything unseen
        empty = {k: v[:0].contiguous() for k, v in params.items()}
        m = TD.topdown_maps(empty, cam, *tc.BAND)
        assert bool((m.free_map_binary == 1).all()) and bool((m.visible_map_binary == 1).all()) and bool((m.visible_rgb == 255).all())
        assert bool((m.free_opacity == 0).all())
    finally:
        undo()


@pytest.mark.parametrize("N,W,H,iso,need_unseen", [(20000, 360, 300, False, True), (200000, 360, 300, False, False), (20000, 368, 368, True, True),
                                                    (20000, 256, 240, False, True), (5000, 120, 150, True, True), (5000, 122, 150, False, True)])
def test_emulated_topdown_maps_match_the_oracle_run_the_references_way(emu, oracle32, N, W, H, iso, need_unseen):
    """360 x 300, 368 x 368 (ragged edge tiles), 240 tiles (below 257), 120 x 150 and 122 x 150 (a width that is not a multiple of 4: the
    epilogue's byte stores); N = 20 000 (89 % free, 23 % unseen at 360 x 300) for
    both maps, N = 200 000 (9.5 % free, nothing unseen) for the free map; the oracle itself shows that both values occur and how many pixels
    are ambiguous (printed)."""
    tc.check_scene(emu, oracle32, N, W, H, iso=iso, need_unseen=need_unseen)


def test_emulated_topdown_grey_rule_scene(emu, oracle32):
    tc.check_grey_rule(emu, oracle32)


def test_emulated_topdown_band_edges(emu, oracle32):
    tc.check_band_edges(emu, oracle32)


def test_emulated_topdown_nonfinite_parameters_leave_finite_maps(emu):
    tc.check_nonfinite(emu)


@pytest.mark.parametrize("N,W,H,iso", [(20000, 360, 300, False), (20000, 368, 368, True)])
def test_emulated_topdown_integer_artefacts_are_the_oracles(emu, oracle32, N, W, H, iso):
    tc.check_integer_artefacts(emu, oracle32, N, W, H, iso=iso)


@pytest.mark.parametrize("N,W,H,iso", [(20000, 360, 300, False), (20000, 368, 368, True), (20000, 256, 240, False), (5000, 120, 150, True),
                                       (5000, 122, 150, False)])
def test_emulated_topdown_maps_equal_the_two_pass_composition(emu, N, W, H, iso):
    tc.check_equivalence(emu, N, W, H, iso=iso)


def test_emulated_mapper_topdown_maps(emu):
    tc.check_mapper(emu)


def test_emulated_topdown_optimistic_launch_hits_and_misses_reproduce_the_exact_maps(emu):
    tc.check_optimistic_launch(emu)
