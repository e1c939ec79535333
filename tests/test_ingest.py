"""CPU (host-emulated kernels): the on-device frame ingest (activesplat_amd/ingest.py; gs_frame_ingest).  The checks and where their expected values
come from: tests/ingest_cases.py.  The same checks run on the MI355X in tests/test_gpu_ingest.py."""
import numpy as np
import pytest
import torch

from tests import ingest_cases as ic


def test_the_restated_rules_are_the_host_resizes():
    """frames.resize_linear / frames.resize_nearest (numpy, what to_mapping_tensors calls) against the scalar restatement, on the shapes of this file"""
    from activesplat_amd import frames as FR
    for i, (h, w, H, W) in enumerate(ic.SHAPES):
        image, depth = ic.raw_frame(h, w, seed=10 + i)
        assert np.array_equal(FR.resize_linear(image, W, H), ic.restate_levels(image, W, H)), (h, w, H, W)
    for h, w, H, W in ic.SHAPES + (ic.DEPTH_ONLY,):
        depth = np.arange(h * w, dtype=np.float32).reshape(h, w)
        assert np.array_equal(FR.resize_nearest(depth, W, H), depth[ic.restate_rows(H, h)][:, ic.restate_rows(W, w)]), (h, w, H, W)
    # the integer index (y * h) // H is another rule: 2 -> 98 is one of the size pairs on which the two differ
    assert not np.array_equal(ic.restate_rows(98, 2), (np.arange(98) * 2) // 98)


def test_the_ingest_has_no_cpu_fallback():
    import os
    from activesplat_amd import _lib
    from activesplat_amd import ingest as IN
    _lib.unload_for_tests()
    have = os.path.exists(_lib.LIB_PATH)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IN.ingest_frame(torch.zeros(4, 6, 3, dtype=torch.uint8), torch.zeros(4, 6), [(3, 2)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IN.FrameIngest(6, 4, [(3, 2)], "cpu")
    assert have or _lib._lib is None


def test_emulated_resize_shapes(emu):
    ic.check_resize_shapes(emu)


def test_emulated_rounding(emu):
    ic.check_rounding(emu)


def test_emulated_depth_bit_patterns(emu):
    ic.check_depth_bits(emu)


def test_emulated_two_outputs_in_one_call(emu):
    ic.check_two_outputs(emu)


def test_emulated_two_calls_are_bit_identical(emu):
    ic.check_repeatable(emu)


def test_emulated_refusals(emu):
    ic.check_refusals(emu)


def test_emulated_frame_ingest_slots(emu):
    ic.check_frame_ingest(emu)


def test_emulated_mapper_with_and_without_device_ingest(emu):
    """(on ONE emulator thread the mapping iterations add their gradients in a fixed order: the maps can be compared bit for bit)"""
    import ctypes
    omp = ctypes.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        ic.check_mapper(emu, deterministic_mapping=True)
    finally:
        omp.omp_set_num_threads(before)
