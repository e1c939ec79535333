"""CPU (host-emulated kernels): the map-quality evaluation (activesplat_amd/evaluate.py; gs_eval_frame_layout, gs_eval_frame).  The checks, their
references and tolerances: tests/eval_cases.py.  The same checks run on the MI355X in tests/test_gpu_eval.py."""
import numpy as np
import pytest
import torch

from tests import eval_cases as ec


def test_the_golden_is_close_to_the_fp64_restatement():
    """the reference's fp32 torch sums against the fp64 restatement of the same arithmetic: the measured distance (printed) is what the kernel
    tests add to the kernel's bound; it must itself be fp32-sized"""
    d = ec.golden_distance()
    assert d["psnr"] < 1e-4 and d["l1"] < 1e-6 and d["rmse"] < 1e-6 and d["ssim"] < 1e-5, d


def test_the_restated_calc_ssim_is_this_repositorys():
    """the same-padding restatement is not new arithmetic: in fp32 it is mapping.calc_ssim on the golden pairs, and the reference's own value"""
    from activesplat_amd import mapping as M
    g = ec.golden()
    for f in range(3):
        c = ec.golden_case(g, f)
        ours = float(M.calc_ssim(c["im"], c["gt"]))
        assert abs(ours - g["calc_ssim"][f]) <= 2 ** -22                       # (both are fp32 means of the same fp32 map)
        x, y = c["im"].double(), c["gt"].double()
        assert abs(ec.ssim_same(x, y, rounded_window=True) - float(M.calc_ssim(x, y))) <= 1e-12
        shift = abs(ec.ssim_same(x, y) - ec.ssim_same(x, y, rounded_window=True))
        print(f"frame {f}: rounding the 2-D window to fp32 moves the fp64 SSIM by {shift:.2e}")
        assert shift <= 4e-6                                                   # (fp32-sized: sum of the window off by ~1e-8 against variances of 1e-3)


@pytest.mark.parametrize("H,W", ec.MS_SIZES)
def test_no_ms_ssim_case_sits_on_the_clamp(H, W):
    worst = ec.condition(H, W)
    print(f"smallest |term| at {H}x{W}: {worst:.3f}")
    assert worst >= 0.05


def test_the_clamp_case_is_far_below_zero():
    terms = ec.ms_terms(*ec.masked_pair(ec.inverted(161, 163), False, False))
    ec.assert_clamp_case(terms)
    assert ec.ms_value(terms) == 0.0


def test_the_pooling_rule_and_level_sizes():
    """avg_pool2d(kernel 2, padding = size % 2): size n -> n // 2 + n % 2, the zero padding counted in the divisor"""
    x = torch.arange(1.0, 16.0).reshape(1, 1, 3, 5)
    p = torch.nn.functional.avg_pool2d(x, 2, padding=[1, 1])
    assert tuple(p.shape[2:]) == (2, 3) and float(p[0, 0, 0, 0]) == 0.25 and float(p[0, 0, 1, 1]) == (7 + 8 + 12 + 13) / 4


def test_the_evaluation_has_no_cpu_fallback():
    import os
    from activesplat_amd import _lib
    from activesplat_amd import evaluate as E
    _lib.unload_for_tests()
    have = os.path.exists(_lib.LIB_PATH)
    z = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.frame_metrics(z, z[0], z[0], z, z[0], 0.98, ms_ssim=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.MapEvaluator(8, 8, 4, device="cpu")
    assert have or _lib._lib is None


def test_align_and_evaluate_ate_match_the_golden():
    ec.check_ate_golden()


@pytest.mark.parametrize("H,W", ec.SMALL)
def test_emulated_sums_and_flags(emu, H, W):
    ec.check_sums_and_flags(emu, H, W)


@pytest.mark.parametrize("H,W", ec.SMALL)
def test_emulated_ssim_same(emu, H, W):
    ec.check_ssim_same(emu, H, W)


@pytest.mark.parametrize("H,W", ec.MS_SIZES)
def test_emulated_ms_ssim(emu, H, W):
    ec.check_ms_ssim(emu, H, W)


def test_emulated_clamp(emu):
    ec.check_clamp(emu)


def test_emulated_identities_and_ieee_rows(emu):
    ec.check_identities(emu)


def test_emulated_golden(emu):
    ec.check_golden(emu)


def test_emulated_two_evaluators_are_bit_identical(emu):
    ec.check_repeatable(emu)


def test_emulated_refusals_and_write(emu):
    ec.check_refusals_and_write(emu)


def test_emulated_evaluate_map_and_the_mapper_hook(emu):
    ec.check_evaluate_map(emu)


def test_emulated_evaluate_map_with_ms_ssim(emu):
    ec.check_evaluate_map_ms_ssim(emu)


def test_emulated_mapper_default_is_unchanged(emu):
    """(on ONE emulator thread the mapping iterations add their gradients in a fixed order: the maps can be compared bit for bit)"""
    import ctypes
    omp = ctypes.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        ec.check_mapper_default_is_unchanged(emu, deterministic_mapping=True)
    finally:
        omp.omp_set_num_threads(before)
