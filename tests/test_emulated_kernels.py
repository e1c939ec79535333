"""CPU: the UNMODIFIED HIP kernel sources, compiled against the host emulator in tests/hipemu, run the
whole C-ABI pipeline (preprocess -> scan -> emit -> sort stand-in -> ranges -> blend -> backward) and
must agree with the oracle.  This is a kernel-logic check for the container without a GPU; the
parity tests proper are tests/test_gpu_parity.py (-m gpu), which run the same cases on the MI355X.
Integer artefacts and the per-Gaussian screen-space records are bit-identical to the fp32 oracle; the
images are compared at the same fp32 tolerance as on the GPU (the blend evaluates 2^(log2e-scaled power))."""
import numpy as np
import pytest
import torch

from tests import parity_cases as pc
from tests import util


@pytest.mark.parametrize("case", pc.CASES)
def test_emulated_forward_matches_oracle(emu, oracle32, case):
    rs, rv = pc.build_case(case, emu)
    pc.check_forward(rs, rv, oracle32)
    assert util.artefacts()["path"] == 1        # tile-binning + LDS sort path


@pytest.mark.parametrize("case,path", [("merge_tiles", 1), ("merge_passes", 1), ("merge_passes_even", 1), ("bucket_lists", 1), ("bucket_lists_long", 1),
                                       ("crowded_depth", 1), ("crowded_depth_long", 1), ("equal_depth", 1), ("bucket_lists_big", 1), ("crowded_depth_big", 1)])
def test_emulated_big_tile_lists(emu, oracle32, case, path):
    """tile lists beyond one sort chunk: sorted chunks + LDS rank-merge; beyond the LDS capacity: pairwise merge passes."""
    rs, rv = pc.build_case(case, emu)
    pc.check_forward(rs, rv, oracle32)
    assert util.artefacts()["path"] == path


@pytest.mark.parametrize("case", ["basic", "ragged_image", "all_culled", "huge_gaussians", "dense_overdraw", "one_gaussian", "equal_depth", "merge_tiles"])   # (merge_tiles: 22 run blocks of the sort in six workgroups; equal_depth: 9000 keys that differ in the
# tile bits only inside a tile -- the order inside a tile is the STABILITY of sort_radix.hip, pass after pass)
def test_emulated_forward_radix_path_matches_oracle(emu, oracle32, case):
    rs, rv = pc.build_case(case, emu)
    pc.set_sort_path("radix")
    try:
        pc.check_forward(rs, rv, oracle32)
        assert util.artefacts()["path"] == 2
    finally:
        pc.set_sort_path("auto")


@pytest.mark.parametrize("case", ["basic", "ragged_image", "posed_white_bg", "scale_modifier", "dense_overdraw", "mixed_sizes",
                                  "huge_gaussians", "all_culled", "sh3", "sh2_ragged", "sh3_half_culled", "cov3d_precomp", "lookaround_intrinsics",
                                  "scale_modifier_001", "topdown_1000m", "topdown_1000m_white"] + pc.NONFINITE_CASES)
def test_emulated_backward_matches_fp64_oracle(emu, oracle64, case):
    rs, rv = pc.build_case(case, emu)
    pc.check_backward(rs, rv, oracle64)


def test_emulated_adam_matches_torch(emu):
    import ctypes as C
    from activesplat_amd import _lib
    lib = _lib.get()
    torch.manual_seed(0)
    n = 1003
    p = torch.randn(n); ref = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [ref], "lr": 1e-3}], lr=0.0, eps=1e-15)
    m, v = torch.zeros(n), torch.zeros(n)
    for step in range(1, 5):
        g = torch.randn(n)
        ref.grad = g.clone(); opt.step()
        _lib.check(lib.gs_adam_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 0.9, 0.999, 1e-15,
                                    step, None))
        np.testing.assert_allclose(p.numpy(), ref.detach().numpy(), rtol=2e-6, atol=1e-7)


def test_emulated_multi_tensor_adam_equals_per_tensor_launches(emu):
    """11 tensors of ragged sizes (two launches of <= 8) must be bit-identical to 11 single-tensor steps."""
    from activesplat_amd import _lib
    lib = _lib.get()
    g0 = torch.Generator().manual_seed(4)
    sizes = [1, 3, 4, 5, 1003, 4096, 0, 777, 2, 64, 1501]
    one = [[torch.randn(n, generator=g0) for _ in range(4)] for n in sizes]          # p, g, m, v
    for t in one:
        t[3].abs_()
    many = [[x.clone() for x in t] for t in one]
    for i, (p, g, m, v) in enumerate(one):
        _lib.check(lib.gs_adam_step(p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3 * (i + 1), 0.9, 0.999,
                                    1e-15, i + 1, None))
    arr = (_lib.GsAdamTensor * len(sizes))(*[_lib.GsAdamTensor(p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                               1e-3 * (i + 1), 0.9, 0.999, 1e-15, i + 1, 0)
                                             for i, (p, g, m, v) in enumerate(many)])
    _lib.check(lib.gs_adam_step_multi(len(sizes), arr, None))
    for a, b in zip(one, many):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert lib.gs_adam_step_multi(1, (_lib.GsAdamTensor * 1)(_lib.GsAdamTensor(4, None, None, None, None, 1e-3, 0.9, 0.999, 1e-15, 1, 0)), None) != 0


@pytest.mark.parametrize("case", ["basic", "posed_white_bg", "ragged_image", "sh2", "dense_overdraw", "mixed_sizes"])
def test_emulated_fused_rgbd_matches_two_passes_and_oracle(emu, oracle64, case):
    rs, rv = pc.build_case(case, emu)
    pc.check_fused_rgbd(rs, rv, oracle64)


def test_emulated_fused_loss_equals_two_pass_loss(emu):
    """mapping.get_loss(fused=True) == the reference-style two-pass loss, value and parameter gradients."""
    from activesplat_amd import mapping as M
    from tests.test_parallel import _scene
    out = []
    for fused, floss, finp in ((False, False, False), (True, False, False), (True, True, True)):
        params, kfs = _scene(n=500)
        n = params["means3D"].shape[0]
        variables = {k: torch.zeros(n) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
        loss, variables, _ = M.get_loss(params, kfs[1], variables, 1, dict(im=0.5, depth=1.0), fused=fused, fused_loss=floss,
                                        fused_inputs=finp)
        loss.backward()
        out.append((float(loss.detach()), {k: v.grad.clone() for k, v in params.items() if v.grad is not None},
                    variables["max_2D_radius"].clone(), variables["seen"].clone()))
    for o in out[1:]:
        assert abs(out[0][0] - o[0]) < 2e-6 * abs(out[0][0])
        assert torch.equal(out[0][2], o[2]) and torch.equal(out[0][3], o[3])
        for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
            a, b = out[0][1][k], o[1][k]
            assert float((a - b).norm() / a.norm()) < 2e-4, k


def test_emulated_fused_loss_masks_nonfinite_depth_pixels(emu):
    pc.check_loss_masks_nonfinite_depth("cpu")


def test_emulated_raw_parameter_rasteriser_equals_the_activation_kernels(emu):
    pc.check_raw_parameter_mode("cpu")
    pc.check_raw_parameter_mode_sh("cpu")
    pc.check_raw_parameter_mode_nonfinite("cpu")
    assert pc.check_raw_entry_random_draw(1, "cpu") == "ok"                 # one draw of the device sweep (1111 Gaussians, 96 x 157): the same checker code


def test_emulated_loss_call_fully_fused_equals_the_reference_call_pattern(emu):
    """Two draws of the device sweep of profiles/r05_fuzz_get_loss.txt: 1 (1111 Gaussians, 96 x 157) agrees outright; 604 (11 384 large splats on 31 x 33 pixels) is the
    sweep's depth-tie scene, which the emulated kernels reproduce with the device's numbers -- the classifier, not a tolerance, lets it through."""
    assert pc.check_get_loss_random_draw(1, "cpu") == "ok"
    v = pc.check_get_loss_random_draw(604, "cpu")
    assert v[0] == "depth tie" and v[1] == "unnorm_rotations", v


def test_emulated_adam_inside_the_backward_equals_backward_plus_step(emu):
    """(one OpenMP thread for the emulator's block loop: the blend backward's float atomics then sum in a fixed order and the two loops can be
    compared bit for bit)"""
    import ctypes
    omp = ctypes.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        pc.check_adam_inside_the_backward(emu)
    finally:
        omp.omp_set_num_threads(before)


def test_emulated_adam_inside_the_backward_is_applied_once_and_never_silently(emu):
    pc.check_adam_backward_guards(emu)


def test_emulated_unrendered_rows_of_a_keyframe_batch_are_written(emu):
    pc.check_unrendered_rows_are_written(emu)


def test_emulated_unrendered_rows_of_dense_gradients_are_zero(emu):
    pc.check_unrendered_rows_of_dense_gradients(emu)


def test_emulated_mapping_iteration_without_autograd_equals_the_autograd_path(emu):
    import ctypes
    omp = ctypes.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        pc.check_mapping_iteration_without_autograd(emu)
    finally:
        omp.omp_set_num_threads(before)


def test_emulated_optimistic_launch_hit_and_miss_equal_exact_launch(emu):
    pc.check_optimistic_launch(emu)
    pc.check_optimistic_tile_list_growth(emu)


def test_emulated_render_views_leaves_the_capacity_table_alone(emu):
    pc.check_render_views_leaves_the_capacity_table_alone(emu)


def test_emulated_raw_inputs_by_name_and_the_direct_entry(emu):
    import ctypes
    omp = ctypes.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)                  # (one thread: the emulated atomics then sum in one order, and equal means equal)
    try:
        pc.check_raw_inputs_by_name(emu)
    finally:
        omp.omp_set_num_threads(before)


def test_emulated_densification_statistics_kernels(emu):
    from activesplat_amd import optim as O
    g0 = torch.Generator().manual_seed(8)
    P = 1003
    radius = torch.randint(0, 9, (P,), generator=g0, dtype=torch.int32)
    radius[::3] = 0
    mx = torch.rand(P, generator=g0) * 6
    ref_seen = radius > 0
    ref_mx = torch.maximum(mx, radius.float())
    seen = O.visibility_stats(radius, mx)
    assert seen.dtype == torch.bool and torch.equal(seen, ref_seen) and torch.equal(mx, ref_mx)
    m2d = torch.zeros(P, 3, requires_grad=True)
    m2d.grad = torch.randn(P, 3, generator=g0)
    accum, denom = torch.rand(P, generator=g0), torch.randint(0, 5, (P,), generator=g0).float()
    ref_acc, ref_den = accum.clone(), denom.clone()
    ref_acc[ref_seen] += torch.norm(m2d.grad[ref_seen, :2], dim=-1)
    ref_den[ref_seen] += 1
    O.accumulate_mean2d_gradient({"means2D": m2d, "seen": seen, "means2D_gradient_accum": accum, "denom": denom})
    assert torch.allclose(accum, ref_acc, rtol=1e-6, atol=0) and torch.equal(denom, ref_den)
    # dtype the kernel does not take: same result through the torch fallback
    mx64 = torch.zeros(P, dtype=torch.float64)
    assert torch.equal(O.visibility_stats(radius, mx64), ref_seen) and torch.equal(mx64, radius.double())


def test_emulated_segmented_forward(emu, oracle32):
    pc.check_segmented_forward(emu, oracle32)



def test_whole_quadrants_on_small_images(emu, oracle32, oracle64):
    pc.check_whole_quadrants_on_small_images(emu, oracle32, oracle64)


def test_emulated_chained_backward(emu, oracle64, oracle32):
    pc.check_chained_backward(emu, oracle64, oracle32=oracle32)


def test_emulated_chained_backward_fails_safe(emu):
    pc.check_chained_backward_fails_safe(emu, N=2500)


def test_emulated_few_tile_backward_segments(emu, oracle64, oracle32):
    pc.check_few_tile_backward_segments(emu, oracle64, oracle32, N=9000, W=48, H=48)
