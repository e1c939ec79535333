"""The optimiser, row-exchange and statistics kernels (adam.hip, rows.hip, stats.hip's two streaming kernels, gs_keyframe_overlap) on the
host-emulated build against float64 / exact references: the cases of tests/optimstep_cases.py.  The same cases run on the device in
tests/test_gpu_optimstep_fp64.py.  Device only, because the emulated build takes more than about ten seconds for them: the two sizes around
the non-temporal threshold (C.ADAM_STREAM_SIZES, 9.6 M elements), the 19-tensor batch with a tensor that takes a second trip in it (big=True; here
that tensor is small, the one with a second piece per trip stays) and the second trip of the row-block loop (C.ROWS_NARROW_BIG, C.ROWS_WIDE_BIG)."""
import pytest

from tests import optimstep_cases as C


@pytest.mark.parametrize("kind", C.ADAM_SETS)
def test_adam_rule_holds_for_the_fp32_mirror(kind):
    C.check_adam_mirror(kind)


def test_row_index_of_the_rows_kernel_is_exact():
    C.check_row_index_rule()


@pytest.mark.parametrize("kind", C.ADAM_SETS)
def test_emulated_adam_step_against_fp64(emu, kind):
    C.check_adam_set("cpu", kind)


@pytest.mark.parametrize("kind", C.ADAM_SETS)
def test_emulated_adam_step_equals_the_fp32_sequence_bit_for_bit(emu, kind):
    C.check_adam_bits_equal_mirror("cpu", kind)


def test_emulated_adam_thirty_steps_each_against_fp64(emu):
    C.check_adam_evolution("cpu")


def test_emulated_adam_non_finite_gradient_stays_in_its_element(emu):
    C.check_adam_nonfinite("cpu")


@pytest.mark.parametrize("n", C.ADAM_SIZES)
def test_emulated_adam_sizes_single_equals_multi_and_fp64(emu, n):
    C.check_adam_size("cpu", n)


def test_emulated_adam_nineteen_tensors_three_launches(emu):
    C.check_adam_multi("cpu", big=False)


def test_emulated_gaussian_adam_against_torch_adam_fp64(emu):
    C.check_gaussian_adam_api("cpu")


def test_emulated_adam_refuses_misaligned_tensors(emu):
    C.check_adam_refuses_misaligned("cpu")


def test_emulated_gaussian_adam_refusal_leaves_state_and_counters(emu):
    C.check_gaussian_adam_refuses_misaligned("cpu")


def test_emulated_backward_adam_refuses_misaligned_moments(emu):
    C.check_backward_adam_refuses_misaligned("cpu")


@pytest.mark.parametrize("widths", C.ROW_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_emulated_pack_unpack_columns_exact(emu, widths):
    for n in C.row_counts(widths):
        C.check_rows_pack_unpack("cpu", widths, n)


@pytest.mark.parametrize("widths", C.ROW_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_emulated_adam_rows_equals_multi_and_fp64(emu, widths):
    for n in C.row_counts(widths):
        C.check_rows_adam("cpu", widths, n)


def test_emulated_rows_take_any_four_byte_aligned_pointer(emu):
    C.check_rows_pack_unpack("cpu", (3, 3, 4, 1, 3), 257, offset1=True)
    C.check_rows_adam("cpu", (3, 3, 4, 1, 3), 257, offset1=True)


def test_emulated_rows_refusals(emu):
    C.check_rows_refusals("cpu")


@pytest.mark.parametrize("P", C.STATS_P)
def test_emulated_visibility_stats_exact(emu, P):
    C.check_visibility_stats("cpu", P)


def test_emulated_fused_forward_follows_the_same_nan_rule(emu):
    C.check_fused_visibility_nan_rule("cpu")


@pytest.mark.parametrize("P", C.STATS_P)
def test_emulated_accumulate_grad2d_against_fp64(emu, P):
    C.check_accumulate_grad2d("cpu", P)


@pytest.mark.parametrize("n_kf", C.OVERLAP_KF)
@pytest.mark.parametrize("n_pts", C.OVERLAP_NPTS)
def test_emulated_keyframe_overlap_against_fp64(emu, n_pts, n_kf):
    C.check_keyframe_overlap("cpu", n_pts, n_kf)


def test_emulated_keyframe_overlap_edges(emu):
    C.check_keyframe_overlap("cpu", 257, 3, edge=0)
    C.check_keyframe_overlap("cpu", 257, 3, edge=20, W=40, H=30)          # W - edge <= edge: nothing can be counted
