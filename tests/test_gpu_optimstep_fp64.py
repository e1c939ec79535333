"""The optimiser, row-exchange and statistics kernels (adam.hip, rows.hip, stats.hip's two streaming kernels, gs_keyframe_overlap) on the MI355X
against float64 / exact references: the cases of tests/optimstep_cases.py.  The same cases run on the host-emulated build in
tests/test_optimstep_fp64.py; the sizes that build is too slow for run here only."""
import pytest

from tests import optimstep_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", C.ADAM_SETS)
def test_gpu_adam_step_against_fp64(hip, kind):
    C.check_adam_set(hip, kind)


@pytest.mark.parametrize("kind", C.ADAM_SETS)
def test_gpu_adam_step_equals_the_fp32_sequence_bit_for_bit(hip, kind):
    C.check_adam_bits_equal_mirror(hip, kind)


def test_gpu_adam_thirty_steps_each_against_fp64(hip):
    C.check_adam_evolution(hip)


def test_gpu_adam_non_finite_gradient_stays_in_its_element(hip):
    C.check_adam_nonfinite(hip)


@pytest.mark.parametrize("n", C.ADAM_SIZES + C.ADAM_STREAM_SIZES)
def test_gpu_adam_sizes_single_equals_multi_and_fp64(hip, n):
    C.check_adam_size(hip, n)


def test_gpu_adam_nineteen_tensors_three_launches(hip):
    C.check_adam_multi(hip, big=True)


def test_gpu_gaussian_adam_against_torch_adam_fp64(hip):
    C.check_gaussian_adam_api(hip)


def test_gpu_adam_refuses_misaligned_tensors(hip):
    C.check_adam_refuses_misaligned(hip)


def test_gpu_gaussian_adam_refusal_leaves_state_and_counters(hip):
    C.check_gaussian_adam_refuses_misaligned(hip)


def test_gpu_backward_adam_refuses_misaligned_moments(hip):
    C.check_backward_adam_refuses_misaligned(hip)


@pytest.mark.parametrize("widths", C.ROW_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_gpu_pack_unpack_columns_exact(hip, widths):
    for n in C.row_counts(widths):
        C.check_rows_pack_unpack(hip, widths, n)


@pytest.mark.parametrize("widths", C.ROW_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_gpu_adam_rows_equals_multi_and_fp64(hip, widths):
    for n in C.row_counts(widths):
        C.check_rows_adam(hip, widths, n)


def test_gpu_rows_take_any_four_byte_aligned_pointer(hip):
    C.check_rows_pack_unpack(hip, (3, 3, 4, 1, 3), 257, offset1=True)
    C.check_rows_adam(hip, (3, 3, 4, 1, 3), 257, offset1=True)


def test_gpu_rows_refusals(hip):
    C.check_rows_refusals(hip)


@pytest.mark.parametrize("P", C.STATS_P)
def test_gpu_visibility_stats_exact(hip, P):
    C.check_visibility_stats(hip, P)


def test_gpu_fused_forward_follows_the_same_nan_rule(hip):
    C.check_fused_visibility_nan_rule(hip)


@pytest.mark.parametrize("P", C.STATS_P)
def test_gpu_accumulate_grad2d_against_fp64(hip, P):
    C.check_accumulate_grad2d(hip, P)


@pytest.mark.parametrize("n_kf", C.OVERLAP_KF)
@pytest.mark.parametrize("n_pts", C.OVERLAP_NPTS)
def test_gpu_keyframe_overlap_against_fp64(hip, n_pts, n_kf):
    C.check_keyframe_overlap(hip, n_pts, n_kf)


def test_gpu_keyframe_overlap_edges(hip):
    C.check_keyframe_overlap(hip, 257, 3, edge=0)
    C.check_keyframe_overlap(hip, 257, 3, edge=20, W=40, H=30)          # W - edge <= edge: nothing can be counted


@pytest.mark.parametrize("widths,n", [((3, 3, 4, 1, 3), C.ROWS_NARROW_BIG), ((3, 48, 4, 1, 3), C.ROWS_WIDE_BIG)], ids=["narrow", "wide"])
def test_gpu_rows_second_trip_of_the_block_loop(hip, widths, n):
    C.check_rows_pack_unpack(hip, widths, n)
    C.check_rows_adam(hip, widths, n, windows=((5, n - 7, n),))            # row_lo off the block grid, seven padding rows in the shard
