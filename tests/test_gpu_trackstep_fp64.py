"""The tracking tail (gs_tracking_step, the pose-gradient finish, the per-workgroup pose rows, the loss rows) on the MI355X against
float64 / bit-exact references: the cases of tests/trackstep_cases.py.  The same cases run on the host-emulated build in tests/test_trackstep_fp64.py."""
import pytest

from tests import trackstep_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", C.STEP_P)
def test_gpu_step_gradient_against_fp64_in_two_tiers(hip, P):
    C.check_finish_through_step(hip, P)


def test_gpu_step_gradient_of_the_zero_column_is_fp32_torchs(hip):
    C.check_zero_column(hip)


@pytest.mark.parametrize("P", C.ACT_P)
def test_gpu_finish_at_a_host_pose_on_exact_integer_rows(hip, P):
    C.check_finish_through_activate(hip, P)


@pytest.mark.parametrize("P", C.SHARE_P)
def test_gpu_single_gaussian_pose_share_against_fp64(hip, P):
    C.check_single_share(hip, P)


@pytest.mark.parametrize("P,iso", C.DENSE)
def test_gpu_dense_pose_shares_against_fp64(hip, P, iso):
    C.check_dense_shares(hip, P, iso)


@pytest.mark.parametrize("W,H", C.LOSS_ROW_IMAGES)
def test_gpu_injected_loss_rows_weighted_bit_for_bit(hip, W, H):
    C.check_injected_loss_rows(hip, W, H)


@pytest.mark.parametrize("W,H", C.REAL_LOSS_IMAGES)
def test_gpu_tracking_loss_rows_against_fp64(hip, W, H):
    C.check_real_loss_rows(hip, W, H)


def test_gpu_pose_adam_translation_bit_for_bit(hip):
    C.check_translation_bits(hip)


def test_gpu_pose_adam_quaternion_bit_for_bit(hip):
    C.check_quaternion_bits(hip)


@pytest.mark.parametrize("name", C.EVOLUTION_COLUMNS)
def test_gpu_pose_adam_thirty_steps_each_against_fp64(hip, name):
    C.check_adam_evolution(hip, name)


@pytest.mark.parametrize("T,t", C.LAYOUTS)
def test_gpu_step_writes_its_column_only(hip, T, t):
    C.check_layout(hip, T, t)


@pytest.mark.parametrize("name", list(C.LOSS_SEQUENCES))
def test_gpu_candidate_rule(hip, name):
    C.check_candidate_rule(hip, name)
