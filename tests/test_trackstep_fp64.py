"""The tracking tail (gs_tracking_step, the pose-gradient finish, the per-workgroup pose rows, the loss rows) on the host-emulated build against
float64 / bit-exact references: the cases of tests/trackstep_cases.py.  The same cases run on the device in tests/test_gpu_trackstep_fp64.py."""
import pytest

from tests import trackstep_cases as C


@pytest.mark.parametrize("name", C.EVOLUTION_COLUMNS)
def test_pose_adam_rule_holds_for_the_fp32_mirror(name):
    C.check_adam_evolution("cpu", name, kernel=False)


@pytest.mark.parametrize("P", C.STEP_P)
def test_emulated_step_gradient_against_fp64_in_two_tiers(emu, P):
    C.check_finish_through_step("cpu", P)


def test_emulated_step_gradient_of_the_zero_column_is_fp32_torchs(emu):
    C.check_zero_column("cpu")


@pytest.mark.parametrize("P", C.ACT_P)
def test_emulated_finish_at_a_host_pose_on_exact_integer_rows(emu, P):
    C.check_finish_through_activate("cpu", P)


@pytest.mark.parametrize("P", C.SHARE_P)
def test_emulated_single_gaussian_pose_share_against_fp64(emu, P):
    C.check_single_share("cpu", P)


@pytest.mark.parametrize("P,iso", C.DENSE)
def test_emulated_dense_pose_shares_against_fp64(emu, P, iso):
    C.check_dense_shares("cpu", P, iso)


@pytest.mark.parametrize("W,H", C.LOSS_ROW_IMAGES)
def test_emulated_injected_loss_rows_weighted_bit_for_bit(emu, W, H):
    C.check_injected_loss_rows("cpu", W, H)


@pytest.mark.parametrize("W,H", C.REAL_LOSS_IMAGES)
def test_emulated_tracking_loss_rows_against_fp64(emu, W, H):
    C.check_real_loss_rows("cpu", W, H)


def test_emulated_pose_adam_translation_bit_for_bit(emu):
    C.check_translation_bits("cpu")


def test_emulated_pose_adam_quaternion_bit_for_bit(emu):
    C.check_quaternion_bits("cpu")


@pytest.mark.parametrize("name", C.EVOLUTION_COLUMNS)
def test_emulated_pose_adam_thirty_steps_each_against_fp64(emu, name):
    C.check_adam_evolution("cpu", name)


@pytest.mark.parametrize("T,t", C.LAYOUTS)
def test_emulated_step_writes_its_column_only(emu, T, t):
    C.check_layout("cpu", T, t)


@pytest.mark.parametrize("name", list(C.LOSS_SEQUENCES))
def test_emulated_candidate_rule(emu, name):
    C.check_candidate_rule("cpu", name)
