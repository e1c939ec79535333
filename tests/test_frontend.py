"""CPU: the cases of tests/frontend_cases.py through the Python twin of the drop-in call's autograd plumbing on the host-emulated kernels (the C++
front-end itself needs the device: tests/test_gpu_frontend.py runs both routes there).  The emulated block loop runs on ONE OpenMP thread here, so the
blend backward's float atomics sum in a fixed order and the gradients are held bit for bit."""
import pytest

from tests import frontend_cases as fc
from tests.pose_cases import one_openmp_thread


def one_thread(check, *args, **kw):
    with one_openmp_thread():
        check(*args, **kw)


@pytest.mark.parametrize("name,key", fc.INPUTS)
def test_input_forms(emu, name, key):
    one_thread(fc.check_input_forms, name, key, emu, False)


@pytest.mark.parametrize("name", fc.SCENES)
def test_all_forms_together(emu, name):
    one_thread(fc.check_all_forms_together, name, emu, False)


def test_settings_forms(emu):
    one_thread(fc.check_settings_forms, "plain", emu, False)


def test_expanded_scales(emu):
    one_thread(fc.check_expanded_scales, emu, False)


@pytest.mark.parametrize("name", fc.SCENES)
def test_scene_against_the_oracles(emu, oracle32, oracle64, name):
    one_thread(fc.check_scene_against_the_oracles, name, emu, False, oracle32, oracle64)


@pytest.mark.parametrize("which", ["means3D", "colour", "means2D"])
@pytest.mark.parametrize("name", ["plain", "sh3"])
def test_requires_grad_subset(emu, name, which):
    one_thread(fc.check_requires_grad_subset, name, which, emu, False)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_no_gradient_wanted(emu, name):
    one_thread(fc.check_no_gradient_wanted, name, emu, False)


@pytest.mark.parametrize("which", ["depth", "opacity"])
def test_colour_left_alone(emu, oracle64, oracle32, which):
    one_thread(fc.check_colour_left_alone, which, emu, False, oracle64, oracle32)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_second_backward(emu, name):
    one_thread(fc.check_second_backward, name, emu, False)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_optimistic_hit_and_miss(emu, oracle64, oracle32, name):
    one_thread(fc.check_hit_and_miss, name, emu, False, oracle64, oracle32)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_hit_and_miss_outside_capture(emu, name):
    one_thread(fc.check_hit_and_miss, name, emu, False, capture=False)


@pytest.mark.parametrize("which", ["P0", "P1", "culled"])
def test_p_edges(emu, which):
    one_thread(fc.check_p_edges, which, emu, False)
