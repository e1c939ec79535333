"""CPU: gradients of every image output (differentiable_outputs=) on the host-emulated kernels -- the cases of tests/output_grad_cases.py.
The emulated build takes the Python twin of the autograd plumbing only; the C++ front-end's run of the drop-in case is in the GPU file."""
import pytest

from tests import output_grad_cases as og


def test_silhouette_only_loss_has_a_gradient(emu, oracle64, oracle32):
    og.check_silhouette_only(emu, oracle64, oracle32)


@pytest.mark.parametrize("name", og.SCENES)
def test_all_outputs_against_the_two_pass_oracle(emu, oracle64, oracle32, name):
    og.check_all_outputs(name, emu, oracle64, oracle32)


@pytest.mark.parametrize("name", ["plain", "partial"])
def test_dropin_depth_and_opacity(emu, oracle64, oracle32, name):
    og.check_dropin(name, emu, oracle64, oracle32, frontend=False)


def test_raw_parameter_path(emu):
    og.check_raw(emu)


@pytest.mark.parametrize("name", ["plain", "few_tile", "chained"])
def test_background_identity(emu, name):
    og.check_background_identity(name, emu)


def test_defaults_unchanged(emu):
    og.check_defaults(emu)


def test_refusals(emu):
    og.check_refusals(emu)


def test_empty_scenes(emu):
    og.check_empty(emu)
