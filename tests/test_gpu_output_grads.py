"""GPU: gradients of every image output (differentiable_outputs=) on the MI355X -- the cases of tests/output_grad_cases.py, the drop-in case
through the C++ autograd front-end as well as through the Python twin."""
import pytest

from tests import output_grad_cases as og

pytestmark = pytest.mark.gpu


def test_silhouette_only_loss_has_a_gradient(hip, oracle64, oracle32):
    og.check_silhouette_only(hip, oracle64, oracle32)


@pytest.mark.parametrize("name", og.SCENES)
def test_all_outputs_against_the_two_pass_oracle(hip, oracle64, oracle32, name):
    og.check_all_outputs(name, hip, oracle64, oracle32)


@pytest.mark.parametrize("frontend", [True, False])
@pytest.mark.parametrize("name", ["plain", "partial"])
def test_dropin_depth_and_opacity(hip, oracle64, oracle32, name, frontend):
    if frontend:
        from activesplat_amd import _frontend
        _frontend.get()                                      # (the run is about the C++ route: no quiet use of the twin)
    og.check_dropin(name, hip, oracle64, oracle32, frontend)


def test_raw_parameter_path(hip):
    og.check_raw(hip)


@pytest.mark.parametrize("name", ["plain", "few_tile", "chained"])
def test_background_identity(hip, name):
    og.check_background_identity(name, hip)


def test_defaults_unchanged(hip):
    og.check_defaults(hip)


def test_refusals(hip):
    og.check_refusals(hip)


def test_empty_scenes(hip):
    og.check_empty(hip)
