"""GPU: the C++ autograd front-end of the drop-in call (csrc/torch_frontend.cpp) and its Python twin on the MI355X -- the cases of
tests/frontend_cases.py, every one through both routes, against the canonical call of the same values and against the oracles."""
import pytest

from tests import frontend_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[True, False], ids=["frontend", "twin"])
def route(request, hip):
    if request.param:
        from activesplat_amd import _frontend
        _frontend.get()                                      # (the run is about the C++ route: no quiet use of the twin)
    return request.param


@pytest.mark.parametrize("name,key", fc.INPUTS)
def test_input_forms(hip, route, name, key):
    fc.check_input_forms(name, key, hip, route)


@pytest.mark.parametrize("name", fc.SCENES)
def test_all_forms_together(hip, route, name):
    fc.check_all_forms_together(name, hip, route)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_settings_forms(hip, route, name):
    fc.check_settings_forms(name, hip, route)


def test_expanded_scales(hip, route):
    fc.check_expanded_scales(hip, route)


@pytest.mark.parametrize("name", fc.SCENES)
def test_scene_against_the_oracles(hip, route, oracle32, oracle64, name):
    fc.check_scene_against_the_oracles(name, hip, route, oracle32, oracle64)


@pytest.mark.parametrize("which", ["means3D", "colour", "means2D"])
@pytest.mark.parametrize("name", ["plain", "sh3", "tiles306"])
def test_requires_grad_subset(hip, route, name, which):
    fc.check_requires_grad_subset(name, which, hip, route)


@pytest.mark.parametrize("name", fc.SCENES)
def test_no_gradient_wanted(hip, route, name):
    fc.check_no_gradient_wanted(name, hip, route)


@pytest.mark.parametrize("which", ["depth", "opacity"])
def test_colour_left_alone(hip, route, oracle64, oracle32, which):
    fc.check_colour_left_alone(which, hip, route, oracle64, oracle32)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_second_backward(hip, route, name):
    fc.check_second_backward(name, hip, route)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_optimistic_hit_and_miss(hip, route, oracle64, oracle32, name):
    fc.check_hit_and_miss(name, hip, route, oracle64, oracle32)


@pytest.mark.parametrize("name", ["plain", "tiles306"])
def test_hit_and_miss_outside_capture(hip, route, name):
    fc.check_hit_and_miss(name, hip, route, capture=False)


@pytest.mark.parametrize("which", ["P0", "P1", "culled"])
def test_p_edges(hip, route, which):
    fc.check_p_edges(which, hip, route)
