"""The multi-view atlas render view by view against the oracles, on the device (tests/atlas_cases.py; the host-emulated twin is
tests/test_atlas.py)."""
import pytest

from tests import atlas_cases as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ac.NAMES)
def test_case(hip, oracle64, oracle32, name):
    ac.check_case(name, hip, oracle64, oracle32)


@pytest.mark.parametrize("name", ["pano3", "sh48"])
def test_settings_on_host_and_device(hip, oracle64, oracle32, name):
    ac.check_settings_on_host_and_device(name, hip, oracle64, oracle32)


@pytest.mark.parametrize("name", ["pano3", "sh48"])
def test_list_form_is_the_atlas(hip, oracle64, oracle32, name):
    ac.check_list_form(name, hip, oracle64, oracle32)


def test_look_around_gathers_the_judged_atlas(hip, oracle64, oracle32):
    ac.check_look_around(hip, oracle64, oracle32)


def test_look_around_nodes_gathers_the_judged_atlas(hip, oracle64, oracle32):
    ac.check_look_around_nodes(hip, oracle64, oracle32)
