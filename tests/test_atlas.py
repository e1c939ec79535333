"""The multi-view atlas render view by view against the oracles, on the host-emulated kernels (tests/atlas_cases.py; the device twin is
tests/test_gpu_atlas.py)."""
import pytest

from tests import atlas_cases as ac
from tests import blendpix_cases as bp


def test_fp32_oracle_alone_stays_under_half_the_floor(emu, oracle64, oracle32):
    """The floor is blendpix_cases' and is not re-tuned here: the fp32 oracle's largest |o_32 - o_64| / A_p over every case, view, pixel and
    output is printed and must be at most FLOOR_F / 2; so must the settling stay under its cap (asserted where a reference is built).  The
    oracles alone: the kernels only activate the parameters of the two panorama cases, as look_around does."""
    worst = (0.0, None)
    for name in ac.NAMES:
        _case, ref = ac.reference(name, emu, oracle64, oracle32)
        e, where = ref["oracle32_error"]
        print(f"[atlas] fp32 oracle alone: {name:12s} {e:.3e} of A_p (view, output: {where}); predicted flips {ref['flips']}; dimmed {ref['dimmed']} of {ref['P']}")
        assert ref["dimmed"] < ac.SETTLE_CAP * ref["P"], name
        worst = max(worst, (e, name))
    print(f"[atlas] fp32 oracle alone: largest per-pixel error {worst[0]:.3e} ({worst[1]}); FLOOR_F / 2 = {0.5 * bp.FLOOR_F:g}")
    assert worst[0] <= 0.5 * bp.FLOOR_F, worst


@pytest.mark.parametrize("name", ac.NAMES)
def test_case(emu, oracle64, oracle32, name):
    ac.check_case(name, emu, oracle64, oracle32)


@pytest.mark.parametrize("name", ["pano3", "sh48"])
def test_settings_on_host_and_device(emu, oracle64, oracle32, name):
    ac.check_settings_on_host_and_device(name, emu, oracle64, oracle32)


@pytest.mark.parametrize("name", ["pano3", "sh48"])
def test_list_form_is_the_atlas(emu, oracle64, oracle32, name):
    ac.check_list_form(name, emu, oracle64, oracle32)


def test_look_around_gathers_the_judged_atlas(emu, oracle64, oracle32):
    ac.check_look_around(emu, oracle64, oracle32)


def test_look_around_nodes_gathers_the_judged_atlas(emu, oracle64, oracle32):
    ac.check_look_around_nodes(emu, oracle64, oracle32)
