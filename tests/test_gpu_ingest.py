"""GPU (-m gpu): the frame ingest on the MI355X -- the checks of tests/ingest_cases.py (where the expected values come from is stated there) on the
real kernel."""
import pytest

from tests import ingest_cases as ic

pytestmark = pytest.mark.gpu


def test_resize_shapes(hip):
    ic.check_resize_shapes(hip)


def test_rounding(hip):
    ic.check_rounding(hip)


def test_depth_bit_patterns(hip):
    ic.check_depth_bits(hip)


def test_two_outputs_in_one_call(hip):
    ic.check_two_outputs(hip)


def test_two_calls_are_bit_identical(hip):
    ic.check_repeatable(hip)


def test_refusals(hip):
    ic.check_refusals(hip)


def test_frame_ingest_slots(hip):
    ic.check_frame_ingest(hip)


def test_mapper_with_and_without_device_ingest(hip):
    """(the backward adds with hardware float atomics on the GPU: only the frame tensors are compared)"""
    ic.check_mapper(hip, deterministic_mapping=False)
