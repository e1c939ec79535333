"""CPU (host-emulated kernels): the mesh RGB-D sensor (activesplat_amd/sensor.py; gs_mesh_render).  The checks and where their expected values come
from: tests/mesh_cases.py.  The same checks run on the MI355X in tests/test_gpu_mesh_sensor.py."""
import numpy as np
import pytest
import torch

from tests import mesh_cases as mc


def test_the_restatement_on_a_case_worked_by_hand():
    """one triangle at z = 2 seen through f = 1, centre (1, 1), 3 x 3 pixels: the rays are (x - 1, y - 1, 1), so pixel (x, y) meets the plane at
    (2 (x - 1), 2 (y - 1), 2); the triangle (-1, -1), (3, -1), (-1, 3) holds the points with X >= -1, Y >= -1, X + Y <= 2"""
    v = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], np.float32)
    c = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    r = mc.restate(v, np.array([[0, 1, 2]]), c, (1.0, 1.0, 1.0, 1.0), np.eye(4), 3, 3, 0.05)
    assert r["tri_id"].tolist() == [[-1, -1, -1], [-1, 0, 0], [-1, 0, -1]]
    assert r["depth"].tolist() == [[0, 0, 0], [0, 2, 2], [0, 2, 0]]
    # pixel (1, 1) is the point (0, 0): weights (1/2, 1/4, 1/4) -> floor(127.5 + 0.5), floor(63.75 + 0.5)
    assert r["color"][1, 1].tolist() == [128, 64, 64]
    # pixel (2, 1) is the point (2, 0), on the edge X + Y = 2: flagged; pixel (1, 1) is well inside
    assert r["flagged"][1, 2] and not r["flagged"][1, 1]
    # float32 gives the same image here
    r32 = mc.restate(v, np.array([[0, 1, 2]]), c, (1.0, 1.0, 1.0, 1.0), np.eye(4), 3, 3, 0.05, np.float32)
    assert np.array_equal(r32["tri_id"], r["tri_id"]) and r32["depth"].dtype == np.float32


def test_the_mesh_sensor_has_no_cpu_fallback():
    import os
    from activesplat_amd import _lib
    from activesplat_amd import sensor as S
    _lib.unload_for_tests()
    have = os.path.exists(_lib.LIB_PATH)
    v, t, c = mc.flat_room()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.MeshScene(v, t, c, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.MeshScene(torch.from_numpy(v), torch.from_numpy(t))
    assert have or _lib._lib is None


def test_emulated_random_scene(emu):
    mc.check_random_scene(emu)


def test_emulated_partial_tiles(emu):
    mc.check_partial_tiles(emu)


def test_emulated_closed_bumpy_room_is_watertight(emu):
    mc.check_closed_room(emu)


def test_emulated_near_plane_crossing(emu):
    mc.check_near_plane(emu)


def test_emulated_known_answers(emu):
    mc.check_known_answers(emu)


def test_emulated_capacity(emu):
    mc.check_capacity(emu)


def test_emulated_repeatable_and_order_independent(emu):
    mc.check_repeatable(emu)


def test_emulated_refusals(emu):
    mc.check_refusals(emu)


def test_emulated_sample_surface(emu):
    mc.check_sample_surface(emu)


def test_emulated_render_and_back_projection_round_trip(emu):
    mc.check_round_trip(emu)


def test_emulated_mapper_run_sensor(emu):
    mc.check_mapper(emu)
