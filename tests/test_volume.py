"""CPU (host-emulated kernels): TSDF fusion and surface extraction (activesplat_amd/volume.py; gs_tsdf_integrate, gs_tsdf_count, gs_tsdf_emit).
The checks, their restatements and bars: tests/volume_cases.py.  The same checks run on the MI355X in tests/test_gpu_volume.py."""
import types

import numpy as np
import pytest
import torch

from tests import volume_cases as vc


def test_the_integration_reference_meets_its_conditions():
    vc.check_reference_conditions()


def test_the_interpolation_twin_against_float64():
    vc.check_twin_against_float64()


def test_the_restated_table_on_a_case_worked_by_hand():
    """the tetrahedron 0 -> x -> xy -> xyz with only the cell's origin inside: one triangle on the edges towards x, xy and xyz, its normal
    pointing away from the origin; the restated extraction of that single-cell volume has a vertex on each of the seven edges of the origin"""
    tets, cases = vc.tet_table()
    assert tets[0] == (0, 1, 3, 7) and len(tets) == 6 and len({t for t in tets}) == 6
    (tri,) = cases[0][1]
    assert sorted(tri) == [(0, 1), (0, 2), (0, 3)]
    mid = [0.5 * (vc.corner_xyz(tets[0][a]) + vc.corner_xyz(tets[0][b])) for a, b in tri]
    assert np.cross(mid[1] - mid[0], mid[2] - mid[0]) @ np.ones(3) > 0
    assert [len(c) for c in cases[0]] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    values = np.full((2, 2, 2), 0.5, np.float32)
    values[0, 0, 0] = -0.5
    r = vc.restate_extract(values, np.ones((2, 2, 2), np.float32), np.zeros((2, 2, 2, 3), np.float32), (0.0, 0.0, 0.0), 1.0, 1.0)
    assert r["vertices"].shape == (7, 3) and r["triangles"].shape == (6, 3)
    assert np.array_equal(r["vertices"][:3], np.float32([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]])) and np.array_equal(r["vertices"][6], np.float32([1.0, 1.0, 1.0]))
    # a fan of six triangles around the vertex on the cell's diagonal: every edge to it has one triangle on each side
    assert (r["triangles"] == 6).sum() == 6 and vc.manifold_report(r["triangles"], lambda a, b: 6 not in (a, b)) == (0, 12)


def test_volume_has_no_cpu_fallback():
    from activesplat_amd import _lib
    from activesplat_amd import volume as VOL
    _lib.unload_for_tests()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VOL.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), 0.3, device="cpu")


def test_ply_round_trip(tmp_path):
    """io.save_mesh_ply, then header and payload parsed back with numpy: vertices, colours and faces equal (also for an empty mesh)"""
    from activesplat_amd import io as IO
    rng = np.random.RandomState(2)
    v = rng.normal(size=(57, 3)).astype(np.float32)
    c = rng.randint(0, 256, (57, 3)).astype(np.uint8)
    t = rng.randint(0, 57, (101, 3)).astype(np.int32)
    mesh = types.SimpleNamespace(vertices=torch.from_numpy(v), triangles=torch.from_numpy(t), vertex_colors=torch.from_numpy(c))
    path = IO.save_mesh_ply(mesh, str(tmp_path / "out" / "mesh.ply"))
    gv, gc, gf = vc.read_ply(path)
    assert vc.same_bytes(gv, v) and np.array_equal(gc, c) and np.array_equal(gf, t)
    empty = types.SimpleNamespace(vertices=torch.zeros(0, 3), triangles=torch.zeros(0, 3, dtype=torch.int32), vertex_colors=torch.zeros(0, 3, dtype=torch.uint8))
    gv, gc, gf = vc.read_ply(IO.save_mesh_ply(empty, str(tmp_path / "empty.ply")))
    assert gv.shape == (0, 3) and gc.shape == (0, 3) and gf.shape == (0, 3)
    with pytest.raises(ValueError, match="vertex colours"):
        IO.save_mesh_ply(types.SimpleNamespace(vertices=mesh.vertices, triangles=mesh.triangles, vertex_colors=mesh.vertex_colors[:5]), str(tmp_path / "bad.ply"))


def test_emulated_integration(emu):
    vc.check_integration(emu)


def test_emulated_batch_weight_cap_and_repeatability(emu):
    vc.check_batch_cap_repeat(emu)


def test_emulated_tails(emu):
    vc.check_tails(emu)


def test_emulated_extraction(emu):
    vc.check_extraction(emu)


def test_emulated_all_sign_patterns(emu):
    vc.check_all_sign_patterns(emu)


def test_emulated_random_volumes_are_manifold(emu):
    vc.check_random_volumes_are_manifold(emu)


def test_emulated_sphere(emu):
    vc.check_sphere(emu)


def test_emulated_sensor_loop(emu):
    vc.check_sensor_loop(emu)


def test_emulated_mapper(emu):
    vc.check_mapper(emu)


def test_emulated_refusals(emu):
    vc.check_refusals(emu)
