"""CPU (host-emulated kernels): the completion / accuracy judge (activesplat_amd/judge.py; gs_depth_cloud, gs_cloud_nearest, gs_completion_row).
The checks, their references and tolerances: tests/completion_cases.py.  The same checks run on the MI355X in tests/test_gpu_completion.py."""
import numpy as np
import pytest
import torch

from tests import completion_cases as cc


def test_the_brute_force_restatement_is_scipys_kdtree():
    """scipy.spatial.KDTree(points).query(query): the reference's two calls (eval_actions.py:36-39), both directions, on the cases of this file"""
    from scipy.spatial import KDTree
    r = cc.room_reference()
    pairs = [(r["samples"], pts[ok]) for pts, ok in r["clouds"][:2]]
    pairs += [((r["samples"].astype(np.float64) + cc.FAR).astype(np.float32), (r["clouds"][0][0][r["clouds"][0][1]] + cc.FAR).astype(np.float32))]
    pairs += [cc.remainder_case(Q, M) for Q, M in ((63, 65), (1031, 1021), (257, 1))]
    worst = 0.0
    for a, b in pairs:
        for q, p in ((a, b), (b, a)):
            q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
            want, _ = KDTree(p).query(q)
            got = cc.brute_force(q, p)
            assert np.allclose(got, want, rtol=1e-12, atol=0.0), (len(q), len(p))
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
    print(f"brute force against scipy's KD-tree: max relative difference {worst:.2e}")


def test_the_restated_rows_follow_the_references_loop():
    """eval_actions.py:67-68,142-149 written out with scipy on the room frames: the restatement's rows"""
    from scipy.spatial import KDTree
    r = cc.room_reference()
    samples = r["samples"].astype(np.float64)
    lo, inf = np.ones(len(samples)), np.inf * np.ones(len(samples))
    for f, ((pts, ok), (_, _, path)) in enumerate(zip(r["clouds"], r["frames"])):
        cloud = pts[ok]
        d, _ = KDTree(cloud).query(samples)
        acc, _ = KDTree(samples).query(cloud)
        lo, inf = np.minimum(lo, d), np.minimum(inf, d)
        row = (np.mean(lo), np.mean(np.float64(lo < 0.05)), np.mean(inf), np.mean(np.float64(inf < 0.05)), path, np.mean(acc))
        assert np.allclose(r["rows"][f], row, rtol=1e-12, atol=0.0) and r["rows"][f][1] == row[1] and r["rows"][f][3] == row[3]


def test_the_seeds_keep_every_reference_distance_clear_of_the_threshold():
    r = cc.room_reference()
    atol = 2 * cc.cloud_atol(r["samples"], *(p for p, _ in r["clouds"]))
    for f, m in enumerate(r["minima"]):
        cc.assert_clear_of_threshold(m, atol + cc.RTOL * cc.THRESHOLD, f"room frame {f}")


def test_the_judge_has_no_cpu_fallback():
    import os
    from activesplat_amd import _lib
    from activesplat_amd import judge as J
    _lib.unload_for_tests()
    have = os.path.exists(_lib.LIB_PATH)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        J.nearest_distances(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        J.CompletionJudge(torch.zeros(4, 3))
    assert have or _lib._lib is None


def test_emulated_exact_arithmetic(emu):
    cc.check_exact(emu)


def test_emulated_remainders(emu):
    cc.check_remainders(emu)


def test_emulated_large_coordinates(emu):
    cc.check_large_coordinates(emu)


def test_emulated_depth_cloud(emu):
    cc.check_depth_cloud(emu)


def test_emulated_validity_frames(emu):
    cc.check_validity_frames(emu)


def test_emulated_running_state(emu):
    cc.check_running_state(emu)


def test_emulated_two_judges_are_bit_identical(emu):
    cc.check_repeatable(emu)


def test_emulated_map_distances(emu):
    cc.check_map_distances(emu)


def test_emulated_mapper_with_and_without_a_judge(emu):
    """(on ONE emulator thread the mapping iterations add their gradients in a fixed order: the maps can be compared bit for bit)"""
    import ctypes
    omp = ctypes.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        cc.check_mapper(emu, deterministic_mapping=True)
    finally:
        omp.omp_set_num_threads(before)


def test_emulated_refusals_and_write(emu):
    cc.check_refusals_and_write(emu)
