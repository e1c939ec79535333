"""bench.py's stdout contract (CPU): rank 0 prints ONE JSON line and nothing else, whatever the libraries underneath write to file descriptor 1
(RCCL announces its version there when a process group comes up); --dump-outputs writes the last timed step's outputs (CPU + one GPU run)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stdout_carries_the_result_line_only():
    code = ("import os, sys; sys.path.insert(0, %r); import bench; bench.claim_stdout(); "
            "os.write(1, b'library banner on fd 1\\n'); print('python print after the claim'); "
            "bench.emit({'metric': 'm', 'value': 1.5}); os.write(1, b'more noise\\n')") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == {"metric": "m", "value": 1.5}
    assert "library banner on fd 1" in r.stderr and "python print after the claim" in r.stderr and "more noise" in r.stderr


def test_emit_without_a_claim_still_prints_the_line():
    code = "import sys; sys.path.insert(0, %r); import bench; bench.emit({'k': [1, 2]})" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [json.loads(ln) for ln in r.stdout.splitlines()] == [{"k": [1, 2]}]


def test_configs3_roofline_block_arithmetic():
    """The N > 1 line's `roofline` block (bench.c4_roofline): per-GPU fraction of the HBM roofline from SURVEY 8(d)'s bytes per frame, the
    exchange against 7 xGMI links, for both exchanges SURVEY 8(e) names (G = 14 -> 112 MB, G = 59 -> 472 MB at 2 M Gaussians)."""
    sys.path.insert(0, ROOT)
    import bench
    N, D, px = 2_000_000, 4_500_000, 640 * 480
    assert bench.frame_bytes(N, D, px, sh=True) == N * 832 + D * 160 + px * 48        # C3 render, 2.40 GB
    for sh, G in ((False, 14), (True, 59)):
        S = N * G * 4
        r = bench.c4_roofline(N, D, px, sh, 8, 64, 6e-3, 1.0, S, single_fps=1000.0)
        B = bench.frame_bytes(N, D, px, sh=sh)
        assert r["alg_bytes_per_keyframe"] == B and r["keyframes_per_gpu_per_step"] == 8
        assert abs(r["frame_frac"] - 8 * B / 6e-3 / 8e12) < 1e-5 and r["frac"] == r["frame_frac"] and r["bound"] == "hbm"
        assert r["exchange_buffer_bytes"] == S == {14: 112_000_000, 59: 472_000_000}[G]
        assert r["exchange_wire_bytes_per_rank"] == int(2 * S * 7 / 8)
        assert abs(r["exchange_frac_xgmi"] - (2 * S * 7 / 8) / 1e-3 / (7 * 153e9)) < 1e-4
        assert abs(r["single_gpu_frame_frac"] - 1000.0 * B / 8e12) < 1e-5
    one = bench.c4_roofline(N, D, px, False, 1, 64, 32e-3, None, None)
    assert "exchange_frac_xgmi" not in one and one["keyframes_per_gpu_per_step"] == 64


def test_profiled_kernels_merges_the_rocprof_table_with_the_counter_summary():
    """bench.profiled_kernels: the committed rocprofv3 kernel table of a leg + its PMC summary -> per-kernel duration, counter bytes (FETCH doubled
    + WRITE), fraction of 8 TB/s.  Checked on the committed 2 M profile (any round's: the newest is taken)."""
    sys.path.insert(0, ROOT)
    import bench
    pr = bench.profiled_kernels("2m")
    assert pr and any(s.endswith("_2m_kernel_stats.csv") for s in pr["source"]) and any(s.endswith("_2m_pmc_summary.json") for s in pr["source"])
    by, us = bench.counters_for(pr, "blend_backward_kernel<false,1,false>")
    assert by and us and 100 < us < 400 and 2e8 < by < 6e8                      # ~180 us, ~367 MB at 2 M Gaussians / 4.84 M instances
    e = next(v for k, v in pr["kernels"].items() if k.startswith("blend_backward_kernel<"))
    assert abs(e["frac_hbm_pmc"] - by / (us * 1e-6) / 8e12) < 1e-3 and 0.3 < e["valu_busy"] < 1.0
    assert bench.profiled_kernels("no_such_leg") is None and bench.counters_for(None, "x") == (None, None)


def test_dump_outputs_writes_float32_arrays_at_a_fixed_sample_of_rows(tmp_path):
    """bench.dump_outputs (--dump-outputs DIR): the image-sized forward outputs whole, the per-Gaussian ones (radii, every input gradient) at
    the same seeded DUMP_ROWS rows on every run, float32, well under 64 MB."""
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    N, H, W = bench.DUMP_ROWS + 1000, 6, 8
    wl = types.SimpleNamespace(N=N, keys=["means3D", "shs"])
    outs = (torch.rand(3, H, W), torch.arange(N, dtype=torch.int32), torch.rand(1, H, W), torch.rand(1, H, W))
    grads = (torch.arange(N * 3, dtype=torch.float32).reshape(N, 3), torch.rand(N, 16, 3), torch.rand(N, 3))
    names = bench.dump_outputs(str(tmp_path / "a"), wl, outs, grads)
    assert names == sorted(["color", "radii", "depth", "opacity", "grad_means3D", "grad_shs", "grad_means2D"])
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert all(v.dtype == np.float32 for v in got.values())
    np.testing.assert_array_equal(got["color"], outs[0].numpy())
    rows = got["radii"].astype(np.int64)                                  # radii[i] == i: the sampled row indices themselves
    assert rows.shape == (bench.DUMP_ROWS,) and (np.diff(rows) > 0).all() and rows[-1] < N
    np.testing.assert_array_equal(got["grad_means3D"], grads[0].numpy()[rows])
    assert got["grad_shs"].shape == (bench.DUMP_ROWS, 16, 3)
    bench.dump_outputs(str(tmp_path / "b"), wl, outs, grads)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "radii.npy"), got["radii"])  # the same sample every run
    assert sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in names) < 64 << 20


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_ones_outputs(hip, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the line carries what a plain run measures and nothing of --full's legs,
    the last timed step's outputs land in DIR, and the same arguments give the same inputs (the forward outputs agree run to run)."""
    import numpy as np
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--gaussians", "100000",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        ln = r.stdout.splitlines()
        assert len(ln) == 1
        lines.append(json.loads(ln[0]))
        dumps.append(d)
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "frames/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f32" and abs(d["value"] * d["ms_per_step"] - 1000.0) < 10.0
        assert not {"roofline", "cpu_baseline", "side_legs", "configs3_single_gpu", "mapping_iteration"} & set(d)
    for name in ("color", "radii", "depth", "opacity", "grad_means3D", "grad_shs", "grad_opacities", "grad_scales", "grad_rotations", "grad_means2D"):
        a, b = (np.load(d / f"{name}.npy") for d in dumps)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), name
        if name in ("color", "radii", "depth", "opacity"):
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)
    assert np.abs(np.load(dumps[0] / "grad_means3D.npy")).max() > 0
