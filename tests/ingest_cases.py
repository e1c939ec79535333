"""Shared checks of the on-device frame ingest (activesplat_amd/ingest.py; gs_frame_ingest): run on the host-emulated kernels by
tests/test_ingest.py and on the MI355X by tests/test_gpu_ingest.py.

Expected values
* `frames.to_mapping_tensors(image, depth, W, H, device)` on the SAME device -- the host path the ingest replaces: `torch.equal` for the colour,
  equality of the int32 views for the depth (so NaN payloads and the sign of zero count).  Nothing is compared with a tolerance.
* `restate_levels` / `restate_rows`: the two rules of include/gsplat_hip.h written out with Python floats (IEEE fp64, one rounding per operation) and
  integers.  tests/test_ingest.py pins the restatement to `frames.resize_linear` / `frames.resize_nearest` on the shapes of this file.

Shapes are written source h x w -> destination H x W; the library takes (W, H) pairs.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from activesplat_amd import _lib
from activesplat_amd import frames as FR
from activesplat_amd import ingest as IN
from activesplat_amd import rasterizer as R

GS_EINVAL = 1
#: (h, w, H, W): non-integer down | up (i0 = -1 and the upper clamp) | factor 2 | identity | one pixel | a row longer than a wavefront with a
#: partial last workgroup
SHAPES = ((7, 13, 3, 5), (3, 5, 7, 13), (6, 10, 3, 5), (5, 9, 5, 9), (1, 1, 4, 3), (9, 70, 4, 33))
DEPTH_ONLY = (2, 2, 98, 98)           # the fp64 index rule: (y * h) / H in integers picks other rows here

# ---- the rules, restated ----------------------------------------------------------------------------------------------------------------


def _axis(n_dst, n_src):
    r = float(n_src) / float(n_dst)
    out = []
    for d in range(n_dst):
        c = (d + 0.5) * r - 0.5
        i0 = math.floor(c)
        out.append((min(max(i0, 0), n_src - 1), min(max(i0 + 1, 0), n_src - 1), c - i0))
    return out


def restate_levels(image, W, H):
    """the colour rule of gs_frame_ingest, scalar fp64 -> uint8 [H, W, 3]"""
    h, w = image.shape[:2]
    ys, xs = _axis(H, h), _axis(W, w)
    out = np.zeros((H, W, 3), np.uint8)
    for y, (y0, y1, fy) in enumerate(ys):
        for x, (x0, x1, fx) in enumerate(xs):
            for ch in range(3):
                a, b = float(image[y0, x0, ch]), float(image[y0, x1, ch])
                c, d = float(image[y1, x0, ch]), float(image[y1, x1, ch])
                top = a * (1.0 - fx) + b * fx
                bot = c * (1.0 - fx) + d * fx
                o = top * (1.0 - fy) + bot * fy
                out[y, x, ch] = int(min(max(math.floor(o + 0.5), 0), 255))
    return out


def restate_rows(n_dst, n_src):
    """the depth rule's source index per destination index"""
    r = float(n_src) / float(n_dst)
    return np.array([min(int(math.floor(float(d) * r)), n_src - 1) for d in range(n_dst)], np.int64)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------


def raw_frame(h, w, seed):
    """random bytes with runs forced to 0 and to 255, a random positive depth with holes"""
    rng = np.random.RandomState(seed)
    image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    flat = image.reshape(-1)
    n = flat.size
    flat[n // 5: n // 5 + max(1, n // 7)] = 0
    flat[3 * n // 5: 3 * n // 5 + max(1, n // 7)] = 255
    depth = rng.uniform(0.2, 6.0, size=(h, w)).astype(np.float32)
    depth[rng.uniform(size=(h, w)) < 0.1] = 0.0
    return image, depth


def on_device(image, depth, device):
    return torch.from_numpy(image).to(device), torch.from_numpy(depth).to(device)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_is_host_path(got, image, depth, W, H, device, what):
    color, d = FR.to_mapping_tensors(image, depth, W, H, device)
    assert got[0].shape == (3, H, W) and got[1].shape == (1, H, W), what
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[0].is_contiguous() and got[1].is_contiguous(), what
    assert torch.equal(got[0], color), (what, "colour")
    assert same_bits(got[1], d), (what, "depth")


# ---- the checks -------------------------------------------------------------------------------------------------------------------------


def check_resize_shapes(device):
    table = IN.level_table(device)
    for i, (h, w, H, W) in enumerate(SHAPES + (DEPTH_ONLY,)):
        image, depth = raw_frame(h, w, seed=10 + i)
        got = IN.ingest_frame(*on_device(image, depth, device), [(W, H)])[0]
        what = f"{h}x{w} -> {H}x{W}"
        assert_is_host_path(got, image, depth, W, H, device, what)
        # ... and the restated rules
        rows, cols = restate_rows(H, h), restate_rows(W, w)
        want_d = torch.from_numpy(np.ascontiguousarray(depth[rows][:, cols])).to(device)
        assert same_bits(got[1][0], want_d), what
        if (h, w, H, W) != DEPTH_ONLY:
            levels = torch.from_numpy(restate_levels(image, W, H)).to(device).long()
            assert torch.equal(got[0], table[levels].permute(2, 0, 1)), what


def check_rounding(device):
    table = IN.level_table(device).cpu()
    depth = np.ones((2, 2), np.float32)
    for quad, level in (((1, 1, 0, 0), 1), ((1, 0, 0, 0), 0), ((255, 255, 255, 255), 255)):
        image = np.repeat(np.array(quad, np.uint8).reshape(2, 2, 1), 3, axis=2)
        color, _ = IN.ingest_frame(*on_device(image, depth, device), [(1, 1)])[0]
        assert torch.equal(color.cpu().reshape(3), table[level].expand(3)), (quad, color.cpu().reshape(3).tolist())
        assert int(restate_levels(image, 1, 1)[0, 0, 0]) == level
    assert float(table[0]) == 0.0 and float(table[255]) == 1.0


def special_depth():
    bits = np.array([[0x7fc12345, 0xffc00001, 0x7f812345, 0x7f800000],       # quiet NaNs with payloads, a signalling NaN, +inf
                     [0xff800000, 0x80000000, 0x00000001, 0x807fffff],       # -inf, -0.0, the smallest and the largest-magnitude negative denormal
                     [0xc0490fdb, 0x00000000, 0x3f800000, 0x7f7fffff]], np.uint32)   # -pi, 0, 1, the largest float
    return bits.view(np.float32)


def check_depth_bits(device):
    depth = special_depth()
    h, w = depth.shape
    image = raw_frame(h, w, seed=3)[0]
    img_t, dep_t = on_device(image, depth, device)
    assert same_bits(dep_t, torch.from_numpy(depth).to(device))
    for H, W in ((h, w), (2 * h, 2 * w), (5, 7), (2, 3)):
        got = IN.ingest_frame(img_t, dep_t, [(W, H)])[0]
        want = depth.view(np.int32)[restate_rows(H, h)][:, restate_rows(W, w)]
        assert torch.equal(got[1][0].view(torch.int32).cpu(), torch.from_numpy(np.ascontiguousarray(want))), (H, W)
        assert_is_host_path(got, image, depth, W, H, device, f"special depth -> {H}x{W}")
    seen = set(IN.ingest_frame(img_t, dep_t, [(w, h)])[0][1].view(torch.int32).cpu().numpy().reshape(-1).tolist())
    assert seen == set(depth.view(np.int32).reshape(-1).tolist())


def check_two_outputs(device):
    for (h, w), sizes in (((48, 64), [(32, 24), (16, 12)]), ((48, 64), [(64, 48), (32, 24)]), ((256, 256), [(256, 256), (128, 128)])):
        image, depth = raw_frame(h, w, seed=h + w)
        img_t, dep_t = on_device(image, depth, device)
        both = IN.ingest_frame(img_t, dep_t, sizes)
        assert len(both) == 2
        for k, (W, H) in enumerate(sizes):
            single = IN.ingest_frame(img_t, dep_t, [(W, H)])[0]
            assert torch.equal(both[k][0], single[0]) and same_bits(both[k][1], single[1]), (h, w, W, H)
            assert_is_host_path(both[k], image, depth, W, H, device, f"{h}x{w} -> {H}x{W} of two")


def check_repeatable(device):
    image, depth = raw_frame(37, 53, seed=5)
    depth[0, 0] = np.float32(np.nan)
    img_t, dep_t = on_device(image, depth, device)
    a = IN.ingest_frame(img_t, dep_t, [(29, 17), (64, 40)])
    b = IN.ingest_frame(img_t, dep_t, [(29, 17), (64, 40)])
    for (ca, da), (cb, db) in zip(a, b):
        assert same_bits(ca, cb) and same_bits(da, db)
        assert ca.data_ptr() != cb.data_ptr() and da.data_ptr() != db.data_ptr()          # freshly allocated


def check_refusals(device):
    lib = _lib.get()
    image, depth = raw_frame(4, 6, seed=1)
    img_t, dep_t = on_device(image, depth, device)
    table = IN.level_table(device)
    out_c = torch.zeros(2, 3 * 16, dtype=torch.float32, device=device)
    out_d = torch.zeros(2, 16, dtype=torch.float32, device=device)

    def call(w, h, n_out, sizes, image=img_t):
        flat = (C.c_int32 * 4)(*(list(sizes) + [1] * (4 - len(sizes))))
        return lib.gs_frame_ingest(w, h, R._ptr(image), R._ptr(dep_t), R._ptr(table), n_out, flat, R._ptr(out_c[0]), R._ptr(out_d[0]),
                                   R._ptr(out_c[1]), R._ptr(out_d[1]), _lib.stream_ptr(torch.device(device)))
    assert call(6, 4, 1, (4, 4)) == 0                                            # (the call itself is well formed)
    assert call(6, 4, 0, (4, 4)) == GS_EINVAL and b"n_out" in lib.gs_last_error()
    assert call(6, 4, 3, (4, 4)) == GS_EINVAL
    assert call(0, 4, 1, (4, 4)) == GS_EINVAL and b"out of range" in lib.gs_last_error()
    assert call(6, 4, 1, (4, 0)) == GS_EINVAL
    assert call(6, 4, 2, (4, 4, 0, 4)) == GS_EINVAL
    assert call(16385, 4, 1, (4, 4)) == GS_EINVAL
    assert call(6, 4, 1, (16385, 4)) == GS_EINVAL
    assert call(6, 4, 1, (4, 4), image=None) == GS_EINVAL and b"null" in lib.gs_last_error()
    assert float(out_c[1].abs().sum()) == 0.0 and float(out_d[1].abs().sum()) == 0.0   # nothing was launched on the refused calls
    with pytest.raises(TypeError, match="uint8"):
        IN.ingest_frame(img_t.float(), dep_t, [(4, 4)])
    with pytest.raises(TypeError, match="uint8"):
        IN.FrameIngest(6, 4, [(4, 4)], device).put(image.astype(np.float32), depth, [1, 0, 0, 0], [0, 0, 0])
    with pytest.raises(ValueError):
        IN.ingest_frame(img_t, dep_t, [])
    with pytest.raises(ValueError):
        IN.ingest_frame(img_t, dep_t, [(4, 4), (4, 4), (4, 4)])
    with pytest.raises(ValueError):
        IN.ingest_frame(img_t, dep_t, [(16385, 4)])
    if torch.device(device).type == "cuda":                  # the product path (the emulated build is the one thing that takes host tensors)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            IN.ingest_frame(torch.from_numpy(image), torch.from_numpy(depth), [(4, 4)])


def check_frame_ingest(device):
    h, w, sizes = 30, 44, [(22, 15), (11, 7)]
    fi = IN.FrameIngest(w, h, sizes, device)
    rng = np.random.RandomState(7)
    kept, originals = [], []
    for f in range(5):
        image, depth = raw_frame(h, w, seed=100 + f)
        quat, pos, gt = rng.normal(size=4).astype(np.float32), rng.normal(size=3).astype(np.float32), rng.normal(size=(4, 4)).astype(np.float32)
        originals.append((image.copy(), depth.copy()))
        outs, q_d, p_d, g_d = fi.put(image, depth, quat, pos, gt)
        # the caller reuses its arrays as soon as put returns
        image[:] = 255 - image
        depth[:] = -1.0
        assert torch.equal(q_d.cpu(), torch.from_numpy(quat)) and torch.equal(p_d.cpu(), torch.from_numpy(pos))
        assert g_d.shape == (4, 4) and torch.equal(g_d.cpu(), torch.from_numpy(gt))
        kept.append(outs)
    # every frame's tensors are that frame's, also after later puts through the same slot (keyframes keep them)
    for f, outs in enumerate(kept):
        for k, (W, H) in enumerate(sizes):
            assert_is_host_path(outs[k], originals[f][0], originals[f][1], W, H, device, f"frame {f} output {k}")
    # device tensors are taken as they are; a float64 depth is rounded to float32 as the host path's .float() rounds it
    image, depth = raw_frame(h, w, seed=200)
    outs, *_ = fi.put(*on_device(image, depth, device), [1, 0, 0, 0], [0, 0, 0])
    assert_is_host_path(outs[0], image, depth, *sizes[0], device, "device tensors in")
    d64 = depth.astype(np.float64) * (1.0 + 1e-9)
    outs, _, _, g_d = fi.put(image, d64, [1, 0, 0, 0], [0, 0, 0])
    assert g_d is None
    assert_is_host_path(outs[1], image, d64, *sizes[1], device, "float64 depth")


def run_raw_sequence(device, device_ingest, cfg=None):
    """the sequence of tests/test_mapper.py::test_raw_frames_with_densification_resolution"""
    from activesplat_amd import synthetic as syn
    from activesplat_amd.mapper import SplatMapper
    W, H, frames = 64, 48, 6
    gt = syn.shell_scene(3000, seed=2, W=W, H=H)
    gt["logit_opacities"] = gt["logit_opacities"] + 3.0
    seq = list(syn.orbit_sequence(gt, frames, W, H, device))
    mp = SplatMapper(syn.intrinsics(W, H), W, H, config=dict(step_num=frames, densify_downscale_factor=2, device_ingest=device_ingest, **(cfg or {})),
                     device=device)
    for fr in seq:
        image = (fr["color"].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        depth = fr["depth"][0].cpu().numpy()
        mp.run_raw(image, depth, np.linalg.inv(np.asarray(fr["w2c"], dtype=np.float64)), fr["id"], fr["quat"], fr["position"])
    return mp


def check_mapper(device, deterministic_mapping):
    a = run_raw_sequence(device, False)
    b = run_raw_sequence(device, True)
    assert a._ingest is None and b._ingest is not None and b._ingest.sizes == [(64, 48), (32, 24)]
    assert [k["id"] for k in a.keyframe_list] == [k["id"] for k in b.keyframe_list] and len(a.keyframe_list) >= 2
    for ka, kb in zip(a.keyframe_list, b.keyframe_list):
        assert torch.equal(ka["color"], kb["color"]) and same_bits(ka["depth"], kb["depth"]), ka["id"]
    assert len(a.gt_w2c_all_frames) == len(b.gt_w2c_all_frames) == 6
    for ga, gb in zip(a.gt_w2c_all_frames, b.gt_w2c_all_frames):
        assert same_bits(ga, gb)
    for mp in (a, b):
        assert (mp.densify_cam.image_width, mp.densify_cam.image_height) == (32, 24)
    if not deterministic_mapping:
        return
    assert a.stats["iters"] == b.stats["iters"] > 0 and a.params["means3D"].shape == b.params["means3D"].shape
    for k in a.params:
        assert torch.equal(a.params[k].detach(), b.params[k].detach()), k
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        sa, sb = a.optimizer.state[a.params[k]], b.optimizer.state[b.params[k]]
        assert int(sa["step"]) == int(sb["step"]) and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), k
