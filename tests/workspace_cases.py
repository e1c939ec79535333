"""Where do the kernels write?  One table of entries, run inside tests/guard.py's guarded_allocations by tests/test_workspace.py (the
host-emulated kernels, under every interior fill) and tests/test_gpu_workspace.py (the device, under the NaN fill).

An entry is (family, name, run(ctx), shapes, emulated).  `run` is built from the check_* functions and scene builders of the *_cases modules
and keeps their assertions as they are: a check that still passes at its own bars under every fill is the "the result does not depend on
what the workspace held" half; the bands around every allocation are the "nothing is written outside" half.  The inputs that must stay
unchanged and the layouts to region-check exist only once `run` has built them, so `run` hands them to the context instead of the table
naming them up front:

    with ctx.const(name=tensor, ...):   the `const` inputs of the calls inside: byte-identical afterwards (guard.unchanged)
    ctx.raster_regions(want_bwd)        the three raster state buffers of the last captured forward against GsGeomLayout / GsImageLayout /
                                        GsBinLayout: every byte outside the regions' used extents still holds the interior fill
    ctx.regions(buffer, fill, pairs)    any other workspace against its published layout

The used extent of a region is the header's description of it (include/gsplat_hip.h), with the launch constants read from csrc/gs_common.h.
A padding check needs a known fill.  Workspaces the hosts take from torch.empty have one under the "bytes" fills only, i.e. on the emulated
build; the direct ABI calls of this file (grid DBSCAN, the mesh render) allocate theirs with torch.full and are region-checked on the device
too.  GsEvalLayout publishes a size and no offsets: its workspace is found by size and guarded by its bands.

emulated = False would mark shapes that only the device runs; the emulator walks every entry of today's table in a few seconds, so none is."""
import collections
import ctypes as C
import os
import re

import numpy as np
import torch

from tests import guard as G
from tests import parity_cases as pc
from tests import regime_cases as rc
from tests import util

Entry = collections.namedtuple("Entry", "family name run shapes emulated")
ENTRIES = []

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constants():
    """The launch constants of csrc/gs_common.h / sort_radix.hip, read from the sources."""
    out = {}
    for rel in ("gs_common.h", "sort_radix.hip", "compact.hip"):
        text = open(os.path.join(_ROOT, "activesplat_amd", "csrc", rel)).read()
        m = re.search(r"#define GS_BIN_CHUNK (\d+)", text)
        if m:
            out["GS_BIN_CHUNK"] = int(m.group(1))
        # every `constexpr int kName = <integer expression of earlier constants>;` in source order (kCutLevels, kRadixChunk are expressions)
        for name, expr in re.findall(r"constexpr int (k\w+) = ([^;{}]+);", text):
            if re.fullmatch(r"[\w\s+\-*/()]+", expr):
                try:
                    out[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(out)))
                except (NameError, SyntaxError, TypeError):
                    pass
    return out


K = constants()
assert (K["kWave"], K["kBlock"]) == (64, 256) and K["kRadixChunk"] == 2048, K


def entry(family, name, shapes, emulated=True):
    def add(fn):
        ENTRIES.append(Entry(family, name, fn, shapes, emulated))
        return fn
    return add


def clear_workspace_caches():
    """No workspace may predate the guard (and none of the guard's may outlive it)."""
    from activesplat_amd import ingest, lookaround, mapping, rasterizer
    rasterizer._capacity.clear(); rasterizer._layouts.clear()
    for name in ("optimistic_hits", "optimistic_misses"):
        rasterizer.last_stats.pop(name, None)
    mapping._LOSS_SCRATCH.clear(); mapping._MEDIAN_SCRATCH.clear(); mapping._WINDOWS.clear(); mapping._UNIT_GRADS.clear()
    ingest._tables.clear()
    lookaround._COLS.clear()
    util.LAST.clear()


class Context:
    def __init__(self, device, guard, oracle32, oracle64):
        self.device, self.g, self.o32, self.o64 = device, guard, oracle32, oracle64
        self.emulated = torch.device(device).type == "cpu"
        self.region_buffers = 0
        self.const_inputs = 0

    def const(self, **tensors):
        self.const_inputs += sum(t is not None for t in tensors.values())
        return G.unchanged(tensors)

    def regions(self, buffer, fill, pairs, name):
        G.check_regions(buffer, fill, pairs, name=name)
        self.region_buffers += 1

    def raster_regions(self, want_backward):
        """util.LAST (rasterizer.capture) against the three published layouts.  want_backward: whether the captured forward ran with a
        backward to follow -- the header has `sh_jac` written then and `clamped` not, and the other way round without: the one that is not
        written counts as padding and must keep the fill."""
        d = util.LAST
        P, D, W, H, gl, il, bl = max(d["P"], 1), max(d["D"], 1), d["W"], d["H"], d["gl"], d["il"], d["bl"]
        tiles, hw, nb = ((W + 15) // 16) * ((H + 15) // 16), W * H, (P + K["kBlock"] - 1) // K["kBlock"]
        geom = [(gl.geom, P * 48), (gl.rect, P * 8), (gl.tiles_touched, P * 4), (gl.offsets, P * 4), (gl.block_sums, (nb + 1) * 4),
                (gl.tile_total, tiles * 4),
                (gl.tile_base, (P + K["kBinChunk"] - 1) // K["kBinChunk"] * tiles * 4 if tiles <= K["kMaxLdsTiles"] else 4),
                (gl.sh_jac, P * K["kShJacFloats"] * 4) if want_backward else (gl.clamped, P * 4), (gl.depth_bits, P * 4)]
        few = tiles <= K["kFewTiles"]
        split = ((K["kCutLevels"] * 5 + 4) * hw + 1) * 4
        # (the layout itself reserves exactly this extent, rounded up to a line: a level count read wrongly from the sources shows here)
        assert not few or (split + 255) // 256 * 256 == il.total_bytes - il.split_state, (split, il.total_bytes - il.split_state)
        image = [(il.ranges, tiles * 8), (il.final_T, hw * 4), (il.n_contrib, hw * 4),
                 (il.split_state, split if few else il.total_bytes - il.split_state)]
        if bl.path == 1:
            binning = [(bl.pairs, D * 8)] + ([(bl.pairs_alt, D * 8)] if bl.pairs_alt else [])
        else:
            binning = [(bl.keys_unsorted, D * 8), (bl.vals_unsorted, D * 4), (bl.keys_sorted, D * 8)]
        tail = bl.seg_T if bl.segments > 1 else bl.total_bytes
        if bl.path != 1:
            binning.append((bl.sort_temp, tail - bl.sort_temp))             # (the sort's own scratch: no extent is published for its parts)
        if bl.segments > 1:
            binning.append((bl.seg_T, tiles * bl.segments * K["kBlock"] * 4 + tiles * 16))
        for name, buf, pairs in (("geom (GsGeomLayout)", d["geom"], geom), ("image (GsImageLayout)", d["image"], image),
                                 ("binning (GsBinLayout)", d["binning"], binning)):
            al = self.g.owner(buf)
            assert al is not None, f"{name}: the state buffer was not allocated inside the guard"
            assert al.nbytes == buf.numel(), (name, al.nbytes, buf.numel())
            if isinstance(al.fill, int):
                self.regions(al, al.fill, pairs, name)
        return bl


# =====================================================================================================================================
# Drop-in rasteriser, forward + backward
# =====================================================================================================================================

def _resized(rs, size):
    return rs if size is None else rs._replace(image_width=size[0], image_height=size[1])


def _const_render(ctx, rs, rv, backward=True):
    """One more forward (+ backward) of the scene in which the tensors the kernels read are the ones watched."""
    from activesplat_amd import rasterizer as R
    H, W = int(rs.image_height), int(rs.image_width)
    inp = {k: v.detach().clone().requires_grad_(backward) for k, v in rv.items()}
    m2d = torch.zeros(inp["means3D"].shape[0], 3, device=ctx.device, requires_grad=backward)
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(0)).to(ctx.device)
    with ctx.const(bg=rs.bg, viewmatrix=rs.viewmatrix, projmatrix=rs.projmatrix, campos=rs.campos, dL=dL, **inp):
        color = R.GaussianRasterizer(raster_settings=rs)(means2D=m2d, **inp)[0]
        if backward:
            color.backward(dL)


def raster(ctx, case, P=None, size=None, path="auto", backward=True, expect_path=None):
    rs, rv = pc.build_case(case, ctx.device)
    rs = _resized(rs, size)
    if P is not None:
        assert P <= rv["means3D"].shape[0]
        rv = {k: v[:P].clone() for k, v in rv.items()}
    pc.set_sort_path(path)
    try:
        pc.check_forward(rs, rv, ctx.o32)
        bl = ctx.raster_regions(False)
        assert expect_path is None or bl.path == expect_path, bl.path
        if backward:
            pc.check_backward(rs, rv, ctx.o64, oracle32=ctx.o32)
            ctx.raster_regions(True)
        _const_render(ctx, rs, rv, backward)
    finally:
        pc.set_sort_path("auto")
    return bl


WAVE, BLOCK, CHUNK = K["kWave"], K["kBlock"], K["kBinChunk"]
FEW = K["kFewTiles"]                                           # 256 tiles = 16 x 16
assert FEW == 256 and K["kChainMinTiles"] < 40 * 20


@entry("dropin", "inputs", "colours 96x80 P2500 | SH3 16 rows | SH2 ragged P1003 | cov3D | all culled | one Gaussian")
def _(ctx):
    for case in ("basic", "sh3", "sh2_ragged", "cov3d_precomp", "all_culled", "one_gaussian"):
        raster(ctx, case, expect_path=1)


@entry("dropin", "P_wave_block", f"P {WAVE - 1}/{WAVE}/{WAVE + 1} at 17x17, {BLOCK - 1}/{BLOCK}/{BLOCK + 1} at 50x35, colours and SH3")
def _(ctx):
    for P in (WAVE - 1, WAVE, WAVE + 1):
        raster(ctx, "basic", P=P, size=(17, 17))
    for P in (BLOCK - 1, BLOCK, BLOCK + 1):
        raster(ctx, "sh3" if P == BLOCK + 1 else "basic", P=P, size=(50, 35))


@entry("dropin", "P_bin_chunk", f"P {CHUNK - 1}/{CHUNK}/{CHUNK + 1} at 50x35 (binning chunk)")
def _(ctx):
    for P in (CHUNK - 1, CHUNK, CHUNK + 1):
        raster(ctx, "basic", P=P, size=(50, 35))


@entry("dropin", "few_tiles_edge", "256x256 (kFewTiles) and 272x256 (one tile column more), P 700")
def _(ctx):
    raster(ctx, "basic", P=700, size=(256, 256))
    raster(ctx, "basic", P=700, size=(272, 256))


@entry("dropin", "chained_backward", "640x320 = 40x20 tiles > kChainMinTiles, P 700")
def _(ctx):
    raster(ctx, "basic", P=700, size=(640, 320))


def exact_list_scene(ctx, lengths, gx, gy, path, backward=False):
    rs, rv = rc.exact_lists(lengths, gx, gy, 0, device=ctx.device)
    pc.set_sort_path(path)
    try:
        _, ref = pc.check_forward(rs, rv, ctx.o32)
        rc.assert_lists(ref, lengths, gx, gy)
        bl = ctx.raster_regions(False)
        if backward:
            pc.check_backward(rs, rv, ctx.o64, oracle32=ctx.o32)
            ctx.raster_regions(True)
        _const_render(ctx, rs, rv, backward)
    finally:
        pc.set_sort_path("auto")
    return bl, ref


@entry("dropin", "radix_run_block", f"radix path forced, D = {K['kRadixChunk'] - 1} / {K['kRadixChunk'] + 1} (one run block -+ 1), 32x16")
def _(ctx):
    run = K["kRadixChunk"]
    for D in (run - 1, run + 1):
        bl, ref = exact_list_scene(ctx, {0: D - 300, 1: 300}, 2, 1, "radix", backward=True)
        assert bl.path == 2 and ref["D"] == D, (bl.path, ref["D"])
    raster(ctx, "ragged_image", path="radix", expect_path=2)


@entry("dropin", "lds_segments_and_pairs_alt", "LDS path: lists 8192+3 (segments, no pairs_alt) and 16385+100 (segments + pairs_alt), 32x16")
def _(ctx):
    bl, _ = exact_list_scene(ctx, {0: 8192, 1: 3}, 2, 1, "auto")
    assert bl.path == 1 and bl.segments > 1 and not bl.pairs_alt, (bl.path, bl.segments, bl.pairs_alt)
    bl, _ = exact_list_scene(ctx, {0: K["kSortCapMax"] + 1, 1: 100}, 2, 1, "auto")
    assert bl.path == 1 and bl.segments > 1 and bl.pairs_alt, (bl.path, bl.segments, bl.pairs_alt)


@entry("dropin", "lds_plain", "LDS path without pairs_alt and segments: lists 2049 + 32 (past one sort chunk; D = 2081, one pair past a 256-byte line), 32x16, backward")
def _(ctx):
    bl, ref = exact_list_scene(ctx, {0: K["kSortChunk"] + 1, 1: 32}, 2, 1, "auto", backward=True)
    assert bl.path == 1 and bl.segments == 1 and not bl.pairs_alt and ref["D"] * 8 % 256 == 8


# =====================================================================================================================================
# Optimistic launch that MISSES
# =====================================================================================================================================

@entry("optimistic_miss", "instance_count", "P 3000 96x80: a sparse frame, then a dense one under the same capacity key; tile-list growth at 48x48")
def _(ctx):
    pc.check_optimistic_launch(ctx.device, N=3000)
    clear_workspace_caches()
    pc.check_optimistic_tile_list_growth(ctx.device)
    clear_workspace_caches()
    # the same miss once more with the attempt's own buffers in view: the binning workspace and point_list sized from the GUESS
    from activesplat_amd import rasterizer as R
    N, W, H = 3000, 96, 80
    rs_far, rv = util.scene(N, W, H, seed=11, device=ctx.device, w2c=util.pose(0.0, (0.0, 0.0, -3.3)))
    rs_near, _ = util.scene(N, W, H, seed=11, device=ctx.device)
    util.run_product(rs_far, rv)                              # no guess yet: exact
    guess = R._capacity[(N, W, H, rv["means3D"].device.index)]
    seen = len(ctx.g.allocations)
    with ctx.const(bg=rs_near.bg, viewmatrix=rs_near.viewmatrix, projmatrix=rs_near.projmatrix, campos=rs_near.campos, **rv):
        util.run_product(rs_near, rv)
    assert R.last_stats.get("optimistic_misses", 0) == 1 and R.last_stats["num_rendered"] > guess[0]
    ctx.raster_regions(False)                                 # (the exact re-launch)
    attempt_regions(ctx, guess, W, H, seen)


def attempt_regions(ctx, guess, W, H, first):
    """The binning workspace of an optimistic attempt -- found by the size gs_bin_layout gives for the guess among the allocations from
    `first` on -- against that layout: `pairs` holds guess[0] entries and not one more."""
    from activesplat_amd import _lib
    bl = _lib.GsBinLayout(); _lib.check(_lib.get().gs_bin_layout(guess[0], guess[1], W, H, C.byref(bl)))
    assert bl.path == 1
    found = [al for al in ctx.g.allocations[first:] if al.nbytes == bl.total_bytes and al.dtype == torch.uint8 and al.factory == "empty"]
    assert found, "the attempt's binning workspace was not allocated inside the guard"
    plist = [al for al in ctx.g.allocations[first:] if al.shape == (max(guess[0], 1),) and al.dtype == torch.int32]
    assert plist, "the attempt's point_list was not allocated inside the guard"
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    pairs = [(bl.pairs, guess[0] * 8)] + ([(bl.pairs_alt, guess[0] * 8)] if bl.pairs_alt else [])
    if bl.segments > 1:
        pairs.append((bl.seg_T, tiles * bl.segments * K["kBlock"] * 4 + tiles * 16))
    for al in found:
        if isinstance(al.fill, int):
            ctx.regions(al, al.fill, pairs, f"binning workspace of the optimistic attempt (GsBinLayout for the guess {guess})")


@entry("optimistic_miss", "segment_flip", "P 8500 32x16: lists 4250+4250 then 8300+200 (the exact re-launch is segmented), then back (the guess would segment)")
def _(ctx):
    from activesplat_amd import rasterizer as R
    even, long_ = {0: 4250, 1: 4250}, {0: 8300, 1: 200}
    rs, rv_even = rc.exact_lists(even, 2, 1, 0, device=ctx.device)
    _, rv_long = rc.exact_lists(long_, 2, 1, 0, device=ctx.device)
    stats = lambda: (R.last_stats.get("optimistic_hits", 0), R.last_stats.get("optimistic_misses", 0))  # noqa: E731
    R.optimistic = False
    try:
        exact = [util.run_product(rs, rv) for rv in (rv_even, rv_long)]
        art = []
        for rv in (rv_even, rv_long):
            util.run_product(rs, rv); art.append(util.artefacts())
    finally:
        R.optimistic = True
    R._capacity.clear()
    got = util.run_product(rs, rv_even)                       # no guess yet: exact
    assert stats() == (0, 0) and int(util.LAST["bl"].segments) == 1
    ctx.raster_regions(False)
    guess = R._capacity[(8500, 32, 16, rv_even["means3D"].device.index)]
    seen = len(ctx.g.allocations)
    with ctx.const(**rv_long):
        got_long = util.run_product(rs, rv_long)              # the attempt runs under the guess (lists of at most 4579), misses, is re-launched segmented
    assert stats() == (0, 1) and R.last_stats["max_tile_instances"] == 8300 > guess[1] and int(util.LAST["bl"].segments) > 1
    ctx.raster_regions(False)
    attempt_regions(ctx, guess, 32, 16, seen)
    long_art = util.artefacts()
    got_even = util.run_product(rs, rv_even)                  # the guess (8300 + margin in 2 tiles) would segment: never optimistic, exact and unsegmented
    assert stats() == (0, 2) and int(util.LAST["bl"].segments) == 1
    ctx.raster_regions(False)
    for a, b in ((got, exact[0]), (got_even, exact[0])):
        for k in ("color", "depth", "opacity", "radii"):
            assert np.array_equal(a[k], b[k]), k
    for k in ("color", "depth", "opacity"):                   # (segmented compositing: the segments' order of summation, check_segmented_forward's bar)
        assert np.abs(got_long[k] - exact[1][k]).max() <= 2e-5 * max(1.0, float(np.abs(exact[1][k]).max())), k
    for k in rc.INTEGER_ARTEFACTS:
        if k != "n_contrib":
            assert np.array_equal(long_art[k], art[1][k]), k


# =====================================================================================================================================
# render_rgbd / render_rgbd_raw, pose gradients, tracking
# =====================================================================================================================================

def _one_omp_thread(fn):
    omp = C.CDLL("libgomp.so.1")
    before = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        fn()
    finally:
        omp.omp_set_num_threads(before)


@entry("rgbd", "fused_two_pass", "render_rgbd 50x37 P800 (ragged), 96x80 P2500 SH2")
def _(ctx):
    for case in ("ragged_image", "sh2"):
        rs, rv = pc.build_case(case, ctx.device)
        pc.check_fused_rgbd(rs, rv, ctx.o64, oracle32=ctx.o32)


@entry("rgbd", "raw_parameters", "render_rgbd_raw P500 64x48, anisotropic and isotropic, against the activation kernels")
def _(ctx):
    pc.check_raw_parameter_mode(ctx.device)


@entry("rgbd", "raw_parameters_sh", "render_rgbd_raw with 16-coefficient SH rows, P400 64x48")
def _(ctx):
    pc.check_raw_parameter_mode_sh(ctx.device)


@entry("rgbd", "raw_unrendered_rows", f"render_rgbd_raw accumulating into .grad, P{BLOCK + 1} 64x48, whole wavefronts unrendered, colours and SH")
def _(ctx):
    pc.check_unrendered_rows_are_written(ctx.device, n=BLOCK + 1)


@entry("rgbd", "adam_in_backward", "Adam inside the raw backward, P600 64x48, three steps; the direct (no-autograd) iteration P500")
def _(ctx):
    if ctx.emulated:
        _one_omp_thread(lambda: (pc.check_adam_inside_the_backward(ctx.device), pc.check_mapping_iteration_without_autograd(ctx.device)))
    else:
        pc.check_adam_inside_the_backward(ctx.device, exact=False)
        pc.check_mapping_iteration_without_autograd(ctx.device, exact=False)


@entry("rgbd", "pose_gradient", "pose-gradient backward, host pose: P600 64x48 aniso / iso / SH; BA bit-identity + pose-only")
def _(ctx):
    from tests import pose_cases as P
    for kw in (dict(), dict(iso=True), dict(sh=True)):
        P.check_pose_against_torch(ctx.device, 600, 64, 48, **kw)
    if ctx.emulated:
        _one_omp_thread(lambda: P.check_ba_bit_identity_and_pose_only(ctx.device))
    else:
        P.check_close_ba_and_pose_only(ctx.device)


@entry("rgbd", "pose_gradient_dev", "pose-gradient backward, device pose (_dev): P600 64x48 aniso / iso; tracking step against torch Adam")
def _(ctx):
    from tests import tracking_cases as T
    for kw in (dict(), dict(iso=True)):
        T.check_device_pose_matches_host_pose(ctx.device, exact_ok=ctx.emulated, **kw)
    T.check_step_matches_torch_adam(ctx.device)


@entry("rgbd", "track_frame", "track_frame, 8 iterations, P600 64x48")
def _(ctx):
    from tests import tracking_cases as T
    if ctx.emulated:
        _one_omp_thread(lambda: T.check_track_frame_deterministic(ctx.device))
    else:
        T.check_track_frame_deterministic(ctx.device, exact=False)
    T.check_first_iteration_parity(ctx.device)


def _camera_tensors(cam):
    return dict(bg=cam.bg, viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, campos=cam.campos)


def _watched(params, prefix=""):
    return {prefix + k: v.detach() for k, v in params.items()}


@entry("rgbd", "const_raw", f"render_rgbd / render_rgbd_raw forward + backward with every input watched: P{BLOCK + 1} 50x35, aniso / iso / SH; plain, with camera (BA), pose-only")
def _(ctx):
    from activesplat_amd import rasterizer as R
    from tests import pose_cases as P
    n, W, H = BLOCK + 1, 50, 35
    for kw in (dict(), dict(iso=True), dict(sh=True)):
        params, cam, t = P.make_scene(n, W, H, ctx.device, **kw)
        dLc, dLd = P.upstream(W, H, ctx.device)
        with ctx.const(dL_color=dLc, dL_depth=dLd, **_camera_tensors(cam), **_watched(params)):
            # the mapper's call: parameters in, host pose, no camera tensors
            m2d = torch.empty_like(params["means3D"], requires_grad=True)
            im, radius, depth, _sil, _dsq = R.render_rgbd_raw(cam, params["means3D"], m2d, params["logit_opacities"], params["log_scales"],
                                                              params["unnorm_rotations"], [0.998, 0.0, 0.06, 0.0, 0.05, -0.03, 0.1], **P._cols(params))
            ((im * dLc).sum() + (depth * dLd).sum()).backward()
            assert int((radius > 0).sum()) > 0 and all(bool(torch.isfinite(params[k].grad).all()) for k in P.G_KEYS if k in params)
            assert bool(torch.isfinite(m2d.grad).all())
            # bundle adjustment (parameter + pose gradients from one launch), then the pose-only backward of tracking
            pose_ba, gauss, _ = P.run(params, cam, t, "raw", (dLc, dLd))
            pose_only, none, _ = P.run(params, cam, t, "raw", (dLc, dLd), gaussians_grad=False)
            assert gauss and not none
            for k in P.CAM_KEYS:
                assert P.rel(pose_only[k][..., t], pose_ba[k][..., t]) < P.POSE_RTOL, k
            # the activation kernels + render_rgbd (the two-launch form of the same frame)
            P.run(params, cam, t, "act", (dLc, dLd))


@entry("rgbd", "const_dev_and_adam", f"device-pose forward + _dev pose backward, track_frame (3 iterations), Adam inside the backward: P{BLOCK + 1} 50x35, aniso / iso; everything but what the call updates is watched")
def _(ctx):
    from activesplat_amd import mapping as M, optim as O, rasterizer as R
    from tests import pose_cases as P, tracking_cases as T
    n, W, H = BLOCK + 1, 50, 35
    for iso in (False, True):
        params, curr, variables, t, _truth = T.track_scene(n, W, H, ctx.device, iso=iso)
        g = torch.Generator().manual_seed(4)
        dL_im, dL_depth = (torch.randn(3, H, W, generator=g) * 0.01).to(ctx.device), (torch.randn(1, H, W, generator=g) * 0.01).to(ctx.device)
        frame = dict(target_im=curr["im"], target_depth=curr["depth"], w2c=curr["w2c"], **_camera_tensors(curr["cam"]))
        with ctx.const(dL_im=dL_im, dL_depth=dL_depth, **frame, **_watched(params)):
            out = T._dev_pose_render(params, curr, t, dL_im, dL_depth)        # the pose is read from cam_unnorm_rots / cam_trans in place
            assert bool(torch.isfinite(out["pose"]).all()) and bool(torch.isfinite(out["m2d"]).all()) and int(out["seen"].sum()) > 0
        # a tracked frame: column t of the two camera tensors is what the step updates; the map, the targets and the other columns are not
        gaussians = {k: v for k, v in params.items() if not k.startswith("cam_")}
        others = {f"{k}[..., {c}]": params[k].detach()[..., c] for k in ("cam_unnorm_rots", "cam_trans") for c in range(params[k].shape[-1]) if c != t}
        with ctx.const(**frame, **_watched(gaussians), **others):
            res = M.track_frame(params, curr, variables, t, dict(tracking_iters=3, sil_thres=0.5), fused=True)
        assert res["iterations"] == 3 and np.isfinite(res["final_loss"])
        # Adam inside the backward: parameters and moments are the outputs, everything else is const
        prm = {k: torch.nn.Parameter(v.detach().clone()) for k, v in gaussians.items()}
        lrs = dict(means3D=1e-3, rgb_colors=2.5e-3, unnorm_rotations=1e-3, logit_opacities=0.05, log_scales=1e-3)
        opt = O.initialize_optimizer(prm, {k: lrs[k] for k in prm})
        cam = curr["cam"]
        dLc, dLd = P.upstream(W, H, ctx.device)
        before = {k: v.detach().clone() for k, v in prm.items()}
        with ctx.const(dL_color=dLc, dL_depth=dLd, **_camera_tensors(cam)):
            for _step in range(2):
                m2d = torch.empty_like(prm["means3D"], requires_grad=True)
                im, radius, depth, _sil, _dsq = R.render_rgbd_raw(cam, prm["means3D"], m2d, prm["logit_opacities"], prm["log_scales"], prm["unnorm_rotations"],
                                                                  [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], adam=opt, colors_precomp=prm["rgb_colors"])
                ((im * dLc).sum() + (depth * dLd).sum()).backward()
                assert all(v.grad is None for v in prm.values()) and bool(torch.isfinite(m2d.grad).all())
        assert all(int(opt.state[v]["step"]) == 2 for v in prm.values()) and not torch.equal(before["means3D"], prm["means3D"].detach())
        assert all(bool(torch.isfinite(v).all()) for v in prm.values())


# =====================================================================================================================================
# Top-down pass
# =====================================================================================================================================

@entry("topdown", "maps", "topdown_maps (truncated image state) P5000 120x150 iso, band edges P3000, optimistic hit / miss P3000")
def _(ctx):
    from activesplat_amd import _lib, topdown as TD
    from tests import topdown_cases as tc
    tc.check_equivalence(ctx.device, 5000, 120, 150, iso=True)
    tc.check_band_edges(ctx.device, ctx.o32)
    tc.check_optimistic_launch(ctx.device)
    # the truncated image state: "everything in front of final_T" is the tile ranges and the padding behind them
    params = tc.scene_params(777, 50, 35, ctx.device)
    cam = tc.camera(50, 35, ctx.device)
    il = _lib.GsImageLayout(); _lib.check(_lib.get().gs_image_layout(50, 35, C.byref(il)))
    seen = len(ctx.g.allocations)
    with ctx.const(**{k: v for k, v in params.items() if torch.is_tensor(v)}):
        TD.topdown_maps(params, cam, *tc.BAND)
    state = [al for al in ctx.g.allocations[seen:] if al.nbytes == il.final_T and al.dtype == torch.uint8 and al.factory == "empty"]
    assert len(state) >= 1, "the truncated image state was not found"
    if isinstance(state[0].fill, int):
        ctx.regions(state[0], state[0].fill, [(il.ranges, 4 * 3 * 8)], "topdown image state (GsImageLayout.ranges only)")


# =====================================================================================================================================
# Losses
# =====================================================================================================================================

@entry("losses", "mapping", "fused mapping loss 5x7, 17x33, 37x50 (odd sides, W H not a multiple of 256); no valid depth pixel")
def _(ctx):
    from tests import mapstep_cases as MC
    for H, W in ((5, 7), (17, 33), (37, 50)):
        MC.check_mapping_loss(ctx.device, H, W, "noise")
    MC.check_mapping_loss(ctx.device, 37, 50, "smooth", all_invalid=True)
    # targets and renders are const, with and without the outlier rule
    from activesplat_amd import mapping as M
    from tests import outlier_cases as OC
    names = ("im", "depth", "depth_sq", "gt_im", "gt_depth")
    ins = dict(zip(names, (t.to(ctx.device) for t in OC.mapping_loss_inputs(35, 51))))
    for option in (False, True):
        a, d = ins["im"].clone().requires_grad_(True), ins["depth"].clone().requires_grad_(True)
        with ctx.const(**ins):
            loss, _ = M.fused_mapping_loss(a, d, ins["depth_sq"], ins["gt_im"], ins["gt_depth"], dict(im=0.5, depth=1.0), ignore_outlier_depth_loss=option)
            loss.backward()
        assert torch.equal(a.detach(), ins["im"]) and torch.equal(d.detach(), ins["depth"]) and bool(torch.isfinite(a.grad).all())


@entry("losses", "mapping_outlier", "mapping loss with outlier rejection 17x33, 37x50, boundary 4x8")
def _(ctx):
    from tests import outlier_cases as OC
    for H, W in ((17, 33), (37, 50)):
        OC.check_mapping_loss(ctx.device, H, W, im_exact=ctx.emulated)
    OC.check_mapping_loss(ctx.device, 37, 50, "boundary", im_exact=ctx.emulated)


@entry("losses", "median", "depth-error median, plain and grid: 1x1, 7x9, 33x47, 2 chunks -+ 1")
def _(ctx):
    from tests import outlier_cases as OC
    for H, W in ((1, 1), (7, 9), (33, 47)):
        for variant in ("random", "ties", "nan_render"):
            OC.check_median(ctx.device, H, W, variant)
    OC.check_median_at_chunk_edges(ctx.device, "random")


@entry("losses", "tracking", "tracking loss 45x67 and its outlier form 45x67, 33x47, 91x91 (33 scratch rows: one row past a 256-byte line)")
def _(ctx):
    from tests import outlier_cases as OC, tracking_cases as T
    T.check_tracking_loss(ctx.device)
    plain = T.loss_inputs(51, 35, ctx.device)
    with ctx.const(**dict(zip(("im", "gt", "depth", "depth_sq", "gt_depth", "sil"), plain))):
        for use_sil in (True, False):
            T.kernel_tracking_loss(*plain, use_sil, 0.99, dict(im=0.5, depth=1.0))
    OC.check_tracking_loss(ctx.device, 45, 67)
    OC.check_tracking_loss(ctx.device, 33, 47)
    # const inputs of the outlier form
    OC.check_tracking_loss(ctx.device, 91, 91)
    ins = [x.to(ctx.device) for x in OC.tracking_loss_inputs(91, 91)]
    with ctx.const(**dict(zip(("im", "gt", "depth", "depth_sq", "gt_depth", "sil"), ins))):
        OC.kernel_tracking_loss(*ins, True, 0.99, dict(im=0.5, depth=1.0))


# =====================================================================================================================================
# Optimiser and surgery
# =====================================================================================================================================

@entry("optim", "adam", "gs_adam_step n 0/1/3/1023/1024/1025; _multi: ragged sizes, more tensors than one launch takes")
def _(ctx):
    from activesplat_amd import _lib
    from tests import optimstep_cases as oc
    for n in (0, 1, 3, 1023, 1024, 1025):
        oc.check_adam_size(ctx.device, n)
    oc.check_adam_multi(ctx.device, False)
    # the gradient handed to Adam is const
    lib = _lib.get()
    n = BLOCK + 1
    p, g, m, v = (torch.rand(n, generator=torch.Generator().manual_seed(i)).to(ctx.device) for i in range(4))
    with ctx.const(grad=g):
        _lib.check(lib.gs_adam_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 0.9, 0.999, 1e-15, 1, oc._stream(ctx.device)))
    # ... and so are the gradients of a multi-tensor launch: ragged sizes, one more tensor than a launch takes, an empty one among them
    sizes = [1, 3, BLOCK - 1, BLOCK, BLOCK + 1, 0, 1023, 1024, 1025][:K["kAdamMaxTensors"] + 1]
    gen = torch.Generator().manual_seed(9)
    ts = [[torch.rand(s, generator=gen).to(ctx.device) for _ in range(4)] for s in sizes]           # p, g, m, v
    before = [t[0].clone() for t in ts]
    arr = (_lib.GsAdamTensor * len(sizes))(*[_lib.GsAdamTensor(s, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1e-3, 0.9, 0.999, 1e-15, 1, 0)
                                             for s, (p, g, m, v) in zip(sizes, ts)])
    with ctx.const(**{f"grad{i}": t[1] for i, t in enumerate(ts)}):
        _lib.check(lib.gs_adam_step_multi(len(sizes), arr, oc._stream(ctx.device)))
    assert all(s == 0 or not torch.equal(b, t[0]) for s, b, t in zip(sizes, before, ts))


@entry("optim", "compact", "compact_index / compact_index3 n 1/255/256/257/1023/1024/1025, masks all / none / first / last / random")
def _(ctx):
    from activesplat_amd import _lib, optim as O
    from tests import mapstep_cases as MC
    lib = _lib.get()
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, K["kCompactBlock"] - 1, K["kCompactBlock"], K["kCompactBlock"] + 1):
        MC.check_build_index(ctx.device, n)
        MC.check_compact_index3(ctx.device, n)
        for kind in ("none", "all"):
            a = MC.compact_mask(n, kind, ctx.device).to(torch.uint8).contiguous()
            idx = torch.full((3 * n,), -1, dtype=torch.int32, device=ctx.device)
            cnt = torch.zeros(3, dtype=torch.int32, device=ctx.device)
            scratch = torch.empty(int(lib.gs_compact3_scratch_bytes(n)), dtype=torch.uint8, device=ctx.device)
            with ctx.const(mask=a):
                _lib.check(lib.gs_compact_index3(n, a.data_ptr(), a.data_ptr(), a.data_ptr(), 1, idx.data_ptr(), cnt.data_ptr(), scratch.data_ptr(), O._stream(idx)))
            k = n if kind == "all" else 0
            assert cnt.tolist() == [k] * 3 and bool((idx[3 * k:] == -1).all())
            assert k == 0 or torch.equal(idx[:3 * k], torch.arange(n, dtype=torch.int32, device=ctx.device).repeat(3))


@entry("optim", "gather", "gather_rows vec4 (width 4, 48) and scalar (width 1, 3, misaligned 4) routes, n 1/255/256/257; zero tail")
def _(ctx):
    from activesplat_amd import optim as O
    g = torch.Generator().manual_seed(3)
    for width, misaligned in ((4, False), (48, False), (1, False), (3, False), (4, True)):
        for n_out in (1, BLOCK - 1, BLOCK, BLOCK + 1):
            n_src = 37
            buf = torch.randn(3 + n_src * width, generator=g).to(ctx.device)
            src = buf[3:].view(n_src, width) if misaligned else buf[: n_src * width].view(n_src, width)
            index = torch.randint(0, n_src, (n_out,), generator=g).to(torch.int32).to(ctx.device)
            want = src[index.long()]
            with ctx.const(src=buf, src_index=index):
                got = O.gather_rows(src, index)
                keep = max(n_out - 5, 0)
                tail = O.gather_rows_zero_tail(src, index, keep)
            assert torch.equal(got, want), (width, misaligned, n_out)
            want[keep:] = 0.0
            assert torch.equal(tail, want), (width, misaligned, n_out)


@entry("optim", "surgery", "prune + densify + remove_points through optim.py, N 4097, anisotropic and isotropic")
def _(ctx):
    from tests import mapstep_cases as MC
    for iso in (False, True):
        MC.check_remove_points(ctx.device, iso, N=4 * K["kCompactBlock"] + 1)
        MC.check_prune(ctx.device, iso, N=4 * K["kCompactBlock"] + 1)
        MC.check_densify(ctx.device, iso, N=4 * K["kCompactBlock"] + 1)


# =====================================================================================================================================
# Growth and keyframes, row exchange, statistics
# =====================================================================================================================================

@entry("growth", "grow", "gs_grow_gaussians 1x1, 7x9, 33x47, 32x64; no pixel growing (sil 1, depth exact) and all pixels growing (sil 0)")
def _(ctx):
    from activesplat_amd import mapping as M
    from tests import mapstep_cases as MC
    for H, W in ((1, 1), (7, 9), (33, 47), (32, 64)):
        MC.check_grow(ctx.device, H, W, "random")
    MC.check_grow(ctx.device, 33, 47, "all_gt_zero")
    H, W = 33, 47
    Kc, c2w = MC.grow_camera(H, W)
    g = torch.Generator().manual_seed(1)
    gt, color = torch.rand(H, W, generator=g) + 0.5, torch.rand(3, H, W, generator=g)
    for sil_value, n_want in ((1.0, 0), (0.0, H * W)):
        ins = dict(render_depth=gt.clone().to(ctx.device), sil=torch.full((H, W), sil_value).to(ctx.device), gt=gt.to(ctx.device), color=color.to(ctx.device))
        with ctx.const(**ins):
            rows, n_cand = M.grow_rows(ins["render_depth"], ins["sil"], ins["gt"], ins["color"], Kc, c2w, MC.SIL_THRES, "anisotropic")
        assert n_cand == n_want and rows["means3D"].shape[0] == n_want, (sil_value, n_cand, rows["means3D"].shape)
        _, want = MC.grow_reference(gt.clone(), torch.full((H, W), sil_value), gt, color, Kc, c2w, False)
        assert torch.equal(rows["rgb_colors"].cpu(), want["rgb_colors"])


@entry("growth", "keyframe_overlap", "gs_keyframe_overlap n_pts 0/1/255/256/257 x 1/3 keyframes")
def _(ctx):
    from tests import optimstep_cases as oc
    for n_pts in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1):
        for n_kf in (1, 3):
            oc.check_keyframe_overlap(ctx.device, n_pts, n_kf)


@entry("rows", "pack_adam_unpack", "gs_pack_columns / gs_adam_rows / gs_unpack_columns: widths (3,3,4,1,3), (17,), (1,)x8; n 0/1/255/256/257; ragged windows")
def _(ctx):
    from tests import optimstep_cases as oc
    for widths in ((3, 3, 4, 1, 3), (17,), (1,) * 8):
        for n in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1):
            oc.check_rows_pack_unpack(ctx.device, widths, n)
            if n:
                oc.check_rows_adam(ctx.device, widths, n)
    oc.check_rows_pack_unpack(ctx.device, (3, 48, 4, 1, 3), WAVE + 1, offset1=True)
    oc.check_rows_adam(ctx.device, (3, 48, 4, 1, 3), WAVE + 1, offset1=True)
    # the const sides of the three calls: the gradients gs_pack_columns reads, the gradient shard gs_adam_rows reads, the rows gs_unpack_columns reads
    L, lib = oc._lib()
    widths, n = (3, 3, 4, 1, 3), BLOCK + 1
    G_, gen = sum(widths), torch.Generator().manual_seed(5)
    mk = lambda: [oc._alloc(n * w, ctx.device, False, gen=gen).view(n, w) for w in widths]  # noqa: E731
    grads, p, m, v = mk(), mk(), mk(), [t.abs() for t in mk()]
    flat = oc._alloc(n * G_, ctx.device, False, fill=float("nan")).view(n, G_)
    with ctx.const(**{f"grad{k}": g for k, g in enumerate(grads)}):
        L.check(lib.gs_pack_columns(len(widths), oc._row_array(L, widths, g=grads), n, n, flat.data_ptr(), oc._stream(ctx.device)))
    assert torch.equal(flat, torch.cat(grads, dim=1))
    out = oc._alloc(n * G_, ctx.device, False, fill=float("nan")).view(n, G_)
    hyper = [(1e-3, 1e-15, 1)] * len(widths)
    with ctx.const(shard=flat):
        L.check(lib.gs_adam_rows(len(widths), oc._row_array(L, widths, p=p, m=m, v=v, hyper=hyper), 0, n, n, flat.data_ptr(), out.data_ptr(), oc._stream(ctx.device)))
    assert torch.equal(out, torch.cat(p, dim=1)) and bool(torch.isfinite(out).all())
    back = [oc._alloc(n * w, ctx.device, False, fill=-5.5).view(n, w) for w in widths]
    with ctx.const(rows=out):
        L.check(lib.gs_unpack_columns(len(widths), oc._row_array(L, widths, p=back), n, out.data_ptr(), oc._stream(ctx.device)))
    assert all(torch.equal(a, b) for a, b in zip(back, p))


@entry("stats", "visibility_and_grad2d", "gs_visibility_stats / gs_accumulate_grad2d P 0/1/255/256/257")
def _(ctx):
    from tests import optimstep_cases as oc
    for P in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1):
        oc.check_visibility_stats(ctx.device, P)
        oc.check_accumulate_grad2d(ctx.device, P)
    oc.check_fused_visibility_nan_rule(ctx.device)


# =====================================================================================================================================
# Planner
# =====================================================================================================================================

def dbscan_direct(ctx, values, thr, eps, ms, max_clusters, fill=0xAB):
    """gs_grid_dbscan on values [B, H, W] (rows and images may be strided) with a workspace of a known fill -> the fields of GridClusters"""
    from activesplat_amd import _lib
    from activesplat_amd import rasterizer as R
    lib = _lib.get()
    B, H, W = (int(s) for s in values.shape)
    M = int(max_clusters)
    lay = _lib.GsDbscanLayout(); _lib.check(lib.gs_grid_dbscan_layout(B, H, W, M, C.byref(lay)))
    dev = values.device
    words, pixels = B * H * ((W + 63) // 64), B * H * W
    used = [(lay.mask_bits, words * 8), (lay.core_bits, words * 8), (lay.root_bits, words * 8), (lay.word_prefix, words * 4),
            (lay.parent, pixels * 4), (lay.root, pixels * 4), (lay.row_range, B * M * 8)]
    G.check_extents(lay.total_bytes, used, "grid DBSCAN workspace (GsDbscanLayout)")     # (before the launch: a short layout makes the kernel's arrays alias)
    ws = torch.full((int(lay.total_bytes),), fill, dtype=torch.uint8, device=dev)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(B, dtype=torch.int32, device=dev)
    table = torch.empty(B, M, 4, dtype=torch.int32, device=dev)
    sum_value = torch.empty(B, M, dtype=torch.float32, device=dev)
    total = torch.empty(B, dtype=torch.float32, device=dev)
    whole = values._base if values._base is not None else values
    with ctx.const(values=whole):
        _lib.check(lib.gs_grid_dbscan(B, H, W, R._ptr(values), int(values.stride(1)), int(values.stride(0)), float(thr), 0, int(eps), int(ms), M,
                                      R._ptr(ws), R._ptr(labels), R._ptr(n_clusters), R._ptr(table), R._ptr(sum_value), R._ptr(total), _lib.stream_ptr(dev)))
    assert len(ctx.g.find(lay.total_bytes, torch.uint8)) >= 1
    ctx.regions(ws, fill, used, "grid DBSCAN workspace (GsDbscanLayout)")
    out = dict(labels=labels, n_clusters=n_clusters, count=table[..., 0], sum_row=table[..., 1], sum_col=table[..., 2], root=table[..., 3],
               sum_value=sum_value, total=total)
    return {k: v.cpu().numpy() for k, v in out.items()}


@entry("planner", "dbscan", "grid DBSCAN 33x70 (W not a multiple of 64): B 1 and 3, row_stride 70 and 83, max_clusters 1, 5 (exceeded) and 256; 5x13; 24x40 eps 1")
def _(ctx):
    from tests import cluster_cases as cc
    refs = [cc.reference("ragged", s) for s in cc.SEEDS]
    _, H, W, thr, eps, ms, _comp = next(c for c in cc.RANDOM_CASES if c[0] == "ragged")
    batch = np.stack([v for v, _ in refs])
    for B in (1, 3):
        for stride in (W, W + 13):
            padded = torch.full((B, H + 1, stride), 0.25, dtype=torch.float32)
            padded[:, :H, :W] = torch.from_numpy(batch[:B])
            padded = padded.to(ctx.device)
            for M in (1, 256):
                got = dbscan_direct(ctx, padded[:, :H, :W], thr, eps, ms, M)
                for b in range(B):
                    cc.compare(got, refs[b][1], b, max_clusters=M, what=f"ragged B {B} stride {stride} max_clusters {M} image {b}")
    v = cc.smooth_field(5, 13, 0.5, 3, sigma=1.5, jitter=0.2)      # 65 pixels: `parent` and `root` end one word past a 256-byte line
    cc.compare(dbscan_direct(ctx, torch.from_numpy(np.array(v, np.float32))[None].to(ctx.device), 0.5, 2, 3, 4), cc.restate(v, 0.5, 2, 3), 0, max_clusters=4, what="5 x 13")
    values, ref = cc.reference("eps1", 0)
    assert ref["n_clusters"] > 5
    got = dbscan_direct(ctx, torch.from_numpy(np.array(values, np.float32))[None].to(ctx.device), 0.5, 1, 1, 5)
    cc.compare(got, ref, 0, max_clusters=5, what="eps1, max_clusters 5 exceeded")
    cc.check_small_sizes(ctx.device)                          # through visibility.grid_dbscan (its workspace comes from torch.empty)
    cc.check_truncated(ctx.device)


@entry("planner", "hulls", "cluster hulls 24x40: the small cases of the fixture (max_points 1024, and 8 with contours of 13 and 18); max_points 4 with a 4-point contour (fits exactly) and with contours of 13 and 18 (larger than max_points)")
def _(ctx):
    from tests import hull_cases as hc
    for name in hc.small_cases():
        hc.check_small(ctx.device, name)
    # the smallest legal max_points: the shortest per-cluster point buffer.  No scipy fixture exists for these two: the volumes are compared
    # with the restatement's incremental hull at the fixture's own bars
    d = hc.poly_depth(24, 40)
    rect = np.full((24, 40), -2, np.int32)
    rect[1:4, 2:6] = 0
    for what, k in (("a contour of exactly 4 points", hc._case(rect, d, rows=[1], kw=1, max_points=4)),
                    ("contours longer than max_points", hc._case(hc.blocks(4, 16), d, max_points=4))):
        ref = hc.restate(k["labels"][0], k["depth"][0], k["n"][0], k["sum_value"][0], k["M"], k["rows"], k["kw"], max_points=4)
        got = {f: v[0] for f, v in hc.run_case(ctx.device, k).items()}
        m = len(ref["contours"])
        assert got["contour_xy"].shape[1] == 4, got["contour_xy"].shape
        assert np.array_equal(got["n_points"], ref["n_points"][:k["M"]]) and int(got["status"]) == ref["status"], (what, got["n_points"], int(got["status"]))
        for c in range(m):
            stored = ref["contours"][c]
            assert len(stored) <= 4 and [tuple(p) for p in got["contour_xy"][c, :len(stored)].tolist()] == stored, (what, c)
            assert (got["contour_xy"][c, len(stored):] == 0).all(), (what, c)
        assert (got["contour_xy"][m:] == 0).all() and (got["volume"][m:] == 0).all() and (got["n_points"][m:] == 0).all(), what
        assert (np.abs(got["volume"] - ref["volume"]) <= hc.VOL_ATOL + hc.VOL_RTOL * np.abs(ref["volume"])).all(), (what, got["volume"], ref["volume"])
        assert abs(got["sum_volume"] - ref["sum_volume"]) <= hc.VOL_ATOL + hc.VOL_RTOL * abs(ref["sum_volume"]), what
        assert abs(got["sum_invisibility"] - ref["sum_invisibility"]) <= hc.SUM_RTOL * abs(ref["sum_invisibility"]), what
        if what.startswith("a contour of exactly"):
            assert ref["contours"][0] == hc.RECTANGLE_CONTOUR and ref["status"] == 0 and ref["volume"][0] != 0
        else:
            assert ref["status"] == hc.OVERFLOW and (ref["n_points"][:2] > 4).all() and (ref["volume"] == 0).all() and (got["volume"] == 0).all()


@entry("planner", "high_loss", "gs_high_loss_grid: pixel rule, resize 7x5 -> 11x9, 37x53 -> 90x90, 150x120 -> 90x90; decisions")
def _(ctx):
    from tests import highloss_cases as hl
    hl.check_pixel_rule(ctx.device)
    for name in ("up", "up_t", "mixed", "s150x120"):
        hl.check_resize(ctx.device, name)
    for name in list(hl.decision_masks())[:3]:
        hl.check_decision(ctx.device, name)


@entry("planner", "look_around", "one batched look-around of 2 nodes (three 120x150 views each), P1500")
def _(ctx):
    from tests import cluster_cases as cc
    cc.check_look_around_nodes(ctx.device, 2)


# =====================================================================================================================================
# Sensing and judging
# =====================================================================================================================================

@entry("sensing", "ingest", "gs_frame_ingest: outputs smaller than, equal to and larger than the source, one and two outputs; FrameIngest slots")
def _(ctx):
    from tests import ingest_cases as ic
    ic.check_resize_shapes(ctx.device)
    ic.check_two_outputs(ctx.device)
    ic.check_depth_bits(ctx.device)
    ic.check_frame_ingest(ctx.device)


@entry("sensing", "clouds", "gs_depth_cloud 23x17; gs_cloud_nearest n_query x n_points over 0/1/63/255/257/1031 x 0/1/65/255/1021; gs_completion_row")
def _(ctx):
    from activesplat_amd import judge as J
    from tests import completion_cases as cc
    cc.check_depth_cloud(ctx.device)
    cc.check_exact(ctx.device)
    cc.check_remainders(ctx.device)
    cc.check_validity_frames(ctx.device)
    for Q, M in ((0, 0), (0, 5), (5, 0), (1, 1), (BLOCK + 1, BLOCK - 1)):
        q, p = cc.remainder_case(max(Q, 1), max(M, 1))
        q, p = cc.t(q[:Q], ctx.device), cc.t(p[:M], ctx.device)
        with ctx.const(query=q, points=p):
            got = J.nearest_distances(q, p).cpu().numpy()
        assert got.shape == (Q,)
        if Q and M:
            cc.compare_distances(got, cc.brute_force(q.cpu().numpy(), p.cpu().numpy()), f"nearest {Q} x {M}")
        else:
            assert np.isinf(got).all()


def mesh_call(ctx, scene, k4, w2c, W, H, capacity):
    from tests import mesh_cases as mc
    with ctx.const(vertices=scene.vertices, triangles=scene.triangles, vertex_colors=scene.vertex_colors):
        rcode, outs, (need, longest), _intact, lay = mc._abi_call(ctx.device, scene, k4, w2c, W, H, mc.NEAR, capacity, guard=0)
    assert rcode == 0
    T, tiles = scene.num_triangles, ((W + 15) // 16) * ((H + 15) // 16)
    ws = ctx.g.find(lay.total_bytes, torch.uint8)
    assert len(ws) >= 1
    fits = need <= capacity
    ctx.regions(ws[-1], 0xAB, [(lay.total, 8), (lay.records, T * 64), (lay.rects, T * 8), (lay.tile_count, (tiles + 1) * 4),
                               (lay.tile_offset, (tiles + 1) * 4), (lay.list, need * 4 if fits else 0)], f"mesh scratch (GsMeshLayout), capacity {capacity}, D {need}")
    return outs, need, longest


@entry("sensing", "mesh", "gs_mesh_render 37x21 (partial tiles), 48x40: 0 triangles, capacity == D, capacity == D - 1, capacity 1; render_mesh")
def _(ctx):
    from activesplat_amd import sensor as S
    from tests import mesh_cases as mc
    mesh = mc.random_scene()
    scene = S.MeshScene(*mesh, device=ctx.device)
    for W, H in ((37, 21), (48, 40)):
        k4, w2c = mc.k_for(W, H, 24.0), mc.GENERIC_POSES[0]
        ref, tol = mc.reference(("partial", W, H) if W == 37 else ("random", 0), mesh, k4, w2c, W, H, mc.NEAR)
        _, need, _ = mesh_call(ctx, scene, k4, w2c, W, H, 1)
        got, need2, _ = mesh_call(ctx, scene, k4, w2c, W, H, need)
        assert need2 == need
        mc.compare(f"capacity == D, {W} x {H}", got, ref, tol, 0.01)
        (color, depth, tri_id), need3, _ = mesh_call(ctx, scene, k4, w2c, W, H, need - 1)
        assert need3 == need and (tri_id == -1).all() and (depth == 0).all() and (color == 0).all()
    empty = S.MeshScene(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, device=ctx.device)
    (color, depth, tri_id), need, _ = mesh_call(ctx, empty, mc.k_for(37, 21, 24.0), np.eye(4), 37, 21, 0)
    assert need == 0 and (tri_id == -1).all() and (depth == 0).all() and (color == 0).all()
    mc.check_partial_tiles(ctx.device)
    mc.check_capacity(ctx.device)


@entry("sensing", "eval", "gs_eval_frame 1x1, 5x17, 33x47 (odd), every mask combination, with SSIM")
def _(ctx):
    from tests import eval_cases as ec
    for H, W in ((1, 1), (5, 17), (33, 47)):
        ec.check_sums_and_flags(ctx.device, H, W)
        ec.check_ssim_same(ctx.device, H, W)


@entry("sensing", "eval_ms_ssim", "gs_eval_frame with MS-SSIM at the smallest legal size 161x163 (odd at every level)")
def _(ctx):
    from activesplat_amd import evaluate as E
    from tests import eval_cases as ec
    ec.check_ms_ssim(ctx.device, 161, 163)
    lay = E.frame_layout(163, 161, 4 | 8)
    assert len(ctx.g.find(lay.total_bytes, torch.uint8)) >= 1, "the evaluation workspace was not allocated inside the guard"


FAMILIES = sorted({e.family for e in ENTRIES})
REPORT = []


def run_entry(e, device, poison, oracle32, oracle64, byte=0xFF):
    """One entry inside the guard, through the Python twin of the front end (the same library calls in the same order; the C++ front end
    allocates where Python cannot see) -> (guarded allocations, region-checked buffers, const inputs)."""
    from activesplat_amd import rasterizer as R
    was = R.use_frontend
    R.use_frontend = False
    clear_workspace_caches()
    try:
        with G.guarded_allocations(device, poison=poison, byte=byte) as g:
            ctx = Context(device, g, oracle32, oracle64)
            e.run(ctx)
            g.verify()
            n = len(g.allocations)
            clear_workspace_caches()
    finally:
        R.use_frontend = was
        clear_workspace_caches()
    REPORT.append((e.family, e.name, poison, n, ctx.region_buffers, ctx.const_inputs))
    print(f"workspace {e.family}/{e.name} [{poison}{'' if poison != 'bytes' else ' %#x' % byte}]: {n} guarded allocations, "
          f"{ctx.region_buffers} region-checked buffers, {ctx.const_inputs} const inputs; shapes: {e.shapes}")
    return n, ctx.region_buffers, ctx.const_inputs
