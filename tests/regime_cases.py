"""Size regimes of the raster pipeline that the random scenes of tests/parity_cases.py land near and never on, shared by the host-emulated
kernel tests (tests/test_regimes.py) and the device tests (tests/test_gpu_regimes.py):

* tile lists of EXACTLY a threshold's length, and one more, with lists of other classes in the same launch -- every kernel of
  launch_tile_scatter_sort (csrc/tilebin.hip) decides per tile from the tile's own length (`n > CAP`, `BIG && n <= kBucketCap`, `skip_le`,
  `n <= CHUNK`), and the radix path sorts the same scenes;
* lists of 63, 64, 65, ... 1023, 1024, 1025 entries that ALL contribute, in the three families of blend kernels (the blend walks step 64 records
  at a time, the few-tile backward cuts lists at multiples of 256);
* images of 2049 .. 8192 tiles on the LDS path (tile_scan_kernel with 4 and 8 tiles per thread, the limit itself and one tile column past it) and
  a radix scene whose digit rows and block sums take a second trip.

Every comparison is parity_cases.check_forward / check_backward at the bars stated at the top of that module; nothing here adds a tolerance.  What a
scene is built to hold (list lengths, a walk that reaches the last entry, D and P past a trip) is asserted from the ORACLE's output."""
import numpy as np
import torch

from activesplat_amd import synthetic as syn
from tests import parity_cases as pc
from tests import util


def exact_lists(lengths, gx, gy, seed, crowded=False, blend=False, device="cpu"):
    """A 16 gx x 16 gy image whose tile t = ty gx + tx holds exactly lengths[t] Gaussians and every other tile none: pixel centres 5 .. 11 px inside
    the tile, splats of radius 2 (sort scenes: 0.3 px + the low-pass) or 3 (blend scenes: 0.4 .. 0.6 px per axis), so nothing reaches a
    neighbour.  Sort scenes are faint (opacity 0.005 .. 0.025); blend scenes scale the opacity with 4 / n so that a pixel's walk is still running
    at the list's last entry.  crowded: every depth inside 1e-4 of 2 (one bin of the bucket sort holds the list: its comparison network).  The
    rows are shuffled, so ids and tiles interleave across the binning chunks."""
    W, H = 16 * gx, 16 * gy
    rs, _ = util.scene(1, W, H, device=device)
    K = syn.intrinsics(W, H)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    g = torch.Generator().manual_seed(seed)
    tiles = sorted(lengths)
    counts = torch.tensor([lengths[t] for t in tiles])
    tile_of = torch.repeat_interleave(torch.tensor(tiles), counts)
    n_of = torch.repeat_interleave(counts, counts).float()
    N = int(counts.sum())
    u = 16.0 * (tile_of % gx).float() + 5.0 + 6.0 * torch.rand(N, generator=g)
    v = 16.0 * (tile_of // gx).float() + 5.0 + 6.0 * torch.rand(N, generator=g)
    z = 2.0 + 1e-4 * torch.rand(N, generator=g) if crowded else 0.5 + 3.5 * torch.rand(N, generator=g)
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    if blend:
        scales = (0.5 * z / fx)[:, None] * (0.8 + 0.4 * torch.rand(N, 3, generator=g))
        opac = torch.clamp(4.0 / n_of, 0.012, 0.9) * (0.5 + 0.5 * torch.rand(N, generator=g))
    else:
        scales = (0.3 * z / fx)[:, None].expand(N, 3)
        opac = 0.005 + 0.02 * torch.rand(N, generator=g)
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g))
    col = torch.rand(N, 3, generator=g)
    perm = torch.randperm(N, generator=g)
    rv = dict(means3D=means, rotations=rot, opacities=opac[:, None], scales=scales, colors_precomp=col)
    return rs, {k: t[perm].float().contiguous().to(device) for k, t in rv.items()}


def assert_lists(ref, lengths, gx, gy, contributing=False):
    """From the oracle's forward `ref`: every listed tile's range holds exactly its length, every other tile is empty; contributing: some pixel of
    each listed tile blends the list's LAST entry (the largest n_contrib of the tile's 256 pixels is the length)."""
    n = (ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0].astype(np.int64)).reshape(-1)
    want = np.zeros(gx * gy, np.int64)
    for t, c in lengths.items():
        want[t] = c
    assert np.array_equal(n, want), {t: (int(n[t]), int(want[t])) for t in np.nonzero(n != want)[0]}
    if contributing:
        last = np.asarray(ref["n_contrib"]).reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)
        assert np.array_equal(last, want), {t: (int(last[t]), int(want[t])) for t in np.nonzero(last != want)[0]}


# ---- sort-selection boundaries (csrc/tilebin.hip: kSortChunk 2048, its double 4096, kBucketCap 5632, the 8192-key merge, kBucketCapBig 11264,
# kSortCapMax 16384, and 32768 = the fourth merge pass) ------------------------------------------------------------------------------------------
# Each scene is rendered twice.  The second launch is OPTIMISTIC -- sized from the first one's counts plus a margin, so every kernel's per-tile
# decision runs under a bound no list has -- only where the guessed bound does not choose the algorithm (rasterizer._bin_and_render): not on the
# radix path, and not where gs_bin_layout would cut the lists into segments (a guessed bound of 8192 or more in at most 160 tiles, of 32768 or
# more in at most 640).  There the second launch is another exact one.  The `_wide` cases put the same boundary lengths into grids above those
# tile counts, so that they ARE launched under a guess: 272 tiles (at most 512: the 1024-thread bucket sort is available) and 656.
#: name -> (gx, gy, {tile: length}, crowded, forced path, expected path, the second launch is an optimistic hit)
SORT_CASES = {
    "A": (2, 1, {0: 5632, 1: 5633}, False, "auto", 1, True),                # guess 6049: the bucket sort next to the run sort + 8192-key merge
    "A_crowded": (2, 1, {0: 5632, 1: 5633}, True, "auto", 1, True),         # the comparison-network branch of both bucket instantiations
    "B": (4, 1, {0: 11264, 1: 11265, 2: 100, 3: 1}, False, "auto", 1, False),                 # (few tiles, guess >= 8192: segmented, exact)
    "C1": (2, 2, {0: 2048, 1: 2049, 2: 4096, 3: 4097}, False, "auto", 1, True),
    "C2": (2, 2, {0: 8192, 1: 8193, 3: 5632}, False, "auto", 1, False),
    "C3": (3, 2, {0: 16384, 1: 16385, 2: 5632, 5: 1}, False, "auto", 1, False),   # three merge passes; the short lists ride along through them
    "C4": (2, 2, {0: 32768, 1: 32769, 2: 4097}, False, "auto", 1, False),         # an even pass count: the run sort starts in pairs_alt
    "D": (33, 16, {0: 5632, 7: 5633, 100: 8192, 527: 8193, 300: 11265}, False, "auto", 1, True),   # 528 tiles > 512: no 1024-thread bucket sort
    "E": (33, 16, {0: 5632, 7: 5633, 100: 8192, 527: 8193}, False, "radix", 2, False),             # (radix: never optimistic)
    # guess 12033: both bucket instantiations AND the run sort + 16384-key merge are launched, each taking its own tiles
    "B_wide": (17, 16, {0: 11264, 1: 11265, 100: 100, 271: 1}, False, "auto", 1, True),
    "C2_wide": (17, 16, {0: 8192, 1: 8193, 3: 5632}, False, "auto", 1, True),                      # guess 8769
    # guess 17473 > kSortCapMax: merge passes through pairs_alt for lists the LDS merge would have taken at their true length
    "C3_wide": (17, 16, {0: 16384, 1: 16385, 2: 5632, 5: 1}, False, "auto", 1, True),
    "C4_wide": (41, 16, {0: 32768, 1: 32769, 2: 4097}, False, "auto", 1, True),                    # guess 34881: four passes
}

INTEGER_ARTEFACTS = ("tiles_touched", "rect", "keys_sorted", "point_list", "ranges", "n_contrib")


def check_sort_boundary(name, device, oracle32):
    """Forward of one SORT_CASES scene against the fp32 oracle (keys, ids and ranges bit for bit: check_forward), on the expected binning path, and
    rendered AGAIN through the same rasteriser: the first launch is sized from the exact counts; the second is the optimistic launch where the
    case table says so (asserted from the hit / miss counters: one hit, no re-launch) and a second exact launch elsewhere.  The integer artefacts
    of the two are identical."""
    from activesplat_amd import rasterizer as R
    gx, gy, lengths, crowded, force, path, optimistic = SORT_CASES[name]
    rs, rv = exact_lists(lengths, gx, gy, 0, crowded=crowded, device=device)
    R._capacity.clear()
    pc.set_sort_path(force)
    try:
        got, ref = pc.check_forward(rs, rv, oracle32)
        first = util.artefacts()
        assert first["path"] == path, first["path"]
        assert_lists(ref, lengths, gx, gy)
        hits, misses = R.last_stats.get("optimistic_hits", 0), R.last_stats.get("optimistic_misses", 0)
        again = util.run_product(rs, rv)
        second = util.artefacts()
        hits, misses = R.last_stats.get("optimistic_hits", 0) - hits, R.last_stats.get("optimistic_misses", 0) - misses
    finally:
        pc.set_sort_path("auto")
        R._capacity.clear()
    assert (hits, misses) == ((1, 0) if optimistic else (0, 1)), (hits, misses)
    assert second["path"] == path and again["D"] == got["D"] and np.array_equal(again["radii"], got["radii"])
    for k in INTEGER_ARTEFACTS:
        assert np.array_equal(first[k], second[k]), k
    return got, ref


# ---- blend chunk edges -------------------------------------------------------------------------------------------------------------------------
EDGES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
#: name -> (gx, gy, tile of EDGES[i], seed): 24 tiles (few-tile pipeline forward, three-walker backward), 272 (streams forward, plain backward), 800
#: (above kChainMinTiles = 768: chained backward).
#: The seed is the LOWEST whose scene the two oracles agree on (WELL_CONDITIONED below, a property of the references alone).  Of seeds 0 .. 5 the fp32
#: oracle sits at 3e-6 .. 4e-5 of the fp64 gradients on fourteen scenes and at 5e-3 .. 9e-3 on four (streams 2, chained 0 and 1): there ONE splat owns
#: a pixel at the alpha = 1/255 threshold that fp32 and fp64 decide differently and carries 98-100 % of the squared error in its row (DESIGN section 6,
#: tiers 2 and 3) -- such a scene measures the threshold, not the walk, and these cases run without the escape hatch.
BLEND_GRIDS = {
    "few_tiles": (6, 4, lambda i: i, 0),
    "streams": (17, 16, lambda i: 3 * i + 1, 0),
    "chained": (40, 20, lambda i: 40 * i + 7, 2),
}
#: the fp32 oracle's gradients within a tenth of the 1e-3 bar of the fp64 oracle's: no visibility decision separates the two arithmetics
WELL_CONDITIONED = 1e-4


def check_blend_edges(grid, device, oracle32, oracle64):
    """One tile per entry of EDGES, every entry of every list contributing: forward against the fp32 oracle, gradients against the fp64 oracle at
    the stated bar -- WITHOUT the fp32 escape hatch."""
    gx, gy, tile, seed = BLEND_GRIDS[grid]
    lengths = {tile(i): n for i, n in enumerate(EDGES)}
    assert len(lengths) == len(EDGES) and max(lengths) < gx * gy
    rs, rv = exact_lists(lengths, gx, gy, seed, blend=True, device=device)
    got, ref = pc.check_forward(rs, rv, oracle32)
    assert util.artefacts()["path"] == 1
    assert_lists(ref, lengths, gx, gy, contributing=True)
    dL = torch.randn(3, 16 * gy, 16 * gx, generator=torch.Generator().manual_seed(0))         # (check_backward's own)
    g64, g32 = (util.run_oracle(o, rs, rv, dL)["grads"] for o in (oracle64, oracle32))
    for k, r in g64.items():
        if np.abs(r).max() > 0:
            rel = np.linalg.norm(np.asarray(g32[k], np.float64).reshape(r.shape) - r) / np.linalg.norm(r)
            assert rel < WELL_CONDITIONED, ("the scene is ill-conditioned in fp32: pick another seed", k, rel)
    pc.check_backward(rs, rv, oracle64)
    return got, ref


# ---- large images and large counts -------------------------------------------------------------------------------------------------------------
def _every_97th_large_and_faint(rv):
    # 1 % of the splats cover more than 16 tiles each (the balanced emitter), spread over all binning chunks of the scatter
    s, o = rv["scales"].clone(), rv["opacities"].clone()
    s[::97] *= 40.0
    o[::97] *= 0.3
    rv.update(scales=s, opacities=o)


def _larger_and_fainter(rv):
    rv.update(scales=rv["scales"] * 3.0, opacities=rv["opacities"] * 0.5)


#: name -> (N, W, H, seed, scene keywords, mutation, forced path, expected path, backward too)
LARGE_CASES = {
    "replica_frame": (12_000, 1200, 680, 3, {}, _every_97th_large_and_faint, "auto", 1, True),       # 75 x 43 = 3225 tiles: 4 per scan thread
    "full_hd": (9_000, 1920, 1080, 4, {}, _every_97th_large_and_faint, "auto", 1, False),            # 120 x 68 = 8160 tiles: 8 per scan thread
    # (full_hd's sub-pixel splats put the fp32 ORACLE at 0.992 of the gradient elements: the gradient check gets splats of a few pixels)
    "full_hd_grad": (9_000, 1920, 1080, 4, dict(scale_jitter=0.1), _larger_and_fainter, "auto", 1, True),
    "lds_limit": (6_000, 2048, 1024, 5, {}, _every_97th_large_and_faint, "auto", 1, False),          # exactly kMaxLdsTiles = 8192 tiles
    "past_lds_limit": (6_000, 2064, 1024, 5, {}, _every_97th_large_and_faint, "auto", 2, False),     # 129 x 64 = 8256 tiles: radix
    # D > 256 x 2048 (a second trip of radix_rowscan_kernel) and P > 1024 x 256 (a second trip of scan_block_sums_kernel)
    "radix_two_trips": (280_000, 160, 120, 2, {}, None, "radix", 2, False),
}


def check_large(name, device, oracle32, oracle64=None):
    """Forward of one LARGE_CASES scene on the expected binning path; with oracle64, and where the case asks for it, the gradients at the stated bar
    without the fp32 escape hatch."""
    N, W, H, seed, kw, mutate, force, path, backward = LARGE_CASES[name]
    rs, rv = util.scene(N, W, H, seed=seed, device=device, **kw)
    if mutate:
        mutate(rv)
    pc.set_sort_path(force)
    try:
        got, ref = pc.check_forward(rs, rv, oracle32)
        assert util.artefacts()["path"] == path, util.artefacts()["path"]
        if name == "radix_two_trips":
            assert ref["D"] > 256 * 2048 and ref["radii"].shape[0] > 1024 * 256, (ref["D"], ref["radii"].shape)
        if backward and oracle64 is not None:
            pc.check_backward(rs, rv, oracle64)
    finally:
        pc.set_sort_path("auto")
    return got, ref
