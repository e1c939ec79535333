/*
 * gsplat_hip.h -- C ABI of libgsplat_hip.so, the MI355X (gfx950) native replacement for the
 * `_C.rasterize_gaussians{,_backward}` extension entry points that ActiveSplat reaches through
 * `diff_gaussian_rasterization.GaussianRasterizer`.
 *
 * Reference interface replaced (the implementation itself is an un-vendored submodule, reference
 * .gitmodules:1-3; these are the call sites that define the contract):
 *   settings      : src/mapper/splatam/utils/recon_helpers.py:14-27 (12-field settings tuple)
 *   forward call  : src/mapper/splatam/splatam.py:208,212,338,430,431 and
 *                   src/mapper/splatam/utils/slam_helpers.py:131-138 (keyword tensors)
 *   backward      : autograd of `color` incl. means2D.grad, src/mapper/splatam/splatam.py:207-209,
 *                   src/mapper/splatam/__init__.py:470, utils/slam_external.py:100-108
 *   Adam          : src/mapper/splatam/splatam.py:118-124, src/mapper/splatam/__init__.py:479-480
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with h_ (pinned/pageable host);
 *   - all float tensors are contiguous fp32, layouts exactly those of the Python API
 *     (means3D [P,3], shs [P,M,3], colors_precomp [P,3], opacities [P,1], scales [P,3],
 *      rotations [P,4] (w,x,y,z), cov3D_precomp [P,6]); base pointers 16-byte aligned;
 *   - `stream` is a hipStream_t; every entry point only enqueues work on it (no implicit sync);
 *   - return value 0 = success, otherwise a GS_E* code; gs_last_error() gives the message;
 *   - no torch types.  Process-wide state: the last-error string (thread-local), the host-mapped status word (gs_async_status_word) and the
 *     development knobs gs_set_sort_path, gs_set_forward_segments, gs_set_half_quadrants, gs_set_backward_chain[_tickets|_polls],
 *     gs_set_backward_segments, gs_set_forward_priority, gs_set_node_distance_path (defaults: automatic path choice, segments on, few-tile kernels up to 256 tiles, three chained pieces above 768 tiles).
 *     The knobs are atomics that every launch reads ONCE: set from another thread (the reference runs a visualiser thread next to the mapper) a
 *     new value takes effect at a launch boundary of the other threads, never inside one launch's decisions; a forward and the backward that
 *     consumes its state tolerate a change in between (the forward clears the hand-over flags and records its "recorded" word whatever the
 *     knobs say).  The gs_profile_* event log (off by default) is not thread-safe: one profiling thread at a time.
 *
 * Call sequence for one forward:
 *     gs_preprocess_forward(...)            // per-Gaussian stage + tile counting; writes the counts
 *                                           // {D, max instances per tile} to d_counts / h_counts
 *     <caller synchronises `stream`, reads the counts, allocates binning workspace + point_list>
 *     gs_render_forward(...)                // scatter into tile segments, per-tile depth sort, alpha-blend
 * and for the backward:
 *     gs_render_backward(...)               // per-pixel replay -> per-Gaussian grads -> input grads
 * Optional: gs_render_forward may run optimistically right behind gs_preprocess_forward with capacities from the previous
 * frame (see its comment), and may zero-fill the backward's scratch as a side job (backward_scratch).
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_OK 0
#define GS_EINVAL 1      /* bad argument (null pointer, bad size, both/neither of an xor pair) */
#define GS_ELAUNCH 2     /* a HIP launch / runtime call failed */
#define GS_ECAPACITY 3   /* workspace too small for this call */

#define GS_TILE 16       /* tile edge in pixels (spec constant) */
#define GS_GEOM_FLOATS 12

typedef void* gs_stream_t;

/* Mirror of GaussianRasterizationSettings (recon_helpers.py:14-27). bg/viewmatrix/projmatrix/campos
 * stay device tensors exactly as the reference hands them over (transposed [1,4,4] matrices). */
typedef struct GsCamera {
    int32_t image_width;
    int32_t image_height;
    int32_t sh_degree;      /* active SH degree 0..3 (only read when shs != NULL) */
    int32_t sh_coeffs;      /* M = coefficients per Gaussian stored in shs; 0 when colors_precomp */
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t num_views;      /* 0/1: one view.  V > 1: multi-view ATLAS (forward only, see gs_atlas_layout): viewmatrix / projmatrix /
                             * campos hold V consecutive blocks; image_width is the width of ONE view */
    const float* bg;          /* [3] */
    const float* viewmatrix;  /* [16] = w2c^T row-major */
    const float* projmatrix;  /* [16] = (P w2c)^T row-major */
    const float* campos;      /* [3] */
} GsCamera;

/* Byte offsets of the arrays inside the caller-allocated state buffers, so that tests (and other
 * hosts) can inspect the integer artefacts without any private header. */
typedef struct GsGeomLayout {
    uint64_t total_bytes;
    uint64_t geom;          /* float [P][12]: x, y, conic_a, conic_b, conic_c, opacity, r, g, b, depth, ext_x, ext_y */
    uint64_t rect;          /* uint32 [P][2]: (xmin | xmax<<16), (ymin | ymax<<16) in tiles */
    uint64_t tiles_touched; /* uint32 [P] */
    uint64_t offsets;       /* uint32 [P]  inclusive scan of tiles_touched (radix-sort path only) */
    uint64_t block_sums;    /* uint32 [ceil(P/256)+1] exclusive scan of per-block tile counts */
    uint64_t clamped;       /* uint8  [P][4]: SH colour clamp flags (r,g,b,pad) */
    uint64_t tile_total;    /* uint32 [tiles]: instances per tile */
    uint64_t tile_base;     /* uint32 [ceil(P/2048)][tiles]: slice reserved by each binning workgroup (one row per 2048 Gaussians is written; the
                             * region holds ceil(P/1024) rows; images of more than 8192 tiles: one word) */
    uint64_t sh_jac;        /* float [P][10]: 3x3 d(rgb)/d(view direction) of SH inputs + the colour clamp flags in the tenth word, written when
                             * want_backward (the `clamped` array is then not written) */
    uint64_t depth_bits;    /* uint32 [P]: float bits of the view-space depth (binning key) */
} GsGeomLayout;

typedef struct GsImageLayout {
    uint64_t total_bytes;
    uint64_t ranges;        /* uint32 [tiles][2] : [start,end) into point_list */
    uint64_t final_T;       /* float  [H*W] */
    uint64_t n_contrib;     /* uint32 [H*W] : 1-based position in the tile list of the last contributor */
    uint64_t split_state;   /* images of at most 256 tiles: float [21][5][H*W] + [4][H*W] + 1 word, per-pixel running state at the recorded list
                             * positions (every 256th up to 4096, then the powers of two up to 131072), where the backward may cut a
                             * quadrant's walk; larger images: the hand-over state of the chained backward walks, the whole region */
} GsImageLayout;

#define GS_SORT_AUTO 0
#define GS_SORT_TILE_LDS 1   /* count/scatter into tile segments + per-tile sort in LDS / registers (bucket sort for lists of <= 5632 keys, else bitonic
                              * runs + merges); <= 8192 tiles */
#define GS_SORT_RADIX 2      /* duplicate with 64-bit keys + device radix sort (any image size) */

typedef struct GsBinLayout {
    uint64_t total_bytes;
    uint64_t path;          /* GS_SORT_TILE_LDS or GS_SORT_RADIX: what gs_render_forward will run */
    uint64_t pairs;         /* TILE_LDS: uint64 [D] : (float_bits(view depth) << 32) | Gaussian index, tile-major -- scratch: as the scatter pass
                             * left them for tile lists of <= 5632 keys (the bucket sort writes point_list only), sorted in place for longer lists */
    uint64_t keys_unsorted; /* RADIX: uint64 [D] : (tile << 32) | float_bits(view depth) */
    uint64_t vals_unsorted; /* RADIX: uint32 [D] : Gaussian index */
    uint64_t keys_sorted;   /* RADIX: uint64 [D] */
    uint64_t sort_temp;     /* RADIX: scratch of the sort */
    uint64_t segments;      /* > 1: gs_render_forward composites every tile list in this many parallel segments (few tiles, long lists) */
    uint64_t seg_T;         /* float [tiles][segments][256]: per-segment transmittance of the segmented forward, then uint32 [tiles][4] flag words */
    uint64_t pairs_alt;     /* TILE_LDS, tile lists longer than 16384: uint64 [D], the second buffer of the pairwise merge passes */
} GsBinLayout;

/* Multi-view atlas (the planner's look-around: V small views of one map, src/mapper/splatam/__init__.py:707-736): with
 * GsCamera.num_views = V > 1 the per-Gaussian stage runs once over V x P virtual Gaussians (view-major, each view's rows
 * padded to whole 256-row blocks) and binning, sorting and blending see ONE image of V view slots side by side, every slot
 * padded to whole tiles.  Sizes for the caller: virtual_P = rows of radii[] and the P to pass to gs_geom_layout; atlas_width =
 * the width to pass to the layout functions and the row length of the output images; view v occupies columns
 * [v * view_stride, v * view_stride + view_width).  gs_preprocess_forward / gs_render_forward still take the INPUT count P.
 * THE SLOT RULE.  With rows = virtual_P / V and gxv = view_stride / 16, input Gaussian i of view v is virtual row v * rows + i; the rows
 * [v * rows + P, (v + 1) * rows) are padding (radius 0, tile count 0).  A live row's record is the single view's record with ONE change: its
 * pixel x is fl32(x_in_view + 16 * gxv * v), the view-local fp32 pixel mean plus the slot offset, rounded once to fp32.  Pixel y, conic,
 * opacity, colour and depth are bit for bit what a single-view forward of view v's settings computes.  The tile rect is clamped to the view's
 * own gxv columns and both x bounds are then moved by v * gxv; atlas tile (ty, v * gxv + tx) holds the list of view v's tile (tx, ty) with
 * v * rows added to every index.  (The blend forms pixel - mean in fp32 from the rounded x: a view in a later slot differs from its
 * single-view render by that rounding -- up to 2^-12 px in slots past column 4096 -- and by nothing else.) */
int gs_atlas_layout(int32_t P, int32_t view_width, int32_t num_views, int32_t* virtual_P, int32_t* atlas_width, int32_t* view_stride);
int gs_geom_layout(int32_t P, int32_t width, int32_t height, GsGeomLayout* out);
int gs_image_layout(int32_t width, int32_t height, GsImageLayout* out);
int gs_bin_layout(int64_t D, uint32_t max_tile_instances, int32_t width, int32_t height, GsBinLayout* out);
/* Force a binning path (GS_SORT_*; default GS_SORT_AUTO picks TILE_LDS whenever the image has at most 8192 tiles). */
int gs_set_sort_path(int32_t path);
/* Segmented compositing of long tile lists in images of few tiles (GsBinLayout.segments > 1): on by default; 0 switches it
 * off (every list is then walked by one workgroup, bit-reproducible forward). */
int gs_set_forward_segments(int32_t on);
/* Images of at most max_tiles tiles (default 256; 0 = never) get twice the wavefronts: 256 tiles x 4 quadrants are one wavefront per SIMD of
 * an MI355X.  The forward's wavefronts take half an 8 x 8 quadrant each (half their lanes idle; results unchanged); the backward walks every
 * tile list in up to three segments (gs_set_backward_segments), the front ones from per-pixel states the forward recorded at the cuts
 * (gradients agree to rounding). */
int gs_set_half_quadrants(int32_t max_tiles);
/* Images of more than min_tiles tiles (default 768 = more quadrants than the chip holds backward walkers; negative: the default; values
 * below 256 act as 256): every quadrant's backward walk is cut into `pieces` consecutive pieces (default 3, the maximum; 1 = one walker per
 * quadrant) that run as separate workgroups in dispatch order and hand the per-pixel running state on through the image workspace.  The
 * arithmetic per pixel is the same sequence either way (gradients differ only by the order of the atomic sums). */
int gs_set_backward_chain(int32_t pieces, int32_t min_tiles);
/* Chained walks, robustness.  Ordered tickets (gs_set_backward_chain_tickets(1); default OFF: one more dependent round trip per walker, measured
 * +2.5-5 % of the backward blend): a workgroup's place in the chain order is a ticket it draws when it starts, so the piece it waits for is by
 * construction already running or done -- no assumption about the order in which the hardware starts workgroups.  Off: the place is the
 * workgroup index, which the dispatcher hands out in order (a piece only ever waits for a lower index of its own XCD class).
 * gs_set_backward_chain_polls: bound of a piece's wait, in polls (-1: the default, 2^21 ~ 0.3 s; below -1: every piece gives up without
 * looking -- the tests' way to take the timeout path).
 * A wait that runs out sets bit 0 of the process' host-mapped status word and the walk continues with NaN state (NaN gradients for that
 * quadrant's Gaussians).  gs_async_status_word returns the word's HOST address (created on first call; call it once before the first
 * backward): the caller reads it -- a plain load -- before its next launch; non-zero = the previous chained backward's gradients are invalid:
 * gs_set_backward_chain(1, -1), gs_async_status_clear(), clear the word, and render again (activesplat_amd/rasterizer.py does exactly that).
 * The backward is asynchronous: the host learns of the event a render later, by which time an optimiser step on the NaN gradients would have
 * been enqueued (optimizer.step(), gs_adam_rows, or the Adam inside gs_render_backward_raw_adam -- the same launch).  The timed-out walker
 * therefore also sets a sticky word in DEVICE memory (created together with the host word) that every optimiser kernel of this library reads
 * first: while it is set gs_adam_step / gs_adam_step_multi / gs_adam_rows / gs_render_backward_raw_adam leave parameters and moments
 * untouched (gs_adam_rows still forwards the unstepped rows; the raw_adam backward writes zeros to dL_dmeans2D).  gs_async_status_clear
 * synchronises the device and clears that word: steps run again.  Step counters the host advanced for skipped steps stay advanced. */
int gs_set_backward_chain_tickets(int32_t on);
int gs_set_backward_chain_polls(int32_t polls);
/* Issue priority of the forward blend's quadrant walkers (images of more than 256 tiles, unsegmented lists).  All walkers of a frame are resident
 * from the start and end by saturation at very different list depths; once per 64-entry chunk a walker estimates how far it still has to go and
 * sets its wavefront's priority (0 ... 3) from that, so that the longest walk of a SIMD runs at its own pace while the others fill the issue slots
 * it leaves.  The library starts in mode 1 with its default parameter (measurements: profiles/forward_priority.txt).
 *      mode 0: off (every wavefront at priority 0);
 *      1: by the largest transmittance T among the quadrant's pixels that still blend: one level for each of T > param, param^2, param^3
 *         (param in (0, 1); default 0.1);
 *      2: by the chunks still to go if that pixel keeps the decay rate it has shown so far: one level for each of more than param, 2 param,
 *         4 param chunks (default 3);
 *      3: by the chunk index alone (a control without information about the walk): one level for each of param, 2 param, 3 param chunks walked
 *         (default 6).
 * Modes 1 and 2 never rate a walk longer than its list: one level less below 9, 6 and 3 chunks of list left.  param <= 0 selects the mode's
 * default; a negative mode restores the mode and parameter the library starts with.  Only the order in which wavefronts issue changes: every
 * output is bit-identical in all modes. */
int gs_set_forward_priority(int32_t mode, float param);
int gs_async_status_word(uint32_t** host_word);
int gs_async_status_clear(void);
/* Introspection of the few-tile backward's cuts: the recorded list position nearest to `target` (0: none below it) and its level (-1: none) --
 * every 256th position up to 4096, then the powers of two up to 131072, nearest in ratio above 4096. */
int gs_recorded_cut(uint32_t target, uint32_t* nearest, int32_t* level);
/* Test / tuning knob: list segments (walkers) per quadrant in the backward blend of images of few tiles (at most 256): 3 (default: 3 x 256
 * tiles x 4 quadrants = the chip's 3072 walker slots), 2, or 1 (one walker per quadrant; the forward then records nothing).  The walkers
 * of a quadrant resume from the per-pixel state the forward recorded at every 256th list position up to 4096 and at the powers of two
 * beyond. */
int gs_set_backward_segments(int32_t segments);
/* bytes of the scratch gs_render_backward needs (per-Gaussian 2-D gradient records) */
uint64_t gs_backward_scratch_bytes(int32_t P);

const char* gs_last_error(void);
const char* gs_version(void);
/* Integer version of THIS binary interface: bumped whenever an entry point's argument list or a published record layout changes (e.g.
 * the seed argument of gs_densify_children, the 40-byte SH Jacobian record).  A host binding compares it with the GS_ABI_VERSION it was
 * written against before the first call, so that a stale prebuilt library fails at load time instead of misreading its arguments. */
#define GS_ABI_VERSION 28
int32_t gs_abi_version(void);

/* Optional per-stage timing (hipEvents recorded on the caller's stream around each stage's launches).
 * Off by default; bench.py switches it on for its roofline leg.  gs_profile_collect synchronises the
 * recorded events, sums elapsed ms and call counts per stage into arrays of gs_profile_stage_count()
 * entries, and clears the log. */
int gs_profile_enable(int32_t on);
int32_t gs_profile_stage_count(void);
const char* gs_profile_stage_name(int32_t stage);
int gs_profile_collect(float* ms_sum, int32_t* calls, int32_t n_stages);

/* Stage 1: per-Gaussian preprocess (view/projective transform, near cull, 3-D -> 2-D covariance, conic,
 * radius, tile rect, SH -> RGB), tile counting and the tile-range scan.  Writes radii[P] (0 = culled),
 * the geom state and the tile ranges (image state); d_counts[0] = D (number of tile instances),
 * d_counts[1] = largest per-tile instance count; if h_counts != NULL both also reach that host buffer
 * asynchronously -- stored by the scan kernel itself when h_counts is mapped pinned memory (hipHostMalloc), by an
 * async copy otherwise (read them after synchronising `stream` or an event recorded behind this call). Exactly one of shs/colors_precomp and
 * exactly one of (scales,rotations)/cov3D_precomp must be given.
 * want_backward != 0 with shs: the stage also stores, per Gaussian, the 3x3 block sum_k coef[k] (x) grad b_k(direction) in the geom
 * state, so that gs_render_backward (have_sh_jacobian = 1) does not read the coefficient rows a second time.
 * PAIRING RULE: want_backward and have_sh_jacobian go together.  With want_backward != 0 the colour clamp flags travel in the Jacobian
 * record and the separate `clamped` array is NOT written: a backward over that geom state must pass have_sh_jacobian = 1 (with 0 it
 * would read an unwritten `clamped` array); with want_backward = 0 the backward must pass have_sh_jacobian = 0. */
int gs_preprocess_forward(const GsCamera* cam, int32_t P,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities, const float* scales, const float* rotations,
                          const float* cov3D_precomp,
                          int32_t* radii, void* geom_state, void* image_state, uint32_t* d_counts,
                          uint32_t* h_counts, int32_t want_backward, gs_stream_t stream);

/* Stage 2: bin the instances by tile and depth-sort every tile list, then front-to-back alpha blend.
 * out_color [3,H,W], out_depth [1,H,W] (sum z*alpha*T), out_opacity [1,H,W] (1 - T_final).
 * point_list [D] receives the (tile, depth, index)-sorted Gaussian ids (kept for the backward).
 * out_depth_sq [1,H,W] (nullable) additionally receives sum z^2*alpha*T: with out_depth and out_opacity these are
 * the three channels of the reference's second, [z, 1, z^2] raster pass (slam_helpers.py:196-249), produced by
 * the SAME pass as the colour.
 * D and max_tile_instances may be UPPER BOUNDS (the capacity the caller sized bin_state / point_list for) as long as
 * gs_bin_layout reports GS_SORT_TILE_LDS for them: no kernel reads or writes past D, so a host may enqueue this call
 * right behind gs_preprocess_forward with bounds from the previous frame, read h_counts afterwards, and simply call it
 * again with the exact counts in the rare frame where they exceed the bounds (the call is idempotent; a frame whose
 * true counts exceed the bounds it was launched with has unspecified outputs).
 * backward_scratch (nullable, gs_backward_scratch_bytes(P) bytes): the gradient records gs_render_backward accumulates into
 * are zero-filled by the blend workgroups of THIS call (stores riding along an arithmetic-bound kernel) instead of by a
 * separate fill in front of the backward; pass the same buffer to gs_render_backward with scratch_zeroed = 1. */
int gs_render_forward(const GsCamera* cam, int32_t P, int64_t D, uint32_t max_tile_instances,
                      void* geom_state, void* bin_state, uint32_t* point_list, void* image_state,
                      float* out_color, float* out_depth, float* out_opacity, float* out_depth_sq,
                      void* backward_scratch, gs_stream_t stream);

/* Backward of `out_color` (and, when dL_ddepth [1,H,W] is non-NULL, of `out_depth`; of out_opacity and out_depth_sq as well through
 * gs_render_backward_grads below) w.r.t. every input.  Any dL_d* output pointer may be NULL if that input
 * was not given (shs vs colors_precomp, scales/rotations vs cov3D_precomp).
 * dL_dmeans2D [P,3] receives the NDC-scaled screen-space gradient (x*0.5W, y*0.5H, 0).
 * scratch: gs_backward_scratch_bytes(P) bytes; scratch_zeroed != 0 promises that it is all zero (see gs_render_forward's
 * backward_scratch) -- the call leaves it dirty either way.  have_sh_jacobian != 0: geom_state comes from a
 * gs_preprocess_forward(want_backward = 1) call. */
int gs_render_backward(const GsCamera* cam, int32_t P, int64_t D,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* scales, const float* rotations, const float* cov3D_precomp,
                       const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                       const void* image_state, const float* dL_dcolor, const float* dL_ddepth,
                       float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacities,
                       float* dL_dcolors_precomp, float* dL_dshs, float* dL_dscales,
                       float* dL_drotations, float* dL_dcov3D, void* scratch, int32_t scratch_zeroed,
                       int32_t have_sh_jacobian, gs_stream_t stream);

/* Raw-parameter mode of the two calls above ("fused pre-activations", one step further than gs_activate_*): the inputs are
 * the mapper's PARAMETERS -- world-frame means, logit opacities, log scales ([P,3], or [P,1] when isotropic != 0), unnormalised quaternions --
 * and the frame transform + activations of slam_helpers.py:252-304,124-139 run inside the per-Gaussian kernels (h_pose7: HOST array
 * {qw,qx,qy,qz,tx,ty,tz} of the frame's relative w2c, as for gs_activate_forward).  Colours given or 16-coefficient SH rows; no precomputed
 * covariance; one view.  The backward returns the gradients w.r.t. the parameters; accumulate != 0: dL_dmeans3D, dL_dlogit_opacities,
 * dL_dlog_scales, dL_dunnorm_rotations and dL_dcolors_precomp are ADDED to what the buffers hold (rows of Gaussians that were not rendered stay
 * untouched) -- the gradient accumulation over the keyframes of a batch without autograd's `grad += new` passes.
 * max_2D_radius / seen (both nullable): the mapper's visibility statistics of this render, as gs_visibility_stats would leave them --
 * max_2D_radius[i] = max(max_2D_radius[i], radii[i]) in place, seen[i] = radii[i] > 0 -- written by the forward kernel itself. */
int gs_preprocess_forward_raw(const GsCamera* cam, int32_t P, const float* means3D, const float* shs, const float* colors_precomp,
                              const float* logit_opacities, const float* log_scales, const float* unnorm_rotations,
                              const float* h_pose7, int32_t isotropic, float* max_2D_radius, uint8_t* seen, int32_t* radii, void* geom_state,
                              void* image_state, uint32_t* d_counts, uint32_t* h_counts, int32_t want_backward, gs_stream_t stream);
int gs_render_backward_raw(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                           const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                           int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                           const void* image_state, const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, float* dL_dmeans3D,
                           float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                           float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, gs_stream_t stream);

/* Camera-pose gradient (tracking / bundle adjustment: transform_to_frame(camera_grad=True), slam_helpers.py:252-304).  The same backward as
 * gs_render_backward_raw, which also writes dL_dpose7[7] (DEVICE) = dL/d(qw,qx,qy,qz,tx,ty,tz) of the h_pose7 the call received: through the
 * frame transform of every rendered Gaussian's mean and, for an anisotropic map, through q_cam (x) normalize(q) of its rotation.  The
 * reduction is deterministic (per-workgroup rows in pose_scratch, gs_pose_grad_scratch_bytes(P) bytes, summed in a fixed order in fp64):
 * two calls on the same inputs give the same bits, and the parameter gradients are bit-identical to gs_render_backward_raw's.
 * The rotation part is the reference's (slam_helpers.py:252-304): the matrix as build_rotation(q) = R(q / |q|), the Gaussians' rotations as
 * quat_mult(q, normalize(q_i)) -- the derivative of both as written, including build_rotation's normalisation.
 * pose_only != 0 (tracking): no parameter gradient is formed -- the five dL_d* parameter outputs may be NULL and are not written,
 * `accumulate` is ignored; dL_dmeans2D and the pose gradient are written as usual.  dL_dpose7 is always overwritten (never accumulated).
 * There is no pose-gradient form of gs_render_backward_raw_adam. */
uint64_t gs_pose_grad_scratch_bytes(int32_t P);
int gs_render_backward_raw_pose(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                                const void* image_state, const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, float* dL_dmeans3D,
                                float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                                float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, int32_t pose_only,
                                float* dL_dpose7, void* pose_scratch, gs_stream_t stream);

/* Gradients of EVERY image output (opt-in: the three calls above differentiate colour and depth only).  The four images a loss may hang on:
 * dL_dcolor [3,H,W] (required), dL_ddepth [1,H,W], dL_dopacity [1,H,W] (out_opacity = the silhouette, 1 - T_final) and dL_ddepth_sq [1,H,W]
 * (out_depth_sq, sum z^2*alpha*T); the last three nullable.  With them the one pass is a complete differentiable replacement of the
 * reference's second, [z, 1, z^2] raster pass (slam_helpers.py:196-249), not only for the losses the reference happens to use.
 * The three *_grads entry points are gs_render_backward, gs_render_backward_raw and gs_render_backward_raw_pose with the (dL_dcolor, dL_ddepth)
 * pair replaced by this block; those three are wrappers that pass NULL for the two new images and launch the same kernels as before.
 * dL_dopacity costs one per-pixel scalar.  dL_ddepth_sq adds a blended channel to the replay; the forward records no sum z^2 state for the
 * list segments of few-tile images, so a call that carries it walks such an image with one walker per quadrant whatever
 * gs_set_backward_segments says (chained walks are unaffected).
 * NOT covered: gs_render_backward_raw_adam, gs_render_backward_raw_pose_dev and the fused loss kernels in front of them (gs_mapping_loss*,
 * gs_tracking_loss*) produce and take colour and depth gradients only. */
typedef struct GsImageGrads {
    const float* dL_dcolor;
    const float* dL_ddepth;
    const float* dL_dopacity;
    const float* dL_ddepth_sq;
} GsImageGrads;
int gs_render_backward_grads(const GsCamera* cam, int32_t P, int64_t D,
                             const float* means3D, const float* shs, const float* colors_precomp,
                             const float* scales, const float* rotations, const float* cov3D_precomp,
                             const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                             const void* image_state, const GsImageGrads* grads,
                             float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacities,
                             float* dL_dcolors_precomp, float* dL_dshs, float* dL_dscales,
                             float* dL_drotations, float* dL_dcov3D, void* scratch, int32_t scratch_zeroed,
                             int32_t have_sh_jacobian, gs_stream_t stream);
int gs_render_backward_raw_grads(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                 int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                                 const void* image_state, const GsImageGrads* grads, float* dL_dmeans2D, float* dL_dmeans3D,
                                 float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                                 float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, gs_stream_t stream);
int gs_render_backward_raw_pose_grads(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                      const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                      int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state,
                                      const uint32_t* point_list, const void* image_state, const GsImageGrads* grads, float* dL_dmeans2D,
                                      float* dL_dmeans3D, float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs,
                                      float* dL_dlog_scales, float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed,
                                      int32_t have_sh_jacobian, int32_t pose_only, float* dL_dpose7, void* pose_scratch, gs_stream_t stream);

/* Fused dense Adam step over one flat parameter tensor with torch.optim.Adam semantics
 * (non-amsgrad, no weight decay): splatam.py:118-124 uses betas (0.9,0.999), eps 1e-15.
 * `step` is the 1-based step count of this tensor AFTER the increment.  Hyper-parameters are doubles (as the
 * Python floats torch receives): 1-beta, the bias corrections and lr/(1-beta1^t) are formed in double and
 * rounded to fp32 once, exactly like torch's scalar handling.
 * param, grad, exp_avg and exp_avg_sq of a tensor with n > 0 must be 16-byte aligned (the kernels make 128-bit accesses): anything else --
 * a contiguous view at an odd element offset -- is GS_EINVAL, with the index of the tensor in the message, before anything is launched
 * (gs_adam_step_multi: before the first launch of the batch, so no tensor of a refused call is stepped).  gs_render_backward_raw_adam
 * asks the same of param / exp_avg / exp_avg_sq of unnorm_rotations and of the SH rows.  gs_adam_rows takes any 4-byte-aligned pointer. */
int gs_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                 double lr, double beta1, double beta2, double eps, int32_t step, gs_stream_t stream);

/* The same step for several parameter tensors in one launch (the mapper's five per-Gaussian groups; each keeps its
 * own lr and step counter exactly like torch's per-group state).  `tensors` is a HOST array. */
typedef struct GsAdamTensor {
    int64_t n;
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    double lr, beta1, beta2, eps;
    int32_t step;
    int32_t reserved;       /* padding; set to 0 */
} GsAdamTensor;
int gs_adam_step_multi(int32_t count, const GsAdamTensor* tensors, gs_stream_t stream);

/* gs_render_backward_raw with the optimiser step INSIDE (single-keyframe steps: the reference's mapping loop -- loss.backward() followed by
 * optimizer.step() on the same keyframe's gradients, src/mapper/splatam/__init__.py:470-480 -- and BASELINE configs[2]'s loop): the
 * per-Gaussian backward kernel applies Adam to the five per-Gaussian parameter tensors and their moments in place with the gradient it
 * forms, instead of writing gradient tensors that gs_adam_step_multi reads back one launch later.  Same arithmetic as gs_adam_step*, so the
 * parameters and moments afterwards are those of gs_render_backward_raw + gs_adam_step_multi, bit for bit.
 * adam5: HOST array of exactly five descriptors in the order {means3D, logit_opacities, log_scales, unnorm_rotations, colours | SH rows};
 * .param must be the very tensors passed as inputs (they are updated in place), .grad is ignored, .n = elements of the tensor
 * (3P, P, 3P | P, 4P, 3P | 48P), .step >= 1 is the step number this call performs.  Gaussians that were not rendered are stepped with a zero
 * gradient (their moments decay), as a dense optimiser does.  dL_dmeans2D is written as usual; no parameter gradient is written, no
 * accumulation.  SH rows need have_sh_jacobian = 1 (the kernel overwrites the rows it would otherwise read). */
int gs_render_backward_raw_adam(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                int32_t isotropic, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                                const void* image_state, const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, void* scratch,
                                int32_t scratch_zeroed, int32_t have_sh_jacobian, const GsAdamTensor* adam5, gs_stream_t stream);

/* Keyframe-sharded optimiser step (activesplat_amd/parallel.py; SURVEY.md section 8e -- new capability, the reference steps one
 * keyframe on one GPU, src/mapper/splatam/__init__.py:450-480): glue between the K per-key tensors ([N, width] fp32, K <= 8,
 * sum of widths <= 64) and ONE flat [rows, G] buffer, G = sum of widths.  `tensors` is a HOST array.
 *   gs_pack_columns  : flat[r][.] = the keys' `grad` rows (NULL grad = zeros) for r < n, zeros for n <= r < n_padded
 *                      (the send buffer of the reduce-scatter / all-reduce);
 *   gs_adam_rows     : Adam (arithmetic of gs_adam_step) on rows [row_lo, row_lo + n_valid) of every key, gradient from
 *                      grad_shard[r - row_lo][.]; the updated rows are also written to out_shard (may be NULL), rows
 *                      n_valid..n_rows-1 of it zero (the send buffer of the all-gather);
 *   gs_unpack_columns: the keys' `param` rows r < n = flat[r][.]. */
typedef struct GsRowTensor {
    float* param;
    float* exp_avg;
    float* exp_avg_sq;
    const float* grad;
    double lr, beta1, beta2, eps;
    int32_t width;
    int32_t step;
} GsRowTensor;
int gs_pack_columns(int32_t count, const GsRowTensor* tensors, int64_t n, int64_t n_padded, float* flat, gs_stream_t stream);
int gs_adam_rows(int32_t count, const GsRowTensor* tensors, int64_t row_lo, int64_t n_valid, int64_t n_rows, const float* grad_shard,
                 float* out_shard, gs_stream_t stream);
int gs_unpack_columns(int32_t count, const GsRowTensor* tensors, int64_t n, const float* flat, gs_stream_t stream);

/* Fused frame transform + activations (replaces transform_to_frame + transformed_params2rendervar,
 * src/mapper/splatam/utils/slam_helpers.py:252-304,124-139).  h_pose7 is a HOST array {qw,qx,qy,qz,tx,ty,tz}: the
 * normalised camera quaternion and translation of the relative w2c.  isotropic != 0: log_scales is [P,1] (tiled to 3,
 * rotations only normalised).  The backward takes the gradients w.r.t. the four outputs (any may be NULL = zero). */
int gs_activate_forward(int32_t P, int32_t isotropic, const float* h_pose7, const float* means3D, const float* unnorm_rotations,
                        const float* logit_opacities, const float* log_scales, float* out_means3D, float* out_rotations,
                        float* out_opacities, float* out_scales, gs_stream_t stream);
int gs_activate_backward(int32_t P, int32_t isotropic, const float* h_pose7, const float* unnorm_rotations,
                         const float* out_opacities, const float* out_scales, const float* g_means3D, const float* g_rotations,
                         const float* g_opacities, const float* g_scales, float* d_means3D, float* d_unnorm_rotations,
                         float* d_logit_opacities, float* d_log_scales, gs_stream_t stream);
/* The same, ADDED to what the four d_* buffers hold: the gradient accumulation over the keyframes of a batch (autograd's `grad += new`
 * passes) inside the kernel that produces the gradient. */
int gs_activate_backward_accumulate(int32_t P, int32_t isotropic, const float* h_pose7, const float* unnorm_rotations,
                                    const float* out_opacities, const float* out_scales, const float* g_means3D, const float* g_rotations,
                                    const float* g_opacities, const float* g_scales, float* d_means3D, float* d_unnorm_rotations,
                                    float* d_logit_opacities, float* d_log_scales, gs_stream_t stream);

/* gs_activate_backward / _accumulate (accumulate != 0) with the camera-pose gradient: dL_dpose7[7] (DEVICE) as for gs_render_backward_raw_pose,
 * from g_means3D / g_rotations and the world-frame means3D; pose_scratch = gs_pose_grad_scratch_bytes(P) bytes.  pose_only != 0: only the pose
 * gradient (out_opacities, out_scales and the four d_* may be NULL).  A row whose g_means3D and g_rotations are all zero (a Gaussian the
 * rasteriser did not render) adds nothing, whatever its parameters hold. */
int gs_activate_backward_pose(int32_t P, int32_t isotropic, const float* h_pose7, const float* means3D, const float* unnorm_rotations,
                              const float* out_opacities, const float* out_scales, const float* g_means3D, const float* g_rotations,
                              const float* g_opacities, const float* g_scales, float* d_means3D, float* d_unnorm_rotations,
                              float* d_logit_opacities, float* d_log_scales, int32_t accumulate, int32_t pose_only, float* dL_dpose7,
                              void* pose_scratch, gs_stream_t stream);

/* Fused mapping loss, forward AND backward (replaces src/mapper/splatam/splatam.py:213-249 + the SSIM of
 * utils/slam_external.py:54-97 and their autograd):
 *   loss = w_depth * mean_{gt_depth>0, finite} |gt_depth - depth| + w_im * (0.8 * mean|im - gt_im| + 0.2 * (1 - SSIM))
 * im, gt_im [3,H,W]; depth, gt_depth [1,H,W]; depth_sq [1,H,W] nullable (only its NaN-ness enters the mask).
 * Writes losses[4] = {loss, weighted image term, weighted depth term, loss again} (device), dL_dim [3,H,W],
 * dL_ddepth [1,H,W]. */
/* persistent_call = 0: `scratch` is any buffer of gs_mapping_loss_scratch_bytes bytes (its accumulators are cleared by a memset in front of the
 * two kernels).  persistent_call = k >= 1: the k-th call (k counts up by one) on a scratch that its owner zeroed ONCE and keeps for this
 * stream: the call accumulates in one of two accumulator sets and its second kernel zeroes the other for call k + 1 -- no memset launch. */
uint64_t gs_mapping_loss_scratch_bytes(int32_t width, int32_t height);
int gs_mapping_loss(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth,
                    const float* depth_sq, const float* gt_depth, float w_im, float w_depth, float* losses,
                    float* dL_dim, float* dL_ddepth, void* scratch, int64_t persistent_call, gs_stream_t stream);

/* ---- ignore_outlier_depth_loss (src/mapper/splatam/splatam.py:220-228), all in fp32 without FMA contraction ----
 *   err    = |gt_depth - depth| * (gt_depth > 0)            (the product: NaN * 0 and inf * 0 are NaN, as in torch)
 *   median = torch.median(err): element (n - 1) / 2 of the sorted errors of ALL n = width * height pixels -- unmeasured pixels count as zeros,
 *            the LOWER of two middle values -- and NaN as soon as one err is NaN
 *   keep   = err < 10 * median                              (strict; the product rounded to fp32 once)
 * gs_depth_error_median writes the median to d_median (DEVICE, 1 float), bit-identical to torch's and from call to call: an exact radix
 * select in three histogram passes (11 + 11 + 10 bits of the error's bit pattern), each ONE launch over a grid of workgroups (LDS histogram,
 * then integer atomics into the pass' global histogram) and a one-workgroup launch that picks the value.  The workgroups of a pass re-derive
 * the prefix of the pass before from its finished histogram: no workgroup waits for another inside a launch.  scratch:
 * gs_depth_error_median_scratch_bytes bytes, cleared by a memset inside the call.  The grid is a function of width * height only
 * (gs_depth_error_median_workgroups reports it); gs_depth_error_median_grid is the same call with the grid given, for tests and
 * measurements (workgroups = 1: a single workgroup; 0: the automatic grid; at most 1024).  No state is kept between calls.
 * The _outlier forms of the two losses take that scalar: their depth mask is the plain mask AND keep.  A median of 0 (half of the pixels
 * unmeasured or exact) or NaN keeps nothing: gs_mapping_loss_outlier then gives a NaN depth term and loss (the mean of nothing), dL_ddepth all
 * zero and the usual dL_dim; gs_tracking_loss_outlier gives zero sums and zero gradient images.  In gs_tracking_loss_outlier the colour mask
 * is always the mask tiled to 3 channels (splatam.py:242), with or without use_sil_for_loss.  No gradient passes through the median.
 * Everything else -- arguments, scratch protocol, row layout -- is gs_mapping_loss' / gs_tracking_loss'. */
uint64_t gs_depth_error_median_scratch_bytes(int32_t width, int32_t height);
int gs_depth_error_median(int32_t width, int32_t height, const float* depth, const float* gt_depth, void* scratch, float* d_median,
                          gs_stream_t stream);
int gs_depth_error_median_grid(int32_t width, int32_t height, const float* depth, const float* gt_depth, void* scratch, float* d_median,
                               int32_t workgroups, gs_stream_t stream);
int32_t gs_depth_error_median_workgroups(int32_t width, int32_t height);
int gs_mapping_loss_outlier(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth,
                            const float* depth_sq, const float* gt_depth, float w_im, float w_depth, float* losses,
                            float* dL_dim, float* dL_ddepth, void* scratch, int64_t persistent_call, const float* d_median, gs_stream_t stream);

/* ---- Camera tracking on the device (SplaTAM's per-frame pose optimisation; tracking loss src/mapper/splatam/splatam.py:220-249) ----
 * One iteration, no host round trip beyond the render's counters:
 *   gs_preprocess_forward_raw_dev -> gs_render_forward -> gs_tracking_loss -> gs_render_backward_raw_pose_dev -> gs_tracking_step
 * The pose lives in the caller's parameter tensors cam_unnorm_rots [1,4,T] and cam_trans [1,3,T] (contiguous fp32, DEVICE): column time_idx
 * (stride num_frames = T) is read in place by the kernels, the quaternion normalised as F.normalize does (x / max(|x|, 1e-12)), and the step
 * updates that column in place.  With ignore_outlier_depth_loss the iteration is
 *   ... -> gs_render_forward -> gs_depth_error_median -> gs_tracking_loss_outlier -> gs_render_backward_raw_pose_dev -> gs_tracking_step
 * (same rows, same step).  What stays on torch: use_l1 = False, and tracking on the activation path. */

/* Tracking loss, value and gradient in one pass (tracking=True, use_l1=True):
 *   mask  = (gt_depth > 0) & !isnan(depth) & !isnan(depth_sq - depth^2), & (silhouette > sil_thres) when use_sil_for_loss
 *   depth = sum_mask |gt_depth - depth| ;  im = sum |gt_im - im| over the mask tiled to 3 channels (use_sil_for_loss) or over every pixel
 *   dL_ddepth [1,H,W] = w_depth sign(depth - gt_depth) [mask], dL_dim [3,H,W] = w_im sign(im - gt_im) [colour mask]  (sign(0) = 0; the
 *   values, signed zeros included, are autograd's for loss = w_depth depth + w_im im).  silhouette [1,H,W] may be NULL without use_sil_for_loss.
 * loss_rows: gs_tracking_loss_scratch_bytes(width, height) bytes, one row of partial sums per workgroup (no atomics).  losses (DEVICE, may be
 * NULL) = {w_depth depth + w_im im, w_depth depth, w_im im}, the rows reduced in fp64 in a fixed order: bit-identical from call to call.
 * gs_tracking_step reduces the same rows itself. */
uint64_t gs_tracking_loss_scratch_bytes(int32_t width, int32_t height);
int gs_tracking_loss(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth, const float* depth_sq,
                     const float* gt_depth, const float* silhouette, int32_t use_sil_for_loss, float sil_thres, float w_im, float w_depth,
                     float* dL_dim, float* dL_ddepth, void* loss_rows, float* losses, gs_stream_t stream);
/* the same with the outlier rule (see gs_depth_error_median above) */
int gs_tracking_loss_outlier(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth, const float* depth_sq,
                             const float* gt_depth, const float* silhouette, int32_t use_sil_for_loss, float sil_thres, float w_im, float w_depth,
                             float* dL_dim, float* dL_ddepth, void* loss_rows, float* losses, const float* d_median, gs_stream_t stream);

/* gs_preprocess_forward_raw with the pose read from device memory: cam_unnorm_rots[0, :, time_idx], cam_trans[0, :, time_idx] in place of
 * h_pose7 (everything else, the visibility statistics included, as gs_preprocess_forward_raw). */
int gs_preprocess_forward_raw_dev(const GsCamera* cam, int32_t P, const float* means3D, const float* shs, const float* colors_precomp,
                                  const float* logit_opacities, const float* log_scales, const float* unnorm_rotations,
                                  const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, int32_t isotropic,
                                  float* max_2D_radius, uint8_t* seen, int32_t* radii, void* geom_state, void* image_state, uint32_t* d_counts,
                                  uint32_t* h_counts, int32_t want_backward, gs_stream_t stream);

/* The planner's top-down maps (src/visualizer/visualizer.py:923-965: the free map and the visible map the Voronoi planner thresholds) from the
 * map's PARAMETERS in ONE raster pass.  The reference renders them as two passes through one camera (1000 m above the scene, scale_modifier
 * 0.01): the Gaussians between the agent's head and foot (__cut_gaussian_by_height) for the accumulated opacity, every Gaussian on a white
 * background for the image.  Both share camera, projection, tile rectangles and depth order, and a tile's in-band list is a subsequence of its
 * full list, so here every pixel carries two running states through one walk.
 *   gs_preprocess_forward_topdown : gs_preprocess_forward_raw (colours given, identity pose: cam->viewmatrix is the world-to-camera matrix)
 *       that also tests every Gaussian's height -- IN BAND iff !(-y < band_upper || -y > band_lower), y = means3D[i][1] as stored, fp32: the
 *       complement of the reference's cut, both ends inclusive; a NaN y is in band and is then culled like any non-finite input.  The
 *       visualiser passes band_upper = agent_head, band_lower = agent_foot - agent_foot_adjust.  The bit travels as the SIGN of the opacity
 *       in the 48-byte record: geom_state of this call is for gs_render_forward_topdown only.  Everything else -- radii, rects, counts,
 *       d_counts / h_counts, the caller's synchronisation -- as gs_preprocess_forward_raw.  image_state: only its tile ranges are used
 *       (GsImageLayout.ranges, the first region: a buffer of GsImageLayout.final_T bytes is enough).  A NaN band is refused (GS_EINVAL).
 *   gs_render_forward_topdown : binning and depth sort as gs_render_forward (same capacities, also capacity-safe and idempotent), then one
 *       blend launch that writes, all DEVICE, 4-byte aligned:
 *         free_opacity       float32 [H*W]   : 1 - T composited over the in-band Gaussians only
 *         free_map_binary    uint8   [H*W]   : free_opacity <= 0.4f
 *         visible_rgb        uint8   [H*W*3] : (clamp(colour, 0, 1) * 255) truncated, interleaved RGB; colour = all Gaussians over cam->bg
 *                                              (the reference: white)
 *         visible_map_binary uint8   [H*W]   : grey(visible_rgb) == 255, grey = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's 8-bit
 *                                              COLOR_RGB2GRAY in its published fixed-point form)
 *       Per state the fp32 operations per list entry are gs_render_forward's, in its order (stop rule T (1 - alpha) < 1e-4 per state).
 *       No depth, final_T, contributor index or backward state is written: there is no backward of this path.  One view only. */
int gs_preprocess_forward_topdown(const GsCamera* cam, int32_t P, const float* means3D, const float* colors_precomp, const float* logit_opacities,
                                  const float* log_scales, const float* unnorm_rotations, int32_t isotropic, float band_upper, float band_lower,
                                  int32_t* radii, void* geom_state, void* image_state, uint32_t* d_counts, uint32_t* h_counts, gs_stream_t stream);
int gs_render_forward_topdown(const GsCamera* cam, int32_t P, int64_t D, uint32_t max_tile_instances, void* geom_state, void* bin_state,
                              uint32_t* point_list, void* image_state, float* free_opacity, uint8_t* free_map_binary, uint8_t* visible_rgb,
                              uint8_t* visible_map_binary, gs_stream_t stream);

/* gs_render_backward_raw_pose with pose_only = 1 and the pose read from device memory (as gs_preprocess_forward_raw_dev).  The per-workgroup
 * pose rows go to pose_scratch (gs_pose_grad_scratch_bytes(P)); dL_dpose7 (DEVICE, may be NULL: gs_tracking_step reduces the rows itself) =
 * dL/d(qw,qx,qy,qz,tx,ty,tz) of the NORMALISED column, as gs_render_backward_raw_pose's of the h_pose7 it receives.  dL_dmeans2D is written. */
int gs_render_backward_raw_pose_dev(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                    const float* logit_opacities, const float* log_scales, const float* unnorm_rotations,
                                    const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, int32_t isotropic,
                                    const int32_t* radii, const void* geom_state, const uint32_t* point_list, const void* image_state,
                                    const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, void* scratch, int32_t scratch_zeroed,
                                    int32_t have_sh_jacobian, float* dL_dpose7, void* pose_scratch, gs_stream_t stream);

/* Per-frame tracking state (gs_tracking_state_bytes() bytes, DEVICE; 32 floats): [0,7) Adam first moments, [7,14) second moments, [14] the
 * smallest loss so far, [15,22) the candidate pose (qw..qz unnormalised, tx..tz), [22,25) the last step's {loss, depth, im} (weighted), [25] the
 * number of steps skipped.  gs_tracking_begin starts a frame: moments 0, smallest loss 1e20, candidate = the column as it is (a fresh
 * torch.optim.Adam per frame, as the reference builds one). */
uint64_t gs_tracking_state_bytes(void);
int gs_tracking_begin(const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, void* state, gs_stream_t stream);

/* The tail of tracking iteration `step` (1-based), one workgroup: (1) the loss rows of gs_tracking_loss (same width, height, weights) reduced as
 * that call reduces them; (2) the pose rows of gs_render_backward_raw_pose_dev (same P) reduced as gs_render_backward_raw_pose reduces them, then
 * taken through F.normalize's Jacobian at the unnormalised column, all in double and rounded to fp32 once: dL/dcam_unnorm_rots[..., t] and
 * dL/dcam_trans[..., t]; (3) torch.optim.Adam's
 * update of those 7 values in place (betas 0.9 / 0.999, eps 1e-8, lr_rot for the quaternion and lr_trans for the translation, the bias
 * corrections of `step`, torch's fp32 operation order); skipped while a chained backward in front has failed (gs_async_status_word);
 * (4) the best candidate: loss < the smallest loss so far (strict) -> that loss and the column AFTER this update become the candidate;
 * (5) history_row (DEVICE, may be NULL) = {loss, depth, im, the 7 values after the update}. */
int gs_tracking_step(int32_t P, const void* pose_scratch, int32_t width, int32_t height, const void* loss_rows, float w_im, float w_depth,
                     float* cam_unnorm_rots, float* cam_trans, int64_t num_frames, int64_t time_idx, double lr_rot, double lr_trans, int32_t step,
                     void* state, float* history_row, gs_stream_t stream);


/* Stream compaction for prune / densify surgery (replaces the boolean-mask gathers of
 * src/mapper/splatam/utils/slam_external.py:143-164 remove_points and the torch.cat appends of
 * :126-140): gs_compact_index turns a keep mask [n] (uint8) into the ascending list of kept row indices
 * src_index[0..count) and writes count to *d_count; gs_gather_rows then copies dst[r][:] = src[src_index[r]][:]
 * for a tensor of `row_floats` floats per row (one index build serves params, Adam moments and statistics;
 * an index list with repeats implements clone / split). */
uint64_t gs_compact_scratch_bytes(int64_t n);
int gs_compact_index(int64_t n, const uint8_t* keep, uint32_t* src_index, uint32_t* d_count, void* scratch,
                     gs_stream_t stream);
int gs_gather_rows(int64_t n_out, int32_t row_floats, const uint32_t* src_index, const float* src, float* dst,
                   gs_stream_t stream);
/* The same gather for rows [0, n_copy); rows [n_copy, n_out) of dst are zero-filled by the same launch (Adam moments of appended
 * Gaussians, slam_external.py:131-134). */
int gs_gather_rows_zero_tail(int64_t n_out, int64_t n_copy, int32_t row_floats, const uint32_t* src_index, const float* src,
                             float* dst, gs_stream_t stream);

/* Densify / prune decisions of slam_external.py:171-247 in ONE launch.  Per Gaussian i of the N present before the event:
 *   keep_orig[i]  = 1 if it stays (not split, not culled)
 *   keep_clone[i] = 1 if it is cloned AND the clone survives the cull        (nullable; densify only)
 *   keep_child[i] = 1 if it is split AND its children survive the cull       (nullable; densify only)
 *   split_mask[i] = 1 if it is split (before the cull; indexes injected samples)   (nullable)
 * grad_accum/denom NULL = prune only (slam_external.py:171-192: keep_orig = not culled).  d_scene_radius: DEVICE pointer to
 * variables['scene_radius'] (no host read-back).  scale_dim = 1 (isotropic) or 3.  remove_big: the `iter >= remove_big_after`
 * clause (scale > 0.1 scene_radius). */
int gs_densify_classify(int32_t N, int32_t scale_dim, const float* log_scales, const float* logit_opacities,
                        const float* grad_accum, const float* denom, const float* d_scene_radius, float grad_thresh,
                        float opacity_thresh, int32_t remove_big, int32_t num_to_split_into, uint8_t* keep_orig,
                        uint8_t* keep_clone, uint8_t* keep_child, uint8_t* split_mask, gs_stream_t stream);
/* Split children (a contiguous block of rows): means3D += R(normalised unnorm_rotation) * sample, log_scale = log(exp(log_scale) /
 * (0.8 n)) in place (slam_external.py:224-230).  samples [n_child,3] are the N(0, scale) offsets (slam_external.py:221-224:
 * torch.normal(0, the parent's scale)); samples == NULL: they are drawn inside the kernel by a counter-based generator
 * (splitmix64 of (seed, child row, draw) -> Box-Muller; per-axis scales when scale_dim = 3): no sample tensor, no extra launches. */
int gs_densify_children(int32_t n_child, int32_t scale_dim, int32_t num_to_split_into, const float* unnorm_rotations,
                        const float* samples, uint64_t seed, float* means3D, float* log_scales, gs_stream_t stream);
/* The densify event's ONE index list from its three masks in one count / scan / write sequence:
 *   src_index = [ rows with keep_a | rows with keep_b | repeat_c blocks of the rows with keep_c ]   (each ascending)
 * d_counts[0..2] = the three totals (device; the host reads them once, afterwards, to size the new tensors).  src_index must hold
 * n * (2 + repeat_c) entries in the worst case.  Replaces three gs_compact_index passes, a torch.cat and a repeat. */
uint64_t gs_compact3_scratch_bytes(int64_t n);
int gs_compact_index3(int64_t n, const uint8_t* keep_a, const uint8_t* keep_b, const uint8_t* keep_c, int32_t repeat_c,
                      uint32_t* src_index, uint32_t* d_counts, void* scratch, gs_stream_t stream);

/* Densification statistics, one launch each.
 * gs_visibility_stats : seen[i] = radii[i] > 0 (uint8, nullable); max_2D_radius[i] = max(max_2D_radius[i], radii[i]) (nullable)
 *                       -- src/mapper/splatam/splatam.py:296-298.
 * gs_accumulate_grad2d: for seen rows, grad_accum += ||means2D_grad[i,:2]||, denom += 1; means2D_grad is [P,3]
 *                       -- src/mapper/splatam/utils/slam_external.py:100-108. */
int gs_visibility_stats(int32_t P, const int32_t* radii, uint8_t* seen, float* max_2D_radius, gs_stream_t stream);
int gs_accumulate_grad2d(int32_t P, const float* means2D_grad, const uint8_t* seen, float* grad_accum, float* denom,
                         gs_stream_t stream);

/* DBSCAN on a pixel grid, batched over images: the clustering the reference's mapper runs on its look-around panoramas
 * (src/mapper/__init__.py:8-19 get_convexhull_volume: DBSCAN(eps=5, min_samples=25) on np.where(invisibility > 0.8); :92-117
 * get_invisibility_clusters: threshold 0.3, DBSCAN(eps=5, min_samples=10), per-cluster centre and sum).  For image b, row y, column x the value
 * read is values[b * image_stride + y * row_stride + x] (strides in floats: a panorama is read in place from an atlas or a gathered tensor).
 * The rule, which reproduces sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(np.column_stack(np.where(mask))) label for label:
 *   1. tested = complement ? 1.0f - v : v (fp32); mask = tested > threshold (fp32; a NaN is unmasked);
 *   2. count(p) = masked pixels q with dy*dy + dx*dx <= eps*eps (integers, p included, the disc clipped at the image border);
 *      core(p) = mask(p) && count(p) >= min_samples;
 *   3. core pixels within eps of each other are connected; a component's root is its smallest row-major pixel index y * W + x; clusters are
 *      numbered 0..C-1 in ascending root order;
 *   4. a masked pixel that is not core takes the SMALLEST cluster number among the core pixels of its disc (border), or is noise;
 *   5. labels: -2 unmasked, -1 noise, else the cluster number.
 * Outputs, all DEVICE:
 *   labels     int32 [B, H, W]
 *   n_clusters int32 [B]                   the true count, also when it exceeds max_clusters (the tables are then truncated, the labels are not)
 *   table      int32 [B, max_clusters, 4]  {count, sum_row, sum_col, root} over the cluster's pixels, border pixels included -- exact; the centre
 *                                          points.mean(axis=0) is (sum_row / count, sum_col / count).  Rows at or beyond n_clusters: {0, 0, 0, -1}
 *   sum_value  float32 [B, max_clusters]   sum of the tested value over the cluster's pixels; 0 beyond n_clusters
 *   total      float32 [B]                 sum of the tested value over the whole image
 * The two float sums run in a fixed order (at most 64 terms per thread, then butterflies over 1024 threads: no float atomics) and are
 * bit-identical from run to run; a tested value that is not finite counts as 0 in them, so they are always finite.  The integer outputs do
 * not depend on scheduling (components are united by atomic minimum).  No host synchronisation; every loop in the kernels has a bound that
 * follows from the image size.  Supported: 1 <= B <= 65535, 1 <= H, W <= 4096 with H * W <= 65536, 1 <= eps <= 8, min_samples >= 1,
 * 1 <= max_clusters <= 65535, row_stride >= W; anything else is GS_EINVAL.  workspace: gs_grid_dbscan_layout(...).total_bytes bytes, DEVICE,
 * 8-byte aligned, contents irrelevant before and after (the offsets are published for debugging only). */
typedef struct GsDbscanLayout {
    uint64_t total_bytes, mask_bits, core_bits, root_bits, word_prefix, parent, root, row_range;
} GsDbscanLayout;
int gs_grid_dbscan_layout(int32_t B, int32_t H, int32_t W, int32_t max_clusters, GsDbscanLayout* out);
int gs_grid_dbscan(int32_t B, int32_t H, int32_t W, const float* values, int64_t row_stride, int64_t image_stride, float threshold,
                   int32_t complement, int32_t eps, int32_t min_samples, int32_t max_clusters, void* workspace, int32_t* labels,
                   int32_t* n_clusters, int32_t* table, float* sum_value, float* total, gs_stream_t stream);

/* Hull volumes of the clusters gs_grid_dbscan found: the loop of get_convexhull_volume behind its DBSCAN line (src/mapper/__init__.py:29-90:
 * cv2.dilate, cv2.findContours, the contour's depth lookup, scipy.spatial.ConvexHull, the two sums), batched over images and clusters, so that
 * a Voronoi node's score is two doubles.  labels [B, H, W] int32, n_clusters [B] and sum_value [B, max_clusters] are gs_grid_dbscan's outputs
 * at the same max_clusters; depth is read as depth[b * image_stride + y * row_stride + x] (strides in floats).
 * The rule, for image b and cluster c with 0 <= c < min(n_clusters[b], max_clusters):
 *   a. mask(y, x) = labels[b, y, x] == c.
 *   b. dil(y, x) = OR of mask(y + i - ay, x + j - ax) over the set cells (i, j) of the footprint, ay = kh / 2, ax = kw / 2; pixels outside the
 *      image count as 0 (cv2.dilate with its default anchor and border).  The footprint is DATA: footprint_rows is a HOST array of kh words,
 *      bit j of word i = cell (i, j); kh and kw odd, 1..15.  OpenCV's getStructuringElement(MORPH_ELLIPSE, (15, 15)) restated: row i is the run
 *      of half-width round_half_even(7 * sqrt((49 - (i - 7)^2) / 49)) around column 7 -- 7,7,7,6,6,5,4,0 for |i - 7| = 0..7.
 *   c. the outer border, OpenCV's border following with CHAIN_APPROX_SIMPLE.  Direction codes 0..7 are (dx, dy) = (1,0),(1,-1),(0,-1),(-1,-1),
 *      (-1,0),(-1,1),(0,1),(1,1).  p0 = the first set pixel of dil in row-major order.  s = 4; repeat s = (s - 1) & 7 until the neighbour of p0
 *      in direction s is set (call it p1) or s is 4 again (the contour is then the single point p0).  p = p0, prev = s ^ 4; loop: search
 *      s + 1, s + 2, ... (mod 8, at most 8 candidates) for the first set neighbour q of p, in direction s'; if s' != prev emit p and set
 *      prev = s'; if q == p0 and p == p1 stop; else p = q, s = (s' + 4) & 7.  At most 4 H W + 8 steps.
 *      ONLY the 8-connected component of dil that contains p0 is traced.  The reference takes max(contours, key=contourArea); the two agree
 *      when dil is one component, which holds for the shipped parameters (two pixels within eps = 5 of each other lie inside each other's
 *      15 x 15 ellipse, so a DBSCAN cluster dilates to one component).  With a footprint smaller than the clustering radius a cluster can
 *      dilate to several components, and this call then scores the one that holds the first pixel.
 *   d. for every emitted (x, y): z = depth[b, y, x] (fp32); the point is skipped when z == skip_depth (the reference: 15.0f) and when z is not
 *      finite (status bit 1).  Points may repeat (a thin shape is walked along both sides).
 *   e. volume[b, c] = x_scale * y_scale * the volume of the convex hull of the points in PIXEL coordinates (x, y integers, z widened to fp64);
 *      the reference scales x by deg2rad(360 / W) and y by deg2rad(150 / H) first, which multiplies the volume by their product.  In pixel
 *      units four points that share a column, a row or a depth have an orientation determinant of exactly 0, which keeps the plateaus of a
 *      depth image from deciding faces by rounding.  An incremental hull in fp64: a first simplex, a face is visible iff det > 0 strictly, the
 *      visible faces are replaced by the fan over their horizon; the determinant is evaluated without FMA contraction.  Fewer than 4 points,
 *      or no four points off one plane: volume 0 (the reference gives 0 or, through its 1e-10 jitter, something of that order).
 *      More than max_points emitted points: status bit 0, volume 0.  More than 2 n - 4 faces (the visible set of a point was not a disc:
 *      rounding on nearly coplanar points): status bit 3, volume 0.  That branch is DEFENSIVE: it keeps the face table in bounds, no input
 *      is known that takes it (exact zeros in pixel units are what keeps the visible set a disc), and no test reaches it.
 *   f. sum_volume[b] = sum over c of volume[b, c]; sum_invisibility[b] = sum over c of (double) sum_value[b, c] * volume[b, c]; ascending c,
 *      fp64, one thread.  Status bit 2: n_clusters[b] > max_clusters (the sums then cover the first max_clusters clusters only).
 * Outputs, all DEVICE: volume fp64 [B, max_clusters] (0 beyond n_clusters); n_points int32 [B, max_clusters], the number of EMITTED points
 * (before the skips of d, and the true number when it exceeds max_points); contour_xy int32 [B, max_clusters, max_points, 2] (nullable; the
 * first min(n_points, max_points) emitted points of a cluster, the rest is not written); sum_volume, sum_invisibility fp64 [B]; status int32
 * [B], the OR over the image's clusters.  No atomics: two calls give the same bits.  Every loop is bounded by the image size, max_points or the
 * face bound; the bound that matters is the horizon search of e, 3 V^2 edge-against-face tests for a point that sees V <= 2 n - 4 faces, shared
 * by 64 lanes: a handful for a contour in general position, ~3e6 steps per lane for one point at V ~ 2 max_points = 8192.  The dilation and border rules restate OpenCV's documented behaviour; they were NOT run against cv2.
 * Supported: the sizes of gs_grid_dbscan and 4 <= max_points <= 4096; anything else is GS_EINVAL.  workspace: gs_cluster_hulls_layout(...)
 * .total_bytes bytes, DEVICE, 8-byte aligned. */
typedef struct GsHullLayout {
    uint64_t total_bytes, cluster_status;
} GsHullLayout;
int gs_cluster_hulls_layout(int32_t B, int32_t H, int32_t W, int32_t max_clusters, int32_t max_points, GsHullLayout* out);
int gs_cluster_hulls(int32_t B, int32_t H, int32_t W, const int32_t* labels, const float* depth, int64_t row_stride, int64_t image_stride,
                     const int32_t* n_clusters, const float* sum_value, int32_t max_clusters, const uint32_t* footprint_rows, int32_t kh,
                     int32_t kw, float skip_depth, double x_scale, double y_scale, int32_t max_points, void* workspace, double* volume,
                     int32_t* n_points, int32_t* contour_xy, double* sum_volume, double* sum_invisibility, int32_t* status, gs_stream_t stream);

/* The per-frame look target's image half (get_high_loss_samples, src/mapper/splatam/__init__.py:212-218): the mask of the pixels where the
 * map's render lies behind the measured depth, and that mask shrunk to a grid_height x grid_width grid (90 x 90: one pixel per degree), which
 * gs_grid_dbscan(grid, threshold 0, eps 5, min_samples 10) clusters next.  render_depth, opacity, gt_depth: [height * width] fp32, DEVICE.
 * Pixel rule (fp32, operation for operation :212-215):
 *   err = fabsf(depth - gt) * (gt > 0 ? 1.0f : 0.0f);   m = depth > gt && err > depth_err_thres && opacity > opacity_thres
 *   -- a NaN in any of the three makes the pixel 0, and so does an infinite depth over gt <= 0 (inf * 0 is NaN).
 * Resize rule: cv2.resize(mask_u8, (grid_width, grid_height), INTER_LINEAR) on the 0 / 1 image, in integers.  Per axis with n_src source and
 * n_dst destination samples, for destination sample d:
 *   den = 2 n_dst;  num = (2 d + 1) n_src - n_dst   (the pixel-centre coordinate (d + 0.5) n_src / n_dst - 0.5, times den);
 *   i0 = floor(num / den) (towards -inf);  w1 = num - i0 den;  w0 = den - w1;  taps clamp(i0), clamp(i0 + 1) into [0, n_src - 1];
 *   S = sum over the four taps of m[tap_y][tap_x] * wy * wx;   grid = 1.0f iff 2 S >= den_x * den_y (the bilinear value rounded half up), else 0.0f.
 * The rule is exact on every machine and equals float64 bilinear sampling of that convention pixel for pixel, exact ties included.  NOT pinned:
 * for uint8 input cv2 quantises the two weights of an axis to 11 bits, so a grid pixel whose exact value lies within about 2^-11 of one half
 * may come out differently in cv2 (exact ties are about 0.6 % of the grid pixels at 256 x 256 -> 90 x 90 on random masks); nobody has run cv2
 * against this rule.
 * Outputs, DEVICE: mask_full uint8 [height * width] (0 / 1; nullable -- the grid is the same with and without it), grid fp32 [grid_height *
 * grid_width].  One launch, integer arithmetic behind the pixel rule, no atomics, no host synchronisation: nothing depends on scheduling.
 * Supported: 1 <= width, height <= 16384; 1 <= grid_width, grid_height <= 4096 with grid_width * grid_height <= 65536 (what gs_grid_dbscan
 * takes); finite thresholds >= 0; anything else, or a null pointer other than mask_full, is GS_EINVAL before any launch. */
int gs_high_loss_grid(int32_t width, int32_t height, const float* render_depth, const float* opacity, const float* gt_depth,
                      float depth_err_thres, float opacity_thres, int32_t grid_width, int32_t grid_height, uint8_t* mask_full, float* grid,
                      gs_stream_t stream);

/* Map growth (replaces add_new_gaussians, src/mapper/splatam/splatam.py:332-379, with get_pointcloud :25-75 and
 * initialize_new_params :304-329).  render_depth / silhouette / gt_depth are [H*W] device images, color is [3,H*W];
 * h_intrinsics4 = HOST {fx,fy,cx,cy}; h_c2w12 = HOST row-major 3x4 camera-to-world of the frame.  Outputs must hold H*W
 * rows (the worst case); d_counts[0] = pixels flagged non-present BEFORE the valid-depth mask (the reference enters its
 * append branch, which also resets the densification statistics, iff this is > 0), d_counts[1] = rows written, in
 * row-major pixel order.  log_scales is [rows,1] when isotropic != 0, else [rows,3].
 * NaN rule: the median of the depth error is torch.median's -- the lower median, and NaN as soon as ONE error is NaN (a NaN pixel in
 * render_depth or gt_depth, or an infinite render_depth where gt_depth <= 0).  `error > 2 median` is then false for every pixel and only
 * the silhouette test (silhouette < sil_thres) flags pixels.  The median is gs_depth_error_median's select (its histograms are part of the
 * scratch); width * height < 2^31 as there, else GS_EINVAL. */
uint64_t gs_grow_scratch_bytes(int32_t width, int32_t height);
int gs_grow_gaussians(int32_t width, int32_t height, const float* render_depth, const float* silhouette,
                      const float* gt_depth, const float* color, const float* h_intrinsics4, const float* h_c2w12,
                      float sil_thres, int32_t isotropic, float* out_means3D, float* out_rgb_colors,
                      float* out_unnorm_rotations, float* out_logit_opacities, float* out_log_scales,
                      uint32_t* d_counts, void* scratch, gs_stream_t stream);

/* Keyframe overlap scores (the loop of keyframe_selection_overlap, src/mapper/splatam/utils/keyframe_selection.py:62-86):
 * counts[k] = number of the n_pts world points [n_pts,3] that project into keyframe k (row-major 4x4 w2c at
 * w2c[16k]) inside the image shrunk by `edge` pixels, with positive depth.  h_intrinsics9 = HOST row-major 3x3. */
int gs_keyframe_overlap(int32_t n_pts, const float* pts_world, int32_t n_keyframes, const float* w2c,
                        const float* h_intrinsics9, int32_t width, int32_t height, int32_t edge, uint32_t* counts,
                        gs_stream_t stream);

/* ---- Frame ingest (the pre-processing of a sensor frame, src/mapper/splatam/__init__.py:341-376) ----
 * The raw frame resized to n_out (1 or 2) resolutions -- the mapping and the densification resolution -- in ONE launch.  image: uint8
 * [height * width * 3], interleaved RGB; depth: fp32 [height * width]; level_value: fp32 [256]; all DEVICE.  h_sizes: HOST, n_out pairs
 * (W_k, H_k).  Output k: color_k fp32 [3 * H_k * W_k], PLANAR, and depth_k fp32 [H_k * W_k], DEVICE (color1 / depth1 are ignored when n_out
 * is 1).  No atomics, no scratch, nothing depends on scheduling: two calls on the same inputs give the same bits.
 *
 * Colour (cv2.resize(INTER_LINEAR)'s sampling, as activesplat_amd/frames.py resize_linear restates it), in fp64, EVERY operation rounded on its
 * own.  Per axis, destination sample d of n_dst from n_src:
 *   r = double(n_src) / double(n_dst);  c = (d + 0.5) * r - 0.5;  i0 = floor(c);  f = c - i0;  taps clamp(i0), clamp(i0 + 1) into [0, n_src - 1]
 * and per channel, with the taps a b (upper row) and c d (lower row):
 *   top = a * (1 - fx) + b * fx;  bot = c * (1 - fx) + d * fx;  o = top * (1 - fy) + bot * fy;  level = clamp(floor(o + 0.5), 0, 255)
 * The value written is level_value[level].  The table is an argument, not level / 255.0f, so that the caller decides what a grey level is: the
 * binding fills it with the operations its host path applies (uint8 -> float, / 255, by torch on the same device) and the loop receives the bits
 * it would have received from there.  Equal sizes reproduce the source levels (f = 0 on both axes).
 * UNPINNED: the product build of the kernel's file allows FMA contraction; the kernel switches it off for itself.  The host-emulated test
 * build compiles every file without contraction, so no test can tell whether the product kernel contracts: a contraction could move a level
 * only where o + 0.5 lies within an ulp of an integer.  It is right by construction (the pragma), not by a test.
 * cv2 itself was NOT run against this rule; its uint8 path quantises the interpolation weights to 11 bits, which can move a result by one level.
 *
 * Depth (cv2.resize(INTER_NEAREST); frames.py resize_nearest): source row min((int)floor(double(y) * (double(height) / double(H_k))),
 * height - 1), likewise for the column, in fp64 -- NOT (y * height) / H_k in integers, which picks another row for some size pairs (2 -> 98
 * is one).  The 32-bit pattern is copied: NaN payloads, +-inf, -0, negatives and denormals pass through unchanged.
 *
 * Supported: 1 <= width, height, W_k, H_k <= 16384, n_out in {1, 2}; anything else, or a null pointer, is GS_EINVAL before any launch. */
int gs_frame_ingest(int32_t width, int32_t height, const uint8_t* image, const float* depth, const float* level_value, int32_t n_out,
                    const int32_t* h_sizes, float* color0, float* depth0, float* color1, float* depth1, gs_stream_t stream);

/* ---- Mesh RGB-D sensor (the frame the reference takes from Habitat-sim: colour, planar depth, src/dataloader/dataloader.py:168-235) ----
 * A vertex-coloured triangle mesh rendered to the frame gs_frame_ingest takes, by ray casting on the compute path (no graphics pipeline).
 * vertices fp32 [num_vertices, 3] world frame, triangles int32 [num_triangles, 3], vertex_colors uint8 [num_vertices, 3]: DEVICE.
 * h_intrinsics4 = HOST {fx, fy, cx, cy}; h_w2c12 = HOST row-major 3x4 [R|t] world-to-camera, the inverse of the c2w gs_depth_cloud takes
 * (camera: x right, y down, z forward).  THE RULE, all fp32:
 *   camera-frame vertex   p = R v + t
 *   ray of pixel (x, y)   d = ((x - cx) / fx, (y - cy) / fy, 1): d.z = 1, so a hit's ray parameter IS its planar depth (what Habitat's depth
 *                         sensor returns)
 *   edge function         for vertex indices i < j: E(i, j) = d . (p_i x p_j); for i > j: E(i, j) = -E(j, i), evaluated with the lower index
 *                         first and negated.  A shared edge then gives both of its triangles the same magnitude from the same operands, which
 *                         keeps a closed mesh watertight in fp32.  (The kernels form p_i x p_j once per triangle with separately rounded
 *                         operations and negate the vector; negation is exact and passes unchanged through the two fused multiply-adds
 *                         fma(dx, n.x, fma(dy, n.y, n.z)) that evaluate every edge.)
 *   hit test              triangle (a, b, c): U = E(b, c), V = E(c, a), W = E(a, b), S = (U + V) + W.  Hit iff (U, V, W all >= 0 or all <= 0)
 *                         and S != 0 and z = (U z_a + V z_b + W z_c) / S is finite and z >= near.  TWO-SIDED: no back-face culling (whether
 *                         Habitat's renderer culls back faces was not established).  A degenerate triangle has S = 0 and never hits; so does one
 *                         with an index outside 0 .. num_vertices - 1, which is dropped without being read.
 *   winner                the smallest z; among equal z the lowest triangle index: the image does not depend on the order of any list
 *   outputs               depth fp32 [height * width], 0 where nothing is hit; tri_id int32 [height * width], -1 where nothing is hit; color uint8
 *                         [height * width * 3] interleaved, clamp(floor((U C_a + V C_b + W C_c) / S + 0.5), 0, 255), 0 where nothing is hit.
 * Not modelled: sensor noise, a far plane; textures are gs_mesh_render_textured's (below), with what THEY leave unmodelled stated there.
 * Four launches on `stream`: per-triangle setup (edge vectors, a conservative rectangle of 16 x 16 tiles -- clipped against z = near where the
 * triangle crosses it -- and the tile counts), a scan over the tiles, the fill of the tile lists, and one workgroup per tile that casts its 256
 * rays.  Integer atomics only; nothing a workgroup reads was written by another workgroup of the same launch; two calls on the same inputs give
 * the same bits.  The total length D of the tile lists depends on the data: the caller provides room for `capacity` entries;
 * d_counts[0] (DEVICE) receives D (0xffffffff when it does not fit 32 bits) and d_counts[1] the longest tile list.  When D > capacity nothing is
 * written to the lists and the three outputs are CLEARED (0, -1, 0): read d_counts[0] and call again with capacity >= D.
 * KNOWN LIMITS.  (1) Needle triangles.  A triangle is tested only by the tiles of its rectangle: the projection of its (clipped) vertices grown by
 * one pixel (by a further 1/1024 of the image where it crosses the near plane).  The hit test uses the fp32-rounded edge vectors; where two
 * edges meet at an angle well below about 1e-3 rad the two rounded edge lines can cross more than a pixel beyond the true vertex, and a pixel
 * there that a brute-force evaluation of the rule over all triangles would hit is not tested: the tip of such a needle can lose pixels.
 * Triangles with angles above that are covered with room to spare.  (2) Large images.  The scan over the tiles is ONE workgroup that walks them
 * 256 at a time (4 chunks at 512 x 512); at the largest permitted image, 16384 x 16384, that is 4096 serial chunks of about 18 barriers each,
 * i.e. milliseconds: correct, but not tuned for images of that size.
 * scratch: DEVICE, gs_mesh_render_layout(num_triangles, width, height, capacity).total_bytes bytes, 16-byte aligned; the offsets are published
 * for tests.  Refused with GS_EINVAL before any launch: a null pointer (the three mesh arrays may be null when num_triangles is 0), width or
 * height outside 1 .. 16384, num_triangles < 0, num_vertices < 0, near not positive and finite, an intrinsic that is not finite, fx or fy zero.
 * num_triangles == 0 is valid and clears the outputs. */
typedef struct GsMeshLayout {
    uint64_t total_bytes;
    uint64_t total;         /* uint64: D */
    uint64_t records;       /* num_triangles x 64 bytes: three (edge vector, z of the opposite vertex), then three packed colours and the index */
    uint64_t rects;         /* num_triangles x 2 uint32: tile rectangle x0 | x1 << 16, y0 | y1 << 16 (x0 > x1: no tile) */
    uint64_t tile_count;    /* (tiles + 1) uint32 */
    uint64_t tile_offset;   /* (tiles + 1) uint32: exclusive offsets, [tiles] = D */
    uint64_t list;          /* capacity uint32: triangle indices, tile after tile */
} GsMeshLayout;
int gs_mesh_render_layout(int32_t num_triangles, int32_t width, int32_t height, uint32_t capacity, GsMeshLayout* layout);
int gs_mesh_render(int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles, const uint8_t* vertex_colors,
                   const float* h_intrinsics4, const float* h_w2c12, float near_z, int32_t width, int32_t height, void* scratch, uint32_t capacity,
                   float* depth, int32_t* tri_id, uint8_t* color, uint32_t* d_counts, gs_stream_t stream);

/* ---- Textures of the mesh sensor (the reference's scenes are Gibson / Matterport GLBs, config/datasets/gibson.json, whose colour lives in
 * texture images) ----
 * gs_mesh_render_textured is gs_mesh_render followed by ONE more launch that overwrites the colour of the hits whose triangle has a texture:
 * depth, tri_id and the colour of every other pixel are gs_mesh_render's bits.  gs_mesh_render itself is unchanged.
 * SCENE ADDITIONS.  uvs fp32 [num_vertices, 2] DEVICE, 8-byte aligned, glTF convention: origin top-left, v down, row = v * h, no flip.
 * tri_texture int32 [num_triangles] DEVICE: the texture of each triangle; -1, or any value outside 0 .. num_textures - 1, means "vertex
 * colour, as gs_mesh_render gives it" -- such a value is never used to index the table.  A texture pool: texture k has a level 0 of
 * width x height texels (1 .. 16384 each), wrap_s / wrap_t in {GS_WRAP_REPEAT 0, GS_WRAP_CLAMP 1, GS_WRAP_MIRROR 2} and
 * L = 1 + floor(log2(max(width, height))) levels; level l has max(1, width >> l) x max(1, height >> l) texels, so level L - 1 is ONE texel.
 * The pool is one DEVICE array of packed 32-bit RGBX words, one per texel (R in bits 0-7, G 8-15, B 16-23, X = 0), row-major, level after level,
 * texture after texture: a fetch is one dword load.  gs_texture_layout fills `levels` and `level_offset` (in texels) of every entry of a HOST
 * table and returns the pool's size; the caller writes level 0 of every texture into the pool and copies the table to the device.
 * MIP CHAIN (exact integers; gs_texture_build_mips, on the device, once per scene).  Level l + 1 texel (i, j), per channel:
 *   (t[2j][2i] + t[2j][i1] + t[j1][2i] + t[j1][i1] + 2) >> 2   with i1 = min(2i + 1, w_l - 1), j1 = min(2j + 1, h_l - 1), t = level l.
 * One launch per level index over all textures (not one per texture), one destination texel per thread, integer arithmetic only.
 * THE RULE per pixel (x, y) whose winner t = (a, b, c) has a texture, all fp32:
 *   q(x', y')   = (U uv_a + V uv_b + W uv_c) / ((U + V) + W), with U, V, W the winner's three edge functions at the ray of pixel (x', y'): the edge
 *                 vectors gs_mesh_render stored and the same two fused multiply-adds per edge, so that at (x, y) they are exactly the
 *                 barycentrics that decided the hit.  q is evaluated at (x, y), (x + 1, y) and (x, y + 1), ON THE WINNER'S PLANE: the two
 *                 neighbours are taken whether or not they hit the triangle (or anything), and also beyond the image edge.
 *   footprint     ex = (q(x + 1, y) - q(x, y)) o (width, height), ey likewise from (x, y + 1); rho = max(|ex|_2, |ey|_2)
 *   level         lambda = clamp(log2 rho, 0, L - 1); lambda = 0 when rho <= 1; lambda = L - 1 when rho is NaN or infinite
 *   level sample  at (u, v) = q(x, y), level l of w_l x h_l texels: s = u w_l - 0.5, i = floor(s), alpha = s - i; t = v h_l - 0.5, j = floor(t),
 *                 beta = t - j; the texels T[wrap(j), wrap(j + 1)][wrap(i), wrap(i + 1)]; columns first, then rows:
 *                   top = (1 - alpha) T[j][i] + alpha T[j][i+1];  bot = (1 - alpha) T[j+1][i] + alpha T[j+1][i+1];  (1 - beta) top + beta bot
 *   wrap over n   REPEAT: i mod n, non-negative.  CLAMP: clip to 0 .. n - 1.  MIRROR: m = i mod 2n (non-negative); m >= n -> 2n - 1 - m.
 *   safety        if a component of q(x, y) is not finite or exceeds 2^20 in magnitude the pixel takes the single texel of level L - 1: the
 *                 float -> integer conversion of floor(s) is then always defined (|s| < 2^35, converted to 64 bits)
 *   mix           l0 = floor(lambda), f = lambda - l0;  c = (1 - f) sample(l0) + f sample(min(l0 + 1, L - 1));  out = clamp(floor(c + 0.5), 0, 255)
 * TEXELS ARE USED AS STORED.  Not modelled: sRGB decoding (filtering happens in stored space), base-colour factors, vertex-colour modulation,
 * alpha, anisotropic filtering.  Nothing was run against Habitat-sim.
 * THE TEXTURE PASS: one workgroup per 16 x 16 pixels with the pixel-to-lane map of the render's last launch (an 8 x 8 quadrant per wavefront, so
 * that the texel fetches of a wavefront stay local).  A thread reads tri_id of its pixel, the winner's three edge records from the scratch the
 * render just wrote, its three vertex indices and uvs, eight texels, and stores three bytes.  No atomics; nothing is read that the same launch
 * writes; two calls on the same inputs give the same bits.  When D > capacity the outputs are cleared as by gs_mesh_render.
 * THE TABLE TWICE.  gs_texture_build_mips and gs_mesh_render_textured take the table as h_textures (HOST: checked before any launch, and it sizes
 * the mip launches) and as textures (DEVICE: what the kernels read).  The caller passes two copies of the same bytes; only the host copy
 * can be checked without waiting for the device.
 * Refused with GS_EINVAL before any launch, besides everything gs_mesh_render refuses: num_textures < 0; with num_textures > 0 a null uvs (or one
 * not 8-byte aligned), tri_texture, h_textures, textures or pool; a wrap mode outside 0 .. 2; a texture size outside 1 .. 16384; levels or
 * level offsets that are not gs_texture_layout's, or a pool_texels that is not its total.  With num_textures == 0 everything texture-related
 * may be null and the call equals gs_mesh_render.  uvs and tri_texture may also be null when num_triangles is 0. */
#define GS_WRAP_REPEAT 0
#define GS_WRAP_CLAMP 1
#define GS_WRAP_MIRROR 2
#define GS_TEXTURE_MAX_LEVELS 15     /* 1 + log2(16384) */
typedef struct GsTextureDesc {
    int32_t width, height;           /* level 0: 1 .. 16384 */
    int32_t wrap_s, wrap_t;          /* GS_WRAP_* along u (columns) and v (rows) */
    int32_t levels;                  /* written by gs_texture_layout: 1 + floor(log2(max(width, height))) */
    int32_t reserved;                /* 0 */
    uint64_t level_offset[GS_TEXTURE_MAX_LEVELS];   /* written by gs_texture_layout: first texel of level l in the pool; 0 beyond the last level */
} GsTextureDesc;
int gs_texture_layout(int32_t num_textures, GsTextureDesc* h_textures, uint64_t* pool_texels);
int gs_texture_build_mips(int32_t num_textures, const GsTextureDesc* h_textures, const GsTextureDesc* textures, uint32_t* pool, uint64_t pool_texels,
                          gs_stream_t stream);
int gs_mesh_render_textured(int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles, const uint8_t* vertex_colors,
                            const float* h_intrinsics4, const float* h_w2c12, float near_z, int32_t width, int32_t height, void* scratch,
                            uint32_t capacity, float* depth, int32_t* tri_id, uint8_t* color, uint32_t* d_counts, const float* uvs,
                            const int32_t* tri_texture, int32_t num_textures, const GsTextureDesc* h_textures, const GsTextureDesc* textures,
                            const uint32_t* pool, uint64_t pool_texels, gs_stream_t stream);

/* ---- Navigable grid of a storey from the mesh (the reference moves its agent with Habitat-sim's sim.step on a navmesh,
 * src/dataloader/dataloader.py:237-272) ----
 * A top-down, CONSERVATIVE classification of grid_height x grid_width square cells.  This is a grid rule of this project, NOT Recast and NOT
 * Habitat's navmesh; it was not run against Habitat-sim.  Stairs are not modelled: one floor height per call.
 * vertices fp32 [num_vertices, 3] in the simulator's world frame, y UP, triangles int32 [num_triangles, 3]: DEVICE (MeshScene's arrays).
 * x0, z0, cell, floor_y, max_climb, agent_height: HOST scalars, fp64.
 * THE GRID.  Cell (r, c), 0 <= r < grid_height, 0 <= c < grid_width, is the CLOSED square
 *   [xa, xb] x [za, zb] = [x0 + c * cell, x0 + (c + 1) * cell] x [z0 + r * cell, z0 + (r + 1) * cell],  the borders computed in fp64 exactly
 * as written (one product, one sum).
 * THE RULE.  All arithmetic is fp64, every operation rounded on its own (no fused multiply-add), so that a numpy restatement gives the same bits.
 *   dropped     a triangle with a vertex index outside 0 .. num_vertices - 1 is dropped without being read; so is one with a non-finite vertex.
 *   pre-test    [Ylo, Yhi] = the y range of the triangle's own three vertices.  If that range sets neither bit (below), the triangle
 *               contributes nothing to any cell.  Decided first, per triangle.
 *   clipping    for every other triangle and every cell: the 3-D triangle (vertices widened to fp64) is clipped against the four half-spaces
 *               x >= xa, x <= xb, z >= za, z <= zb, in this order, by Sutherland-Hodgman: the edges (a, b) of the polygon are walked in order
 *               (the last edge closes it); a is emitted if it is inside; if exactly one of a, b is inside, p = a + t * (b - a) with
 *               t = (bound - a.k) / (b.k - a.k) is emitted (k the clipped coordinate; per coordinate one difference, one product, one sum), and
 *               the clipped coordinate of p is set to `bound` exactly.  "Inside" is the closed comparison.  An empty polygon contributes
 *               nothing.  A vertical triangle (zero-area projection) and a degenerate one need no special case.
 *   bits        [lo, hi] = the y range of the clipped polygon's vertices.
 *               bit 1 (obstacle) iff hi >  floor_y + max_climb  and  lo <  floor_y + agent_height
 *               bit 0 (floor)    iff hi >= floor_y - max_climb  and  lo <= floor_y + max_climb      (the three sums in fp64)
 *   output      grid uint8 [grid_height * grid_width], row r, column c: the OR of the bits over all triangles.  1 = navigable floor, 0 = void,
 *               2 and 3 = blocked.  The result depends on the order of no list; two calls on the same inputs give the same bytes.
 * Four launches on `stream`, gs_mesh_render's structure: per-triangle setup (a 48-byte record of the nine coordinates, the pre-test, a
 * conservative rectangle of 16 x 16-cell tiles around the xz bounding box, the tile counts), gs_mesh_render's scan and fill of the tile lists,
 * and one 256-thread workgroup per tile in which a thread owns one cell, keeps its byte in a register and stores it once; the records are
 * staged through LDS in chunks.  Integer atomics only, and only for the list fill.  The clip runs in registers (no scratch memory): each stage
 * hands a vertex to the next as it emits it, which gives the vertices, and the operands of every interpolation, of the formulation above.
 * Shortcuts taken, each of which only skips a (triangle, cell) pair whose polygon the rule makes empty: the tile rectangle, and a per-cell
 * rejection by the triangle's exact x range and its z range padded by 2^-30 max|z| (the x stages can move an interpolated z by a few units of
 * 2^-52 max|z| beyond the triangle's own range).  A cell whose bits are both set skips the remaining triangles.  No other shortcut: in
 * particular no "cell inside the triangle" path that evaluates the plane at the corners, which is different arithmetic.
 * CAPACITY, as gs_mesh_render: d_counts[0] (DEVICE) receives the total length D of the tile lists (0xffffffff when it does not fit 32 bits),
 * d_counts[1] the longest list.  When D > capacity nothing is written to the lists and the grid is CLEARED (0): read d_counts[0] and call
 * again with capacity >= D.  The scan over the tiles is one workgroup (gs_mesh_render's known limit (2)).
 * scratch: DEVICE, gs_mesh_navgrid_layout(num_triangles, grid_width, grid_height, capacity).total_bytes bytes, 16-byte aligned; the offsets
 * are published for tests in a GsMeshLayout whose records are 48 bytes here (nine fp32 coordinates, three unused floats).
 * Refused with GS_EINVAL before any launch: a null pointer (the two mesh arrays may be null when num_triangles is 0, which is valid and clears
 * the grid), grid_width or grid_height outside 1 .. 16384, num_triangles < 0, num_vertices < 0, cell not positive and finite, a non-finite
 * scalar, max_climb < 0, agent_height <= max_climb. */
int gs_mesh_navgrid_layout(int32_t num_triangles, int32_t grid_width, int32_t grid_height, uint32_t capacity, GsMeshLayout* layout);
int gs_mesh_navgrid(int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles, double x0, double z0, double cell,
                    double floor_y, double max_climb, double agent_height, int32_t grid_width, int32_t grid_height, void* scratch, uint32_t capacity,
                    uint8_t* grid, uint32_t* d_counts, gs_stream_t stream);

/* ---- Completion / accuracy judge (ActiveSplat's own figure: scripts/judges/eval_actions.py:33-40,139-152) ----
 * Per frame the reference back-projects the sensor depth (rgbd_to_pointcloud, src/utils/gui_utils.py:96-125, called with depth scale 1000 and
 * depth max inf), builds a KD-tree over that cloud and queries it with 200 000 mesh samples, builds one over the samples and queries it with
 * the cloud, keeps two running minima per sample (starting at 1 and at inf) and writes a row of six means.  The three calls below are those
 * steps on the device; none of them waits for the host, none uses atomics, and two calls on the same inputs give the same bits.
 *
 * gs_depth_cloud: depth [height * width] fp32 metres, DEVICE; h_intrinsics4 = HOST {fx, fy, cx, cy}; h_c2w12 = HOST row-major 3x4
 * camera-to-world.  Pixel i = v * width + u, all in fp32:
 *   q = truncf(depth * 1000.0f)                  (the uint16 millimetre image the reference hands to Open3D)
 *   valid[i] = q >= 1 && q <= 65535              (0, negative and NaN are dropped; so is q > 65535, where the reference's uint16 cast would wrap:
 *                                                 dropping is THIS build's choice)
 *   z = q / 1000.0f;  x = (u - cx) * z / fx;  y = (v - cy) * z / fy;  points[i] = R (x, y, z) + t
 * points fp32 [height * width, 3] (0, 0, 0 where invalid), valid uint8 [height * width]; no compaction.  This restates what Open3D's
 * create_from_rgbd_image documents; it was NOT run against Open3D.
 *
 * gs_cloud_nearest: for every query point the squared distance to the nearest of the n_points streamed points, exact brute force in the
 * difference form (qx - px)^2 + (qy - py)^2 + (qz - pz)^2, fp32 (not |q|^2 + |p|^2 - 2 q.p, which cancels at room coordinates).  query
 * [n_query, 3], points [n_points, 3] fp32 DEVICE; query_valid / points_valid: uint8 per row, nullable (null = all valid).  An invalid point
 * contributes nothing; an invalid query's out[] entry is left untouched.  A query with no valid point gets +inf.  flags: GS_NEAREST_ROOT writes
 * the distance instead of its square; GS_NEAREST_ACCUMULATE writes min(out[q], value) -- the running minimum of the judge.  The streamed set is
 * split over workgroups and the partial minima are combined by a second launch (a min is exact in any order); scratch: DEVICE,
 * gs_cloud_nearest_scratch_bytes(n_query, n_points) bytes, 4-byte aligned.  0 <= n_query, n_points <= 2^30.
 *
 * gs_completion_row: min_dist [n_samples] = the running minimum DISTANCES (inf where a sample has not been seen), acc_dist [n_acc] with the
 * optional acc_valid bytes = this frame's accuracy distances.  Writes six doubles at the DEVICE address row6, the reference's columns:
 *   0 mean of min(1, d)   1 share of min(1, d) < 0.05   2 mean of d (inf while a sample is unseen)   3 share of d < 0.05
 *   4 path_length as passed   5 mean of the valid accuracy distances (NaN when there is none: the reference would raise on an empty cloud)
 * The < 0.05 test is made on the fp32 distance widened to double against the double 0.05 (float32(0.05) is not below it).  Sums in fp64 in a
 * fixed order: every thread adds its elements in index order, a pairwise tree per workgroup, the same tree over the workgroups' records in a
 * second launch.  scratch: DEVICE, gs_completion_row_scratch_bytes() bytes, 8-byte aligned.  1 <= n_samples, 0 <= n_acc, both <= 2^30. */
#define GS_NEAREST_ACCUMULATE 1
#define GS_NEAREST_ROOT 2
int gs_depth_cloud(int32_t width, int32_t height, const float* depth, const float* h_intrinsics4, const float* h_c2w12, float* points,
                   uint8_t* valid, gs_stream_t stream);
uint64_t gs_cloud_nearest_scratch_bytes(int64_t n_query, int64_t n_points);
int gs_cloud_nearest(int64_t n_query, const float* query, const uint8_t* query_valid, int64_t n_points, const float* points,
                     const uint8_t* points_valid, int32_t flags, float* out, void* scratch, gs_stream_t stream);
uint64_t gs_completion_row_scratch_bytes(void);
int gs_completion_row(int64_t n_samples, const float* min_dist, int64_t n_acc, const float* acc_dist, const uint8_t* acc_valid,
                      double path_length, double* row6, void* scratch, gs_stream_t stream);

/* ---- Map-quality evaluation of one frame (report_progress, src/mapper/splatam/utils/eval_helpers.py:211-245, and eval, :464-508) ----
 * im / gt_im [3, height, width], depth / silhouette / gt_depth [height, width]: fp32, DEVICE, contiguous.  The reference's two masks are applied on
 * load: valid = gt_depth > 0, presence = silhouette > sil_thres (strict).  flags:
 *   GS_EVAL_SIL_MASK          image and depth differences are multiplied by presence (eval with mapping_iters == 0 and no new Gaussians;
 *                             report_progress(tracking=True))
 *   GS_EVAL_IMAGE_VALID_MASK  both images are multiplied by valid (eval does, report_progress does not)
 *   GS_EVAL_SSIM              column 3,  GS_EVAL_MS_SSIM  column 4 (a column whose flag is off is NaN)
 * Writes eight doubles at the DEVICE address row (8-byte aligned); with D = (depth - gt_depth) [presence], N = width * height:
 *   0 psnr           the MEAN of the three per-channel values 20 log10(1 / sqrt(mse_c)), mse_c = sum (im_c - gt_c)^2 [masks] / N
 *                    (calc_psnr(...).mean(), slam_external.py: not the PSNR of the mean error)
 *   1 depth_rmse     the reference's "Depth RMSE": sum sqrt(D^2) valid / sum valid.  This IS the mean absolute error -- the root is taken per
 *                    pixel -- and equals column 2 in every mode; it is kept because the reference writes both files (rmse.txt, l1.txt)
 *   2 depth_l1       sum |D| valid / sum valid
 *   3 ssim           the mean SSIM map of the masked pair with the mapping loss' window (calc_ssim, slam_external.py:66-97: 11 taps, sigma 1.5,
 *                    zero padding 5, C1 = 0.01^2, C2 = 0.03^2)
 *   4 ms_ssim        the five-scale MS-SSIM of the masked pair to the PUBLISHED definition of the package the reference imports (not installed
 *                    here, so this column is not pinned to it): the same window as a VALID convolution; cs = (2 s12 + C2) / (s1 + s2 + C2),
 *                    ssim = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1) cs; per channel the spatial means, clamped at 0; levels 0-3 contribute cs, level 4
 *                    ssim, with the powers 0.0448, 0.2856, 0.3001, 0.2363, 0.1333; the product, then the mean over the channels.  Between levels:
 *                    2 x 2 mean pooling with zero padding size % 2 on each axis, the padding counted (divisor 4), size n -> n / 2 + n % 2.
 *                    Defined for min(width, height) > 160
 *   5 valid_pixels   the count of gt_depth > 0
 *   6 depth_rmse_l2  sqrt(sum D^2 valid / sum valid): the root of the mean square.  NOT a reference quantity
 *   7 reserved, 0
 * Every term is formed in fp32 and added in fp64; no float atomics; every final sum is a fixed-order reduction (one record per workgroup, one
 * finishing workgroup), so two calls on the same inputs give the same bits.  Divisions are IEEE, as torch's: no valid pixel gives NaN in columns
 * 1, 2 and 6, identical images give +inf dB.  LPIPS is not provided.
 * gs_eval_frame_layout fills the layout for (width, height, flags): scratch bytes, the level sizes, and whether MS-SSIM is defined for the size.
 * scratch: DEVICE, total_bytes bytes, 8-byte aligned.  1 <= width, height <= 16384; GS_EVAL_MS_SSIM on a size where it is undefined, an unknown
 * flag or a null pointer is GS_EINVAL and nothing is launched. */
#define GS_EVAL_SIL_MASK 1
#define GS_EVAL_IMAGE_VALID_MASK 2
#define GS_EVAL_SSIM 4
#define GS_EVAL_MS_SSIM 8
typedef struct GsEvalLayout {
    uint64_t total_bytes;
    int32_t ms_ssim_defined;      /* min(width, height) > 160 */
    int32_t levels;               /* 5 with GS_EVAL_MS_SSIM, else 1 */
    int32_t level_width[5], level_height[5];
} GsEvalLayout;
int gs_eval_frame_layout(int32_t width, int32_t height, int32_t flags, GsEvalLayout* layout);
int gs_eval_frame(int32_t width, int32_t height, const float* im, const float* depth, const float* silhouette, const float* gt_im,
                  const float* gt_depth, float sil_thres, int32_t flags, double* row, void* scratch, gs_stream_t stream);

/* ---- TSDF fusion and surface extraction: from depth frames to an indexed triangle mesh ----
 * A NEW CAPABILITY: the reference has no counterpart (its family fuses rendered depth with Open3D, offline).  The arithmetic below is this
 * build's own and is pinned to restatements kept with the tests (tests/volume_cases.py), not to the reference.
 *
 * The volume: nx * ny * nz grid points, x fastest (point (i, j, k) at index (k * ny + j) * nx + i), DEVICE, fp32:
 *   tsdf [n] (a fresh volume holds 1), weight [n] (0), color [n, 3] (0).  Grid point (i, j, k) is the voxel centre
 *   origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_size, each coordinate formed as o + ((float)i + 0.5f) * voxel_size.
 *
 * gs_tsdf_integrate folds n_frames frames into the volume, in frame order.  depth [n_frames, height, width], frame_color [n_frames, 3, height, width]
 * (planar, the rasteriser's layout; nullable: the volume's colour is then neither read nor written and `color` may be null), silhouette
 * [n_frames, height, width] (nullable): fp32, DEVICE.  h_intrinsics4 = HOST {fx, fy, cx, cy}, shared by the frames; h_w2c12 = HOST n_frames row-major
 * 3x4 [R|t] world-to-camera.  Per grid point p and frame, all in fp32, every operation rounded on its own (no fused multiply-add):
 *   1. c = R p + t (each row as r0 * px + r1 * py + r2 * pz + t).  Skipped unless c.z > 0.
 *   2. u = fx * c.x / c.z + cx, v = fy * c.y / c.z + cy.  Pixel centres sit at integer coordinates (gs_depth_cloud's convention).  The pixel is
 *      (floor(u + 0.5), floor(v + 0.5)); skipped when outside the image.
 *   3. d = depth[pixel].  With a silhouette: skipped unless silhouette[pixel] > sil_thres, and d = depth / silhouette (the rasteriser's depth
 *      image is sum z alpha T, not normalised).  Skipped unless 0 < d <= depth_max (infinity: no limit).  A NaN is skipped.
 *   4. sdf = d - c.z.  Skipped when sdf < -trunc.  s = min(1, sdf / trunc).
 *   5. tsdf = (tsdf * w + s) / (w + 1); each colour channel likewise with the frame's colour at the pixel; then w = min(w + 1, max_weight).
 * One thread owns four consecutive grid points for the whole call and keeps their state in registers across the frames: the volume is read
 * and written once per call (16-byte accesses), and a batch gives the bits of the same frames integrated one call at a time.  No atomics; two
 * calls on the same inputs give the same bytes.  At most 16 frames per call (the poses travel in the kernel arguments); a host loops for more.
 * Refused with GS_EINVAL before any launch: a null pointer (color only with frame_color null); tsdf / weight / color not 16-byte aligned, an
 * image not 4-byte aligned; a dimension below 1 or nx * ny * nz >= 2^31; voxel_size, trunc, fx or fy not positive and finite; an origin, cx, cy
 * or pose entry that is not finite; max_weight below 1 or not finite; n_frames outside 0 .. 16; width or height outside 1 .. 16384 (the range of
 * gs_depth_cloud); depth_max not positive; a NaN sil_thres.
 *
 * Extraction is marching tetrahedra on Kuhn's split of every cell (a cell = eight neighbouring grid points, named by its lowest one): for each
 * permutation (a, b, c) of the axes, in lexicographic order, one tetrahedron with the corners 0 -> e_a -> e_a + e_b -> (1, 1, 1).  The split
 * is the same in every cell, so neighbours agree on the diagonals of their shared faces and the surface is watertight without a matching
 * pass.  The 16-case table of a tetrahedron is derived by the library (from which corners are inside and the geometry of a reference
 * tetrahedron), not typed in.
 *   validity     a grid point is valid when weight >= min_weight, inside when tsdf < 0.  A cell emits only when all eight corners are valid.
 *   vertices     live on edges.  A grid point owns seven edges, towards +x, +y, +z, +xy, +xz, +yz, +xyz (slots 0 .. 6).  An owned edge gets a
 *                vertex when its ends differ in sign and a valid cell contains it.  With a the value at the owner (the lower index), b at the
 *                other end: t = a / (a - b), position p_a + t * (p_b - p_a), colour c_a + t * (c_b - c_a), each operation rounded on its own.
 *                Every cell that touches the edge refers to that one vertex: the mesh is welded.
 *   triangles    with q0 .. q3 the corners of a tetrahedron in the order above: a lone corner q (the only one inside, or the only one outside)
 *                with the others r0 < r1 < r2 gives the triangle (q r0, q r1, q r2); two inside p0 < p1 against two outside o0 < o1 give the
 *                quad (p0 o0, p0 o1, p1 o1, p1 o0), split into its corners (0, 1, 2) and (0, 2, 3).  The last two corners of every triangle of a
 *                case change places where the right-hand normal would otherwise point towards the inside corners: the normal points from
 *                negative to positive tsdf, towards free space.  A triangle with a vertex at t == 0 has no area; it is KEPT, so that the
 *                topology stays a manifold.
 *   order        vertices in (grid point, slot) order, triangles in (cell, tetrahedron, triangle) order: exclusive scans, no atomics, the same
 *                bytes every run.
 * gs_tsdf_count writes the per-point edge masks, per-cell triangle counts and their scanned block sums into scratch and the two totals to the
 * DEVICE words d_counts[0] = vertices, d_counts[1] = triangles; the host copies those 8 bytes, allocates, and calls gs_tsdf_emit with the SAME
 * scratch, dimensions and tsdf.  gs_tsdf_emit writes vertices fp32 [V, 3], vertex_colors fp32 [V, 3] (only with color) and triangles int32
 * [T, 3]; nothing is written at or beyond max_vertices / max_triangles rows.  A volume with a dimension of 1, or without a valid cell, gives 0 and
 * 0.  scratch: DEVICE, gs_tsdf_extract_scratch_bytes(nx, ny, nz) bytes (0 for a shape that is refused), 16-byte aligned.
 * Refused with GS_EINVAL before any launch: a null pointer (color may be null; an output may be null when its maximum is 0), a misaligned
 * one, a dimension below 1, nx * ny * nz >= 2^31 or 7 * nx * ny * nz >= 2^31 (vertex indices are int32), a NaN min_weight, an origin or
 * voxel_size as above, a negative maximum. */
int gs_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* h_origin3, float voxel_size, float trunc, float max_weight, float* tsdf,
                      float* weight, float* color, int32_t n_frames, int32_t width, int32_t height, const float* depth, const float* frame_color,
                      const float* silhouette, const float* h_intrinsics4, const float* h_w2c12, float sil_thres, float depth_max, gs_stream_t stream);
uint64_t gs_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int gs_tsdf_count(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight, void* scratch, uint32_t* d_counts,
                  gs_stream_t stream);
int gs_tsdf_emit(int32_t nx, int32_t ny, int32_t nz, const float* h_origin3, float voxel_size, const float* tsdf, const float* color, void* scratch,
                 int32_t max_vertices, int32_t max_triangles, float* vertices, float* vertex_colors, int32_t* triangles, gs_stream_t stream);

/* Planner roadmap on the device (stats.hip): from the planner's top-down maps to candidate viewpoints and the paths to them.  A grid
 * formulation of the reference's host chain (src/planner/planner.py:111-370: contours, scipy.spatial.Voronoi of sampled contour points, networkx
 * Dijkstra) -- a medial axis of free space, candidate nodes on it, shortest paths along it -- in exact integers; NOT a bit-for-bit restatement
 * of that chain.  Maps are uint8 [H, W] DEVICE arrays (0 = clear, anything else = set), a pixel is (r, c) with linear index r * W + c, and every
 * output is the same bytes from run to run.  Supported: 1 <= H, W <= 4096.  scratch: DEVICE, gs_roadmap_scratch_bytes(H, W) bytes (0 for a shape
 * that is refused), 16-byte aligned; one scratch serves all the calls below, one after the other.  Refused with GS_EINVAL before any launch:
 * a null or misaligned pointer, a shape out of range, and what each call names.
 *
 * gs_traversable_map   free_map, unseen: gs_render_forward_topdown's free_map_binary and visible_map_binary (1 = never seen).
 *   1  m0 = free_map != 0 and unseen == 0;
 *   2  opening: the union of all open_size x open_size squares that lie wholly inside the image and inside m0 (the reference's 4 x 4 MORPH_OPEN);
 *   3  dilation: a pixel is set if any pixel of the dilate x dilate window centred on it, clipped to the image, is set (its 3 x 3 dilate);
 *   4  of the result, the 8-connected component that holds the agent's pixel (agent_r, agent_c) is kept;
 *   5  if that pixel is not set, trav is all 0 and bit 0 of *d_status is raised (OR-ed in: the caller clears the word).
 *   The reference's contour fill and approxPolyDP are deliberately replaced by the component rule of step 4.
 *   1 <= open_size <= 16; dilate odd, 1 <= dilate <= 15; the agent's pixel inside the image.
 *
 * gs_clearance_field   obstacles are the pixels with trav == 0 plus a one-pixel frame around the image (rows -1 and H, columns -1 and W).
 *   dist2 [H, W] int32: the squared distance to the nearest obstacle, 0 on obstacles.  feature [H, W, 2] int16: that obstacle (r, c); among
 *   equidistant obstacles the one with the smallest (r, c) in lexicographic order.  Two passes: per column the nearest obstacle above or below
 *   (above on a tie), then per row the minimum of (c - c')^2 + g(c')^2 over the columns' picks (the frame's columns included).
 *
 * gs_voronoi_roadmap   the integer medial axis.  For every pair of 4-adjacent pixels p, q with trav set and |f(p) - f(q)|^2 > gamma2 (f: feature):
 *   ap = |p + q - 2 f(p)|^2, aq = |p + q - 2 f(q)|^2; p is marked if aq <= ap, q is marked if ap <= aq (both on equality).  roadmap = marked
 *   and dist2 >= min_dist2 (the caller passes ceil(radius_px^2)).  min_dist2, gamma2 >= 0.
 *
 * gs_grid_geodesic     field [H, W] int32: the shortest path length from the seed over the 8-connected pixels of mask, a straight step weighing
 *   12 and a diagonal step 17; a diagonal step needs only its two end pixels in the mask.  Unreachable pixels (and pixels outside the mask)
 *   hold INT32_MAX.  The seed is (seed_r, seed_c), or the DEVICE pair d_seed_rc[0..1] when d_seed_rc is not null; a seed outside the image
 *   or outside the mask gives an all-unreachable field and raises bit 1 of *d_status.  The call repeats a relaxation launch (a workgroup
 *   relaxes a 32 x 32 tile plus halo to local convergence; no workgroup waits for another) while a changed word is set, reading 4 bytes per
 *   round (and 12 once, before the first): it WAITS for the stream.  *h_rounds (HOST): the number of rounds that changed something -- fewer than
 *   the mask has pixels, else GS_ECAPACITY.
 *
 * gs_roadmap_entry     d_entry4 (DEVICE int32[4]) = (r, c, field value, linear index) of the roadmap pixel with the smallest finite field value,
 *   the smallest index on a tie; (-1, -1, INT32_MAX, -1) when there is none.  Per-workgroup minima of the keys (field << 32 | index) go through
 *   scratch, one workgroup takes their minimum: no atomics.
 *
 * gs_roadmap_nodes     cells of cell x cell pixels anchored at (0, 0) (the last row and column of cells may be cut by the image).  Per cell the
 *   roadmap pixel with a finite field value and the largest dist2, the smallest index on a tie; the picks in row-major cell order (count, scan,
 *   emit: no atomics) as node_rc [K, 2], node_dist2 [K], node_field [K] int32, each with room for ceil(H / cell) * ceil(W / cell) rows;
 *   d_count[0] = K stays on the DEVICE.  1 <= cell <= 64.
 *
 * gs_trace_path        from the target (target_r, target_c) -- or the DEVICE pair d_target_rc -- step to a neighbour n in the mask with
 *   field[n] + w == field[current] (w = 12 or 17), trying (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1) in this order and taking the
 *   first that qualifies, until the field reads 0.  One wavefront walks; at most `capacity` pixels are written.  path_rc [capacity, 2] int32: the
 *   pixels from the target to the seed, both included; d_count2 (DEVICE int32[2]) = (pixels written, 0 done | 1 target outside the image or the
 *   mask, or unreachable | 2 capacity reached first | 3 no neighbour qualifies: not a field of this mask). */
uint64_t gs_roadmap_scratch_bytes(int32_t H, int32_t W);
int gs_traversable_map(int32_t H, int32_t W, const uint8_t* free_map, const uint8_t* unseen, int32_t agent_r, int32_t agent_c, int32_t open_size,
                       int32_t dilate, uint8_t* trav, void* scratch, uint32_t* d_status, gs_stream_t stream);
int gs_clearance_field(int32_t H, int32_t W, const uint8_t* trav, int32_t* dist2, int16_t* feature, void* scratch, gs_stream_t stream);
int gs_voronoi_roadmap(int32_t H, int32_t W, const uint8_t* trav, const int32_t* dist2, const int16_t* feature, int32_t min_dist2, int32_t gamma2,
                       uint8_t* roadmap, gs_stream_t stream);
int gs_grid_geodesic(int32_t H, int32_t W, const uint8_t* mask, int32_t seed_r, int32_t seed_c, const int32_t* d_seed_rc, int32_t* field,
                     void* scratch, uint32_t* d_status, int32_t* h_rounds, gs_stream_t stream);
int gs_roadmap_entry(int32_t H, int32_t W, const uint8_t* roadmap, const int32_t* field, int32_t* d_entry4, void* scratch, gs_stream_t stream);
int gs_roadmap_nodes(int32_t H, int32_t W, const uint8_t* roadmap, const int32_t* dist2, const int32_t* field, int32_t cell, int32_t* node_rc,
                     int32_t* node_dist2, int32_t* node_field, int32_t* d_count, void* scratch, gs_stream_t stream);
int gs_trace_path(int32_t H, int32_t W, const uint8_t* mask, const int32_t* field, int32_t target_r, int32_t target_c, const int32_t* d_target_rc,
                  int32_t capacity, int32_t* path_rc, int32_t* d_count2, gs_stream_t stream);

/* Roadmap subregions (stats.hip): what the reference's hierarchical target choice needs on top of the roadmap above -- the all-pairs path
 * lengths between the nodes, line tests on the clearance field, and the average-linkage clustering of src/planner/planner.py:530-574
 * (get_subregions) -- as three calls that only enqueue work: no host read, no wait.  Integers wherever the rule is integer, no float atomics,
 * the same bytes from run to run.  Refused with GS_EINVAL before any launch: a null or misaligned pointer, a shape or count out of range.
 * GS_MAX_NODES bounds the node count of gs_node_distances and gs_subregions (the clustering workgroup keeps its per-cluster caches in LDS and
 * 8 K^2 bytes of pair sums in scratch).
 *
 * gs_node_distances    D [K, K] int32: D[i][j] = the shortest path length from node i to node j over the 8-connected pixels of roadmap, with
 *   gs_grid_geodesic's weights (straight step 12, diagonal step 17, a diagonal step needs only its two end pixels): D[i][j] is exactly what
 *   gs_grid_geodesic seeded at node i holds at node j, so D is symmetric, D[i][i] = 0 and D[i][j] = INT32_MAX where no path exists; a node
 *   outside the image or off the roadmap has INT32_MAX in its whole row and column (its own diagonal entry included), as that field has.
 *   node_rc [K, 2] int32 (r, c).  The roadmap's pixels are listed in row-major order (count, scan, emit); one workgroup per seed node relaxes
 *   the list's distances in place until a sweep changes nothing and writes the K values at the node pixels.  While the list has at most 32768
 *   pixels the distances sit in LDS; beyond, workgroups share scratch arrays, as many as fit, and take the seeds in turns.  scratch: DEVICE,
 *   gs_node_distances_scratch_bytes(H, W) bytes (16 H W and some: it does not grow with K), 16-byte aligned.  0 <= K <= GS_MAX_NODES.
 *   gs_set_node_distance_path forces a path (GS_NODE_DISTANCES_*; LDS only where the list fits): a test knob, the results are the same.
 *
 * gs_segment_clearance clearance [n] int32: the minimum of dist2 over the pixels of the integer line of segment s = (r0, c0, r1, c1)
 *   (segments [n, 4] int32).  N = max(|r1 - r0|, |c1 - c0|); for i = 0..N the pixel is (r0 + rnd(i (r1 - r0), N), c0 + rnd(i (c1 - c0), N)) with
 *   rnd(a, N) = floor((2 a + N) / (2 N)) in exact integers (floor division also for negative a: a half rounds towards +infinity); N = 0: the
 *   single pixel.  A pixel outside the image counts as an obstacle: the minimum is 0 -- so a segment with an end point outside the image has
 *   clearance 0, whatever its coordinates.  A segment is "clear for radius rho" when its clearance >= ceil(rho^2).  One wavefront per
 *   segment, a minimum over its lanes; no atomics.  0 <= n <= 2^24.
 *
 * gs_subregions        average-linkage clustering of the K nodes in fp64, cut at `threshold` (the caller passes scope_m * px_per_m).
 *   C[i][j] = path_weight * (D[i][j] / 12) + coord_weight * |node_i - node_j| (pixels; two products and one sum, none fused; D is read
 *   above the diagonal, i < j, and taken as symmetric); where D is INT32_MAX, C = (the largest finite C, 0 without one) + 1 (planner.py:553-555).
 *   Every node starts as a cluster.  The distance of two clusters A, B is (the sum of C over their member pairs) / (|A| |B|); the sums are kept
 *   per cluster pair and added when clusters merge: sum(A u B, X) = sum(A, X) + sum(B, X).  Repeatedly the two clusters with the smallest
 *   distance are merged -- among equal distances the pair whose smallest members (a, b), a < b, are lexicographically smallest -- until the
 *   smallest distance exceeds threshold or one cluster is left.  For a reducible linkage such as this one that is
 *   fcluster(linkage(C, 'average'), threshold, 'distance').  labels [K] int32: clusters numbered 0, 1, .. by their smallest member;
 *   d_count[0] (DEVICE) = their number; heights [K - 1] fp64: the merge distances in merge order, +inf from the first merge not made.
 *   One workgroup merges; each cluster caches its nearest later cluster.  scratch: DEVICE, gs_subregions_scratch_bytes(K) bytes, 8-byte
 *   aligned.  0 <= K <= GS_MAX_NODES; weights finite and >= 0, threshold >= 0 (+inf: merge everything). */
#define GS_MAX_NODES 1024
#define GS_NODE_DISTANCES_AUTO 0
#define GS_NODE_DISTANCES_LDS 1
#define GS_NODE_DISTANCES_GLOBAL 2
int gs_set_node_distance_path(int32_t path);
uint64_t gs_node_distances_scratch_bytes(int32_t H, int32_t W);
int gs_node_distances(int32_t H, int32_t W, const uint8_t* roadmap, int32_t K, const int32_t* node_rc, int32_t* D, void* scratch, gs_stream_t stream);
int gs_segment_clearance(int32_t H, int32_t W, const int32_t* dist2, int32_t n, const int32_t* segments, int32_t* clearance, gs_stream_t stream);
uint64_t gs_subregions_scratch_bytes(int32_t K);
int gs_subregions(int32_t K, const int32_t* node_rc, const int32_t* D, double path_weight, double coord_weight, double threshold, int32_t* labels,
                  int32_t* d_count, double* heights, void* scratch, gs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
