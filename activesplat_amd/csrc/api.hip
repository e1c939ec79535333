// api.hip -- the C ABI of libgsplat_hip.so (declared in include/gsplat_hip.h).
// Plain pointers and sizes in, launches on the caller's stream out; no torch types, no hidden sync.
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "gs_common.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* a = "")
{
    snprintf(g_err, sizeof(g_err), fmt, a);
    return code;
}

// GS_OK, or the recorded GS_ELAUNCH failure "who: [what ]<the runtime's text>"
int launched(const char* who, const char* what, hipError_t e)
{
    if (e == hipSuccess) return GS_OK;
    snprintf(g_err, sizeof(g_err), "%s: %s%s%s", who, what, *what ? " " : "", hipGetErrorString(e));
    return GS_ELAUNCH;
}

// adam.hip and the Adam inside the per-Gaussian backward reinterpret these pointers as float4*
bool adam_aligned16(const void* p, const void* g, const void* m, const void* v)
{
    return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;
}

int fail_adam_alignment(const char* who, int tensor)
{
    snprintf(g_err, sizeof(g_err), "%s: tensor %d: param / grad / exp_avg / exp_avg_sq must be 16-byte aligned (the kernel makes 128-bit accesses)", who, tensor);
    return GS_EINVAL;
}

uint64_t align_up(uint64_t v, uint64_t a = 256) { return (v + a - 1) / a * a; }

// ---- optional per-stage timing with HIP events on the caller's stream (bench.py roofline leg) ----
enum Stage { ST_PREPROCESS = 0, ST_TILE_COUNT, ST_EMIT, ST_SORT, ST_RANGES, ST_TILE_SCATTER_SORT, ST_BLEND_FWD, ST_BLEND_BWD, ST_PREPROCESS_BWD, ST_ADAM, ST_COUNT };
const char* kStageNames[ST_COUNT] = {"preprocess_forward+scan", "tile_count+scan", "emit", "sort", "ranges",
                                     "tile_scatter+sort", "blend_forward", "blend_backward", "preprocess_backward", "adam"};
std::atomic<int> g_sort_path{GS_SORT_AUTO};          // (development knobs: atomics, read once per decision -- see the header's note on threads)
std::atomic<bool> g_segments_enabled{true};

int choose_path(int tiles, uint32_t max_tile_instances)
{
    // any list length a grid's y dimension can index in 2048-key blocks (runs beyond the LDS merge are merged pass by pass
    // through global memory); 0xffffffff = counts unknown (more tiles than the LDS histogram holds)
    const bool fits = tiles <= gs::kMaxLdsTiles && max_tile_instances <= 65535u * (uint32_t)gs::kSortChunk;
    if (g_sort_path == GS_SORT_RADIX) return GS_SORT_RADIX;
    return fits ? GS_SORT_TILE_LDS : GS_SORT_RADIX;
}
constexpr int kMaxPairs = 8192;
struct Prof {
    bool on = false;
    int n = 0;
    hipEvent_t ev[kMaxPairs][2];
    int stage[kMaxPairs];
    int created = 0;
} g_prof;

struct ScopedStage {
    int idx = -1;
    hipStream_t st;
    ScopedStage(int stage, hipStream_t s) : st(s)
    {
        if (!g_prof.on || g_prof.n >= kMaxPairs) return;
        idx = g_prof.n++;
        if (idx >= g_prof.created) { (void)hipEventCreate(&g_prof.ev[idx][0]); (void)hipEventCreate(&g_prof.ev[idx][1]); g_prof.created = idx + 1; }
        g_prof.stage[idx] = stage;
        (void)hipEventRecord(g_prof.ev[idx][0], st);
    }
    ~ScopedStage() { if (idx >= 0) (void)hipEventRecord(g_prof.ev[idx][1], st); }
};

int tile_bits(int tiles)
{
    int b = 1;
    while ((1 << b) < tiles) b++;
    return b;
}

int32_t tiles_across(int32_t pixels) { return (pixels + gs::kTile - 1) / gs::kTile; }
uint64_t tiles_of(int32_t width, int32_t height) { return (uint64_t)tiles_across(width) * tiles_across(height); }
// multi-view atlas: every view padded to whole tiles; V x (P rounded up to whole 256-row blocks) virtual Gaussians (one view: nothing padded)
int32_t atlas_view_stride(int32_t view_width, int32_t V) { return V > 1 ? tiles_across(view_width) * gs::kTile : view_width; }
int32_t blocks_of(int32_t P) { return (P + gs::kBlock - 1) / gs::kBlock; }
int32_t virtual_rows(int32_t P, int32_t V) { return V > 1 ? V * blocks_of(P) * gs::kBlock : P; }

bool make_cam(const GsCamera* c, gs::Cam& k)
{
    if (!c || c->image_width <= 0 || c->image_height <= 0 || !c->bg || !c->viewmatrix || !c->projmatrix) return false;
    if (!(c->tanfovx > 0.f) || !(c->tanfovy > 0.f)) return false;
    if (c->num_views < 0 || c->num_views > 64) return false;
    k.V = c->num_views > 1 ? c->num_views : 1;
    k.Wv = c->image_width; k.H = c->image_height;
    k.gxv = tiles_across(k.Wv);
    k.gx = k.V * k.gxv; k.gy = tiles_across(k.H);
    k.W = k.V * atlas_view_stride(k.Wv, k.V);
    k.nbv = 0;                                             // set by virtual_count()
    if (k.gx >= 65536 || k.gy >= 65536) return false;
    k.tanfovx = c->tanfovx; k.tanfovy = c->tanfovy;
    k.fx = (float)k.Wv / (2.0f * c->tanfovx); k.fy = (float)k.H / (2.0f * c->tanfovy);
    k.mod = c->scale_modifier;
    k.sh_degree = c->sh_degree; k.sh_coeffs = c->sh_coeffs;
    k.bg = c->bg; k.view = c->viewmatrix; k.proj = c->projmatrix; k.campos = c->campos;
    k.half = 0; k.split = 0;                               // decided by the blend launchers
    k.act = k.act_iso = k.act_accumulate = 0;
    return true;
}

// rows of the per-Gaussian state: P for one view; the atlas's virtual Gaussians
int32_t virtual_count(gs::Cam& k, int32_t P)
{
    k.nbv = blocks_of(P);
    return virtual_rows(P, k.V);
}

gs::GeomPtrs carve_geom(void* base, int32_t P, const gs::Cam& k)
{
    GsGeomLayout L;
    gs_geom_layout(P, k.W, k.H, &L);
    char* b = (char*)base;
    gs::GeomPtrs g;
    g.geom = (float4*)(b + L.geom); g.rect = (uint2*)(b + L.rect); g.tiles = (uint32_t*)(b + L.tiles_touched);
    g.offsets = (uint32_t*)(b + L.offsets); g.block_sums = (uint32_t*)(b + L.block_sums);
    g.clamped = (uint32_t*)(b + L.clamped);
    g.tile_total = (uint32_t*)(b + L.tile_total); g.tile_base = (uint32_t*)(b + L.tile_base);
    g.sh_jac = (float2*)(b + L.sh_jac);
    g.depth_bits = (uint32_t*)(b + L.depth_bits);
    g.vis_max = nullptr; g.vis_seen = nullptr;
    return g;
}

}  // namespace

extern "C" {

const char* gs_last_error(void) { return g_err; }
const char* gs_version(void) { return "activesplat_amd gsplat_hip 0.4 (gfx950)"; }
int32_t gs_abi_version(void) { return GS_ABI_VERSION; }

int gs_profile_enable(int32_t on)
{
    g_prof.on = on != 0;
    g_prof.n = 0;
    return GS_OK;
}

int32_t gs_profile_stage_count(void) { return ST_COUNT; }

const char* gs_profile_stage_name(int32_t stage) { return stage >= 0 && stage < ST_COUNT ? kStageNames[stage] : ""; }

int gs_profile_collect(float* ms_sum, int32_t* calls, int32_t n_stages)
{
    if (!ms_sum || !calls || n_stages < ST_COUNT) return fail(GS_EINVAL, "gs_profile_collect: bad argument");
    for (int i = 0; i < n_stages; i++) { ms_sum[i] = 0.f; calls[i] = 0; }
    for (int i = 0; i < g_prof.n; i++) {
        if (hipEventSynchronize(g_prof.ev[i][1]) != hipSuccess) return fail(GS_ELAUNCH, "gs_profile_collect: event sync failed");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof.ev[i][0], g_prof.ev[i][1]) != hipSuccess) return fail(GS_ELAUNCH, "gs_profile_collect: elapsed failed");
        ms_sum[g_prof.stage[i]] += ms; calls[g_prof.stage[i]]++;
    }
    g_prof.n = 0;
    return GS_OK;
}

int gs_set_sort_path(int32_t path)
{
    if (path < GS_SORT_AUTO || path > GS_SORT_RADIX) return fail(GS_EINVAL, "gs_set_sort_path: bad path");
    g_sort_path = path;
    return GS_OK;
}

int gs_set_half_quadrants(int32_t max_tiles)
{
    gs::g_half_quadrant_tiles = max_tiles < 0 ? 0 : max_tiles;
    return GS_OK;
}

int gs_set_backward_chain(int32_t pieces, int32_t min_tiles)
{
    if (pieces < 1 || pieces > gs::kChainPieces) return fail(GS_EINVAL, "gs_set_backward_chain: pieces out of range");
    gs::g_chain_pieces = pieces;
    gs::g_chain_min_tiles = min_tiles < 0 ? gs::kChainMinTiles : min_tiles;
    return GS_OK;
}

int gs_set_backward_chain_tickets(int32_t on)
{
    gs::g_chain_tickets = on != 0;
    return GS_OK;
}

int gs_set_backward_chain_polls(int32_t polls)
{
    gs::g_chain_polls = polls == -1 ? gs::kChainPollsDefault : polls;      // (below -1: every waiting piece gives up at once -- tests)
    return GS_OK;
}

int gs_set_forward_priority(int32_t mode, float param)
{
    if (mode > gs::kFwdPrioChunk) return fail(GS_EINVAL, "gs_set_forward_priority: mode out of range");
    if (mode == gs::kFwdPrioT && param >= 1.0f) return fail(GS_EINVAL, "gs_set_forward_priority: a transmittance threshold lies below 1");
    if (mode < 0) { mode = gs::kFwdPrioDefault; param = gs::kFwdPrioDefaultParam; }      // negative: what the library ships with
    gs::g_fwd_prio_param = param > 0.0f ? param : 0.0f;         // (0: the predictor's default, chosen at the launch)
    gs::g_fwd_prio = mode;
    return GS_OK;
}

int gs_async_status_word(uint32_t** host_word)
{
    // one host-mapped word per process (portable: every device can raise it); plain host reads see it once the raising kernel has ended
    static uint32_t* word = nullptr;
    static std::mutex mu;                               // (both hosts above the ABI may ask for it first, from different threads)
    std::lock_guard<std::mutex> lock(mu);
    if (!word) {
        void* h = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            return fail(GS_ELAUNCH, "gs_async_status_word: hipHostMalloc failed");
        }
        memset(h, 0, 64);
        void* d = nullptr;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); return fail(GS_ELAUNCH, "gs_async_status_word: no device view of the host word"); }
        // the sticky device-memory twin the optimiser kernels read (Cam::chain_fail).  Without it the library still works -- the step is then not
        // protected against a timed-out walk, as before round 6
        void* f = nullptr;
        if (hipMalloc(&f, 64) == hipSuccess && hipMemset(f, 0, 64) == hipSuccess && hipGetDevice(&gs::g_chain_fail_device) == hipSuccess) gs::g_chain_fail_dev = (uint32_t*)f;
        else (void)hipGetLastError();
        word = (uint32_t*)h;
        gs::g_async_status_dev = (uint32_t*)d;
    }
    if (host_word) *host_word = word;
    return GS_OK;
}

int gs_async_status_clear(void)
{
    // the host has seen and reported the event: optimiser steps run again.  Synchronous (the rare path): every launch enqueued so far has ended
    // when this returns, so no walker of an old launch can raise the word again behind the clear
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return fail(GS_ELAUNCH, "gs_async_status_clear: device synchronisation failed"); }
    if (gs::g_chain_fail_dev && hipMemset(gs::g_chain_fail_dev, 0, 4) != hipSuccess) { (void)hipGetLastError(); return fail(GS_ELAUNCH, "gs_async_status_clear: hipMemset failed"); }
    return GS_OK;
}

int gs_recorded_cut(uint32_t target, uint32_t* nearest, int32_t* level)
{
    const uint32_t pos = gs::cut_nearest(target);
    if (nearest) *nearest = pos;
    if (level) *level = pos ? gs::cut_level(pos) : -1;
    return GS_OK;
}

int gs_set_backward_segments(int32_t segments)
{
    if (segments < 1 || segments > gs::kFewSegmentsMax) return fail(GS_EINVAL, "gs_set_backward_segments: 1, 2 or 3");
    gs::g_few_segments = segments;
    return GS_OK;
}

int gs_set_forward_segments(int32_t on)
{
    g_segments_enabled = on != 0;
    return GS_OK;
}

int gs_atlas_layout(int32_t P, int32_t view_width, int32_t num_views, int32_t* virtual_P, int32_t* atlas_width, int32_t* view_stride)
{
    if (P < 0 || view_width <= 0 || num_views < 1 || num_views > 64) return fail(GS_EINVAL, "gs_atlas_layout: bad argument");
    const int32_t stride = atlas_view_stride(view_width, num_views);
    if (virtual_P) *virtual_P = virtual_rows(P, num_views);
    if (atlas_width) *atlas_width = num_views * stride;
    if (view_stride) *view_stride = stride;
    return GS_OK;
}

int gs_geom_layout(int32_t P, int32_t width, int32_t height, GsGeomLayout* out)
{
    if (!out || P < 0 || width <= 0 || height <= 0) return fail(GS_EINVAL, "gs_geom_layout: bad argument");
    const uint64_t n = (uint64_t)(P > 0 ? P : 1);
    const uint64_t nb = (n + gs::kBlock - 1) / gs::kBlock;
    const uint64_t tiles = tiles_of(width, height);
    const uint64_t rows = (n + 1023) / 1024;   // sized for the smallest binning chunk
    uint64_t o = 0;
    out->geom = o; o = align_up(o + n * GS_GEOM_FLOATS * 4);
    out->rect = o; o = align_up(o + n * 8);
    out->tiles_touched = o; o = align_up(o + n * 4);
    out->offsets = o; o = align_up(o + n * 4);
    out->block_sums = o; o = align_up(o + (nb + 1) * 4);
    out->clamped = o; o = align_up(o + n * 4);
    out->tile_total = o; o = align_up(o + tiles * 4);
    out->tile_base = o; o = align_up(o + (tiles <= (uint64_t)gs::kMaxLdsTiles ? rows * tiles * 4 : 4));
    out->sh_jac = o; o = align_up(o + n * gs::kShJacFloats * 4);
    out->depth_bits = o; o = align_up(o + n * 4);
    out->total_bytes = o;
    return GS_OK;
}

int gs_image_layout(int32_t width, int32_t height, GsImageLayout* out)
{
    if (!out || width <= 0 || height <= 0) return fail(GS_EINVAL, "gs_image_layout: bad argument");
    const uint64_t tiles = tiles_of(width, height);
    const uint64_t hw = (uint64_t)width * height;
    uint64_t o = 0;
    out->ranges = o; o = align_up(o + tiles * 8);
    out->final_T = o; o = align_up(o + hw * 4);
    out->n_contrib = o; o = align_up(o + hw * 4);
    // (recorded only for images of few tiles: every pixel's state at the recorded list positions the segmented backward resumes from)
    // (images of many tiles: the hand-over state of the chained backward walks lives at the same offset)
    out->split_state = o; o = align_up(o + (tiles <= (uint64_t)gs::kFewTiles ? ((uint64_t)gs::kCutLevels * 5 + 4) * hw + 4
                                             : (uint64_t)gs::chain_state_words(tiles)) * 4);
    out->total_bytes = o;
    return GS_OK;
}

int gs_bin_layout(int64_t D, uint32_t max_tile_instances, int32_t width, int32_t height, GsBinLayout* out)
{
    if (!out || D < 0 || width <= 0 || height <= 0) return fail(GS_EINVAL, "gs_bin_layout: bad argument");
    const int tiles = (int)tiles_of(width, height);
    const uint64_t n = (uint64_t)(D > 0 ? D : 1);
    memset(out, 0, sizeof(*out));
    out->path = (uint64_t)choose_path(tiles, max_tile_instances);
    uint64_t o = 0;
    if (out->path == GS_SORT_TILE_LDS) {
        out->pairs = o; o = align_up(o + n * 8);
        if (max_tile_instances > (uint32_t)gs::kSortCapMax) { out->pairs_alt = o; o = align_up(o + n * 8); }
    } else {
        out->keys_unsorted = o; o = align_up(o + n * 8);
        out->vals_unsorted = o; o = align_up(o + n * 4);
        out->keys_sorted = o; o = align_up(o + n * 8);
        out->sort_temp = o; o = align_up(o + gs::sort_temp_bytes(D, 32 + tile_bits(tiles)));
    }
    // few tiles with very long lists (the planner's 120 x 150 views of a large map): cut every list into segments that are
    // composited in parallel -- enough of them to fill the 5120 wavefront slots, each at least 1024 records long
    out->segments = 1;
    // (pass 1 walks the WHOLE list, the normal walk stops where T saturates: at 256 tiles x 11 k records the normal path is 1.8x
    // faster, at 80 tiles x 78 k the segmented one 4.7x, at the 240 tiles x 78 k of a three-view atlas 2.5x -- so: lists of at least
    // 8192 in at most 160 tiles, or of at least 32768 as long as the tiles alone cannot fill the wavefront slots)
    const bool few_tiles = tiles * 4 * 8 <= gs::kWaveSlots && max_tile_instances >= 8192;
    const bool long_lists = tiles * 4 * 2 <= gs::kWaveSlots && max_tile_instances >= 32768;
    if (g_segments_enabled && max_tile_instances != 0xffffffffu && (few_tiles || long_lists)) {
        uint64_t S = 3 * (uint64_t)gs::kWaveSlots / ((uint64_t)tiles * 4);      // 3x oversubscribed: segments differ in work (early stop);
                                                                                // measured on the 240-tile atlas: 1x 1.10, 2x 1.06, 3x 0.95, 4x 0.96, 6x 1.05 ms
        const uint64_t by_len = max_tile_instances / 1024;
        if (S > by_len) S = by_len;
        if (S > 32) S = 32;
        if (S >= 2) { out->segments = S; out->seg_T = o; o = align_up(o + (uint64_t)tiles * S * gs::kBlock * 4 + (uint64_t)tiles * 16); }
    }
    out->total_bytes = o;
    return GS_OK;
}

uint64_t gs_backward_scratch_bytes(int32_t P) { return align_up((uint64_t)(P > 0 ? P : 1) * gs::kGradStride * 4); }

// raw-parameter mode (Cam::act) is on for every pose source but POSE_NONE
static void set_input_activation(gs::Cam& k, const gs::PoseRequest& pose, int32_t isotropic, int32_t accumulate)
{
    // the frame transform of the kernels that take it from the camera block: the host's pose, or the world frame (CamBand: the view matrix is the
    // whole camera; CamDP: the kernels overwrite it with the device column)
    static const float world[7] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* p = pose.source == gs::POSE_HOST ? pose.pose7 : world;
    k.act = pose.source != gs::POSE_NONE;
    k.act_iso = k.act && isotropic != 0; k.act_accumulate = k.act && accumulate != 0;
    for (int c = 0; c < 4; c++) k.act_q[c] = p[c];
    for (int c = 0; c < 3; c++) k.act_t[c] = p[4 + c];
}

// the device-resident pose of the tracking entry points (gs::CamDP)
static bool dev_pose(const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, gs::DevPose& dp)
{
    if (!cam_unnorm_rots || !cam_trans || num_frames < 1 || time_idx < 0 || time_idx >= num_frames) return false;
    dp.q = cam_unnorm_rots + time_idx; dp.t = cam_trans + time_idx; dp.stride = num_frames;
    return true;
}

static gs::CamDP with_dev_pose(const gs::Cam& k, const gs::DevPose& dp)
{
    gs::CamDP kd;
    static_cast<gs::Cam&>(kd) = k;
    kd.dev_q = dp.q; kd.dev_t = dp.t; kd.stride = dp.stride;
    return kd;
}

// one per-Gaussian forward, as its entry point describes it (what an entry point does not have stays zero)
struct ForwardCall {
    int32_t P;
    gs::GaussianInputs in;
    gs::PoseRequest pose;
    int32_t isotropic;
    float* max_2D_radius; uint8_t* seen;        // raw-parameter mode: the mapper's visibility statistics
    int32_t* radii;
    void* geom_state; void* image_state;
    uint32_t* d_counts; uint32_t* h_counts;
    int32_t want_backward;
};

static int preprocess_forward_impl(const GsCamera* cam, const ForwardCall& c, gs_stream_t stream)
{
    const gs::GaussianInputs& in = c.in;
    const int32_t P = c.P;
    gs::Cam k;
    if (!make_cam(cam, k)) return fail(GS_EINVAL, "gs_preprocess_forward: invalid camera settings");
    set_input_activation(k, c.pose, c.isotropic, 0);
    if (k.act && k.V != 1) return fail(GS_EINVAL, "gs_preprocess_forward_raw: one view only");
    if (k.act && (in.cov3D || (in.shs && k.sh_coeffs != 16)))
        return fail(GS_EINVAL, "gs_preprocess_forward_raw: scale / rotation parameters with colours or 16-coefficient SH rows only");
    if (P < 0 || !c.geom_state || !c.image_state || !c.d_counts) return fail(GS_EINVAL, "gs_preprocess_forward: null state pointer");
    if (P > 0 && (!in.means3D || !in.opac || !c.radii)) return fail(GS_EINVAL, "gs_preprocess_forward: null input pointer");
    if ((in.shs == nullptr) == (in.colors == nullptr) && P > 0)
        return fail(GS_EINVAL, "Please provide excatly one of either SHs or precomputed colors!");
    const bool have_sr = in.scales != nullptr && in.rots != nullptr;
    if (P > 0 && (have_sr == (in.cov3D != nullptr) || ((in.scales != nullptr) != (in.rots != nullptr))))
        return fail(GS_EINVAL, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (in.shs && (k.sh_degree < 0 || k.sh_degree > 3 || k.sh_coeffs < (k.sh_degree + 1) * (k.sh_degree + 1) || k.sh_coeffs > 16 || !k.campos))
        return fail(GS_EINVAL, "gs_preprocess_forward: sh_degree / sh_coeffs / campos inconsistent");
    hipStream_t st = (hipStream_t)stream;
    const int32_t Pv = virtual_count(k, P);
    gs::GeomPtrs gp = carve_geom(c.geom_state, Pv, k);
    if (!(c.want_backward && in.shs)) gp.sh_jac = nullptr;        // written only for SH inputs whose backward will follow
    gp.vis_max = k.act ? c.max_2D_radius : nullptr; gp.vis_seen = k.act ? c.seen : nullptr;
    GsImageLayout IL; gs_image_layout(k.W, k.H, &IL);
    uint2* ranges = (uint2*)((char*)c.image_state + IL.ranges);
    const int tiles = k.gx * k.gy;
    hipError_t e;
    {
        ScopedStage ps(ST_PREPROCESS, st);
        if (c.pose.source == gs::POSE_BAND) {   // the planner's top-down maps: raw parameters + height band
            gs::CamBand kb;
            static_cast<gs::Cam&>(kb) = k;
            kb.band_upper = c.pose.band_upper; kb.band_lower = c.pose.band_lower;
            e = gs::launch_preprocess_forward(kb, P, in, c.radii, gp, st);
        } else if (c.pose.source == gs::POSE_DEVICE)
            e = gs::launch_preprocess_forward(with_dev_pose(k, c.pose.dev), P, in, c.radii, gp, st);
        else
            e = gs::launch_preprocess_forward(k, P, in, c.radii, gp, st);
    }
    if (int rc = launched("gs_preprocess_forward", "", e)) return rc;
    bool mirrored = false;
    if (tiles <= gs::kMaxLdsTiles) {          // tile counting: ranges, D and the largest tile list
        // if h_counts is mapped pinned host memory the scan kernel stores the counters there itself (no copy engine hop)
        uint32_t* host_dev = nullptr;
        if (c.h_counts && hipHostGetDevicePointer((void**)&host_dev, c.h_counts, 0) != hipSuccess) { host_dev = nullptr; (void)hipGetLastError(); }
        mirrored = host_dev != nullptr;
        ScopedStage ps(ST_TILE_COUNT, st);
        e = gs::launch_tile_count(k, Pv, gp, gp.tile_total, gp.tile_base, ranges, c.d_counts, host_dev, st);
        if (int rc = launched("gs_preprocess_forward", "tile count", e)) return rc;
    } else {                                   // too many tiles for the LDS histogram: radix path, counts = {D, 2^32-1}
        e = gs::launch_scan_block_sums(Pv, gp, c.d_counts, st);
        if (int rc = launched("gs_preprocess_forward", "scan", e)) return rc;
        e = hipMemsetAsync(c.d_counts + 1, 0xff, sizeof(uint32_t), st);
        if (int rc = launched("gs_preprocess_forward", "memset", e)) return rc;
    }
    if (c.h_counts && !mirrored) {
        e = hipMemcpyAsync(c.h_counts, c.d_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (int rc = launched("gs_preprocess_forward", "D2H", e)) return rc;
    }
    return GS_OK;
}

int gs_preprocess_forward(const GsCamera* cam, int32_t P, const float* means3D, const float* shs,
                          const float* colors_precomp, const float* opacities, const float* scales,
                          const float* rotations, const float* cov3D_precomp, int32_t* radii, void* geom_state,
                          void* image_state, uint32_t* d_counts, uint32_t* h_counts, int32_t want_backward, gs_stream_t stream)
{
    ForwardCall c{};
    c.in.means3D = means3D; c.in.shs = shs; c.in.colors = colors_precomp; c.in.opac = opacities; c.in.scales = scales; c.in.rots = rotations;
    c.in.cov3D = cov3D_precomp; c.P = P;
    c.radii = radii; c.geom_state = geom_state; c.image_state = image_state; c.d_counts = d_counts; c.h_counts = h_counts; c.want_backward = want_backward;
    return preprocess_forward_impl(cam, c, stream);
}

int gs_preprocess_forward_raw(const GsCamera* cam, int32_t P, const float* means3D, const float* shs, const float* colors_precomp,
                              const float* logit_opacities, const float* log_scales, const float* unnorm_rotations,
                              const float* h_pose7, int32_t isotropic, float* max_2D_radius, uint8_t* seen, int32_t* radii, void* geom_state,
                              void* image_state, uint32_t* d_counts, uint32_t* h_counts, int32_t want_backward, gs_stream_t stream)
{
    if (!h_pose7) return fail(GS_EINVAL, "gs_preprocess_forward_raw: null pose");
    ForwardCall c{};
    c.in.means3D = means3D; c.in.shs = shs; c.in.colors = colors_precomp; c.in.opac = logit_opacities; c.in.scales = log_scales; c.in.rots = unnorm_rotations;
    c.P = P; c.pose.source = gs::POSE_HOST; c.pose.pose7 = h_pose7; c.isotropic = isotropic; c.max_2D_radius = max_2D_radius; c.seen = seen;
    c.radii = radii; c.geom_state = geom_state; c.image_state = image_state; c.d_counts = d_counts; c.h_counts = h_counts; c.want_backward = want_backward;
    return preprocess_forward_impl(cam, c, stream);
}

int gs_preprocess_forward_raw_dev(const GsCamera* cam, int32_t P, const float* means3D, const float* shs, const float* colors_precomp,
                                  const float* logit_opacities, const float* log_scales, const float* unnorm_rotations,
                                  const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, int32_t isotropic,
                                  float* max_2D_radius, uint8_t* seen, int32_t* radii, void* geom_state, void* image_state, uint32_t* d_counts,
                                  uint32_t* h_counts, int32_t want_backward, gs_stream_t stream)
{
    ForwardCall c{};
    c.pose.source = gs::POSE_DEVICE;
    if (!dev_pose(cam_unnorm_rots, cam_trans, num_frames, time_idx, c.pose.dev))
        return fail(GS_EINVAL, "gs_preprocess_forward_raw_dev: null pose columns or time index outside [0, num_frames)");
    if (P > 0 && (!log_scales || !unnorm_rotations)) return fail(GS_EINVAL, "gs_preprocess_forward_raw_dev: null scale / rotation parameters");
    c.in.means3D = means3D; c.in.shs = shs; c.in.colors = colors_precomp; c.in.opac = logit_opacities; c.in.scales = log_scales; c.in.rots = unnorm_rotations;
    c.P = P; c.isotropic = isotropic; c.max_2D_radius = max_2D_radius; c.seen = seen;
    c.radii = radii; c.geom_state = geom_state; c.image_state = image_state; c.d_counts = d_counts; c.h_counts = h_counts; c.want_backward = want_backward;
    return preprocess_forward_impl(cam, c, stream);
}

// binning + depth sort of one forward (the tile lists behind `ranges` / point_list): shared by gs_render_forward and gs_render_forward_topdown
static int bin_tile_lists(const char* who, const gs::Cam& k, int32_t P, int64_t D, uint32_t max_tile_instances, gs::GeomPtrs gp, uint2* ranges,
                          const GsBinLayout& BL, char* bb, uint32_t* point_list, hipStream_t st)
{
    hipError_t e;
    if (BL.path == GS_SORT_TILE_LDS) {
        if (D > 0) {          // ranges were written by gs_preprocess_forward
            ScopedStage ps(ST_TILE_SCATTER_SORT, st);
            e = gs::launch_tile_scatter_sort(k, P, gp, gp.tile_base, ranges, max_tile_instances,
                                             (unsigned long long*)(bb + BL.pairs), (unsigned long long*)(bb + BL.pairs_alt), point_list, (uint32_t)D, st);
            if (int rc = launched(who, "tile scatter/sort", e)) return rc;
        }
    } else {
        e = hipMemsetAsync(ranges, 0, (size_t)k.gx * k.gy * 8, st);
        if (int rc = launched(who, "memset", e)) return rc;
        if (k.gx * k.gy <= gs::kMaxLdsTiles) {   // per-Gaussian offsets were not needed before the sync: scan them now
            e = gs::launch_scan_block_sums(P, gp, gp.block_sums + (P + gs::kBlock - 1) / gs::kBlock, st);
            if (int rc = launched(who, "scan", e)) return rc;
        }
        if (D == 0) {   // nothing visible: the emitter still writes the (all-zero) scan offsets
            e = gs::launch_emit(k, P, gp, nullptr, nullptr, st);
            if (int rc = launched(who, "emit", e)) return rc;
        } else {
            uint64_t* ku = (uint64_t*)(bb + BL.keys_unsorted); uint32_t* vu = (uint32_t*)(bb + BL.vals_unsorted);
            uint64_t* ks = (uint64_t*)(bb + BL.keys_sorted);
            { ScopedStage ps(ST_EMIT, st); e = gs::launch_emit(k, P, gp, ku, vu, st); }
            if (int rc = launched(who, "emit", e)) return rc;
            const int end_bit = 32 + tile_bits(k.gx * k.gy);
            {
                ScopedStage ps(ST_SORT, st);
                e = gs::sort_pairs(bb + BL.sort_temp, (size_t)(BL.total_bytes - BL.sort_temp), ku, ks, vu, point_list, D, end_bit, st);
            }
            if (int rc = launched(who, "sort", e)) return rc;
            { ScopedStage ps(ST_RANGES, st); e = gs::launch_ranges(D, ks, ranges, st); }
            if (int rc = launched(who, "ranges", e)) return rc;
        }
    }
    return GS_OK;
}

int gs_render_forward(const GsCamera* cam, int32_t P, int64_t D, uint32_t max_tile_instances, void* geom_state,
                      void* bin_state, uint32_t* point_list, void* image_state, float* out_color, float* out_depth,
                      float* out_opacity, float* out_depth_sq, void* backward_scratch, gs_stream_t stream)
{
    gs::Cam k;
    if (!make_cam(cam, k)) return fail(GS_EINVAL, "gs_render_forward: invalid camera settings");
    if (P < 0 || D < 0 || !geom_state || !image_state || !out_color || !out_depth || !out_opacity)
        return fail(GS_EINVAL, "gs_render_forward: null pointer");
    if (D > 0 && (!bin_state || !point_list)) return fail(GS_EINVAL, "gs_render_forward: null binning workspace");
    if (D >= (int64_t)1 << 32) return fail(GS_ECAPACITY, "gs_render_forward: more than 2^32 tile instances");
    hipStream_t st = (hipStream_t)stream;
    const int32_t Pin = P;
    P = virtual_count(k, Pin);                             // every stage below works on the virtual Gaussians of the atlas
    gs::GeomPtrs gp = carve_geom(geom_state, P, k);
    GsImageLayout IL; gs_image_layout(k.W, k.H, &IL);
    char* ib = (char*)image_state;
    uint2* ranges = (uint2*)(ib + IL.ranges);
    GsBinLayout BL; gs_bin_layout(D, max_tile_instances, k.W, k.H, &BL);
    char* bb = (char*)bin_state;
    if (int rc = bin_tile_lists("gs_render_forward", k, P, D, max_tile_instances, gp, ranges, BL, bb, point_list, st)) return rc;
    ScopedStage ps(ST_BLEND_FWD, st);
    return launched("gs_render_forward", "blend", gs::launch_blend_forward(k, ranges, point_list, gp.geom, out_color, out_depth, out_opacity,
                    (float*)(ib + IL.final_T), (uint32_t*)(ib + IL.n_contrib), out_depth_sq, BL.path == GS_SORT_TILE_LDS ? (uint32_t)D : 0xffffffffu,
                    (int)BL.segments, BL.segments > 1 ? (float*)(bb + BL.seg_T) : nullptr, (float*)(ib + IL.split_state), (uint32_t)P,
                    (float*)backward_scratch, st));
}

int gs_preprocess_forward_topdown(const GsCamera* cam, int32_t P, const float* means3D, const float* colors_precomp, const float* logit_opacities,
                                  const float* log_scales, const float* unnorm_rotations, int32_t isotropic, float band_upper, float band_lower,
                                  int32_t* radii, void* geom_state, void* image_state, uint32_t* d_counts, uint32_t* h_counts, gs_stream_t stream)
{
    if (cam && cam->num_views > 1) return fail(GS_EINVAL, "gs_preprocess_forward_topdown: one view only");
    if (P > 0 && (!colors_precomp || !log_scales || !unnorm_rotations))
        return fail(GS_EINVAL, "gs_preprocess_forward_topdown: null colour / scale / rotation parameters");
    if (band_upper != band_upper || band_lower != band_lower) return fail(GS_EINVAL, "gs_preprocess_forward_topdown: NaN height band");
    ForwardCall c{};
    c.in.means3D = means3D; c.in.colors = colors_precomp; c.in.opac = logit_opacities; c.in.scales = log_scales; c.in.rots = unnorm_rotations;
    c.P = P; c.pose.source = gs::POSE_BAND; c.pose.band_upper = band_upper; c.pose.band_lower = band_lower; c.isotropic = isotropic;
    c.radii = radii; c.geom_state = geom_state; c.image_state = image_state; c.d_counts = d_counts; c.h_counts = h_counts;
    return preprocess_forward_impl(cam, c, stream);
}

int gs_render_forward_topdown(const GsCamera* cam, int32_t P, int64_t D, uint32_t max_tile_instances, void* geom_state, void* bin_state,
                              uint32_t* point_list, void* image_state, float* free_opacity, uint8_t* free_map_binary, uint8_t* visible_rgb,
                              uint8_t* visible_map_binary, gs_stream_t stream)
{
    gs::Cam k;
    if (!make_cam(cam, k)) return fail(GS_EINVAL, "gs_render_forward_topdown: invalid camera settings");
    if (k.V != 1) return fail(GS_EINVAL, "gs_render_forward_topdown: one view only");
    if (P < 0 || D < 0 || !geom_state || !image_state || !free_opacity || !free_map_binary || !visible_rgb || !visible_map_binary)
        return fail(GS_EINVAL, "gs_render_forward_topdown: null pointer");
    if (((uintptr_t)free_map_binary | (uintptr_t)visible_rgb | (uintptr_t)visible_map_binary | (uintptr_t)free_opacity) & 3)
        return fail(GS_EINVAL, "gs_render_forward_topdown: output maps must be 4-byte aligned");
    if (D > 0 && (!bin_state || !point_list)) return fail(GS_EINVAL, "gs_render_forward_topdown: null binning workspace");
    if (D >= (int64_t)1 << 32) return fail(GS_ECAPACITY, "gs_render_forward_topdown: more than 2^32 tile instances");
    hipStream_t st = (hipStream_t)stream;
    virtual_count(k, P);
    gs::GeomPtrs gp = carve_geom(geom_state, P, k);
    GsImageLayout IL; gs_image_layout(k.W, k.H, &IL);
    uint2* ranges = (uint2*)((char*)image_state + IL.ranges);
    GsBinLayout BL; gs_bin_layout(D, max_tile_instances, k.W, k.H, &BL);
    if (int rc = bin_tile_lists("gs_render_forward_topdown", k, P, D, max_tile_instances, gp, ranges, BL, (char*)bin_state, point_list, st)) return rc;
    ScopedStage ps(ST_BLEND_FWD, st);
    return launched("gs_render_forward_topdown", "blend", gs::launch_blend_topdown(k, ranges, point_list, gp.geom, free_opacity, free_map_binary, visible_rgb,
                    visible_map_binary, BL.path == GS_SORT_TILE_LDS ? (uint32_t)D : 0xffffffffu, (uint32_t)P, st));
}

// one backward, as its entry point describes it (what an entry point does not have stays zero)
struct BackwardCall {
    int32_t P;
    int64_t D;
    gs::GaussianBackward g;      // in, out and radii from the entry point; the rest from render_backward_impl
    gs::PoseRequest pose;
    int32_t isotropic, accumulate;
    const void* geom_state; const uint32_t* point_list; const void* image_state;
    const float* dL_dcolor; const float* dL_ddepth;
    const float* dL_dopacity; const float* dL_ddepth_sq;      // the opt-in image gradients (GsImageGrads; the *_grads entry points only)
    void* scratch; int32_t scratch_zeroed, have_sh_jacobian;
    const GsAdamTensor* adam5;
};

static int render_backward_impl(const GsCamera* cam, const BackwardCall& c, gs_stream_t stream)
{
    gs::GaussianBackward g = c.g;
    const gs::GaussianInputs& in = g.in;
    const gs::GaussianGrads& out = g.out;
    const gs::PoseRequest& pose = c.pose;
    const int32_t P = c.P;
    const bool pose_only = pose.grad == gs::POSE_GRAD_ONLY;
    gs::Cam k;
    if (!make_cam(cam, k)) return fail(GS_EINVAL, "gs_render_backward: invalid camera settings");
    set_input_activation(k, pose, c.isotropic, pose_only ? 0 : c.accumulate);       // (pose only: no parameter gradient is written, nothing to add to)
    if (k.act && k.V != 1) return fail(GS_EINVAL, "gs_render_backward_raw: one view only");
    if (k.act && (!in.opac || in.cov3D || (in.shs && k.sh_coeffs != 16)))
        return fail(GS_EINVAL, "gs_render_backward_raw: scale / rotation parameters with colours or 16-coefficient SH rows only");
    if (k.V > 1) return fail(GS_EINVAL, "gs_render_backward: multi-view atlas renders are forward-only");
    if (P < 0 || c.D < 0 || !c.geom_state || !c.image_state || !c.dL_dcolor || !c.scratch)
        return fail(GS_EINVAL, "gs_render_backward: null pointer");
    if (pose.grad && (!k.act || c.adam5 || (!pose.dL_dpose7 && pose.source != gs::POSE_DEVICE) || !pose.pose_scratch))
        return fail(GS_EINVAL, "gs_render_backward_raw_pose: raw-parameter mode with a pose-gradient output and its scratch only");
    if (pose.source == gs::POSE_DEVICE && !pose_only) return fail(GS_EINVAL, "gs_render_backward_raw_pose_dev: the pose-only backward only");
    if ((c.dL_dopacity || c.dL_ddepth_sq) && (c.adam5 || pose.source == gs::POSE_DEVICE))
        return fail(GS_EINVAL, "gs_render_backward: opacity / depth_sq gradients have no optimiser-step or device-pose form");
    if (P == 0) {
        if (pose.grad && pose.dL_dpose7)
            return launched("gs_render_backward_raw_pose", "memset", hipMemsetAsync(pose.dL_dpose7, 0, 7 * sizeof(float), (hipStream_t)stream));
        return GS_OK;
    }
    gs::FusedAdam fa{};
    if (c.adam5) {
        // the optimiser step inside the per-Gaussian kernel: the five descriptors must describe the very tensors this call reads
        if (!k.act || c.accumulate) return fail(GS_EINVAL, "gs_render_backward_raw_adam: raw-parameter mode without accumulation only");
        if (!in.means3D || !g.radii || !out.dmeans2D || !in.scales || !in.rots || (in.shs == nullptr) == (in.colors == nullptr))
            return fail(GS_EINVAL, "gs_render_backward_raw_adam: null input/output pointer");
        if (in.shs && !c.have_sh_jacobian) return fail(GS_EINVAL, "gs_render_backward_raw_adam: SH rows need the forward's saved Jacobian (have_sh_jacobian = 1)");
        const float* par[5] = {in.means3D, in.opac, in.scales, in.rots, in.shs ? in.shs : in.colors};
        const int64_t width[5] = {3, 1, c.isotropic ? 1 : 3, 4, in.shs ? 48 : 3};
        for (int t = 0; t < 5; ++t) {
            const GsAdamTensor& a = c.adam5[t];
            if (a.param != par[t] || !a.exp_avg || !a.exp_avg_sq || a.step < 1 || a.n != width[t] * (int64_t)P)
                return fail(GS_EINVAL, "gs_render_backward_raw_adam: descriptor of %s does not describe the input tensor (param / moments / n / step)",
                            t == 0 ? "means3D" : t == 1 ? "logit_opacities" : t == 2 ? "log_scales" : t == 3 ? "unnorm_rotations" : "the colours");
            // the kernel reads and writes the rotation rows, and the SH rows, of parameter and moments as float4
            if (P > 0 && (t == 3 || (t == 4 && in.shs)) && !adam_aligned16(a.param, a.param, a.exp_avg, a.exp_avg_sq))
                return fail_adam_alignment("gs_render_backward_raw_adam", t);
            fa.p[t] = a.param; fa.m[t] = a.exp_avg; fa.v[t] = a.exp_avg_sq;
            fa.c[t] = gs::adam_coef(a.lr, a.beta1, a.beta2, a.eps, a.step);
        }
        fa.fail = gs::chain_fail_word();
        g.adam = &fa;
    } else if (pose_only) {
        // (tracking: no parameter gradient is formed; the colour / SH inputs are still read)
        if (!in.means3D || !g.radii || !out.dmeans2D || !in.scales || !in.rots || (in.shs == nullptr) == (in.colors == nullptr))
            return fail(GS_EINVAL, "gs_render_backward_raw_pose: null input/output pointer");
    } else {
        if (!in.means3D || !g.radii || !out.dmeans2D || !out.dmeans3D || !out.dopac)
            return fail(GS_EINVAL, "gs_render_backward: null input/output pointer");
        if (in.shs ? !out.dshs : !out.dcolors) return fail(GS_EINVAL, "gs_render_backward: missing colour gradient output");
        if (in.cov3D ? !out.dcov3D : (!in.scales || !in.rots || !out.dscales || !out.drots))
            return fail(GS_EINVAL, "gs_render_backward: missing covariance inputs/outputs");
    }
    hipStream_t st = (hipStream_t)stream;
    gs::GeomPtrs gp = carve_geom(const_cast<void*>(c.geom_state), P, k);
    GsImageLayout IL; gs_image_layout(k.W, k.H, &IL);
    const char* ib = (const char*)c.image_state;
    float* grad2d = (float*)c.scratch;
    hipError_t e = c.scratch_zeroed ? hipSuccess : hipMemsetAsync(grad2d, 0, (size_t)P * gs::kGradStride * 4, st);
    if (int rc = launched("gs_render_backward", "memset", e)) return rc;
    if (c.D > 0) {
        ScopedStage ps(ST_BLEND_BWD, st);
        e = gs::launch_blend_backward(k, (const uint2*)(ib + IL.ranges), c.point_list, gp.geom,
                                      (const float*)(ib + IL.split_state),
                                      (const float*)(ib + IL.final_T),
                                      (const uint32_t*)(ib + IL.n_contrib), c.dL_dcolor, c.dL_ddepth, grad2d, st, c.dL_dopacity, c.dL_ddepth_sq);
        if (int rc = launched("gs_render_backward", "blend", e)) return rc;
    }
    g.clamped = gp.clamped; g.sh_jac = (in.shs && c.have_sh_jacobian) ? gp.sh_jac : nullptr; g.grad2d = grad2d;
    {
        ScopedStage ps(ST_PREPROCESS_BWD, st);
        if (pose.source == gs::POSE_DEVICE) e = gs::launch_preprocess_backward(with_dev_pose(k, pose.dev), P, g, pose, st);
        else e = gs::launch_preprocess_backward(k, P, g, pose, st);
    }
    if (int rc = launched("gs_render_backward", "preprocess", e)) return rc;
    const int64_t pose_rows = gs::pose_rows_count(P);
    if (pose.source == gs::POSE_DEVICE) {
        if (pose.dL_dpose7)
            return launched("gs_render_backward_raw_pose_dev", "pose reduction", gs::launch_pose_grad_finish_dev(pose_rows, pose.dev.q, pose.dev.stride,
                            (const float*)pose.pose_scratch, pose.dL_dpose7, st));
    } else if (pose.grad)
        return launched("gs_render_backward_raw_pose", "pose reduction", gs::launch_pose_grad_finish(pose_rows, pose.pose7, (const float*)pose.pose_scratch,
                        pose.dL_dpose7, st));
    return GS_OK;
}

int gs_render_backward_grads(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs,
                       const float* colors_precomp, const float* scales, const float* rotations,
                       const float* cov3D_precomp, const int32_t* radii, const void* geom_state,
                       const uint32_t* point_list, const void* image_state, const GsImageGrads* grads, float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacities, float* dL_dcolors_precomp,
                       float* dL_dshs, float* dL_dscales, float* dL_drotations, float* dL_dcov3D, void* scratch,
                       int32_t scratch_zeroed, int32_t have_sh_jacobian, gs_stream_t stream)
{
    if (!grads) return fail(GS_EINVAL, "gs_render_backward_grads: null image-gradient block");
    BackwardCall c{};
    c.P = P; c.D = D;
    c.g.in.means3D = means3D; c.g.in.shs = shs; c.g.in.colors = colors_precomp; c.g.in.scales = scales; c.g.in.rots = rotations; c.g.in.cov3D = cov3D_precomp;
    c.g.radii = radii; c.geom_state = geom_state; c.point_list = point_list; c.image_state = image_state; c.dL_dcolor = grads->dL_dcolor; c.dL_ddepth = grads->dL_ddepth; c.dL_dopacity = grads->dL_dopacity; c.dL_ddepth_sq = grads->dL_ddepth_sq;
    c.g.out.dmeans2D = dL_dmeans2D; c.g.out.dmeans3D = dL_dmeans3D; c.g.out.dopac = dL_dopacities; c.g.out.dcolors = dL_dcolors_precomp;
    c.g.out.dshs = dL_dshs; c.g.out.dscales = dL_dscales; c.g.out.drots = dL_drotations; c.g.out.dcov3D = dL_dcov3D;
    c.scratch = scratch; c.scratch_zeroed = scratch_zeroed; c.have_sh_jacobian = have_sh_jacobian;
    return render_backward_impl(cam, c, stream);
}

int gs_render_backward(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs,
                       const float* colors_precomp, const float* scales, const float* rotations,
                       const float* cov3D_precomp, const int32_t* radii, const void* geom_state,
                       const uint32_t* point_list, const void* image_state, const float* dL_dcolor,
                       const float* dL_ddepth, float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacities, float* dL_dcolors_precomp,
                       float* dL_dshs, float* dL_dscales, float* dL_drotations, float* dL_dcov3D, void* scratch,
                       int32_t scratch_zeroed, int32_t have_sh_jacobian, gs_stream_t stream)
{
    // (the two new images NULL: the kernels of every call before GsImageGrads)
    const GsImageGrads grads{dL_dcolor, dL_ddepth, nullptr, nullptr};
    return gs_render_backward_grads(cam, P, D, means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, radii, geom_state, point_list, image_state, &grads, dL_dmeans2D, dL_dmeans3D, dL_dopacities, dL_dcolors_precomp, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D, scratch, scratch_zeroed, have_sh_jacobian, stream);
}

int gs_render_backward_raw_grads(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                           const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                           int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                           const void* image_state, const GsImageGrads* grads, float* dL_dmeans2D, float* dL_dmeans3D,
                           float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                           float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, gs_stream_t stream)
{
    if (!grads) return fail(GS_EINVAL, "gs_render_backward_raw_grads: null image-gradient block");
    if (!h_pose7 || (P > 0 && !logit_opacities)) return fail(GS_EINVAL, "gs_render_backward_raw: null pose / opacity parameters");
    BackwardCall c{};
    c.g.in.means3D = means3D; c.g.in.shs = shs; c.g.in.colors = colors_precomp; c.g.in.opac = logit_opacities; c.g.in.scales = log_scales; c.g.in.rots = unnorm_rotations;
    c.P = P; c.D = D; c.pose.source = gs::POSE_HOST; c.pose.pose7 = h_pose7; c.isotropic = isotropic; c.accumulate = accumulate;
    c.g.radii = radii; c.geom_state = geom_state; c.point_list = point_list; c.image_state = image_state; c.dL_dcolor = grads->dL_dcolor; c.dL_ddepth = grads->dL_ddepth; c.dL_dopacity = grads->dL_dopacity; c.dL_ddepth_sq = grads->dL_ddepth_sq;
    c.g.out.dmeans2D = dL_dmeans2D; c.g.out.dmeans3D = dL_dmeans3D; c.g.out.dopac = dL_dlogit_opacities; c.g.out.dcolors = dL_dcolors_precomp;
    c.g.out.dshs = dL_dshs; c.g.out.dscales = dL_dlog_scales; c.g.out.drots = dL_dunnorm_rotations;
    c.scratch = scratch; c.scratch_zeroed = scratch_zeroed; c.have_sh_jacobian = have_sh_jacobian;
    return render_backward_impl(cam, c, stream);
}

int gs_render_backward_raw(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                           const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                           int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                           const void* image_state, const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, float* dL_dmeans3D,
                           float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                           float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, gs_stream_t stream)
{
    // (the two new images NULL: the kernels of every call before GsImageGrads)
    const GsImageGrads grads{dL_dcolor, dL_ddepth, nullptr, nullptr};
    return gs_render_backward_raw_grads(cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, accumulate, radii, geom_state, point_list, image_state, &grads, dL_dmeans2D, dL_dmeans3D, dL_dlogit_opacities, dL_dcolors_precomp, dL_dshs, dL_dlog_scales, dL_dunnorm_rotations, scratch, scratch_zeroed, have_sh_jacobian, stream);
}

uint64_t gs_pose_grad_scratch_bytes(int32_t P) { return align_up((uint64_t)gs::pose_rows_count(P > 0 ? P : 1) * gs::kPoseAcc * 4); }

int gs_render_backward_raw_pose_grads(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                                const void* image_state, const GsImageGrads* grads, float* dL_dmeans2D, float* dL_dmeans3D,
                                float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                                float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, int32_t pose_only,
                                float* dL_dpose7, void* pose_scratch, gs_stream_t stream)
{
    if (!grads) return fail(GS_EINVAL, "gs_render_backward_raw_pose_grads: null image-gradient block");
    if (!h_pose7 || (P > 0 && !logit_opacities)) return fail(GS_EINVAL, "gs_render_backward_raw_pose: null pose / opacity parameters");
    if (!dL_dpose7 || !pose_scratch) return fail(GS_EINVAL, "gs_render_backward_raw_pose: null pose-gradient output or scratch");
    BackwardCall c{};
    c.g.in.means3D = means3D; c.g.in.shs = shs; c.g.in.colors = colors_precomp; c.g.in.opac = logit_opacities; c.g.in.scales = log_scales; c.g.in.rots = unnorm_rotations;
    c.P = P; c.D = D; c.pose.source = gs::POSE_HOST; c.pose.pose7 = h_pose7; c.isotropic = isotropic; c.accumulate = accumulate;
    c.pose.grad = pose_only ? gs::POSE_GRAD_ONLY : gs::POSE_GRAD_WITH_PARAMS; c.pose.dL_dpose7 = dL_dpose7; c.pose.pose_scratch = pose_scratch;
    c.g.radii = radii; c.geom_state = geom_state; c.point_list = point_list; c.image_state = image_state; c.dL_dcolor = grads->dL_dcolor; c.dL_ddepth = grads->dL_ddepth; c.dL_dopacity = grads->dL_dopacity; c.dL_ddepth_sq = grads->dL_ddepth_sq;
    c.g.out.dmeans2D = dL_dmeans2D; c.g.out.dmeans3D = dL_dmeans3D; c.g.out.dopac = dL_dlogit_opacities; c.g.out.dcolors = dL_dcolors_precomp;
    c.g.out.dshs = dL_dshs; c.g.out.dscales = dL_dlog_scales; c.g.out.drots = dL_dunnorm_rotations;
    c.scratch = scratch; c.scratch_zeroed = scratch_zeroed; c.have_sh_jacobian = have_sh_jacobian;
    return render_backward_impl(cam, c, stream);
}

int gs_render_backward_raw_pose(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                int32_t isotropic, int32_t accumulate, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                                const void* image_state, const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, float* dL_dmeans3D,
                                float* dL_dlogit_opacities, float* dL_dcolors_precomp, float* dL_dshs, float* dL_dlog_scales,
                                float* dL_dunnorm_rotations, void* scratch, int32_t scratch_zeroed, int32_t have_sh_jacobian, int32_t pose_only,
                                float* dL_dpose7, void* pose_scratch, gs_stream_t stream)
{
    // (the two new images NULL: the kernels of every call before GsImageGrads)
    const GsImageGrads grads{dL_dcolor, dL_ddepth, nullptr, nullptr};
    return gs_render_backward_raw_pose_grads(cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, accumulate, radii, geom_state, point_list, image_state, &grads, dL_dmeans2D, dL_dmeans3D, dL_dlogit_opacities, dL_dcolors_precomp, dL_dshs, dL_dlog_scales, dL_dunnorm_rotations, scratch, scratch_zeroed, have_sh_jacobian, pose_only, dL_dpose7, pose_scratch, stream);
}

int gs_render_backward_raw_pose_dev(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                    const float* logit_opacities, const float* log_scales, const float* unnorm_rotations,
                                    const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, int32_t isotropic,
                                    const int32_t* radii, const void* geom_state, const uint32_t* point_list, const void* image_state,
                                    const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, void* scratch, int32_t scratch_zeroed,
                                    int32_t have_sh_jacobian, float* dL_dpose7, void* pose_scratch, gs_stream_t stream)
{
    BackwardCall c{};
    c.pose.source = gs::POSE_DEVICE;
    if (!dev_pose(cam_unnorm_rots, cam_trans, num_frames, time_idx, c.pose.dev))
        return fail(GS_EINVAL, "gs_render_backward_raw_pose_dev: null pose columns or time index outside [0, num_frames)");
    if (P > 0 && !logit_opacities) return fail(GS_EINVAL, "gs_render_backward_raw_pose_dev: null opacity parameters");
    if (!pose_scratch) return fail(GS_EINVAL, "gs_render_backward_raw_pose_dev: null pose scratch");
    c.g.in.means3D = means3D; c.g.in.shs = shs; c.g.in.colors = colors_precomp; c.g.in.opac = logit_opacities; c.g.in.scales = log_scales; c.g.in.rots = unnorm_rotations;
    c.P = P; c.D = D; c.isotropic = isotropic; c.pose.grad = gs::POSE_GRAD_ONLY; c.pose.dL_dpose7 = dL_dpose7; c.pose.pose_scratch = pose_scratch;
    c.g.radii = radii; c.geom_state = geom_state; c.point_list = point_list; c.image_state = image_state; c.dL_dcolor = dL_dcolor; c.dL_ddepth = dL_ddepth;
    c.g.out.dmeans2D = dL_dmeans2D;
    c.scratch = scratch; c.scratch_zeroed = scratch_zeroed; c.have_sh_jacobian = have_sh_jacobian;
    return render_backward_impl(cam, c, stream);
}

uint64_t gs_tracking_loss_scratch_bytes(int32_t width, int32_t height)
{
    const int64_t n = (int64_t)(width > 0 ? width : 1) * (height > 0 ? height : 1);
    return align_up((uint64_t)gs::tracking_loss_rows(n) * gs::kTrackRow * 4);
}

// d_median: the outlier rejection of gs_tracking_loss_outlier (`who` then requires it)
static int tracking_loss_impl(const char* who, bool outlier, int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth,
                              const float* depth_sq, const float* gt_depth, const float* silhouette, int32_t use_sil_for_loss, float sil_thres, float w_im,
                              float w_depth, float* dL_dim, float* dL_ddepth, void* loss_rows, float* losses, const float* d_median, gs_stream_t stream)
{
    if (width <= 0 || height <= 0 || (int64_t)width * height >= ((int64_t)1 << 31)) return fail(GS_EINVAL, "%s: bad image size", who);
    if (!im || !gt_im || !depth || !depth_sq || !gt_depth || !dL_dim || !dL_ddepth || !loss_rows || (outlier && !d_median) || (use_sil_for_loss && !silhouette))
        return fail(GS_EINVAL, "%s: null pointer", who);
    return launched(who, "", gs::launch_tracking_loss(width, height, im, gt_im, depth, depth_sq, gt_depth, silhouette, use_sil_for_loss != 0, sil_thres, w_im,
                    w_depth, dL_dim, dL_ddepth, (float*)loss_rows, losses, (hipStream_t)stream, d_median));
}

int gs_tracking_loss(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth, const float* depth_sq,
                     const float* gt_depth, const float* silhouette, int32_t use_sil_for_loss, float sil_thres, float w_im, float w_depth,
                     float* dL_dim, float* dL_ddepth, void* loss_rows, float* losses, gs_stream_t stream)
{
    return tracking_loss_impl("gs_tracking_loss", false, width, height, im, gt_im, depth, depth_sq, gt_depth, silhouette, use_sil_for_loss, sil_thres, w_im,
                              w_depth, dL_dim, dL_ddepth, loss_rows, losses, nullptr, stream);
}

int gs_tracking_loss_outlier(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth, const float* depth_sq,
                             const float* gt_depth, const float* silhouette, int32_t use_sil_for_loss, float sil_thres, float w_im, float w_depth,
                             float* dL_dim, float* dL_ddepth, void* loss_rows, float* losses, const float* d_median, gs_stream_t stream)
{
    return tracking_loss_impl("gs_tracking_loss_outlier", true, width, height, im, gt_im, depth, depth_sq, gt_depth, silhouette, use_sil_for_loss, sil_thres,
                              w_im, w_depth, dL_dim, dL_ddepth, loss_rows, losses, d_median, stream);
}

uint64_t gs_tracking_state_bytes(void) { return align_up((uint64_t)gs::kTrackState * 4); }

int gs_tracking_begin(const float* cam_unnorm_rots, const float* cam_trans, int64_t num_frames, int64_t time_idx, void* state, gs_stream_t stream)
{
    gs::DevPose dp;
    if (!dev_pose(cam_unnorm_rots, cam_trans, num_frames, time_idx, dp) || !state)
        return fail(GS_EINVAL, "gs_tracking_begin: null pointer or time index outside [0, num_frames)");
    return launched("gs_tracking_begin", "", gs::launch_tracking_begin(dp.q, dp.t, dp.stride, (float*)state, (hipStream_t)stream));
}

int gs_tracking_step(int32_t P, const void* pose_scratch, int32_t width, int32_t height, const void* loss_rows, float w_im, float w_depth,
                     float* cam_unnorm_rots, float* cam_trans, int64_t num_frames, int64_t time_idx, double lr_rot, double lr_trans, int32_t step,
                     void* state, float* history_row, gs_stream_t stream)
{
    gs::DevPose dp;
    if (!dev_pose(cam_unnorm_rots, cam_trans, num_frames, time_idx, dp) || !state || !loss_rows || (P > 0 && !pose_scratch))
        return fail(GS_EINVAL, "gs_tracking_step: null pointer or time index outside [0, num_frames)");
    if (P < 0 || width <= 0 || height <= 0 || step < 1) return fail(GS_EINVAL, "gs_tracking_step: bad size or step (the first step is 1)");
    // torch.optim.Adam (splatam.py:118-124, tracking=True): betas (0.9, 0.999), eps 1e-8; bias corrections of step `step` in double, as torch forms
    // them for its python-number step counts, handed to the kernel as the fp32 scalars its foreach kernels take
    const double b1 = 0.9, b2 = 0.999, bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    gs::TrackAdam c;
    c.one_m_b1 = (float)(1.0 - b1); c.b2 = (float)b2; c.one_m_b2 = (float)(1.0 - b2); c.bc2_sqrt = (float)pow(bc2, 0.5); c.eps = (float)1e-8;
    c.neg_step_size[0] = (float)(-(lr_rot / bc1)); c.neg_step_size[1] = (float)(-(lr_trans / bc1));
    const int64_t npix = (int64_t)width * height;
    return launched("gs_tracking_step", "", gs::launch_tracking_step(gs::pose_rows_count(P), (const float*)pose_scratch, gs::tracking_loss_rows(npix),
                    (const float*)loss_rows, w_im, w_depth, cam_unnorm_rots + time_idx, cam_trans + time_idx, num_frames, c, (float*)state, history_row,
                    (hipStream_t)stream));
}

int gs_render_backward_raw_adam(const GsCamera* cam, int32_t P, int64_t D, const float* means3D, const float* shs, const float* colors_precomp,
                                const float* logit_opacities, const float* log_scales, const float* unnorm_rotations, const float* h_pose7,
                                int32_t isotropic, const int32_t* radii, const void* geom_state, const uint32_t* point_list,
                                const void* image_state, const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans2D, void* scratch,
                                int32_t scratch_zeroed, int32_t have_sh_jacobian, const GsAdamTensor* adam5, gs_stream_t stream)
{
    if (!h_pose7 || !adam5 || (P > 0 && !logit_opacities)) return fail(GS_EINVAL, "gs_render_backward_raw_adam: null pose / opacity parameters / descriptors");
    BackwardCall c{};
    c.g.in.means3D = means3D; c.g.in.shs = shs; c.g.in.colors = colors_precomp; c.g.in.opac = logit_opacities; c.g.in.scales = log_scales; c.g.in.rots = unnorm_rotations;
    c.P = P; c.D = D; c.pose.source = gs::POSE_HOST; c.pose.pose7 = h_pose7; c.isotropic = isotropic; c.adam5 = adam5;
    c.g.radii = radii; c.geom_state = geom_state; c.point_list = point_list; c.image_state = image_state; c.dL_dcolor = dL_dcolor; c.dL_ddepth = dL_ddepth;
    c.g.out.dmeans2D = dL_dmeans2D;
    c.scratch = scratch; c.scratch_zeroed = scratch_zeroed; c.have_sh_jacobian = have_sh_jacobian;
    return render_backward_impl(cam, c, stream);
}

int gs_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr,
                 double beta1, double beta2, double eps, int32_t step, gs_stream_t stream)
{
    if (n < 0 || step < 1) return fail(GS_EINVAL, "gs_adam_step: bad n/step");
    if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return fail(GS_EINVAL, "gs_adam_step: null pointer");
    if (n > 0 && !adam_aligned16(param, grad, exp_avg, exp_avg_sq))
        return fail_adam_alignment("gs_adam_step", 0);
    ScopedStage ps(ST_ADAM, (hipStream_t)stream);
    return launched("gs_adam_step", "", gs::launch_adam(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, (hipStream_t)stream));
}

int gs_adam_step_multi(int32_t count, const GsAdamTensor* tensors, gs_stream_t stream)
{
    if (count < 0 || (count > 0 && !tensors)) return fail(GS_EINVAL, "gs_adam_step_multi: bad count/tensors");
    for (int i = 0; i < count; ++i) {
        const GsAdamTensor& t = tensors[i];
        if (t.n < 0 || t.step < 1) return fail(GS_EINVAL, "gs_adam_step_multi: a tensor has bad n/step");
        if (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return fail(GS_EINVAL, "gs_adam_step_multi: a tensor has a null pointer");
        // checked for the whole array before the first launch: a refusal leaves every tensor of the call untouched
        if (t.n > 0 && !adam_aligned16(t.param, t.grad, t.exp_avg, t.exp_avg_sq))
            return fail_adam_alignment("gs_adam_step_multi", i);
    }
    ScopedStage sc(ST_ADAM, (hipStream_t)stream);
    return launched("gs_adam_step_multi", "", gs::launch_adam_multi(count, tensors, (hipStream_t)stream));
}

static int rows_args_ok(int32_t count, const GsRowTensor* t, int mode)
{
    if (count < 1 || count > gs::kAdamMaxTensors || !t) return 0;
    int G = 0;
    for (int i = 0; i < count; ++i) {
        if (t[i].width < 1 || t[i].width > 64) return 0;
        G += t[i].width;
        if (mode != 0 && !t[i].param) return 0;
        if (mode == 2 && (!t[i].exp_avg || !t[i].exp_avg_sq || t[i].step < 1)) return 0;
    }
    return G <= 64;
}

int gs_pack_columns(int32_t count, const GsRowTensor* tensors, int64_t n, int64_t n_padded, float* flat, gs_stream_t stream)
{
    if (!rows_args_ok(count, tensors, 0) || n < 0 || n_padded < n || (n_padded > 0 && !flat)) return fail(GS_EINVAL, "gs_pack_columns: bad argument");
    return launched("gs_pack_columns", "", gs::launch_rows(0, count, tensors, 0, n, n_padded, nullptr, flat, (hipStream_t)stream));
}

int gs_adam_rows(int32_t count, const GsRowTensor* tensors, int64_t row_lo, int64_t n_valid, int64_t n_rows, const float* grad_shard,
                 float* out_shard, gs_stream_t stream)
{
    if (!rows_args_ok(count, tensors, 2) || row_lo < 0 || n_valid < 0 || n_rows < n_valid || (n_rows > 0 && !grad_shard))
        return fail(GS_EINVAL, "gs_adam_rows: bad argument");
    ScopedStage sc(ST_ADAM, (hipStream_t)stream);
    return launched("gs_adam_rows", "", gs::launch_rows(2, count, tensors, row_lo, n_valid, n_rows, grad_shard, out_shard, (hipStream_t)stream));
}

int gs_unpack_columns(int32_t count, const GsRowTensor* tensors, int64_t n, const float* flat, gs_stream_t stream)
{
    if (!rows_args_ok(count, tensors, 1) || n < 0 || (n > 0 && !flat)) return fail(GS_EINVAL, "gs_unpack_columns: bad argument");
    return launched("gs_unpack_columns", "", gs::launch_rows(1, count, tensors, 0, n, n, flat, nullptr, (hipStream_t)stream));
}

int gs_activate_forward(int32_t P, int32_t isotropic, const float* h_pose7, const float* means3D, const float* unnorm_rotations,
                        const float* logit_opacities, const float* log_scales, float* out_means3D, float* out_rotations,
                        float* out_opacities, float* out_scales, gs_stream_t stream)
{
    if (P < 0 || !h_pose7 || (P > 0 && (!means3D || !unnorm_rotations || !logit_opacities || !log_scales || !out_means3D ||
                                        !out_rotations || !out_opacities || !out_scales)))
        return fail(GS_EINVAL, "gs_activate_forward: bad argument");
    return launched("gs_activate_forward", "", gs::launch_activate_forward(P, isotropic, h_pose7, means3D, unnorm_rotations, logit_opacities, log_scales,
                    out_means3D, out_rotations, out_opacities, out_scales, (hipStream_t)stream));
}

static int activate_backward_impl(const char* who, int accumulate, int32_t P, int32_t isotropic, const float* h_pose7, const float* unnorm_rotations,
                                  const float* out_opacities, const float* out_scales, const float* g_means3D, const float* g_rotations,
                                  const float* g_opacities, const float* g_scales, float* d_means3D, float* d_unnorm_rotations, float* d_logit_opacities,
                                  float* d_log_scales, gs_stream_t stream)
{
    if (P < 0 || !h_pose7 || (P > 0 && (!unnorm_rotations || !out_opacities || !out_scales || !d_means3D || !d_unnorm_rotations ||
                                        !d_logit_opacities || !d_log_scales)))
        return fail(GS_EINVAL, "%s: bad argument", who);
    return launched(who, "", gs::launch_activate_backward(P, isotropic, h_pose7, unnorm_rotations, out_opacities, out_scales, g_means3D, g_rotations,
                    g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities, d_log_scales, accumulate, (hipStream_t)stream));
}

int gs_activate_backward(int32_t P, int32_t isotropic, const float* h_pose7, const float* unnorm_rotations, const float* out_opacities,
                         const float* out_scales, const float* g_means3D, const float* g_rotations, const float* g_opacities,
                         const float* g_scales, float* d_means3D, float* d_unnorm_rotations, float* d_logit_opacities,
                         float* d_log_scales, gs_stream_t stream)
{
    return activate_backward_impl("gs_activate_backward", 0, P, isotropic, h_pose7, unnorm_rotations, out_opacities, out_scales, g_means3D, g_rotations,
                                  g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities, d_log_scales, stream);
}

int gs_activate_backward_accumulate(int32_t P, int32_t isotropic, const float* h_pose7, const float* unnorm_rotations, const float* out_opacities,
                                    const float* out_scales, const float* g_means3D, const float* g_rotations, const float* g_opacities,
                                    const float* g_scales, float* d_means3D, float* d_unnorm_rotations, float* d_logit_opacities,
                                    float* d_log_scales, gs_stream_t stream)
{
    return activate_backward_impl("gs_activate_backward_accumulate", 1, P, isotropic, h_pose7, unnorm_rotations, out_opacities, out_scales, g_means3D,
                                  g_rotations, g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities, d_log_scales, stream);
}

int gs_activate_backward_pose(int32_t P, int32_t isotropic, const float* h_pose7, const float* means3D, const float* unnorm_rotations,
                              const float* out_opacities, const float* out_scales, const float* g_means3D, const float* g_rotations,
                              const float* g_opacities, const float* g_scales, float* d_means3D, float* d_unnorm_rotations,
                              float* d_logit_opacities, float* d_log_scales, int32_t accumulate, int32_t pose_only, float* dL_dpose7,
                              void* pose_scratch, gs_stream_t stream)
{
    if (P < 0 || !h_pose7 || !dL_dpose7 || !pose_scratch || (P > 0 && (!means3D || !unnorm_rotations)) ||
        (P > 0 && !pose_only && (!out_opacities || !out_scales || !d_means3D || !d_unnorm_rotations || !d_logit_opacities || !d_log_scales)))
        return fail(GS_EINVAL, "gs_activate_backward_pose: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) {
        return launched("gs_activate_backward_pose", "memset", hipMemsetAsync(dL_dpose7, 0, 7 * sizeof(float), st));
    }
    hipError_t e = gs::launch_activate_backward_pose(P, isotropic, h_pose7, means3D, unnorm_rotations, out_opacities, out_scales, g_means3D,
                                                     g_rotations, g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities,
                                                     d_log_scales, accumulate, pose_only ? 2 : 1, (float*)pose_scratch, st);
    if (int rc = launched("gs_activate_backward_pose", "", e)) return rc;
    e = gs::launch_pose_grad_finish(gs::pose_rows_count(P), h_pose7, (const float*)pose_scratch, dL_dpose7, st);
    return launched("gs_activate_backward_pose", "pose reduction", e);
}

uint64_t gs_mapping_loss_scratch_bytes(int32_t width, int32_t height)
{
    return align_up((uint64_t)(2 * gs::kLossAccSlots * 16 + 9 * (uint64_t)(width > 0 ? width : 1) * (uint64_t)(height > 0 ? height : 1)) * 4);   // two sets of accumulator lines + 9 maps
}

// d_median: the outlier rejection of gs_mapping_loss_outlier (`who` then requires it)
static int mapping_loss_impl(const char* who, bool outlier, int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth,
                             const float* depth_sq, const float* gt_depth, float w_im, float w_depth, float* losses, float* dL_dim, float* dL_ddepth,
                             void* scratch, int64_t persistent_call, const float* d_median, gs_stream_t stream)
{
    if (width <= 0 || height <= 0 || !im || !gt_im || !depth || !gt_depth || !losses || !dL_dim || !dL_ddepth || !scratch || persistent_call < 0 ||
        (outlier && !d_median))
        return fail(GS_EINVAL, "%s: bad argument", who);
    return launched(who, "", gs::launch_mapping_loss(width, height, im, gt_im, depth, depth_sq, gt_depth, w_im, w_depth, losses, dL_dim, dL_ddepth,
                    (float*)scratch, persistent_call, (hipStream_t)stream, d_median));
}

int gs_mapping_loss(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth,
                    const float* depth_sq, const float* gt_depth, float w_im, float w_depth, float* losses, float* dL_dim,
                    float* dL_ddepth, void* scratch, int64_t persistent_call, gs_stream_t stream)
{
    return mapping_loss_impl("gs_mapping_loss", false, width, height, im, gt_im, depth, depth_sq, gt_depth, w_im, w_depth, losses, dL_dim, dL_ddepth,
                             scratch, persistent_call, nullptr, stream);
}

int gs_mapping_loss_outlier(int32_t width, int32_t height, const float* im, const float* gt_im, const float* depth,
                            const float* depth_sq, const float* gt_depth, float w_im, float w_depth, float* losses, float* dL_dim,
                            float* dL_ddepth, void* scratch, int64_t persistent_call, const float* d_median, gs_stream_t stream)
{
    return mapping_loss_impl("gs_mapping_loss_outlier", true, width, height, im, gt_im, depth, depth_sq, gt_depth, w_im, w_depth, losses, dL_dim,
                             dL_ddepth, scratch, persistent_call, d_median, stream);
}

int32_t gs_depth_error_median_workgroups(int32_t width, int32_t height)
{
    return gs::depth_median_grid((int64_t)(width > 0 ? width : 1) * (height > 0 ? height : 1));
}

uint64_t gs_depth_error_median_scratch_bytes(int32_t width, int32_t height)
{
    (void)width; (void)height;          // three histograms and a flag, whatever the frame
    return align_up((uint64_t)gs::kMedianScratchWords * 4);
}

int gs_depth_error_median_grid(int32_t width, int32_t height, const float* depth, const float* gt_depth, void* scratch, float* d_median,
                               int32_t workgroups, gs_stream_t stream)
{
    if (width <= 0 || height <= 0 || (int64_t)width * height >= ((int64_t)1 << 31)) return fail(GS_EINVAL, "gs_depth_error_median: bad image size");
    if (!depth || !gt_depth || !scratch || !d_median) return fail(GS_EINVAL, "gs_depth_error_median: null pointer");
    if (workgroups < 0 || workgroups > gs::kMedianMaxGrid) return fail(GS_EINVAL, "gs_depth_error_median_grid: 0 (automatic) .. 1024 workgroups");
    return launched("gs_depth_error_median", "", gs::launch_depth_error_median((int64_t)width * height, depth, gt_depth, (uint32_t*)scratch, d_median,
                    workgroups, (hipStream_t)stream));
}

int gs_depth_error_median(int32_t width, int32_t height, const float* depth, const float* gt_depth, void* scratch, float* d_median,
                          gs_stream_t stream)
{
    return gs_depth_error_median_grid(width, height, depth, gt_depth, scratch, d_median, 0, stream);
}

uint64_t gs_compact_scratch_bytes(int64_t n) { return align_up(gs::compact_scratch_bytes(n > 0 ? n : 1)); }

int gs_compact_index(int64_t n, const uint8_t* keep, uint32_t* src_index, uint32_t* d_count, void* scratch, gs_stream_t stream)
{
    if (n < 0 || !d_count || !scratch || (n > 0 && (!keep || !src_index))) return fail(GS_EINVAL, "gs_compact_index: bad argument");
    if (n >= (int64_t)1 << 32) return fail(GS_ECAPACITY, "gs_compact_index: more than 2^32 rows");
    return launched("gs_compact_index", "", gs::launch_compact_index(n, keep, src_index, d_count, scratch, (hipStream_t)stream));
}

uint64_t gs_compact3_scratch_bytes(int64_t n) { return align_up(gs::compact3_scratch_bytes(n > 0 ? n : 1)); }

int gs_compact_index3(int64_t n, const uint8_t* keep_a, const uint8_t* keep_b, const uint8_t* keep_c, int32_t repeat_c, uint32_t* src_index,
                      uint32_t* d_counts, void* scratch, gs_stream_t stream)
{
    if (n < 0 || repeat_c < 1 || !d_counts || !scratch || (n > 0 && (!keep_a || !keep_b || !keep_c || !src_index)))
        return fail(GS_EINVAL, "gs_compact_index3: bad argument");
    if (n * (2 + (int64_t)repeat_c) >= (int64_t)1 << 32) return fail(GS_ECAPACITY, "gs_compact_index3: more than 2^32 rows");
    return launched("gs_compact_index3", "", gs::launch_compact_index3(n, keep_a, keep_b, keep_c, repeat_c, src_index, d_counts, scratch, (hipStream_t)stream));
}

int gs_gather_rows(int64_t n_out, int32_t row_floats, const uint32_t* src_index, const float* src, float* dst, gs_stream_t stream)
{
    if (n_out < 0 || row_floats <= 0 || (n_out > 0 && (!src_index || !src || !dst))) return fail(GS_EINVAL, "gs_gather_rows: bad argument");
    return launched("gs_gather_rows", "", gs::launch_gather_rows(n_out, row_floats, src_index, src, dst, n_out, (hipStream_t)stream));
}

int gs_gather_rows_zero_tail(int64_t n_out, int64_t n_copy, int32_t row_floats, const uint32_t* src_index, const float* src, float* dst,
                             gs_stream_t stream)
{
    if (n_out < 0 || n_copy < 0 || n_copy > n_out || row_floats <= 0 || (n_out > 0 && !dst) || (n_copy > 0 && (!src_index || !src)))
        return fail(GS_EINVAL, "gs_gather_rows_zero_tail: bad argument");
    return launched("gs_gather_rows_zero_tail", "", gs::launch_gather_rows(n_out, row_floats, src_index, src, dst, n_copy, (hipStream_t)stream));
}

int gs_densify_classify(int32_t N, int32_t scale_dim, const float* log_scales, const float* logit_opacities, const float* grad_accum,
                        const float* denom, const float* d_scene_radius, float grad_thresh, float opacity_thresh, int32_t remove_big,
                        int32_t num_to_split_into, uint8_t* keep_orig, uint8_t* keep_clone, uint8_t* keep_child, uint8_t* split_mask,
                        gs_stream_t stream)
{
    if (N < 0 || (scale_dim != 1 && scale_dim != 3) || num_to_split_into < 1 || !d_scene_radius ||
        (N > 0 && (!log_scales || !logit_opacities || !keep_orig)) || ((grad_accum == nullptr) != (denom == nullptr)))
        return fail(GS_EINVAL, "gs_densify_classify: bad argument");
    return launched("gs_densify_classify", "", gs::launch_densify_classify(N, scale_dim, log_scales, logit_opacities, grad_accum, denom, d_scene_radius,
                    grad_thresh, opacity_thresh, remove_big, num_to_split_into, keep_orig, keep_clone, keep_child, split_mask, (hipStream_t)stream));
}

int gs_densify_children(int32_t n_child, int32_t scale_dim, int32_t num_to_split_into, const float* unnorm_rotations, const float* samples,
                        uint64_t seed, float* means3D, float* log_scales, gs_stream_t stream)
{
    if (n_child < 0 || (scale_dim != 1 && scale_dim != 3) || num_to_split_into < 1 ||
        (n_child > 0 && (!unnorm_rotations || !means3D || !log_scales)))
        return fail(GS_EINVAL, "gs_densify_children: bad argument");
    return launched("gs_densify_children", "", gs::launch_densify_children(n_child, scale_dim, num_to_split_into, unnorm_rotations, samples, seed, means3D,
                    log_scales, (hipStream_t)stream));
}

int gs_visibility_stats(int32_t P, const int32_t* radii, uint8_t* seen, float* max_2D_radius, gs_stream_t stream)
{
    if (P < 0 || (P > 0 && !radii)) return fail(GS_EINVAL, "gs_visibility_stats: bad argument");
    return launched("gs_visibility_stats", "", gs::launch_visibility_stats(P, radii, seen, max_2D_radius, (hipStream_t)stream));
}

int gs_accumulate_grad2d(int32_t P, const float* means2D_grad, const uint8_t* seen, float* grad_accum, float* denom, gs_stream_t stream)
{
    if (P < 0 || (P > 0 && (!means2D_grad || !seen || !grad_accum || !denom))) return fail(GS_EINVAL, "gs_accumulate_grad2d: bad argument");
    return launched("gs_accumulate_grad2d", "", gs::launch_accumulate_grad2d(P, means2D_grad, seen, grad_accum, denom, (hipStream_t)stream));
}

static bool dbscan_size_ok(int32_t B, int32_t H, int32_t W, int32_t max_clusters)
{
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 4096 && W <= 4096 && (int64_t)H * W <= 65536 && max_clusters >= 1 && max_clusters <= 65535;
}

int gs_grid_dbscan_layout(int32_t B, int32_t H, int32_t W, int32_t max_clusters, GsDbscanLayout* out)
{
    if (!out || !dbscan_size_ok(B, H, W, max_clusters))
        return fail(GS_EINVAL, "gs_grid_dbscan_layout: size out of range (1 <= B <= 65535, H, W <= 4096, H * W <= 65536, 1 <= max_clusters <= 65535)");
    const uint64_t words = (uint64_t)B * H * ((W + 63) / 64), pixels = (uint64_t)B * H * W;
    uint64_t o = 0;
    out->mask_bits = o; o = align_up(o + words * 8);
    out->core_bits = o; o = align_up(o + words * 8);
    out->root_bits = o; o = align_up(o + words * 8);
    out->word_prefix = o; o = align_up(o + words * 4);
    out->parent = o; o = align_up(o + pixels * 4);
    out->root = o; o = align_up(o + pixels * 4);
    out->row_range = o; o = align_up(o + (uint64_t)B * max_clusters * 8);
    out->total_bytes = o;
    return GS_OK;
}

int gs_grid_dbscan(int32_t B, int32_t H, int32_t W, const float* values, int64_t row_stride, int64_t image_stride, float threshold,
                   int32_t complement, int32_t eps, int32_t min_samples, int32_t max_clusters, void* workspace, int32_t* labels,
                   int32_t* n_clusters, int32_t* table, float* sum_value, float* total, gs_stream_t stream)
{
    GsDbscanLayout L;
    if (!dbscan_size_ok(B, H, W, max_clusters))
        return fail(GS_EINVAL, "gs_grid_dbscan: size out of range (1 <= B <= 65535, H, W <= 4096, H * W <= 65536, 1 <= max_clusters <= 65535)");
    if (eps < 1 || eps > 8 || min_samples < 1) return fail(GS_EINVAL, "gs_grid_dbscan: eps must be 1..8 and min_samples at least 1");
    if (!values || !workspace || !labels || !n_clusters || !table || !sum_value || !total || row_stride < W || image_stride < 0 ||
        ((uintptr_t)workspace & 7))
        return fail(GS_EINVAL, "gs_grid_dbscan: null pointer, workspace not 8-byte aligned, or row_stride below W");
    gs_grid_dbscan_layout(B, H, W, max_clusters, &L);
    char* ws = (char*)workspace;
    gs::DbscanArgs a;
    a.values = values; a.row_stride = row_stride; a.image_stride = image_stride;
    a.H = H; a.W = W; a.Ww = (W + 63) / 64; a.npix = H * W;
    a.threshold = threshold; a.complement = complement != 0; a.eps = eps; a.min_samples = min_samples; a.max_clusters = max_clusters;
    for (int dy = 0; dy <= 8; dy++) {
        int w = 0;
        while (dy <= eps && (w + 1) * (w + 1) + dy * dy <= eps * eps) w++;
        a.half_width[dy] = w;
    }
    a.mask_bits = (uint64_t*)(ws + L.mask_bits); a.core_bits = (uint64_t*)(ws + L.core_bits); a.root_bits = (uint64_t*)(ws + L.root_bits);
    a.word_prefix = (uint32_t*)(ws + L.word_prefix); a.parent = (uint32_t*)(ws + L.parent); a.root = (int32_t*)(ws + L.root);
    a.row_range = (uint32_t*)(ws + L.row_range);
    a.labels = labels; a.n_clusters = n_clusters; a.table = table; a.sum_value = sum_value; a.total = total;
    return launched("gs_grid_dbscan", "", gs::launch_grid_dbscan(a, B, (hipStream_t)stream));
}

int gs_cluster_hulls_layout(int32_t B, int32_t H, int32_t W, int32_t max_clusters, int32_t max_points, GsHullLayout* out)
{
    if (!out || !dbscan_size_ok(B, H, W, max_clusters) || max_points < 4 || max_points > 4096)
        return fail(GS_EINVAL, "gs_cluster_hulls_layout: size out of range (1 <= B <= 65535, H, W <= 4096, H * W <= 65536, 1 <= max_clusters <= 65535, "
                               "4 <= max_points <= 4096)");
    out->cluster_status = 0;
    out->total_bytes = align_up((uint64_t)B * max_clusters * 4);
    return GS_OK;
}

int gs_cluster_hulls(int32_t B, int32_t H, int32_t W, const int32_t* labels, const float* depth, int64_t row_stride, int64_t image_stride,
                     const int32_t* n_clusters, const float* sum_value, int32_t max_clusters, const uint32_t* footprint_rows, int32_t kh,
                     int32_t kw, float skip_depth, double x_scale, double y_scale, int32_t max_points, void* workspace, double* volume,
                     int32_t* n_points, int32_t* contour_xy, double* sum_volume, double* sum_invisibility, int32_t* status, gs_stream_t stream)
{
    GsHullLayout L;
    if (!dbscan_size_ok(B, H, W, max_clusters) || max_points < 4 || max_points > 4096)
        return fail(GS_EINVAL, "gs_cluster_hulls: size out of range (1 <= B <= 65535, H, W <= 4096, H * W <= 65536, 1 <= max_clusters <= 65535, "
                               "4 <= max_points <= 4096)");
    if (kh < 1 || kh > 15 || kw < 1 || kw > 15 || !(kh & 1) || !(kw & 1) || !footprint_rows)
        return fail(GS_EINVAL, "gs_cluster_hulls: the footprint must have odd kh and kw in 1..15");
    for (int i = 0; i < kh; i++)
        if (footprint_rows[i] >> kw) return fail(GS_EINVAL, "gs_cluster_hulls: a footprint row has a cell at or beyond kw");
    if (!labels || !depth || !n_clusters || !sum_value || !workspace || !volume || !n_points || !sum_volume || !sum_invisibility || !status ||
        row_stride < W || image_stride < 0 || ((uintptr_t)workspace & 7))
        return fail(GS_EINVAL, "gs_cluster_hulls: null pointer (only contour_xy may be null), workspace not 8-byte aligned, or row_stride below W");
    // (written so that a NaN fails it)
    if (!(fabs(x_scale) <= 1.7976931348623157e308) || !(fabs(y_scale) <= 1.7976931348623157e308))
        return fail(GS_EINVAL, "gs_cluster_hulls: x_scale and y_scale must be finite");
    gs_cluster_hulls_layout(B, H, W, max_clusters, max_points, &L);
    gs::HullArgs a;
    a.labels = labels; a.depth = depth; a.row_stride = row_stride; a.image_stride = image_stride;
    a.n_clusters = n_clusters; a.sum_value = sum_value;
    a.H = H; a.W = W; a.Ww = (W + 63) / 64; a.max_clusters = max_clusters; a.max_points = max_points;
    a.kh = kh; a.kw = kw;
    for (int i = 0; i < 15; i++) a.footprint[i] = i < kh ? footprint_rows[i] : 0u;
    a.skip_depth = skip_depth; a.scale = x_scale * y_scale;
    a.cluster_status = (int32_t*)((char*)workspace + L.cluster_status);
    a.volume = volume; a.n_points = n_points; a.contour_xy = contour_xy;
    a.sum_volume = sum_volume; a.sum_invisibility = sum_invisibility; a.status = status;
    return launched("gs_cluster_hulls", "", gs::launch_cluster_hulls(a, B, (hipStream_t)stream));
}

int gs_high_loss_grid(int32_t width, int32_t height, const float* render_depth, const float* opacity, const float* gt_depth,
                      float depth_err_thres, float opacity_thres, int32_t grid_width, int32_t grid_height, uint8_t* mask_full, float* grid,
                      gs_stream_t stream)
{
    if (width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(GS_EINVAL, "gs_high_loss_grid: image size out of range (1 <= width, height <= 16384)");
    if (grid_width < 1 || grid_height < 1 || grid_width > 4096 || grid_height > 4096 || (int64_t)grid_width * grid_height > 65536)
        return fail(GS_EINVAL, "gs_high_loss_grid: grid size out of range (1 <= grid_width, grid_height <= 4096, grid_width * grid_height <= 65536)");
    // (written so that a NaN fails them: finite and not negative)
    if (!(depth_err_thres >= 0.0f && depth_err_thres <= 3.402823466e38f) || !(opacity_thres >= 0.0f && opacity_thres <= 3.402823466e38f))
        return fail(GS_EINVAL, "gs_high_loss_grid: thresholds must be finite and not negative");
    if (!render_depth || !opacity || !gt_depth || !grid) return fail(GS_EINVAL, "gs_high_loss_grid: null pointer (only mask_full may be null)");
    gs::HighLossArgs a;
    a.depth = render_depth; a.opacity = opacity; a.gt = gt_depth;
    a.W = width; a.H = height; a.gw = grid_width; a.gh = grid_height;
    a.depth_thres = depth_err_thres; a.opacity_thres = opacity_thres;
    a.mask_full = mask_full; a.grid = grid;
    return launched("gs_high_loss_grid", "", gs::launch_high_loss_grid(a, (hipStream_t)stream));
}

uint64_t gs_grow_scratch_bytes(int32_t width, int32_t height)
{
    return align_up(gs::grow_scratch_bytes((int64_t)(width > 0 ? width : 1) * (height > 0 ? height : 1)));
}

int gs_grow_gaussians(int32_t width, int32_t height, const float* render_depth, const float* silhouette, const float* gt_depth,
                      const float* color, const float* h_intrinsics4, const float* h_c2w12, float sil_thres, int32_t isotropic,
                      float* out_means3D, float* out_rgb_colors, float* out_unnorm_rotations, float* out_logit_opacities,
                      float* out_log_scales, uint32_t* d_counts, void* scratch, gs_stream_t stream)
{
    if (width <= 0 || height <= 0 || !render_depth || !silhouette || !gt_depth || !color || !h_intrinsics4 || !h_c2w12 ||
        !out_means3D || !out_rgb_colors || !out_unnorm_rotations || !out_logit_opacities || !out_log_scales || !d_counts || !scratch)
        return fail(GS_EINVAL, "gs_grow_gaussians: bad argument");
    if ((int64_t)width * height >= ((int64_t)1 << 31)) return fail(GS_EINVAL, "gs_grow_gaussians: bad image size");     // (the median select's 32-bit rank)
    return launched("gs_grow_gaussians", "", gs::launch_grow(width, height, render_depth, silhouette, gt_depth, color, h_intrinsics4, h_c2w12, sil_thres,
                    isotropic != 0, out_means3D, out_rgb_colors, out_unnorm_rotations, out_logit_opacities, out_log_scales, d_counts, scratch,
                    (hipStream_t)stream));
}

int gs_keyframe_overlap(int32_t n_pts, const float* pts_world, int32_t n_keyframes, const float* w2c, const float* h_intrinsics9,
                        int32_t width, int32_t height, int32_t edge, uint32_t* counts, gs_stream_t stream)
{
    if (n_pts < 0 || n_keyframes < 0 || width <= 0 || height <= 0 || !h_intrinsics9 ||
        (n_keyframes > 0 && (!w2c || !counts)) || (n_pts > 0 && !pts_world))
        return fail(GS_EINVAL, "gs_keyframe_overlap: bad argument");
    return launched("gs_keyframe_overlap", "", gs::launch_keyframe_overlap(n_pts, pts_world, n_keyframes, w2c, h_intrinsics9, width, height, edge, counts,
                    (hipStream_t)stream));
}

int gs_frame_ingest(int32_t width, int32_t height, const uint8_t* image, const float* depth, const float* level_value, int32_t n_out,
                    const int32_t* h_sizes, float* color0, float* depth0, float* color1, float* depth1, gs_stream_t stream)
{
    if (n_out < 1 || n_out > 2) return fail(GS_EINVAL, "gs_frame_ingest: n_out must be 1 or 2");
    if (!image || !depth || !level_value || !h_sizes || !color0 || !depth0 || (n_out == 2 && (!color1 || !depth1)))
        return fail(GS_EINVAL, "gs_frame_ingest: null pointer");
    if (width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(GS_EINVAL, "gs_frame_ingest: source size out of range (1 <= width, height <= 16384)");
    for (int k = 0; k < 2 * n_out; ++k)
        if (h_sizes[k] < 1 || h_sizes[k] > 16384) return fail(GS_EINVAL, "gs_frame_ingest: output size out of range (1 <= W, H <= 16384)");
    float* const colors[2] = {color0, color1};
    float* const depths[2] = {depth0, depth1};
    return launched("gs_frame_ingest", "", gs::launch_frame_ingest(width, height, image, depth, level_value, n_out, h_sizes, colors, depths, (hipStream_t)stream));
}

int gs_depth_cloud(int32_t width, int32_t height, const float* depth, const float* h_intrinsics4, const float* h_c2w12, float* points,
                   uint8_t* valid, gs_stream_t stream)
{
    if (width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(GS_EINVAL, "gs_depth_cloud: image size out of range (1 <= width, height <= 16384)");
    if (!depth || !h_intrinsics4 || !h_c2w12 || !points || !valid) return fail(GS_EINVAL, "gs_depth_cloud: null pointer");
    // (written so that a NaN fails it)
    if (!(fabsf(h_intrinsics4[0]) > 0.0f) || !(fabsf(h_intrinsics4[1]) > 0.0f))
        return fail(GS_EINVAL, "gs_depth_cloud: fx and fy must not be zero");
    return launched("gs_depth_cloud", "", gs::launch_depth_cloud(width, height, depth, h_intrinsics4, h_c2w12, points, valid, (hipStream_t)stream));
}

// ---- TSDF fusion and surface extraction (grow.hip) ----
static bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }                  // (a NaN fails it)
static bool positive_finite(float v) { return v > 0.0f && v <= 3.402823466e38f; }

// the checks on a volume's shape shared by the three calls; fills g
static int tsdf_grid_checked(const char* who, int32_t nx, int32_t ny, int32_t nz, const float* h_origin3, float voxel_size, gs::TsdfGrid& g)
{
    if (nx < 1 || ny < 1 || nz < 1) return fail(GS_EINVAL, "%s: volume dimensions must be at least 1", who);
    if ((int64_t)nx * ny >= ((int64_t)1 << 31) || (int64_t)nx * ny * nz >= ((int64_t)1 << 31))
        return fail(GS_EINVAL, "%s: nx * ny * nz must be below 2^31", who);
    g.nx = nx; g.ny = ny; g.nz = nz; g.n = (int64_t)nx * ny * nz;
    g.ox = g.oy = g.oz = 0.0f; g.vs = 1.0f;
    if (h_origin3) {
        if (!finite_f(h_origin3[0]) || !finite_f(h_origin3[1]) || !finite_f(h_origin3[2])) return fail(GS_EINVAL, "%s: origin must be finite", who);
        if (!positive_finite(voxel_size)) return fail(GS_EINVAL, "%s: voxel_size must be positive and finite", who);
        g.ox = h_origin3[0]; g.oy = h_origin3[1]; g.oz = h_origin3[2]; g.vs = voxel_size;
    }
    return GS_OK;
}

int gs_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* h_origin3, float voxel_size, float trunc, float max_weight, float* tsdf,
                      float* weight, float* color, int32_t n_frames, int32_t width, int32_t height, const float* depth, const float* frame_color,
                      const float* silhouette, const float* h_intrinsics4, const float* h_w2c12, float sil_thres, float depth_max, gs_stream_t stream)
{
    gs::TsdfArgs a;
    if (!h_origin3 || !h_intrinsics4 || !h_w2c12 || !tsdf || !weight || !depth || (frame_color && !color))
        return fail(GS_EINVAL, "gs_tsdf_integrate: null pointer (color may be null only without frame_color; frame_color and silhouette may be null)");
    if ((((uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)color) & 15) || (((uintptr_t)depth | (uintptr_t)frame_color | (uintptr_t)silhouette) & 3))
        return fail(GS_EINVAL, "gs_tsdf_integrate: tsdf / weight / color must be 16-byte aligned (the kernel makes 128-bit accesses), the images 4-byte aligned");
    const int rc = tsdf_grid_checked("gs_tsdf_integrate", nx, ny, nz, h_origin3, voxel_size, a.g);
    if (rc != GS_OK) return rc;
    if (!positive_finite(trunc)) return fail(GS_EINVAL, "gs_tsdf_integrate: trunc must be positive and finite");
    if (!(max_weight >= 1.0f && max_weight <= 3.402823466e38f)) return fail(GS_EINVAL, "gs_tsdf_integrate: max_weight must be at least 1 and finite");
    if (n_frames < 0 || n_frames > gs::kTsdfMaxFrames) return fail(GS_EINVAL, "gs_tsdf_integrate: 0 <= n_frames <= 16 (the poses travel in the kernel arguments)");
    if (width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(GS_EINVAL, "gs_tsdf_integrate: image size out of range (1 <= width, height <= 16384)");
    if (!positive_finite(h_intrinsics4[0]) || !positive_finite(h_intrinsics4[1])) return fail(GS_EINVAL, "gs_tsdf_integrate: fx and fy must be positive and finite");
    if (!finite_f(h_intrinsics4[2]) || !finite_f(h_intrinsics4[3])) return fail(GS_EINVAL, "gs_tsdf_integrate: cx and cy must be finite");
    for (int i = 0; i < 12 * n_frames; ++i)
        if (!finite_f(h_w2c12[i])) return fail(GS_EINVAL, "gs_tsdf_integrate: poses must be finite");
    if (!(depth_max > 0.0f)) return fail(GS_EINVAL, "gs_tsdf_integrate: depth_max must be positive (infinity: no limit)");
    if (sil_thres != sil_thres) return fail(GS_EINVAL, "gs_tsdf_integrate: sil_thres must not be NaN");
    a.trunc = trunc; a.max_weight = max_weight;
    a.tsdf = tsdf; a.weight = weight; a.color = color;
    a.frames = n_frames; a.W = width; a.H = height;
    a.depth = depth; a.frame_color = frame_color; a.silhouette = silhouette;
    a.fx = h_intrinsics4[0]; a.fy = h_intrinsics4[1]; a.cx = h_intrinsics4[2]; a.cy = h_intrinsics4[3];
    a.sil_thres = sil_thres; a.depth_max = depth_max;
    memset(a.f, 0, sizeof(a.f));
    for (int f = 0; f < n_frames; ++f) {
        const float* m = h_w2c12 + 12 * f;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) a.f[f].r[3 * r + c] = m[4 * r + c];
            a.f[f].t[r] = m[4 * r + 3];
        }
    }
    return launched("gs_tsdf_integrate", "", gs::launch_tsdf_integrate(a, (hipStream_t)stream));
}

// a vertex index is an int32 and a grid point owns up to seven vertices
static const int64_t kTsdfExtractMaxPoints = (((int64_t)1 << 31) - 1) / 7;

uint64_t gs_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    gs::TsdfGrid g;
    if (tsdf_grid_checked("gs_tsdf_extract_scratch_bytes", nx, ny, nz, nullptr, 1.0f, g) != GS_OK || g.n > kTsdfExtractMaxPoints) return 0;
    return gs::tsdf_extract_scratch_bytes(g.n);
}

int gs_tsdf_count(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight, void* scratch, uint32_t* d_counts,
                  gs_stream_t stream)
{
    gs::TsdfExtractArgs a;
    if (!tsdf || !weight || !scratch || !d_counts || ((uintptr_t)scratch & 15) || (((uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)d_counts) & 3))
        return fail(GS_EINVAL, "gs_tsdf_count: null pointer, scratch not 16-byte aligned or an array not 4-byte aligned");
    const int rc = tsdf_grid_checked("gs_tsdf_count", nx, ny, nz, nullptr, 1.0f, a.g);
    if (rc != GS_OK) return rc;
    if (a.g.n > kTsdfExtractMaxPoints) return fail(GS_EINVAL, "gs_tsdf_count: 7 * nx * ny * nz must be below 2^31 (vertex indices are int32)");
    if (min_weight != min_weight) return fail(GS_EINVAL, "gs_tsdf_count: min_weight must not be NaN");
    a.min_weight = min_weight; a.tsdf = tsdf; a.weight = weight; a.color = nullptr;
    gs::tsdf_extract_carve(a.g.n, scratch, a);
    return launched("gs_tsdf_count", "", gs::launch_tsdf_count(a, d_counts, (hipStream_t)stream));
}

int gs_tsdf_emit(int32_t nx, int32_t ny, int32_t nz, const float* h_origin3, float voxel_size, const float* tsdf, const float* color, void* scratch,
                 int32_t max_vertices, int32_t max_triangles, float* vertices, float* vertex_colors, int32_t* triangles, gs_stream_t stream)
{
    gs::TsdfExtractArgs a;
    if (max_vertices < 0 || max_triangles < 0) return fail(GS_EINVAL, "gs_tsdf_emit: max_vertices and max_triangles must not be negative");
    if (!h_origin3 || !tsdf || !scratch || (max_vertices > 0 && (!vertices || (color && !vertex_colors))) || (max_triangles > 0 && !triangles) ||
        ((uintptr_t)scratch & 15) || (((uintptr_t)tsdf | (uintptr_t)color | (uintptr_t)vertices | (uintptr_t)vertex_colors | (uintptr_t)triangles) & 3))
        return fail(GS_EINVAL, "gs_tsdf_emit: null pointer (color may be null: no vertex colours; an output may be null when its maximum is 0), scratch not "
                               "16-byte aligned or an array not 4-byte aligned");
    const int rc = tsdf_grid_checked("gs_tsdf_emit", nx, ny, nz, h_origin3, voxel_size, a.g);
    if (rc != GS_OK) return rc;
    if (a.g.n > kTsdfExtractMaxPoints) return fail(GS_EINVAL, "gs_tsdf_emit: 7 * nx * ny * nz must be below 2^31 (vertex indices are int32)");
    a.min_weight = 0.0f; a.tsdf = tsdf; a.weight = nullptr; a.color = color;
    gs::tsdf_extract_carve(a.g.n, scratch, a);
    return launched("gs_tsdf_emit", "", gs::launch_tsdf_emit(a, (uint32_t)max_vertices, (uint32_t)max_triangles, vertices, vertex_colors, triangles,
                    (hipStream_t)stream));
}

static int mesh_layout_checked(const char* who, int32_t num_triangles, int32_t width, int32_t height, uint32_t capacity, GsMeshLayout& L)
{
    if (num_triangles < 0) return fail(GS_EINVAL, "%s: num_triangles must not be negative", who);
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail(GS_EINVAL, "%s: image size out of range (1 <= width, height <= 16384)", who);
    const uint64_t tiles = tiles_of(width, height);
    uint64_t at = 0;
    L.total = at;       at += 256;
    L.records = at;     at += align_up((uint64_t)num_triangles * 64u);
    L.rects = at;       at += align_up((uint64_t)num_triangles * 8u);
    L.tile_count = at;  at += align_up((tiles + 1) * 4u);
    L.tile_offset = at; at += align_up((tiles + 1) * 4u);
    L.list = at;        at += align_up((uint64_t)capacity * 4u);
    L.total_bytes = at;
    return GS_OK;
}

int gs_mesh_render_layout(int32_t num_triangles, int32_t width, int32_t height, uint32_t capacity, GsMeshLayout* layout)
{
    if (!layout) return fail(GS_EINVAL, "gs_mesh_render_layout: null pointer");
    return mesh_layout_checked("gs_mesh_render_layout", num_triangles, width, height, capacity, *layout);
}

// the argument checks of gs_mesh_render and the carving of its scratch, shared with gs_mesh_render_textured
static int mesh_args_checked(const char* who, int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles,
                             const uint8_t* vertex_colors, const float* h_intrinsics4, const float* h_w2c12, float near_z, int32_t width, int32_t height,
                             void* scratch, uint32_t capacity, float* depth, int32_t* tri_id, uint8_t* color, uint32_t* d_counts, gs::MeshArgs& a)
{
    GsMeshLayout L;
    const int rc = mesh_layout_checked(who, num_triangles, width, height, capacity, L);
    if (rc != GS_OK) return rc;
    if (num_vertices < 0) return fail(GS_EINVAL, "%s: num_vertices must not be negative", who);
    if (!h_intrinsics4 || !h_w2c12 || !scratch || !depth || !tri_id || !color || !d_counts ||
        (num_triangles > 0 && (!vertices || !triangles || !vertex_colors)) || ((uintptr_t)scratch & 15))
        return fail(GS_EINVAL, "%s: null pointer (the mesh arrays may be null only with num_triangles == 0) or scratch not 16-byte aligned", who);
    // (written so that a NaN fails them)
    if (!(near_z > 0.0f && near_z <= 3.402823466e38f)) return fail(GS_EINVAL, "%s: near must be positive and finite", who);
    for (int i = 0; i < 4; ++i)
        if (!(fabsf(h_intrinsics4[i]) <= 3.402823466e38f)) return fail(GS_EINVAL, "%s: intrinsics must be finite", who);
    if (!(fabsf(h_intrinsics4[0]) > 0.0f) || !(fabsf(h_intrinsics4[1]) > 0.0f)) return fail(GS_EINVAL, "%s: fx and fy must not be zero", who);
    a.V = num_vertices; a.T = num_triangles;
    a.vertices = vertices; a.triangles = triangles; a.vertex_colors = vertex_colors;
    a.fx = h_intrinsics4[0]; a.fy = h_intrinsics4[1]; a.cx = h_intrinsics4[2]; a.cy = h_intrinsics4[3];
    for (int i = 0; i < 12; ++i) a.w2c[i] = h_w2c12[i];
    a.near_z = near_z; a.W = width; a.H = height;
    char* b = (char*)scratch;
    a.total = (uint64_t*)(b + L.total); a.records = (float4*)(b + L.records); a.rects = (uint2*)(b + L.rects);
    a.tile_count = (uint32_t*)(b + L.tile_count); a.tile_offset = (uint32_t*)(b + L.tile_offset); a.list = (uint32_t*)(b + L.list);
    a.capacity = capacity;
    a.depth = depth; a.tri_id = tri_id; a.color = color; a.d_counts = d_counts;
    return GS_OK;
}

int gs_mesh_render(int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles, const uint8_t* vertex_colors,
                   const float* h_intrinsics4, const float* h_w2c12, float near_z, int32_t width, int32_t height, void* scratch, uint32_t capacity,
                   float* depth, int32_t* tri_id, uint8_t* color, uint32_t* d_counts, gs_stream_t stream)
{
    gs::MeshArgs a;
    const int rc = mesh_args_checked("gs_mesh_render", num_vertices, vertices, num_triangles, triangles, vertex_colors, h_intrinsics4, h_w2c12, near_z, width,
                                     height, scratch, capacity, depth, tri_id, color, d_counts, a);
    if (rc != GS_OK) return rc;
    return launched("gs_mesh_render", "", gs::launch_mesh_render(a, (hipStream_t)stream));
}

// gs_mesh_navgrid's scratch: gs_mesh_render's regions, with 48-byte records
static int navgrid_layout_checked(const char* who, int32_t num_triangles, int32_t grid_width, int32_t grid_height, uint32_t capacity, GsMeshLayout& L)
{
    if (num_triangles < 0) return fail(GS_EINVAL, "%s: num_triangles must not be negative", who);
    if (grid_width < 1 || grid_height < 1 || grid_width > 16384 || grid_height > 16384)
        return fail(GS_EINVAL, "%s: grid size out of range (1 <= grid_width, grid_height <= 16384)", who);
    const uint64_t tiles = tiles_of(grid_width, grid_height);
    uint64_t at = 0;
    L.total = at;       at += 256;
    L.records = at;     at += align_up((uint64_t)num_triangles * 48u);
    L.rects = at;       at += align_up((uint64_t)num_triangles * 8u);
    L.tile_count = at;  at += align_up((tiles + 1) * 4u);
    L.tile_offset = at; at += align_up((tiles + 1) * 4u);
    L.list = at;        at += align_up((uint64_t)capacity * 4u);
    L.total_bytes = at;
    return GS_OK;
}

int gs_mesh_navgrid_layout(int32_t num_triangles, int32_t grid_width, int32_t grid_height, uint32_t capacity, GsMeshLayout* layout)
{
    if (!layout) return fail(GS_EINVAL, "gs_mesh_navgrid_layout: null pointer");
    return navgrid_layout_checked("gs_mesh_navgrid_layout", num_triangles, grid_width, grid_height, capacity, *layout);
}

int gs_mesh_navgrid(int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles, double x0, double z0, double cell,
                    double floor_y, double max_climb, double agent_height, int32_t grid_width, int32_t grid_height, void* scratch, uint32_t capacity,
                    uint8_t* grid, uint32_t* d_counts, gs_stream_t stream)
{
    const char* who = "gs_mesh_navgrid";
    GsMeshLayout L;
    const int rc = navgrid_layout_checked(who, num_triangles, grid_width, grid_height, capacity, L);
    if (rc != GS_OK) return rc;
    if (num_vertices < 0) return fail(GS_EINVAL, "%s: num_vertices must not be negative", who);
    if (!scratch || !grid || !d_counts || (num_triangles > 0 && (!vertices || !triangles)) || ((uintptr_t)scratch & 15))
        return fail(GS_EINVAL, "%s: null pointer (the mesh arrays may be null only with num_triangles == 0) or scratch not 16-byte aligned", who);
    // (written so that a NaN fails them)
    const double big = 1.7976931348623157e308;
    if (!(fabs(x0) <= big) || !(fabs(z0) <= big) || !(fabs(floor_y) <= big) || !(fabs(max_climb) <= big) || !(fabs(agent_height) <= big))
        return fail(GS_EINVAL, "%s: x0, z0, floor_y, max_climb and agent_height must be finite", who);
    if (!(cell > 0.0 && cell <= big)) return fail(GS_EINVAL, "%s: cell must be positive and finite", who);
    if (!(max_climb >= 0.0)) return fail(GS_EINVAL, "%s: max_climb must not be negative", who);
    if (!(agent_height > max_climb)) return fail(GS_EINVAL, "%s: agent_height must exceed max_climb", who);
    gs::NavGridArgs a;
    a.V = num_vertices; a.T = num_triangles; a.vertices = vertices; a.triangles = triangles;
    a.x0 = x0; a.z0 = z0; a.cell = cell; a.floor_y = floor_y; a.max_climb = max_climb; a.agent_height = agent_height;
    a.W = grid_width; a.H = grid_height;
    char* b = (char*)scratch;
    a.total = (uint64_t*)(b + L.total); a.records = (float4*)(b + L.records); a.rects = (uint2*)(b + L.rects);
    a.tile_count = (uint32_t*)(b + L.tile_count); a.tile_offset = (uint32_t*)(b + L.tile_offset); a.list = (uint32_t*)(b + L.list);
    a.capacity = capacity; a.grid = grid; a.d_counts = d_counts;
    return launched(who, "", gs::launch_mesh_navgrid(a, (hipStream_t)stream));
}

// levels and offsets of one texture after `at` texels; false: a size out of range
static bool texture_plan(int32_t width, int32_t height, uint64_t& at, int32_t& levels, uint64_t (&offset)[GS_TEXTURE_MAX_LEVELS])
{
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return false;
    levels = 1;
    for (int m = width > height ? width : height; m > 1; m >>= 1) ++levels;
    for (int l = 0; l < GS_TEXTURE_MAX_LEVELS; ++l) {
        offset[l] = l < levels ? at : 0;
        if (l < levels) at += (uint64_t)((width >> l) > 1 ? (width >> l) : 1) * (uint64_t)((height >> l) > 1 ? (height >> l) : 1);
    }
    return true;
}

// a HOST table as gs_texture_layout left it, for a pool of pool_texels
static int texture_table_checked(const char* who, int32_t num_textures, const GsTextureDesc* h, uint64_t pool_texels)
{
    uint64_t at = 0;
    for (int k = 0; k < num_textures; ++k) {
        int32_t levels;
        uint64_t offset[GS_TEXTURE_MAX_LEVELS];
        if (!texture_plan(h[k].width, h[k].height, at, levels, offset)) return fail(GS_EINVAL, "%s: texture size out of range (1 <= width, height <= 16384)", who);
        if ((uint32_t)h[k].wrap_s > 2u || (uint32_t)h[k].wrap_t > 2u) return fail(GS_EINVAL, "%s: wrap mode out of range (0 repeat, 1 clamp, 2 mirror)", who);
        bool same = h[k].levels == levels;
        for (int l = 0; l < GS_TEXTURE_MAX_LEVELS; ++l) same = same && h[k].level_offset[l] == offset[l];
        if (!same) return fail(GS_EINVAL, "%s: levels / level offsets of the texture table are not gs_texture_layout's", who);
    }
    if (at != pool_texels) return fail(GS_EINVAL, "%s: pool_texels is not the total gs_texture_layout returned", who);
    return GS_OK;
}

int gs_texture_layout(int32_t num_textures, GsTextureDesc* h_textures, uint64_t* pool_texels)
{
    if (num_textures < 0) return fail(GS_EINVAL, "gs_texture_layout: num_textures must not be negative");
    if (!pool_texels || (num_textures > 0 && !h_textures)) return fail(GS_EINVAL, "gs_texture_layout: null pointer");
    for (int k = 0; k < num_textures; ++k) {                   // (everything is checked before anything is written)
        if (h_textures[k].width < 1 || h_textures[k].height < 1 || h_textures[k].width > 16384 || h_textures[k].height > 16384)
            return fail(GS_EINVAL, "gs_texture_layout: texture size out of range (1 <= width, height <= 16384)");
        if ((uint32_t)h_textures[k].wrap_s > 2u || (uint32_t)h_textures[k].wrap_t > 2u)
            return fail(GS_EINVAL, "gs_texture_layout: wrap mode out of range (0 repeat, 1 clamp, 2 mirror)");
    }
    uint64_t at = 0;
    for (int k = 0; k < num_textures; ++k) {
        texture_plan(h_textures[k].width, h_textures[k].height, at, h_textures[k].levels, h_textures[k].level_offset);
        h_textures[k].reserved = 0;
    }
    *pool_texels = at;
    return GS_OK;
}

int gs_texture_build_mips(int32_t num_textures, const GsTextureDesc* h_textures, const GsTextureDesc* textures, uint32_t* pool, uint64_t pool_texels,
                          gs_stream_t stream)
{
    if (num_textures < 0) return fail(GS_EINVAL, "gs_texture_build_mips: num_textures must not be negative");
    if (num_textures == 0) return GS_OK;
    if (!h_textures || !textures || !pool || ((uintptr_t)textures & 7) || ((uintptr_t)pool & 3))
        return fail(GS_EINVAL, "gs_texture_build_mips: null pointer, table not 8-byte aligned or pool not 4-byte aligned");
    const int rc = texture_table_checked("gs_texture_build_mips", num_textures, h_textures, pool_texels);
    if (rc != GS_OK) return rc;
    if (num_textures > 65535) return fail(GS_EINVAL, "gs_texture_build_mips: at most 65535 textures");
    return launched("gs_texture_build_mips", "", gs::launch_texture_mips(num_textures, h_textures, textures, pool, (hipStream_t)stream));
}

int gs_mesh_render_textured(int32_t num_vertices, const float* vertices, int32_t num_triangles, const int32_t* triangles, const uint8_t* vertex_colors,
                            const float* h_intrinsics4, const float* h_w2c12, float near_z, int32_t width, int32_t height, void* scratch,
                            uint32_t capacity, float* depth, int32_t* tri_id, uint8_t* color, uint32_t* d_counts, const float* uvs,
                            const int32_t* tri_texture, int32_t num_textures, const GsTextureDesc* h_textures, const GsTextureDesc* textures,
                            const uint32_t* pool, uint64_t pool_texels, gs_stream_t stream)
{
    gs::MeshArgs a;
    int rc = mesh_args_checked("gs_mesh_render_textured", num_vertices, vertices, num_triangles, triangles, vertex_colors, h_intrinsics4, h_w2c12, near_z,
                               width, height, scratch, capacity, depth, tri_id, color, d_counts, a);
    if (rc != GS_OK) return rc;
    if (num_textures < 0) return fail(GS_EINVAL, "gs_mesh_render_textured: num_textures must not be negative");
    if (num_textures > 0) {
        if (!h_textures || !textures || !pool || (num_triangles > 0 && (!uvs || !tri_texture)) || ((uintptr_t)uvs & 7) || ((uintptr_t)textures & 7) ||
            ((uintptr_t)pool & 3))
            return fail(GS_EINVAL, "gs_mesh_render_textured: null pointer (uvs, tri_texture, the two tables and the pool may be null only with num_textures == 0), "
                                   "uvs or table not 8-byte aligned, or pool not 4-byte aligned");
        rc = texture_table_checked("gs_mesh_render_textured", num_textures, h_textures, pool_texels);
        if (rc != GS_OK) return rc;
    }
    return launched("gs_mesh_render_textured", "", gs::launch_mesh_render_textured(a, uvs, tri_texture, num_textures, textures, pool, (hipStream_t)stream));
}

static bool nearest_size_ok(int64_t n) { return n >= 0 && n <= ((int64_t)1 << 30); }

uint64_t gs_cloud_nearest_scratch_bytes(int64_t n_query, int64_t n_points)
{
    if (!nearest_size_ok(n_query) || !nearest_size_ok(n_points)) return 0;
    return align_up(gs::cloud_nearest_scratch_bytes(n_query, n_points) + 4);
}

int gs_cloud_nearest(int64_t n_query, const float* query, const uint8_t* query_valid, int64_t n_points, const float* points,
                     const uint8_t* points_valid, int32_t flags, float* out, void* scratch, gs_stream_t stream)
{
    if (!nearest_size_ok(n_query) || !nearest_size_ok(n_points))
        return fail(GS_EINVAL, "gs_cloud_nearest: size out of range (0 <= n_query, n_points <= 2^30)");
    if (flags & ~(GS_NEAREST_ACCUMULATE | GS_NEAREST_ROOT)) return fail(GS_EINVAL, "gs_cloud_nearest: unknown flag");
    if (n_query == 0) return GS_OK;
    if (!query || !out || !scratch || (n_points > 0 && !points) || ((uintptr_t)scratch & 3))
        return fail(GS_EINVAL, "gs_cloud_nearest: null pointer (only query_valid and points_valid may be null) or scratch not 4-byte aligned");
    return launched("gs_cloud_nearest", "", gs::launch_cloud_nearest(n_query, query, query_valid, n_points, points, points_valid, flags, out, scratch, (hipStream_t)stream));
}

uint64_t gs_completion_row_scratch_bytes(void) { return align_up(gs::completion_row_scratch_bytes()); }

int gs_completion_row(int64_t n_samples, const float* min_dist, int64_t n_acc, const float* acc_dist, const uint8_t* acc_valid,
                      double path_length, double* row6, void* scratch, gs_stream_t stream)
{
    if (n_samples < 1 || !nearest_size_ok(n_samples) || !nearest_size_ok(n_acc))
        return fail(GS_EINVAL, "gs_completion_row: size out of range (1 <= n_samples <= 2^30, 0 <= n_acc <= 2^30)");
    if (!min_dist || !row6 || !scratch || (n_acc > 0 && !acc_dist) || ((uintptr_t)scratch & 7) || ((uintptr_t)row6 & 7))
        return fail(GS_EINVAL, "gs_completion_row: null pointer (only acc_valid may be null), or scratch / row6 not 8-byte aligned");
    return launched("gs_completion_row", "", gs::launch_completion_row(n_samples, min_dist, n_acc, acc_dist, acc_valid, path_length, row6, scratch, (hipStream_t)stream));
}

static int eval_plan_checked(const char* who, int32_t width, int32_t height, int32_t flags, gs::EvalPlan& p)
{
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail(GS_EINVAL, "%s: image size out of range (1 <= width, height <= 16384)", who);
    if (flags & ~(GS_EVAL_SIL_MASK | GS_EVAL_IMAGE_VALID_MASK | GS_EVAL_SSIM | GS_EVAL_MS_SSIM)) return fail(GS_EINVAL, "%s: unknown flag", who);
    if (!gs::eval_plan(width, height, flags, p))
        return fail(GS_EINVAL, "%s: GS_EVAL_MS_SSIM needs min(width, height) > 160 (five scales of an 11-tap valid window)", who);
    return GS_OK;
}

int gs_eval_frame_layout(int32_t width, int32_t height, int32_t flags, GsEvalLayout* layout)
{
    if (!layout) return fail(GS_EINVAL, "gs_eval_frame_layout: null pointer");
    gs::EvalPlan p;
    // (the layout call answers "is MS-SSIM defined here" instead of refusing: the plan is made without that flag when it is not)
    const bool ms_ok = width >= 1 && height >= 1 && (width < height ? width : height) > 160;
    const int rc = eval_plan_checked("gs_eval_frame_layout", width, height, ms_ok ? flags : (flags & ~GS_EVAL_MS_SSIM), p);
    if (rc != GS_OK) return rc;
    layout->total_bytes = align_up(p.total_bytes);
    layout->ms_ssim_defined = p.ms_defined;
    layout->levels = p.levels;
    for (int l = 0; l < 5; l++) { layout->level_width[l] = p.w[l]; layout->level_height[l] = p.h[l]; }
    return GS_OK;
}

int gs_eval_frame(int32_t width, int32_t height, const float* im, const float* depth, const float* silhouette, const float* gt_im,
                  const float* gt_depth, float sil_thres, int32_t flags, double* row, void* scratch, gs_stream_t stream)
{
    gs::EvalPlan p;
    const int rc = eval_plan_checked("gs_eval_frame", width, height, flags, p);
    if (rc != GS_OK) return rc;
    if (!im || !depth || !silhouette || !gt_im || !gt_depth || !row || !scratch || ((uintptr_t)scratch & 7) || ((uintptr_t)row & 7))
        return fail(GS_EINVAL, "gs_eval_frame: null pointer, or scratch / row not 8-byte aligned");
    return launched("gs_eval_frame", "", gs::launch_eval_frame(p, im, depth, silhouette, gt_im, gt_depth, sil_thres, flags, row, scratch, (hipStream_t)stream));
}

// ---- planner roadmap (stats.hip) ----
static int road_grid_checked(const char* who, int32_t H, int32_t W, gs::RoadGrid& g)
{
    if (H < 1 || W < 1 || H > gs::kRoadMaxSide || W > gs::kRoadMaxSide) return fail(GS_EINVAL, "%s: map size out of range (1 <= H, W <= 4096)", who);
    g.H = H; g.W = W; g.npix = H * W;
    return GS_OK;
}

uint64_t gs_roadmap_scratch_bytes(int32_t H, int32_t W)
{
    gs::RoadGrid g;
    if (road_grid_checked("gs_roadmap_scratch_bytes", H, W, g) != GS_OK) return 0;
    return 2 * align_up((uint64_t)g.npix) + align_up(4 * (uint64_t)g.npix) + 256;      // two byte maps, one int32 map, the relaxation's four words
}

int gs_traversable_map(int32_t H, int32_t W, const uint8_t* free_map, const uint8_t* unseen, int32_t agent_r, int32_t agent_c, int32_t open_size,
                       int32_t dilate, uint8_t* trav, void* scratch, uint32_t* d_status, gs_stream_t stream)
{
    gs::TravArgs a;
    const int rc = road_grid_checked("gs_traversable_map", H, W, a.g);
    if (rc != GS_OK) return rc;
    if (!free_map || !unseen || !trav || !scratch || !d_status || ((uintptr_t)scratch & 15) || ((uintptr_t)d_status & 3))
        return fail(GS_EINVAL, "gs_traversable_map: null pointer, scratch not 16-byte aligned or d_status not 4-byte aligned");
    if (agent_r < 0 || agent_r >= H || agent_c < 0 || agent_c >= W) return fail(GS_EINVAL, "gs_traversable_map: the agent's pixel must lie in the image");
    if (open_size < 1 || open_size > 16) return fail(GS_EINVAL, "gs_traversable_map: 1 <= open_size <= 16");
    if (dilate < 1 || dilate > 15 || !(dilate & 1)) return fail(GS_EINVAL, "gs_traversable_map: dilate must be odd, 1 <= dilate <= 15");
    const uint64_t map_bytes = align_up((uint64_t)a.g.npix);
    a.free_map = free_map; a.unseen = unseen; a.agent = agent_r * W + agent_c; a.open_size = open_size; a.dilate = dilate;
    a.map_a = (uint8_t*)scratch; a.map_b = a.map_a + map_bytes; a.parent = (uint32_t*)(a.map_a + 2 * map_bytes);
    a.out = trav; a.status = d_status;
    return launched("gs_traversable_map", "", gs::launch_traversable_map(a, (hipStream_t)stream));
}

int gs_clearance_field(int32_t H, int32_t W, const uint8_t* trav, int32_t* dist2, int16_t* feature, void* scratch, gs_stream_t stream)
{
    gs::RoadGrid g;
    const int rc = road_grid_checked("gs_clearance_field", H, W, g);
    if (rc != GS_OK) return rc;
    if (!trav || !dist2 || !feature || !scratch || ((uintptr_t)scratch & 15) || ((uintptr_t)dist2 & 3) || ((uintptr_t)feature & 1))
        return fail(GS_EINVAL, "gs_clearance_field: null pointer, scratch not 16-byte aligned, dist2 not 4-byte or feature not 2-byte aligned");
    return launched("gs_clearance_field", "", gs::launch_clearance_field(g, trav, (int32_t*)scratch, dist2, feature, (hipStream_t)stream));
}

int gs_voronoi_roadmap(int32_t H, int32_t W, const uint8_t* trav, const int32_t* dist2, const int16_t* feature, int32_t min_dist2, int32_t gamma2,
                       uint8_t* roadmap, gs_stream_t stream)
{
    gs::RoadGrid g;
    const int rc = road_grid_checked("gs_voronoi_roadmap", H, W, g);
    if (rc != GS_OK) return rc;
    if (!trav || !dist2 || !feature || !roadmap || ((uintptr_t)dist2 & 3) || ((uintptr_t)feature & 1))
        return fail(GS_EINVAL, "gs_voronoi_roadmap: null pointer, dist2 not 4-byte or feature not 2-byte aligned");
    if (min_dist2 < 0 || gamma2 < 0) return fail(GS_EINVAL, "gs_voronoi_roadmap: min_dist2 and gamma2 must not be negative");
    return launched("gs_voronoi_roadmap", "", gs::launch_voronoi_roadmap(g, trav, dist2, feature, min_dist2, gamma2, roadmap, (hipStream_t)stream));
}

int gs_grid_geodesic(int32_t H, int32_t W, const uint8_t* mask, int32_t seed_r, int32_t seed_c, const int32_t* d_seed_rc, int32_t* field,
                     void* scratch, uint32_t* d_status, int32_t* h_rounds, gs_stream_t stream)
{
    gs::RoadGrid g;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = road_grid_checked("gs_grid_geodesic", H, W, g);
    if (rc != GS_OK) return rc;
    if (!mask || !field || !scratch || !d_status || !h_rounds || ((uintptr_t)scratch & 15) || (((uintptr_t)field | (uintptr_t)d_status | (uintptr_t)d_seed_rc) & 3))
        return fail(GS_EINVAL, "gs_grid_geodesic: null pointer (d_seed_rc may be null), scratch not 16-byte aligned or an array not 4-byte aligned");
    int32_t* other = (int32_t*)scratch;
    uint32_t* words = (uint32_t*)((uint8_t*)scratch + align_up(4 * (uint64_t)g.npix));
    uint32_t h_words[4] = {0, 0, 0, 0};
    *h_rounds = 0;
    if (int e = launched("gs_grid_geodesic", "init", gs::launch_geodesic_init(g, mask, seed_r, seed_c, d_seed_rc, field, words, d_status, st))) return e;
    if (int e = launched("gs_grid_geodesic", "D2H", hipMemcpyAsync(h_words, words, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st))) return e;
    if (int e = launched("gs_grid_geodesic", "sync", hipStreamSynchronize(st))) return e;
    if (!h_words[2]) return GS_OK;                                       // seed outside the mask: all unreachable, status bit 1 raised
    const int64_t mask_pixels = h_words[1];
    // a round that changes something fixes the final value of at least one more mask pixel (the unfinished pixel nearest to the seed has a
    // finished neighbour on its shortest path, in its tile or in the halo), and the seed is final from the start: fewer than mask_pixels
    // rounds change anything.  The round that changes nothing ends the loop and is not counted; both buffers then hold the field.
    int32_t *src = field, *dst = other;
    for (int64_t rounds = 0;; rounds++) {
        if (rounds >= mask_pixels) return fail(GS_ECAPACITY, "gs_grid_geodesic: the relaxation did not settle within as many rounds as the mask has pixels");
        if (int e = launched("gs_grid_geodesic", "round", gs::launch_geodesic_round(g, mask, src, dst, words, st))) return e;
        if (int e = launched("gs_grid_geodesic", "D2H", hipMemcpyAsync(h_words, words, sizeof(uint32_t), hipMemcpyDeviceToHost, st))) return e;
        if (int e = launched("gs_grid_geodesic", "sync", hipStreamSynchronize(st))) return e;
        if (!h_words[0]) break;
        *h_rounds = (int32_t)(rounds + 1);
        int32_t* t = src; src = dst; dst = t;
    }
    return GS_OK;
}

int gs_roadmap_entry(int32_t H, int32_t W, const uint8_t* roadmap, const int32_t* field, int32_t* d_entry4, void* scratch, gs_stream_t stream)
{
    gs::RoadGrid g;
    const int rc = road_grid_checked("gs_roadmap_entry", H, W, g);
    if (rc != GS_OK) return rc;
    if (!roadmap || !field || !d_entry4 || !scratch || ((uintptr_t)scratch & 15) || (((uintptr_t)field | (uintptr_t)d_entry4) & 3))
        return fail(GS_EINVAL, "gs_roadmap_entry: null pointer, scratch not 16-byte aligned or an array not 4-byte aligned");
    return launched("gs_roadmap_entry", "", gs::launch_roadmap_entry(g, roadmap, field, scratch, d_entry4, (hipStream_t)stream));
}

int gs_roadmap_nodes(int32_t H, int32_t W, const uint8_t* roadmap, const int32_t* dist2, const int32_t* field, int32_t cell, int32_t* node_rc,
                     int32_t* node_dist2, int32_t* node_field, int32_t* d_count, void* scratch, gs_stream_t stream)
{
    gs::NodeArgs a;
    const int rc = road_grid_checked("gs_roadmap_nodes", H, W, a.g);
    if (rc != GS_OK) return rc;
    if (!roadmap || !dist2 || !field || !node_rc || !node_dist2 || !node_field || !d_count || !scratch || ((uintptr_t)scratch & 15) ||
        (((uintptr_t)dist2 | (uintptr_t)field | (uintptr_t)node_rc | (uintptr_t)node_dist2 | (uintptr_t)node_field | (uintptr_t)d_count) & 3))
        return fail(GS_EINVAL, "gs_roadmap_nodes: null pointer, scratch not 16-byte aligned or an array not 4-byte aligned");
    if (cell < 1 || cell > 64) return fail(GS_EINVAL, "gs_roadmap_nodes: 1 <= cell <= 64");
    a.roadmap = roadmap; a.dist2 = dist2; a.field = field; a.cell = cell;
    a.cells_y = (H + cell - 1) / cell; a.cells_x = (W + cell - 1) / cell;
    a.pick = (int32_t*)scratch;
    a.node_rc = node_rc; a.node_dist2 = node_dist2; a.node_field = node_field; a.count = d_count;
    return launched("gs_roadmap_nodes", "", gs::launch_roadmap_nodes(a, (hipStream_t)stream));
}

int gs_trace_path(int32_t H, int32_t W, const uint8_t* mask, const int32_t* field, int32_t target_r, int32_t target_c, const int32_t* d_target_rc,
                  int32_t capacity, int32_t* path_rc, int32_t* d_count2, gs_stream_t stream)
{
    gs::RoadGrid g;
    const int rc = road_grid_checked("gs_trace_path", H, W, g);
    if (rc != GS_OK) return rc;
    if (capacity < 0) return fail(GS_EINVAL, "gs_trace_path: capacity must not be negative");
    if (!mask || !field || !d_count2 || (capacity > 0 && !path_rc) || (((uintptr_t)field | (uintptr_t)d_target_rc | (uintptr_t)path_rc | (uintptr_t)d_count2) & 3))
        return fail(GS_EINVAL, "gs_trace_path: null pointer (d_target_rc may be null; path_rc when capacity is 0) or an array not 4-byte aligned");
    return launched("gs_trace_path", "", gs::launch_trace_path(g, mask, field, target_r, target_c, d_target_rc, capacity, path_rc, d_count2, (hipStream_t)stream));
}

// ---- roadmap subregions (stats.hip) ----
static std::atomic<int> g_node_distance_path{GS_NODE_DISTANCES_AUTO};

int gs_set_node_distance_path(int32_t path)
{
    if (path < GS_NODE_DISTANCES_AUTO || path > GS_NODE_DISTANCES_GLOBAL) return fail(GS_EINVAL, "gs_set_node_distance_path: bad path");
    g_node_distance_path = path;
    return GS_OK;
}

uint64_t gs_node_distances_scratch_bytes(int32_t H, int32_t W)
{
    gs::RoadGrid g;
    if (road_grid_checked("gs_node_distances_scratch_bytes", H, W, g) != GS_OK) return 0;
    return gs::node_distances_scratch_bytes(g);
}

int gs_node_distances(int32_t H, int32_t W, const uint8_t* roadmap, int32_t K, const int32_t* node_rc, int32_t* D, void* scratch, gs_stream_t stream)
{
    gs::NodeDistArgs a;
    const int rc = road_grid_checked("gs_node_distances", H, W, a.g);
    if (rc != GS_OK) return rc;
    if (K < 0 || K > gs::kMaxNodes) return fail(GS_EINVAL, "gs_node_distances: node count out of range (0 <= K <= 1024)");
    if (!roadmap || !scratch || (K > 0 && (!node_rc || !D)) || ((uintptr_t)scratch & 15) || (((uintptr_t)node_rc | (uintptr_t)D) & 3))
        return fail(GS_EINVAL, "gs_node_distances: null pointer (node_rc and D when K is 0), scratch not 16-byte aligned or an array not 4-byte aligned");
    a.mask = roadmap; a.K = K; a.path = g_node_distance_path; a.node_rc = node_rc; a.D = D;
    gs::node_distances_carve(scratch, a);
    return launched("gs_node_distances", "", gs::launch_node_distances(a, (hipStream_t)stream));
}

int gs_segment_clearance(int32_t H, int32_t W, const int32_t* dist2, int32_t n, const int32_t* segments, int32_t* clearance, gs_stream_t stream)
{
    gs::RoadGrid g;
    const int rc = road_grid_checked("gs_segment_clearance", H, W, g);
    if (rc != GS_OK) return rc;
    if (n < 0 || n > (1 << 24)) return fail(GS_EINVAL, "gs_segment_clearance: segment count out of range (0 <= n <= 2^24)");
    if (!dist2 || (n > 0 && (!segments || !clearance)) || (((uintptr_t)dist2 | (uintptr_t)segments | (uintptr_t)clearance) & 3))
        return fail(GS_EINVAL, "gs_segment_clearance: null pointer (segments and clearance when n is 0) or an array not 4-byte aligned");
    return launched("gs_segment_clearance", "", gs::launch_segment_clearance(g, dist2, n, segments, clearance, (hipStream_t)stream));
}

uint64_t gs_subregions_scratch_bytes(int32_t K)
{
    if (K < 0 || K > gs::kMaxNodes) { fail(GS_EINVAL, "gs_subregions_scratch_bytes: node count out of range (0 <= K <= 1024)"); return 0; }
    return gs::subregions_scratch_bytes(K);
}

int gs_subregions(int32_t K, const int32_t* node_rc, const int32_t* D, double path_weight, double coord_weight, double threshold, int32_t* labels,
                  int32_t* d_count, double* heights, void* scratch, gs_stream_t stream)
{
    gs::SubregionArgs a;
    if (K < 0 || K > gs::kMaxNodes) return fail(GS_EINVAL, "gs_subregions: node count out of range (0 <= K <= 1024)");
    // (written so that a NaN fails them)
    if (!(path_weight >= 0.0 && path_weight <= 1.7976931348623157e308) || !(coord_weight >= 0.0 && coord_weight <= 1.7976931348623157e308) || !(threshold >= 0.0))
        return fail(GS_EINVAL, "gs_subregions: the weights must be finite and not negative, the threshold not negative");
    if (!d_count || !scratch || (K > 0 && (!node_rc || !D || !labels)) || (K > 1 && !heights) || (((uintptr_t)scratch | (uintptr_t)heights) & 7) ||
        (((uintptr_t)node_rc | (uintptr_t)D | (uintptr_t)labels | (uintptr_t)d_count) & 3))
        return fail(GS_EINVAL, "gs_subregions: null pointer (the arrays a K of 0 or 1 leaves empty may be null), scratch or heights not 8-byte aligned or an "
                               "array not 4-byte aligned");
    a.K = K; a.node_rc = node_rc; a.D = D; a.path_weight = path_weight; a.coord_weight = coord_weight; a.threshold = threshold;
    a.labels = labels; a.count = d_count; a.heights = heights;
    gs::subregions_carve(scratch, a);
    return launched("gs_subregions", "", gs::launch_subregions(a, (hipStream_t)stream));
}

}  // extern "C"
