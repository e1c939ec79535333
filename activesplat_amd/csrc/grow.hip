// grow.hip -- map growth and keyframe-overlap scoring, the two per-map-frame steps either side of the optimise loop
// (SURVEY.md section 8f-3).
//
// 1. add_new_gaussians (src/mapper/splatam/splatam.py:332-379, helpers get_pointcloud :25-75 and
//    initialize_new_params :304-329): from the rendered depth + silhouette of the current map and the sensor frame,
//      err          = |gt - render| * (gt > 0)
//      non_presence = sil < thr  |  (render > gt  &  err > 2 median(err)  &  sil > thr  &  gt < 5)
//    every non_presence pixel with valid depth becomes a Gaussian: mean = c2w * ((u-cx)/fx z, (v-cy)/fy z, z), colour =
//    pixel RGB, rotation (1,0,0,0), logit opacity 0, log scale = log(sqrt((z / ((fx+fy)/2))^2)).  The reference does this
//    with ~40 torch launches, a device-wide sort for the median and boolean-mask gathers; here: the exact radix
//    select of the median that the loss' outlier rejection uses (loss.hip, a grid of workgroups), one mask kernel,
//    the ordered compaction of compact.hip and one row-emitting kernel.  Row order = row-major pixel order, as
//    boolean-mask indexing yields.
// 2. keyframe_selection_overlap's scoring loop (src/mapper/splatam/utils/keyframe_selection.py:62-86): for every keyframe,
//    the number of sampled world points that project inside its image with a 20 px border -- one workgroup per keyframe
//    instead of ~12 torch launches and a blocking .sum() each.
#include "gs_common.h"

namespace gs {

// The median of err: torch.median of a flat tensor = the LOWER median, propagating NaN -- the exact select of loss.hip (launch_depth_error_median,
// shared with the loss' outlier rejection; depth_error itself is in gs_common.h).  If ANY error is NaN (a NaN in either depth image, or
// inf * 0 where gt <= 0) the median is NaN, `err > 2 median` is false everywhere and only the silhouette candidates remain.
__global__ __launch_bounds__(kBlock) void grow_mask_kernel(int64_t n, const float* __restrict__ gt, const float* __restrict__ rd,
                                                            const float* __restrict__ sil, const float* __restrict__ d_median,
                                                            float sil_thres, uint8_t* __restrict__ keep, uint32_t* __restrict__ d_candidates)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool cand = false, take = false;
    if (i < n) {
        const float g = gt[i], r = rd[i], s = sil[i];
        const bool behind = (r > g) && (depth_error(g, r) > 2.0f * d_median[0]);
        cand = (s < sil_thres) || (behind && (s > sil_thres) && (g < 5.0f));
        take = cand && (g > 0.0f);
        keep[i] = take ? 1 : 0;
    }
    // candidate count: 64 accumulator lines (thousands of same-address device atomics would serialise for ~70 us)
    const unsigned long long m = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(d_candidates + (blockIdx.x & 63) * 16, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(kWave) void grow_sum_slots_kernel(const uint32_t* __restrict__ slots, uint32_t* __restrict__ out)
{
    const uint32_t v = wave_sum_u32(slots[threadIdx.x * 16]);
    if (threadIdx.x == 0) *out = v;
}

struct GrowCam { float fx, fy, cx, cy; float c2w[12]; int W; int isotropic; };

__global__ __launch_bounds__(kBlock) void grow_rows_kernel(GrowCam c, int64_t npix, const uint32_t* __restrict__ d_count,
                                                            const uint32_t* __restrict__ index, const float* __restrict__ gt,
                                                            const float* __restrict__ color, float* __restrict__ means3D,
                                                            float* __restrict__ rgb, float* __restrict__ rot, float* __restrict__ logit,
                                                            float* __restrict__ log_scales)
{
    const int64_t count = (int64_t)*d_count;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < count; r += stride) {
        const uint32_t pix = index[r];
        const int u = (int)(pix % (uint32_t)c.W), v = (int)(pix / (uint32_t)c.W);
        const float z = gt[pix];
        const float x = ((float)u - c.cx) / c.fx * z;
        const float y = ((float)v - c.cy) / c.fy * z;
        means3D[3 * r + 0] = c.c2w[0] * x + c.c2w[1] * y + c.c2w[2] * z + c.c2w[3];
        means3D[3 * r + 1] = c.c2w[4] * x + c.c2w[5] * y + c.c2w[6] * z + c.c2w[7];
        means3D[3 * r + 2] = c.c2w[8] * x + c.c2w[9] * y + c.c2w[10] * z + c.c2w[11];
        rgb[3 * r + 0] = color[pix];
        rgb[3 * r + 1] = color[npix + pix];
        rgb[3 * r + 2] = color[2 * npix + pix];
        rot[4 * r + 0] = 1.0f; rot[4 * r + 1] = 0.0f; rot[4 * r + 2] = 0.0f; rot[4 * r + 3] = 0.0f;
        logit[r] = 0.0f;
        const float sd = z / ((c.fx + c.fy) / 2.0f);
        const float ls = logf(sqrtf(sd * sd));
        if (c.isotropic) log_scales[r] = ls;
        else { log_scales[3 * r + 0] = ls; log_scales[3 * r + 1] = ls; log_scales[3 * r + 2] = ls; }
    }
}

uint64_t grow_scratch_bytes(int64_t npix)
{   // keep mask | index list | median | candidate counters | the select's histograms | compaction block sums
    return (uint64_t)((npix + 255) / 256 * 256) + (uint64_t)npix * 4 + 256 + 64 * 64 + (uint64_t)kMedianScratchWords * 4 +
           compact_scratch_bytes(npix) + 256;
}

hipError_t launch_grow(int W, int H, const float* rd, const float* sil, const float* gt, const float* color, const float* k4,
                       const float* c2w12, float sil_thres, int isotropic, float* means3D, float* rgb, float* rot, float* logit,
                       float* log_scales, uint32_t* d_counts, void* scratch, hipStream_t st)
{
    const int64_t n = (int64_t)W * H;
    uint8_t* keep = (uint8_t*)scratch;
    uint32_t* index = (uint32_t*)(keep + (n + 255) / 256 * 256);
    float* med = (float*)(index + n);
    uint32_t* slots = (uint32_t*)(med + 64);                 // 64 lines of candidate counters
    uint32_t* hists = slots + 64 * 16;
    void* cscr = (void*)(hists + kMedianScratchWords);
    hipError_t e = hipMemsetAsync(slots, 0, 64 * 64, st);
    if (e != hipSuccess) return e;
    e = launch_depth_error_median(n, rd, gt, hists, med, 0, st);
    if (e != hipSuccess) return e;
    const int nb = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(grow_mask_kernel, dim3(nb), dim3(kBlock), 0, st, n, gt, rd, sil, (const float*)med, sil_thres, keep, slots);
    hipLaunchKernelGGL(grow_sum_slots_kernel, dim3(1), dim3(kWave), 0, st, (const uint32_t*)slots, d_counts);
    e = launch_compact_index(n, keep, index, d_counts + 1, cscr, st);
    if (e != hipSuccess) return e;
    GrowCam c;
    c.fx = k4[0]; c.fy = k4[1]; c.cx = k4[2]; c.cy = k4[3]; c.W = W; c.isotropic = isotropic;
    for (int i = 0; i < 12; ++i) c.c2w[i] = c2w12[i];
    int nbr = nb > 256 * 4 ? 256 * 4 : nb;
    hipLaunchKernelGGL(grow_rows_kernel, dim3(nbr), dim3(kBlock), 0, st, c, n, (const uint32_t*)(d_counts + 1), (const uint32_t*)index, gt,
                       color, means3D, rgb, rot, logit, log_scales);
    return hipGetLastError();
}

// ---- keyframe overlap ------------------------------------------------------------------------------------------------
struct OverlapCam { float k[9]; float w, h, edge; };

__global__ __launch_bounds__(kBlock) void keyframe_overlap_kernel(OverlapCam c, int n_pts, const float* __restrict__ pts,
                                                                   const float* __restrict__ w2c, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_sum;
    const float* m = w2c + 16 * (int64_t)blockIdx.x;            // row-major 4x4 estimated w2c of keyframe blockIdx.x
    if (threadIdx.x == 0) s_sum = 0u;
    __syncthreads();
    uint32_t mine = 0;
    for (int i = threadIdx.x; i < n_pts; i += kBlock) {
        const float X = pts[3 * i], Y = pts[3 * i + 1], Z = pts[3 * i + 2];
        const float x = m[0] * X + m[1] * Y + m[2] * Z + m[3];
        const float y = m[4] * X + m[5] * Y + m[6] * Z + m[7];
        const float z = m[8] * X + m[9] * Y + m[10] * Z + m[11];
        const float px = c.k[0] * x + c.k[1] * y + c.k[2] * z;
        const float py = c.k[3] * x + c.k[4] * y + c.k[5] * z;
        const float pz = (c.k[6] * x + c.k[7] * y + c.k[8] * z) + 1e-5f;
        const float u = px / pz, v = py / pz;
        if (u < c.w - c.edge && u > c.edge && v < c.h - c.edge && v > c.edge && pz > 0.0f) ++mine;
    }
    const unsigned long long any = __ballot(mine != 0);
    if (any) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_sum;
}

hipError_t launch_keyframe_overlap(int n_pts, const float* pts, int n_kf, const float* w2c, const float* k9, int W, int H, int edge,
                                   uint32_t* counts, hipStream_t st)
{
    if (n_kf <= 0) return hipSuccess;
    OverlapCam c;
    for (int i = 0; i < 9; ++i) c.k[i] = k9[i];
    c.w = (float)W; c.h = (float)H; c.edge = (float)edge;
    hipLaunchKernelGGL(keyframe_overlap_kernel, dim3(n_kf), dim3(kBlock), 0, st, c, n_pts, pts, w2c, counts);
    return hipGetLastError();
}

// ---- frame ingest (src/mapper/splatam/__init__.py:341-376; the rules: include/gsplat_hip.h, gs_frame_ingest) -------------------------
// The raw sensor frame -- interleaved uint8 RGB and fp32 depth -- resized to one or two resolutions in ONE launch: bilinear colour at pixel
// centres in fp64 with every operation rounded on its own (the host's numpy expression, operation for operation), rounded half up to a grey
// level and looked up in level_value[256]; nearest depth with the fp64 index rule, its 32 bits copied.  One thread per destination pixel; the
// workgroups of output 0 come first, then those of output 1, so the choice of output is uniform over a workgroup.  A gather: 12 source bytes and
// three coalesced planar stores per colour sample, no LDS, no atomics, no scratch.
struct IngestOut { float* color; uint32_t* depth; double rx, ry; int W, H; unsigned blocks; int pad; };   // rx = double(w) / double(W), host-divided
struct IngestArgs { const uint8_t* image; const uint32_t* depth; const float* level_value; int w, h; IngestOut o[2]; };

// (d + 0.5) * r - 0.5 -> the two clamped taps and the weight of the second; contraction is off in the caller
__device__ __forceinline__ void ingest_axis(int d, double r, int n_src, int& i0, int& i1, double& f)
{
#pragma clang fp contract(off)
    const double c = ((double)d + 0.5) * r - 0.5;
    const double fl = floor(c);
    f = c - fl;
    const int i = (int)fl;                                       // >= -1: c >= 0.5 r - 0.5 > -0.5
    i0 = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);
    i1 = i + 1 < 0 ? 0 : (i + 1 > n_src - 1 ? n_src - 1 : i + 1);
}

__global__ __launch_bounds__(kBlock) void frame_ingest_kernel(IngestArgs a)
{
    // the product build of this file allows FMA contraction; the colour rule is separately rounded operations (the header says why no test sees it)
#pragma clang fp contract(off)
    const bool second = blockIdx.x >= a.o[0].blocks;
    const unsigned block = second ? blockIdx.x - a.o[0].blocks : blockIdx.x;
    const int W = second ? a.o[1].W : a.o[0].W, H = second ? a.o[1].H : a.o[0].H;
    const double rx = second ? a.o[1].rx : a.o[0].rx, ry = second ? a.o[1].ry : a.o[0].ry;
    float* __restrict__ color = second ? a.o[1].color : a.o[0].color;
    uint32_t* __restrict__ depth = second ? a.o[1].depth : a.o[0].depth;
    const int64_t n = (int64_t)W * H;
    const int64_t p = (int64_t)block * kBlock + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % W), y = (int)(p / W);
    // depth: floor(y * (h / H)) in fp64, clamped; never (y * h) / H in integers (the two differ, e.g. 2 -> 98)
    int sy = (int)floor((double)y * ry), sx = (int)floor((double)x * rx);
    sy = sy < a.h - 1 ? sy : a.h - 1;
    sx = sx < a.w - 1 ? sx : a.w - 1;
    depth[p] = a.depth[(int64_t)sy * a.w + sx];
    int x0, x1, y0, y1;
    double fx, fy;
    ingest_axis(x, rx, a.w, x0, x1, fx);
    ingest_axis(y, ry, a.h, y0, y1, fy);
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const uint8_t* __restrict__ r0 = a.image + (int64_t)y0 * a.w * 3;
    const uint8_t* __restrict__ r1 = a.image + (int64_t)y1 * a.w * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double ta = (double)r0[3 * x0 + ch], tb = (double)r0[3 * x1 + ch];
        const double tc = (double)r1[3 * x0 + ch], td = (double)r1[3 * x1 + ch];
        const double top = ta * gx + tb * fx;
        const double bot = tc * gx + td * fx;
        const double o = top * gy + bot * fy;
        const double l = floor(o + 0.5);
        const int level = l < 0.0 ? 0 : (l > 255.0 ? 255 : (int)l);
        color[(int64_t)ch * n + p] = a.level_value[level];
    }
}

hipError_t launch_frame_ingest(int w, int h, const uint8_t* image, const float* depth, const float* level_value, int n_out, const int* sizes,
                               float* const* colors, float* const* depths, hipStream_t st)
{
    IngestArgs a;
    a.image = image; a.depth = (const uint32_t*)depth; a.level_value = level_value; a.w = w; a.h = h;
    unsigned blocks = 0;
    for (int k = 0; k < 2; ++k) {
        IngestOut& o = a.o[k];
        if (k < n_out) {
            o.W = sizes[2 * k]; o.H = sizes[2 * k + 1];
            o.color = colors[k]; o.depth = (uint32_t*)depths[k];
            o.rx = (double)w / (double)o.W; o.ry = (double)h / (double)o.H;
            o.blocks = (unsigned)(((int64_t)o.W * o.H + kBlock - 1) / kBlock);
        } else {
            o.W = o.H = 0; o.color = nullptr; o.depth = nullptr; o.rx = o.ry = 1.0; o.blocks = 0;
        }
        o.pad = 0;
        blocks += o.blocks;
    }
    hipLaunchKernelGGL(frame_ingest_kernel, dim3(blocks), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

// ---- completion / accuracy judge (scripts/judges/eval_actions.py:33-40,139-152) ------------------------------------------------------
// The reference builds two KD-trees per frame -- one over the frame's back-projected cloud, queried with the 200 000 mesh samples, one over the
// samples, queried with the cloud -- keeps two running minima per sample and writes a row of six means per frame.  Here: the back-projection
// (rgbd_to_pointcloud, src/utils/gui_utils.py:96-125, restated in include/gsplat_hip.h), an exact brute-force nearest-distance kernel for both
// directions, and a fixed-order fp64 reduction of the row.  No atomics anywhere: a min is exact, the sums are trees, two calls give the same bits.
struct CloudCam { float fx, fy, cx, cy; float c2w[12]; int W; };

__global__ __launch_bounds__(kBlock) void depth_cloud_kernel(CloudCam c, int64_t npix, const float* __restrict__ depth, float* __restrict__ points,
                                                              uint8_t* __restrict__ valid)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= npix) return;
    // the uint16 millimetre image the reference hands to Open3D; written so that a NaN fails the test
    const float q = truncf(depth[i] * 1000.0f);
    const bool ok = q >= 1.0f && q <= 65535.0f;
    float X = 0.0f, Y = 0.0f, Z = 0.0f;
    if (ok) {
        const int u = (int)(i % c.W), v = (int)(i / c.W);
        const float z = q / 1000.0f;
        const float x = ((float)u - c.cx) * z / c.fx;
        const float y = ((float)v - c.cy) * z / c.fy;
        X = c.c2w[0] * x + c.c2w[1] * y + c.c2w[2] * z + c.c2w[3];
        Y = c.c2w[4] * x + c.c2w[5] * y + c.c2w[6] * z + c.c2w[7];
        Z = c.c2w[8] * x + c.c2w[9] * y + c.c2w[10] * z + c.c2w[11];
    }
    points[3 * i + 0] = X; points[3 * i + 1] = Y; points[3 * i + 2] = Z;
    valid[i] = ok ? 1 : 0;
}

hipError_t launch_depth_cloud(int W, int H, const float* depth, const float* k4, const float* c2w12, float* points, uint8_t* valid, hipStream_t st)
{
    const int64_t n = (int64_t)W * H;
    CloudCam c;
    c.fx = k4[0]; c.fy = k4[1]; c.cx = k4[2]; c.cy = k4[3]; c.W = W;
    for (int i = 0; i < 12; ++i) c.c2w[i] = c2w12[i];
    hipLaunchKernelGGL(depth_cloud_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, c, n, depth, points, valid);
    return hipGetLastError();
}

// Nearest squared distance, brute force, N-body style: a lane keeps kNnQ queries and their running minima in registers, the workgroup stages
// kNnTile streamed points in LDS and every lane reads each of them once (one broadcast ds_read_b128 per point and wavefront) for its kNnQ
// queries: seven vector operations per pair (three differences, a product, two FMAs, a min) and nothing else in the loop -- and the first six of
// them are packed fp32 instructions that serve two queries each (the loop compiles to 3 v_pk_add_f32, 1 v_pk_mul_f32, 2 v_pk_fma_f32 and one
// v_min3_f32 per two pairs).  Written with the vector type on purpose: the scalar form is re-associated by the SLP vectoriser into a mix of packed
// and plain instructions with register moves in the loop.  A packed instruction takes the time of two plain ones here, so this form and a
// purely scalar one (measured with packed fp32 switched off for the kernel) run within 1.5 % of each other (profiles/completion_judge.txt).  The grid is
// (blocks of kNnGroup queries) x (pieces of the streamed set): the pieces are sized so that both of the judge's directions -- 200 000 queries
// against 16 384 points, and the reverse -- put about kNnWorkgroups workgroups on the chip: seven per CU, what the kernel's 72 registers let a CU
// hold at once, so that no workgroup waits for another to finish.  Every workgroup writes the minima
// of its piece to partial[piece][query]; the combine kernel takes the min over the pieces, which is exact in any order.
// The arithmetic is the difference form: |q|^2 + |p|^2 - 2 q.p cancels at room coordinates (in fp32 it is wrong by more than the distance itself at
// centimetre distances in a 6 m room).
constexpr int kNnQ = 8;
constexpr int kNnTile = 256;
constexpr int kNnGroup = kBlock * kNnQ;
constexpr int kNnWorkgroups = 7 * 256;
constexpr int kNnMaxPieces = 2048;

typedef float nn_f2 __attribute__((vector_size(8)));

struct NnPlan { int64_t qblocks, pieces, chunk; };
static NnPlan nn_plan(int64_t Q, int64_t M)
{
    NnPlan p;
    p.qblocks = (Q + kNnGroup - 1) / kNnGroup;
    int64_t pieces = p.qblocks > 0 ? kNnWorkgroups / p.qblocks : 1;
    const int64_t most = (M + kNnTile - 1) / kNnTile;           // no piece shorter than one tile
    if (pieces > most) pieces = most;
    if (pieces > kNnMaxPieces) pieces = kNnMaxPieces;
    if (pieces < 1) pieces = 1;
    p.chunk = (M + pieces - 1) / pieces;
    p.pieces = p.chunk > 0 ? (M + p.chunk - 1) / p.chunk : 1;   // (pieces that would start beyond M are not launched)
    if (p.pieces < 1) p.pieces = 1;
    return p;
}

uint64_t cloud_nearest_scratch_bytes(int64_t Q, int64_t M)
{
    const NnPlan p = nn_plan(Q, M);
    return (uint64_t)p.pieces * (uint64_t)Q * 4u;
}

__global__ __launch_bounds__(kBlock) void cloud_nearest_kernel(int64_t Q, const float* __restrict__ query, int64_t M, const float* __restrict__ points,
                                                                const uint8_t* __restrict__ pvalid, int64_t chunk, float* __restrict__ partial)
{
    __shared__ float4 s_pt[kNnTile];
    const float inf = __uint_as_float(0x7f800000u);
    const int64_t q0 = (int64_t)blockIdx.x * kNnGroup + threadIdx.x;
    // two queries per register pair: the differences, the product and the two FMAs of a pair of queries are one packed fp32 instruction each
    nn_f2 qx[kNnQ / 2], qy[kNnQ / 2], qz[kNnQ / 2];
    float best[kNnQ];
#pragma unroll
    for (int j = 0; j < kNnQ; ++j) {
        const int64_t q = q0 + (int64_t)j * kBlock;
        const bool in = q < Q;
        qx[j >> 1][j & 1] = in ? query[3 * q + 0] : 0.0f;
        qy[j >> 1][j & 1] = in ? query[3 * q + 1] : 0.0f;
        qz[j >> 1][j & 1] = in ? query[3 * q + 2] : 0.0f;
        best[j] = inf;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk;
    const int64_t p1 = p0 + chunk < M ? p0 + chunk : M;
    for (int64_t base = p0; base < p1; base += kNnTile) {
        const int n = p1 - base < kNnTile ? (int)(p1 - base) : kNnTile;
        __syncthreads();                                        // the tile before this one has been read by every wavefront
        if ((int)threadIdx.x < n) {
            const int64_t p = base + threadIdx.x;
            // an invalid point sits at infinity: its distance to any finite query is inf, and a NaN (an infinite query) never wins an fminf
            const bool ok = pvalid == nullptr || pvalid[p] != 0;
            s_pt[threadIdx.x] = ok ? make_float4(points[3 * p + 0], points[3 * p + 1], points[3 * p + 2], 0.0f) : make_float4(inf, inf, inf, 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 p = s_pt[k];
#pragma unroll
            for (int j = 0; j < kNnQ / 2; ++j) {
                const nn_f2 dx = qx[j] - p.x, dy = qy[j] - p.y, dz = qz[j] - p.z;
                const nn_f2 d = dx * dx + dy * dy + dz * dz;
                best[2 * j] = fminf(best[2 * j], d[0]);
                best[2 * j + 1] = fminf(best[2 * j + 1], d[1]);
            }
        }
    }
    float* row = partial + (int64_t)blockIdx.y * Q;
#pragma unroll
    for (int j = 0; j < kNnQ; ++j) {
        const int64_t q = q0 + (int64_t)j * kBlock;
        if (q < Q) row[q] = best[j];
    }
}

__global__ __launch_bounds__(kBlock) void cloud_nearest_combine_kernel(int64_t Q, int pieces, const float* __restrict__ partial,
                                                                        const uint8_t* __restrict__ qvalid, int flags, float* __restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= Q) return;
    if (qvalid != nullptr && qvalid[q] == 0) return;            // an invalid query's output is left as it was
    float m = partial[q];
    for (int s = 1; s < pieces; ++s) m = fminf(m, partial[(int64_t)s * Q + q]);
    if (flags & GS_NEAREST_ROOT) m = sqrtf(m);
    if (flags & GS_NEAREST_ACCUMULATE) m = fminf(out[q], m);
    out[q] = m;
}

hipError_t launch_cloud_nearest(int64_t Q, const float* query, const uint8_t* qvalid, int64_t M, const float* points, const uint8_t* pvalid,
                                int flags, float* out, void* scratch, hipStream_t st)
{
    if (Q <= 0) return hipSuccess;
    const NnPlan p = nn_plan(Q, M);
    float* partial = (float*)scratch;
    hipLaunchKernelGGL(cloud_nearest_kernel, dim3((unsigned)p.qblocks, (unsigned)p.pieces), dim3(kBlock), 0, st, Q, query, M, points, pvalid, p.chunk,
                       partial);
    hipLaunchKernelGGL(cloud_nearest_combine_kernel, dim3((unsigned)((Q + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, Q, (int)p.pieces,
                       (const float*)partial, qvalid, flags, out);
    return hipGetLastError();
}

// The judge's row (eval_actions.py:142-149).  Partial sums in fp64: every thread adds its elements in index order (stride = the grid), the pairwise
// tree of gs_common.h over the workgroup's kBlock partials, one record per workgroup; a second single-workgroup launch runs the same tree over the records.
// The grid depends on the sizes alone, so the order of every addition is fixed.
constexpr int kRowVals = 5;                 // sum min(1, d) | count d < 0.05 | sum d | sum of the accuracy distances | their count
constexpr int kRowStride = 8;               // doubles per record
constexpr int kRowGridMax = kBlock;         // the second launch reads one record per thread

__global__ __launch_bounds__(kBlock) void completion_partial_kernel(int64_t N, const float* __restrict__ min_d, int64_t P, const float* __restrict__ acc_d,
                                                                     const uint8_t* __restrict__ acc_valid, double* __restrict__ partial)
{
    __shared__ double s_tree[kRowVals][kBlock];
    double a[kRowVals] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
        const float d = min_d[i];
        a[0] += (double)fminf(d, 1.0f);
        a[1] += (double)d < 0.05 ? 1.0 : 0.0;                   // the fp32 distance widened, against the double 0.05
        a[2] += (double)d;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += stride) {
        if (acc_valid == nullptr || acc_valid[i] != 0) { a[3] += (double)acc_d[i]; a[4] += 1.0; }
    }
    block_tree_sum(a, s_tree);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kRowVals; ++k) partial[(int64_t)blockIdx.x * kRowStride + k] = a[k];
    }
}

__global__ __launch_bounds__(kBlock) void completion_finish_kernel(int records, const double* __restrict__ partial, int64_t N, double path_length,
                                                                    double* __restrict__ row)
{
    __shared__ double s_tree[kRowVals][kBlock];
    double a[kRowVals] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if ((int)threadIdx.x < records) {
#pragma unroll
        for (int k = 0; k < kRowVals; ++k) a[k] = partial[(int64_t)threadIdx.x * kRowStride + k];
    }
    block_tree_sum(a, s_tree);
    if (threadIdx.x != 0) return;
    const double n = (double)N;
    row[0] = a[0] / n;                      // completion error, capped at 1 m
    row[1] = a[1] / n;                      // completion ratio (min(1, d) < 0.05 iff d < 0.05)
    row[2] = a[2] / n;                      // ... uncapped: inf while a sample is unseen
    row[3] = a[1] / n;
    row[4] = path_length;
    row[5] = a[3] / a[4];                   // accuracy of this frame; 0 / 0 = NaN for a frame without a valid pixel
}

static int completion_records(int64_t N, int64_t P)
{
    const int64_t most = N > P ? N : P;
    const int64_t g = (most + 4 * kBlock - 1) / (4 * kBlock);   // at least four elements per thread before another workgroup is worth its launch
    return g < 1 ? 1 : g > kRowGridMax ? kRowGridMax : (int)g;
}

uint64_t completion_row_scratch_bytes() { return (uint64_t)kRowGridMax * kRowStride * 8u; }

hipError_t launch_completion_row(int64_t N, const float* min_d, int64_t P, const float* acc_d, const uint8_t* acc_valid, double path_length,
                                 double* row, void* scratch, hipStream_t st)
{
    const int g = completion_records(N, P);
    double* partial = (double*)scratch;
    hipLaunchKernelGGL(completion_partial_kernel, dim3(g), dim3(kBlock), 0, st, N, min_d, P, acc_d, acc_valid, partial);
    hipLaunchKernelGGL(completion_finish_kernel, dim3(1), dim3(kBlock), 0, st, g, (const double*)partial, N, path_length, row);
    return hipGetLastError();
}

// ---- mesh RGB-D sensor (the frame the reference takes from Habitat-sim, src/dataloader/dataloader.py:168-235; the rendering rule:
// include/gsplat_hip.h, gs_mesh_render) ----------------------------------------------------------------------------------------------
// A vertex-coloured triangle mesh rendered to planar depth, triangle id and colour by ray casting through per-tile triangle lists:
//   setup  one thread per triangle: camera-frame vertices, the three edge normals p_i x p_j of the rule (lower vertex index first, separately
//          rounded operations, negated when the edge runs the other way -- a shared edge gives both triangles the same bits), a 64-byte record,
//          a conservative rectangle of 16 x 16 tiles (clipped against the near plane where the triangle crosses it) and the tile counts;
//   scan   one workgroup: exclusive offsets of the tiles, the needed list length D (64 bits) and the longest list;
//   fill   one thread per triangle: its id into every tile list of its rectangle (nothing when D exceeds the capacity); in setup and fill a
//          rectangle of more than kMeshSerialTiles tiles is walked by the whole workgroup;
//   shade  one workgroup per tile, one pixel per thread, a wavefront per 8 x 8 quadrant: the tile's records staged through LDS in chunks of
//          kMeshChunk, every lane reads each of them once (broadcast reads) and keeps (z, id) of its nearest hit in registers.
// Integer atomics only (tile counters and list cursors); every cross-workgroup read happens in a later launch.  The order of a tile list depends
// on scheduling, the image does not: the winner is the smallest z and, among equal z, the lowest triangle index.
constexpr int kMeshChunk = 256;             // records per pass: 4 x 256 x 16 B = 16 KiB of LDS per workgroup

struct MeshCam { float fx, fy, cx, cy, w2c[12], near_z, clip_z; int W, H, gx, gy; };

// p_i x p_j of the edge (i, j): the lower vertex index first, then negated if that swapped them.  Negation is exact, and so is its passage
// through the fused multiply-adds of the edge function: the two triangles of an edge get E of the same magnitude from the same operands.
__device__ __forceinline__ float4 mesh_edge_normal(int i, int j, const float (&pi)[3], const float (&pj)[3], float w)
{
#pragma clang fp contract(off)
    const bool flip = i > j;
    const float ax = flip ? pj[0] : pi[0], ay = flip ? pj[1] : pi[1], az = flip ? pj[2] : pi[2];
    const float bx = flip ? pi[0] : pj[0], by = flip ? pi[1] : pj[1], bz = flip ? pi[2] : pj[2];
    const float x = ay * bz - az * by;
    const float y = az * bx - ax * bz;
    const float z = ax * by - ay * bx;
    return make_float4(flip ? -x : x, flip ? -y : y, flip ? -z : z, w);
}

__device__ __forceinline__ void mesh_project(const MeshCam& c, float X, float Y, float Z, float (&lo)[2], float (&hi)[2], bool& wild)
{
    const float u = c.fx * (X / Z) + c.cx, v = c.fy * (Y / Z) + c.cy;
    wild = wild || u != u || v != v;
    lo[0] = fminf(lo[0], u); hi[0] = fmaxf(hi[0], u);
    lo[1] = fminf(lo[1], v); hi[1] = fmaxf(hi[1], v);
}

// The tile rectangle that holds every pixel the triangle can hit, or (1, 0) for none.  A hit has z >= near and lies, seen from the pixel centre,
// inside the projection of the part of the triangle with z >= near; the clip plane is put a little in front of near (clip_z = near (1 - 2^-10)),
// so that a z the kernel rounds up to near is still inside.  The box is grown by a pixel; where the triangle crosses the plane the cut points are
// rounded and projected with a small divisor, and the box is grown by a further 1/1024 of the image.  A projection that is not a number lists the
// triangle in every tile.  Known limit (stated in the header): the pad does not scale with the rounding of the edge vectors, so the tip of a
// needle whose edges meet well below 1e-3 rad can reach beyond the box.
__device__ __forceinline__ uint2 mesh_tile_rect(const MeshCam& c, const float (&p)[3][3])
{
    const uint2 none = make_uint2(1u, 0u);
    const bool in[3] = {p[0][2] >= c.clip_z, p[1][2] >= c.clip_z, p[2][2] >= c.clip_z};
    if (!in[0] && !in[1] && !in[2]) return none;
    const float inf = __uint_as_float(0x7f800000u);
    float lo[2] = {inf, inf}, hi[2] = {-inf, -inf};
    bool wild = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int l = k == 2 ? 0 : k + 1;
        if (in[k]) mesh_project(c, p[k][0], p[k][1], p[k][2], lo, hi, wild);
        if (in[k] != in[l]) {
            const float s = (c.clip_z - p[k][2]) / (p[l][2] - p[k][2]);
            mesh_project(c, p[k][0] + s * (p[l][0] - p[k][0]), p[k][1] + s * (p[l][1] - p[k][1]), c.clip_z, lo, hi, wild);
        }
    }
    int x0 = 0, x1 = c.W - 1, y0 = 0, y1 = c.H - 1;
    if (!wild) {
        const bool crossing = !(in[0] && in[1] && in[2]);
        const float pad = crossing ? 1.0f + (float)(c.W > c.H ? c.W : c.H) * (1.0f / 1024.0f) : 1.0f;
        lo[0] -= pad; lo[1] -= pad; hi[0] += pad; hi[1] += pad;
        if (hi[0] < 0.0f || hi[1] < 0.0f || lo[0] > (float)(c.W - 1) || lo[1] > (float)(c.H - 1)) return none;
        x0 = (int)floorf(fmaxf(lo[0], 0.0f)); x1 = (int)ceilf(fminf(hi[0], (float)(c.W - 1)));
        y0 = (int)floorf(fmaxf(lo[1], 0.0f)); y1 = (int)ceilf(fminf(hi[1], (float)(c.H - 1)));
    }
    return make_uint2((uint32_t)(x0 / kTile) | ((uint32_t)(x1 / kTile) << 16), (uint32_t)(y0 / kTile) | ((uint32_t)(y1 / kTile) << 16));
}

// Every tile of the rectangles of a workgroup's triangles goes to visit(tile, triangle): a rectangle of at most kMeshSerialTiles tiles is walked
// by its own thread, a larger one (a wall seen from inside the room covers the image) by all threads of the workgroup together -- one thread
// walking 1 024 tiles, an atomic each, took 0.25 ms at 512 x 512.  Called by every thread of the workgroup (live = false: no triangle).
constexpr int kMeshSerialTiles = 8;

template <class F>
__device__ __forceinline__ void mesh_for_tiles(uint2 rect, bool live, int gx, uint2* s_rect, int* s_big, int* s_nbig, F visit)
{
    if (threadIdx.x == 0) *s_nbig = 0;
    s_rect[threadIdx.x] = rect;
    __syncthreads();
    const int x0 = rect.x & 0xffff, x1 = rect.x >> 16, y0 = rect.y & 0xffff, y1 = rect.y >> 16;
    const int w = x1 - x0 + 1, n = live && w > 0 ? w * (y1 - y0 + 1) : 0;
    if (n > kMeshSerialTiles) s_big[atomicAdd(s_nbig, 1)] = (int)threadIdx.x;
    else
        for (int i = 0; i < n; ++i) visit((y0 + i / w) * gx + x0 + i % w, (int)threadIdx.x);
    __syncthreads();
    const int nbig = *s_nbig;
    for (int b = 0; b < nbig; ++b) {
        const int who = s_big[b];
        const uint2 r = s_rect[who];
        const int bx0 = r.x & 0xffff, by0 = r.y & 0xffff, bw = (int)(r.x >> 16) - bx0 + 1, bn = bw * ((int)(r.y >> 16) - by0 + 1);
        for (int i = threadIdx.x; i < bn; i += kBlock) visit((by0 + i / bw) * gx + bx0 + i % bw, who);
    }
}

__global__ __launch_bounds__(kBlock) void mesh_setup_kernel(MeshCam c, int T, int V, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                             const uint8_t* __restrict__ cols, float4* __restrict__ records, uint2* __restrict__ rects,
                                                             uint32_t* __restrict__ tile_count)
{
    __shared__ uint2 s_rect[kBlock];
    __shared__ int s_big[kBlock], s_nbig;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < T;
    const int idx[3] = {live ? tris[3 * t] : -1, live ? tris[3 * t + 1] : -1, live ? tris[3 * t + 2] : -1};
    uint2 rect = make_uint2(1u, 0u);
    // (a triangle with an index outside the vertex array is dropped, not read)
    if ((unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V) {
        float p[3][3];
        uint32_t col[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* v = verts + 3 * (int64_t)idx[k];
            const uint8_t* q = cols + 3 * (int64_t)idx[k];
            const float X = v[0], Y = v[1], Z = v[2];
            p[k][0] = c.w2c[0] * X + c.w2c[1] * Y + c.w2c[2] * Z + c.w2c[3];
            p[k][1] = c.w2c[4] * X + c.w2c[5] * Y + c.w2c[6] * Z + c.w2c[7];
            p[k][2] = c.w2c[8] * X + c.w2c[9] * Y + c.w2c[10] * Z + c.w2c[11];
            col[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        }
        // U = E(b, c) weighs vertex a, V = E(c, a) vertex b, W = E(a, b) vertex c; .w carries that vertex's z
        records[4 * t + 0] = mesh_edge_normal(idx[1], idx[2], p[1], p[2], p[0][2]);
        records[4 * t + 1] = mesh_edge_normal(idx[2], idx[0], p[2], p[0], p[1][2]);
        records[4 * t + 2] = mesh_edge_normal(idx[0], idx[1], p[0], p[1], p[2][2]);
        records[4 * t + 3] = make_float4(__uint_as_float(col[0]), __uint_as_float(col[1]), __uint_as_float(col[2]), __uint_as_float((uint32_t)t));
        rect = mesh_tile_rect(c, p);
    }
    if (live) rects[t] = rect;
    mesh_for_tiles(rect, live, c.gx, s_rect, s_big, &s_nbig, [&](int tile, int) { atomicAdd(tile_count + tile, 1u); });
}

// One workgroup: exclusive offsets of the tile lists (a 64-bit running sum, chunk after chunk), the counters set back to zero for the fill's
// cursors, the total and the longest list.  Serial in the number of tiles (4 chunks at 512 x 512, 4 096 at 16384 x 16384: a known limit, in the header).
__global__ __launch_bounds__(kBlock) void mesh_scan_kernel(int tiles, uint32_t* __restrict__ tile_count, uint32_t* __restrict__ tile_offset,
                                                            uint64_t* __restrict__ total, uint32_t* __restrict__ d_counts)
{
    __shared__ uint64_t s_sum[kBlock];
    __shared__ uint32_t s_max[kBlock];
    uint64_t carry = 0;
    uint32_t longest = 0;
    for (int base = 0; base < tiles; base += kBlock) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < tiles ? tile_count[i] : 0u;
        if (i < tiles) tile_count[i] = 0u;
        longest = v > longest ? v : longest;
        s_sum[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < kBlock; d <<= 1) {
            const uint64_t add = (int)threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
            __syncthreads();
            s_sum[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < tiles) tile_offset[i] = (uint32_t)(carry + s_sum[threadIdx.x] - v);   // (wraps only when D exceeds 2^32: then nothing reads it)
        carry += s_sum[kBlock - 1];
        __syncthreads();
    }
    s_max[threadIdx.x] = longest;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s_max[threadIdx.x] = s_max[threadIdx.x] > s_max[threadIdx.x + d] ? s_max[threadIdx.x] : s_max[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tile_offset[tiles] = (uint32_t)carry;
        *total = carry;
        d_counts[0] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
        d_counts[1] = s_max[0];
    }
}

__global__ __launch_bounds__(kBlock) void mesh_fill_kernel(int T, int gx, const uint2* __restrict__ rects, const uint32_t* __restrict__ tile_offset,
                                                            uint32_t* __restrict__ cursor, const uint64_t* __restrict__ total, uint32_t capacity,
                                                            uint32_t* __restrict__ list)
{
    __shared__ uint2 s_rect[kBlock];
    __shared__ int s_big[kBlock], s_nbig;
    if (*total > (uint64_t)capacity) return;                    // too short a list: nothing is written, the shade clears the image
    const int64_t first = (int64_t)blockIdx.x * kBlock, t = first + threadIdx.x;
    const bool live = t < T;
    mesh_for_tiles(live ? rects[t] : make_uint2(1u, 0u), live, gx, s_rect, s_big, &s_nbig, [&](int tile, int who) {
        list[tile_offset[tile] + atomicAdd(cursor + tile, 1u)] = (uint32_t)(first + who);  // < tile_offset[tile + 1] <= D <= capacity
    });
}

__global__ __launch_bounds__(kBlock) void mesh_shade_kernel(MeshCam c, const float4* __restrict__ records, const uint32_t* __restrict__ tile_offset,
                                                             const uint32_t* __restrict__ list, const uint64_t* __restrict__ total, uint32_t capacity,
                                                             float* __restrict__ depth, int32_t* __restrict__ tri_id, uint8_t* __restrict__ color)
{
    __shared__ float4 s_rec[4][kMeshChunk];
    const int tile = blockIdx.y * c.gx + blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * kTile + (wave & 1) * kQuad + (lane & 7);
    const int y = blockIdx.y * kTile + (wave >> 1) * kQuad + (lane >> 3);
    const bool listed = *total <= (uint64_t)capacity;
    const uint32_t begin = listed ? tile_offset[tile] : 0u, end = listed ? tile_offset[tile + 1] : 0u;
    const float dx = ((float)x - c.cx) / c.fx, dy = ((float)y - c.cy) / c.fy;
    float best_z = __uint_as_float(0x7f800000u), best_u = 0.0f, best_v = 0.0f, best_w = 0.0f;
    uint32_t best_id = 0xffffffffu;
    for (uint32_t base = begin; base < end; base += kMeshChunk) {
        const int n = end - base < (uint32_t)kMeshChunk ? (int)(end - base) : kMeshChunk;
        __syncthreads();                                        // the chunk before this one has been read by every wavefront
        if ((int)threadIdx.x < n) {
            const float4* r = records + 4 * (int64_t)list[base + threadIdx.x];
#pragma unroll
            for (int j = 0; j < 4; ++j) s_rec[j][threadIdx.x] = r[j];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float4 a = s_rec[0][k], b = s_rec[1][k], w = s_rec[2][k];
            // E = d . n with d = (dx, dy, 1): explicit fused multiply-adds, so that every edge is evaluated by the same two operations
            const float U = __fmaf_rn(dx, a.x, __fmaf_rn(dy, a.y, a.z));
            const float V = __fmaf_rn(dx, b.x, __fmaf_rn(dy, b.y, b.z));
            const float W = __fmaf_rn(dx, w.x, __fmaf_rn(dy, w.y, w.z));
            if (!((U >= 0.0f && V >= 0.0f && W >= 0.0f) || (U <= 0.0f && V <= 0.0f && W <= 0.0f))) continue;
            const float S = U + V + W;
            if (S == 0.0f) continue;
            const float z = (U * a.w + V * b.w + W * w.w) / S;
            const uint32_t id = __float_as_uint(s_rec[3][k].w);
            if (fabsf(z) <= 3.402823466e38f && z >= c.near_z && (z < best_z || (z == best_z && id < best_id))) {
                best_z = z; best_id = id; best_u = U; best_v = V; best_w = W;
            }
        }
    }
    if (x >= c.W || y >= c.H) return;
    const int64_t pix = (int64_t)y * c.W + x;
    const bool hit = best_id != 0xffffffffu;
    uint32_t rgb[3] = {0u, 0u, 0u};
    if (hit) {
        const float4 q = records[4 * (int64_t)best_id + 3];
        const uint32_t ca = __float_as_uint(q.x), cb = __float_as_uint(q.y), cc = __float_as_uint(q.z);
        const float S = best_u + best_v + best_w;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float va = (float)((ca >> (8 * ch)) & 255u), vb = (float)((cb >> (8 * ch)) & 255u), vc = (float)((cc >> (8 * ch)) & 255u);
            const float l = floorf((best_u * va + best_v * vb + best_w * vc) / S + 0.5f);
            rgb[ch] = l < 0.0f ? 0u : (l > 255.0f ? 255u : (uint32_t)l);
        }
    }
    depth[pix] = hit ? best_z : 0.0f;
    tri_id[pix] = hit ? (int32_t)best_id : -1;
    color[3 * pix + 0] = (uint8_t)rgb[0]; color[3 * pix + 1] = (uint8_t)rgb[1]; color[3 * pix + 2] = (uint8_t)rgb[2];
}

hipError_t launch_mesh_render(const MeshArgs& a, hipStream_t st)
{
    MeshCam c;
    c.fx = a.fx; c.fy = a.fy; c.cx = a.cx; c.cy = a.cy; c.near_z = a.near_z; c.clip_z = a.near_z * (1.0f - 1.0f / 1024.0f);
    for (int i = 0; i < 12; ++i) c.w2c[i] = a.w2c[i];
    c.W = a.W; c.H = a.H; c.gx = (a.W + kTile - 1) / kTile; c.gy = (a.H + kTile - 1) / kTile;
    const int tiles = c.gx * c.gy;
    hipError_t e = hipMemsetAsync(a.tile_count, 0, (size_t)(tiles + 1) * 4, st);
    if (e != hipSuccess) return e;
    const unsigned tb = (unsigned)(((int64_t)a.T + kBlock - 1) / kBlock);
    if (a.T > 0)
        hipLaunchKernelGGL(mesh_setup_kernel, dim3(tb), dim3(kBlock), 0, st, c, a.T, a.V, a.vertices, a.triangles, a.vertex_colors, a.records, a.rects,
                           a.tile_count);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kBlock), 0, st, tiles, a.tile_count, a.tile_offset, a.total, a.d_counts);
    if (a.T > 0)
        hipLaunchKernelGGL(mesh_fill_kernel, dim3(tb), dim3(kBlock), 0, st, a.T, c.gx, (const uint2*)a.rects, (const uint32_t*)a.tile_offset, a.tile_count,
                           (const uint64_t*)a.total, a.capacity, a.list);
    hipLaunchKernelGGL(mesh_shade_kernel, dim3(c.gx, c.gy), dim3(kBlock), 0, st, c, (const float4*)a.records, (const uint32_t*)a.tile_offset,
                       (const uint32_t*)a.list, (const uint64_t*)a.total, a.capacity, a.depth, a.tri_id, a.color);
    return hipGetLastError();
}

// ---- textures of the mesh sensor (the rule: include/gsplat_hip.h, gs_mesh_render_textured) -----------------------------------------------
// The pool holds every level of every texture, one packed RGBX word per texel (R in the low byte, X = 0); the table says where.
//   mips     one launch per level index over all textures (blockIdx.y = texture), one destination texel per thread, integers only; level l
//            reads level l - 1, which the launch before it wrote;
//   texture  after the four launches of the render: one workgroup per 16 x 16 tile with mesh_shade_kernel's pixel-to-lane map (an 8 x 8 quadrant
//            per wavefront, so that the texels of a wavefront lie together).  A thread reads tri_id of its pixel, the winner's three edge records
//            from the scratch the render wrote, its three vertex indices and uvs, eight texels, and stores three bytes.  It reads nothing this
//            launch writes and uses no atomics.
__global__ __launch_bounds__(kBlock) void texture_mip_kernel(const GsTextureDesc* __restrict__ table, int level, uint32_t* __restrict__ pool)
{
    const GsTextureDesc* d = table + blockIdx.y;                // (read field by field: a copy indexed by `level` would live in scratch)
    if (level >= d->levels) return;
    const int w0 = d->width, h0 = d->height;
    const int ws = w0 >> (level - 1) > 1 ? w0 >> (level - 1) : 1, hs = h0 >> (level - 1) > 1 ? h0 >> (level - 1) : 1;
    const int wd = w0 >> level > 1 ? w0 >> level : 1, hd = h0 >> level > 1 ? h0 >> level : 1;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (int64_t)wd * hd) return;
    const int i = (int)(idx % wd), j = (int)(idx / wd);
    const int i0 = 2 * i, i1 = 2 * i + 1 < ws ? 2 * i + 1 : ws - 1, j0 = 2 * j, j1 = 2 * j + 1 < hs ? 2 * j + 1 : hs - 1;
    const uint32_t* src = pool + d->level_offset[level - 1];
    const uint32_t a = src[(int64_t)j0 * ws + i0], b = src[(int64_t)j0 * ws + i1], c = src[(int64_t)j1 * ws + i0], e = src[(int64_t)j1 * ws + i1];
    uint32_t out = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const uint32_t sum = ((a >> (8 * ch)) & 255u) + ((b >> (8 * ch)) & 255u) + ((c >> (8 * ch)) & 255u) + ((e >> (8 * ch)) & 255u) + 2u;
        out |= (sum >> 2) << (8 * ch);
    }
    pool[d->level_offset[level] + idx] = out;
}

hipError_t launch_texture_mips(int num_textures, const GsTextureDesc* h_table, const GsTextureDesc* table, uint32_t* pool, hipStream_t st)
{
    for (int level = 1; level < GS_TEXTURE_MAX_LEVELS; ++level) {
        int64_t most = 0;                                       // the largest level `level` of any texture that has one
        for (int k = 0; k < num_textures; ++k) {
            if (level >= h_table[k].levels) continue;
            const int64_t wd = h_table[k].width >> level > 1 ? h_table[k].width >> level : 1, hd = h_table[k].height >> level > 1 ? h_table[k].height >> level : 1;
            most = wd * hd > most ? wd * hd : most;
        }
        if (most == 0) break;
        hipLaunchKernelGGL(texture_mip_kernel, dim3((unsigned)((most + kBlock - 1) / kBlock), (unsigned)num_textures), dim3(kBlock), 0, st, table, level, pool);
    }
    return hipGetLastError();
}

// wrap(i) and wrap(i + 1) over n texels.  i is an integer of magnitude below 2^35 (|u| <= 2^20 times at most 2^14 texels): the remainder is taken
// in 32 bits where i fits them, which is every case but a wild uv
__device__ __forceinline__ void texture_wrap2(long long i, int n, int mode, int& m0, int& m1)
{
    if (mode == GS_WRAP_CLAMP) {
        m0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : (int)i);
        m1 = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : (int)(i + 1));
        return;
    }
    const int p = mode == GS_WRAP_MIRROR ? 2 * n : n;
    int m = i >= -2147483647ll && i <= 2147483647ll ? (int)i % p : (int)(i % p);
    if (m < 0) m += p;
    const int mn = m + 1 == p ? 0 : m + 1;
    m0 = m >= n ? 2 * n - 1 - m : m;                            // (only MIRROR has m >= n)
    m1 = mn >= n ? 2 * n - 1 - mn : mn;
}

// the bilinear sample of one level at (u, v), both finite and of magnitude at most 2^20: columns first, then rows
__device__ __forceinline__ void texture_level_sample(const GsTextureDesc* d, int w0, int h0, int wrap_s, int wrap_t, const uint32_t* __restrict__ pool,
                                                     int level, float u, float v, float (&out)[3])
{
#pragma clang fp contract(off)
    const int wl = w0 >> level > 1 ? w0 >> level : 1, hl = h0 >> level > 1 ? h0 >> level : 1;
    const float s = u * (float)wl - 0.5f, t = v * (float)hl - 0.5f;
    const float fi = floorf(s), fj = floorf(t);
    const float al = s - fi, be = t - fj;
    int i0, i1, j0, j1;
    texture_wrap2((long long)fi, wl, wrap_s, i0, i1);
    texture_wrap2((long long)fj, hl, wrap_t, j0, j1);
    const uint32_t* base = pool + d->level_offset[level];
    const uint32_t t00 = base[(int64_t)j0 * wl + i0], t01 = base[(int64_t)j0 * wl + i1];
    const uint32_t t10 = base[(int64_t)j1 * wl + i0], t11 = base[(int64_t)j1 * wl + i1];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a = (float)((t00 >> (8 * ch)) & 255u), b = (float)((t01 >> (8 * ch)) & 255u);
        const float c = (float)((t10 >> (8 * ch)) & 255u), e = (float)((t11 >> (8 * ch)) & 255u);
        const float top = (1.0f - al) * a + al * b, bot = (1.0f - al) * c + al * e;
        out[ch] = (1.0f - be) * top + be * bot;
    }
}

__global__ __launch_bounds__(kBlock) void mesh_texture_kernel(MeshCam c, const float4* __restrict__ records, const int32_t* __restrict__ tris, int V,
                                                               const float2* __restrict__ uvs, const int32_t* __restrict__ tri_texture, int num_textures,
                                                               const GsTextureDesc* __restrict__ table, const uint32_t* __restrict__ pool,
                                                               const int32_t* __restrict__ tri_id, uint8_t* __restrict__ color)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * kTile + (wave & 1) * kQuad + (lane & 7);
    const int y = blockIdx.y * kTile + (wave >> 1) * kQuad + (lane >> 3);
    if (x >= c.W || y >= c.H) return;
    const int64_t pix = (int64_t)y * c.W + x;
    const int32_t t = tri_id[pix];
    if (t < 0) return;
    const int32_t tex = tri_texture[t];
    if ((unsigned)tex >= (unsigned)num_textures) return;       // vertex colour, as gs_mesh_render left it
    const int32_t ia = tris[3 * (int64_t)t], ib = tris[3 * (int64_t)t + 1], ic = tris[3 * (int64_t)t + 2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return;   // (never a winner: dropped by the setup)
    const float4 ea = records[4 * (int64_t)t], eb = records[4 * (int64_t)t + 1], ec = records[4 * (int64_t)t + 2];
    const float2 ua = uvs[ia], ub = uvs[ib], uc = uvs[ic];
    const GsTextureDesc* d = table + tex;                       // (read field by field: a copy indexed by the level would live in scratch)
    const int w0 = d->width, h0 = d->height, wrap_s = d->wrap_s, wrap_t = d->wrap_t;
    // q at the pixel, at its right neighbour and at the one below, on the winner's plane: the edge functions as mesh_shade_kernel evaluates them
    float qu[3], qv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dx = ((float)(x + (k == 1)) - c.cx) / c.fx, dy = ((float)(y + (k == 2)) - c.cy) / c.fy;
        const float U = __fmaf_rn(dx, ea.x, __fmaf_rn(dy, ea.y, ea.z));
        const float Vv = __fmaf_rn(dx, eb.x, __fmaf_rn(dy, eb.y, eb.z));
        const float Ww = __fmaf_rn(dx, ec.x, __fmaf_rn(dy, ec.y, ec.z));
        const float S = U + Vv + Ww;
        qu[k] = (U * ua.x + Vv * ub.x + Ww * uc.x) / S;
        qv[k] = (U * ua.y + Vv * ub.y + Ww * uc.y) / S;
    }
    const int top = d->levels - 1;
    float col[3];
    if (!(fabsf(qu[0]) <= 1048576.0f) || !(fabsf(qv[0]) <= 1048576.0f)) {                  // (a NaN fails both)
        const uint32_t w = pool[d->level_offset[top]];
        col[0] = (float)(w & 255u); col[1] = (float)((w >> 8) & 255u); col[2] = (float)((w >> 16) & 255u);
    } else {
        const float exu = (qu[1] - qu[0]) * (float)w0, exv = (qv[1] - qv[0]) * (float)h0;
        const float eyu = (qu[2] - qu[0]) * (float)w0, eyv = (qv[2] - qv[0]) * (float)h0;
        const float rx = sqrtf(exu * exu + exv * exv), ry = sqrtf(eyu * eyu + eyv * eyv);
        const float rho = rx != rx || ry != ry ? rx + ry : fmaxf(rx, ry);                   // (fmaxf would drop a NaN)
        float lambda = (float)top;
        if (rho <= 1.0f) lambda = 0.0f;
        else if (rho <= 3.402823466e38f) lambda = fminf(log2f(rho), (float)top);
        const float l0 = floorf(lambda), f = lambda - l0;
        const int level0 = (int)l0, level1 = level0 + 1 < top ? level0 + 1 : top;
        float s0[3], s1[3];
        texture_level_sample(d, w0, h0, wrap_s, wrap_t, pool, level0, qu[0], qv[0], s0);
        texture_level_sample(d, w0, h0, wrap_s, wrap_t, pool, level1, qu[0], qv[0], s1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) col[ch] = (1.0f - f) * s0[ch] + f * s1[ch];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float l = floorf(col[ch] + 0.5f);
        color[3 * pix + ch] = (uint8_t)(l < 0.0f ? 0u : (l > 255.0f ? 255u : (uint32_t)l));
    }
}

hipError_t launch_mesh_render_textured(const MeshArgs& a, const float* uvs, const int32_t* tri_texture, int num_textures, const GsTextureDesc* table,
                                       const uint32_t* pool, hipStream_t st)
{
    const hipError_t e = launch_mesh_render(a, st);
    if (e != hipSuccess || num_textures == 0 || a.T == 0) return e;
    MeshCam c;
    c.fx = a.fx; c.fy = a.fy; c.cx = a.cx; c.cy = a.cy; c.near_z = a.near_z; c.clip_z = 0.0f;
    for (int i = 0; i < 12; ++i) c.w2c[i] = a.w2c[i];
    c.W = a.W; c.H = a.H; c.gx = (a.W + kTile - 1) / kTile; c.gy = (a.H + kTile - 1) / kTile;
    hipLaunchKernelGGL(mesh_texture_kernel, dim3(c.gx, c.gy), dim3(kBlock), 0, st, c, (const float4*)a.records, a.triangles, a.V, (const float2*)uvs,
                       tri_texture, num_textures, table, pool, (const int32_t*)a.tri_id, a.color);
    return hipGetLastError();
}

// ---- navigable grid of a storey from the triangle mesh (what the reference takes from Habitat-sim's navmesh, src/dataloader/dataloader.py:237-272;
// the rule: include/gsplat_hip.h, gs_mesh_navgrid) ---------------------------------------------------------------------------------------------
// A top-down, conservative classification of H x W square cells: every triangle is clipped against every cell it can reach, in fp64, and the y
// range of what is left sets the cell's floor and obstacle bits.  The launches are gs_mesh_render's:
//   setup  one thread per triangle: the nine fp32 coordinates as a 48-byte record, the per-triangle height pre-test, a conservative rectangle of
//          16 x 16-cell tiles around its xz bounding box and the tile counts;
//   scan, fill   mesh_scan_kernel and mesh_fill_kernel as they are;
//   tile   one workgroup per tile, one cell per thread, a wavefront per 8 x 8 quadrant: the tile's records staged through LDS in chunks of
//          kNavChunk, every lane reads each of them once (broadcast reads), rejects by bounding box, clips, and ORs two bits into a register;
//          one byte store per cell.
// The clip is Sutherland-Hodgman in its re-entrant form: a vertex a stage emits is fed to the next stage at once, and each stage keeps only its
// first and its previous vertex, so the polygon (up to 7 vertices of 3 doubles) is never stored -- no array indexed at run time, no scratch
// memory.  The vertices reach the last stage in the order, and from the operands, of the stage-after-stage formulation in the header: stage k
// sees a0 [if inside], I(a0, a1), a1 [if inside], .., I(a_n-1, a0), which is that formulation's output list.
// What the rectangle and the bounding-box rejection may skip (both only skip work whose result the rule fixes as "empty polygon"):
//   x  the first two half-spaces test the triangle's own x: all three below xa, or all three above xb, leave nothing (exact comparisons);
//   z  the last two test z of vertices that the x stages may have interpolated, p = a + t (b - a) with 0 <= t <= 1 (the quotient of two
//      correctly rounded differences of which the first is not the larger).  Its three roundings keep p.z within a few units of 2^-52 max|z|
//      of [min z, max z], twice over for a point interpolated from interpolated points; the box is padded by 2^-30 max|z|, far beyond that;
//   the rectangle's cell range comes from a division and is widened by one cell plus 2^-50 (|origin| / cell + 32768) cells, which covers
//   the rounding of the quotient and of the cell borders x0 + c cell; the borders are monotonic in c, so cells outside the range are
//   rejected by the exact test as well.  Listing a triangle in a tile it cannot reach costs time and changes nothing.
constexpr int kNavChunk = 256;              // records per pass: 256 x 48 B = 12 KiB of LDS per workgroup

// y_floor = floor_y - max_climb, y_step = floor_y + max_climb, y_head = floor_y + agent_height (fp64 sums of the host)
struct NavGridCam { double x0, z0, cell, y_floor, y_step, y_head; int W, H, gx, gy; };

__device__ __forceinline__ uint32_t nav_bits(const NavGridCam& c, double lo, double hi)
{
    return (hi >= c.y_floor && lo <= c.y_step ? 1u : 0u) | (hi > c.y_step && lo < c.y_head ? 2u : 0u);
}

__device__ __forceinline__ double nav_z_pad(double zmin, double zmax)
{
    const double m = fabs(zmin) > fabs(zmax) ? fabs(zmin) : fabs(zmax);
    return m * (1.0 / 1073741824.0);
}

// cells lo .. hi (clamped to 0 .. n - 1; lo > hi: none) that the interval [vmin, vmax] can reach along one axis
__device__ __forceinline__ bool nav_cell_range(double vmin, double vmax, double origin, double cell, int n, int& lo, int& hi)
{
#pragma clang fp contract(off)
    const double slack = 1.0 + (fabs(origin) / cell + 32768.0) * (1.0 / 1125899906842624.0);
    const double a = floor((vmin - origin) / cell - slack), b = floor((vmax - origin) / cell + slack);
    if (b < 0.0 || a > (double)(n - 1)) return false;
    lo = !(a > 0.0) ? 0 : (int)a;                                           // (written so that a NaN -- inf - inf at an absurd cell size -- lists every cell)
    hi = !(b < (double)(n - 1)) ? n - 1 : (int)b;
    return true;
}

__global__ __launch_bounds__(kBlock) void navgrid_setup_kernel(NavGridCam c, int T, int V, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                                float4* __restrict__ records, uint2* __restrict__ rects, uint32_t* __restrict__ tile_count)
{
    __shared__ uint2 s_rect[kBlock];
    __shared__ int s_big[kBlock], s_nbig;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < T;
    const int idx[3] = {live ? tris[3 * t] : -1, live ? tris[3 * t + 1] : -1, live ? tris[3 * t + 2] : -1};
    uint2 rect = make_uint2(1u, 0u);
    // (a triangle with an index outside the vertex array is dropped, not read)
    if ((unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V) {
        float p[3][3];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* v = verts + 3 * (int64_t)idx[k];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                p[k][j] = v[j];
                finite = finite && fabsf(p[k][j]) <= 3.402823466e38f;
            }
        }
        if (finite) {
            float lo[3], hi[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lo[j] = fminf(p[0][j], fminf(p[1][j], p[2][j]));
                hi[j] = fmaxf(p[0][j], fmaxf(p[1][j], p[2][j]));
            }
            // the height pre-test on the triangle's own y range: a triangle that sets neither bit is never listed
            if (nav_bits(c, (double)lo[1], (double)hi[1]) != 0u) {
                const double pad = nav_z_pad((double)lo[2], (double)hi[2]);
                int c0, c1, r0, r1;
                if (nav_cell_range((double)lo[0], (double)hi[0], c.x0, c.cell, c.W, c0, c1) &&
                    nav_cell_range((double)lo[2] - pad, (double)hi[2] + pad, c.z0, c.cell, c.H, r0, r1)) {
                    records[3 * t + 0] = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
                    records[3 * t + 1] = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
                    records[3 * t + 2] = make_float4(p[2][2], 0.0f, 0.0f, 0.0f);
                    rect = make_uint2((uint32_t)(c0 / kTile) | ((uint32_t)(c1 / kTile) << 16), (uint32_t)(r0 / kTile) | ((uint32_t)(r1 / kTile) << 16));
                }
            }
        }
    }
    if (live) rects[t] = rect;
    mesh_for_tiles(rect, live, c.gx, s_rect, s_big, &s_nbig, [&](int tile, int) { atomicAdd(tile_count + tile, 1u); });
}

// The four clip stages (x >= xa, x <= xb, z >= za, z <= zb).  Every member is addressed with a compile-time stage number, so the whole state
// lives in registers.
struct NavClip {
    double bound[4];
    double fx[4], fy[4], fz[4];             // the first vertex a stage received
    double sx[4], sy[4], sz[4];             // the vertex it received last
    bool have[4];
    double lo, hi;                          // y range of what left the last stage
    bool any;
};

template <int K>
__device__ __forceinline__ bool nav_inside(const NavClip& s, double x, double z)
{
    return K == 0 ? x >= s.bound[0] : (K == 1 ? x <= s.bound[1] : (K == 2 ? z >= s.bound[2] : z <= s.bound[3]));
}

template <int K>
__device__ __forceinline__ void nav_feed(NavClip& s, double x, double y, double z);

// the two things an edge (a, b) can hand to the next stage, in the rule's order: the crossing point, then b itself
template <int K>
__device__ __forceinline__ void nav_edge(NavClip& s, bool crossing, double ax, double ay, double az, double bx, double by, double bz, bool emit_b)
{
#pragma clang fp contract(off)
    const double bound = s.bound[K];
    const double ak = K < 2 ? ax : az, bk = K < 2 ? bx : bz;
    const double t = (bound - ak) / (bk - ak);                                 // (used only where the edge crosses: ak != bk)
    const double qx = ax + t * (bx - ax), qy = ay + t * (by - ay), qz = az + t * (bz - az);
    const double px = K < 2 ? bound : qx, pz = K < 2 ? qz : bound;
    // one call site for both, so that the next stage's code exists once and lanes that emit either walk it together
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        const bool first = j == 0;
        if (first ? crossing : emit_b) nav_feed<K + 1>(s, first ? px : bx, first ? qy : by, first ? pz : bz);
    }
}

template <int K>
__device__ __forceinline__ void nav_feed(NavClip& s, double x, double y, double z)
{
    if constexpr (K == 4) {
        s.lo = y < s.lo ? y : s.lo;
        s.hi = y > s.hi ? y : s.hi;
        s.any = true;
    } else {
        const bool in = nav_inside<K>(s, x, z);
        const bool had = s.have[K];
        const double ax = s.sx[K], ay = s.sy[K], az = s.sz[K];
        if (!had) { s.fx[K] = x; s.fy[K] = y; s.fz[K] = z; s.have[K] = true; }
        s.sx[K] = x; s.sy[K] = y; s.sz[K] = z;
        nav_edge<K>(s, had && nav_inside<K>(s, ax, az) != in, ax, ay, az, x, y, z, in);
    }
}

// the closing edge (last vertex, first vertex) of every stage, front to back
template <int K>
__device__ __forceinline__ void nav_close(NavClip& s)
{
    if constexpr (K < 4) {
        const double ax = s.sx[K], ay = s.sy[K], az = s.sz[K], bx = s.fx[K], by = s.fy[K], bz = s.fz[K];
        nav_edge<K>(s, s.have[K] && nav_inside<K>(s, ax, az) != nav_inside<K>(s, bx, bz), ax, ay, az, bx, by, bz, false);
        nav_close<K + 1>(s);
    }
}

__global__ __launch_bounds__(kBlock) void navgrid_tile_kernel(NavGridCam c, const float4* __restrict__ records, const uint32_t* __restrict__ tile_offset,
                                                               const uint32_t* __restrict__ list, const uint64_t* __restrict__ total, uint32_t capacity,
                                                               uint8_t* __restrict__ grid)
{
#pragma clang fp contract(off)
    __shared__ float4 s_rec[3 * kNavChunk];
    const float* s_v = (const float*)s_rec;
    const int tile = blockIdx.y * c.gx + blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * kTile + (wave & 1) * kQuad + (lane & 7);
    const int row = blockIdx.y * kTile + (wave >> 1) * kQuad + (lane >> 3);
    const bool listed = *total <= (uint64_t)capacity;
    const uint32_t begin = listed ? tile_offset[tile] : 0u, end = listed ? tile_offset[tile + 1] : 0u;
    // the cell's borders, exactly as the rule writes them
    const double xa = c.x0 + (double)col * c.cell, xb = c.x0 + (double)(col + 1) * c.cell;
    const double za = c.z0 + (double)row * c.cell, zb = c.z0 + (double)(row + 1) * c.cell;
    const double inf = (double)__uint_as_float(0x7f800000u);
    uint32_t bits = 0u;
    for (uint32_t base = begin; base < end; base += kNavChunk) {
        const int n = end - base < (uint32_t)kNavChunk ? (int)(end - base) : kNavChunk;
        __syncthreads();                                        // the chunk before this one has been read by every wavefront
        if ((int)threadIdx.x < n) {
            const float4* r = records + 3 * (int64_t)list[base + threadIdx.x];
#pragma unroll
            for (int j = 0; j < 3; ++j) s_rec[3 * threadIdx.x + j] = r[j];
        }
        __syncthreads();
        for (int k = 0; k < n && bits != 3u; ++k) {             // (both bits set: no triangle can add to them)
            const float* v = s_v + 12 * k;
            const float x0 = v[0], x1 = v[3], x2 = v[6], z0 = v[2], z1 = v[5], z2 = v[8];
            const double xmin = (double)fminf(x0, fminf(x1, x2)), xmax = (double)fmaxf(x0, fmaxf(x1, x2));
            if (xmax < xa || xmin > xb) continue;
            const double zmin = (double)fminf(z0, fminf(z1, z2)), zmax = (double)fmaxf(z0, fmaxf(z1, z2));
            const double pad = nav_z_pad(zmin, zmax);
            if (zmax + pad < za || zmin - pad > zb) continue;
            NavClip s;
            s.bound[0] = xa; s.bound[1] = xb; s.bound[2] = za; s.bound[3] = zb;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s.have[q] = false;
                s.fx[q] = s.fy[q] = s.fz[q] = s.sx[q] = s.sy[q] = s.sz[q] = 0.0;
            }
            s.lo = inf; s.hi = -inf; s.any = false;
#pragma unroll 1
            for (int i = 0; i < 3; ++i) nav_feed<0>(s, (double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]);
            nav_close<0>(s);
            if (s.any) bits |= nav_bits(c, s.lo, s.hi);
        }
    }
    if (col < c.W && row < c.H) grid[(int64_t)row * c.W + col] = (uint8_t)bits;
}

hipError_t launch_mesh_navgrid(const NavGridArgs& a, hipStream_t st)
{
    NavGridCam c;
    c.x0 = a.x0; c.z0 = a.z0; c.cell = a.cell;
    c.y_floor = a.floor_y - a.max_climb; c.y_step = a.floor_y + a.max_climb; c.y_head = a.floor_y + a.agent_height;
    c.W = a.W; c.H = a.H; c.gx = (a.W + kTile - 1) / kTile; c.gy = (a.H + kTile - 1) / kTile;
    const int tiles = c.gx * c.gy;
    hipError_t e = hipMemsetAsync(a.tile_count, 0, (size_t)(tiles + 1) * 4, st);
    if (e != hipSuccess) return e;
    const unsigned tb = (unsigned)(((int64_t)a.T + kBlock - 1) / kBlock);
    if (a.T > 0)
        hipLaunchKernelGGL(navgrid_setup_kernel, dim3(tb), dim3(kBlock), 0, st, c, a.T, a.V, a.vertices, a.triangles, a.records, a.rects, a.tile_count);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kBlock), 0, st, tiles, a.tile_count, a.tile_offset, a.total, a.d_counts);
    if (a.T > 0)
        hipLaunchKernelGGL(mesh_fill_kernel, dim3(tb), dim3(kBlock), 0, st, a.T, c.gx, (const uint2*)a.rects, (const uint32_t*)a.tile_offset, a.tile_count,
                           (const uint64_t*)a.total, a.capacity, a.list);
    hipLaunchKernelGGL(navgrid_tile_kernel, dim3(c.gx, c.gy), dim3(kBlock), 0, st, c, (const float4*)a.records, (const uint32_t*)a.tile_offset,
                       (const uint32_t*)a.list, (const uint64_t*)a.total, a.capacity, a.grid);
    return hipGetLastError();
}

// ---- TSDF fusion and surface extraction (a NEW capability: the reference has no counterpart; the rules: include/gsplat_hip.h,
// gs_tsdf_integrate / gs_tsdf_count / gs_tsdf_emit) --------------------------------------------------------------------------------------
// Integration: a thread owns a run of four voxels along the flat index (x fastest) for the whole call and keeps their tsdf, weight and colour
// in registers across the frames of the batch: the volume is read and written once per call (16-byte accesses: the flat index of a run is a
// multiple of four, so a run is aligned whatever nx is), and a batch gives the bits of the same frames integrated call by call -- a store and a
// load of an fp32 value change nothing.  A run no frame touched is not written back.  Poses and intrinsics are kernel arguments; the frame
// loop is uniform over the grid, so they are scalar loads.  No atomics, no LDS, no scratch.  Every fp32 operation is rounded on its own.
__device__ __forceinline__ float tsdf_centre(float o, int i, float vs)
{
#pragma clang fp contract(off)
    return o + ((float)i + 0.5f) * vs;
}

__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(TsdfArgs a)
{
#pragma clang fp contract(off)
    const int64_t runs = (a.g.n + 3) >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t npix = (int64_t)a.W * a.H;
    const int64_t nxy = (int64_t)a.g.nx * a.g.ny;
    const bool colour = a.frame_color != nullptr;
    for (int64_t run = (int64_t)blockIdx.x * kBlock + threadIdx.x; run < runs; run += stride) {
        const int64_t first = run << 2;
        const int live = a.g.n - first < 4 ? (int)(a.g.n - first) : 4;
        float tv[4], wv[4], cv[12];
        if (live == 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(a.tsdf + first), w4 = *reinterpret_cast<const float4*>(a.weight + first);
            tv[0] = t4.x; tv[1] = t4.y; tv[2] = t4.z; tv[3] = t4.w;
            wv[0] = w4.x; wv[1] = w4.y; wv[2] = w4.z; wv[3] = w4.w;
            if (colour) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float4 c4 = *reinterpret_cast<const float4*>(a.color + 3 * first + 4 * q);
                    cv[4 * q] = c4.x; cv[4 * q + 1] = c4.y; cv[4 * q + 2] = c4.z; cv[4 * q + 3] = c4.w;
                }
            }
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const bool in = v < live;
                tv[v] = in ? a.tsdf[first + v] : 0.0f;
                wv[v] = in ? a.weight[first + v] : 0.0f;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) cv[3 * v + ch] = in && colour ? a.color[3 * (first + v) + ch] : 0.0f;
            }
        }
        // the voxel centres of the run (a run may wrap into the next row)
        float px[4], py[4], pz[4];
        {
            int k = (int)(first / nxy);
            const int64_t rest = first - (int64_t)k * nxy;
            int j = (int)(rest / a.g.nx), i = (int)(rest - (int64_t)j * a.g.nx);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                px[v] = tsdf_centre(a.g.ox, i, a.g.vs); py[v] = tsdf_centre(a.g.oy, j, a.g.vs); pz[v] = tsdf_centre(a.g.oz, k, a.g.vs);
                if (++i == a.g.nx) { i = 0; if (++j == a.g.ny) { j = 0; ++k; } }
            }
        }
        bool dirty = false;
        for (int f = 0; f < a.frames; ++f) {
            const TsdfFrame& m = a.f[f];
            const float* __restrict__ depth = a.depth + (int64_t)f * npix;
            const float* __restrict__ sil = a.silhouette ? a.silhouette + (int64_t)f * npix : nullptr;
            const float* __restrict__ fcol = colour ? a.frame_color + 3 * (int64_t)f * npix : nullptr;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (v >= live) continue;
                const float z = m.r[6] * px[v] + m.r[7] * py[v] + m.r[8] * pz[v] + m.t[2];
                if (!(z > 0.0f)) continue;
                const float x = m.r[0] * px[v] + m.r[1] * py[v] + m.r[2] * pz[v] + m.t[0];
                const float y = m.r[3] * px[v] + m.r[4] * py[v] + m.r[5] * pz[v] + m.t[1];
                const float fu = floorf(a.fx * x / z + a.cx + 0.5f), fv = floorf(a.fy * y / z + a.cy + 0.5f);
                if (!(fu >= 0.0f && fu < (float)a.W && fv >= 0.0f && fv < (float)a.H)) continue;     // (a NaN fails it)
                const int64_t pix = (int64_t)fv * a.W + (int64_t)fu;
                float d = depth[pix];
                if (sil != nullptr) {
                    const float s = sil[pix];
                    if (!(s > a.sil_thres)) continue;
                    d = d / s;
                }
                if (!(d > 0.0f && d <= a.depth_max)) continue;                                         // (a NaN fails it)
                const float sdf = d - z;
                if (sdf < -a.trunc) continue;
                const float s = fminf(1.0f, sdf / a.trunc), w = wv[v], w1 = w + 1.0f;
                tv[v] = (tv[v] * w + s) / w1;
                if (colour) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) cv[3 * v + ch] = (cv[3 * v + ch] * w + fcol[ch * npix + pix]) / w1;
                }
                wv[v] = fminf(w1, a.max_weight);
                dirty = true;
            }
        }
        if (!dirty) continue;
        if (live == 4) {
            *reinterpret_cast<float4*>(a.tsdf + first) = make_float4(tv[0], tv[1], tv[2], tv[3]);
            *reinterpret_cast<float4*>(a.weight + first) = make_float4(wv[0], wv[1], wv[2], wv[3]);
            if (colour) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    *reinterpret_cast<float4*>(a.color + 3 * first + 4 * q) = make_float4(cv[4 * q], cv[4 * q + 1], cv[4 * q + 2], cv[4 * q + 3]);
            }
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (v >= live) continue;
                a.tsdf[first + v] = tv[v];
                a.weight[first + v] = wv[v];
                if (colour) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) a.color[3 * (first + v) + ch] = cv[3 * v + ch];
                }
            }
        }
    }
}

hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st)
{
    if (a.frames <= 0 || a.g.n <= 0) return hipSuccess;
    int64_t nb = ((a.g.n + 3) / 4 + kBlock - 1) / kBlock;
    if (nb > 256 * 16) nb = 256 * 16;                            // the rest of the runs by the grid's stride
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

// Extraction: marching tetrahedra on Kuhn's split of every cell.  For each permutation (a, b, c) of the axes one tetrahedron with the corners
// 0 -> e_a -> e_a + e_b -> (1, 1, 1); the split is the same in every cell, so neighbours agree on the diagonals of their shared faces and the
// surface closes without a matching pass.  The 16-case table of a tetrahedron is DERIVED (make_tet_table, on the host, once per launch): the
// triangles of a case from which corners are inside, their winding from the geometry of a reference tetrahedron -- the right-hand normal points
// from the inside corners (tsdf < 0) to the outside ones.  A tetrahedron of an odd permutation is the mirror image: its winding is flipped.
//   count   tsdf_cell_kernel    one thread per cell (= its lowest grid point): valid iff all eight corners have weight >= min_weight; 0..12 triangles
//           tsdf_point_kernel   one thread per grid point: the 7-bit mask of its live owned edges (towards +x, +y, +z, +xy, +xz, +yz, +xyz: ends of
//                               different sign, inside a valid cell) and the sums of both counts per 1 024 grid points
//   scan    compact.hip's block-count scan, two lists; the totals go to d_counts for the host to size the outputs
//   emit    tsdf_vertex_kernel  the workgroup's exclusive scan of the mask counts -> the first vertex of every grid point, its vertices
//           tsdf_triangle_kernel the same over the cells; a triangle's corner is the vertex of an edge: first vertex of the owner + the rank of
//                               the edge's slot in the owner's mask
// Vertices come out in (grid point, slot) order, triangles in (cell, tetrahedron, triangle) order: no atomics, the same bytes every run.
struct TetTable {
    uint32_t cases[16];      // bits 0-1: triangles; corner c of triangle t at bits 2 + 4 (3 t + c): the tetrahedron's edge (qa, qb), qa | qb << 2, qa < qb
    uint32_t tets[6];        // the cell corners (bit 0 +x, bit 1 +y, bit 2 +z) of the four tetrahedron corners, 3 bits each; bit 12: odd permutation
};

static TetTable make_tet_table()
{
    TetTable T;
    const double P[4][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};    // a reference tetrahedron of positive orientation
    for (int m = 0; m < 16; ++m) {
        int in[4], out[4], nin = 0, nout = 0;
        for (int q = 0; q < 4; ++q) { if ((m >> q) & 1) in[nin++] = q; else out[nout++] = q; }
        int tri[2][3][2], ntri = 0;                              // triangle corners as (inside corner, outside corner) edges
        if (nin == 1 || nin == 3) {                              // the lone corner is cut off
            const int lone = nin == 1 ? in[0] : out[0];
            const int* rest = nin == 1 ? out : in;
            for (int c = 0; c < 3; ++c) { tri[0][c][0] = nin == 1 ? lone : rest[c]; tri[0][c][1] = nin == 1 ? rest[c] : lone; }
            ntri = 1;
        } else if (nin == 2) {                                   // a quad: consecutive corners share a face of the tetrahedron
            const int quad[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
            const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
            for (int t = 0; t < 2; ++t)
                for (int c = 0; c < 3; ++c) { tri[t][c][0] = quad[pick[t][c]][0]; tri[t][c][1] = quad[pick[t][c]][1]; }
            ntri = 2;
        }
        if (ntri) {
            // the winding: normal of the first triangle (corners at the edge midpoints) against centroid(outside) - centroid(inside)
            double v[3][3], g[3] = {0, 0, 0};
            for (int c = 0; c < 3; ++c)
                for (int x = 0; x < 3; ++x) v[c][x] = 0.5 * (P[tri[0][c][0]][x] + P[tri[0][c][1]][x]);
            for (int x = 0; x < 3; ++x) {
                for (int q = 0; q < nout; ++q) g[x] += P[out[q]][x] / nout;
                for (int q = 0; q < nin; ++q) g[x] -= P[in[q]][x] / nin;
            }
            const double e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]}, e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
            const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            if (n[0] * g[0] + n[1] * g[1] + n[2] * g[2] < 0.0)
                for (int t = 0; t < ntri; ++t)
                    for (int x = 0; x < 2; ++x) { const int s = tri[t][1][x]; tri[t][1][x] = tri[t][2][x]; tri[t][2][x] = s; }
        }
        uint32_t word = (uint32_t)ntri;
        for (int t = 0; t < ntri; ++t)
            for (int c = 0; c < 3; ++c) {
                const int lo = tri[t][c][0] < tri[t][c][1] ? tri[t][c][0] : tri[t][c][1], hi = tri[t][c][0] + tri[t][c][1] - lo;
                word |= (uint32_t)(lo | (hi << 2)) << (2 + 4 * (3 * t + c));
            }
        T.cases[m] = word;
    }
    int k = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            if (b == a) continue;
            const int c = 3 - a - b;
            const bool odd = ((a > b) + (a > c) + (b > c)) & 1;
            T.tets[k++] = 0u | ((1u << a) << 3) | (((1u << a) | (1u << b)) << 6) | (7u << 9) | ((odd ? 1u : 0u) << 12);
        }
    return T;
}

constexpr int kTsdfBlock = 1024;            // grid points per workgroup of the scanned passes (= the records of block_sums)

__host__ __device__ constexpr int tsdf_slot_dir(int slot) { return slot == 0 ? 1 : slot == 1 ? 2 : slot == 2 ? 4 : slot == 3 ? 3 : slot == 4 ? 5 : slot == 5 ? 6 : 7; }
__host__ __device__ constexpr int tsdf_dir_slot(int d) { return d == 1 ? 0 : d == 2 ? 1 : d == 4 ? 2 : d == 3 ? 3 : d == 5 ? 4 : d == 6 ? 5 : 6; }

// every thread of the workgroup calls it (static indices: the table is a kernel argument and stays in scalar registers)
__device__ __forceinline__ void tet_table_stage(const TetTable& t, uint32_t* s_cases, uint32_t* s_tets)
{
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if ((int)threadIdx.x == q) s_cases[q] = t.cases[q];
#pragma unroll
    for (int q = 0; q < 6; ++q)
        if ((int)threadIdx.x == 16 + q) s_tets[q] = t.tets[q];
    __syncthreads();
}

// the 4-bit case of a tetrahedron from the cell's 8-bit inside pattern
__device__ __forceinline__ uint32_t tet_case(uint32_t pattern, uint32_t tet)
{
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) m |= ((pattern >> ((tet >> (3 * q)) & 7u)) & 1u) << q;
    return m;
}

__device__ __forceinline__ void tsdf_ijk(const TsdfGrid& g, int64_t p, int& i, int& j, int& k)
{
    const int64_t nxy = (int64_t)g.nx * g.ny;
    k = (int)(p / nxy);
    const int64_t rest = p - (int64_t)k * nxy;
    j = (int)(rest / g.nx);
    i = (int)(rest - (int64_t)j * g.nx);
}

__device__ __forceinline__ uint32_t tsdf_cell_pattern(const TsdfGrid& g, const float* __restrict__ tsdf, int64_t p)
{
    const int64_t nxy = (int64_t)g.nx * g.ny;
    uint32_t pattern = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) pattern |= (tsdf[p + (c & 1) + ((c >> 1) & 1) * (int64_t)g.nx + (c >> 2) * nxy] < 0.0f ? 1u : 0u) << c;
    return pattern;
}

__global__ __launch_bounds__(kBlock) void tsdf_cell_kernel(TsdfExtractArgs a, TetTable table)
{
    __shared__ uint32_t s_cases[16], s_tets[6];
    tet_table_stage(table, s_cases, s_tets);
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.g.n) return;
    int i, j, k;
    tsdf_ijk(a.g, p, i, j, k);
    uint32_t info = 0;
    if (i + 1 < a.g.nx && j + 1 < a.g.ny && k + 1 < a.g.nz) {
        const int64_t nxy = (int64_t)a.g.nx * a.g.ny;
        bool valid = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) valid = valid && a.weight[p + (c & 1) + ((c >> 1) & 1) * (int64_t)a.g.nx + (c >> 2) * nxy] >= a.min_weight;   // (a NaN fails it)
        if (valid) {
            const uint32_t pattern = tsdf_cell_pattern(a.g, a.tsdf, p);
            uint32_t count = 0;
            for (int t = 0; t < 6; ++t) count += s_cases[tet_case(pattern, s_tets[t])] & 3u;
            info = 0x80u | count;
        }
    }
    a.cell_info[p] = (uint8_t)info;
}

// the sum of v over the workgroup's kTsdfBlock threads, returned to thread 0 (every thread calls it)
__device__ __forceinline__ uint32_t tsdf_block_sum(uint32_t v, uint32_t* s_w)
{
    const uint32_t w = wave_sum_u32(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = w;
    __syncthreads();
    uint32_t s = 0;
    if (threadIdx.x == 0)
        for (int q = 0; q < kTsdfBlock / kWave; ++q) s += s_w[q];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_point_kernel(TsdfExtractArgs a)
{
    __shared__ uint32_t s_w[kTsdfBlock / kWave];
    const int64_t p = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
    const int64_t nxy = (int64_t)a.g.nx * a.g.ny;
    uint32_t mask = 0, triangles = 0;
    if (p < a.g.n) {
        int i, j, k;
        tsdf_ijk(a.g, p, i, j, k);
        triangles = a.cell_info[p] & 0x7fu;
        const bool inside = a.tsdf[p] < 0.0f;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
            if (i + dx >= a.g.nx || j + dy >= a.g.ny || k + dz >= a.g.nz) continue;
            if ((a.tsdf[p + dx + dy * (int64_t)a.g.nx + dz * nxy] < 0.0f) == inside) continue;
            // a valid cell that holds both ends: its lowest point is this one moved back along the axes the edge does not run along
            bool live = false;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (s & d) continue;
                const int sx = s & 1, sy = (s >> 1) & 1, sz = s >> 2;
                if (i - sx < 0 || j - sy < 0 || k - sz < 0) continue;
                live = live || (a.cell_info[p - sx - sy * (int64_t)a.g.nx - sz * nxy] & 0x80u) != 0;
            }
            if (live) mask |= 1u << tsdf_dir_slot(d);
        }
        a.edge_mask[p] = (uint8_t)mask;
    }
    const uint32_t nv = tsdf_block_sum((uint32_t)__popc(mask), s_w), nt = tsdf_block_sum(triangles, s_w);
    if (threadIdx.x == 0) { a.block_sums[blockIdx.x] = nv; a.block_sums[a.blocks + blockIdx.x] = nt; }
}

// the exclusive prefix of v over the workgroup's kTsdfBlock threads (every thread calls it)
__device__ __forceinline__ uint32_t tsdf_block_exclusive(uint32_t v, uint32_t* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int q = 0; q < wave; ++q) before += s_w[q];
    return before + inc - v;
}

// vertex on the edge from grid point a (the owner: the lower linear index) to b: t = va / (va - vb), a + t (b - a), operation by operation
__global__ __launch_bounds__(kTsdfBlock) void tsdf_vertex_kernel(TsdfExtractArgs a, uint32_t max_vertices, float* __restrict__ vertices,
                                                                 float* __restrict__ vertex_colors)
{
#pragma clang fp contract(off)
    __shared__ uint32_t s_w[kTsdfBlock / kWave];
    // (a workgroup whose grid points own no vertex: the scanned sums say so to every thread alike; the last workgroup always runs)
    if ((int)blockIdx.x + 1 < a.blocks && a.block_sums[blockIdx.x + 1] == a.block_sums[blockIdx.x]) return;
    const int64_t p = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
    const int64_t nxy = (int64_t)a.g.nx * a.g.ny;
    const uint32_t mask = p < a.g.n ? a.edge_mask[p] : 0u;
    uint32_t at = a.block_sums[blockIdx.x] + tsdf_block_exclusive((uint32_t)__popc(mask), s_w);
    if (mask == 0) return;
    a.vertex_offset[p] = at;
    int i, j, k;
    tsdf_ijk(a.g, p, i, j, k);
    const float va = a.tsdf[p];
    const float ax = tsdf_centre(a.g.ox, i, a.g.vs), ay = tsdf_centre(a.g.oy, j, a.g.vs), az = tsdf_centre(a.g.oz, k, a.g.vs);
    float ca[3] = {0.0f, 0.0f, 0.0f};
    if (a.color != nullptr) { ca[0] = a.color[3 * p]; ca[1] = a.color[3 * p + 1]; ca[2] = a.color[3 * p + 2]; }
#pragma unroll
    for (int slot = 0; slot < 7; ++slot) {
        if (!((mask >> slot) & 1u)) continue;
        const int d = tsdf_slot_dir(slot), dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        const int64_t q = p + dx + dy * (int64_t)a.g.nx + dz * nxy;
        const float vb = a.tsdf[q];
        const float t = va / (va - vb);
        if (at < max_vertices) {
            const float bx = tsdf_centre(a.g.ox, i + dx, a.g.vs), by = tsdf_centre(a.g.oy, j + dy, a.g.vs), bz = tsdf_centre(a.g.oz, k + dz, a.g.vs);
            vertices[3 * (int64_t)at + 0] = ax + t * (bx - ax);
            vertices[3 * (int64_t)at + 1] = ay + t * (by - ay);
            vertices[3 * (int64_t)at + 2] = az + t * (bz - az);
            if (a.color != nullptr) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) vertex_colors[3 * (int64_t)at + ch] = ca[ch] + t * (a.color[3 * q + ch] - ca[ch]);
            }
        }
        ++at;
    }
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_triangle_kernel(TsdfExtractArgs a, TetTable table, uint32_t max_triangles, int32_t* __restrict__ triangles)
{
    __shared__ uint32_t s_cases[16], s_tets[6], s_w[kTsdfBlock / kWave];
    if ((int)blockIdx.x + 1 < a.blocks && a.block_sums[a.blocks + blockIdx.x + 1] == a.block_sums[a.blocks + blockIdx.x]) return;   // (no triangle in this workgroup's cells)
    tet_table_stage(table, s_cases, s_tets);
    const int64_t p = (int64_t)blockIdx.x * kTsdfBlock + threadIdx.x;
    const int64_t nxy = (int64_t)a.g.nx * a.g.ny;
    const uint32_t count = p < a.g.n ? a.cell_info[p] & 0x7fu : 0u;
    uint32_t at = a.block_sums[a.blocks + blockIdx.x] + tsdf_block_exclusive(count, s_w);
    if (count == 0) return;
    const uint32_t pattern = tsdf_cell_pattern(a.g, a.tsdf, p);
    for (int t = 0; t < 6; ++t) {
        const uint32_t tet = s_tets[t], word = s_cases[tet_case(pattern, tet)];
        const bool mirrored = (tet >> 12) & 1u;
        for (uint32_t n = 0; n < (word & 3u); ++n, ++at) {
            if (at >= max_triangles) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int from = mirrored && c ? 3 - c : c;         // (a mirror image: corners 1 and 2 change places)
                const uint32_t edge = (word >> (2 + 4 * (3 * n + from))) & 15u;
                const uint32_t lo = (tet >> (3 * (edge & 3u))) & 7u, hi = (tet >> (3 * (edge >> 2))) & 7u;   // cell corners; lo is a subset of hi
                const int64_t owner = p + (lo & 1u) + ((lo >> 1) & 1u) * (int64_t)a.g.nx + (lo >> 2) * nxy;
                const uint32_t d = lo ^ hi;
                const uint32_t slot = (0x65423100u >> (4 * d)) & 15u;                                        // tsdf_dir_slot as nibbles, d = 1..7
                triangles[3 * (int64_t)at + c] = (int32_t)(a.vertex_offset[owner] + (uint32_t)__popc(a.edge_mask[owner] & ((1u << slot) - 1u)));
            }
        }
    }
}

static_assert(((0x65423100u >> 4) & 15u) == (uint32_t)tsdf_dir_slot(1) && ((0x65423100u >> 8) & 15u) == (uint32_t)tsdf_dir_slot(2) &&
              ((0x65423100u >> 12) & 15u) == (uint32_t)tsdf_dir_slot(3) && ((0x65423100u >> 16) & 15u) == (uint32_t)tsdf_dir_slot(4) &&
              ((0x65423100u >> 20) & 15u) == (uint32_t)tsdf_dir_slot(5) && ((0x65423100u >> 24) & 15u) == (uint32_t)tsdf_dir_slot(6) &&
              (0x65423100u >> 28) == (uint32_t)tsdf_dir_slot(7), "the nibble table of tsdf_triangle_kernel");

static uint64_t tsdf_align(uint64_t v) { return (v + 255) / 256 * 256; }

uint64_t tsdf_extract_scratch_bytes(int64_t n)
{
    const uint64_t blocks = (uint64_t)((n + kTsdfBlock - 1) / kTsdfBlock);
    return 2 * tsdf_align((uint64_t)n) + tsdf_align((uint64_t)n * 4) + tsdf_align(2 * blocks * 4);
}

void tsdf_extract_carve(int64_t n, void* scratch, TsdfExtractArgs& a)
{
    char* b = (char*)scratch;
    a.edge_mask = (uint8_t*)b;                   b += tsdf_align((uint64_t)n);
    a.cell_info = (uint8_t*)b;                   b += tsdf_align((uint64_t)n);
    a.vertex_offset = (uint32_t*)b;              b += tsdf_align((uint64_t)n * 4);
    a.block_sums = (uint32_t*)b;
    a.blocks = (int)((n + kTsdfBlock - 1) / kTsdfBlock);
}

hipError_t launch_tsdf_count(const TsdfExtractArgs& a, uint32_t* d_counts, hipStream_t st)
{
    const TetTable table = make_tet_table();
    hipLaunchKernelGGL(tsdf_cell_kernel, dim3((unsigned)((a.g.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, table);
    hipLaunchKernelGGL(tsdf_point_kernel, dim3((unsigned)a.blocks), dim3(kTsdfBlock), 0, st, a);
    return launch_block_counts_scan(a.block_sums, a.blocks, 2, d_counts, st);
}

hipError_t launch_tsdf_emit(const TsdfExtractArgs& a, uint32_t max_vertices, uint32_t max_triangles, float* vertices, float* vertex_colors,
                            int32_t* triangles, hipStream_t st)
{
    const TetTable table = make_tet_table();
    if (max_vertices > 0) hipLaunchKernelGGL(tsdf_vertex_kernel, dim3((unsigned)a.blocks), dim3(kTsdfBlock), 0, st, a, max_vertices, vertices, vertex_colors);
    if (max_triangles > 0) hipLaunchKernelGGL(tsdf_triangle_kernel, dim3((unsigned)a.blocks), dim3(kTsdfBlock), 0, st, a, table, max_triangles, triangles);
    return hipGetLastError();
}

}  // namespace gs
