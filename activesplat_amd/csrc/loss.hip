// loss.hip -- fused mapping loss, forward AND backward in two launches.
//
// Replaces the ~40 torch kernels the reference's get_loss issues per iteration for
//     loss = w_depth * mean_{gt_depth > 0} |gt_depth - depth|
//          + w_im    * ( 0.8 * mean |im - gt_im|  +  0.2 * (1 - mean SSIM(im, gt_im)) )
// (src/mapper/splatam/splatam.py:213-249; SSIM = src/mapper/splatam/utils/slam_external.py:54-97: 11x11 Gaussian
// window sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2, five depthwise convolutions + their autograd) and
// produces dL/dim and dL/ddepth directly for the rasteriser's backward.  On MI355X the depthwise 11x11
// convolutions alone cost ~1.7 ms per iteration through MIOpen; here every 16x16 pixel tile stages the rendered
// and target tiles (+5 px halo) in LDS and runs the separable window there.
//
//   loss_stats_kernel : per tile and channel, the window moments by separable 11-tap passes in LDS -> SSIM value and its
//                       partials w.r.t. (mu1, E[x^2], E[xy]) per pixel; block-reduced sums of 1 - SSIM, |x-y|, masked
//                       |depth error| and the mask count go to 4 device accumulators.
//                       Arithmetic: the moments are CENTRED -- both tiles are staged minus one pivot c (the target's value at
//                       the tile's first pixel; the zero padding becomes -c), and the five moments are those of x' = x - c,
//                       y' = y - c and (x' - y')^2.  Variances do not move with c, mu = mu' + c.  On a smooth render close to a
//                       smooth target E[x^2] - mu^2 of the raw values cancels seven digits against C2 = 9e-4 (a relative
//                       error of 1e-4 per pixel in SSIM, and the loss' image term off by 1e-4 .. 7e-3 relative); centred, the
//                       moments are small.  sigma_12 comes from var(x - y) = s1 + s2 - 2 s12, and what is summed is
//                       1 - SSIM = (B1 var(x - y) + A2 (mu1 - mu2)^2) / (B1 B2), a sum of non-negative terms (exactly 0 for
//                       im == gt), not 1 - (a sum of values near 1).
//   loss_grad_kernel  : convolves the three partial maps with the (symmetric) window, combines them into dL/dim,
//                       adds the L1 terms, writes dL/ddepth (needs the mask count of pass 1 -- read from device
//                       memory, no host sync) and the three loss scalars.
//   depth_median_kernel<0..3> + the kOutlier instantiations of the two kernels above and of tracking_loss_kernel: ignore_outlier_depth_loss
//                       (splatam.py:220-228) -- torch.median of the depth error as an exact select over a grid of workgroups, and the depth
//                       mask ANDed with err < 10 median.  The plain instantiations are what they were.
#include "gs_common.h"

namespace gs {

constexpr int kLT = 16;              // output tile edge
constexpr int kLH = 5;               // window half-width
constexpr int kLP = kLT + 2 * kLH;   // 26: tile + halo

// normalised 1-D Gaussian window, sigma 1.5 (exp(-(i-5)^2 / 4.5) / sum)
__device__ __constant__ float kWin[11] = {0.00102838f, 0.00759876f, 0.03600077f, 0.10936069f, 0.21300554f, 0.26601172f,
                                          0.21300554f, 0.10936069f, 0.03600077f, 0.00759876f, 0.00102838f};

__device__ __forceinline__ float block_sum(float v, float* s_red, int tid)
{
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// Accumulators: kAccSlots copies of {sum (1 - SSIM), sum |im - gt|, sum masked |gt_depth - depth|, mask count}, one 64-byte line
// each; a block adds to slot (block index mod kAccSlots).  With a single copy the 4 x 1200 same-line device atomics of a
// 640x480 frame serialise at the memory side and cost ~70 us -- more than all the arithmetic of the loss.
// (round 3: 256 copies, and a block's four sums leave as ONE request -- four lanes of one atomic instruction on one line -- instead of four:
// 3600 blocks on 64 lines were 4 x 56 same-line atomics in a row)
constexpr int kAccSlots = kLossAccSlots;
constexpr int kAccFloats = kAccSlots * 16;
__device__ __forceinline__ void acc_totals(const float* __restrict__ acc, float* s_tot, int tid)
{
    if (tid < kWave) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < kAccSlots / kWave; k++) {
            const float4 u = *reinterpret_cast<const float4*>(acc + (k * kWave + tid) * 16);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        const float a = wave_sum(v.x), b = wave_sum(v.y), c = wave_sum(v.z), d = wave_sum(v.w);
        if (tid == 0) { s_tot[0] = a; s_tot[1] = b; s_tot[2] = c; s_tot[3] = d; }
    }
    __syncthreads();
}
// ---- ignore_outlier_depth_loss (src/mapper/splatam/splatam.py:220-228) ----
//   err = |gt_depth - depth| * (gt_depth > 0),  keep = err < 10 * median(err)   (strict; torch.median over ALL pixels: the lower median, NaN as
//   soon as one err is NaN).  The median is a DEVICE scalar of gs_depth_error_median; the kOutlier instantiations of the three loss kernels AND
//   `keep` into their depth mask.  A median of 0 or NaN keeps nothing.  err is depth_error (gs_common.h); fp32 without contraction: the decision is
//   torch's, bit for bit.
__device__ __forceinline__ bool outlier_keep(float g, float d, float median)
{
#pragma clang fp contract(off)
    return depth_error(g, d) < 10.0f * median;
}
// the depth mask of the three loss kernels (splatam.py:231-234): a sensor depth, and neither the rendered depth nor its uncertainty a NaN
__device__ __forceinline__ bool depth_measured(float g, float d, float unc) { return g > 0.0f && d == d && unc == unc; }

// Exact select of the depth error's lower median (element (n - 1) / 2 of the sorted values) over a GRID of workgroups; map growth (grow.hip) calls it
// too.  err >= +0, so the floats order as their bit patterns do: three passes over 11 + 11 + 10 bits pin the value.  A NaN's bit pattern would be
// counted as the largest value and a finite median come out: the first pass raises a flag for it, and the pick returns NaN.
// One launch per pass: a workgroup histograms its pixels in LDS and adds its
// non-zero bins to the pass' global histogram with integer atomics (order-independent: the same bits on every run).  The workgroups of pass p + 1
// each re-derive the prefix of pass p from that FINISHED histogram -- nothing is handed from workgroup to workgroup inside a launch, the
// kernel boundary is the only synchronisation -- and a one-workgroup launch resolves the third pass.  A grid of 1 is the same code.
constexpr int kMedThreads = 1024;
constexpr int kMedBins = kMedianBins;                  // 2048
constexpr int kMedPer = kMedBins / kMedThreads;        // bins per thread in the scan
constexpr int kMedGroup = 32;                          // threads per second-level group of the scan (32 x 32 = 1024)

struct MedianPick { uint32_t prefix, mask, k; };

// the bin of `hist` (2048 counts, finished by an earlier launch) that holds the element of rank k, and the rank inside it.  All threads call;
// all return the same pick.  Thread t owns bins [kMedPer t, kMedPer t + kMedPer): two-level sums in LDS give its exclusive prefix.
__device__ __forceinline__ void median_pick(const uint32_t* __restrict__ hist, int shift, uint32_t bin_mask, MedianPick& p, uint32_t* s_part,
                                            uint32_t* s_group, uint32_t* s_sel, int tid)
{
    uint32_t c[kMedPer], own = 0u;
#pragma unroll
    for (int j = 0; j < kMedPer; j++) { c[j] = hist[tid * kMedPer + j]; own += c[j]; }
    __syncthreads();                                   // (s_part / s_group / s_sel of the previous pick are read no more)
    s_part[tid] = own;
    if (tid == 0) { s_sel[0] = 0u; s_sel[1] = 0u; }
    __syncthreads();
    if (tid < kMedThreads / kMedGroup) {
        uint32_t g = 0u;
        for (int j = 0; j < kMedGroup; j++) g += s_part[tid * kMedGroup + j];
        s_group[tid] = g;
    }
    __syncthreads();
    uint32_t excl = 0u;
    const int grp = tid / kMedGroup;
    for (int j = 0; j < grp; j++) excl += s_group[j];
    for (int j = grp * kMedGroup; j < tid; j++) excl += s_part[j];
    if (p.k >= excl && p.k - excl < own) {             // exactly one thread: the counts of the histogram sum to more than k
        uint32_t k = p.k - excl;
        int j = 0;
        for (; j < kMedPer - 1; j++) {
            if (k < c[j]) break;
            k -= c[j];
        }
        s_sel[0] = (uint32_t)(tid * kMedPer + j); s_sel[1] = k;
    }
    __syncthreads();
    p.prefix |= (s_sel[0] & bin_mask) << shift;
    p.mask |= bin_mask << shift;
    p.k = s_sel[1];
}

__device__ __forceinline__ int median_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ uint32_t median_bin_mask(int pass) { return pass == 2 ? 0x3ffu : 0x7ffu; }

// hists: three histograms of kMedBins counts, then the NaN flag.  kPass = 0..2: histogram pass; kPass = 3: the pick of the value.
template <int kPass>
__global__ __launch_bounds__(kMedThreads) void depth_median_kernel(int64_t n, const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                                   uint32_t* __restrict__ hists, float* __restrict__ d_median)
{
    __shared__ uint32_t s_hist[kMedBins];
    __shared__ uint32_t s_part[kMedThreads];
    __shared__ uint32_t s_group[kMedThreads / kMedGroup];
    __shared__ uint32_t s_sel[2];
    const int tid = threadIdx.x;
    MedianPick p;
    p.prefix = 0u; p.mask = 0u; p.k = (uint32_t)((n - 1) / 2);
    for (int q = 0; q < (kPass < 3 ? kPass : 3); q++)
        median_pick(hists + q * kMedBins, median_shift(q), median_bin_mask(q), p, s_part, s_group, s_sel, tid);
    if (kPass == 3) {
        if (tid == 0) *d_median = hists[3 * kMedBins] ? __uint_as_float(0x7fc00000u) : __uint_as_float(p.prefix);
        return;
    }
    for (int b = tid; b < kMedBins; b += kMedThreads) s_hist[b] = 0u;
    __syncthreads();
    const int sh = median_shift(kPass);
    const uint32_t bm = median_bin_mask(kPass);
    bool saw_nan = false;
    const int64_t stride = (int64_t)gridDim.x * kMedThreads;
    for (int64_t i = (int64_t)blockIdx.x * kMedThreads + tid; i < n; i += stride) {
        const float err = depth_error(gt_depth[i], depth[i]);
        if (kPass == 0 && err != err) saw_nan = true;
        const uint32_t bits = __float_as_uint(err);
        if ((bits & p.mask) == p.prefix) atomicAdd(&s_hist[(bits >> sh) & bm], 1u);
    }
    if (kPass == 0 && saw_nan) hists[3 * kMedBins] = 1u;   // (every writer stores the same value)
    __syncthreads();
    uint32_t* out = hists + kPass * kMedBins;
    for (int b = tid; b < kMedBins; b += kMedThreads) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(out + b, c);
    }
}

// grid of the three histogram passes: a function of n only.  A call is five short launches (memset, three passes, the pick).  Measured
// (profiles/outlier_loss.txt): 20.6 us at 256 x 256 for every G from 32 to 256, 23.2 us at 640 x 480 with the minimum at G = 64; one workgroup
// takes 58.6 / 206 us.  2048 pixels per workgroup up to 64 workgroups gives G = 32 and 64 there
int depth_median_grid(int64_t n)
{
    const int64_t g = (n + kMedianChunk - 1) / kMedianChunk;
    return (int)(g < 1 ? 1 : (g > kMedianAutoGrid ? kMedianAutoGrid : g));
}

hipError_t launch_depth_error_median(int64_t n, const float* depth, const float* gt_depth, uint32_t* scratch, float* d_median, int grid,
                                     hipStream_t st)
{
    const int G = grid > 0 ? (grid > kMedianMaxGrid ? kMedianMaxGrid : grid) : depth_median_grid(n);
    hipError_t e = hipMemsetAsync(scratch, 0, kMedianScratchWords * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((depth_median_kernel<0>), dim3(G), dim3(kMedThreads), 0, st, n, depth, gt_depth, scratch, d_median);
    hipLaunchKernelGGL((depth_median_kernel<1>), dim3(G), dim3(kMedThreads), 0, st, n, depth, gt_depth, scratch, d_median);
    hipLaunchKernelGGL((depth_median_kernel<2>), dim3(G), dim3(kMedThreads), 0, st, n, depth, gt_depth, scratch, d_median);
    hipLaunchKernelGGL((depth_median_kernel<3>), dim3(1), dim3(kMedThreads), 0, st, n, depth, gt_depth, scratch, d_median);
    return hipGetLastError();
}

// The window moments of one 16 x 16 output tile, shared by the loss and the evaluation: the tile + halo of two images staged in LDS minus one
// pivot, then the separable 11-tap passes over the five CENTRED moments (of x' = x - pivot, y' = y - pivot: means, second moments and the mean of
// (x' - y')^2).  load(p, x, y) reads both images at pixel offset p = row * W + column.  kValid: valid window (staged element (r, c) is input
// pixel (y0 + r, x0 + c)), else zero padding kLH (pixel (y0 + r - kLH, x0 + c - kLH); the padding becomes -pivot).  Every thread of the
// workgroup calls; thread (tx, ty) gets the moments of output (x0 + tx, y0 + ty), and s_x / s_y stay staged for the caller.
struct SsimMoments { float n1, n2, e11, e22, edd; };

template <bool kValid, typename Load>
__device__ __forceinline__ SsimMoments ssim_tile_moments(const float (&window)[11], int W, int H, int x0, int y0, float pivot, Load load,
                                                         float (&s_x)[kLP][kLP + 1], float (&s_y)[kLP][kLP + 1], float (&s_h)[5][kLP][kLT + 1])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int off = kValid ? 0 : kLH;
    // the tile + halo: 676 values of each image, three per thread.  ALL loads are issued before the first LDS store: as a loop with a store
    // behind each load the staging was three dependent memory round trips -- 5 of a wavefront's 6.8 us (round 6, rocprofv3 SQ_WAVE_CYCLES)
    constexpr int kStage = (kLP * kLP + kBlock - 1) / kBlock;
    float vx[kStage], vy[kStage];
#pragma unroll
    for (int it = 0; it < kStage; it++) {
        const int e = tid + it * kBlock;
        const int r = e / kLP, c = e - r * kLP;
        const int gx = x0 + c - off, gy = y0 + r - off;
        const bool in = e < kLP * kLP && gx >= 0 && gx < W && gy >= 0 && gy < H;
        load((size_t)(in ? gy : 0) * W + (in ? gx : 0), vx[it], vy[it]);
        if (!in) { vx[it] = 0.f; vy[it] = 0.f; }
    }
#pragma unroll
    for (int it = 0; it < kStage; it++) {
        const int e = tid + it * kBlock;
        if (e < kLP * kLP) { const int r = e / kLP, c = e - r * kLP; s_x[r][c] = vx[it] - pivot; s_y[r][c] = vy[it] - pivot; }
    }
    __syncthreads();
    for (int e = tid; e < kLP * kLT; e += kBlock) {       // horizontal pass: 26 rows x 16 columns
        const int r = e / kLT, c = e - r * kLT;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, dd = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float w = window[k], xv = s_x[r][c + k], yv = s_y[r][c + k], dv = xv - yv;
            a += w * xv; b += w * yv; aa += w * xv * xv; bb += w * yv * yv; dd += w * dv * dv;
        }
        s_h[0][r][c] = a; s_h[1][r][c] = b; s_h[2][r][c] = aa; s_h[3][r][c] = bb; s_h[4][r][c] = dd;
    }
    __syncthreads();
    SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};             // centred: n = mu - pivot
#pragma unroll
    for (int k = 0; k < 11; k++) {                         // vertical pass
        const float w = window[k];
        m.n1 += w * s_h[0][ty + k][tx]; m.n2 += w * s_h[1][ty + k][tx]; m.e11 += w * s_h[2][ty + k][tx];
        m.e22 += w * s_h[3][ty + k][tx]; m.edd += w * s_h[4][ty + k][tx];
    }
    return m;
}

template <bool kOutlier>
__global__ __launch_bounds__(kBlock) void loss_stats_kernel(int W, int H, const float* __restrict__ im,
                                                            const float* __restrict__ gt, const float* __restrict__ depth,
                                                            const float* __restrict__ depth_sq,
                                                            const float* __restrict__ gt_depth, float* __restrict__ partials,
                                                            float* __restrict__ acc, const float* __restrict__ d_median)
{
    __shared__ float s_x[kLP][kLP + 1];
    __shared__ float s_y[kLP][kLP + 1];
    __shared__ float s_h[5][kLP][kLT + 1];          // horizontal-pass results of x', y', x'x', y'y', (x' - y')^2
    __shared__ float s_red[16];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = blockIdx.x * kLT, y0 = blockIdx.y * kLT;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const size_t HW = (size_t)W * H;
    float sum_ssim = 0.f, sum_l1 = 0.f;         // (sum_ssim: of 1 - SSIM)
    const int ch = blockIdx.z;                  // one colour channel per workgroup: 3x the workgroups, a third of the serial chain
    {
        const float pivot = gt[ch * HW + (size_t)y0 * W + x0];          // (x0 < W and y0 < H for every workgroup of the grid)
        const SsimMoments mo = ssim_tile_moments<false>(kWin, W, H, x0, y0, pivot,
                                                        [&](size_t p, float& x, float& y) { x = im[ch * HW + p]; y = gt[ch * HW + p]; }, s_x, s_y, s_h);
        const float n1 = mo.n1, n2 = mo.n2, e11 = mo.e11, e22 = mo.e22, edd = mo.edd;
        if (inside) {
            const float c1 = 0.0001f, c2 = 0.0009f;
            const float dm = n1 - n2, vd = edd - dm * dm;                    // mu1 - mu2, var(x - y)
            const float m1 = n1 + pivot, m2 = n2 + pivot;
            const float B2 = (e11 - n1 * n1) + (e22 - n2 * n2) + c2, A2 = B2 - vd;   // A2 = 2 sigma_12 + C2
            const float A1 = 2.f * m1 * m2 + c1, B1 = m1 * m1 + m2 * m2 + c1;
            const float inv = 1.0f / (B1 * B2);
            const float S = A1 * A2 * inv;
            sum_ssim += (B1 * vd + A2 * (dm * dm)) * inv;                     // 1 - S
            const size_t o = ch * HW + (size_t)py * W + px;
            partials[o] = 2.f * m2 * (A2 - A1) * inv - 2.f * m1 * S * (1.0f / B1 - 1.0f / B2);   // dS/dmu1
            partials[3 * HW + o] = -S / B2;                                                      // dS/dE[x^2]
            partials[6 * HW + o] = 2.f * A1 * inv;                                               // dS/dE[xy]
            sum_l1 += fabsf(s_x[ty + kLH][tx + kLH] - s_y[ty + kLH][tx + kLH]);
        }
    }
    float sum_d = 0.f, cnt = 0.f;
    if (inside && ch == 0) {                    // the depth term rides with the channel-0 workgroups
        const size_t o = (size_t)py * W + px;
        const float d = depth[o], g = gt_depth[o];
        const float unc = depth_sq ? depth_sq[o] - d * d : 0.f;
        bool m = depth_measured(g, d, unc);
        if (kOutlier) m = m && outlier_keep(g, d, d_median[0]);
        if (m) { sum_d = fabsf(g - d); cnt = 1.f; }
    }
    // the four sums of the workgroup in ONE reduction (two barriers instead of eight): wave sums -> LDS -> four lanes add the four waves' values
    sum_ssim = wave_sum(sum_ssim); sum_l1 = wave_sum(sum_l1); sum_d = wave_sum(sum_d); cnt = wave_sum(cnt);
    __syncthreads();
    if ((tid & 63) == 0) { float* r = s_red + (tid >> 6) * 4; r[0] = sum_ssim; r[1] = sum_l1; r[2] = sum_d; r[3] = cnt; }
    __syncthreads();
    if (tid < 4) {
        float* a = acc + (((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) & (kAccSlots - 1)) * 16;
        atomicAdd(a + tid, (s_red[tid] + s_red[4 + tid]) + (s_red[8 + tid] + s_red[12 + tid]));
    }
}

template <bool kOutlier>
__global__ __launch_bounds__(kBlock) void loss_grad_kernel(int W, int H, const float* __restrict__ im,
                                                           const float* __restrict__ gt, const float* __restrict__ depth,
                                                           const float* __restrict__ depth_sq,
                                                           const float* __restrict__ gt_depth, const float* __restrict__ partials,
                                                           const float* __restrict__ acc, float w_im, float w_depth,
                                                           float* __restrict__ dL_dim, float* __restrict__ dL_ddepth,
                                                           float* __restrict__ losses, float* __restrict__ acc_other,
                                                           const float* __restrict__ d_median)
{
    __shared__ float s_p[3][kLP][kLP + 1];
    __shared__ float s_h[3][kLP][kLT + 1];
    __shared__ float s_tot[4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    acc_totals(acc, s_tot, tid);
    // persistent scratch: the accumulator set of the NEXT call is zeroed here (nobody touches it during this call), so that no memset is needed
    if (acc_other && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int e = tid; e < kAccFloats; e += kBlock) acc_other[e] = 0.0f;
    const int x0 = blockIdx.x * kLT, y0 = blockIdx.y * kLT;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const size_t HW = (size_t)W * H;
    const float n3 = 3.0f * (float)HW;
    const float k_ssim = -0.2f * w_im / n3, k_l1 = 0.8f * w_im / n3;
    const int ch = blockIdx.z;
    {
        // (all nine loads of a thread -- and the centre pixel's im / gt of the combine below -- in flight before the first LDS store: see loss_stats_kernel)
        constexpr int kStage = (kLP * kLP + kBlock - 1) / kBlock;
        float v0[kStage], v1[kStage], v2[kStage];
#pragma unroll
        for (int it = 0; it < kStage; it++) {
            const int e = tid + it * kBlock;
            const int r = e / kLP, c = e - r * kLP;
            const int gx = x0 + c - kLH, gy = y0 + r - kLH;
            const bool in = e < kLP * kLP && gx >= 0 && gx < W && gy >= 0 && gy < H;
            const size_t o = ch * HW + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
            v0[it] = partials[o]; v1[it] = partials[3 * HW + o]; v2[it] = partials[6 * HW + o];
            if (!in) { v0[it] = 0.f; v1[it] = 0.f; v2[it] = 0.f; }
        }
#pragma unroll
        for (int it = 0; it < kStage; it++) {
            const int e = tid + it * kBlock;
            if (e < kLP * kLP) { const int r = e / kLP, c = e - r * kLP; s_p[0][r][c] = v0[it]; s_p[1][r][c] = v1[it]; s_p[2][r][c] = v2[it]; }
        }
        __syncthreads();
        for (int e = tid; e < kLP * kLT; e += kBlock) {
            const int r = e / kLT, c = e - r * kLT;
            float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = kWin[k];
                a += w * s_p[0][r][c + k]; b += w * s_p[1][r][c + k]; d += w * s_p[2][r][c + k];
            }
            s_h[0][r][c] = a; s_h[1][r][c] = b; s_h[2][r][c] = d;
        }
        __syncthreads();
        float g1 = 0.f, g2 = 0.f, g3 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float w = kWin[k];
            g1 += w * s_h[0][ty + k][tx]; g2 += w * s_h[1][ty + k][tx]; g3 += w * s_h[2][ty + k][tx];
        }
        if (inside) {
            const size_t o = ch * HW + (size_t)py * W + px;
            const float x = im[o], y = gt[o];
            const float diff = x - y;
            const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
            dL_dim[o] = k_ssim * (g1 + 2.f * x * g2 + y * g3) + k_l1 * sgn;
        }
    }
    const float cnt = s_tot[3];
    if (inside && ch == 0) {
        const size_t o = (size_t)py * W + px;
        const float d = depth[o], g = gt_depth[o];
        const float unc = depth_sq ? depth_sq[o] - d * d : 0.f;
        bool m = depth_measured(g, d, unc);
        if (kOutlier) m = m && outlier_keep(g, d, d_median[0]);
        const float diff = d - g;
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        dL_ddepth[o] = m ? w_depth * sgn / cnt : 0.f;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0) {
        const float l_im = w_im * (0.8f * s_tot[1] / n3 + 0.2f * (s_tot[0] / n3));                  // s_tot[0] = sum of 1 - SSIM
        const float l_depth = w_depth * s_tot[2] / cnt;
        losses[0] = l_im + l_depth; losses[1] = l_im; losses[2] = l_depth;
        losses[3] = l_im + l_depth;      // second copy: the host side hands out [0..2] as the report and [3] as the loss value
    }
}

hipError_t launch_mapping_loss(int W, int H, const float* im, const float* gt, const float* depth, const float* depth_sq,
                               const float* gt_depth, float w_im, float w_depth, float* losses, float* dL_dim,
                               float* dL_ddepth, float* scratch, int64_t persistent_call, hipStream_t st, const float* d_median)
{
    // two sets of kAccSlots x 4 accumulators (one 64-byte line each), then 9 partial maps.  persistent_call = 0: any scratch, set 0 is
    // memset here.  persistent_call = k >= 1: the k-th call on a scratch its owner zeroed ONCE and keeps for this stream -- the call uses
    // set k & 1 and its second kernel zeroes the other one for call k + 1 (no memset launch per call)
    const int set = persistent_call > 0 ? (int)(persistent_call & 1) : 0;
    float* acc = scratch + set * kAccFloats;
    float* acc_other = persistent_call > 0 ? scratch + (1 - set) * kAccFloats : nullptr;
    float* partials = scratch + 2 * kAccFloats;
    if (persistent_call <= 0) {
        hipError_t e = hipMemsetAsync(acc, 0, kAccFloats * sizeof(float), st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((W + kLT - 1) / kLT, (H + kLT - 1) / kLT, 3);
    if (d_median) {      // ignore_outlier_depth_loss: the same two launches, the depth mask ANDed with err < 10 median
        hipLaunchKernelGGL((loss_stats_kernel<true>), grid, dim3(kBlock), 0, st, W, H, im, gt, depth, depth_sq, gt_depth, partials, acc, d_median);
        hipLaunchKernelGGL((loss_grad_kernel<true>), grid, dim3(kBlock), 0, st, W, H, im, gt, depth, depth_sq, gt_depth, partials, acc, w_im,
                           w_depth, dL_dim, dL_ddepth, losses, acc_other, d_median);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((loss_stats_kernel<false>), grid, dim3(kBlock), 0, st, W, H, im, gt, depth, depth_sq, gt_depth, partials, acc, d_median);
    hipLaunchKernelGGL((loss_grad_kernel<false>), grid, dim3(kBlock), 0, st, W, H, im, gt, depth, depth_sq, gt_depth, partials, acc, w_im,
                       w_depth, dL_dim, dL_ddepth, losses, acc_other, d_median);
    return hipGetLastError();
}

// ---- tracking loss (src/mapper/splatam/splatam.py:220-249 with tracking=True, use_l1=True): value AND gradient in one pass over the image ----
//   mask   = (gt_depth > 0) & !isnan(depth) & !isnan(depth_sq - depth^2)  [& (silhouette > sil_thres) with use_sil_for_loss]
//   depth  = sum_mask |gt_depth - depth|,   im = sum |gt_im - im| over the mask tiled to 3 channels (use_sil) or over every pixel
//   dL/ddepth = -(w_depth [mask] * sgn(gt_depth - depth)),  dL/dim = -(w_im [colour mask] * sgn(gt_im - im))  -- autograd's own expression
//   (abs' backward grad * sgn, then the subtraction's negation; sgn(0) = sgn(NaN) = 0), so the images are bit-identical to torch's.
// Every workgroup writes one row of kTrackRow partial sums (no float atomics); tracking_loss_reduce (gs_common.h) sums the rows in a fixed order.
// kOutlier (ignore_outlier_depth_loss): the mask is ANDed with err < 10 median (d_median: gs_depth_error_median's device scalar) and the colour
// mask is ALWAYS the mask tiled to 3 channels (splatam.py:242), with or without use_sil_for_loss.  Same rows, same finish and step kernels.
__device__ __forceinline__ float sgnf(float x) { return (float)((0.f < x) - (x < 0.f)); }

template <bool kOutlier>
__global__ __launch_bounds__(kBlock) void tracking_loss_kernel(int npix, const float* __restrict__ im, const float* __restrict__ gt,
                                                               const float* __restrict__ depth, const float* __restrict__ depth_sq,
                                                               const float* __restrict__ gt_depth, const float* __restrict__ sil, int use_sil,
                                                               float sil_thres, float w_im, float w_depth, float* __restrict__ dL_dim,
                                                               float* __restrict__ dL_ddepth, float* __restrict__ rows,
                                                               const float* __restrict__ d_median)
{
#pragma clang fp contract(off)
    __shared__ float s_red[kTrackRow][kBlock / kWave];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float dsum = 0.f, csum = 0.f;
    if (i < npix) {
        const float d = depth[i], gd = gt_depth[i];
        const float unc = depth_sq[i] - d * d;
        bool m = depth_measured(gd, d, unc);
        if (kOutlier) m = m && outlier_keep(gd, d, d_median[0]);
        if (use_sil) m = m && sil[i] > sil_thres;
        const float ed = gd - d;
        if (m) dsum = fabsf(ed);
        dL_ddepth[i] = -((m ? w_depth : 0.f) * sgnf(ed));
        const bool cm = kOutlier ? m : (!use_sil || m);
        const float gc = cm ? w_im : 0.f;
        for (int ch = 0; ch < 3; ch++) {
            const size_t j = (size_t)ch * npix + i;
            const float ec = gt[j] - im[j];
            if (cm) csum += fabsf(ec);
            dL_dim[j] = -(gc * sgnf(ec));
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    dsum = wave_sum(dsum); csum = wave_sum(csum);
    if (lane == 0) { s_red[0][wave] = dsum; s_red[1][wave] = csum; }
    __syncthreads();
    if (threadIdx.x < kTrackRow) {
        float v = 0.f;
        for (int w = 0; w < kBlock / kWave; w++) v += s_red[threadIdx.x][w];
        rows[(size_t)blockIdx.x * kTrackRow + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(kBlock) void tracking_loss_finish_kernel(int64_t nrows, const float* __restrict__ rows, float w_im, float w_depth,
                                                                      float* __restrict__ losses)
{
    float L[3];
    tracking_loss_reduce(nrows, rows, w_im, w_depth, L);
    if (threadIdx.x == 0) { losses[0] = L[0]; losses[1] = L[1]; losses[2] = L[2]; }
}

hipError_t launch_tracking_loss(int W, int H, const float* im, const float* gt, const float* depth, const float* depth_sq, const float* gt_depth,
                                const float* sil, int use_sil, float sil_thres, float w_im, float w_depth, float* dL_dim, float* dL_ddepth,
                                float* rows, float* losses, hipStream_t st, const float* d_median)
{
    const int npix = W * H;
    const int64_t nb = tracking_loss_rows(npix);
    if (nb > 0 && d_median)
        hipLaunchKernelGGL((tracking_loss_kernel<true>), dim3((unsigned)nb), dim3(kBlock), 0, st, npix, im, gt, depth, depth_sq, gt_depth, sil, use_sil,
                           sil_thres, w_im, w_depth, dL_dim, dL_ddepth, rows, d_median);
    else if (nb > 0)
        hipLaunchKernelGGL((tracking_loss_kernel<false>), dim3((unsigned)nb), dim3(kBlock), 0, st, npix, im, gt, depth, depth_sq, gt_depth, sil, use_sil,
                           sil_thres, w_im, w_depth, dL_dim, dL_ddepth, rows, d_median);
    if (losses) hipLaunchKernelGGL(tracking_loss_finish_kernel, dim3(1), dim3(kBlock), 0, st, nb, rows, w_im, w_depth, losses);
    return hipGetLastError();
}

// ---- map-quality evaluation of one frame (gs_eval_frame; the rules: include/gsplat_hip.h) ----
// The reference's report_progress (src/mapper/splatam/utils/eval_helpers.py:211-245) and eval (:464-508) on one rendered frame: PSNR, the two depth
// errors, SSIM with the loss' own window (same padding, slam_external.py:66-97) and the 5-scale MS-SSIM of the package eval imports (valid
// window).  No float atomics and nothing read across workgroups inside a launch: every kernel writes one fp64 record per workgroup, and
// eval_finish_kernel (one workgroup) adds all records in the fixed order of gs_common.h (strided_record_sum, block_tree_sum), so a row has the same
// bits on every run.
//   eval_sums_kernel        : per-channel sum (d im)^2, sum |d depth| valid, sum (d depth)^2 valid, count of gt_depth > 0; the terms are fp32 (two
//                             roundings each), the accumulation fp64
//   eval_ssim_kernel<V, R>  : loss_stats_kernel's moment pass (ssim_tile_moments) with its own window table; per workgroup the sums of the ssim and
//                             cs maps of its 16 x 16 outputs.  V: valid window (no padding, output (w - 10) x (h - 10)), else zero padding 5.
//                             R: level 0 -- reads the frame itself and applies the masks on load (no masked copy of the frame exists)
//   eval_pool_kernel<R>     : avg_pool2d(kernel 2, padding = size % 2) of both images: the zero padding counts, the divisor is always 4
// the reference's window to the bit: exp(-(i - 5)^2 / 4.5) rounded to fp32 and normalised in fp32 (slam_external.py:54-56).  Its taps sum to
// 1 - 3.1e-8; kWin above (eight printed digits) is up to one ulp per tap away, which moves an SSIM by some 1e-7: enough to matter to a metric
// that is compared at 1e-6, so the evaluation kernels carry their own copy and the loss keeps its constants
__device__ __constant__ float kEvalWin[11] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055279e-01f, 2.660117149e-01f,
                                              2.130055279e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f};
constexpr float kEvalWinDeficit = 6.2398611e-08f;         // 1 - (sum of kEvalWin)^2
constexpr int kEvalSums = 6;                // doubles per record of the sums pass (padded to 8)
constexpr int kEvalRecord = 8;

__device__ __forceinline__ float eval_image_mask(size_t o, const float* __restrict__ gt_depth, const float* __restrict__ sil, float sil_thres, int flags)
{
    float m = 1.0f;
    if (flags & GS_EVAL_IMAGE_VALID_MASK) m *= gt_depth[o] > 0.0f ? 1.0f : 0.0f;
    if (flags & GS_EVAL_SIL_MASK) m *= sil[o] > sil_thres ? 1.0f : 0.0f;
    return m;
}

__global__ __launch_bounds__(kBlock) void eval_sums_kernel(int64_t npix, const float* __restrict__ im, const float* __restrict__ depth,
                                                           const float* __restrict__ sil, const float* __restrict__ gt,
                                                           const float* __restrict__ gt_depth, float sil_thres, int flags,
                                                           double* __restrict__ partial)
{
    __shared__ double s_tree[kEvalSums][kBlock];
    double a[kEvalSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npix; i += stride) {
        const float g = gt_depth[i];
        const float valid = g > 0.0f ? 1.0f : 0.0f;
        const float presence = (flags & GS_EVAL_SIL_MASK) ? (sil[i] > sil_thres ? 1.0f : 0.0f) : 1.0f;       // strict, as the reference's mask
        const float m = (flags & GS_EVAL_IMAGE_VALID_MASK) ? presence * valid : presence;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float d = (im[ch * npix + i] - gt[ch * npix + i]) * m;       // (im m - gt m of the reference, m in {0, 1}: the same float)
            const float sq = d * d;
            a[ch] += (double)sq;
        }
        const float dd = (depth[i] - g) * presence;        // products, not selects: a NaN under a zero mask stays a NaN, as in torch
        const float l1 = fabsf(dd) * valid, l2 = dd * dd;
        a[3] += (double)l1;
        a[4] += (double)(l2 * valid);
        a[5] += (double)valid;
    }
    block_tree_sum(a, s_tree);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kEvalSums; ++k) partial[(int64_t)blockIdx.x * kEvalRecord + k] = a[k];
    }
}

// partial: [3][tiles][2] doubles = (sum of 1 - ssim, sum of 1 - cs) over the workgroup's outputs
template <bool kValid, bool kRaw>
__global__ __launch_bounds__(kBlock) void eval_ssim_kernel(int W, int H, const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ gt_depth, const float* __restrict__ sil, float sil_thres,
                                                           int flags, double* __restrict__ partial)
{
    __shared__ float s_x[kLP][kLP + 1];
    __shared__ float s_y[kLP][kLP + 1];
    __shared__ float s_h[5][kLP][kLT + 1];
    __shared__ double s_tree[2][kBlock];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = blockIdx.x * kLT, y0 = blockIdx.y * kLT;
    const int OW = kValid ? W - 2 * kLH : W, OH = kValid ? H - 2 * kLH : H;
    const bool inside = x0 + tx < OW && y0 + ty < OH;
    const size_t HW = (size_t)W * H;
    const int ch = blockIdx.z;
    // the pivot of the centred moments: the target at the tile's first output pixel (x0 < OW <= W, y0 < OH <= H)
    const size_t po = (size_t)y0 * W + x0;
    const float pivot = y[ch * HW + po] * (kRaw ? eval_image_mask(po, gt_depth, sil, sil_thres, flags) : 1.0f);
    const SsimMoments mo = ssim_tile_moments<kValid>(kEvalWin, W, H, x0, y0, pivot,
                                                     [&](size_t p, float& vx, float& vy) {
                                                         const float m = kRaw ? eval_image_mask(p, gt_depth, sil, sil_thres, flags) : 1.0f;
                                                         vx = x[ch * HW + p] * m; vy = y[ch * HW + p] * m;
                                                     }, s_x, s_y, s_h);
    const float n1 = mo.n1, n2 = mo.n2, e11 = mo.e11, e22 = mo.e22, edd = mo.edd;
    double a[2] = {0.0, 0.0};
    if (inside) {
        // as in loss_stats_kernel: 1 - cs = var(x - y) / B2 and 1 - ssim = (B1 var(x - y) + A2 (mu1 - mu2)^2) / (B1 B2), both exactly 0 for x == y
        const float c1 = 0.0001f, c2 = 0.0009f;
        const float dm = n1 - n2, vd = edd - dm * dm;
        const float m1 = n1 + pivot, m2 = n2 + pivot;
        // kEvalWin's taps sum to 1 - 3.1e-8, the 2-D window to S = 1 - kEvalWinDeficit, and the reference's sum w x^2 - (sum w x)^2 is not
        // shift-invariant then: with x = x' + c it is the centred variance + 2 c (1 - S) sum w x' + c^2 S (1 - S).  The last term is 1.5e-8
        // against variances of a few 1e-3 -- 1e-6 of an SSIM of 0.8 -- so the centred sums get it back.  (var(x - y) has no such term.)
        const float shift = 2.f * pivot * kEvalWinDeficit * ((n1 + n2) + pivot * (1.0f - kEvalWinDeficit));
        const float B2 = ((e11 - n1 * n1) + (e22 - n2 * n2) + shift) + c2, A2 = B2 - vd;
        const float B1 = m1 * m1 + m2 * m2 + c1;
        a[0] = (double)((B1 * vd + A2 * (dm * dm)) / (B1 * B2));        // what is summed is 1 - value: small terms, not values near 1
        a[1] = (double)(vd / B2);
    }
    block_tree_sum(a, s_tree);
    if (tid == 0) {
        double* out = partial + ((size_t)ch * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        out[0] = a[0]; out[1] = a[1];
    }
}

template <bool kRaw>
__global__ __launch_bounds__(kBlock) void eval_pool_kernel(int W, int H, int W2, int H2, const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ gt_depth, const float* __restrict__ sil, float sil_thres,
                                                           int flags, float* __restrict__ ox, float* __restrict__ oy)
{
    const int64_t n2 = (int64_t)W2 * H2;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= 3 * n2) return;
    const int ch = (int)(i / n2);
    const int64_t q = i - ch * n2;
    const int oyi = (int)(q / W2), oxi = (int)(q - (int64_t)oyi * W2);
    const int bx = 2 * oxi - (W & 1), by = 2 * oyi - (H & 1);
    const size_t HW = (size_t)W * H;
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int gx = bx + k, gy = by + j;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t p = (size_t)gy * W + gx;
                const float m = kRaw ? eval_image_mask(p, gt_depth, sil, sil_thres, flags) : 1.0f;
                sx += x[ch * HW + p] * m; sy += y[ch * HW + p] * m;
            }
        }
    ox[i] = sx * 0.25f; oy[i] = sy * 0.25f;
}

// All totals of a row in ONE tree: 6 sums, 3 same-window SSIM sums, 15 MS-SSIM sums.  (A tree per total -- 24 trees, some 240 barriers -- took
// 33 us of a 96 us call at 256 x 256; the additions of every total and their order are the same here.)
constexpr int kEvalTotals = kEvalSums + 3 + 15;

__global__ __launch_bounds__(kBlock) void eval_finish_kernel(EvalPlan p, int flags, const double* __restrict__ partial, double* __restrict__ row)
{
    __shared__ double s_tree[kEvalTotals][kBlock];
    double s[kEvalTotals];
#pragma unroll
    for (int k = 0; k < kEvalSums; ++k) s[k] = strided_record_sum(partial + k, p.sums_records, kEvalRecord);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        s[kEvalSums + ch] = (flags & GS_EVAL_SSIM) ? strided_record_sum(partial + p.same_off + (int64_t)ch * p.same_tiles * 2, p.same_tiles, 2) : 0.0;
#pragma unroll
        for (int l = 0; l < 5; l++)       // levels 0-3 contribute cs (the second double of a record), level 4 ssim
            s[kEvalSums + 3 + ch * 5 + l] = (flags & GS_EVAL_MS_SSIM)
                ? strided_record_sum(partial + p.ms_off[l] + (int64_t)ch * p.ms_tiles[l] * 2 + (l < 4 ? 1 : 0), p.ms_tiles[l], 2) : 0.0;
    }
    block_tree_sum(s, s_tree);
    if (threadIdx.x != 0) return;
    const double nan = __builtin_nan("");
    const double npix = (double)p.w[0] * (double)p.h[0];
    double psnr = 0.0;
    for (int ch = 0; ch < 3; ch++) psnr += 20.0 * log10(1.0 / sqrt(s[ch] / npix));          // calc_psnr(...).mean(): the mean of three values in dB
    double ssim = nan, ms = nan;
    if (flags & GS_EVAL_SSIM) ssim = 1.0 - ((s[kEvalSums] + s[kEvalSums + 1]) + s[kEvalSums + 2]) / (3.0 * npix);      // (what was summed is 1 - value)
    if (flags & GS_EVAL_MS_SSIM) {
        const double wgt[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        ms = 0.0;
        for (int ch = 0; ch < 3; ch++) {
            double prod = 1.0;
            for (int l = 0; l < 5; l++) {
                // the spatial mean over the valid window's outputs, clamped at 0
                const double n = (double)(p.w[l] - 2 * kLH) * (double)(p.h[l] - 2 * kLH);
                const double t = 1.0 - s[kEvalSums + 3 + ch * 5 + l] / n;
                prod *= pow(t > 0.0 ? t : 0.0, wgt[l]);
            }
            ms += prod;
        }
        ms /= 3.0;
    }
    row[0] = psnr / 3.0;
    row[1] = s[3] / s[5];            // the reference's "Depth RMSE": sum sqrt(d^2) valid / sum valid -- the L1 error again
    row[2] = s[3] / s[5];
    row[3] = ssim;
    row[4] = ms;
    row[5] = s[5];
    row[6] = sqrt(s[4] / s[5]);      // the root of the mean square (not a reference quantity)
    row[7] = 0.0;
}

static int eval_tiles(int w, int h, bool valid)
{
    const int ow = valid ? w - 2 * kLH : w, oh = valid ? h - 2 * kLH : h;
    return ((ow + kLT - 1) / kLT) * ((oh + kLT - 1) / kLT);
}

bool eval_plan(int W, int H, int flags, EvalPlan& p)
{
    p = EvalPlan();
    p.w[0] = W; p.h[0] = H;
    p.ms_defined = (W < H ? W : H) > 160 ? 1 : 0;           // (11 - 1) * 2^4: the smallest side must leave an 11-tap window at level 4
    p.levels = 1;
    const int64_t npix = (int64_t)W * H;
    const int64_t g = (npix + 4 * kBlock - 1) / (4 * kBlock);
    p.sums_records = (int)(g > kBlock ? kBlock : g);
    int64_t d = (int64_t)p.sums_records * kEvalRecord;       // doubles so far
    if (flags & GS_EVAL_SSIM) { p.same_tiles = eval_tiles(W, H, false); p.same_off = d; d += (int64_t)p.same_tiles * 6; }
    if (flags & GS_EVAL_MS_SSIM) {
        if (!p.ms_defined) return false;
        p.levels = 5;
        for (int l = 0; l < 5; l++) {
            if (l) { p.w[l] = p.w[l - 1] / 2 + (p.w[l - 1] & 1); p.h[l] = p.h[l - 1] / 2 + (p.h[l - 1] & 1); }
            p.ms_tiles[l] = eval_tiles(p.w[l], p.h[l], true); p.ms_off[l] = d; d += (int64_t)p.ms_tiles[l] * 6;
        }
    }
    uint64_t bytes = (uint64_t)d * 8u;
    for (int l = 1; l < p.levels; l++) { p.image_off[l] = bytes; bytes += (uint64_t)6 * p.w[l] * p.h[l] * sizeof(float); }
    p.total_bytes = bytes;
    return true;
}

hipError_t launch_eval_frame(const EvalPlan& p, const float* im, const float* depth, const float* sil, const float* gt, const float* gt_depth,
                             float sil_thres, int flags, double* row, void* scratch, hipStream_t st)
{
    const int W = p.w[0], H = p.h[0];
    double* partial = (double*)scratch;
    hipLaunchKernelGGL(eval_sums_kernel, dim3(p.sums_records), dim3(kBlock), 0, st, (int64_t)W * H, im, depth, sil, gt, gt_depth, sil_thres, flags,
                       partial);
    if (flags & GS_EVAL_SSIM)
        hipLaunchKernelGGL((eval_ssim_kernel<false, true>), dim3((W + kLT - 1) / kLT, (H + kLT - 1) / kLT, 3), dim3(kBlock), 0, st, W, H, im, gt,
                           gt_depth, sil, sil_thres, flags, partial + p.same_off);
    if (flags & GS_EVAL_MS_SSIM) {
        const float *x = im, *y = gt;
        for (int l = 0; l < 5; l++) {
            const int w = p.w[l], h = p.h[l];
            const dim3 grid((w - 2 * kLH + kLT - 1) / kLT, (h - 2 * kLH + kLT - 1) / kLT, 3);
            if (l == 0)
                hipLaunchKernelGGL((eval_ssim_kernel<true, true>), grid, dim3(kBlock), 0, st, w, h, x, y, gt_depth, sil, sil_thres, flags,
                                   partial + p.ms_off[l]);
            else
                hipLaunchKernelGGL((eval_ssim_kernel<true, false>), grid, dim3(kBlock), 0, st, w, h, x, y, gt_depth, sil, sil_thres, flags,
                                   partial + p.ms_off[l]);
            if (l == 4) break;
            const int w2 = p.w[l + 1], h2 = p.h[l + 1];
            float* ox = (float*)((char*)scratch + p.image_off[l + 1]);
            float* oy = ox + (size_t)3 * w2 * h2;
            const unsigned nb = (unsigned)(((int64_t)3 * w2 * h2 + kBlock - 1) / kBlock);
            if (l == 0)
                hipLaunchKernelGGL((eval_pool_kernel<true>), dim3(nb), dim3(kBlock), 0, st, w, h, w2, h2, x, y, gt_depth, sil, sil_thres, flags, ox, oy);
            else
                hipLaunchKernelGGL((eval_pool_kernel<false>), dim3(nb), dim3(kBlock), 0, st, w, h, w2, h2, x, y, gt_depth, sil, sil_thres, flags, ox, oy);
            x = ox; y = oy;
        }
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(kBlock), 0, st, p, flags, (const double*)partial, row);
    return hipGetLastError();
}

}  // namespace gs
