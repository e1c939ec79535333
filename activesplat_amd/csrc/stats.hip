// stats.hip -- per-Gaussian densification statistics, one launch each instead of strings of element-wise torch kernels.
//
//  visibility_stats : seen = radii > 0 ; max_2D_radius = max(max_2D_radius, radii)
//                     (src/mapper/splatam/splatam.py:296-298: `seen = radius > 0`, `max_2D_radius[seen] = max(radius[seen], ...)`;
//                      a radius of 0 never raises the maximum, so the masked and the unmasked update are the same)
//  accumulate_grad2d: means2D_gradient_accum[seen] += || means2D.grad[seen, :2] || ; denom[seen] += 1
//                     (src/mapper/splatam/utils/slam_external.py:100-108)
// Pure streaming, 4-16 B per Gaussian.
//
//  grid_dbscan      : DBSCAN on a pixel grid (src/mapper/__init__.py:8-19 and :92-117: sklearn's DBSCAN on np.where(invisibility > t)), batched
//                     over images -- the rule is stated in include/gsplat_hip.h.  Seven launches, no host synchronisation, no sweep loop:
//                       mask bits (one __ballot per 64 columns of a row) -> disc counts from the row bitmasks (2 eps + 1 __popcll per pixel),
//                       core bits, parents initialised to the start of the pixel's run of core pixels -> one union pass over the FORWARD half
//                       of the disc (union by atomic minimum: the root of a component is its smallest pixel index whatever the schedule) ->
//                       flatten + root bits -> per-image scan of the root bits (cluster number = rank of the root) -> labels (a border pixel
//                       takes the smallest root in its disc) and each cluster's row range -> per-cluster sums in a fixed order.
//                     Parents and roots are int32 arrays in global memory (216 KiB per 150 x 360 image: L2 resident); see DESIGN.md.
//
//  high_loss_grid   : the mask of get_high_loss_samples (src/mapper/splatam/__init__.py:212-215) and its cv2.resize to one pixel per degree
//                     (:218) in integers, one launch; the grid is what grid_dbscan reads next.  Rules: include/gsplat_hip.h.
#include "gs_common.h"

namespace gs {

__global__ __launch_bounds__(kBlock) void visibility_stats_kernel(int P, const int32_t* __restrict__ radii, uint8_t* __restrict__ seen,
                                                                   float* __restrict__ max_radius)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const int32_t r = radii[i];
    if (seen) seen[i] = r > 0 ? 1 : 0;
    if (max_radius) max_radius[i] = fmaxf(max_radius[i], (float)r);
}

__global__ __launch_bounds__(kBlock) void accumulate_grad2d_kernel(int P, const float* __restrict__ grad, const uint8_t* __restrict__ seen,
                                                                    float* __restrict__ accum, float* __restrict__ denom)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P || !seen[i]) return;
    const float gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
}

hipError_t launch_visibility_stats(int P, const int32_t* radii, uint8_t* seen, float* max_radius, hipStream_t st)
{
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(visibility_stats_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, st, P, radii, seen, max_radius);
    return hipGetLastError();
}

hipError_t launch_accumulate_grad2d(int P, const float* grad, const uint8_t* seen, float* accum, float* denom, hipStream_t st)
{
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_grad2d_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, st, P, grad, seen, accum, denom);
    return hipGetLastError();
}

// ---- DBSCAN on a pixel grid ----------------------------------------------------------------------------------------------------------------
// One wavefront owns 64 consecutive columns of one row (a "word"): its __ballot is that word of the row's bitmask.

// bits of columns [x0, x0 + n) of a row's bitmask (n <= 17), column x0 in bit 0; columns outside the row read as 0 (the last word of a row has no
// bit at or beyond W: the ballots that wrote it had a false predicate there)
__device__ __forceinline__ uint64_t dbscan_window(const uint64_t* __restrict__ row_words, int Ww, int x0, int n)
{
    const int w0 = x0 >= 0 ? x0 >> 6 : -1, sh = x0 & 63;                 // x0 >= -8: floor(x0 / 64) is -1 for every negative start
    const uint64_t lo = w0 >= 0 && w0 < Ww ? row_words[w0] : 0ull;
    const uint64_t hi = w0 + 1 >= 0 && w0 + 1 < Ww ? row_words[w0 + 1] : 0ull;
    const uint64_t v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return v & ((1ull << n) - 1ull);
}

// the value the threshold is applied to (fp32): v, or 1.0f - v
__device__ __forceinline__ float dbscan_tested(const DbscanArgs& a, int b, int y, int x)
{
    const float v = a.values[(size_t)b * a.image_stride + (size_t)y * a.row_stride + x];
    return a.complement ? 1.0f - v : v;
}

// wave -> (row, word) of image blockIdx.y; false for the waves behind the last word (whole waves: the ballots below see every lane)
__device__ __forceinline__ bool dbscan_wave(const DbscanArgs& a, int& y, int& word, int& x)
{
    const int wid = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (wid >= a.H * a.Ww) return false;
    y = wid / a.Ww; word = wid - y * a.Ww; x = word * kWave + (threadIdx.x & 63);
    return true;
}

__global__ __launch_bounds__(kBlock) void dbscan_mask_kernel(DbscanArgs a)
{
    int y, word, x;
    if (!dbscan_wave(a, y, word, x)) return;
    const int b = blockIdx.y;
    const bool m = x < a.W && dbscan_tested(a, b, y, x) > a.threshold;            // (a NaN compares false: unmasked)
    const uint64_t bits = __ballot(m);
    if ((threadIdx.x & 63) == 0) a.mask_bits[((size_t)b * a.H + y) * a.Ww + word] = bits;
}

__global__ __launch_bounds__(kBlock) void dbscan_core_kernel(DbscanArgs a)
{
    int y, word, x;
    if (!dbscan_wave(a, y, word, x)) return;
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const uint64_t* mb = a.mask_bits + (size_t)b * a.H * a.Ww;
    const bool masked = (mb[(size_t)y * a.Ww + word] >> lane) & 1ull;
    int count = 0;
    if (masked)
        for (int dy = -a.eps; dy <= a.eps; dy++) {
            const int yy = y + dy;
            if (yy < 0 || yy >= a.H) continue;
            const int hw = a.half_width[dy < 0 ? -dy : dy];
            count += __popcll(dbscan_window(mb + (size_t)yy * a.Ww, a.Ww, x - hw, 2 * hw + 1));
        }
    const bool core = masked && count >= a.min_samples;
    const uint64_t bits = __ballot(core);
    if (lane == 0) a.core_bits[((size_t)b * a.H + y) * a.Ww + word] = bits;
    if (x < a.W) {
        // adjacent core pixels of a row are connected: start every pixel at the first pixel of its run inside the word (parent <= self, same
        // component -- the union pass then starts from chains of at most W / 64 links per row instead of W)
        uint32_t parent = 0xffffffffu;
        if (core) {
            const uint64_t gaps = ~bits & ((1ull << lane) - 1ull);
            parent = (uint32_t)(y * a.W + word * kWave + (gaps ? 64 - __clzll(gaps) : 0));
        }
        a.parent[(size_t)b * a.npix + y * a.W + x] = ~parent;                       // stored complemented: a minimum is an atomicMax
    }
}

// root of x's tree: the chain descends strictly (parent < child), so it ends within npix steps whatever other workgroups do meanwhile; the
// nodes on the way are then pointed at the root found (it is in their component and not above their parent: the forest stays a forest)
__device__ __forceinline__ uint32_t dbscan_find(uint32_t* __restrict__ C, uint32_t x, int npix, bool compress)
{
    const uint32_t first = ~__hip_atomic_load(&C[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t r = first;
    for (int i = 0; i < npix; i++) {
        const uint32_t p = ~__hip_atomic_load(&C[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == r) break;
        r = p;
    }
    if (compress && first != r)                          // (a node that already points at the root costs no atomic)
        for (int i = 0; i < npix && x > r; i++) x = ~atomicMax(&C[x], ~r);
    return r;
}

// unite the trees of a and b: the larger root is hung below the smaller by an atomic minimum.  When the minimum finds the slot already
// lowered by somebody else (old != a), a continues from that smaller value: a + b falls by at least one per round, so the loop ends within
// 2 npix rounds; the bound is written out so that no input and no schedule can keep a wavefront here.
__device__ __forceinline__ void dbscan_union(uint32_t* __restrict__ C, uint32_t a, uint32_t b, int npix)
{
    for (int it = 0; it < 2 * npix + 2; it++) {
        a = dbscan_find(C, a, npix, true);
        b = dbscan_find(C, b, npix, true);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = ~atomicMax(&C[a], ~b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(kBlock) void dbscan_union_kernel(DbscanArgs a)
{
    const int b = blockIdx.y, p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.npix) return;
    const int y = p / a.W, x = p - y * a.W;
    const uint64_t* cb = a.core_bits + (size_t)b * a.H * a.Ww;
    if (!((cb[(size_t)y * a.Ww + (x >> 6)] >> (x & 63)) & 1ull)) return;
    uint32_t* C = a.parent + (size_t)b * a.npix;
    // the forward half of the disc.  Own row: the nearest core pixel to the right (the ones behind it hang on that one) -- unless it is the
    // adjacent pixel of the same word, which dbscan_core_kernel already put into this pixel's tree.
    const uint64_t right = dbscan_window(cb + (size_t)y * a.Ww, a.Ww, x + 1, a.eps);
    if (right) {
        const int k = __ffsll((unsigned long long)right) - 1;
        if (k > 0 || ((x + 1) & 63) == 0) dbscan_union(C, (uint32_t)p, (uint32_t)(p + 1 + k), a.npix);
    }
    // rows below: the first pixel of every run of core pixels in the window (a run is connected along its own row).  When the pixel to the
    // left is core it is in this pixel's component and its window is this one shifted by a column: it (or a pixel further left) has taken
    // every run that reaches into its window, and only a run that BEGINS in the window's last column is left for this pixel.
    const bool left_core = x > 0 && ((cb[(size_t)y * a.Ww + ((x - 1) >> 6)] >> ((x - 1) & 63)) & 1ull);
    for (int dy = 1; dy <= a.eps && y + dy < a.H; dy++) {
        const int hw = a.half_width[dy];
        uint64_t m = dbscan_window(cb + (size_t)(y + dy) * a.Ww, a.Ww, x - hw, 2 * hw + 1);
        m &= ~(m << 1);
        if (left_core) m &= 1ull << (2 * hw);
        while (m) {
            const int k = __ffsll((unsigned long long)m) - 1;
            m &= m - 1ull;
            dbscan_union(C, (uint32_t)p, (uint32_t)((y + dy) * a.W + x - hw + k), a.npix);
        }
    }
}

__global__ __launch_bounds__(kBlock) void dbscan_flatten_kernel(DbscanArgs a)
{
    int y, word, x;
    if (!dbscan_wave(a, y, word, x)) return;
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const bool core = (a.core_bits[((size_t)b * a.H + y) * a.Ww + word] >> lane) & 1ull;
    int32_t r = -1;
    if (core) r = (int32_t)dbscan_find(a.parent + (size_t)b * a.npix, (uint32_t)(y * a.W + x), a.npix, false);
    if (x < a.W) a.root[(size_t)b * a.npix + y * a.W + x] = r;
    const uint64_t bits = __ballot(core && r == y * a.W + x);
    if (lane == 0) a.root_bits[((size_t)b * a.H + y) * a.Ww + word] = bits;
}

// exclusive scan of the root bits' popcounts over the words of one image, row-major: a root's cluster number is word_prefix[its word] + the
// number of roots below it in the word.  Also resets the clusters' row ranges for the labelling kernel.
__global__ __launch_bounds__(kBlock) void dbscan_scan_kernel(DbscanArgs a)
{
    __shared__ uint32_t s_sum[kBlock];
    const int b = blockIdx.x, t = threadIdx.x, nwords = a.H * a.Ww, per = (nwords + kBlock - 1) / kBlock;
    const uint64_t* rb = a.root_bits + (size_t)b * nwords;
    const int w0 = t * per < nwords ? t * per : nwords, w1 = w0 + per < nwords ? w0 + per : nwords;
    uint32_t s = 0;
    for (int w = w0; w < w1; w++) s += (uint32_t)__popcll(rb[w]);
    s_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < kBlock; i++) { const uint32_t v = s_sum[i]; s_sum[i] = run; run += v; }
        a.n_clusters[b] = (int32_t)run;
    }
    __syncthreads();
    uint32_t run = s_sum[t];
    for (int w = w0; w < w1; w++) { a.word_prefix[(size_t)b * nwords + w] = run; run += (uint32_t)__popcll(rb[w]); }
    for (int c = t; c < 2 * a.max_clusters; c += kBlock) a.row_range[(size_t)b * 2 * a.max_clusters + c] = 0u;
}

__global__ __launch_bounds__(kBlock) void dbscan_label_kernel(DbscanArgs a)
{
    int y, word, x;
    if (!dbscan_wave(a, y, word, x)) return;
    const int b = blockIdx.y, lane = threadIdx.x & 63, nwords = a.H * a.Ww;
    const uint64_t* mb = a.mask_bits + (size_t)b * nwords;
    const uint64_t* cb = a.core_bits + (size_t)b * nwords;
    const int32_t* root = a.root + (size_t)b * a.npix;
    const bool masked = (mb[(size_t)y * a.Ww + word] >> lane) & 1ull;
    int32_t label = -2;
    if (masked) {
        int32_t r = x < a.W ? root[y * a.W + x] : -1;
        if (r < 0) {
            // border rule: the smallest cluster number among the core pixels of the disc = the smallest root (numbers ascend with the roots)
            int32_t best = 0x7fffffff;
            for (int dy = -a.eps; dy <= a.eps; dy++) {
                const int yy = y + dy;
                if (yy < 0 || yy >= a.H) continue;
                const int hw = a.half_width[dy < 0 ? -dy : dy];
                uint64_t m = dbscan_window(cb + (size_t)yy * a.Ww, a.Ww, x - hw, 2 * hw + 1);
                while (m) {
                    const int k = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1ull;
                    const int32_t q = root[yy * a.W + x - hw + k];
                    best = q < best ? q : best;
                }
            }
            r = best == 0x7fffffff ? -1 : best;
        }
        label = -1;
        if (r >= 0) {
            const int ry = r / a.W, rx = r - ry * a.W, rw = ry * a.Ww + (rx >> 6);
            label = (int32_t)(a.word_prefix[(size_t)b * nwords + rw] + (uint32_t)__popcll(a.root_bits[(size_t)b * nwords + rw] & ((1ull << (rx & 63)) - 1ull)));
            if (r == y * a.W + x && label < a.max_clusters) a.table[((size_t)b * a.max_clusters + label) * 4 + 3] = r;
        }
    }
    if (x < a.W) a.labels[(size_t)b * a.npix + y * a.W + x] = label;
    // the cluster's first and last row (maxima of ~row and row: order-free); one atomic pair per run of equal labels along the row
    const int32_t left = __shfl_up(label, 1);
    if (label >= 0 && label < a.max_clusters && (lane == 0 || left != label)) {
        uint32_t* rr = a.row_range + ((size_t)b * a.max_clusters + label) * 2;
        atomicMax(&rr[0], ~(uint32_t)y);
        atomicMax(&rr[1], (uint32_t)y);
    }
}

constexpr int kDbscanSumBlock = 1024;

// fixed-order sums: thread t takes the elements t, t + 1024, ... of its range (at most 64 terms for the 65 536 pixels the call admits), then a
// butterfly over the wavefront, then a butterfly of the 16 wavefront sums.  Block 0 of an image: the sum of the tested value over the whole
// image; block 1 + c: cluster c's row of the table, summed over the rows the cluster touches.  Values that are not finite count as 0.
__global__ __launch_bounds__(kDbscanSumBlock) void dbscan_sums_kernel(DbscanArgs a)
{
    __shared__ float s_v[kDbscanSumBlock / kWave];
    __shared__ int32_t s_i[3][kDbscanSumBlock / kWave];
    const int b = blockIdx.y, c = (int)blockIdx.x - 1, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int y0 = 0, y1 = a.H - 1;
    if (c >= 0) {
        if (c >= a.n_clusters[b]) {
            if (t < 4) a.table[((size_t)b * a.max_clusters + c) * 4 + t] = t == 3 ? -1 : 0;
            if (t == 0) a.sum_value[(size_t)b * a.max_clusters + c] = 0.f;
            return;
        }
        const uint32_t* rr = a.row_range + ((size_t)b * a.max_clusters + c) * 2;
        y0 = (int)~rr[0]; y1 = (int)rr[1];
    }
    const int n = (y1 - y0 + 1) * a.W;
    const int32_t* labels = a.labels + (size_t)b * a.npix + y0 * a.W;
    float sv = 0.f;
    int32_t cnt = 0, sr = 0, sc = 0;
    for (int i = t; i < n; i += kDbscanSumBlock) {
        if (c >= 0 && labels[i] != c) continue;
        const int dy = i / a.W, x = i - dy * a.W;
        const float v = dbscan_tested(a, b, y0 + dy, x);
        sv += fabsf(v) <= 3.402823466e38f ? v : 0.f;
        cnt += 1; sr += y0 + dy; sc += x;
    }
    for (int m = 1; m < kWave; m <<= 1) { sv += __shfl_xor(sv, m); cnt += __shfl_xor(cnt, m); sr += __shfl_xor(sr, m); sc += __shfl_xor(sc, m); }
    if (lane == 0) { s_v[wave] = sv; s_i[0][wave] = cnt; s_i[1][wave] = sr; s_i[2][wave] = sc; }
    __syncthreads();
    if (wave == 0) {
        const bool in = lane < kDbscanSumBlock / kWave;
        sv = in ? s_v[lane] : 0.f; cnt = in ? s_i[0][lane] : 0; sr = in ? s_i[1][lane] : 0; sc = in ? s_i[2][lane] : 0;
        for (int m = 1; m < kDbscanSumBlock / kWave; m <<= 1) { sv += __shfl_xor(sv, m); cnt += __shfl_xor(cnt, m); sr += __shfl_xor(sr, m); sc += __shfl_xor(sc, m); }
        if (lane == 0) {
            if (c < 0) a.total[b] = sv;
            else {
                int32_t* row = a.table + ((size_t)b * a.max_clusters + c) * 4;
                row[0] = cnt; row[1] = sr; row[2] = sc;
                a.sum_value[(size_t)b * a.max_clusters + c] = sv;
            }
        }
    }
}

hipError_t launch_grid_dbscan(const DbscanArgs& a, int B, hipStream_t st)
{
    const dim3 waves((a.H * a.Ww + kBlock / kWave - 1) / (kBlock / kWave), B), pixels((a.npix + kBlock - 1) / kBlock, B);
    hipLaunchKernelGGL(dbscan_mask_kernel, waves, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(dbscan_core_kernel, waves, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(dbscan_union_kernel, pixels, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(dbscan_flatten_kernel, waves, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(dbscan_scan_kernel, dim3(B), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(dbscan_label_kernel, waves, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(dbscan_sums_kernel, dim3(1 + a.max_clusters, B), dim3(kDbscanSumBlock), 0, st, a);
    return hipGetLastError();
}

// ---- the per-frame high-loss mask and its grid ------------------------------------------------------------------------------------------------
// (src/mapper/splatam/__init__.py:212-218; both rules are stated in include/gsplat_hip.h, gs_high_loss_grid)

// the pixel rule, fp32, operation for operation the reference's; every comparison with a NaN is false
__device__ __forceinline__ int high_loss_pixel(const HighLossArgs& a, int i)
{
    const float d = a.depth[i], g = a.gt[i];
    const float err = fabsf(d - g) * (g > 0.0f ? 1.0f : 0.0f);
    return (d > g && err > a.depth_thres && a.opacity[i] > a.opacity_thres) ? 1 : 0;
}

// one axis of the resize in integers: the two taps (clamped into the source) and the weight of the second, out of den = 2 n_dst
__device__ __forceinline__ void high_loss_taps(int d, int n_src, int n_dst, int& t0, int& t1, int& w1)
{
    const int den = 2 * n_dst, num = (2 * d + 1) * n_src - n_dst;      // |num| < 2^28 for the sizes the call admits
    int i0 = num / den;
    if (num - i0 * den < 0) i0 -= 1;                                   // floor towards -inf: num is negative at the first samples when upsampling
    w1 = num - i0 * den;
    t0 = i0 < 0 ? 0 : (i0 > n_src - 1 ? n_src - 1 : i0);
    t1 = i0 + 1 < 0 ? 0 : (i0 + 1 > n_src - 1 ? n_src - 1 : i0 + 1);
}

// thread i: pixel i of the full-resolution mask (when asked for) and pixel i of the grid.  The grid evaluates the pixel rule at its four taps
// itself, so it does not wait for (or depend on) the mask.
__global__ __launch_bounds__(kBlock) void high_loss_grid_kernel(HighLossArgs a)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (a.mask_full && i < a.W * a.H) a.mask_full[i] = (uint8_t)high_loss_pixel(a, i);
    if (i >= a.gw * a.gh) return;
    const int gy = i / a.gw, gx = i - gy * a.gw;
    int x0, x1, wx1, y0, y1, wy1;
    high_loss_taps(gx, a.W, a.gw, x0, x1, wx1);
    high_loss_taps(gy, a.H, a.gh, y0, y1, wy1);
    const int den_x = 2 * a.gw, den_y = 2 * a.gh, wx0 = den_x - wx1, wy0 = den_y - wy1;
    const int S = high_loss_pixel(a, y0 * a.W + x0) * wy0 * wx0 + high_loss_pixel(a, y0 * a.W + x1) * wy0 * wx1 +
                  high_loss_pixel(a, y1 * a.W + x0) * wy1 * wx0 + high_loss_pixel(a, y1 * a.W + x1) * wy1 * wx1;
    a.grid[i] = 2 * S >= den_x * den_y ? 1.0f : 0.0f;                  // S <= den_x * den_y <= 2^26: the bilinear value rounded half up
}

hipError_t launch_high_loss_grid(const HighLossArgs& a, hipStream_t st)
{
    const int npix = a.mask_full ? a.W * a.H : 0, ngrid = a.gw * a.gh, n = npix > ngrid ? npix : ngrid;
    hipLaunchKernelGGL(high_loss_grid_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace gs
