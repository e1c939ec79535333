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
//
//  planner roadmap  : traversable map, clearance field, integer medial axis, geodesic fields, nodes and paths on the planner's top-down maps
//                     (a grid formulation of src/planner/planner.py:111-370, at the end of this file).  Rules: include/gsplat_hip.h.
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

// ---- hull volumes of the clusters ----------------------------------------------------------------------------------------------------------------
// (src/mapper/__init__.py:29-90; the rule a-f is stated in include/gsplat_hip.h, gs_cluster_hulls)
// Workgroups of ONE wavefront, one per CU (kHullGroups), each walking the (image, cluster slot) pairs in cluster-major order with a stride of
// the grid: the cluster counts stay on the device, a slot at or beyond n_clusters[b] costs one compare, and the LDS below is claimed once per
// CU, not once per slot (a grid of max_clusters x B workgroups queues 5376 of them behind it: measured 1.86 ms against 0.56 ms
// for 21 panoramas of three clusters, profiles/hull_volumes.txt).  Everything between
// the labels and the volume stays in LDS: the cluster's bitmask as 64-bit row words, its dilation by word shifts, the border following by
// lane 0 over the dilated words, then -- in the same LDS, the bitmasks being dead by then -- the contour points and the faces of an
// incremental hull whose face tests, horizon search and face replacement are spread over the 64 lanes.  Nothing depends on scheduling: there
// is no atomic, the faces are kept in an order that follows from the points alone, and the volume is summed per lane and by a butterfly.
// LDS: 40 + 48 + 32 + 16 KiB = 136 KiB of the CU's 160, so one workgroup per CU -- a query has about as many live clusters as the chip has CUs,
// and a workgroup's time is expected to go to the ~1000 dependent steps of the trace and the point-by-point hull, not to occupancy (the split
// between the phases has not been measured; profiles/hull_volumes.txt has the kernel's time as a whole).
// Cost of the hull per inserted point that sees V faces: the nf face tests over 64 lanes, then the horizon search, which tests each of the 3 V
// edges against all V visible faces, 3 V^2 / 64 per lane.  V is a handful for a contour in general position but can reach all 2 n - 4 faces
// (a point far outside a nearly flat cluster); with n at its limit of 4096 that is ~3e6 steps for one point, the worst case of this kernel.
// Contours of the shipped query have a few hundred points (profiles/hull_volumes.txt).

constexpr int kHullWords = 65536 / 64 + 4096;            // H * ceil(W / 64) for H * W <= 65536, H <= 4096
constexpr int kHullMaxPoints = 4096;
constexpr int kHullMaxFaces = 2 * kHullMaxPoints - 4;    // a triangulated sphere on n vertices has 2 n - 4 faces
constexpr int kHullGroups = 256;                         // the workgroups of the grid: one per CU of the MI355X.  Any count gives the same results
                                                         // (a workgroup takes every kHullGroups-th slot); on a part with fewer CUs the rest wait their turn
constexpr int kHullOverflow = 1, kHullNonFinite = 2, kHullTruncated = 4, kHullFaces = 8;       // status bits

struct HullPoint { int16_t x, y; float z; };

// direction codes 0..7 of the border following: (dx, dy) = (1,0),(1,-1),(0,-1),(-1,-1),(-1,0),(-1,1),(0,1),(1,1), two bits each of dx + 1 / dy + 1
__device__ __forceinline__ int hull_dx(int s) { return ((0x901A >> (2 * s)) & 3) - 1; }
__device__ __forceinline__ int hull_dy(int s) { return ((0xA901 >> (2 * s)) & 3) - 1; }

__device__ __forceinline__ bool hull_bit(const uint64_t* __restrict__ bits, int H, int W, int Ww, int x, int y)
{
    if (x < 0 || y < 0 || x >= W || y >= H) return false;
    return (bits[y * Ww + (x >> 6)] >> (x & 63)) & 1ull;
}

// det [b - a; c - a; d - a] in pixel units, fp64, no contraction (the emulated build and the device then take the same decisions): > 0 iff d
// sees the face (a, b, c) from outside.  Integer x and y differences are exact, so four points that share a column, a row or a depth give
// exactly 0.
__device__ __forceinline__ double hull_orient(const HullPoint& a, const HullPoint& b, const HullPoint& c, const HullPoint& d)
{
#pragma clang fp contract(off)
    const double bx = (double)(b.x - a.x), by = (double)(b.y - a.y), bz = (double)b.z - (double)a.z;
    const double cx = (double)(c.x - a.x), cy = (double)(c.y - a.y), cz = (double)c.z - (double)a.z;
    const double dx = (double)(d.x - a.x), dy = (double)(d.y - a.y), dz = (double)d.z - (double)a.z;
    const double m0 = cy * dz - cz * dy, m1 = cx * dz - cz * dx, m2 = cx * dy - cy * dx;
    return (bx * m0 - by * m1) + bz * m2;
}

// true iff a, b, c are not on one line (a component of (b - a) x (c - a) is not 0)
__device__ __forceinline__ bool hull_spans(const HullPoint& a, const HullPoint& b, const HullPoint& c)
{
#pragma clang fp contract(off)
    const double bx = (double)(b.x - a.x), by = (double)(b.y - a.y), bz = (double)b.z - (double)a.z;
    const double cx = (double)(c.x - a.x), cy = (double)(c.y - a.y), cz = (double)c.z - (double)a.z;
    return by * cz - bz * cy != 0.0 || bz * cx - bx * cz != 0.0 || bx * cy - by * cx != 0.0;
}

// one live cluster c of image b, by the whole wavefront; the LDS arrays are the kernel's
__device__ __forceinline__ void cluster_hull_slot(const HullArgs& a, int b, int c, uint64_t* s_mask, uint64_t* s_dil, uint32_t* s_horizon,
                                                  uint16_t* s_vlist, int& s_emitted)
{
    const int lane = threadIdx.x, H = a.H, W = a.W, Ww = a.Ww, nwords = H * Ww;
    const size_t slot = (size_t)b * a.max_clusters + c;
    const uint64_t below = (1ull << lane) - 1ull;
    int status = 0;
    double volume = 0.0;
    int n_emitted = 0;
    HullPoint* pts = reinterpret_cast<HullPoint*>(s_mask);
    uint16_t* faces = reinterpret_cast<uint16_t*>(s_dil);

    // a. the mask: one ballot per 64 columns of a row
    {
        const int32_t* lab = a.labels + (size_t)b * H * W;
        for (int idx0 = 0; idx0 < nwords; idx0 += 4) {                // four words per step: their loads are in flight together
            bool m[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int idx = idx0 + k, y = idx / Ww, x = (idx - y * Ww) * kWave + lane;
                m[k] = idx < nwords && x < W && lab[y * W + x] == c;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t bits = __ballot(m[k]);
                if (lane == 0 && idx0 + k < nwords) s_mask[idx0 + k] = bits;
            }
        }
    }
    __syncthreads();
    // b. the dilation: per output word and footprint row the three source words once, then one shift per set cell
    {
        const int ay = a.kh / 2, ax = a.kw / 2;
        for (int idx = lane; idx < nwords; idx += kWave) {
            const int y = idx / Ww, w = idx - y * Ww;
            uint64_t out = 0;
            for (int i = 0; i < a.kh; i++) {
                const int yy = y + i - ay;
                const uint32_t fr = a.footprint[i];
                if (yy < 0 || yy >= H || !fr) continue;
                const uint64_t* row = s_mask + yy * Ww;
                const uint64_t cur = row[w], prev = w > 0 ? row[w - 1] : 0ull, next = w + 1 < Ww ? row[w + 1] : 0ull;
                for (int j = 0; j < a.kw; j++) {
                    if (!((fr >> j) & 1u)) continue;
                    const int d = j - ax;                              // dil(x) |= mask(x + d), |d| <= 7
                    out |= d == 0 ? cur : (d > 0 ? (cur >> d) | (next << (64 - d)) : (cur << -d) | (prev >> (64 + d)));
                }
            }
            if (w == Ww - 1 && (W & 63)) out &= (1ull << (W & 63)) - 1ull;
            s_dil[idx] = out;
        }
    }
    __syncthreads();
    // c. the start: the first set pixel in row-major order
    int first = -1;
    for (int base = 0; base < nwords; base += kWave) {
        const uint64_t bal = __ballot(base + lane < nwords && s_dil[base + lane] != 0ull);
        if (bal) { first = base + __ffsll((unsigned long long)bal) - 1; break; }
    }
    if (first >= 0) {
        if (lane == 0) {
            const int y0 = first / Ww, x0 = (first - y0 * Ww) * 64 + __ffsll((unsigned long long)s_dil[first]) - 1;
            int n = 0, s = 4;
            bool single = true;
            do {
                s = (s - 1) & 7;
                if (hull_bit(s_dil, H, W, Ww, x0 + hull_dx(s), y0 + hull_dy(s))) { single = false; break; }
            } while (s != 4);
            if (single) {
                pts[0].x = (int16_t)x0; pts[0].y = (int16_t)y0;
                n = 1;
            } else {
                const int x1 = x0 + hull_dx(s), y1 = y0 + hull_dy(s), max_steps = 4 * H * W + 8;
                int px = x0, py = y0, prev = s ^ 4;
                for (int step = 0; step < max_steps; step++) {
                    int sp = s, qx = 0, qy = 0;
                    bool found = false;
                    for (int k = 0; k < 8 && !found; k++) {
                        sp = (sp + 1) & 7;
                        qx = px + hull_dx(sp); qy = py + hull_dy(sp);
                        found = hull_bit(s_dil, H, W, Ww, qx, qy);
                    }
                    if (!found) break;                                 // (p has a set neighbour: it was reached from one)
                    if (sp != prev) {
                        if (n < a.max_points) { pts[n].x = (int16_t)px; pts[n].y = (int16_t)py; }
                        n++;
                        prev = sp;
                    }
                    if (qx == x0 && qy == y0 && px == x1 && py == y1) break;
                    px = qx; py = qy; s = (sp + 4) & 7;
                }
            }
            s_emitted = n;
        }
        __syncthreads();
        n_emitted = s_emitted;
    }
    if (n_emitted > a.max_points) status |= kHullOverflow;
    // d. the depths of the emitted points; the points that stay are packed to the front in their order
    const int n_stored = n_emitted < a.max_points ? n_emitted : a.max_points;
    int n = 0, bad = 0;
    for (int base = 0; base < n_stored; base += kWave) {
        const int i = base + lane;
        HullPoint p = {0, 0, 0.f};
        bool keep = false;
        if (i < n_stored) {
            p = pts[i];
            p.z = a.depth[(size_t)b * a.image_stride + (size_t)p.y * a.row_stride + p.x];
            if (a.contour_xy) {
                int32_t* xy = a.contour_xy + (slot * a.max_points + i) * 2;
                xy[0] = p.x; xy[1] = p.y;
            }
            const bool finite = fabsf(p.z) <= 3.402823466e38f;
            bad |= finite ? 0 : 1;
            keep = finite && p.z != a.skip_depth;
        }
        const uint64_t bal = __ballot(keep);
        __syncthreads();
        if (keep) pts[n + __popcll(bal & below)] = p;
        n += __popcll(bal);
        __syncthreads();
    }
    if (__ballot(bad) != 0ull) status |= kHullNonFinite;
    // e. the hull of the n points
    if (!(status & kHullOverflow) && n >= 4) {
        auto first_point = [&](auto pred) -> int {
            for (int base = 0; base < n; base += kWave) {
                const uint64_t bal = __ballot(base + lane < n && pred(pts[base + lane]));
                if (bal) return base + __ffsll((unsigned long long)bal) - 1;
            }
            return -1;
        };
        const HullPoint P0 = pts[0];
        int i1 = first_point([&](const HullPoint& p) { return p.x != P0.x || p.y != P0.y || p.z != P0.z; }), i2 = -1, i3 = -1;
        HullPoint P1 = P0, P2 = P0;
        if (i1 >= 0) { P1 = pts[i1]; i2 = first_point([&](const HullPoint& p) { return hull_spans(P0, P1, p); }); }
        if (i2 >= 0) { P2 = pts[i2]; i3 = first_point([&](const HullPoint& p) { return hull_orient(P0, P1, P2, p) != 0.0; }); }
        if (i3 >= 0) {
            if (hull_orient(P0, P1, P2, pts[i3]) > 0.0) { const int t = i1; i1 = i2; i2 = t; }
            if (lane == 0) {                                           // (a, b, c), (b, a, d), (c, b, d), (a, c, d): d = i3 behind every face
                const uint16_t f0[12] = {0, (uint16_t)i1, (uint16_t)i2, (uint16_t)i1, 0, (uint16_t)i3, (uint16_t)i2, (uint16_t)i1, (uint16_t)i3, 0, (uint16_t)i2, (uint16_t)i3};
                for (int k = 0; k < 12; k++) faces[k] = f0[k];
            }
            __syncthreads();
            int nf = 4;
            const int cap = 2 * n - 4;
            bool failed = false;
            for (int ip = 1; ip < n && !failed; ip++) {
                if (ip == i1 || ip == i2 || ip == i3) continue;
                const HullPoint P = pts[ip];
                int V = 0;                                             // the faces P sees, in ascending order
                for (int base = 0; base < nf; base += kWave) {
                    const int f = base + lane;
                    const bool vis = f < nf && hull_orient(pts[faces[3 * f]], pts[faces[3 * f + 1]], pts[faces[3 * f + 2]], P) > 0.0;
                    const uint64_t bal = __ballot(vis);
                    if (vis) s_vlist[V + __popcll(bal & below)] = (uint16_t)f;
                    V += __popcll(bal);
                }
                if (V == 0) continue;                                  // inside or on the hull
                __syncthreads();
                int Hn = 0;                                            // horizon: the edges of visible faces whose reverse no visible face has
                for (int base = 0; base < 3 * V; base += kWave) {
                    const int t = base + lane;
                    bool hz = false;
                    uint32_t u = 0, v = 0;
                    if (t < 3 * V) {
                        const int f = s_vlist[t / 3], e = t % 3;
                        u = faces[3 * f + e]; v = faces[3 * f + (e == 2 ? 0 : e + 1)];
                        hz = true;
                        for (int g = 0; g < V && hz; g++) {
                            const uint16_t* fg = faces + 3 * s_vlist[g];
                            hz = !((fg[0] == v && fg[1] == u) || (fg[1] == v && fg[2] == u) || (fg[2] == v && fg[0] == u));
                        }
                    }
                    const uint64_t bal = __ballot(hz);
                    const int at = Hn + __popcll(bal & below);
                    if (hz && at < kHullMaxFaces) s_horizon[at] = u | (v << 16);
                    Hn += __popcll(bal);
                }
                if (nf - V + Hn > cap) { failed = true; break; }      // (not a sphere any more: rounding made the visible set ragged)
                __syncthreads();
                for (int k = lane; k < Hn; k += kWave) {               // the fan over the horizon: into the holes first, then behind the last face
                    const int at = k < V ? s_vlist[k] : nf + (k - V);
                    const uint32_t e = s_horizon[k];
                    faces[3 * at] = (uint16_t)(e & 0xffffu); faces[3 * at + 1] = (uint16_t)(e >> 16); faces[3 * at + 2] = (uint16_t)ip;
                }
                __syncthreads();
                if (Hn < V) {                                          // holes left: filled from the tail, the highest hole first
                    if (lane == 0) {
                        int last = nf - 1;
                        for (int k = V - 1; k >= Hn; k--, last--) {
                            const int h = s_vlist[k];
                            if (h != last) { faces[3 * h] = faces[3 * last]; faces[3 * h + 1] = faces[3 * last + 1]; faces[3 * h + 2] = faces[3 * last + 2]; }
                        }
                    }
                    __syncthreads();
                }
                nf = nf - V + Hn;
            }
            if (failed) status |= kHullFaces;
            else {
                double acc = 0.0;                                      // six times the volume: the cones from point 0 over the faces
                for (int f = lane; f < nf; f += kWave) acc += hull_orient(P0, pts[faces[3 * f]], pts[faces[3 * f + 1]], pts[faces[3 * f + 2]]);
                for (int m = 1; m < kWave; m <<= 1) acc += __shfl_xor(acc, m);
                volume = acc / 6.0 * a.scale;
            }
        }
    }
    if (lane == 0) { a.volume[slot] = volume; a.n_points[slot] = n_emitted; a.cluster_status[slot] = status; }
}

__global__ __launch_bounds__(kWave) void cluster_hull_kernel(HullArgs a, int B)
{
    __shared__ uint64_t s_mask[kHullWords];                            // the cluster's bitmask; from the trace on: the points
    __shared__ uint64_t s_dil[kHullWords + 1024];                      // its dilation; from the hull on: the faces, three uint16 each
    __shared__ uint32_t s_horizon[kHullMaxFaces + 4];                  // horizon edges u | v << 16
    __shared__ uint16_t s_vlist[kHullMaxFaces + 4];                    // the visible faces, ascending
    __shared__ int s_emitted;
    static_assert(sizeof(HullPoint) == 8 && kHullMaxPoints * sizeof(HullPoint) <= sizeof(uint64_t) * kHullWords, "points alias the mask words");
    static_assert(kHullMaxFaces * 6 <= (kHullWords + 1024) * 8, "faces alias the dilated words");
    const int64_t total = (int64_t)B * a.max_clusters;
    // the slots at or beyond n_clusters[b]: their zeros, one slot per lane
    for (int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x; i < total; i += (int64_t)gridDim.x * kWave) {
        const int b = (int)(i / a.max_clusters), c = (int)(i - (int64_t)b * a.max_clusters);
        if (c >= a.n_clusters[b]) { a.volume[i] = 0.0; a.n_points[i] = 0; a.cluster_status[i] = 0; }
    }
    // the live ones, cluster-major: cluster c of every image before cluster c + 1 of any, so that they spread over the workgroups
    for (int64_t i = blockIdx.x; i < total; i += gridDim.x) {
        const int c = (int)(i / B), b = (int)(i - (int64_t)c * B);
        if (c >= a.n_clusters[b]) continue;
        cluster_hull_slot(a, b, c, s_mask, s_dil, s_horizon, s_vlist, s_emitted);
        __syncthreads();                                               // (the next cluster overwrites the LDS)
    }
}

// f. per image, thread b: the two sums over the clusters in ascending number, fp64
__global__ __launch_bounds__(kWave) void cluster_hull_sums_kernel(HullArgs a, int B)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * kWave + threadIdx.x;
    if (b >= B) return;
    const int n = a.n_clusters[b], m = n < a.max_clusters ? n : a.max_clusters;
    double sv = 0.0, si = 0.0;
    int st = n > a.max_clusters ? kHullTruncated : 0;
    for (int c = 0; c < m; c++) {
        const size_t slot = (size_t)b * a.max_clusters + c;
        const double v = a.volume[slot];
        sv += v;
        si += (double)a.sum_value[slot] * v;
        st |= a.cluster_status[slot];
    }
    a.sum_volume[b] = sv; a.sum_invisibility[b] = si; a.status[b] = st;
}

hipError_t launch_cluster_hulls(const HullArgs& a, int B, hipStream_t st)
{
    const int64_t total = (int64_t)B * a.max_clusters;
    hipLaunchKernelGGL(cluster_hull_kernel, dim3((unsigned)(total < kHullGroups ? total : kHullGroups)), dim3(kWave), 0, st, a, B);
    hipLaunchKernelGGL(cluster_hull_sums_kernel, dim3((B + kWave - 1) / kWave), dim3(kWave), 0, st, a, B);
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

// ---- planner roadmap: traversable map, clearance field, Voronoi skeleton, geodesic fields, nodes, paths ------------------------------------------
// (a grid formulation of src/planner/planner.py:111-370; every rule is stated in include/gsplat_hip.h, gs_traversable_map .. gs_trace_path).
// Maps are bytes, one pixel per thread, all arithmetic in integers; nothing depends on the schedule: the labelling reuses grid_dbscan's union by
// atomic minimum (the root of a component is its smallest pixel whatever the order), the fields are relaxed between two buffers (a round is a
// function of the previous round), everything else is a gather.

__device__ __forceinline__ bool road_pixel(const RoadGrid& g, int& r, int& c)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= g.npix) return false;
    r = p / g.W; c = p - r * g.W;
    return true;
}

// step 1 and the erosion half of step 2: e(r, c) = the open_size x open_size square whose top-left pixel is (r, c) lies in the image and in m0
__global__ __launch_bounds__(kBlock) void trav_erode_kernel(TravArgs a)
{
    int r, c;
    if (!road_pixel(a.g, r, c)) return;
    const int s = a.open_size, W = a.g.W;
    bool all = r + s <= a.g.H && c + s <= W;
    for (int i = 0; all && i < s; i++)
        for (int j = 0; all && j < s; j++) {
            const int q = (r + i) * W + c + j;
            all = a.free_map[q] != 0 && a.unseen[q] == 0;
        }
    a.map_a[r * W + c] = all ? 1 : 0;
}

// the other half of step 2: a pixel is in the opening iff one of the squares that cover it is whole
__global__ __launch_bounds__(kBlock) void trav_open_kernel(TravArgs a)
{
    int r, c;
    if (!road_pixel(a.g, r, c)) return;
    const int s = a.open_size, W = a.g.W;
    bool any = false;
    for (int i = 0; !any && i < s && i <= r; i++)
        for (int j = 0; !any && j < s && j <= c; j++) any = a.map_a[(r - i) * W + c - j] != 0;
    a.map_b[r * W + c] = any ? 1 : 0;
}

// step 3, and every pixel starts as its own root (parents complemented, as grid_dbscan's)
__global__ __launch_bounds__(kBlock) void trav_dilate_kernel(TravArgs a)
{
    int r, c;
    if (!road_pixel(a.g, r, c)) return;
    const int h = a.dilate / 2, W = a.g.W;
    const int r0 = r - h < 0 ? 0 : r - h, r1 = r + h >= a.g.H ? a.g.H - 1 : r + h, c0 = c - h < 0 ? 0 : c - h, c1 = c + h >= W ? W - 1 : c + h;
    bool any = false;
    for (int i = r0; !any && i <= r1; i++)
        for (int j = c0; !any && j <= c1; j++) any = a.map_b[i * W + j] != 0;
    a.map_a[r * W + c] = any ? 1 : 0;
    a.parent[r * W + c] = ~(uint32_t)(r * W + c);
}

// step 4: one union per set forward neighbour (right, below-left, below, below-right); dbscan_union's loops carry their own bounds
__global__ __launch_bounds__(kBlock) void trav_union_kernel(TravArgs a)
{
    int r, c;
    if (!road_pixel(a.g, r, c)) return;
    const int W = a.g.W, p = r * W + c;
    if (!a.map_a[p]) return;
    if (c + 1 < W && a.map_a[p + 1]) dbscan_union(a.parent, (uint32_t)p, (uint32_t)(p + 1), a.g.npix);
    if (r + 1 < a.g.H)
        for (int dc = -1; dc <= 1; dc++)
            if (c + dc >= 0 && c + dc < W && a.map_a[p + W + dc]) dbscan_union(a.parent, (uint32_t)p, (uint32_t)(p + W + dc), a.g.npix);
}

// steps 4 and 5: keep the pixels whose root is the agent's (the union pass is over: the forest only gets read)
__global__ __launch_bounds__(kBlock) void trav_keep_kernel(TravArgs a)
{
    int r, c;
    if (!road_pixel(a.g, r, c)) return;
    const int p = r * a.g.W + c;
    const bool agent_set = a.map_a[a.agent] != 0;
    if (p == 0 && !agent_set) atomicOr(a.status, 1u);
    bool keep = false;
    if (agent_set && a.map_a[p])
        keep = dbscan_find(a.parent, (uint32_t)p, a.g.npix, false) == dbscan_find(a.parent, (uint32_t)a.agent, a.g.npix, false);
    a.out[p] = keep ? 1 : 0;
}

hipError_t launch_traversable_map(const TravArgs& a, hipStream_t st)
{
    const dim3 grid((a.g.npix + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(trav_erode_kernel, grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(trav_open_kernel, grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(trav_dilate_kernel, grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(trav_union_kernel, grid, dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(trav_keep_kernel, grid, dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

// clearance, pass 1: a thread owns a column and sweeps it down (the nearest obstacle row at or above, -1: the frame) and up (at or below, H: the
// frame); the nearer of the two stays, the one above on a tie.  An obstacle pixel names itself.
__global__ __launch_bounds__(kBlock) void clearance_columns_kernel(RoadGrid g, const uint8_t* __restrict__ trav, int32_t* __restrict__ near_row)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= g.W) return;
    int last = -1;
    for (int r = 0; r < g.H; r++) {
        if (!trav[r * g.W + c]) last = r;
        near_row[r * g.W + c] = last;
    }
    last = g.H;
    for (int r = g.H - 1; r >= 0; r--) {
        if (!trav[r * g.W + c]) last = r;
        const int above = near_row[r * g.W + c];
        near_row[r * g.W + c] = r - above <= last - r ? above : last;
    }
}

// clearance, pass 2: a workgroup owns a row; the per-column picks of the row (and of the frame's columns -1 and W, which hold an obstacle in the
// row itself) sit in LDS and a thread scans outwards from its column until the column offset alone exceeds the best distance: at most W + 2 steps
__global__ __launch_bounds__(kBlock) void clearance_rows_kernel(RoadGrid g, const int32_t* __restrict__ near_row, int32_t* __restrict__ dist2,
                                                                int16_t* __restrict__ feature)
{
    __shared__ int32_t s_row[kRoadMaxSide + 2];
    const int r = blockIdx.x, W = g.W;
    for (int i = threadIdx.x; i < W + 2; i += kBlock) s_row[i] = i == 0 || i == W + 1 ? r : near_row[r * W + i - 1];
    __syncthreads();
    for (int c = threadIdx.x; c < W; c += kBlock) {
        int best = 0x7fffffff, br = 0, bc = 0;
        for (int k = 0; k <= W + 1; k++) {
            if (k * k > best) break;
            for (int side = 0; side < (k ? 2 : 1); side++) {
                const int cc = side ? c + k : c - k;
                if (cc < -1 || cc > W) continue;
                const int fr = s_row[cc + 1], d = k * k + (r - fr) * (r - fr);
                if (d < best || (d == best && (fr < br || (fr == br && cc < bc)))) { best = d; br = fr; bc = cc; }
            }
        }
        dist2[r * W + c] = best;
        feature[2 * (r * W + c)] = (int16_t)br;
        feature[2 * (r * W + c) + 1] = (int16_t)bc;
    }
}

hipError_t launch_clearance_field(const RoadGrid& g, const uint8_t* trav, int32_t* near_row, int32_t* dist2, int16_t* feature, hipStream_t st)
{
    hipLaunchKernelGGL(clearance_columns_kernel, dim3((g.W + kBlock - 1) / kBlock), dim3(kBlock), 0, st, g, trav, near_row);
    hipLaunchKernelGGL(clearance_rows_kernel, dim3(g.H), dim3(kBlock), 0, st, g, near_row, dist2, feature);
    return hipGetLastError();
}

// the integer medial axis, as a gather: a pixel looks at its four neighbours and decides about itself alone
__global__ __launch_bounds__(kBlock) void voronoi_roadmap_kernel(RoadGrid g, const uint8_t* __restrict__ trav, const int32_t* __restrict__ dist2,
                                                                 const int16_t* __restrict__ feature, int min_dist2, int gamma2, uint8_t* __restrict__ out)
{
    int r, c;
    if (!road_pixel(g, r, c)) return;
    const int p = r * g.W + c;
    bool marked = false;
    if (trav[p] && dist2[p] >= min_dist2) {
        const int fr = feature[2 * p], fc = feature[2 * p + 1];
        const int dr[4] = {-1, 0, 0, 1}, dc[4] = {0, -1, 1, 0};
        for (int k = 0; k < 4; k++) {
            const int qr = r + dr[k], qc = c + dc[k];
            if (qr < 0 || qr >= g.H || qc < 0 || qc >= g.W || !trav[qr * g.W + qc]) continue;
            const int q = qr * g.W + qc, gr = feature[2 * q], gc = feature[2 * q + 1];
            if ((fr - gr) * (fr - gr) + (fc - gc) * (fc - gc) <= gamma2) continue;
            const int sr = r + qr, sc = c + qc;
            const int ap = (sr - 2 * fr) * (sr - 2 * fr) + (sc - 2 * fc) * (sc - 2 * fc), aq = (sr - 2 * gr) * (sr - 2 * gr) + (sc - 2 * gc) * (sc - 2 * gc);
            marked = marked || aq <= ap;
        }
    }
    out[p] = marked ? 1 : 0;
}

hipError_t launch_voronoi_roadmap(const RoadGrid& g, const uint8_t* trav, const int32_t* dist2, const int16_t* feature, int min_dist2, int gamma2,
                                  uint8_t* out, hipStream_t st)
{
    hipLaunchKernelGGL(voronoi_roadmap_kernel, dim3((g.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st, g, trav, dist2, feature, min_dist2, gamma2, out);
    return hipGetLastError();
}

constexpr int32_t kGeoInf = 0x7fffffff;
constexpr int kGeoSide = kGeoTile + 2, kGeoCells = kGeoSide * kGeoSide;

// field = unreachable everywhere but the seed; words[1] = the number of mask pixels, words[2] = 1 when the seed is in the image and in the mask
// (status bit 1 otherwise).  The seed comes from the arguments, or from a device pair (r, c) when d_seed_rc is given.
__global__ __launch_bounds__(kBlock) void geodesic_init_kernel(RoadGrid g, const uint8_t* __restrict__ mask, int seed_r, int seed_c,
                                                               const int32_t* __restrict__ d_seed_rc, int32_t* __restrict__ field,
                                                               uint32_t* __restrict__ words, uint32_t* __restrict__ status)
{
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (d_seed_rc) { seed_r = d_seed_rc[0]; seed_c = d_seed_rc[1]; }
    const bool seed_in = seed_r >= 0 && seed_r < g.H && seed_c >= 0 && seed_c < g.W && mask[seed_r * g.W + seed_c] != 0;
    const bool m = p < g.npix && mask[p] != 0;
    if (p < g.npix) field[p] = seed_in && p == seed_r * g.W + seed_c ? 0 : kGeoInf;
    const uint64_t bits = __ballot(m);
    if ((threadIdx.x & 63) == 0 && bits) atomicAdd(&words[1], (uint32_t)__popcll(bits));
    if (p == 0) {
        if (seed_in) words[2] = 1u;
        else atomicOr(status, 2u);
    }
}

// One round: a workgroup loads its 32 x 32 tile and a one-pixel halo from src, relaxes the tile to local convergence in LDS -- Jacobi sweeps
// between barriers, so that the round is a function of src alone; a sweep that changes nothing ends the loop, and a sweep that changes
// something fixes the final value of one more pixel of the tile, hence the written bound of kGeoTile^2 sweeps -- and writes the tile to dst.
// It waits for no other workgroup: what the neighbours find this round arrives through src in the next one.
__global__ __launch_bounds__(kBlock) void geodesic_round_kernel(RoadGrid g, const uint8_t* __restrict__ mask, const int32_t* __restrict__ src,
                                                                int32_t* __restrict__ dst, uint32_t* __restrict__ changed)
{
    __shared__ int32_t s_f[kGeoCells];
    __shared__ uint8_t s_m[kGeoCells];
    const int t = threadIdx.x, r0 = blockIdx.y * kGeoTile - 1, c0 = blockIdx.x * kGeoTile - 1;
    bool finite = false;
    for (int i = t; i < kGeoCells; i += kBlock) {
        const int ly = i / kGeoSide, r = r0 + ly, c = c0 + i - ly * kGeoSide;
        const bool in = r >= 0 && r < g.H && c >= 0 && c < g.W && mask[r * g.W + c] != 0;
        const int32_t v = in ? src[r * g.W + c] : kGeoInf;
        s_f[i] = v; s_m[i] = in ? 1 : 0;
        finite = finite || v != kGeoInf;
    }
    const int lx = (t & (kGeoTile - 1)) + 1, ly0 = (t / kGeoTile) * 4 + 1;       // four pixels of one column per thread
    bool ever = false;
    if (__syncthreads_or(finite)) {
        for (int sweep = 0; sweep < kGeoTile * kGeoTile; sweep++) {
            int32_t nv[4];
            bool ch = false;
            for (int k = 0; k < 4; k++) {
                const int i = (ly0 + k) * kGeoSide + lx;
                int32_t v = s_f[i];
                if (s_m[i])
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++) {
                            const int32_t n = s_f[i + dy * kGeoSide + dx];
                            const int32_t cand = n == kGeoInf ? kGeoInf : n + (dx && dy ? 17 : 12);   // (the centre never wins: n + 12 > n)
                            v = cand < v ? cand : v;
                        }
                nv[k] = v;
                ch = ch || v != s_f[i];
            }
            __syncthreads();
            for (int k = 0; k < 4; k++) s_f[(ly0 + k) * kGeoSide + lx] = nv[k];
            ever = ever || ch;
            if (!__syncthreads_or(ch)) break;
        }
    }
    for (int k = 0; k < 4; k++) {
        const int r = r0 + ly0 + k, c = c0 + lx;
        if (r < g.H && c < g.W) dst[r * g.W + c] = s_f[(ly0 + k) * kGeoSide + lx];
    }
    if (__any(ever) && (t & 63) == 0) atomicOr(changed, 1u);
}

hipError_t launch_geodesic_init(const RoadGrid& g, const uint8_t* mask, int seed_r, int seed_c, const int32_t* d_seed_rc, int32_t* field,
                                uint32_t* words, uint32_t* status, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(words, 0, 4 * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(geodesic_init_kernel, dim3((g.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st, g, mask, seed_r, seed_c, d_seed_rc, field, words, status);
    return hipGetLastError();
}

hipError_t launch_geodesic_round(const RoadGrid& g, const uint8_t* mask, const int32_t* src, int32_t* dst, uint32_t* changed, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(geodesic_round_kernel, dim3((g.W + kGeoTile - 1) / kGeoTile, (g.H + kGeoTile - 1) / kGeoTile), dim3(kBlock), 0, st, g, mask, src, dst, changed);
    return hipGetLastError();
}

// the roadmap pixel with the smallest finite field value, the smallest index on a tie, as the minimum of the keys (field << 32 | index):
// workgroup b of the first launch sweeps pixels [b kEntryChunk, (b + 1) kEntryChunk) and leaves its minimum in partial[b]; one workgroup of
// the second launch takes the minimum of those.  entry = (r, c, field, index), or (-1, -1, unreachable, -1).
constexpr int kEntryChunk = 16 * kBlock;
constexpr unsigned long long kEntryNone = ~0ull;

__device__ __forceinline__ unsigned long long entry_block_min(unsigned long long key)
{
    __shared__ unsigned long long s_key[kBlock / kWave];
    for (int m = 1; m < kWave; m <<= 1) { const unsigned long long o = __shfl_xor(key, m); key = o < key ? o : key; }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    for (int w = 0; w < kBlock / kWave; w++) key = s_key[w] < key ? s_key[w] : key;
    return key;
}

__global__ __launch_bounds__(kBlock) void roadmap_entry_partial_kernel(RoadGrid g, const uint8_t* __restrict__ roadmap, const int32_t* __restrict__ field,
                                                                       unsigned long long* __restrict__ partial)
{
    unsigned long long key = kEntryNone;
    const int p0 = blockIdx.x * kEntryChunk, p1 = p0 + kEntryChunk < g.npix ? p0 + kEntryChunk : g.npix;
    for (int p = p0 + threadIdx.x; p < p1; p += kBlock)
        if (roadmap[p] && field[p] != kGeoInf) {
            const unsigned long long k = ((unsigned long long)(uint32_t)field[p] << 32) | (uint32_t)p;
            key = k < key ? k : key;
        }
    key = entry_block_min(key);
    if (threadIdx.x == 0) partial[blockIdx.x] = key;
}

__global__ __launch_bounds__(kBlock) void roadmap_entry_final_kernel(RoadGrid g, const unsigned long long* __restrict__ partial, int nb,
                                                                     int32_t* __restrict__ entry)
{
    unsigned long long key = kEntryNone;
    for (int b = threadIdx.x; b < nb; b += kBlock) key = partial[b] < key ? partial[b] : key;
    key = entry_block_min(key);
    if (threadIdx.x == 0) {
        const int p = key == kEntryNone ? -1 : (int)(uint32_t)key;
        entry[0] = p < 0 ? -1 : p / g.W; entry[1] = p < 0 ? -1 : p % g.W;
        entry[2] = p < 0 ? kGeoInf : (int32_t)(key >> 32); entry[3] = p;
    }
}

hipError_t launch_roadmap_entry(const RoadGrid& g, const uint8_t* roadmap, const int32_t* field, void* scratch, int32_t* entry, hipStream_t st)
{
    const int nb = (g.npix + kEntryChunk - 1) / kEntryChunk;             // at most 4096: 32 KiB of the scratch
    unsigned long long* partial = (unsigned long long*)scratch;
    hipLaunchKernelGGL(roadmap_entry_partial_kernel, dim3(nb), dim3(kBlock), 0, st, g, roadmap, field, partial);
    hipLaunchKernelGGL(roadmap_entry_final_kernel, dim3(1), dim3(kBlock), 0, st, g, partial, nb, entry);
    return hipGetLastError();
}

// nodes, count: a wavefront owns a cell; its lanes stride over the cell's pixels in row-major order and keep the largest key
// (dist2 << 32 | ~index) among the roadmap pixels with a finite field: the largest clearance, the smallest index on a tie; pick = index or -1
__global__ __launch_bounds__(kBlock) void nodes_pick_kernel(NodeArgs a)
{
    const int cell = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (cell >= a.cells_y * a.cells_x) return;                          // (whole wavefronts: the shuffles below see every lane)
    const int cy = cell / a.cells_x, cx = cell - cy * a.cells_x, W = a.g.W, r0 = cy * a.cell, c0 = cx * a.cell;
    const int h = r0 + a.cell < a.g.H ? a.cell : a.g.H - r0, w = c0 + a.cell < W ? a.cell : W - c0;
    unsigned long long key = 0ull;                                      // (no pixel has index 2^32 - 1: 0 is "none")
    for (int i = lane; i < h * w; i += kWave) {
        const int p = (r0 + i / w) * W + c0 + i % w;
        if (a.roadmap[p] && a.field[p] != kGeoInf) {
            const unsigned long long k = ((unsigned long long)(uint32_t)a.dist2[p] << 32) | (uint32_t)~(uint32_t)p;
            key = k > key ? k : key;
        }
    }
    for (int m = 1; m < kWave; m <<= 1) { const unsigned long long o = __shfl_xor(key, m); key = o > key ? o : key; }
    if (lane == 0) a.pick[cell] = key ? (int32_t)~(uint32_t)key : -1;
}

// nodes, scan and emit: one workgroup; a thread counts the picks of its run of cells, thread 0 scans the 256 counts, and every thread writes
// its run's nodes behind its offset: row-major cell order, no atomics.  The count stays on the device.
__global__ __launch_bounds__(kBlock) void nodes_emit_kernel(NodeArgs a)
{
    __shared__ int32_t s_sum[kBlock];
    const int t = threadIdx.x, n = a.cells_y * a.cells_x, per = (n + kBlock - 1) / kBlock;
    const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    int32_t s = 0;
    for (int i = i0; i < i1; i++) s += a.pick[i] >= 0;
    s_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int i = 0; i < kBlock; i++) { const int32_t v = s_sum[i]; s_sum[i] = run; run += v; }
        a.count[0] = run;
    }
    __syncthreads();
    int32_t k = s_sum[t];
    for (int i = i0; i < i1; i++) {
        const int p = a.pick[i];
        if (p < 0) continue;
        a.node_rc[2 * k] = p / a.g.W; a.node_rc[2 * k + 1] = p % a.g.W;
        a.node_dist2[k] = a.dist2[p]; a.node_field[k] = a.field[p];
        k++;
    }
}

hipError_t launch_roadmap_nodes(const NodeArgs& a, hipStream_t st)
{
    const int n = a.cells_y * a.cells_x;
    hipLaunchKernelGGL(nodes_pick_kernel, dim3((n + kBlock / kWave - 1) / (kBlock / kWave)), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(nodes_emit_kernel, dim3(1), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

// the walk down a field: one wavefront; lanes 0..7 test one neighbour each, in the stated order, and the lowest lane that qualifies is the
// step.  `capacity` bounds the loop.  count2 = (pixels written, 0 done | 1 target outside the mask or unreachable | 2 capacity reached |
// 3 no neighbour qualifies: not a field of this mask)
__global__ __launch_bounds__(kWave) void trace_path_kernel(RoadGrid g, const uint8_t* __restrict__ mask, const int32_t* __restrict__ field, int r, int c,
                                                           const int32_t* __restrict__ d_target_rc, int capacity, int32_t* __restrict__ path_rc,
                                                           int32_t* __restrict__ count2)
{
    const int lane = threadIdx.x, k = lane < 4 ? lane : lane + 1;                 // 3 x 3 window without its centre
    const int dr = k / 3 - 1, dc = k % 3 - 1, w = dr && dc ? 17 : 12;
    if (d_target_rc) { r = d_target_rc[0]; c = d_target_rc[1]; }
    int count = 0, status = 2;
    if (r < 0 || r >= g.H || c < 0 || c >= g.W || !mask[r * g.W + c] || field[r * g.W + c] == kGeoInf) status = 1;
    else
        for (int step = 0; step < capacity; step++) {
            if (lane == 0) { path_rc[2 * count] = r; path_rc[2 * count + 1] = c; }
            count++;
            const int32_t f = field[r * g.W + c];
            if (f == 0) { status = 0; break; }
            const int nr = r + dr, nc = c + dc;
            bool ok = lane < 8 && nr >= 0 && nr < g.H && nc >= 0 && nc < g.W && mask[nr * g.W + nc] != 0;
            if (ok) { const int32_t fn = field[nr * g.W + nc]; ok = fn != kGeoInf && fn + w == f; }
            const uint64_t hits = __ballot(ok);
            if (!hits) { status = 3; break; }
            const int j = __ffsll((unsigned long long)hits) - 1, kk = j < 4 ? j : j + 1;
            r += kk / 3 - 1; c += kk % 3 - 1;
        }
    if (lane == 0) { count2[0] = count; count2[1] = status; }
}

hipError_t launch_trace_path(const RoadGrid& g, const uint8_t* mask, const int32_t* field, int target_r, int target_c, const int32_t* d_target_rc,
                             int capacity, int32_t* path_rc, int32_t* count2, hipStream_t st)
{
    hipLaunchKernelGGL(trace_path_kernel, dim3(1), dim3(kWave), 0, st, g, mask, field, target_r, target_c, d_target_rc, capacity, path_rc, count2);
    return hipGetLastError();
}

// ---- roadmap subregions: all-pairs node distances, segment clearance, average-linkage clustering -------------------------------------------------
// (src/planner/planner.py:473-574 on the grid roadmap; the rules: include/gsplat_hip.h, gs_node_distances .. gs_subregions)

// The skeleton (the mask's pixels) as a list, in row-major order: count, scan, emit, no atomics.  A thread owns 16 consecutive pixels of its
// workgroup's kSkelChunk; thread 0 scans the 256 counts.  emit = false: block_counts[b] = the chunk's count; emit = true: block_counts[b] is
// the chunk's offset, index[p] = the entry of pixel p or -1, pixel[entry] = p.
__global__ __launch_bounds__(kBlock) void skeleton_list_kernel(NodeDistArgs a, bool emit)
{
    __shared__ int32_t s_sum[kBlock];
    constexpr int per = kSkelChunk / kBlock;
    const int t = threadIdx.x, p0 = blockIdx.x * kSkelChunk + t * per, p1 = p0 + per < a.g.npix ? p0 + per : a.g.npix;
    int32_t s = 0;
    for (int p = p0; p < p1; p++) s += a.mask[p] != 0;
    s_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int i = 0; i < kBlock; i++) { const int32_t v = s_sum[i]; s_sum[i] = run; run += v; }
        if (!emit) a.block_counts[blockIdx.x] = (uint32_t)run;
    }
    if (!emit) return;
    __syncthreads();
    int32_t e = (int32_t)a.block_counts[blockIdx.x] + s_sum[t];
    for (int p = p0; p < p1; p++) {
        const bool m = a.mask[p] != 0;
        a.index[p] = m ? e : -1;
        if (!m) continue;
        const int r = p / a.g.W, c = p - r * a.g.W;
        uint32_t nb = 0;                                               // bit k: neighbour k of the 3 x 3 window (row-major, 4 = the centre) is in the mask
        for (int k = 0; k < 9; k++) {
            const int nr = r + k / 3 - 1, nc = c + k % 3 - 1;
            if (k != 4 && nr >= 0 && nr < a.g.H && nc >= 0 && nc < a.g.W && a.mask[nr * a.g.W + nc]) nb |= 1u << k;
        }
        a.pixel[e++] = (int32_t)((uint32_t)p | (nb & 15u) << 24 | (nb >> 5) << 28);       // (p < 2^24: the top byte holds the eight bits)
    }
}

// exclusive scan of the chunk counts in place (at most 4096 of them: a run per thread, thread 0 scans the 256 run sums); words[0] = the total
__global__ __launch_bounds__(kBlock) void skeleton_scan_kernel(NodeDistArgs a, int nb)
{
    __shared__ uint32_t s_sum[kBlock];
    const int t = threadIdx.x, per = (nb + kBlock - 1) / kBlock;
    const int i0 = t * per < nb ? t * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
    uint32_t s = 0;
    for (int i = i0; i < i1; i++) s += a.block_counts[i];
    s_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < kBlock; i++) { const uint32_t v = s_sum[i]; s_sum[i] = run; run += v; }
        a.words[0] = run;
    }
    __syncthreads();
    uint32_t run = s_sum[t];
    for (int i = i0; i < i1; i++) { const uint32_t v = a.block_counts[i]; a.block_counts[i] = run; run += v; }
}

__device__ __forceinline__ int32_t node_entry(const NodeDistArgs& a, int k)
{
    const int r = a.node_rc[2 * k], c = a.node_rc[2 * k + 1];
    return r >= 0 && r < a.g.H && c >= 0 && c < a.g.W ? a.index[r * a.g.W + c] : -1;
}

// One seed node: d (M entries, LDS or global, this workgroup's alone) = unreachable but 0 at the seed, then relaxed IN PLACE until a sweep
// changes nothing.  A thread writes only the entries it owns (t, t + 256, ..) and reads its neighbours' as they are, old or new: every value
// is the length of a real path, values only fall, and the sweep that changes nothing has read only final values, so the fixed point -- the
// shortest distances -- is reached whatever the schedule.  A sweep that changes something makes final the unfinished entry nearest the seed
// (its predecessor was final before the sweep): at most M changing sweeps.  Row `seed` of D = d at the nodes' entries.
__device__ __forceinline__ void node_dist_seed(const NodeDistArgs& a, int M, int seed, int32_t* d)
{
    const int t = threadIdx.x, W = a.g.W;
    const int32_t se = node_entry(a, seed);
    for (int e = t; e < M; e += kBlock) d[e] = e == se ? 0 : kGeoInf;
    __syncthreads();
    if (se >= 0)
        for (int sweep = 0; sweep <= M; sweep++) {
            bool ch = false;
            for (int e = t; e < M; e += kBlock) {
                const uint32_t word = (uint32_t)a.pixel[e];
                const int p = (int)(word & 0xffffffu);
                const int32_t v = d[e];
                int32_t best = v;
                for (uint32_t nb = word >> 24; nb; nb &= nb - 1) {      // the neighbours in the mask alone (two or three on a skeleton): in the image, listed
                    const int bit = __ffs(nb) - 1, k = bit < 4 ? bit : bit + 1, dr = k / 3 - 1, dc = k % 3 - 1;
                    const int32_t n = d[a.index[p + dr * W + dc]];
                    const int32_t cand = n == kGeoInf ? kGeoInf : n + (dr && dc ? 17 : 12);
                    best = cand < best ? cand : best;
                }
                if (best < v) { d[e] = best; ch = true; }
            }
            if (!__syncthreads_or(ch)) break;
        }
    for (int j = t; j < a.K; j += kBlock) {
        const int32_t e = node_entry(a, j);
        a.D[(int64_t)seed * a.K + j] = se >= 0 && e >= 0 ? d[e] : kGeoInf;
    }
    __syncthreads();                                                   // (the next seed of this workgroup starts on the same array)
}

// A workgroup per seed while the skeleton's distances fit the LDS; else the first G workgroups take the seeds G apart, each on its own M
// entries of the global array (G = as many arrays as fit dist_cap, at least one: dist_cap >= npix >= M), and the others leave.
__global__ __launch_bounds__(kBlock) void node_dist_kernel(NodeDistArgs a)
{
    __shared__ int32_t s_d[kNodeLdsCap];
    const int M = (int)a.words[0];
    if (M == 0 || (a.path != 2 && M <= kNodeLdsCap)) { node_dist_seed(a, M, blockIdx.x, s_d); return; }
    const int64_t fit = a.dist_cap / M;
    const int G = fit < (int64_t)gridDim.x ? (int)fit : (int)gridDim.x;
    if ((int)blockIdx.x >= G) return;
    for (int seed = blockIdx.x; seed < a.K; seed += G) node_dist_seed(a, M, seed, a.dist + (int64_t)blockIdx.x * M);
}

uint64_t node_distances_scratch_bytes(const RoadGrid& g)
{
    const uint64_t n = (uint64_t)g.npix, nb = (n + kSkelChunk - 1) / kSkelChunk;
    return 4 * ((4 * n + 255) / 256 * 256) + (4 * nb + 255) / 256 * 256 + 256;          // index, pixel, two maps of distances; chunk counts; words
}

void node_distances_carve(void* scratch, NodeDistArgs& a)
{
    const uint64_t map = (4 * (uint64_t)a.g.npix + 255) / 256 * 256, nb = ((uint64_t)a.g.npix + kSkelChunk - 1) / kSkelChunk;
    uint8_t* p = (uint8_t*)scratch;
    a.index = (int32_t*)p; p += map;
    a.pixel = (int32_t*)p; p += map;
    a.dist = (int32_t*)p; p += 2 * map;
    a.dist_cap = (int64_t)(2 * map / 4);
    a.block_counts = (uint32_t*)p; p += (4 * nb + 255) / 256 * 256;
    a.words = (uint32_t*)p;
}

hipError_t launch_node_distances(const NodeDistArgs& a, hipStream_t st)
{
    if (a.K == 0) return hipSuccess;
    const int nb = (a.g.npix + kSkelChunk - 1) / kSkelChunk;
    hipLaunchKernelGGL(skeleton_list_kernel, dim3(nb), dim3(kBlock), 0, st, a, false);
    hipLaunchKernelGGL(skeleton_scan_kernel, dim3(1), dim3(kBlock), 0, st, a, nb);
    hipLaunchKernelGGL(skeleton_list_kernel, dim3(nb), dim3(kBlock), 0, st, a, true);
    hipLaunchKernelGGL(node_dist_kernel, dim3(a.K), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

// floor((2 a + N) / (2 N)) for N > 0 in exact integers (C's division truncates: the negative numerators go through the positive quotient)
__device__ __forceinline__ int line_round(int a, int N)
{
    const int x = 2 * a + N, y = 2 * N;
    return x >= 0 ? x / y : -((-x + y - 1) / y);
}

// a wavefront per segment: lane l takes the line's pixels l, l + 64, ..; the minimum over the lanes by shuffles.  An end point outside the
// image is a pixel outside the image (i = 0 and i = N give the end points themselves): 0 without a walk; with both inside every pixel of the
// line is inside (each coordinate stays between its ends), N <= 4095 and 2 i |dr| + N stays below 2^31.
__global__ __launch_bounds__(kBlock) void segment_clearance_kernel(RoadGrid g, const int32_t* __restrict__ dist2, int n, const int32_t* __restrict__ seg,
                                                                   int32_t* __restrict__ out)
{
    const int s = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n) return;                                                 // (whole wavefronts)
    const int r0 = seg[4 * s], c0 = seg[4 * s + 1], r1 = seg[4 * s + 2], c1 = seg[4 * s + 3];
    int32_t best = 0;
    if (r0 >= 0 && r0 < g.H && c0 >= 0 && c0 < g.W && r1 >= 0 && r1 < g.H && c1 >= 0 && c1 < g.W) {
        const int dr = r1 - r0, dc = c1 - c0, ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc, N = ar > ac ? ar : ac;
        best = kGeoInf;
        for (int i = lane; i <= N; i += kWave) {
            const int r = N ? r0 + line_round(i * dr, N) : r0, c = N ? c0 + line_round(i * dc, N) : c0;
            const int32_t v = r >= 0 && r < g.H && c >= 0 && c < g.W ? dist2[r * g.W + c] : 0;
            best = v < best ? v : best;
        }
    }
    for (int m = 1; m < kWave; m <<= 1) { const int32_t o = __shfl_xor(best, m); best = o < best ? o : best; }
    if (lane == 0) out[s] = best;
}

hipError_t launch_segment_clearance(const RoadGrid& g, const int32_t* dist2, int n, const int32_t* segments, int32_t* clearance, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(segment_clearance_kernel, dim3((n + kBlock / kWave - 1) / (kBlock / kWave)), dim3(kBlock), 0, st, g, dist2, n, segments, clearance);
    return hipGetLastError();
}

// C of the pair (i, j) from D above the diagonal, +inf where D says unreachable (filled in by the clustering launch): two products and one
// sum, none fused
__device__ __forceinline__ double subregion_pair(const SubregionArgs& a, int i, int j)
{
#pragma clang fp contract(off)
    if (i == j) return 0.0;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int32_t d = a.D[(int64_t)lo * a.K + hi];
    if (d == kGeoInf) return INFINITY;
    const int64_t dr = (int64_t)a.node_rc[2 * lo] - a.node_rc[2 * hi], dc = (int64_t)a.node_rc[2 * lo + 1] - a.node_rc[2 * hi + 1];
    const double path = a.path_weight * ((double)d / 12.0), coord = a.coord_weight * sqrt((double)(dr * dr + dc * dc));
    return path + coord;
}

// sums = C, and per workgroup the largest finite C of its 256 pairs (a maximum does not depend on the order; no atomics)
__global__ __launch_bounds__(kBlock) void subregion_matrix_kernel(SubregionArgs a)
{
    __shared__ double s_max[kBlock / kWave];
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = (int64_t)a.K * a.K;
    double v = 0.0;
    if (q < n) {
        const double c = subregion_pair(a, (int)(q / a.K), (int)(q % a.K));
        a.sums[q] = c;
        v = c == INFINITY ? 0.0 : c;
    }
    for (int m = 1; m < kWave; m <<= 1) { const double o = __shfl_xor(v, m); v = o > v ? o : v; }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; w++) v = s_max[w] > v ? s_max[w] : v;
        a.partial[blockIdx.x] = v;
    }
}

// the smallest (value, index) of the workgroup, the smaller index on equal values, to every thread; (+inf, -1) when no thread has a candidate
struct SubMin { double v; int i; };
__device__ __forceinline__ SubMin subregion_block_min(double v, int i)
{
    __shared__ double s_v[kBlock / kWave];
    __shared__ int s_i[kBlock / kWave];
    for (int m = 1; m < kWave; m <<= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (oi >= 0 && (i < 0 || ov < v || (ov == v && oi < i))) { v = ov; i = oi; }
    }
    __syncthreads();                                                   // (the previous call's readers are done)
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = v; s_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    SubMin r = {INFINITY, -1};
    for (int w = 0; w < kBlock / kWave; w++)
        if (s_i[w] >= 0 && (r.i < 0 || s_v[w] < r.v || (s_v[w] == r.v && s_i[w] < r.i))) { r.v = s_v[w]; r.i = s_i[w]; }
    return r;
}

// Average linkage by one workgroup.  A cluster is named by its smallest member; sums[x][y] = the sum of C over the member pairs of clusters
// x and y, the average = sums / (|x| |y|).  near[x] = the cluster y > x with the smallest average (the smallest y on equal averages) and
// near_v[x] that average: the pair to merge is the smallest (near_v[a], a) -- the lexicographically smallest (a, b) among the closest pairs.
// After a merge of a < b: row and column a of sums take the sums with b added; a cluster that pointed at a or b, and a itself, look again
// (the whole workgroup scans one row); a cluster x < a that pointed elsewhere compares its new average with a (it cannot have fallen below
// near_v[x] -- the linkage is reducible -- but it can tie with a smaller name).
__global__ __launch_bounds__(kBlock) void subregion_cluster_kernel(SubregionArgs a, int nparts)
{
    __shared__ double s_near_v[kMaxNodes];
    __shared__ int32_t s_near[kMaxNodes], s_size[kMaxNodes];
    __shared__ uint8_t s_live[kMaxNodes], s_again[kMaxNodes];
    __shared__ int32_t s_rank[kMaxNodes];
    const int t = threadIdx.x, K = a.K;
    // the largest finite C; unreachable pairs take it plus one
    double mx = 0.0;
    for (int i = t; i < nparts; i += kBlock) mx = a.partial[i] > mx ? a.partial[i] : mx;
    mx = -subregion_block_min(-mx, 0).v;
    const double fill = mx + 1.0;
    for (int64_t q = t; q < (int64_t)K * K; q += kBlock)
        if (a.sums[q] == INFINITY) a.sums[q] = fill;
    for (int x = t; x < K; x += kBlock) { s_size[x] = 1; s_live[x] = 1; a.member[x] = x; }
    __syncthreads();
    auto look = [&](int x) {                                           // near[x], by the whole workgroup
        double bv = INFINITY; int bi = -1;
        for (int y = x + 1 + t; y < K; y += kBlock)
            if (s_live[y]) {
                const double v = a.sums[(int64_t)x * K + y] / (double)(s_size[x] * s_size[y]);
                if (bi < 0 || v < bv) { bv = v; bi = y; }             // (ascending y: the first of equal averages stays)
            }
        const SubMin r = subregion_block_min(bv, bi);
        if (t == 0) { s_near[x] = r.i; s_near_v[x] = r.v; }
    };
    for (int x = 0; x < K; x++) look(x);
    __syncthreads();
    int step = 0;
    for (; step < K - 1; step++) {
        double bv = INFINITY; int bi = -1;
        for (int x = t; x < K; x += kBlock)
            if (s_live[x] && s_near[x] >= 0 && (bi < 0 || s_near_v[x] < bv)) { bv = s_near_v[x]; bi = x; }
        const SubMin pick = subregion_block_min(bv, bi);
        if (pick.i < 0 || pick.v > a.threshold) break;
        const int ca = pick.i, cb = s_near[ca];
        __syncthreads();                                               // (everyone has read near[ca] before thread 0 writes near again)
        if (t == 0) a.heights[step] = pick.v;
        for (int x = t; x < K; x += kBlock) {
            if (a.member[x] == cb) a.member[x] = ca;
            bool again = false;
            if (s_live[x] && x != cb) {
                if (x != ca) {
                    const double s = a.sums[(int64_t)ca * K + x] + a.sums[(int64_t)cb * K + x];
                    a.sums[(int64_t)ca * K + x] = s; a.sums[(int64_t)x * K + ca] = s;
                }
                again = x == ca || s_near[x] == ca || s_near[x] == cb;
            }
            s_again[x] = again ? 1 : 0;
        }
        __syncthreads();
        if (t == 0) { s_size[ca] += s_size[cb]; s_live[cb] = 0; }
        __syncthreads();
        for (int x = t; x < ca; x += kBlock)
            if (s_live[x] && !s_again[x]) {
                const double v = a.sums[(int64_t)x * K + ca] / (double)(s_size[x] * s_size[ca]);
                if (v < s_near_v[x] || (v == s_near_v[x] && ca < s_near[x])) { s_near_v[x] = v; s_near[x] = ca; }
            }
        for (int x = 0; x < cb; x++)                                   // (uniform: s_again is read by every thread alike)
            if (s_again[x]) look(x);
        __syncthreads();
    }
    for (int k = step + t; k < K - 1; k += kBlock) a.heights[k] = INFINITY;
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int x = 0; x < K; x++) { s_rank[x] = run; run += s_live[x]; }
        a.count[0] = run;
    }
    __syncthreads();
    for (int x = t; x < K; x += kBlock) a.labels[x] = s_rank[a.member[x]];
}

uint64_t subregions_scratch_bytes(int K)
{
    const uint64_t n = (uint64_t)K * K;
    return (8 * n + 255) / 256 * 256 + (8 * ((n + kBlock - 1) / kBlock) + 255) / 256 * 256 + (4 * (uint64_t)K + 255) / 256 * 256 + 256;
}

void subregions_carve(void* scratch, SubregionArgs& a)
{
    const uint64_t n = (uint64_t)a.K * a.K;
    uint8_t* p = (uint8_t*)scratch;
    a.sums = (double*)p; p += (8 * n + 255) / 256 * 256;
    a.partial = (double*)p; p += (8 * ((n + kBlock - 1) / kBlock) + 255) / 256 * 256;
    a.member = (int32_t*)p;
}

hipError_t launch_subregions(const SubregionArgs& a, hipStream_t st)
{
    if (a.K == 0) return hipMemsetAsync(a.count, 0, sizeof(int32_t), st);
    const int nparts = (int)(((int64_t)a.K * a.K + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(subregion_matrix_kernel, dim3(nparts), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(subregion_cluster_kernel, dim3(1), dim3(kBlock), 0, st, a, nparts);
    return hipGetLastError();
}

}  // namespace gs
