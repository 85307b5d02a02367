// Depth-error metrics on the device (slam/utils.py:389-442 calc_depth_error, dpp.py:396-440 the same arithmetic inside
// compute_depth_error): resample the prediction at the valid ground-truth pixels, exact medians of both arrays by radix select,
// clamp, eight metrics in one fused reduction.  Per image: [abs_diff, abs_rel, sq_rel, a1, a2, a3, rmse, rmse_log, ratio, n].
//
// Launch sequence of clslam_depth_metrics (all on the caller's stream, nothing allocated, no host synchronisation):
//   memset header | prepare (resample + mask + histogram of digit 0) | select x3 (digits 1..3; skipped without median scaling) |
//   metrics (resolves the last digit -> medians -> ratio; per-block partial sums) | finalize (one block per image, double).
//
// SELECTION.  A masked value is ranked by its order key (the fp32 bit pattern with the sign bit flipped, or all bits flipped for
// a negative value: unsigned order = value order; the ground truth is positive by the mask, the prediction is not assumed to be).
// Four ranks are wanted per image: (n-1)/2 and n/2 of the ground truth and of the resampled prediction (np.median: the mean of
// the two, which are the same element for odd n).  Pass p histograms digit p (8 bits, most significant first) of the values whose
// higher digits equal the prefix found so far; the next kernel turns the finished histogram into the next digit and the rank
// inside its bin (every block does this redundantly from the same global histogram, block 0 stores the state for the kernel
// after).  The two ranks of one array share a histogram while their prefixes are equal -- they are neighbours, so that is the
// normal case; once they part, the upper rank gets its own.  Equal values end in one bin of every pass, whatever their number:
// the rank is always inside the bin the scan finds, so runs of equal values (centimetre-quantised ground truth, all-equal) need
// no special case.
//
// LDS HISTOGRAM.  kCopies = 8 copies per selection, copy = lane & 7, each padded to 257 words: the copies of one bin lie on 8
// different banks, so a wave of equal values is a 4-way same-address update at worst, not 32-way.  Before it touches LDS each
// wave checks by a butterfly whether all its active lanes hold one bin (digit 0 -- sign and exponent -- always does, and so
// does every digit of an all-equal image): then one lane adds the wave's count.  The copies are summed and merged into the
// global histogram with one integer atomic per non-empty bin and block.
//
// SUMS.  Every thread accumulates its pixels in double in pixel order, wave butterfly (wave_sum_f64), the four waves in order,
// one partial per block; the finalising block adds the partials thread-strided in index order and reduces the same way.  No
// floating-point atomics anywhere: two launches agree bitwise.
#include "common.h"

namespace clslam {

constexpr int kDeThreads = 256;
constexpr int kDePixPerBlock = 1024;
constexpr int kDeMaxBlocks = 512;
constexpr int kCopies = 8;
constexpr int kCopyStride = 257;
constexpr int kSel = 4;                    // 0 gt lower rank, 1 gt upper rank, 2 prediction lower rank, 3 prediction upper rank
constexpr int kHistWords = 4 * kSel * 256; // [pass][selection][bin]
constexpr int kStateWords = 64;            // [stage 1..4][selection]{prefix, rank} = 32 words, then n, then ratio / medians
constexpr int kHeaderWords = kHistWords + kStateWords;
constexpr int kStateN = 32, kStateRatio = 33, kStateMedGt = 34, kStateMedPred = 35;
constexpr int kSums = 8;

struct DeGeom {
    int h, w, hg, wg;
    float min_depth, max_depth;
    int has_max, from_disp, scaling;
};

__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ bool gt_valid(float g, const DeGeom& G) {      // utils.py:401-404, both strict
    return g > G.min_depth && (!G.has_max || g < G.max_depth);
}

// ---- the resampling rule, in one place: OpenCV INTER_LINEAR on a float image (cv2.resize at utils.py:397 / dpp.py:408) --------
// source coordinate of destination index d: (d + 0.5) * (src / dst) - 0.5 with the scale in double, narrowed to float; floor ->
// cell, fraction in float; outside the image the border cell with fraction 0.
__device__ __forceinline__ void linear_coord(int d, double scale, int src, int& cell, float& frac) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int c = (int)floorf(f);
    f -= (float)c;
    if (c < 0) { c = 0; f = 0.f; }
    if (c >= src - 1) { c = src - 1; f = 0.f; }
    cell = c;
    frac = f;
}
__device__ __forceinline__ float lerp_rn(float a, float b, float f) {      // (1-f)*a + f*b, each operation rounded (no contraction)
    return __fadd_rn(__fmul_rn(1.f - f, a), __fmul_rn(f, b));
}
// depth of one tap: the plane itself, or min_depth / disparity (disp_to_depth with max_depth=None, dpp.py:405-406 -- the
// reference converts first and resizes DEPTH)
__device__ __forceinline__ float tap(const float* __restrict__ p, int i, const DeGeom& G) {
    const float v = p[i];
    return G.from_disp ? G.min_depth / v : v;
}
__device__ __forceinline__ float resample_at(const float* __restrict__ pred, int y, int x, const DeGeom& G) {
    int x0, y0;
    float fx, fy;
    linear_coord(x, (double)G.w / (double)G.wg, G.w, x0, fx);
    linear_coord(y, (double)G.h / (double)G.hg, G.h, y0, fy);
    const int x1 = min(x0 + 1, G.w - 1), y1 = min(y0 + 1, G.h - 1);
    const float top = lerp_rn(tap(pred, y0 * G.w + x0, G), tap(pred, y0 * G.w + x1, G), fx);      // horizontal pass first
    const float bot = lerp_rn(tap(pred, y1 * G.w + x0, G), tap(pred, y1 * G.w + x1, G), fx);
    return lerp_rn(top, bot, fy);
}

// ---- histogram update with wave pre-aggregation -------------------------------------------------------------------------------
// bin < 0: the lane has nothing to add.  Called by all 64 lanes of the wave.
__device__ __forceinline__ void hist_add(unsigned* __restrict__ h /* one selection: [kCopies][kCopyStride] */, int bin) {
    // state of a lane group: -1 nobody active, 0..255 every active lane holds that bin, 512 mixed (small integers: exact in fp32)
    float st = bin < 0 ? -1.f : (float)bin;
    for (int off = 1; off < kWave; off <<= 1) {
        const float o = wave_shfl_xor(st, off);
        st = st < 0.f ? o : (o < 0.f || o == st) ? st : 512.f;
    }
    if (st < 0.f) return;                                                   // wave-uniform
    if (st < 256.f) {
        const float cnt = wave_sum(bin < 0 ? 0.f : 1.f);
        if (lane_id() == 0) atomicAdd(&h[(int)st], (unsigned)cnt);
    } else if (bin >= 0) {
        atomicAdd(&h[(lane_id() & (kCopies - 1)) * kCopyStride + bin], 1u);
    }
}

__device__ __forceinline__ void hist_clear(unsigned* lds) {
    for (int i = threadIdx.x; i < kSel * kCopies * kCopyStride; i += kDeThreads) lds[i] = 0u;
    __syncthreads();
}
// sum the copies, one integer atomic per non-empty bin into the global histogram of this pass
__device__ __forceinline__ void hist_merge(const unsigned* lds, unsigned* __restrict__ ghist /* [kSel][256] */) {
    __syncthreads();
    const int t = threadIdx.x;
    for (int s = 0; s < kSel; ++s) {
        unsigned c = 0;
        for (int k = 0; k < kCopies; ++k) c += lds[(s * kCopies + k) * kCopyStride + t];
        if (c) atomicAdd(&ghist[s * 256 + t], c);
    }
}

// ---- selection state ----------------------------------------------------------------------------------------------------------
struct SelState {
    unsigned prefix[kSel];   // the digits found so far (stage digits of 8 bits, right-aligned)
    unsigned rank[kSel];     // rank inside the values that carry the prefix
    unsigned n;
};

// Stage s (1..4) from the finished histogram of pass s-1 and the state of stage s-1 (stage 0: no digits, ranks (n-1)/2 and n/2).
// Every block computes the same; block x = 0 stores it for the next kernel.  scan: 2 * kSel * 256 words of LDS.
__device__ void resolve_stage(unsigned* __restrict__ hdr, int stage, unsigned* scan, SelState* out /* LDS */) {
    const int t = threadIdx.x;
    const unsigned* hist = hdr + (stage - 1) * kSel * 256;
    unsigned* state = hdr + kHistWords;
    __shared__ SelState prev;
    if (t == 0) {
        if (stage == 1) {
            for (int s = 0; s < kSel; ++s) { prev.prefix[s] = 0u; prev.rank[s] = 0u; }
            prev.n = 0u;
        } else {
            for (int s = 0; s < kSel; ++s) {
                prev.prefix[s] = state[((stage - 2) * kSel + s) * 2];
                prev.rank[s] = state[((stage - 2) * kSel + s) * 2 + 1];
            }
            prev.n = state[kStateN];
        }
    }
    __syncthreads();
    for (int s = 0; s < kSel; ++s) {
        const int src = (s & 1) && prev.prefix[s] == prev.prefix[s - 1] ? s - 1 : s;   // the upper rank shares the lower one's histogram
        scan[s * 256 + t] = hist[src * 256 + t];
    }
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 256; off <<= 1, cur ^= 1) {                                 // inclusive scan over the 256 bins
        for (int s = 0; s < kSel; ++s) {
            const unsigned* a = scan + cur * kSel * 256 + s * 256;
            scan[(cur ^ 1) * kSel * 256 + s * 256 + t] = a[t] + (t >= off ? a[t - off] : 0u);
        }
        __syncthreads();
    }
    const unsigned* incl = scan + cur * kSel * 256;
    const unsigned n = stage == 1 ? incl[255] : prev.n;
    for (int s = 0; s < kSel; ++s) {
        const unsigned r = stage == 1 ? ((s & 1) ? n / 2u : (n - 1u) / 2u) : prev.rank[s];
        const unsigned below = t ? incl[s * 256 + t - 1] : 0u;
        if (n && below <= r && r < incl[s * 256 + t]) {                                 // exactly one thread per selection
            out->prefix[s] = (prev.prefix[s] << 8) | (unsigned)t;
            out->rank[s] = r - below;
        }
    }
    if (t == 0) {
        out->n = n;
        if (!n)
            for (int s = 0; s < kSel; ++s) { out->prefix[s] = 0u; out->rank[s] = 0u; }
    }
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) {
        for (int s = 0; s < kSel; ++s) {
            state[((stage - 1) * kSel + s) * 2] = out->prefix[s];
            state[((stage - 1) * kSel + s) * 2 + 1] = out->rank[s];
        }
        state[kStateN] = n;
    }
}

__device__ __forceinline__ unsigned* image_header(unsigned* scratch, int img) { return scratch + (size_t)img * kHeaderWords; }

// ---- kernels: grid (blocks, images), 256 threads ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_prepare_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                            float* __restrict__ resampled, unsigned* __restrict__ scratch, DeGeom G) {
    __shared__ unsigned lds[kSel * kCopies * kCopyStride];
    const int img = blockIdx.y, npx = G.hg * G.wg;
    const float* p = pred + (size_t)img * G.h * G.w;
    const float* g = gt + (size_t)img * npx;
    float* rs = resampled + (size_t)img * npx;
    hist_clear(lds);
    for (int base = blockIdx.x * kDeThreads; base < npx; base += gridDim.x * kDeThreads) {   // uniform trip count per block
        const int i = base + threadIdx.x;
        int bg = -1, bp = -1;
        if (i < npx) {
            const float gv = g[i];
            float r = 0.f;
            if (gt_valid(gv, G)) {
                r = resample_at(p, i / G.wg, i % G.wg, G);
                bg = (int)(order_key(gv) >> 24);
                bp = (int)(order_key(r) >> 24);
            }
            rs[i] = r;
        }
        hist_add(lds + 0 * kCopies * kCopyStride, bg);
        hist_add(lds + 2 * kCopies * kCopyStride, bp);
    }
    hist_merge(lds, image_header(scratch, img));
}

__global__ __launch_bounds__(256) void depth_select_kernel(const float* __restrict__ gt, const float* __restrict__ resampled,
                                                           unsigned* __restrict__ scratch, DeGeom G, int pass /* 1..3 */) {
    __shared__ unsigned lds[kSel * kCopies * kCopyStride];
    __shared__ unsigned scan[2 * kSel * 256];
    __shared__ SelState st;
    const int img = blockIdx.y, npx = G.hg * G.wg;
    unsigned* hdr = image_header(scratch, img);
    resolve_stage(hdr, pass, scan, &st);
    if (!st.n) return;                                                                   // block-uniform
    const float* g = gt + (size_t)img * npx;
    const float* rs = resampled + (size_t)img * npx;
    hist_clear(lds);
    const int shift = 24 - 8 * pass;
    const bool split_g = st.prefix[0] != st.prefix[1], split_p = st.prefix[2] != st.prefix[3];
    for (int base = blockIdx.x * kDeThreads; base < npx; base += gridDim.x * kDeThreads) {
        const int i = base + threadIdx.x;
        int b[kSel] = {-1, -1, -1, -1};
        if (i < npx) {
            const float gv = g[i];
            if (gt_valid(gv, G)) {
                const unsigned kg = order_key(gv), kp = order_key(rs[i]);
                const unsigned hg = kg >> (shift + 8), hp = kp >> (shift + 8);
                const int dg = (int)((kg >> shift) & 255u), dp = (int)((kp >> shift) & 255u);
                if (hg == st.prefix[0]) b[0] = dg; else if (hg == st.prefix[1]) b[1] = dg;
                if (hp == st.prefix[2]) b[2] = dp; else if (hp == st.prefix[3]) b[3] = dp;
            }
        }
        hist_add(lds + 0 * kCopies * kCopyStride, b[0]);
        if (split_g) hist_add(lds + 1 * kCopies * kCopyStride, b[1]);
        hist_add(lds + 2 * kCopies * kCopyStride, b[2]);
        if (split_p) hist_add(lds + 3 * kCopies * kCopyStride, b[3]);
    }
    hist_merge(lds, hdr + pass * kSel * 256);
}

// partial[img][block][8]: sums over the block's masked pixels of |d|, |d|/gt, d^2/gt, [t<1.25], [t<1.25^2], [t<1.25^3], d^2,
// (log gt - log pred)^2 (utils.py:419-429), per-pixel terms in fp32 as numpy forms them, accumulated in double
__global__ __launch_bounds__(256) void depth_metrics_kernel(const float* __restrict__ gt, const float* __restrict__ resampled,
                                                            unsigned* __restrict__ scratch, double* __restrict__ partial, DeGeom G) {
    __shared__ unsigned scan[2 * kSel * 256];
    __shared__ SelState st;
    __shared__ double red[4][kSums];
    const int img = blockIdx.y, npx = G.hg * G.wg;
    unsigned* hdr = image_header(scratch, img);
    // without median scaling only n is wanted: stage 1 of the digit-0 histogram delivers it
    resolve_stage(hdr, G.scaling ? 4 : 1, scan, &st);
    double* out = partial + ((size_t)img * gridDim.x + blockIdx.x) * kSums;
    if (!st.n) {                                                                         // block-uniform
        if (threadIdx.x < kSums) out[threadIdx.x] = 0.0;
        return;
    }
    float ratio = 1.f, med_g = 0.f, med_p = 0.f;
    if (G.scaling) {
        // np.median: mean of the two middle elements in fp32 (the same element twice for odd n); utils.py:410
        med_g = (key_value(st.prefix[0]) + key_value(st.prefix[1])) * 0.5f;
        med_p = (key_value(st.prefix[2]) + key_value(st.prefix[3])) * 0.5f;
        ratio = med_g / med_p;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float* fs = reinterpret_cast<float*>(hdr + kHistWords);
        fs[kStateRatio] = ratio;
        fs[kStateMedGt] = med_g;
        fs[kStateMedPred] = med_p;
    }
    const float* g = gt + (size_t)img * npx;
    const float* rs = resampled + (size_t)img * npx;
    double acc[kSums] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * kDeThreads + threadIdx.x; i < npx; i += gridDim.x * kDeThreads) {
        const float gv = g[i];
        if (!gt_valid(gv, G)) continue;
        float p = rs[i];
        if (G.scaling) p = __fmul_rn(p, ratio);                                           // utils.py:411
        if (p < G.min_depth) p = G.min_depth;                                            // utils.py:414-416
        if (G.has_max && p > G.max_depth) p = G.max_depth;
        const float thresh = fmaxf(gv / p, p / gv);
        const float d = __fsub_rn(gv, p);
        const float d2 = __fmul_rn(d, d);
        const float dl = __fsub_rn(logf(gv), logf(p));
        acc[0] += (double)fabsf(d);
        acc[1] += (double)(fabsf(d) / gv);
        acc[2] += (double)(d2 / gv);
        acc[3] += thresh < 1.25f ? 1.0 : 0.0;
        acc[4] += thresh < 1.5625f ? 1.0 : 0.0;
        acc[5] += thresh < 1.953125f ? 1.0 : 0.0;
        acc[6] += (double)d2;
        acc[7] += (double)__fmul_rn(dl, dl);
    }
    for (int k = 0; k < kSums; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if (lane_id() == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        const int k = threadIdx.x;
        out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// one block per image: out[img] = [abs_diff, abs_rel, sq_rel, a1, a2, a3, rmse, rmse_log, ratio, n]
__global__ __launch_bounds__(256) void depth_finalize_kernel(const unsigned* __restrict__ scratch, const double* __restrict__ partial,
                                                             float* __restrict__ out, float* __restrict__ medians, int nblk) {
    __shared__ double red[4][kSums];
    const int img = blockIdx.x;
    const unsigned* state = scratch + (size_t)img * kHeaderWords + kHistWords;
    const unsigned n = state[kStateN];
    double acc[kSums] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblk; b += kDeThreads)
        for (int k = 0; k < kSums; ++k) acc[k] += partial[((size_t)img * nblk + b) * kSums + k];
    for (int k = 0; k < kSums; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if (lane_id() == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = out + (size_t)img * 10;
        const float nan = __uint_as_float(0x7fc00000u);
        const float* fs = reinterpret_cast<const float*>(state);
        if (!n) {
            for (int k = 0; k < 9; ++k) o[k] = nan;
            o[9] = 0.f;
            if (medians) medians[img * 2] = medians[img * 2 + 1] = nan;
        } else {
            double m[kSums];
            for (int k = 0; k < kSums; ++k) m[k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) / (double)n;
            o[0] = (float)m[0]; o[1] = (float)m[1]; o[2] = (float)m[2];
            o[3] = (float)m[3]; o[4] = (float)m[4]; o[5] = (float)m[5];
            o[6] = (float)sqrt(m[6]);
            o[7] = (float)sqrt(m[7]);
            o[8] = fs[kStateRatio];
            o[9] = (float)n;
            if (medians) { medians[img * 2] = fs[kStateMedGt]; medians[img * 2 + 1] = fs[kStateMedPred]; }
        }
    }
}

inline int de_blocks(int npx) { return std::max(1, std::min(kDeMaxBlocks, cdiv(npx, kDePixPerBlock))); }

}  // namespace clslam

using namespace clslam;

// 4-byte words of scratch for n_images ground-truth planes of hg x wg: header (histograms + state), block partials, the
// resampled plane.  0: bad geometry.
extern "C" int clslam_depth_metrics_scratch(int n_images, int hg, int wg) {
    if (n_images <= 0 || hg <= 0 || wg <= 0 || (long long)hg * wg > (1ll << 24)) return 0;
    const long long npx = (long long)hg * wg;
    const long long per = kHeaderWords + 2ll * kSums * de_blocks((int)npx) + npx;
    const long long total = per * n_images;
    return total < (1ll << 31) ? (int)total : 0;
}

extern "C" int clslam_depth_metrics(const float* pred, const float* gt, float* out, void* scratch_, float* resampled_out,
                                    float* medians_out, int n_images, int h, int w, int hg, int wg, float min_depth, float max_depth,
                                    int flags, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(pred && gt && out && scratch_, "depth_metrics: null pointer");
    CLSLAM_REQUIRE(n_images > 0 && n_images <= 65535 && h > 0 && w > 0 && hg > 0 && wg > 0, "depth_metrics: bad geometry");
    CLSLAM_REQUIRE((long long)h * w <= (1ll << 24) && clslam_depth_metrics_scratch(n_images, hg, wg) > 0,
                   "depth_metrics: planes of more than 2^24 pixels (n is reported in fp32) or a batch beyond 2^31 words of scratch");
    CLSLAM_REQUIRE((flags & ~7) == 0, "depth_metrics: unknown flag");
    CLSLAM_REQUIRE(min_depth == min_depth && ((flags & CLSLAM_DEPTH_EVAL_NO_MAX) || max_depth == max_depth), "depth_metrics: NaN depth bound");
    DeGeom G;
    G.h = h; G.w = w; G.hg = hg; G.wg = wg;
    G.min_depth = min_depth; G.max_depth = max_depth;
    G.has_max = (flags & CLSLAM_DEPTH_EVAL_NO_MAX) ? 0 : 1;
    G.from_disp = (flags & CLSLAM_DEPTH_EVAL_FROM_DISP) ? 1 : 0;
    G.scaling = (flags & CLSLAM_DEPTH_EVAL_MEDIAN_SCALING) ? 1 : 0;
    const int npx = hg * wg, nblk = de_blocks(npx);
    unsigned* scratch = (unsigned*)scratch_;
    double* partial = (double*)(scratch + (size_t)n_images * kHeaderWords);                   // kHeaderWords is even: 8-byte aligned
    float* plane = resampled_out ? resampled_out : (float*)(scratch + (size_t)n_images * (kHeaderWords + 2 * kSums * nblk));
    CLSLAM_REQUIRE(((size_t)scratch_ & 7) == 0, "depth_metrics: scratch must be 8-byte aligned");
    if (hipMemsetAsync(scratch, 0, (size_t)n_images * kHeaderWords * sizeof(unsigned), stream) != hipSuccess) {
        set_error("depth_metrics: hipMemsetAsync failed");
        return CLSLAM_ERR_INVALID;
    }
    const dim3 grid(nblk, n_images), block(kDeThreads);
    hipLaunchKernelGGL(depth_prepare_kernel, grid, block, 0, stream, pred, gt, plane, scratch, G);
    if (G.scaling)
        for (int pass = 1; pass < 4; ++pass)
            hipLaunchKernelGGL(depth_select_kernel, grid, block, 0, stream, gt, (const float*)plane, scratch, G, pass);
    hipLaunchKernelGGL(depth_metrics_kernel, grid, block, 0, stream, gt, (const float*)plane, scratch, partial, G);
    hipLaunchKernelGGL(depth_finalize_kernel, dim3(n_images), block, 0, stream, (const unsigned*)scratch, (const double*)partial, out,
                       medians_out, nblk);
    return check_launch("depth_metrics");
}
