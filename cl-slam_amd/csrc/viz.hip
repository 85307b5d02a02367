// Frame panels on the device (slam/utils.py:85-121 generate_figure, dpp.py:1197-1244 save_prediction): the range of a depth
// plane (smallest finite value, a percentile of the finite values), and one composing launch that writes the rows of a panel --
// image rows, the plane through a colour table, the x/z trajectory as 1-pixel lines -- as uint8 RGB into one destination image.
// The arithmetic of every row kind is stated in include/clslam_hip.h "Frame panels"; this file is held to it bit for bit, so
// contraction into fma is off for the whole file.
//
// RANGE.  Launches of clslam_viz_range (caller's stream, nothing allocated, nothing read back):
//   memset header | hist0 (digit 0 of the finite values' keys) | select x3 (digits 1..3) | finish (one block per plane).
// Three ranks are wanted per plane: 0 (vmin), k = floor(q/100 (m-1)) and min(k+1, m-1).  Pass p histograms digit p (8 bits, most
// significant first) of the values whose higher digits equal a rank's prefix; the kernel after it turns the finished histogram
// into the rank's next digit and its rank inside that bin (every block redundantly, block 0 stores the state).  Each rank has a
// histogram of its own from pass 1 on: three independent selections, no case analysis on which prefixes coincide.  Equal values
// end in one bin of every pass, so runs of equal values need no special case.  A wave whose lanes all hold one bin (digit 0 of a
// depth plane nearly always, every digit of a constant plane) adds its count with one LDS atomic.
//
// COMPOSE.  grid (bands, rows, images): a block owns kBand = min(8, 8192 / w) pixel rows of one row of the panel.  Image and
// colour rows are one pixel per thread and step.  The trajectory row is drawn into an LDS tile of one byte per pixel: every
// block walks all segments, thread-strided, clips each to its band -- on the major axis the pixel is start +- k exactly, on the
// minor axis it is monotone in k, so the k that fall into the band are an interval found without walking the segment -- marks gt
// with 1, after a barrier pred with 2 (pred over gt, and equal marks race harmlessly), then colours the band.
#include "common.h"

#pragma clang fp contract(off)

namespace clslam {

constexpr int kVzThreads = 256;
constexpr int kVzPixPerBlock = 1024;
constexpr int kVzMaxBlocks = 512;
constexpr int kVzSel = 3;                        // 0: rank 0, 1: rank k, 2: rank min(k + 1, m - 1)
constexpr int kVzHistWords = 4 * kVzSel * 256;   // [pass][selection][bin]; pass 0 uses selection 0's for all three
constexpr int kVzStateWords = 32;                // [stage 1..4][selection]{prefix, rank} = 24 words, then m
constexpr int kVzStateM = 24;
constexpr int kVzHeaderWords = kVzHistWords + kVzStateWords;
constexpr int kVzTileBytes = 8192;               // = CLSLAM_VIZ_MAX_W: a band is at least one pixel row
constexpr int kVzMaxBand = 8;
constexpr int kVzShortSegment = 16;              // up to this many candidate k the band test is done per k, beyond it by bisection
constexpr double kVzPixClamp = 1073741824.0;     // 2^30

// matplotlib's magma: (lut * 255) truncated, entry i = r | g << 8 | b << 16.  magma_r reads it backwards.
__device__ const unsigned kVzMagma[256] = {
    0x030000u, 0x040000u, 0x060000u, 0x070001u, 0x090101u, 0x0b0101u, 0x0d0202u, 0x0f0202u,
    0x110303u, 0x130304u, 0x150404u, 0x170405u, 0x190506u, 0x1b0507u, 0x1d0608u, 0x1f0709u,
    0x22070au, 0x24080bu, 0x26090cu, 0x280a0du, 0x2a0a0eu, 0x2c0b0fu, 0x2f0c10u, 0x310c11u,
    0x330d12u, 0x350d14u, 0x380e15u, 0x3a0e16u, 0x3c0f17u, 0x3f0f18u, 0x41101au, 0x44101bu,
    0x46101cu, 0x49101eu, 0x4b111fu, 0x4d1120u, 0x501122u, 0x521123u, 0x551125u, 0x571126u,
    0x591128u, 0x5c112au, 0x5e112bu, 0x60102du, 0x62102fu, 0x651030u, 0x671032u, 0x681034u,
    0x6a0f35u, 0x6c0f37u, 0x6e0f39u, 0x6f0f3bu, 0x710f3cu, 0x720f3eu, 0x730f40u, 0x740f42u,
    0x750f43u, 0x760f45u, 0x770f47u, 0x781048u, 0x79104au, 0x79104bu, 0x7a114du, 0x7b114fu,
    0x7b1250u, 0x7c1252u, 0x7c1353u, 0x7d1355u, 0x7d1457u, 0x7e1558u, 0x7e155au, 0x7e165bu,
    0x7e175du, 0x7f175eu, 0x7f1860u, 0x7f1861u, 0x7f1963u, 0x801a65u, 0x801a66u, 0x801b68u,
    0x801c69u, 0x801c6bu, 0x801d6cu, 0x811e6eu, 0x811e6fu, 0x811f71u, 0x811f73u, 0x812074u,
    0x812176u, 0x812177u, 0x812279u, 0x81227au, 0x81237cu, 0x81247eu, 0x81247fu, 0x812581u,
    0x812582u, 0x812684u, 0x812685u, 0x812787u, 0x812889u, 0x81288au, 0x80298cu, 0x80298du,
    0x802a8fu, 0x802a91u, 0x802b92u, 0x802b94u, 0x802c95u, 0x7f2c97u, 0x7f2d99u, 0x7f2d9au,
    0x7f2e9cu, 0x7e2e9eu, 0x7e2f9fu, 0x7e2fa1u, 0x7e30a3u, 0x7d30a4u, 0x7d31a6u, 0x7d31a7u,
    0x7c32a9u, 0x7c33abu, 0x7b33acu, 0x7b34aeu, 0x7b34b0u, 0x7a35b1u, 0x7a35b3u, 0x7936b5u,
    0x7936b6u, 0x7837b8u, 0x7837b9u, 0x7738bbu, 0x7739bdu, 0x7639beu, 0x753ac0u, 0x753ac2u,
    0x743bc3u, 0x743cc5u, 0x733cc6u, 0x723dc8u, 0x723ecau, 0x713ecbu, 0x703fcdu, 0x7040ceu,
    0x6f41d0u, 0x6e42d1u, 0x6d42d3u, 0x6d43d4u, 0x6c44d6u, 0x6b45d7u, 0x6a46d9u, 0x6947dau,
    0x6948dcu, 0x6849ddu, 0x674adeu, 0x664be0u, 0x664ce1u, 0x654de2u, 0x644ee4u, 0x6350e5u,
    0x6251e6u, 0x6252e7u, 0x6154e8u, 0x6055eau, 0x6056ebu, 0x5f58ecu, 0x5f59edu, 0x5e5beeu,
    0x5d5deeu, 0x5d5eefu, 0x5d60f0u, 0x5c61f1u, 0x5c63f2u, 0x5c65f3u, 0x5b67f3u, 0x5b68f4u,
    0x5b6af5u, 0x5b6cf5u, 0x5b6ef6u, 0x5b70f6u, 0x5b71f7u, 0x5c73f7u, 0x5c75f8u, 0x5c77f8u,
    0x5c79f9u, 0x5d7bf9u, 0x5d7df9u, 0x5e7ffau, 0x5e80fau, 0x5f82fau, 0x6084fbu, 0x6086fbu,
    0x6188fbu, 0x628afbu, 0x638cfcu, 0x638efcu, 0x6490fcu, 0x6592fcu, 0x6693fcu, 0x6795fdu,
    0x6897fdu, 0x6999fdu, 0x6a9bfdu, 0x6b9dfdu, 0x6c9ffdu, 0x6ea1fdu, 0x6fa2fdu, 0x70a4fdu,
    0x71a6feu, 0x73a8feu, 0x74aafeu, 0x75acfeu, 0x76aefeu, 0x78affeu, 0x79b1feu, 0x7bb3feu,
    0x7cb5feu, 0x7db7feu, 0x7fb9feu, 0x80bbfeu, 0x82bcfeu, 0x83befeu, 0x85c0feu, 0x86c2feu,
    0x88c4feu, 0x89c6feu, 0x8bc7feu, 0x8dc9feu, 0x8ecbfeu, 0x90cdfdu, 0x92cffdu, 0x93d1fdu,
    0x95d2fdu, 0x97d4fdu, 0x98d6fdu, 0x9ad8fdu, 0x9cdafdu, 0x9ddcfdu, 0x9fddfdu, 0xa1dffdu,
    0xa3e1fdu, 0xa5e3fcu, 0xa6e5fcu, 0xa8e6fcu, 0xaae8fcu, 0xaceafcu, 0xaeecfcu, 0xb0eefcu,
    0xb1f0fcu, 0xb3f1fcu, 0xb5f3fcu, 0xb7f5fcu, 0xb9f7fbu, 0xbbf9fbu, 0xbdfafbu, 0xbffcfbu,
};

// ---- range ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned vz_key(float v) {                       // unsigned order of the keys = order of the values
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vz_key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool vz_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// q / 100 * (m - 1): the one place the fractional rank is formed (stage 1 takes its floor, the finishing block its fraction)
__device__ __forceinline__ double vz_rank_pos(double q, unsigned m) { return q / 100.0 * (double)(m - 1u); }

// h[256] += 1 at `bin` of every lane that has one (bin < 0: nothing).  Called by all 64 lanes of the wave.
__device__ __forceinline__ void vz_hist_add(unsigned* __restrict__ h, int bin) {
    // what a group of lanes holds: -1 nothing, 0..255 that one bin, 512 several (small integers: exact in fp32)
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
        atomicAdd(&h[bin], 1u);
    }
}

struct VzState {
    unsigned prefix[kVzSel];   // the digits found so far, right-aligned
    unsigned rank[kVzSel];     // rank among the values that carry the prefix
    unsigned m;                // finite values of the plane
};

// Stage s (1..4): the finished histograms of pass s-1 and the state of stage s-1 -> digit s-1 of every rank.  All blocks compute
// the same; block x = 0 stores it for the next kernel.  scan: 2 * kVzSel * 256 words of LDS.
__device__ void vz_resolve(unsigned* __restrict__ hdr, int stage, double q, unsigned* scan, VzState* out /* LDS */) {
    const int t = threadIdx.x;
    unsigned* state = hdr + kVzHistWords;
    __shared__ VzState prev;
    if (t == 0) {
        for (int s = 0; s < kVzSel; ++s) {
            prev.prefix[s] = stage == 1 ? 0u : state[((stage - 2) * kVzSel + s) * 2];
            prev.rank[s] = stage == 1 ? 0u : state[((stage - 2) * kVzSel + s) * 2 + 1];
        }
        prev.m = stage == 1 ? 0u : state[kVzStateM];
    }
    for (int s = 0; s < kVzSel; ++s) scan[s * 256 + t] = hdr[((stage - 1) * kVzSel + (stage == 1 ? 0 : s)) * 256 + t];
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 256; off <<= 1, cur ^= 1) {                     // inclusive scan over the 256 bins
        for (int s = 0; s < kVzSel; ++s) {
            const unsigned* a = scan + (cur * kVzSel + s) * 256;
            scan[((cur ^ 1) * kVzSel + s) * 256 + t] = a[t] + (t >= off ? a[t - off] : 0u);
        }
        __syncthreads();
    }
    const unsigned* incl = scan + cur * kVzSel * 256;
    const unsigned m = stage == 1 ? incl[255] : prev.m;
    unsigned first[kVzSel] = {0u, 0u, 0u};
    if (stage == 1 && m) {
        const unsigned k = (unsigned)floor(vz_rank_pos(q, m));
        first[1] = k;
        first[2] = k + 1u < m ? k + 1u : m - 1u;
    }
    for (int s = 0; s < kVzSel; ++s) {
        const unsigned r = stage == 1 ? first[s] : prev.rank[s];
        const unsigned below = t ? incl[s * 256 + t - 1] : 0u;
        if (m && below <= r && r < incl[s * 256 + t]) {                     // exactly one thread per selection
            out->prefix[s] = (prev.prefix[s] << 8) | (unsigned)t;
            out->rank[s] = r - below;
        }
    }
    if (t == 0) {
        out->m = m;
        if (!m)
            for (int s = 0; s < kVzSel; ++s) { out->prefix[s] = 0u; out->rank[s] = 0u; }
    }
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) {
        for (int s = 0; s < kVzSel; ++s) {
            state[((stage - 1) * kVzSel + s) * 2] = out->prefix[s];
            state[((stage - 1) * kVzSel + s) * 2 + 1] = out->rank[s];
        }
        state[kVzStateM] = m;
    }
}

// grid (blocks, planes)
__global__ __launch_bounds__(256) void viz_range_hist0_kernel(const float* __restrict__ planes, unsigned* __restrict__ scratch,
                                                              int npx) {
    __shared__ unsigned lds[256];
    const float* p = planes + (size_t)blockIdx.y * npx;
    lds[threadIdx.x] = 0u;
    __syncthreads();
    for (int base = blockIdx.x * kVzThreads; base < npx; base += gridDim.x * kVzThreads) {   // uniform trip count per block
        const int i = base + threadIdx.x;
        int bin = -1;
        if (i < npx) {
            const float v = p[i];
            if (vz_finite(v)) bin = (int)(vz_key(v) >> 24);
        }
        vz_hist_add(lds, bin);
    }
    __syncthreads();
    const unsigned c = lds[threadIdx.x];
    if (c) atomicAdd(&scratch[(size_t)blockIdx.y * kVzHeaderWords + threadIdx.x], c);
}

__global__ __launch_bounds__(256) void viz_range_select_kernel(const float* __restrict__ planes, unsigned* __restrict__ scratch,
                                                               int npx, double q, int pass /* 1..3 */) {
    __shared__ unsigned lds[kVzSel * 256];
    __shared__ unsigned scan[2 * kVzSel * 256];
    __shared__ VzState st;
    unsigned* hdr = scratch + (size_t)blockIdx.y * kVzHeaderWords;
    vz_resolve(hdr, pass, q, scan, &st);
    if (!st.m) return;                                                      // block-uniform
    const float* p = planes + (size_t)blockIdx.y * npx;
    for (int s = 0; s < kVzSel; ++s) lds[s * 256 + threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    for (int base = blockIdx.x * kVzThreads; base < npx; base += gridDim.x * kVzThreads) {
        const int i = base + threadIdx.x;
        bool ok = false;
        unsigned high = 0u;
        int digit = 0;
        if (i < npx) {
            const float v = p[i];
            const unsigned key = vz_key(v);
            ok = vz_finite(v);
            high = key >> (shift + 8);
            digit = (int)((key >> shift) & 255u);
        }
        for (int s = 0; s < kVzSel; ++s) vz_hist_add(lds + s * 256, ok && high == st.prefix[s] ? digit : -1);
    }
    __syncthreads();
    for (int s = 0; s < kVzSel; ++s) {
        const unsigned c = lds[s * 256 + threadIdx.x];
        if (c) atomicAdd(&hdr[(pass * kVzSel + s) * 256 + threadIdx.x], c);
    }
}

// grid (planes): range[plane] = {vmin, vmax}, count[plane] = m
__global__ __launch_bounds__(256) void viz_range_finish_kernel(unsigned* __restrict__ scratch, float* __restrict__ range,
                                                               int* __restrict__ count, double q) {
    __shared__ unsigned scan[2 * kVzSel * 256];
    __shared__ VzState st;
    const int img = blockIdx.x;
    vz_resolve(scratch + (size_t)img * kVzHeaderWords, 4, q, scan, &st);     // the prefixes are the whole keys now
    if (threadIdx.x != 0) return;
    count[img] = (int)st.m;
    if (!st.m) {
        range[img * 2] = range[img * 2 + 1] = __uint_as_float(0x7fc00000u);
        return;
    }
    const double lo = (double)vz_key_value(st.prefix[1]), hi = (double)vz_key_value(st.prefix[2]);
    const double pos = vz_rank_pos(q, st.m);
    const double g = pos - floor(pos);
    range[img * 2] = vz_key_value(st.prefix[0]);
    range[img * 2 + 1] = (float)(lo + (hi - lo) * g);
}

inline int vz_blocks(long long npx) { return (int)std::max(1ll, std::min((long long)kVzMaxBlocks, (npx + kVzPixPerBlock - 1) / kVzPixPerBlock)); }

// ---- compose -------------------------------------------------------------------------------------------------------------------
struct VzRow {
    const void* src;
    const float* range;
    const double* gt;
    const double* pred;
    long long src_stride;
    double x0, xs, y1, ys;      // u = floor((x - x0) / xs * w), v = floor((y1 - y) / ys * h)
    int kind, reversed, n_gt, n_pred;
};
struct VzPanel {
    VzRow row[CLSLAM_VIZ_MAX_ROWS];
};

template <typename T>
__device__ __forceinline__ unsigned vz_byte(T x) {                          // trunc(clamp(x, 0, 1) * 255 + 0.5), NaN -> 0
    const T c = !(x > (T)0) ? (T)0 : x > (T)1 ? (T)1 : x;
    return (unsigned)(c * (T)255 + (T)0.5);
}
__device__ __forceinline__ unsigned vz_byte(unsigned char x) { return x; }

// packed r | g << 8 | b << 16.  matplotlib's Normalize holds vmin and vmax as float64 and works in place on the float32 plane:
// x - vmin and the quotient by the EXACT vmax - vmin are float64 operations, each rounded to float32 as it is stored; the
// colour map's * 256 is float32.  The float64 division is the correctly rounded one (no reciprocal approximation).
__device__ __forceinline__ unsigned vz_colour(float x, float vmin, float vmax, int reversed) {
    if (x != x) return 0u;
    int idx = 0;
    if (vmin != vmax) {
        const float r = (float)((double)x - (double)vmin);
        const float xa = (float)((double)r / ((double)vmax - (double)vmin)) * 256.f;
        if (xa != xa) return 0u;
        idx = xa < 0.f ? 0 : xa >= 256.f ? 255 : (int)xa;
    }
    return kVzMagma[reversed ? 255 - idx : idx];
}

__device__ __forceinline__ void vz_store(unsigned char* __restrict__ p, unsigned rgb) {
    p[0] = (unsigned char)(rgb & 255u);
    p[1] = (unsigned char)((rgb >> 8) & 255u);
    p[2] = (unsigned char)((rgb >> 16) & 255u);
}

template <typename T>
__device__ __forceinline__ unsigned vz_pixel(const T* __restrict__ img, long long plane, long long i, bool chw) {
    if (chw) return vz_byte(img[i]) | vz_byte(img[plane + i]) << 8 | vz_byte(img[2 * plane + i]) << 16;
    return vz_byte(img[3 * i]) | vz_byte(img[3 * i + 1]) << 8 | vz_byte(img[3 * i + 2]) << 16;
}

__device__ __forceinline__ long long vz_floordiv(long long a, long long b /* > 0 */) {
    const long long d = a / b;
    return a % b < 0 ? d - 1 : d;
}
__device__ __forceinline__ long long vz_to_pixel(double t) {
    return (long long)fmin(fmax(floor(t), -kVzPixClamp), kVzPixClamp);
}
__device__ __forceinline__ bool vz_finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// marks the pixels of the segment (u0,v0)-(u1,v1) that lie in the rows [ylo, yhi) and the columns [0, w) of the tile
__device__ void vz_draw_segment(unsigned char* tile, int ylo, int yhi, int w, long long u0, long long v0, long long u1,
                                long long v1, unsigned char mark) {
    const long long du = u1 - u0, dv = v1 - v0;
    const long long adu = du < 0 ? -du : du, adv = dv < 0 ? -dv : dv;
    const long long n = adu > adv ? adu : adv;
    if (min(u0, u1) >= w || max(u0, u1) < 0 || min(v0, v1) >= yhi || max(v0, v1) < ylo) return;      // the box misses the band
    if (n == 0) {
        tile[(v0 - ylo) * w + u0] = mark;
        return;
    }
    // major axis a: position a0 + sa * k exactly (floor((+-2kn + n) / 2n) = +-k); minor axis b: monotone in k
    const bool xmajor = adu >= adv;
    const long long a0 = xmajor ? u0 : v0, sa = (xmajor ? du : dv) < 0 ? -1 : 1;
    const long long alo = xmajor ? 0 : ylo, ahi = xmajor ? w : yhi;
    const long long b0 = xmajor ? v0 : u0, db = xmajor ? dv : du;
    const long long blo = xmajor ? ylo : 0, bhi = xmajor ? yhi : w;
    long long klo = sa > 0 ? alo - a0 : a0 - (ahi - 1);
    long long khi = sa > 0 ? ahi - 1 - a0 : a0 - alo;                        // inclusive
    klo = klo < 0 ? 0 : klo;
    khi = khi > n ? n : khi;
    if (klo > khi) return;
    // |a0| <= 2^30 and the band is inside [0, 2^13] x [0, 2^24]: k <= 2^30 + 2^24, |db| <= 2^31 -- 2 k db + n stays below 2^63
    auto minor = [&](long long k) { return b0 + vz_floordiv(2 * k * db + n, 2 * n); };
    if (khi - klo >= kVzShortSegment) {
        // first k in [klo, khi + 1] from which on the minor coordinate has passed `bound` in its direction of travel
        auto first = [&](long long bound) {
            long long lo = klo, hi = khi + 1;
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (db >= 0 ? minor(mid) >= bound : minor(mid) < bound) hi = mid; else lo = mid + 1;
            }
            return lo;
        };
        const long long ka = first(db >= 0 ? blo : bhi), kb = first(db >= 0 ? bhi : blo);
        klo = ka;
        khi = kb - 1;
    }
    for (long long k = klo; k <= khi; ++k) {
        const long long a = a0 + sa * k, b = minor(k);
        if (b < blo || b >= bhi) continue;
        const long long x = xmajor ? a : b, y = xmajor ? b : a;
        tile[(y - ylo) * w + x] = mark;
    }
}

__device__ void vz_draw_polyline(unsigned char* tile, int ylo, int yhi, int h, int w, const double* __restrict__ xz, int nv,
                                 const VzRow& R, unsigned char mark) {
    const int nseg = nv == 1 ? 1 : nv - 1;
    for (int s = threadIdx.x; s < nseg; s += kVzThreads) {
        const int e = nv == 1 ? s : s + 1;
        const double xa = xz[2 * s], ya = xz[2 * s + 1], xb = xz[2 * e], yb = xz[2 * e + 1];
        if (!(vz_finite64(xa) && vz_finite64(ya) && vz_finite64(xb) && vz_finite64(yb))) continue;
        vz_draw_segment(tile, ylo, yhi, w, vz_to_pixel((xa - R.x0) / R.xs * (double)w), vz_to_pixel((R.y1 - ya) / R.ys * (double)h),
                        vz_to_pixel((xb - R.x0) / R.xs * (double)w), vz_to_pixel((R.y1 - yb) / R.ys * (double)h), mark);
    }
}

// grid (bands, rows, images)
__global__ __launch_bounds__(256) void viz_compose_kernel(VzPanel P, unsigned char* __restrict__ dst, long long dst_image_stride,
                                                          long long dst_row_stride, int row0, int h, int w, int band) {
    __shared__ unsigned char tile[kVzTileBytes];
    const VzRow& R = P.row[blockIdx.y];
    const int img = blockIdx.z;
    const int ylo = blockIdx.x * band, yhi = min(h, ylo + band);
    const int npix = (yhi - ylo) * w;                                       // <= kVzTileBytes
    unsigned char* out = dst + (size_t)img * dst_image_stride + (size_t)(row0 + (long long)blockIdx.y * h + ylo) * dst_row_stride;
    const long long plane = (long long)h * w, first = (long long)ylo * w;
    if (R.kind == CLSLAM_VIZ_ROW_TRAJ) {
        for (int i = threadIdx.x; i < npix; i += kVzThreads) tile[i] = 0;
        __syncthreads();
        if (R.n_gt > 0) vz_draw_polyline(tile, ylo, yhi, h, w, R.gt, R.n_gt, R, 1);
        __syncthreads();
        if (R.n_pred > 0) vz_draw_polyline(tile, ylo, yhi, h, w, R.pred, R.n_pred, R, 2);
        __syncthreads();
    }
    float vmin = 0.f, vmax = 0.f;
    if (R.kind == CLSLAM_VIZ_ROW_CMAP) {
        vmin = R.range[2 * img];
        vmax = R.range[2 * img + 1];
    }
    for (int i = threadIdx.x; i < npix; i += kVzThreads) {
        const int y = i / w, x = i - y * w;
        const long long at = first + i;                                     // pixel of the row's plane
        unsigned rgb;
        switch (R.kind) {
        case CLSLAM_VIZ_ROW_CHW_F32: rgb = vz_pixel((const float*)R.src + (size_t)img * R.src_stride, plane, at, true); break;
        case CLSLAM_VIZ_ROW_HWC_F32: rgb = vz_pixel((const float*)R.src + (size_t)img * R.src_stride, plane, at, false); break;
        case CLSLAM_VIZ_ROW_HWC_F64: rgb = vz_pixel((const double*)R.src + (size_t)img * R.src_stride, plane, at, false); break;
        case CLSLAM_VIZ_ROW_HWC_U8: rgb = vz_pixel((const unsigned char*)R.src + (size_t)img * R.src_stride, plane, at, false); break;
        case CLSLAM_VIZ_ROW_CMAP:
            rgb = vz_colour(((const float*)R.src)[(size_t)img * R.src_stride + at], vmin, vmax, R.reversed);
            break;
        default: rgb = tile[i] == 2 ? 0x0e7fffu : tile[i] == 1 ? 0xb4771fu : 0xffffffu; break;   // pred C1, gt C0, white
        }
        vz_store(out + (size_t)y * dst_row_stride + 3 * x, rgb);
    }
}

}  // namespace clslam

using namespace clslam;

extern "C" long long clslam_viz_range_scratch(int n) {
    if (n <= 0 || n > 65535) return 0;
    return (long long)n * kVzHeaderWords * (long long)sizeof(unsigned);
}

extern "C" int clslam_viz_range(const float* planes, float* range, int* count, void* scratch_, long long scratch_bytes, int n,
                                long long npx, double q, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n >= 0 && n <= 65535, "viz_range: 0..65535 planes per call");
    CLSLAM_REQUIRE(npx >= 1 && npx <= (1ll << 30), "viz_range: planes of 1..2^30 values");
    CLSLAM_REQUIRE(q >= 0.0 && q <= 100.0, "viz_range: the percentile q must lie in [0, 100]");
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(planes && range && count && scratch_, "viz_range: null pointer");
    CLSLAM_REQUIRE(((size_t)scratch_ & 7) == 0 && scratch_bytes >= clslam_viz_range_scratch(n),
                   "viz_range: scratch must be 8-byte aligned and hold clslam_viz_range_scratch(n) bytes");
    unsigned* scratch = (unsigned*)scratch_;
    if (hipMemsetAsync(scratch, 0, (size_t)clslam_viz_range_scratch(n), stream) != hipSuccess) {
        set_error("viz_range: hipMemsetAsync failed");
        return CLSLAM_ERR_INVALID;
    }
    const dim3 grid(vz_blocks(npx), n), block(kVzThreads);
    hipLaunchKernelGGL(viz_range_hist0_kernel, grid, block, 0, stream, planes, scratch, (int)npx);
    for (int pass = 1; pass < 4; ++pass)
        hipLaunchKernelGGL(viz_range_select_kernel, grid, block, 0, stream, planes, scratch, (int)npx, q, pass);
    hipLaunchKernelGGL(viz_range_finish_kernel, dim3(n), block, 0, stream, scratch, range, count, q);
    return check_launch("viz_range");
}

static bool vz_limits_ok(const double* lim) {
    return lim[0] - lim[0] == 0.0 && lim[1] - lim[1] == 0.0 && lim[0] != lim[1] && (lim[1] - lim[0]) - (lim[1] - lim[0]) == 0.0;
}

extern "C" int clslam_viz_compose(const clslam_viz_row* rows, int n_rows, unsigned char* dst, long long dst_image_stride,
                                  long long dst_row_stride, int row0, int n, int h, int w, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(rows && n_rows >= 1 && n_rows <= CLSLAM_VIZ_MAX_ROWS, "viz_compose: 1..%d rows", CLSLAM_VIZ_MAX_ROWS);
    CLSLAM_REQUIRE(n >= 0 && n <= 65535, "viz_compose: 0..65535 images per call");
    CLSLAM_REQUIRE(h >= 1 && h <= (1 << 24) && w >= 1 && w <= CLSLAM_VIZ_MAX_W && (long long)h * w <= (1ll << 30),
                   "viz_compose: rows of 1 <= h <= 2^24, 1 <= w <= %d, h * w <= 2^30 pixels", CLSLAM_VIZ_MAX_W);
    CLSLAM_REQUIRE(row0 >= 0 && (long long)row0 + (long long)n_rows * h <= (1ll << 30) && dst_row_stride >= 3ll * w && dst_image_stride >= 0,
                   "viz_compose: bad destination geometry (row0 >= 0, dst_row_stride >= 3 * w)");
    VzPanel P;
    for (int r = 0; r < n_rows; ++r) {
        const clslam_viz_row& in = rows[r];
        VzRow& R = P.row[r];
        R = VzRow{};
        R.kind = in.kind;
        if (in.kind == CLSLAM_VIZ_ROW_TRAJ) {
            CLSLAM_REQUIRE(in.n_gt >= 0 && in.n_pred >= 0 && in.n_gt <= (1 << 24) && in.n_pred <= (1 << 24),
                           "viz_compose: polylines of 0..2^24 vertices");
            CLSLAM_REQUIRE((in.n_gt == 0 || (in.gt_xz && ((size_t)in.gt_xz & 7) == 0)) &&
                           (in.n_pred == 0 || (in.pred_xz && ((size_t)in.pred_xz & 7) == 0)),
                           "viz_compose: a polyline with vertices needs an 8-byte-aligned pointer");
            CLSLAM_REQUIRE(vz_limits_ok(in.xlim) && vz_limits_ok(in.ylim), "viz_compose: xlim / ylim must be finite with distinct ends");
            R.gt = in.gt_xz; R.pred = in.pred_xz; R.n_gt = in.n_gt; R.n_pred = in.n_pred;
            R.x0 = in.xlim[0]; R.xs = in.xlim[1] - in.xlim[0];
            R.y1 = in.ylim[1]; R.ys = in.ylim[1] - in.ylim[0];
        } else {
            CLSLAM_REQUIRE(in.kind >= CLSLAM_VIZ_ROW_CHW_F32 && in.kind <= CLSLAM_VIZ_ROW_CMAP, "viz_compose: unknown row kind %d", in.kind);
            const long long per_image = (long long)h * w * (in.kind == CLSLAM_VIZ_ROW_CMAP ? 1 : 3);
            CLSLAM_REQUIRE(in.src && in.src_stride >= per_image, "viz_compose: row %d needs a source and a stride of at least one image", r);
            const size_t align = in.kind == CLSLAM_VIZ_ROW_HWC_F64 ? 7 : in.kind == CLSLAM_VIZ_ROW_HWC_U8 ? 0 : 3;
            CLSLAM_REQUIRE(((size_t)in.src & align) == 0, "viz_compose: row %d's source is not aligned to its element", r);
            R.src = in.src; R.src_stride = in.src_stride;
            if (in.kind == CLSLAM_VIZ_ROW_CMAP) {
                CLSLAM_REQUIRE(in.range && ((size_t)in.range & 3) == 0, "viz_compose: a colour row needs its (n,2) range on the device");
                CLSLAM_REQUIRE(in.cmap == CLSLAM_VIZ_CMAP_MAGMA || in.cmap == CLSLAM_VIZ_CMAP_MAGMA_R, "viz_compose: unknown colour map %d", in.cmap);
                R.range = in.range;
                R.reversed = in.cmap == CLSLAM_VIZ_CMAP_MAGMA_R;
            }
        }
    }
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(dst, "viz_compose: null destination");
    const int band = std::max(1, std::min(kVzMaxBand, kVzTileBytes / w));
    hipLaunchKernelGGL(viz_compose_kernel, dim3(cdiv(h, band), n_rows, n), dim3(kVzThreads), 0, stream, P, dst, dst_image_stride,
                       dst_row_stride, row0, h, w, band);
    return check_launch("viz_compose");
}
