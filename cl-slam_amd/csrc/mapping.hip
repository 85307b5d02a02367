// Dense mapping on the device (slam/utils.py:25-38 depth_to_pcl, :76-82 accumulate_pcl, :41-58 pcl_to_image): a depth plane
// becomes a compacted coloured cloud, a cloud stored per camera frame is posed by one fp64 matrix per segment, and a cloud is
// z-buffered into a camera.  A cloud is (M,6) fp32 rows [x, y, z, r, g, b].
//
// BACKPROJECT is count -> scan -> scatter, because the order of the kept points is part of the contract (the reference's
// boolean mask keeps pixel order) and an atomically bumped cursor would not give it: one block per chunk of kBpChunk pixels
// counts its kept points, ONE block scans the chunk counts into 64-bit chunk offsets and the (N+1) image offsets, and the
// scatter recomputes the points (same function, same bits), ranks them inside the chunk by an LDS scan, compacts them in LDS
// and copies the chunk's rows out as one contiguous, coalesced run.
//
// ROWS OF 24 BYTES.  A thread per point reading its own row would spread every load instruction of a wave over 1.5 KiB.
// Transform and splat therefore stage tiles of kTile rows through LDS with 8-byte accesses (a row offset is a multiple of
// 24 bytes: 8-byte aligned), lane i at base + 8 i, and the transform writes its tile back the same way.
//
// SEGMENTS.  A block finds the segment of its first point by binary search on the offsets (thread 0) and every thread advances
// from there; empty segments are stepped over by the search and by the advance alike.  Neither walks past the last segment,
// whatever the offsets hold.
//
// Z-BUFFER.  key = (bits of the fp32 distance) << 32 | point index inside the launch, minimised with the 64-bit integer
// atomicMin (the only atomic here; no floating-point atomics: two launches agree bitwise).  Non-negative fp32 bit patterns
// order like the numbers, so the smallest key is the closest point and among equal distances the lowest index -- the
// reference's strict `distance < depth[v, u]` in loop order (:55).  A plain read in front of the atomic drops the points that
// have already lost (the buffer only ever decreases, so a stale read costs an atomic, never a winner).
//
// ARITHMETIC.  Contraction is off for this file: the projection, the pose and the norms are the sequences of individually
// rounded operations the header states, so that a numpy restatement matches the pixel assignment bit for bit (hipcc contracts
// a * b + c to an fma by default, and __dmul_rn / __dadd_rn are plain operators in its headers).
#include "common.h"

#pragma clang fp contract(off)

namespace clslam {

constexpr int kMapThreads = 256;
constexpr int kBpChunk = 1024;                       // pixels per backproject block
constexpr int kTile = 256;                           // rows per LDS tile (6 KiB)
constexpr int kTilesPerBlock = 4;
constexpr int kMapChunk = kTile * kTilesPerBlock;    // points per transform / splat block
constexpr unsigned long long kZEmpty = ~0ull;
constexpr double kDblMax = 1.7976931348623157e308;

#if !CLSLAM_DEVICE_BUILD
// host build (kernel sources run block by block on several host threads): the 64-bit minimum as a compare-exchange loop
inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
    unsigned long long o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
    return o;
}
#endif

// ---- backproject --------------------------------------------------------------------------------------------------------------
struct BpPoint {
    float x, y, z;
    int keep;
};

// layers.py:74-79: cam = depth * (inv_K[:3,:3] . (px, py, 1)), every operation rounded to fp32; utils.py:35-37: kept iff the
// fp32 norm is below the threshold (NaN compares false: dropped), or the threshold is infinite
__device__ __forceinline__ BpPoint bp_point(const float* __restrict__ ik, float d, int px, int py, float thr, int keep_all) {
    const float fx = (float)px, fy = (float)py;
    BpPoint p;
    p.x = d * ((ik[0] * fx + ik[1] * fy) + ik[2]);
    p.y = d * ((ik[4] * fx + ik[5] * fy) + ik[6]);
    p.z = d * ((ik[8] * fx + ik[9] * fy) + ik[10]);
    p.keep = keep_all || sqrtf((p.x * p.x + p.y * p.y) + p.z * p.z) < thr;
    return p;
}

// grid (chunks, images): counts[image * chunks + chunk] = kept points of the chunk
__global__ __launch_bounds__(256) void pcl_bp_count_kernel(const float* __restrict__ depth, const float* __restrict__ inv_k,
                                                           unsigned* __restrict__ counts, int npx, int W, float thr, int keep_all) {
    __shared__ float red[kMapThreads / kWave];
    const int img = blockIdx.y, base = blockIdx.x * kBpChunk, t = threadIdx.x;
    unsigned* out = counts + (size_t)img * gridDim.x + blockIdx.x;
    if (keep_all) {
        if (t == 0) *out = (unsigned)min(kBpChunk, npx - base);
        return;
    }
    const float* ik = inv_k + (size_t)img * 16;
    const float* dp = depth + (size_t)img * npx;
    float c = 0.f;                                                             // <= 4 per thread: exact
    for (int j = 0; j < kBpChunk / kMapThreads; ++j) {
        const int p = base + j * kMapThreads + t;
        if (p < npx) c += (float)bp_point(ik, dp[p], p % W, p / W, thr, 0).keep;
    }
    c = wave_sum(c);
    if (lane_id() == 0) red[t >> 6] = c;
    __syncthreads();
    if (t == 0) *out = (unsigned)(((red[0] + red[1]) + red[2]) + red[3]);
}

// one block: exclusive scan of the G chunk counts in 64 bits -> chunk_off[G]; offsets[i] = first row of image i, offsets[N] = total
__global__ __launch_bounds__(256) void pcl_bp_scan_kernel(const unsigned* __restrict__ counts, long long* __restrict__ chunk_off,
                                                          long long* __restrict__ offsets, int G, int chunks, int n_images) {
    __shared__ unsigned long long s[2][kMapThreads];
    const int t = threadIdx.x;
    const int per = (G + kMapThreads - 1) / kMapThreads;
    const int lo = (int)min((long long)t * per, (long long)G), hi = (int)min((long long)lo + per, (long long)G);
    unsigned long long own = 0;
    for (int g = lo; g < hi; ++g) own += counts[g];
    s[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kMapThreads; off <<= 1, cur ^= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= off ? s[cur][t - off] : 0ull);
        __syncthreads();
    }
    unsigned long long run = s[cur][t] - own;
    for (int g = lo; g < hi; ++g) {
        chunk_off[g] = (long long)run;
        if (g % chunks == 0) offsets[g / chunks] = (long long)run;
        run += counts[g];
    }
    if (t == kMapThreads - 1) offsets[n_images] = (long long)s[cur][t];
}

// grid (chunks, images): the chunk's kept rows, in pixel order, at out + chunk_off * 6
__global__ __launch_bounds__(256) void pcl_bp_scatter_kernel(const float* __restrict__ depth, const float* __restrict__ inv_k,
                                                             const float* __restrict__ image, const long long* __restrict__ chunk_off,
                                                             float* __restrict__ out, int npx, int W, float thr, int keep_all) {
    __shared__ float2 rows2[kBpChunk * 3];            // the compacted rows of the chunk, 24 KiB
    __shared__ int rank[kBpChunk];                    // keep flag, then the row's rank inside the chunk
    __shared__ int scan[2][kMapThreads];
    float* rows = reinterpret_cast<float*>(rows2);
    const int img = blockIdx.y, base = blockIdx.x * kBpChunk, t = threadIdx.x;
    const float* ik = inv_k + (size_t)img * 16;
    const float* dp = depth + (size_t)img * npx;
    const float* ip = image + (size_t)img * 3 * npx;
    constexpr int kPer = kBpChunk / kMapThreads;
    float v[kPer][6];
    int keep[kPer];
    for (int j = 0; j < kPer; ++j) {                  // coalesced: lane i at pixel base + 256 j + i of each plane
        const int p = base + j * kMapThreads + t;
        keep[j] = 0;
        if (p < npx) {
            const BpPoint b = bp_point(ik, dp[p], p % W, p / W, thr, keep_all);
            keep[j] = b.keep;
            v[j][0] = b.x; v[j][1] = b.y; v[j][2] = b.z;
            v[j][3] = ip[p]; v[j][4] = ip[npx + p]; v[j][5] = ip[2 * npx + p];
        }
        rank[j * kMapThreads + t] = keep[j];
    }
    __syncthreads();
    int f[kPer], own = 0;                             // thread t ranks the pixels kPer * t ... of the chunk
    for (int k = 0; k < kPer; ++k) { f[k] = rank[kPer * t + k]; own += f[k]; }
    scan[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kMapThreads; off <<= 1, cur ^= 1) {
        scan[cur ^ 1][t] = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0);
        __syncthreads();
    }
    int run = scan[cur][t] - own;
    for (int k = 0; k < kPer; ++k) { rank[kPer * t + k] = run; run += f[k]; }
    const int total = scan[cur][kMapThreads - 1];
    __syncthreads();
    for (int j = 0; j < kPer; ++j)
        if (keep[j]) {
            float* r = rows + 6 * rank[j * kMapThreads + t];
            for (int c = 0; c < 6; ++c) r[c] = v[j][c];
        }
    __syncthreads();
    float2* dst = reinterpret_cast<float2*>(out + chunk_off[(size_t)img * gridDim.x + blockIdx.x] * 6);
    for (int i = t; i < total * 3; i += kMapThreads) dst[i] = rows2[i];
}

// ---- tiles of rows through LDS ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_load(const float* __restrict__ g, float2* tile, int cnt) {
    const float2* s = reinterpret_cast<const float2*>(g);
    for (int i = threadIdx.x; i < cnt * 3; i += kMapThreads) tile[i] = s[i];
}
__device__ __forceinline__ void tile_store(float* __restrict__ g, const float2* tile, int cnt) {
    float2* d = reinterpret_cast<float2*>(g);
    for (int i = threadIdx.x; i < cnt * 3; i += kMapThreads) d[i] = tile[i];
}

// the segment that holds point p: the number of f in [0, F-1) with offsets[f+1] <= p (empty segments end at or before p too)
__device__ __forceinline__ int find_segment(const long long* __restrict__ offs, int F, long long p) {
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (offs[mid + 1] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int advance_segment(const long long* __restrict__ offs, int F, int f, long long p) {
    while (f + 1 < F && p >= offs[f + 1]) ++f;
    return f;
}

// utils.py:79-80 for one point: R . xyz + t in fp64 from the fp32 coordinates, left to right, rounded once to fp32
__device__ __forceinline__ void pose_apply(const double* __restrict__ T, float& x, float& y, float& z) {
    const double X = x, Y = y, Z = z;
    const double a = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    const double b = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    const double c = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    x = (float)a; y = (float)b; z = (float)c;
}

__global__ __launch_bounds__(256) void pcl_transform_kernel(const float* __restrict__ pts, const long long* __restrict__ offs,
                                                            const double* __restrict__ poses, float* __restrict__ out, long long M,
                                                            int F) {
    __shared__ float2 tile2[kTile * 3];
    __shared__ int seg0;
    float* tile = reinterpret_cast<float*>(tile2);
    const long long chunk0 = (long long)blockIdx.x * kMapChunk;
    if (threadIdx.x == 0) seg0 = find_segment(offs, F, chunk0);
    __syncthreads();
    int f = seg0;
    for (int j = 0; j < kTilesPerBlock; ++j) {
        const long long base = chunk0 + (long long)j * kTile;
        if (base >= M) break;                                                  // block-uniform
        const int cnt = (int)min((long long)kTile, M - base);
        tile_load(pts + base * 6, tile2, cnt);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            f = advance_segment(offs, F, f, base + threadIdx.x);
            float* r = tile + 6 * threadIdx.x;
            pose_apply(poses + (size_t)f * 16, r[0], r[1], r[2]);
        }
        __syncthreads();
        tile_store(out + base * 6, tile2, cnt);
        __syncthreads();
    }
}

// ---- splat / resolve ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pcl_splat_kernel(const float* __restrict__ pts, const long long* __restrict__ offs,
                                                        const double* __restrict__ poses, int F, const double* __restrict__ K,
                                                        unsigned long long* __restrict__ zbuf, int rows, int cols,
                                                        long long point_base, long long count, int has_min_z, double min_z) {
    __shared__ float2 tile2[kTile * 3];
    __shared__ int seg0;
    const float* tile = reinterpret_cast<const float*>(tile2);
    const long long chunk0 = (long long)blockIdx.x * kMapChunk;                // inside the launch: [0, count)
    if (poses) {
        if (threadIdx.x == 0) seg0 = find_segment(offs, F, point_base + chunk0);
        __syncthreads();
    }
    int f = poses ? seg0 : 0;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];                   // what projectPoints reads of the camera matrix
    for (int j = 0; j < kTilesPerBlock; ++j) {
        const long long base = chunk0 + (long long)j * kTile;
        if (base >= count) break;                                              // block-uniform
        const int cnt = (int)min((long long)kTile, count - base);
        tile_load(pts + (point_base + base) * 6, tile2, cnt);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const long long i = base + threadIdx.x;
            float x = tile[6 * threadIdx.x], y = tile[6 * threadIdx.x + 1], z = tile[6 * threadIdx.x + 2];
            if (poses) {
                f = advance_segment(offs, F, f, point_base + i);
                pose_apply(poses + (size_t)f * 16, x, y, z);
            }
            const double X = x, Y = y, Z = z;
            const bool finite = fabs(X) <= kDblMax && fabs(Y) <= kDblMax && fabs(Z) <= kDblMax;
            if (finite && (!has_min_z || Z > min_z)) {
                const double zi = Z != 0.0 ? 1.0 / Z : 1.0;
                const double u = floor((X * zi) * fx + cx), v = floor((Y * zi) * fy + cy);
                if (u >= 0.0 && u < (double)cols && v >= 0.0 && v < (double)rows) {      // false for NaN
                    const float d = (float)sqrt((X * X + Y * Y) + Z * Z);
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(unsigned)i;
                    unsigned long long* cell = zbuf + ((size_t)(int)v * cols + (int)u);
                    if (key < *reinterpret_cast<const volatile unsigned long long*>(cell)) atomicMin(cell, key);
                }
            }
        }
        __syncthreads();
    }
}

// a thread per pixel.  merge: the planes hold the result of earlier launches over lower point indices; the winner of this one
// replaces it only where it is strictly closer
__global__ __launch_bounds__(256) void pcl_resolve_kernel(const float* __restrict__ pts, const unsigned long long* __restrict__ zbuf,
                                                          long long point_base, float* __restrict__ image, float* __restrict__ dist,
                                                          long long* __restrict__ index, int npix, int merge) {
    const int i = blockIdx.x * kMapThreads + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = zbuf[i];
    float* px = image + (size_t)i * 3;
    if (key == kZEmpty) {
        if (!merge) {
            px[0] = px[1] = px[2] = 0.f;
            if (dist) dist[i] = __uint_as_float(0x7f800000u);
            if (index) index[i] = -1;
        }
        return;
    }
    const float d = __uint_as_float((unsigned)(key >> 32));
    if (merge && !(d < dist[i])) return;
    const long long p = point_base + (long long)(key & 0xffffffffull);
    const float* r = pts + p * 6;
    px[0] = r[3]; px[1] = r[4]; px[2] = r[5];
    if (dist) dist[i] = d;
    if (index) index[i] = p;
}

// ---- voxel grid -----------------------------------------------------------------------------------------------------------------
// One row per occupied cell of a grid of voxel_size: key -> stable LSD radix sort of (key, point index) -> heads of the runs of
// equal keys, compacted in order -> one fp64 mean per run.  key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20) with
// i = floor(double(c) / voxel_size) (one IEEE division, one floor); a row with a non-finite value, or with an index outside
// [-2^20, 2^20), gets the key 2^63, which sorts behind every cell, and is counted.
//
// SORT.  Digits of 4 bits, tiles of kVxTile = 1024 keys, thread t owns keys 4 t .. 4 t + 3 of its tile.  A thread's sixteen digit
// counts (<= 4 each) are sixteen 16-bit fields of four 64-bit words, so one inclusive block scan of those four words gives every
// thread its rank inside every digit, and the last thread's result is the tile's histogram: no LDS atomics, and the order inside
// a digit is the order of the keys in the tile (stable).  Per pass: tile histograms [digit][tile], a two-level exclusive scan over
// them, and the scatter, which sorts the tile in LDS first so that each digit leaves as one contiguous run.  A pass whose digit
// is the same in every key is skipped: the key kernel ORs the keys and their complements into two words, a one-thread kernel turns
// them into sixteen (run, source buffer) words ON THE DEVICE, and the kernels of a skipped pass return at once -- the host never
// waits in the middle.  The dropped rows carry digit 0 in every pass but the last, which exists to move them to the end.
//
// REDUCE.  A thread per cell finds the end of its run by galloping, sums up to kVxSerial members itself in sorted order (ascending
// point index: the sort is stable) and hands a longer run to a wave: lane l sums members l, l + 64, ... and the six partials are
// added by wave_sum_f64.  Either way the order is a function of the run alone.  Each member is fetched and posed again with
// pose_apply, so the fused form sees the bits the transform would have written.
constexpr int kVxPer = 4;
constexpr int kVxTile = kMapThreads * kVxPer;
constexpr int kVxPasses = 16;
constexpr int kVxSerial = 32;
constexpr unsigned long long kVxDropped = 1ull << 63;
// 64-bit words at the head of the scratch.  2..5 are what the binding reads back.
enum { kVxOr = 0, kVxOrNot = 1, kVxCells = 2, kVxRange = 3, kVxRan = 4, kVxNDropped = 5, kVxFinal = 6, kVxRun = 8, kVxPlanWords = 24 };

#if !CLSLAM_DEVICE_BUILD
// host build: the emulator's header has the integer atomicAdd only.  The 64-bit OR stands here, beside this file's atomicMin and
// for the same reason: the emulator files stay as they are, and the one kernel that needs the primitive carries its host form.
inline unsigned long long atomicOr(unsigned long long* p, unsigned long long v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
#endif

__device__ __forceinline__ unsigned long long vx_key(const float* v, double vs, unsigned long long& out_of_range) {
    for (int c = 0; c < 6; ++c)
        if (!(fabs((double)v[c]) <= kDblMax)) return kVxDropped;                 // NaN compares false
    const double ix = floor((double)v[0] / vs), iy = floor((double)v[1] / vs), iz = floor((double)v[2] / vs);
    const double lo = -1048576.0, hi = 1048575.0;
    if (!(ix >= lo && ix <= hi && iy >= lo && iy <= hi && iz >= lo && iz <= hi)) {
        out_of_range += 1;
        return kVxDropped;
    }
    return ((unsigned long long)((long long)iz + 1048576) << 42) | ((unsigned long long)((long long)iy + 1048576) << 21) |
           (unsigned long long)((long long)ix + 1048576);
}

// row i of the cloud, posed by its segment's matrix
__device__ __forceinline__ void vx_fetch(const float* __restrict__ pts, const long long* __restrict__ offs,
                                         const double* __restrict__ poses, int F, unsigned i, float* v) {
    const float2* r = reinterpret_cast<const float2*>(pts + (size_t)i * 6);
    const float2 a = r[0], b = r[1], c = r[2];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y;
    if (poses) pose_apply(poses + (size_t)find_segment(offs, F, (long long)i) * 16, v[0], v[1], v[2]);
}

__global__ __launch_bounds__(256) void pcl_voxel_key_kernel(const float* __restrict__ pts, const long long* __restrict__ offs,
                                                            const double* __restrict__ poses, int F, long long M, double vs,
                                                            unsigned long long* __restrict__ key, unsigned* __restrict__ idx,
                                                            unsigned long long* __restrict__ plan) {
    __shared__ float2 tile2[kTile * 3];
    __shared__ int seg0;
    __shared__ unsigned long long red[4][kMapThreads];
    const float* tile = reinterpret_cast<const float*>(tile2);
    const int t = threadIdx.x;
    const long long chunk0 = (long long)blockIdx.x * kMapChunk;
    if (poses) {
        if (t == 0) seg0 = find_segment(offs, F, chunk0);
        __syncthreads();
    }
    int f = poses ? seg0 : 0;
    unsigned long long any = 0, any_not = 0, dropped = 0, range = 0;
    for (int j = 0; j < kTilesPerBlock; ++j) {
        const long long base = chunk0 + (long long)j * kTile;
        if (base >= M) break;                                                  // block-uniform
        const int cnt = (int)min((long long)kTile, M - base);
        tile_load(pts + base * 6, tile2, cnt);
        __syncthreads();
        if (t < cnt) {
            const long long i = base + t;
            float v[6];
            for (int c = 0; c < 6; ++c) v[c] = tile[6 * t + c];
            if (poses) {
                f = advance_segment(offs, F, f, i);
                pose_apply(poses + (size_t)f * 16, v[0], v[1], v[2]);
            }
            const unsigned long long k = vx_key(v, vs, range);
            if (k == kVxDropped) dropped += 1; else { any |= k; any_not |= ~k; }
            key[i] = k;
            idx[i] = (unsigned)i;
        }
        __syncthreads();
    }
    red[0][t] = any; red[1][t] = any_not; red[2][t] = dropped; red[3][t] = range;
    __syncthreads();
    for (int off = kMapThreads / 2; off >= 1; off >>= 1) {
        if (t < off) {
            red[0][t] |= red[0][t + off]; red[1][t] |= red[1][t + off];
            red[2][t] += red[2][t + off]; red[3][t] += red[3][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {                                                               // integer atomics: any order, the same result
        atomicOr(plan + kVxOr, red[0][0]);
        atomicOr(plan + kVxOrNot, red[1][0]);
        if (red[2][0]) atomicAdd(plan + kVxNDropped, red[2][0]);
        if (red[3][0]) atomicAdd(plan + kVxRange, red[3][0]);
    }
}

// one thread: plan[kVxRun + p] = (pass p runs) | (its source buffer) << 1
__global__ void pcl_voxel_plan_kernel(unsigned long long* __restrict__ plan, long long M) {
    const unsigned long long dropped = plan[kVxNDropped];
    const bool some = (unsigned long long)M > dropped;
    const unsigned long long varies = plan[kVxOr] & plan[kVxOrNot];             // a 1 somewhere and a 0 somewhere
    unsigned long long src = 0, ran = 0;
    for (int p = 0; p < kVxPasses; ++p) {
        unsigned long long run = some && ((varies >> (4 * p)) & 15ull) ? 1 : 0;
        if (p == kVxPasses - 1 && some && dropped) run = 1;                     // the dropped rows go behind the cells
        plan[kVxRun + p] = run | (src << 1);
        src ^= run;
        ran += run;
    }
    plan[kVxFinal] = src;
    plan[kVxRan] = ran;
}

// a thread's four keys / four indices as 16-byte groups (the buffers are 16-byte aligned: vx_layout)
struct alignas(16) VxKey2 { unsigned long long a, b; };
struct alignas(16) VxIdx4 { unsigned a, b, c, d; };

// keys base .. base + 3 of K; a full tile (block-uniform) takes two 16-byte loads, the last one tests every key
__device__ __forceinline__ void vx_load_keys(const unsigned long long* __restrict__ K, long long base, long long M, bool full,
                                             unsigned long long* k) {
    if (full) {
        const VxKey2* p = reinterpret_cast<const VxKey2*>(K + base);
        const VxKey2 lo = p[0], hi = p[1];
        k[0] = lo.a; k[1] = lo.b; k[2] = hi.a; k[3] = hi.b;
    } else {
        for (int j = 0; j < kVxPer; ++j) k[j] = base + j < M ? K[base + j] : 0ull;
    }
}

__device__ __forceinline__ void vx_bump(unsigned long long* w, int d) {
    for (int q = 0; q < 4; ++q) w[q] += (unsigned long long)((d >> 2) == q) << (16 * (d & 3));
}
__device__ __forceinline__ unsigned vx_field(const unsigned long long* w, int d) {
    const int q = d >> 2;
    const unsigned long long x = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
    return (unsigned)(x >> (16 * (d & 3))) & 0xffffu;
}

// hist[digit * tiles + tile] = keys of the tile with that digit
__global__ __launch_bounds__(256) void pcl_voxel_hist_kernel(const unsigned long long* __restrict__ key0,
                                                             const unsigned long long* __restrict__ key1,
                                                             const unsigned long long* __restrict__ plan, int pass, long long M,
                                                             unsigned* __restrict__ hist) {
    __shared__ unsigned long long s[4][kMapThreads];
    const unsigned long long ctl = plan[kVxRun + pass];
    if (!(ctl & 1)) return;
    const unsigned long long* K = (ctl >> 1) ? key1 : key0;
    const int t = threadIdx.x;
    const long long tile0 = (long long)blockIdx.x * kVxTile, base = tile0 + kVxPer * t;
    unsigned long long key[kVxPer], c[4] = {0, 0, 0, 0};
    vx_load_keys(K, base, M, tile0 + kVxTile <= M, key);
    for (int k = 0; k < kVxPer; ++k)
        if (base + k < M) vx_bump(c, (int)((key[k] >> (4 * pass)) & 15ull));
    for (int q = 0; q < 4; ++q) s[q][t] = c[q];
    __syncthreads();
    for (int off = kMapThreads / 2; off >= 1; off >>= 1) {
        if (t < off)
            for (int q = 0; q < 4; ++q) s[q][t] += s[q][t + off];                // a field holds at most 1024
        __syncthreads();
    }
    if (t < 16) hist[(size_t)t * gridDim.x + blockIdx.x] = (unsigned)(s[t >> 2][0] >> (16 * (t & 3))) & 0xffffu;
}

// block g: the exclusive scan of entries [1024 g, 1024 g + 1024) in place, their sum to sums[g].  ctl: the pass word, or NULL
__global__ __launch_bounds__(256) void pcl_voxel_scan_kernel(unsigned* __restrict__ v, unsigned* __restrict__ sums, int G,
                                                             const unsigned long long* __restrict__ ctl) {
    __shared__ unsigned s[2][kMapThreads];
    if (ctl && !(*ctl & 1)) return;
    const int t = threadIdx.x, base = blockIdx.x * kVxTile + kVxPer * t;
    unsigned x[kVxPer], own = 0;
    for (int k = 0; k < kVxPer; ++k) { x[k] = base + k < G ? v[base + k] : 0u; own += x[k]; }
    s[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kMapThreads; off <<= 1, cur ^= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= off ? s[cur][t - off] : 0u);
        __syncthreads();
    }
    unsigned run = s[cur][t] - own;
    for (int k = 0; k < kVxPer; ++k)
        if (base + k < G) { v[base + k] = run; run += x[k]; }
    if (t == kMapThreads - 1) sums[blockIdx.x] = s[cur][t];
}

// one block: the exclusive scan of the n sums in place; the grand total to *total if given
__global__ __launch_bounds__(256) void pcl_voxel_scan_sums_kernel(unsigned* __restrict__ sums, int n,
                                                                  const unsigned long long* __restrict__ ctl,
                                                                  unsigned long long* __restrict__ total) {
    __shared__ unsigned s[2][kMapThreads];
    if (ctl && !(*ctl & 1)) return;
    const int t = threadIdx.x;
    const int per = (n + kMapThreads - 1) / kMapThreads;
    const int lo = min(t * per, n), hi = min(lo + per, n);
    unsigned own = 0;
    for (int g = lo; g < hi; ++g) own += sums[g];
    s[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kMapThreads; off <<= 1, cur ^= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= off ? s[cur][t - off] : 0u);
        __syncthreads();
    }
    unsigned run = s[cur][t] - own;
    for (int g = lo; g < hi; ++g) { const unsigned c = sums[g]; sums[g] = run; run += c; }
    if (total && t == kMapThreads - 1) *total = s[cur][t];
}

__global__ __launch_bounds__(256) void pcl_voxel_scatter_kernel(unsigned long long* __restrict__ key0, unsigned long long* __restrict__ key1,
                                                                unsigned* __restrict__ idx0, unsigned* __restrict__ idx1,
                                                                const unsigned long long* __restrict__ plan, int pass, long long M,
                                                                const unsigned* __restrict__ hist, const unsigned* __restrict__ sums) {
    __shared__ unsigned long long skey[kVxTile];
    __shared__ unsigned sidx[kVxTile];
    __shared__ unsigned long long sc[2][4][kMapThreads];
    __shared__ unsigned lstart[16], gbase[16];
    const unsigned long long ctl = plan[kVxRun + pass];
    if (!(ctl & 1)) return;
    const int src = (int)(ctl >> 1), t = threadIdx.x, shift = 4 * pass;
    const unsigned long long* K = src ? key1 : key0;
    const unsigned* I = src ? idx1 : idx0;
    unsigned long long* Kd = src ? key0 : key1;
    unsigned* Id = src ? idx0 : idx1;
    const long long tile0 = (long long)blockIdx.x * kVxTile, base = tile0 + kVxPer * t;
    const int cnt = (int)min((long long)kVxTile, M - tile0);
    unsigned long long k[kVxPer], c[4] = {0, 0, 0, 0};
    unsigned id[kVxPer];
    const bool full = tile0 + kVxTile <= M;                                    // block-uniform
    vx_load_keys(K, base, M, full, k);
    if (full) {
        const VxIdx4 q = *reinterpret_cast<const VxIdx4*>(I + base);
        id[0] = q.a; id[1] = q.b; id[2] = q.c; id[3] = q.d;
    } else {
        for (int j = 0; j < kVxPer; ++j) id[j] = base + j < M ? I[base + j] : 0u;
    }
    for (int j = 0; j < kVxPer; ++j)
        if (base + j < M) vx_bump(c, (int)((k[j] >> shift) & 15ull));
    for (int q = 0; q < 4; ++q) sc[0][q][t] = c[q];
    if (t < 16) {
        const size_t g = (size_t)t * gridDim.x + blockIdx.x;
        gbase[t] = hist[g] + sums[g / kVxTile];
    }
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kMapThreads; off <<= 1, cur ^= 1) {
        for (int q = 0; q < 4; ++q) sc[cur ^ 1][q][t] = sc[cur][q][t] + (t >= off ? sc[cur][q][t - off] : 0ull);
        __syncthreads();
    }
    unsigned long long rank[4];                                                // keys of the threads before this one, per digit
    for (int q = 0; q < 4; ++q) rank[q] = sc[cur][q][t] - c[q];
    if (t == 0) {
        unsigned long long tot[4];
        for (int q = 0; q < 4; ++q) tot[q] = sc[cur][q][kMapThreads - 1];
        unsigned run = 0;
        for (int d = 0; d < 16; ++d) { lstart[d] = run; run += vx_field(tot, d); }
    }
    __syncthreads();
    for (int j = 0; j < kVxPer; ++j)
        if (base + j < M) {
            const int d = (int)((k[j] >> shift) & 15ull);
            const unsigned pos = lstart[d] + vx_field(rank, d);
            vx_bump(rank, d);
            skey[pos] = k[j];
            sidx[pos] = id[j];
        }
    __syncthreads();
    for (int i = t; i < cnt; i += kMapThreads) {
        const unsigned long long kk = skey[i];
        const int d = (int)((kk >> shift) & 15ull);
        const size_t dst = (size_t)gbase[d] + (unsigned)(i - (int)lstart[d]);
        Kd[dst] = kk;
        Id[dst] = sidx[i];
    }
}

// position i of the sorted keys opens a run of at least min_points cells
__device__ __forceinline__ int vx_head(const unsigned long long* __restrict__ K, long long i, long long mv, int min_points) {
    if (i >= mv) return 0;
    const unsigned long long k = K[i];
    if (i > 0 && K[i - 1] == k) return 0;
    const long long e = i + min_points - 1;
    return e < mv && K[e] == k;
}

// scatter == 0: cnt[tile] = heads of the tile.  scatter != 0: cnt holds the scanned counts; start[rank of the head] = its position
__global__ __launch_bounds__(256) void pcl_voxel_heads_kernel(const unsigned long long* __restrict__ key0,
                                                              const unsigned long long* __restrict__ key1, unsigned* __restrict__ idx0,
                                                              unsigned* __restrict__ idx1, const unsigned long long* __restrict__ plan,
                                                              long long M, int min_points, unsigned* __restrict__ cnt,
                                                              const unsigned* __restrict__ sums, int scatter) {
    __shared__ unsigned s[2][kMapThreads];
    const int fin = (int)plan[kVxFinal], t = threadIdx.x;
    const unsigned long long* K = fin ? key1 : key0;
    unsigned* start = fin ? idx0 : idx1;                                        // the index buffer the sort left free
    const long long mv = M - (long long)plan[kVxNDropped];
    const long long base = (long long)blockIdx.x * kVxTile + kVxPer * t;
    int h[kVxPer];
    unsigned own = 0;
    for (int j = 0; j < kVxPer; ++j) { h[j] = vx_head(K, base + j, mv, min_points); own += (unsigned)h[j]; }
    s[0][t] = own;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kMapThreads; off <<= 1, cur ^= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= off ? s[cur][t - off] : 0u);
        __syncthreads();
    }
    if (!scatter) {
        if (t == kMapThreads - 1) cnt[blockIdx.x] = s[cur][t];
        return;
    }
    size_t at = (size_t)cnt[blockIdx.x] + sums[blockIdx.x / kVxTile] + (s[cur][t] - own);
    for (int j = 0; j < kVxPer; ++j)
        if (h[j]) start[at++] = (unsigned)(base + j);
}

// a block per 256 cells: rows[v] = the fp64 mean of the members of cell v, rounded once; counts[v] = their number
__global__ __launch_bounds__(256) void pcl_voxel_reduce_kernel(const float* __restrict__ pts, const long long* __restrict__ offs,
                                                               const double* __restrict__ poses, int F,
                                                               const unsigned long long* __restrict__ key0,
                                                               const unsigned long long* __restrict__ key1,
                                                               const unsigned* __restrict__ idx0, const unsigned* __restrict__ idx1,
                                                               const unsigned long long* __restrict__ plan, long long M, long long V,
                                                               float* __restrict__ rows, int* __restrict__ counts) {
    __shared__ float2 tile2[kTile * 3];
    __shared__ int big[kMapThreads];
    __shared__ long long big_start[kMapThreads], big_n[kMapThreads];
    __shared__ unsigned nbig;
    float* tile = reinterpret_cast<float*>(tile2);
    const int fin = (int)plan[kVxFinal], t = threadIdx.x;
    const unsigned long long* K = fin ? key1 : key0;
    const unsigned* I = fin ? idx1 : idx0;
    const unsigned* start = fin ? idx0 : idx1;
    const long long mv = M - (long long)plan[kVxNDropped];
    const long long v0 = (long long)blockIdx.x * kTile, v = v0 + t;
    if (t == 0) nbig = 0;
    __syncthreads();
    if (v < V) {
        const long long s = start[v];
        const unsigned long long k = K[s];
        long long a = s, step = 1;                                             // K[a] == k; gallop, then bisect
        while (a + step < mv && K[a + step] == k) { a += step; step <<= 1; }
        long long lo = a + 1, hi = min(a + step, mv);
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (K[mid] == k) lo = mid + 1; else hi = mid;
        }
        const long long n = lo - s;
        counts[v] = (int)n;
        if (n <= kVxSerial) {
            double acc[6] = {0, 0, 0, 0, 0, 0};
            for (long long j = 0; j < n; ++j) {
                float p[6];
                vx_fetch(pts, offs, poses, F, I[s + j], p);
                for (int c = 0; c < 6; ++c) acc[c] += (double)p[c];
            }
            for (int c = 0; c < 6; ++c) tile[6 * t + c] = (float)(acc[c] / (double)n);
        } else {
            const unsigned slot = atomicAdd(&nbig, 1u);                        // which slot: irrelevant to the values
            big[slot] = t; big_start[slot] = s; big_n[slot] = n;
        }
    }
    __syncthreads();
    const int lane = lane_id();
    for (unsigned b = (unsigned)t >> 6; b < nbig; b += kMapThreads / kWave) {  // wave-uniform
        const long long s = big_start[b], n = big_n[b];
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (long long j = lane; j < n; j += kWave) {
            float p[6];
            vx_fetch(pts, offs, poses, F, I[s + j], p);
            for (int c = 0; c < 6; ++c) acc[c] += (double)p[c];
        }
        for (int c = 0; c < 6; ++c) acc[c] = wave_sum_f64(acc[c]);
        if (lane == 0)
            for (int c = 0; c < 6; ++c) tile[6 * big[b] + c] = (float)(acc[c] / (double)n);
    }
    __syncthreads();
    tile_store(rows + v0 * 6, tile2, (int)min((long long)kTile, V - v0));
}

}  // namespace clslam

using namespace clslam;

static bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_error("%s failed", what);
    return false;
}

// 8-byte words of scratch for n_images planes of h x w: 64-bit chunk offsets, then the 32-bit chunk counts.  0: out of range.
extern "C" int clslam_pcl_backproject_scratch(int n_images, int h, int w) {
    if (n_images <= 0 || n_images > 65535 || h <= 0 || w <= 0 || (long long)h * w > (1ll << 30)) return 0;
    const long long G = (long long)n_images * cdiv(h * w, kBpChunk);
    return G < (1ll << 30) ? (int)(G + (G + 1) / 2) : 0;
}

extern "C" int clslam_pcl_backproject(const float* depth, const float* inv_k, const float* image, float* points, long long* offsets,
                                      void* scratch, int n_images, int h, int w, float dist_threshold, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n_images >= 0 && offsets, "pcl_backproject: bad arguments");
    if (n_images == 0) {
        if (!hip_ok(hipMemsetAsync(offsets, 0, sizeof(long long), stream), "pcl_backproject: hipMemsetAsync")) return CLSLAM_ERR_INVALID;
        return CLSLAM_OK;
    }
    CLSLAM_REQUIRE(depth && inv_k && image && points && scratch, "pcl_backproject: null pointer");
    CLSLAM_REQUIRE(clslam_pcl_backproject_scratch(n_images, h, w) > 0,
                   "pcl_backproject: bad geometry (1..65535 images, planes of 1..2^30 pixels, fewer than 2^30 chunks)");
    CLSLAM_REQUIRE(dist_threshold == dist_threshold, "pcl_backproject: NaN dist_threshold");
    CLSLAM_REQUIRE(((size_t)points & 7) == 0 && ((size_t)scratch & 7) == 0, "pcl_backproject: points and scratch must be 8-byte aligned");
    const int npx = h * w, chunks = cdiv(npx, kBpChunk), G = n_images * chunks;
    const int keep_all = std::isinf(dist_threshold) ? 1 : 0;                   // np.isinf at utils.py:35
    long long* chunk_off = (long long*)scratch;
    unsigned* counts = (unsigned*)(chunk_off + G);
    const dim3 grid(chunks, n_images), block(kMapThreads);
    hipLaunchKernelGGL(pcl_bp_count_kernel, grid, block, 0, stream, depth, inv_k, counts, npx, w, dist_threshold, keep_all);
    hipLaunchKernelGGL(pcl_bp_scan_kernel, dim3(1), block, 0, stream, (const unsigned*)counts, chunk_off, offsets, G, chunks, n_images);
    hipLaunchKernelGGL(pcl_bp_scatter_kernel, grid, block, 0, stream, depth, inv_k, image, (const long long*)chunk_off, points, npx, w,
                       dist_threshold, keep_all);
    return check_launch("pcl_backproject");
}

extern "C" int clslam_pcl_transform(const float* points, const long long* offsets, const double* poses, float* out, long long m,
                                    int n_segments, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(m >= 0 && m < (1ll << 40), "pcl_transform: bad point count");
    if (m == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(points && offsets && poses && out && n_segments > 0, "pcl_transform: null pointer or no segment");
    CLSLAM_REQUIRE(((size_t)points & 7) == 0 && ((size_t)out & 7) == 0, "pcl_transform: clouds must be 8-byte aligned");
    const long long blocks = (m + kMapChunk - 1) / kMapChunk;
    hipLaunchKernelGGL(pcl_transform_kernel, dim3((unsigned)blocks), dim3(kMapThreads), 0, stream, points, offsets, poses, out, m,
                       n_segments);
    return check_launch("pcl_transform");
}

// 8-byte words of the z-buffer of a rows x cols view.  0: out of range.
extern "C" int clslam_pcl_splat_scratch(int rows, int cols) {
    if (rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 28)) return 0;
    return rows * cols;
}

extern "C" int clslam_pcl_splat(const float* points, const long long* offsets, const double* poses, int n_segments, const double* K,
                                unsigned long long* zbuf, int rows, int cols, long long point_base, long long count, int has_min_z,
                                double min_z, int clear, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(zbuf && K && clslam_pcl_splat_scratch(rows, cols) > 0, "pcl_splat: null pointer or a view beyond 2^28 pixels");
    CLSLAM_REQUIRE(point_base >= 0 && point_base < (1ll << 40) && count >= 0 && count <= (1ll << 32),
                   "pcl_splat: one launch takes at most 2^32 points (the key's index field)");
    CLSLAM_REQUIRE(!has_min_z || min_z == min_z, "pcl_splat: NaN min_z");
    if (clear && !hip_ok(hipMemsetAsync(zbuf, 0xFF, (size_t)rows * cols * sizeof(unsigned long long), stream), "pcl_splat: hipMemsetAsync"))
        return CLSLAM_ERR_INVALID;
    if (count == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(points && ((size_t)points & 7) == 0, "pcl_splat: the cloud must be 8-byte aligned");
    CLSLAM_REQUIRE(!poses || (offsets && n_segments > 0), "pcl_splat: poses need segment offsets");
    const long long blocks = (count + kMapChunk - 1) / kMapChunk;
    hipLaunchKernelGGL(pcl_splat_kernel, dim3((unsigned)blocks), dim3(kMapThreads), 0, stream, points, offsets, poses, n_segments, K, zbuf,
                       rows, cols, point_base, count, has_min_z, min_z);
    return check_launch("pcl_splat");
}

extern "C" int clslam_pcl_resolve(const float* points, const unsigned long long* zbuf, long long point_base, float* image, float* dist,
                                  long long* index, int rows, int cols, int merge, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(zbuf && image && clslam_pcl_splat_scratch(rows, cols) > 0, "pcl_resolve: null pointer or a view beyond 2^28 pixels");
    CLSLAM_REQUIRE(point_base >= 0 && point_base < (1ll << 40), "pcl_resolve: bad point base");
    CLSLAM_REQUIRE(!merge || dist, "pcl_resolve: merging needs the distance plane");
    const int npix = rows * cols;
    hipLaunchKernelGGL(pcl_resolve_kernel, dim3(cdiv(npix, kMapThreads)), dim3(kMapThreads), 0, stream, points, zbuf, point_base, image,
                       dist, index, npix, merge);
    return check_launch("pcl_resolve");
}

// ---- voxel grid: host side ------------------------------------------------------------------------------------------------------
namespace {
struct VxScratch {
    unsigned long long* plan;
    unsigned long long* key[2];
    unsigned* idx[2];
    unsigned* hist;
    unsigned* sums;
    int tiles, n_hist, n_sums;
    size_t words;
};

// plan | two key buffers | two index buffers | [digit][tile] histograms | their 1024-entry sums: 24 bytes and a little per point,
// each buffer padded to a multiple of 16 bytes
VxScratch vx_layout(void* scratch, long long m) {
    VxScratch s;
    unsigned long long* w = (unsigned long long*)scratch;
    s.tiles = (int)((m + kVxTile - 1) / kVxTile);
    s.n_hist = 16 * s.tiles;
    s.n_sums = (s.n_hist + kVxTile - 1) / kVxTile;
    const size_t keys = ((size_t)m + 1) & ~(size_t)1;                          // every buffer starts on 16 bytes
    const size_t half = ((size_t)(m + 1) / 2 + 1) & ~(size_t)1;
    s.plan = w; w += kVxPlanWords;
    s.key[0] = w; w += keys;
    s.key[1] = w; w += keys;
    s.idx[0] = (unsigned*)w; w += half;
    s.idx[1] = (unsigned*)w; w += half;
    s.hist = (unsigned*)w; w += (size_t)(s.n_hist + 1) / 2;
    s.sums = (unsigned*)w; w += (size_t)(s.n_sums + 1) / 2;
    s.words = (size_t)(w - (unsigned long long*)scratch);
    return s;
}
}  // namespace

// 8-byte words of scratch for a cloud of m points.  0: out of range (1 <= m < 2^31).
extern "C" size_t clslam_pcl_voxel_scratch(long long m) {
    if (m <= 0 || m >= (1ll << 31)) return 0;
    return vx_layout(nullptr, m).words;
}

extern "C" int clslam_pcl_voxel_sort(const float* points, const long long* offsets, const double* poses, int n_segments, long long m,
                                     double voxel_size, int min_points, void* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(clslam_pcl_voxel_scratch(m) > 0, "pcl_voxel_sort: one call takes 1 .. 2^31 - 1 points");
    CLSLAM_REQUIRE(points && scratch && ((size_t)points & 7) == 0 && ((size_t)scratch & 15) == 0,
                   "pcl_voxel_sort: null pointer, a cloud that is not 8-byte or a scratch that is not 16-byte aligned");
    CLSLAM_REQUIRE(voxel_size > 0.0 && voxel_size <= kDblMax, "pcl_voxel_sort: voxel_size must be finite and above 0");
    CLSLAM_REQUIRE(min_points >= 1, "pcl_voxel_sort: min_points must be at least 1");
    CLSLAM_REQUIRE(!poses || (offsets && n_segments > 0), "pcl_voxel_sort: poses need segment offsets");
    const VxScratch s = vx_layout(scratch, m);
    if (!hip_ok(hipMemsetAsync(s.plan, 0, kVxPlanWords * sizeof(unsigned long long), stream), "pcl_voxel_sort: hipMemsetAsync"))
        return CLSLAM_ERR_INVALID;
    const dim3 block(kMapThreads), tiles(s.tiles), one(1);
    hipLaunchKernelGGL(pcl_voxel_key_kernel, dim3((unsigned)((m + kMapChunk - 1) / kMapChunk)), block, 0, stream, points, offsets, poses,
                       n_segments, m, voxel_size, s.key[0], s.idx[0], s.plan);
    hipLaunchKernelGGL(pcl_voxel_plan_kernel, one, one, 0, stream, s.plan, m);
    for (int p = 0; p < kVxPasses; ++p) {
        const unsigned long long* ctl = s.plan + kVxRun + p;
        hipLaunchKernelGGL(pcl_voxel_hist_kernel, tiles, block, 0, stream, (const unsigned long long*)s.key[0],
                           (const unsigned long long*)s.key[1], (const unsigned long long*)s.plan, p, m, s.hist);
        hipLaunchKernelGGL(pcl_voxel_scan_kernel, dim3(s.n_sums), block, 0, stream, s.hist, s.sums, s.n_hist, ctl);
        hipLaunchKernelGGL(pcl_voxel_scan_sums_kernel, one, block, 0, stream, s.sums, s.n_sums, ctl, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(pcl_voxel_scatter_kernel, tiles, block, 0, stream, s.key[0], s.key[1], s.idx[0], s.idx[1],
                           (const unsigned long long*)s.plan, p, m, (const unsigned*)s.hist, (const unsigned*)s.sums);
    }
    const int head_sums = (s.tiles + kVxTile - 1) / kVxTile;
    hipLaunchKernelGGL(pcl_voxel_heads_kernel, tiles, block, 0, stream, (const unsigned long long*)s.key[0],
                       (const unsigned long long*)s.key[1], s.idx[0], s.idx[1], (const unsigned long long*)s.plan, m, min_points, s.hist,
                       (const unsigned*)s.sums, 0);
    hipLaunchKernelGGL(pcl_voxel_scan_kernel, dim3(head_sums), block, 0, stream, s.hist, s.sums, s.tiles, (const unsigned long long*)nullptr);
    hipLaunchKernelGGL(pcl_voxel_scan_sums_kernel, one, block, 0, stream, s.sums, head_sums, (const unsigned long long*)nullptr,
                       s.plan + kVxCells);
    hipLaunchKernelGGL(pcl_voxel_heads_kernel, tiles, block, 0, stream, (const unsigned long long*)s.key[0],
                       (const unsigned long long*)s.key[1], s.idx[0], s.idx[1], (const unsigned long long*)s.plan, m, min_points, s.hist,
                       (const unsigned*)s.sums, 1);
    return check_launch("pcl_voxel_sort");
}

extern "C" int clslam_pcl_voxel_reduce(const float* points, const long long* offsets, const double* poses, int n_segments, long long m,
                                       const void* scratch, float* rows, int* counts, long long n_cells, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(clslam_pcl_voxel_scratch(m) > 0 && n_cells >= 0 && n_cells <= m, "pcl_voxel_reduce: bad point or cell count");
    if (n_cells == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(points && scratch && rows && counts && ((size_t)points & 7) == 0 && ((size_t)rows & 7) == 0,
                   "pcl_voxel_reduce: null pointer, or a cloud that is not 8-byte aligned");
    CLSLAM_REQUIRE(!poses || (offsets && n_segments > 0), "pcl_voxel_reduce: poses need segment offsets");
    const VxScratch s = vx_layout(const_cast<void*>(scratch), m);
    hipLaunchKernelGGL(pcl_voxel_reduce_kernel, dim3((unsigned)((n_cells + kTile - 1) / kTile)), dim3(kMapThreads), 0, stream, points,
                       offsets, poses, n_segments, (const unsigned long long*)s.key[0], (const unsigned long long*)s.key[1],
                       (const unsigned*)s.idx[0], (const unsigned*)s.idx[1], (const unsigned long long*)s.plan, m, n_cells, rows, counts);
    return check_launch("pcl_voxel_reduce");
}
