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
