// Trajectory and pose-error metrics on the device (slam/utils.py:129-383: scale_optimization, trajectory_distances,
// last_frame_from_segment_length, rotation_error, translation_error, calc_sequence_errors, compute_overall_err, compute_ATE,
// compute_RPE, calc_error; the per-frame relative pose error of slam.py:257-259 and the pair error of dpp.py:505-511).
// Everything is double; poses are (n,4,4) row-major fp64.
//
// Launch sequence of clslam_traj_metrics (all on the caller's stream, nothing allocated, no host synchronisation):
//   terms (one thread per pose: step length, ATE term, RPE pair error of (i, i+1); per-block partial sums) | scale leaves |
//   scale tree (the two sums of the scale, below) | scan totals (only beyond one scan block) | scan (step lengths -> dist, in
//   place) | segments (one thread per (first frame, length): binary search for the last frame, three inverses, two errors) |
//   finalize (one block).
//
// INVERSE.  A general 4x4 inverse, LU with partial pivoting on [A | I] and back substitution, one matrix per thread: the
// reference calls np.linalg.inv on poses whose rotation block is not orthonormal (fp32 composition, rescaled translations), so
// the rigid shortcut [R^T, -R^T t] would compute something else.  Every loop is unrolled and a row exchange is four conditional
// swaps per candidate row, so the matrices are indexed by constants only and stay in registers (a runtime row index would put
// them in scratch memory).  A singular matrix gives non-finite results (the reference raises LinAlgError).
//
// DIST.  The prefix sum of the step lengths is hierarchical and every level is SERIAL in index order: a thread adds its four
// consecutive steps, thread 0 adds the 256 thread sums of the block, thread 0 adds the totals of the blocks before its own.
// dist[i] = block offset + (thread offset + prefix inside the thread), and the offset of the next thread / block is the very sum
// that ends the previous one: dist is non-decreasing by construction (rounding is monotone), so the binary search of the
// segment kernel finds the frame the reference's linear scan finds.  At most 4 + 256 + blocks roundings per element.
//
// SUMS.  One term per thread, wave butterfly (wave_sum_f64), the four waves in order, one partial per block; the finalising
// block adds the partials thread-strided in index order and reduces the same way.  No floating-point atomics anywhere: two
// launches agree bitwise.
//
// SCALE.  calc_error prints the scaling factor with all its digits (utils.py:362), so sum(X * Y) and sum(X ** 2) over the
// flattened (n,3) translations are added in the order np.sum adds a contiguous array.  numpy hands its add loop the array in
// pieces of its buffer size, 8192 elements, and adds the sums of the pieces to the result one after the other, in order; only
// INSIDE a piece is the summation pairwise -- a range of more than 128 elements is split at half its length rounded down to a
// multiple of 8, a leaf of 8..128 elements runs eight interleaved accumulators, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
// (r6 + r7)), then the remainder one by one; fewer than 8 elements are added one by one.  Every piece and every leaf starts at a
// multiple of 8: thread t of the leaf kernel descends the tree of its piece to the leaf that holds element 8t and adds it if it
// starts there; one thread then walks the tree of each piece over the leaf sums with a stack in LDS and adds the pieces up.
// The products are rounded on their own (no fma), as numpy's are.
#include "common.h"

namespace clslam {

constexpr int kTeThreads = 256;
constexpr int kTePerThread = 4;                             // consecutive steps per thread in the scan
constexpr int kTeChunk = kTeThreads * kTePerThread;         // steps per scan block
constexpr int kTeSums = 3;                                  // ATE term, RPE translation, RPE rotation
constexpr int kTeLeaf = 128;                               // numpy's PW_BLOCKSIZE
constexpr int kTePiece = 8192;                              // numpy's default buffer size: one pairwise tree per piece
constexpr int kTeStack = 64;                                // nodes of a summation tree in flight (depth <= 7 for a piece)
constexpr int kTeSegCols = 6;                               // [first_frame, rot/length, trans/length, length, speed, last_frame]
constexpr int kTeHeader = 8;                                // front of the scratch: [sum X.Y, sum X.X, scaling], the rest reserved

struct M4 {
    double m[4][4];
};

__device__ __forceinline__ M4 load_pose(const double* __restrict__ p) {
    M4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r.m[i][j] = p[i * 4 + j];
    return r;
}

__device__ __forceinline__ void swap_if(bool c, double& x, double& y) {
    const double t = c ? y : x;
    y = c ? x : y;
    x = t;
}

__device__ __forceinline__ M4 inv4(M4 a) {
    M4 b;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) b.m[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int p = k;                                              // the first row with the largest |a[r][k]|, r >= k
        double best = fabs(a.m[k][k]);
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
            const double v = fabs(a.m[r][k]);
            if (v > best) { best = v; p = r; }
        }
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
            const bool c = p == r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                swap_if(c, a.m[k][j], a.m[r][j]);
                swap_if(c, b.m[k][j], b.m[r][j]);
            }
        }
        const double piv = a.m[k][k];
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
            const double f = a.m[r][k] / piv;
#pragma unroll
            for (int j = k + 1; j < 4; ++j) a.m[r][j] -= f * a.m[k][j];
#pragma unroll
            for (int j = 0; j < 4; ++j) b.m[r][j] -= f * b.m[k][j];
        }
    }
#pragma unroll
    for (int k = 3; k >= 0; --k)                                // U x = b, column by column
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = b.m[k][j];
#pragma unroll
            for (int c = k + 1; c < 4; ++c) s -= a.m[k][c] * b.m[c][j];
            b.m[k][j] = s / a.m[k][k];
        }
    return b;
}

__device__ __forceinline__ double dot4(const M4& a, const M4& b, int i, int j) {
    return ((a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j]) + a.m[i][2] * b.m[2][j]) + a.m[i][3] * b.m[3][j];
}

__device__ __forceinline__ M4 mul4(const M4& a, const M4& b) {
    M4 c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c.m[i][j] = dot4(a, b, i, j);
    return c;
}

// translation_error and rotation_error (utils.py:191-217) of a @ b: only the diagonal of the rotation block and column 3 of the
// product are formed.  The clamp keeps a NaN (Python's max(min(d, 1.0), -1.0) does).
__device__ __forceinline__ void product_errors(const M4& a, const M4& b, double& trans, double& rot) {
    const double dx = dot4(a, b, 0, 3), dy = dot4(a, b, 1, 3), dz = dot4(a, b, 2, 3);
    trans = sqrt((dx * dx + dy * dy) + dz * dz);
    double d = 0.5 * (((dot4(a, b, 0, 0) + dot4(a, b, 1, 1)) + dot4(a, b, 2, 2)) - 1.0);
    d = d > 1.0 ? 1.0 : d;
    d = d < -1.0 ? -1.0 : d;
    rot = acos(d);
}

// v[k] <- the block's sum of v[k], in every thread; all 256 threads call it
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double (*red)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum_f64(v[k]);
        if (lane_id() == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// ---- per-pose terms: grid ceil(n / 256) ---------------------------------------------------------------------------------------
// step[i] = |gt_xyz[i] - gt_xyz[i-1]| (utils.py:170; 0 for i = 0), pairs[i] = [trans, rot] of inv(gt_rel) @ pred_rel for the
// pair (i, i+1) (utils.py:339-351; zeros for i = n-1), partial[block][3]
__global__ __launch_bounds__(256) void traj_terms_kernel(const double* __restrict__ pred, const double* __restrict__ gt, int n,
                                                         double* __restrict__ step, double* __restrict__ pairs,
                                                         double* __restrict__ partial) {
    __shared__ double red[4][kTeSums];
    const int i = blockIdx.x * kTeThreads + threadIdx.x;
    double v[kTeSums] = {0, 0, 0};
    if (i < n) {
        const double* g = gt + (size_t)i * 16;
        const double* p = pred + (size_t)i * 16;
        const double gx = g[3], gy = g[7], gz = g[11], px = p[3], py = p[7], pz = p[11];
        double st = 0.0;
        if (i > 0) {
            const double dx = gx - g[3 - 16], dy = gy - g[7 - 16], dz = gz - g[11 - 16];
            st = sqrt((dx * dx + dy * dy) + dz * dz);
        }
        step[i] = st;
        const double ex = gx - px, ey = gy - py, ez = gz - pz;
        v[0] = (ex * ex + ey * ey) + ez * ez;                                       // utils.py:322-326
        double tr = 0.0, ro = 0.0;
        if (i + 1 < n) {
            const M4 gt_rel = mul4(inv4(load_pose(g)), load_pose(g + 16));
            const M4 pred_rel = mul4(inv4(load_pose(p)), load_pose(p + 16));
            product_errors(inv4(gt_rel), pred_rel, tr, ro);
        }
        pairs[2 * (size_t)i] = tr;
        pairs[2 * (size_t)i + 1] = ro;
        v[1] = tr;
        v[2] = ro;
    }
    block_sums<kTeSums>(v, red);
    if (threadIdx.x < kTeSums) partial[(size_t)blockIdx.x * kTeSums + threadIdx.x] = v[threadIdx.x];
}

// ---- the scale sums in numpy's order: grid ceil(ceil(3n / 8) / 256), then one block ----------------------------------------------
// element e of the flattened (n,3) translations: X * Y and X * X, each rounded on its own
__device__ __forceinline__ void scale_products(const double* __restrict__ pred, const double* __restrict__ gt, int e, double& xy,
                                               double& xx) {
#pragma clang fp contract(off)
    const int i = e / 3, c = e - 3 * i;
    const double x = pred[(size_t)i * 16 + 3 + 4 * c], y = gt[(size_t)i * 16 + 3 + 4 * c];
    xy = x * y;
    xx = x * x;
}

// one step down the summation tree from the node [o, o + n), n > kTeLeaf: the size of its left child
__device__ __forceinline__ int pairwise_left(int n) {
    const int h = n / 2;
    return h - h % 8;
}

// leaf[t] = [sum X.Y, sum X.X] of the leaf that starts at element 8t (other entries are not written)
__global__ __launch_bounds__(256) void traj_scale_leaves_kernel(const double* __restrict__ pred, const double* __restrict__ gt, int L,
                                                                double* __restrict__ leaf) {
    const int t = blockIdx.x * kTeThreads + threadIdx.x;
    const int e = 8 * t;
    if (e >= L) return;
    int o = e - e % kTePiece, n = min(kTePiece, L - o);                                 // the piece that holds element e
    while (n > kTeLeaf) {
        const int n2 = pairwise_left(n);
        if (e < o + n2) n = n2; else { o += n2; n -= n2; }
    }
    if (o != e) return;
    double sxy = 0.0, sxx = 0.0, a, b;
    int i = 0;
    if (n >= 8) {
        double r[8], q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) scale_products(pred, gt, o + j, r[j], q[j]);
        for (i = 8; i < n - n % 8; i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                scale_products(pred, gt, o + i + j, a, b);
                r[j] += a;
                q[j] += b;
            }
        sxy = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        sxx = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    for (; i < n; ++i) {
        scale_products(pred, gt, o + i, a, b);
        sxy += a;
        sxx += b;
    }
    leaf[2 * (size_t)t] = sxy;
    leaf[2 * (size_t)t + 1] = sxx;
}

// header = [sum X.Y, sum X.X, scaling]: one thread walks the tree of each piece, left child first, a node's sum = left + right,
// and adds the sums of the pieces to 0 in order (np.add.reduce starts from the identity)
__global__ __launch_bounds__(64) void traj_scale_tree_kernel(const double* __restrict__ leaf, int L, double* __restrict__ header) {
    __shared__ int node_o[kTeStack], node_n[kTeStack], node_seen[kTeStack];
    __shared__ double val_xy[kTeStack], val_xx[kTeStack];
    if (threadIdx.x != 0) return;
    double sxy = 0.0, sxx = 0.0;
    for (int piece = 0; piece < L; piece += kTePiece) {
        int sp = 1, vp = 0;
        node_o[0] = piece; node_n[0] = min(kTePiece, L - piece); node_seen[0] = 0;
        while (sp > 0) {
            const int o = node_o[sp - 1], n = node_n[sp - 1];
            if (n <= kTeLeaf) {
                val_xy[vp] = leaf[2 * (size_t)(o / 8)];
                val_xx[vp] = leaf[2 * (size_t)(o / 8) + 1];
                ++vp;
                --sp;
            } else if (!node_seen[sp - 1]) {
                node_seen[sp - 1] = 1;
                const int n2 = pairwise_left(n);
                node_o[sp] = o + n2; node_n[sp] = n - n2; node_seen[sp] = 0;                // the right child waits below the left one
                node_o[sp + 1] = o; node_n[sp + 1] = n2; node_seen[sp + 1] = 0;
                sp += 2;
            } else {
                val_xy[vp - 2] = val_xy[vp - 2] + val_xy[vp - 1];
                val_xx[vp - 2] = val_xx[vp - 2] + val_xx[vp - 1];
                --vp;
                --sp;
            }
        }
        sxy += val_xy[0];
        sxx += val_xx[0];
    }
    header[0] = sxy;
    header[1] = sxx;
    header[2] = sxy / sxx;                                                              // utils.py:160
}

// ---- prefix sum of the steps: grid ceil(n / 1024) -----------------------------------------------------------------------------
// p[j]: the serial prefix inside the thread; returns the thread's offset inside the block; lds[256] = the block's total
__device__ __forceinline__ double chunk_prefix(const double* step, int n, double (&p)[kTePerThread], double* lds /* [257] */) {
    const int t = threadIdx.x;
    const int base = blockIdx.x * kTeChunk + t * kTePerThread;
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < kTePerThread; ++j) {
        run += base + j < n ? step[base + j] : 0.0;
        p[j] = run;
    }
    lds[t] = run;
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        for (int k = 0; k < kTeThreads; ++k) {
            const double s = lds[k];
            lds[k] = acc;
            acc += s;
        }
        lds[kTeThreads] = acc;
    }
    __syncthreads();
    return lds[t];
}

__global__ __launch_bounds__(256) void traj_scan_totals_kernel(const double* __restrict__ step, int n, double* __restrict__ totals) {
    __shared__ double lds[kTeThreads + 1];
    double p[kTePerThread];
    chunk_prefix(step, n, p, lds);
    if (threadIdx.x == 0) totals[blockIdx.x] = lds[kTeThreads];
}

// dist holds the steps on entry (a thread reads its own four elements before it writes them)
__global__ __launch_bounds__(256) void traj_scan_kernel(double* dist, int n, const double* __restrict__ totals) {
    __shared__ double lds[kTeThreads + 1];
    __shared__ double block_offset;
    double p[kTePerThread];
    const double mine = chunk_prefix(dist, n, p, lds);
    if (threadIdx.x == 0) {
        double off = 0.0;
        for (int b = 0; b < (int)blockIdx.x; ++b) off += totals[b];
        block_offset = off;
    }
    __syncthreads();
    const double off = block_offset;
    const int base = blockIdx.x * kTeChunk + threadIdx.x * kTePerThread;
#pragma unroll
    for (int j = 0; j < kTePerThread; ++j)
        if (base + j < n) dist[base + j] = off + (mine + p[j]);
}

// ---- segments: one thread per (first frame, length), grid ceil(nseg / 256) (utils.py:220-250) ----------------------------------
__global__ __launch_bounds__(256) void traj_segments_kernel(const double* __restrict__ pred, const double* __restrict__ gt, int n,
                                                            const double* __restrict__ dist, const double* __restrict__ header,
                                                            int optimize_scale, double* __restrict__ seg, int nseg) {
    const double scale = header[2];
    const int k = blockIdx.x * kTeThreads + threadIdx.x;
    if (k >= nseg) return;
    const int first = (k >> 3) * 10;                                                    // step_size 10, eight lengths
    const double length = 100.0 * (double)((k & 7) + 1);
    const double limit = dist[first] + length;
    int lo = first + 1, hi = n;                                                         // first i with dist[i] > limit (utils.py:185-188)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (dist[mid] > limit) hi = mid; else lo = mid + 1;
    }
    double* row = seg + (size_t)k * kTeSegCols;
    row[0] = (double)first;
    row[3] = length;
    if (lo >= n) {                                                                      // the sequence is not long enough
        const double nan = __builtin_nan("");
        row[1] = nan; row[2] = nan; row[4] = nan; row[5] = -1.0;
        return;
    }
    const int last = lo;
    M4 pf = load_pose(pred + (size_t)first * 16), pl = load_pose(pred + (size_t)last * 16);
    if (optimize_scale) {                                                               // utils.py:144-145: translations only
#pragma unroll
        for (int r = 0; r < 3; ++r) { pf.m[r][3] *= scale; pl.m[r][3] *= scale; }
    }
    const M4 delta_gt = mul4(inv4(load_pose(gt + (size_t)first * 16)), load_pose(gt + (size_t)last * 16));
    const M4 delta_pred = mul4(inv4(pf), pl);
    double tr, ro;
    product_errors(inv4(delta_pred), delta_gt, tr, ro);
    row[1] = ro / length;
    row[2] = tr / length;
    row[4] = length / (0.1 * (double)(last - first + 1));                               // 10 fps assumed (utils.py:246-247)
    row[5] = (double)last;
}

// ---- one block: out = [ave_t_err, ave_r_err, n_segments, ate, rpe_trans, rpe_rot, scaling, path_length] -------------------------
__global__ __launch_bounds__(256) void traj_finalize_kernel(const double* __restrict__ header, const double* __restrict__ partial,
                                                            int nblk, const double* __restrict__ seg, int nseg,
                                                            const double* __restrict__ dist, int n, double* __restrict__ out) {
    __shared__ double red[4][kTeSums + 3];
    double v[kTeSums + 3] = {0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblk; b += kTeThreads)
#pragma unroll
        for (int k = 0; k < kTeSums; ++k) v[k] += partial[(size_t)b * kTeSums + k];
    for (int s = threadIdx.x; s < nseg; s += kTeThreads) {
        const double* row = seg + (size_t)s * kTeSegCols;
        if (row[5] >= 0.0) {
            v[kTeSums] += row[2];
            v[kTeSums + 1] += row[1];
            v[kTeSums + 2] += 1.0;
        }
    }
    block_sums<kTeSums + 3>(v, red);
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        const double cnt = v[kTeSums + 2];
        out[0] = cnt > 0.0 ? v[kTeSums] / cnt : 0.0;                                    // utils.py:307-314
        out[1] = cnt > 0.0 ? v[kTeSums + 1] / cnt : 0.0;
        out[2] = cnt;
        out[3] = sqrt(v[0] / (double)n);                                                // utils.py:327 (NaN without a pose)
        out[4] = n > 1 ? v[1] / (double)(n - 1) : nan;                                  // np.mean of an empty list
        out[5] = n > 1 ? v[2] / (double)(n - 1) : nan;
        out[6] = n > 0 ? header[2] : nan;
        out[7] = n > 0 ? dist[n - 1] : 0.0;
    }
}

// ---- pair errors: out[i] = [trans, rot] of inv(b_i) @ (a_inverted ? inv(a_i) : a_i) ------------------------------------------
__global__ __launch_bounds__(256) void pose_pair_error_kernel(const double* __restrict__ a, const double* __restrict__ b, int n,
                                                              int a_inverted, double* __restrict__ out) {
    const int i = blockIdx.x * kTeThreads + threadIdx.x;
    if (i >= n) return;
    M4 A = load_pose(a + (size_t)i * 16);
    if (a_inverted) A = inv4(A);
    double tr, ro;
    product_errors(inv4(load_pose(b + (size_t)i * 16)), A, tr, ro);
    out[2 * (size_t)i] = tr;
    out[2 * (size_t)i + 1] = ro;
}

inline int te_segments(int n) { return cdiv(n, 10) * 8; }

}  // namespace clslam

using namespace clslam;

extern "C" int clslam_pose_pair_error(const double* a, const double* b, int n, int a_inverted, double* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n >= 0, "pose_pair_error: negative n");
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(a && b && out, "pose_pair_error: null pointer");
    hipLaunchKernelGGL(pose_pair_error_kernel, dim3(cdiv(n, kTeThreads)), dim3(kTeThreads), 0, stream, a, b, n, a_inverted ? 1 : 0, out);
    return check_launch("pose_pair_error");
}

// doubles of scratch for n poses: header, pair errors, block partials, scan totals, the leaf sums of the scale (two per eight
// elements of the (n,3) translations), and room for dist and the segment rows where the caller passes none.  0: n out of range.
extern "C" int clslam_traj_metrics_scratch(int n) {
    if (n < 0 || n > CLSLAM_TRAJ_MAX_POSES) return 0;
    return kTeHeader + 2 * n + kTeSums * cdiv(n, kTeThreads) + cdiv(n, kTeChunk) + 2 * cdiv(3 * n, 8) + n + kTeSegCols * te_segments(n);
}

extern "C" int clslam_traj_metrics(const double* pred, const double* gt, int n, int optimize_scale, double* out, double* segments,
                                   double* dist, double* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n >= 0 && n <= CLSLAM_TRAJ_MAX_POSES, "traj_metrics: n must be 0..%d poses, got %d", CLSLAM_TRAJ_MAX_POSES, n);
    CLSLAM_REQUIRE(out && scratch && (n == 0 || (pred && gt)), "traj_metrics: null pointer");
    CLSLAM_REQUIRE(((size_t)scratch & 7) == 0, "traj_metrics: scratch must be 8-byte aligned");
    const int nblk = cdiv(n, kTeThreads), nscan = cdiv(n, kTeChunk), nseg = te_segments(n);
    double* pairs = scratch + kTeHeader;
    double* partial = pairs + 2 * (size_t)n;
    double* totals = partial + (size_t)kTeSums * nblk;
    double* leaf = totals + nscan;
    double* own = leaf + 2 * (size_t)cdiv(3 * n, 8);
    if (!dist) { dist = own; own += n; }
    if (!segments) segments = own;
    const dim3 block(kTeThreads);
    if (n > 0) {
        hipLaunchKernelGGL(traj_terms_kernel, dim3(nblk), block, 0, stream, pred, gt, n, dist, pairs, partial);
        hipLaunchKernelGGL(traj_scale_leaves_kernel, dim3(cdiv(cdiv(3 * n, 8), kTeThreads)), block, 0, stream, pred, gt, 3 * n, leaf);
        hipLaunchKernelGGL(traj_scale_tree_kernel, dim3(1), dim3(64), 0, stream, (const double*)leaf, 3 * n, scratch);
        if (nscan > 1) hipLaunchKernelGGL(traj_scan_totals_kernel, dim3(nscan), block, 0, stream, (const double*)dist, n, totals);
        hipLaunchKernelGGL(traj_scan_kernel, dim3(nscan), block, 0, stream, dist, n, (const double*)totals);
        hipLaunchKernelGGL(traj_segments_kernel, dim3(cdiv(nseg, kTeThreads)), block, 0, stream, pred, gt, n, (const double*)dist,
                           (const double*)scratch, optimize_scale ? 1 : 0, segments, nseg);
    }
    hipLaunchKernelGGL(traj_finalize_kernel, dim3(1), block, 0, stream, (const double*)scratch, (const double*)partial, nblk, (const double*)segments, nseg,
                       (const double*)dist, n, out);
    return check_launch("traj_metrics");
}
