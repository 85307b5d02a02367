// RobotCar raw frames on the device (datasets/robotcar.py:522-548 _load_image, :617-642 CameraModel.undistort): a Bayer mosaic
// becomes RGB by colour_demosaicing.demosaicing_CFA_Bayer_bilinear, and an image is resampled through the camera model's look-up
// table by scipy.ndimage.map_coordinates(order=1).  Three entry points: the two stages on their own, in the libraries' float64,
// and the two fused for uint8 frames (the path a frame takes into the ring), which never writes the float64 image.
//
// DEMOSAIC.  R = conv(CFA * R_m, H_RB), G = conv(CFA * G_m, H_G), B = conv(CFA * B_m, H_RB) with H_G = [[0,1,0],[1,4,1],[0,1,0]] / 4
// and H_RB = [[1,2,1],[2,4,2],[1,2,1]] / 4.  Every product and every partial sum is a multiple of 1/4 far below 2^53, so the sum is
// formed in integers and scaled once: the same double whatever order the library adds in.  The BORDER is scipy.ndimage.convolve's
// default mode, 'reflect' (d c b a | a b c d), applied to the masked planes: a tap outside the image reads the mirrored pixel WITH
// THE MIRRORED PIXEL'S COLOUR.  That rule is restated from the library's documentation, the library was not at hand to compare
// against; it lives in bayer_reflect() alone.  Pixels one step inside the border do not depend on it.  Under it the outermost ring
// can exceed 255 (a mirrored tap doubles a weight), which is kept.
//
// UNDISTORT.  lut (2,H,W) float64 = the (row, col) source coordinate of every output pixel.  A sample is inside iff 0 <= r <= H-1
// and 0 <= c <= W-1, anything else (NaN too) gives 0 (mode='constant', cval=0).  r0 = floor(r), sy = 1 - (r - r0), ty = 1 - sy -- the
// library forms the last weight as one minus the others, which is NOT always r - r0 again -- the second tap is clamped to H-1 (its
// weight is then 0), likewise for c, and
//     t = 0;  t += (v00 * sy) * sx;  t += (v01 * sy) * tx;  t += (v10 * ty) * sx;  t += (v11 * ty) * tx
// in exactly this grouping and order, every operation rounded on its own: scipy's result to the last bit (contraction is off for
// this file; v * (wy * wx) is another number).  uint8 output is (long long)t & 255: truncation toward zero, then the low byte.
//
// LAUNCH SHAPE.  Blocks are runs of kRcThreads consecutive outputs of the flattened image, so every load of the table and every
// store is a contiguous run per wave.  The stand-alone kernels take one thread per output ELEMENT (pixel x channel): the stores of
// 24-byte or 3-byte pixels are then unit-stride, and the table words a pixel's channels share come from one cache line.  The table
// is 16 bytes per pixel, more than a uint8 frame reads and writes together, so undistort and the fused kernel loop over the N
// frames of a launch INSIDE the thread: coordinates and weights are read and formed once per pixel, not once per frame.
//
// FUSED.  One thread per pixel.  The four taps' 3x3 neighbourhoods overlap in a 4x4 patch of the mosaic: 16 byte loads, the four
// demosaiced taps formed in registers by the stand-alone kernel's function, then the expression above.  A tap clamped at the far
// edge has weight 0; the patch then holds another (finite) neighbourhood for it, which the product with 0 erases -- the output is
// byte for byte the composition of the two stand-alone kernels.  The block's 3 * 256 output bytes are collected in LDS and
// stored as dwords when the run starts on a 4-byte boundary (always, when H * W is a multiple of 4), else byte by byte; two LDS
// buffers alternate, so a frame costs one barrier.
#include "common.h"

#pragma clang fp contract(off)

namespace clslam {

constexpr int kRcThreads = 256;

// sites: the channel (0 R, 1 G, 2 B) of the mosaic sites (0,0), (0,1), (1,0), (1,1), two bits each (bayer_sites(), host side)
__device__ __forceinline__ int bayer_channel(int sites, int y, int x) { return (sites >> (2 * ((y & 1) * 2 + (x & 1)))) & 3; }

// THE border rule: scipy.ndimage 'reflect' for an overhang of one, -1 -> 0 and n -> n - 1 (restated, not compared: see the header;
// at this overhang 'nearest' is the same rule, 'mirror' is not)
__device__ __forceinline__ int bayer_reflect(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the demosaiced pixel whose 3x3 neighbourhood is v[A..A+2][B..B+2] (bytes) with channels ch[..][..]
template <int A, int B>
__device__ __forceinline__ void bayer_bilinear(const int (&v)[4][4], const int (&ch)[4][4], double (&rgb)[3]) {
    constexpr int kG[3][3] = {{0, 1, 0}, {1, 4, 1}, {0, 1, 0}};
    constexpr int kRB[3][3] = {{1, 2, 1}, {2, 4, 2}, {1, 2, 1}};
    int r = 0, g = 0, b = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = ch[A + i][B + j], x = v[A + i][B + j];
            r += c == 0 ? kRB[i][j] * x : 0;
            g += c == 1 ? kG[i][j] * x : 0;
            b += c == 2 ? kRB[i][j] * x : 0;
        }
    }
    rgb[0] = (double)r * 0.25;
    rgb[1] = (double)g * 0.25;
    rgb[2] = (double)b * 0.25;
}

// rows[0..2] / cols[0..2]: the neighbourhood of (y, x); a fourth entry, where wanted, is the caller's
__device__ __forceinline__ void bayer_patch(const unsigned char* __restrict__ cfa, int W, int sites, const int (&rows)[4],
                                            const int (&cols)[4], int nr, int nc, int (&v)[4][4], int (&ch)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i < nr && j < nc;
            v[i][j] = in ? (int)cfa[(size_t)rows[i] * W + cols[j]] : 0;
            ch[i][j] = in ? bayer_channel(sites, rows[i], cols[j]) : 3;
        }
    }
}

// grid (blocks of HW * 3 elements, frames): out (N,H,W,3) float64
__global__ __launch_bounds__(256) void demosaic_bilinear_kernel(const unsigned char* __restrict__ cfa, double* __restrict__ out, int H,
                                                                int W, int sites) {
    const int npx = H * W;
    const int e = blockIdx.x * kRcThreads + threadIdx.x;
    if (e >= npx * 3) return;
    const int p = e / 3, c = e - p * 3, y = p / W, x = p - y * W;
    const int rows[4] = {bayer_reflect(y - 1, H), y, bayer_reflect(y + 1, H), 0};
    const int cols[4] = {bayer_reflect(x - 1, W), x, bayer_reflect(x + 1, W), 0};
    int v[4][4], ch[4][4];
    bayer_patch(cfa + (size_t)blockIdx.y * npx, W, sites, rows, cols, 3, 3, v, ch);
    double rgb[3];
    bayer_bilinear<0, 0>(v, ch, rgb);
    out[(size_t)blockIdx.y * npx * 3 + e] = c == 0 ? rgb[0] : (c == 1 ? rgb[1] : rgb[2]);
}

// where an output pixel samples: the four taps' rows and columns and their weights; inside = 0: the result is 0
struct LutTap {
    int r0, r1, c0, c1, inside;
    double sy, ty, sx, tx;
};

__device__ __forceinline__ LutTap lut_tap(const double* __restrict__ lut, int npx, int p, int H, int W) {
    const double r = lut[p], c = lut[(size_t)npx + p];
    LutTap t;
    t.inside = r >= 0.0 && r <= (double)(H - 1) && c >= 0.0 && c <= (double)(W - 1);
    const double fr = t.inside ? floor(r) : 0.0, fc = t.inside ? floor(c) : 0.0;
    t.r0 = (int)fr;
    t.c0 = (int)fc;
    t.r1 = min(t.r0 + 1, H - 1);
    t.c1 = min(t.c0 + 1, W - 1);
    t.sy = 1.0 - (r - fr);
    t.sx = 1.0 - (c - fc);
    t.ty = 1.0 - t.sy;                       // "all weights add to unity": not r - fr in every case
    t.tx = 1.0 - t.sx;
    return t;
}

// map_coordinates(order=1)'s sum, in its grouping and order
__device__ __forceinline__ double lut_blend(const LutTap& t, double v00, double v01, double v10, double v11) {
    double s = 0.0;
    s += (v00 * t.sy) * t.sx;
    s += (v01 * t.sy) * t.tx;
    s += (v10 * t.ty) * t.sx;
    s += (v11 * t.ty) * t.tx;
    return s;
}

__device__ __forceinline__ unsigned char lut_to_u8(double s) { return (unsigned char)((long long)s & 255); }

__device__ __forceinline__ void lut_store(unsigned char* o, double s) { *o = lut_to_u8(s); }
__device__ __forceinline__ void lut_store(double* o, double s) { *o = s; }

// grid (blocks of HW * C elements): image, out (N,H,W,C) of T; every frame through the one table
template <typename T>
__global__ __launch_bounds__(256) void undistort_lut_kernel(const T* __restrict__ image, const double* __restrict__ lut,
                                                            T* __restrict__ out, int N, int H, int W, int C) {
    const int npx = H * W;
    const int e = blockIdx.x * kRcThreads + threadIdx.x;
    if (e >= npx * C) return;
    const int p = e / C, c = e - p * C;
    const LutTap t = lut_tap(lut, npx, p, H, W);
    const size_t frame = (size_t)npx * C;
    const size_t i00 = ((size_t)t.r0 * W + t.c0) * C + c, i01 = ((size_t)t.r0 * W + t.c1) * C + c;
    const size_t i10 = ((size_t)t.r1 * W + t.c0) * C + c, i11 = ((size_t)t.r1 * W + t.c1) * C + c;
    for (int n = 0; n < N; ++n) {
        const T* im = image + n * frame;
        const double s = t.inside ? lut_blend(t, (double)im[i00], (double)im[i01], (double)im[i10], (double)im[i11]) : 0.0;
        lut_store(out + n * frame + e, s);
    }
}

// grid (blocks of HW pixels): cfa (N,H,W) uint8 -> out (N,H,W,3) uint8 = undistort(demosaic(cfa)), nothing in between in memory
__global__ __launch_bounds__(256) void robotcar_rectify_kernel(const unsigned char* __restrict__ cfa, const double* __restrict__ lut,
                                                               unsigned char* __restrict__ out, int N, int H, int W, int sites) {
    __shared__ unsigned int stage[2][kRcThreads * 3 / 4];
    const int npx = H * W, tid = threadIdx.x;
    const int p0 = blockIdx.x * kRcThreads, p = p0 + tid;
    const bool live = p < npx;
    const int nbytes = min(kRcThreads, npx - p0) * 3;
    LutTap t;
    t.inside = 0;
    int rows[4] = {0, 0, 0, 0}, cols[4] = {0, 0, 0, 0};
    if (live) {
        t = lut_tap(lut, npx, p, H, W);
        // r1 = reflect(r0 + 1): the rows of tap (1, .) are rows[1..3], except at the far edge, where its weight is 0
        rows[0] = bayer_reflect(t.r0 - 1, H); rows[1] = t.r0; rows[2] = t.r1; rows[3] = bayer_reflect(t.r1 + 1, H);
        cols[0] = bayer_reflect(t.c0 - 1, W); cols[1] = t.c0; cols[2] = t.c1; cols[3] = bayer_reflect(t.c1 + 1, W);
    }
    for (int n = 0; n < N; ++n) {
        unsigned char* mine = reinterpret_cast<unsigned char*>(stage[n & 1]) + 3 * tid;
        unsigned char b0 = 0, b1 = 0, b2 = 0;
        if (live && t.inside) {
            int v[4][4], ch[4][4];
            bayer_patch(cfa + (size_t)n * npx, W, sites, rows, cols, 4, 4, v, ch);
            double a[3], b[3], c[3], d[3];
            bayer_bilinear<0, 0>(v, ch, a);
            bayer_bilinear<0, 1>(v, ch, b);
            bayer_bilinear<1, 0>(v, ch, c);
            bayer_bilinear<1, 1>(v, ch, d);
            b0 = lut_to_u8(lut_blend(t, a[0], b[0], c[0], d[0]));
            b1 = lut_to_u8(lut_blend(t, a[1], b[1], c[1], d[1]));
            b2 = lut_to_u8(lut_blend(t, a[2], b[2], c[2], d[2]));
        }
        mine[0] = b0; mine[1] = b1; mine[2] = b2;
        __syncthreads();
        unsigned char* dst = out + ((size_t)n * npx + p0) * 3;
        const unsigned char* src = reinterpret_cast<const unsigned char*>(stage[n & 1]);
        if (((size_t)dst & 3) == 0) {                                          // block-uniform
            if (tid < nbytes / 4) reinterpret_cast<unsigned int*>(dst)[tid] = stage[n & 1][tid];
            if (tid < (nbytes & 3)) dst[(nbytes & ~3) + tid] = src[(nbytes & ~3) + tid];
        } else {
            for (int i = tid; i < nbytes; i += kRcThreads) dst[i] = src[i];
        }
    }
}

}  // namespace clslam

using namespace clslam;

// index = CLSLAM_BAYER_*
static int bayer_sites(int pattern) {
    static const int kSites[4] = {0 | 1 << 2 | 1 << 4 | 2 << 6,      // rggb
                                  2 | 1 << 2 | 1 << 4 | 0 << 6,      // bggr
                                  1 | 0 << 2 | 2 << 4 | 1 << 6,      // grbg
                                  1 | 2 << 2 | 0 << 4 | 1 << 6};     // gbrg
    return kSites[pattern];
}

static bool rc_geometry(int h, int w, int c) { return h > 0 && w > 0 && c > 0 && (long long)h * w * c <= (1ll << 30); }

extern "C" int clslam_demosaic_bilinear(const unsigned char* cfa, double* out, int n, int h, int w, int pattern, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n >= 0 && n <= 65535, "demosaic_bilinear: 0..65535 frames per call");
    CLSLAM_REQUIRE(rc_geometry(h, w, 3), "demosaic_bilinear: bad geometry (frames of 1..2^30 / 3 pixels)");
    CLSLAM_REQUIRE(pattern >= 0 && pattern <= 3, "demosaic_bilinear: unknown pattern (CLSLAM_BAYER_*)");
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(cfa && out && ((size_t)out & 7) == 0, "demosaic_bilinear: null pointer, or an output that is not 8-byte aligned");
    hipLaunchKernelGGL(demosaic_bilinear_kernel, dim3(cdiv(h * w * 3, kRcThreads), n), dim3(kRcThreads), 0, stream, cfa, out, h, w,
                       bayer_sites(pattern));
    return check_launch("demosaic_bilinear");
}

extern "C" int clslam_undistort_lut(const void* image, const double* lut, void* out, int n, int h, int w, int c, int is_f64,
                                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n >= 0, "undistort_lut: negative frame count");
    CLSLAM_REQUIRE(rc_geometry(h, w, c), "undistort_lut: bad geometry (frames of 1..2^30 elements)");
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(image && lut && out && image != out && ((size_t)lut & 7) == 0,
                   "undistort_lut: null pointer, in-place call, or a table that is not 8-byte aligned");
    const dim3 grid(cdiv(h * w * c, kRcThreads)), block(kRcThreads);
    if (is_f64) {
        CLSLAM_REQUIRE((((size_t)image | (size_t)out) & 7) == 0, "undistort_lut: float64 images must be 8-byte aligned");
        hipLaunchKernelGGL(undistort_lut_kernel<double>, grid, block, 0, stream, (const double*)image, lut, (double*)out, n, h, w, c);
    } else {
        hipLaunchKernelGGL(undistort_lut_kernel<unsigned char>, grid, block, 0, stream, (const unsigned char*)image, lut,
                           (unsigned char*)out, n, h, w, c);
    }
    return check_launch("undistort_lut");
}

extern "C" int clslam_robotcar_rectify(const unsigned char* cfa, const double* lut, unsigned char* out, int n, int h, int w, int pattern,
                                       void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(n >= 0, "robotcar_rectify: negative frame count");
    CLSLAM_REQUIRE(rc_geometry(h, w, 3), "robotcar_rectify: bad geometry (frames of 1..2^30 / 3 pixels)");
    CLSLAM_REQUIRE(pattern >= 0 && pattern <= 3, "robotcar_rectify: unknown pattern (CLSLAM_BAYER_*)");
    if (n == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(cfa && lut && out && ((size_t)lut & 7) == 0, "robotcar_rectify: null pointer, or a table that is not 8-byte aligned");
    hipLaunchKernelGGL(robotcar_rectify_kernel, dim3(cdiv(h * w, kRcThreads)), dim3(kRcThreads), 0, stream, cfa, lut, out, n, h, w,
                       bayer_sites(pattern));
    return check_launch("robotcar_rectify");
}
