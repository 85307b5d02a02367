// Image-pyramid ingest: the LANCZOS resize + ToTensor of the reference's datasets
// (datasets/utils.py:62-66 Resize(LANCZOS) per scale, :154-163 every level from the previous one,
// :213-215 ToTensor) on uint8 images that were uploaded once, instead of PIL on one host thread.
//
// torchvision's Resize on a PIL image is PIL.Image.resize(size, LANCZOS) = Pillow's ImagingResample 8-bit
// path (libImaging/Resample.c; not part of /root/reference, restated in oracle/resize.py): per output
// index a window of taps with double-precision Lanczos-3 weights normalised to 1, converted to 22-bit
// fixed point; horizontal pass then vertical pass, int32 accumulation from 1 << 21, (acc >> 22) clipped
// to [0,255], uint8 intermediate.  The tap plan is computed on the HOST with libm exactly like Pillow
// (clslam_lanczos_plan); the kernels are integer multiply-accumulates -> results are BIT-EXACT.
// HBM-bound byte work: 3 B read + 3 B written per pixel per pass (+12 B for the fused float planes).
#include <cmath>
#include <vector>

#include "common.h"

// Pillow's C is compiled without fused multiply-add: every rounding below must happen where C puts it
// (hipcc contracts a*b+c by default, and __fmul_rn/__fadd_rn are plain operators in the ROCm headers).
#pragma clang fp contract(off)

namespace clslam {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;

// One thread per output pixel (all C <= 4 channels).  axis 1: out (B,H,out,C) from in (B,H,in_w,C);
// axis 0: out (B,out,W,C) from in (B,in_h,W,C).  planar (optional): float (B,C,oh,ow) = out / 255.
__global__ __launch_bounds__(256) void resize_pass_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                             float* __restrict__ planar, const int* __restrict__ bounds,
                                                             const int* __restrict__ coeffs, int ksize, int B, int in_h, int in_w,
                                                             int C, int out_size, int axis) {
    const int oh = axis == 0 ? out_size : in_h, ow = axis == 1 ? out_size : in_w;
    const int total = B * oh * ow;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int x = i % ow, y = (i / ow) % oh, b = i / (ow * oh);
        const int o = axis == 1 ? x : y;
        const int first = bounds[2 * o], n = bounds[2 * o + 1];
        const int* k = coeffs + (size_t)o * ksize;
        int acc[4] = {1 << (RS_PRECISION_BITS - 1), 1 << (RS_PRECISION_BITS - 1), 1 << (RS_PRECISION_BITS - 1),
                      1 << (RS_PRECISION_BITS - 1)};
        const size_t step = axis == 1 ? (size_t)C : (size_t)in_w * C;
        const unsigned char* p = src + (((size_t)b * in_h + (axis == 1 ? y : first)) * in_w + (axis == 1 ? first : x)) * C;
        for (int t = 0; t < n; ++t) {
            const int w = k[t];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) acc[c] += (int)p[c] * w;
            p += step;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= C) continue;
            const int v = min(max(acc[c] >> RS_PRECISION_BITS, 0), 255);
            dst[(((size_t)b * oh + y) * ow + x) * C + c] = (unsigned char)v;
            if (planar) planar[(((size_t)b * C + c) * oh + y) * ow + x] = (float)v / 255.f;   // ToTensor
        }
    }
}

// ToTensor alone (level 0 when the raw image already has the model's size)
__global__ __launch_bounds__(256) void u8_to_planar_kernel(const unsigned char* __restrict__ src, float* __restrict__ planar, int B,
                                                           int H, int W, int C) {
    const int total = B * H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int x = i % W, y = (i / W) % H, b = i / (W * H);
        for (int c = 0; c < C; ++c)
            planar[(((size_t)b * C + c) * H + y) * W + x] = (float)src[(size_t)i * C + c] / 255.f;
    }
}

// ------------------------------------------------------------------------------------------------
// Colour jitter (datasets/utils.py:236-259: torchvision adjust_{brightness,contrast,saturation,hue} on PIL
// images in a random order; restated with Pillow's exact C arithmetic in oracle/jitter.py).  uint8 RGB
// interleaved; every op is one elementwise kernel, contrast additionally needs the image's mean luminance
// (exact integer sum by 64-bit atomics: order-independent, hence deterministic).
__device__ __forceinline__ int lum_u8(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(other, img, alpha): float32 multiply and add, NOT fused (Pillow's C is not contracted);
// alpha in [0,1] truncates, otherwise clips.
__device__ __forceinline__ unsigned char blend_u8(int other, int v, float alpha, bool interp) {
    const float m = alpha * (float)(v - other);    // separate roundings (contraction is off in this file)
    const float t = (float)other + m;
    if (interp) return (unsigned char)t;
    return t <= 0.f ? (unsigned char)0 : (t >= 255.f ? (unsigned char)255 : (unsigned char)t);
}

__global__ __launch_bounds__(256) void jitter_lsum_kernel(const unsigned char* __restrict__ img, unsigned long long* __restrict__ lsum,
                                                          int HW) {
    __shared__ unsigned long long red[4];
    const int b = blockIdx.y;
    unsigned long long s = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const unsigned char* p = img + ((size_t)b * HW + i) * 3;
        s += (unsigned long long)lum_u8(p[0], p[1], p[2]);
    }
    // block reduction through LDS (integers: any order gives the same sum)
    for (int off = 32; off >= 1; off >>= 1) {
        const float lo = wave_shfl_xor(__uint_as_float((unsigned)(s & 0xffffffffu)), off);
        const float hi = wave_shfl_xor(__uint_as_float((unsigned)(s >> 32)), off);
        s += ((unsigned long long)__float_as_uint(hi) << 32) | (unsigned long long)__float_as_uint(lo);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&lsum[b], red[0] + red[1] + red[2] + red[3]);
}

// mode 0: brightness (other = 0), 1: contrast (other = int(mean L + 0.5)), 2: saturation (other = L of the pixel)
__global__ __launch_bounds__(256) void jitter_blend_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                           const unsigned long long* __restrict__ lsum, int B, int HW, int mode,
                                                           float alpha) {
    const bool interp = alpha >= 0.f && alpha <= 1.f;
    const int total = B * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const unsigned char* p = src + (size_t)i * 3;
        const int r = p[0], g = p[1], b = p[2];
        int other = 0;
        if (mode == 1) other = (int)((double)lsum[i / HW] / (double)HW + 0.5);    // ImageStat mean, Python float
        else if (mode == 2) other = lum_u8(r, g, b);
        unsigned char* o = dst + (size_t)i * 3;
        o[0] = blend_u8(other, r, alpha, interp);
        o[1] = blend_u8(other, g, alpha, interp);
        o[2] = blend_u8(other, b, alpha, interp);
    }
}

// Pillow's rgb2hsv_row -> h += shift (uint8 wrap) -> hsv2rgb, with its float / double mix
__global__ __launch_bounds__(256) void jitter_hue_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                         int total, int shift) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const unsigned char* p = src + (size_t)i * 3;
        const int r = p[0], g = p[1], b = p[2];
        const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
        int uh = 0, us = 0;
        const int uv = maxc;
        if (minc != maxc) {
            const float cr = (float)(maxc - minc);
            const float s = cr / (float)maxc;
            const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
            float h;
            if (r == maxc) h = bc - gc;
            else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
            else h = (float)(4.0 + (double)gc - (double)rc);
            h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
            uh = min(max((int)((double)h * 255.0), 0), 255);
            us = min(max((int)((double)s * 255.0), 0), 255);
        }
        uh = (uh + shift) & 255;
        unsigned char* o = dst + (size_t)i * 3;
        if (us == 0) {
            o[0] = o[1] = o[2] = (unsigned char)uv;
            continue;
        }
        const double h6 = (double)(float)uh * 6.0 / 255.0;
        const int ii = (int)floor(h6);
        const double f = (double)(float)(h6 - (double)(float)ii);
        const double fs = (double)(float)((double)(float)us / 255.0);
        const double v = (double)(float)uv;
        const int pp = min(max((int)round(v * (1.0 - fs)), 0), 255);
        const int qq = min(max((int)round(v * (1.0 - fs * f)), 0), 255);
        const int tt = min(max((int)round(v * (1.0 - fs * (1.0 - f))), 0), 255);
        int R, G, Bc;
        switch (ii % 6) {
            case 0: R = uv; G = tt; Bc = pp; break;
            case 1: R = qq; G = uv; Bc = pp; break;
            case 2: R = pp; G = uv; Bc = tt; break;
            case 3: R = pp; G = qq; Bc = uv; break;
            case 4: R = tt; G = pp; Bc = uv; break;
            default: R = uv; G = pp; Bc = qq; break;
        }
        o[0] = (unsigned char)R; o[1] = (unsigned char)G; o[2] = (unsigned char)Bc;
    }
}

static double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

static double lanczos_filter(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}

}  // namespace clslam

using namespace clslam;

// Taps per output index of a LANCZOS resize in_size -> out_size (the row length of the coefficient table).
extern "C" int clslam_lanczos_ksize(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0) return 0;
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(3.0 * filterscale) * 2 + 1;
}

// HOST function: bounds[out_size][2] = (first tap, tap count), coeffs[out_size][ksize] = 22-bit fixed-point
// weights, computed in double with libm like Pillow's precompute_coeffs + normalize_coeffs_8bpc.
extern "C" int clslam_lanczos_plan(int in_size, int out_size, int* bounds, int* coeffs) {
    CLSLAM_REQUIRE(in_size > 0 && out_size > 0 && bounds && coeffs, "lanczos_plan: bad args");
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = lanczos_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = xmax; x < ksize; ++x) k[x] = 0.0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
        for (int x = 0; x < ksize; ++x) {
            const double f = k[x] * (1 << RS_PRECISION_BITS);
            coeffs[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + f) : (int)(0.5 + f);
        }
    }
    return CLSLAM_OK;
}

// One pass of the separable resize on interleaved uint8 images (device pointers; bounds/coeffs = the plan
// uploaded by the caller).  axis 1 = horizontal (width in_w -> out_size), axis 0 = vertical (height in_h ->
// out_size).  planar (optional): additionally writes ToTensor(out) as float (B,C,oh,ow).
extern "C" int clslam_resize_pass_u8(const unsigned char* src, unsigned char* dst, float* planar, const int* bounds,
                                     const int* coeffs, int ksize, int batch, int in_h, int in_w, int ch, int out_size, int axis,
                                     void* stream) {
    if (batch == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(src && dst && bounds && coeffs && ksize > 0 && ch >= 1 && ch <= 4 && (axis == 0 || axis == 1) && out_size > 0,
                   "resize_pass_u8: bad args");
    const size_t total = (size_t)batch * (axis == 0 ? out_size : in_h) * (axis == 1 ? out_size : in_w);
    CLSLAM_REQUIRE(total < ((size_t)1 << 31), "resize_pass_u8: image too large for 32-bit indexing");
    if (!total) return CLSLAM_OK;
    const unsigned blocks = (unsigned)std::min<size_t>(8192, (total + 255) / 256);
    hipLaunchKernelGGL(resize_pass_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, dst, planar, bounds, coeffs,
                       ksize, batch, in_h, in_w, ch, out_size, axis);
    return check_launch("resize_pass_u8");
}

extern "C" int clslam_u8_to_planar_f32(const unsigned char* src, float* planar, int batch, int h, int w, int ch, void* stream) {
    if (batch == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(src && planar && ch >= 1, "u8_to_planar_f32: bad args");
    const size_t total = (size_t)batch * h * w;
    CLSLAM_REQUIRE(total < ((size_t)1 << 31), "u8_to_planar_f32: image too large for 32-bit indexing");
    if (!total) return CLSLAM_OK;
    const unsigned blocks = (unsigned)std::min<size_t>(8192, (total + 255) / 256);
    hipLaunchKernelGGL(u8_to_planar_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, planar, batch, h, w, ch);
    return check_launch("u8_to_planar_f32");
}

// Colour jitter of interleaved uint8 RGB images (B,h,w,3).  order[n_ops]: op ids in application order
// (0 brightness, 1 contrast, 2 saturation, 3 hue), factors[4] (double, as Python draws them) indexed by op id
// (HOST arrays).  scratch: a
// second image buffer of the same size (ops ping-pong, the result ends in dst); lsum: batch uint64 of
// device scratch for the contrast mean.  src is not modified.
extern "C" int clslam_color_jitter_u8(const unsigned char* src, unsigned char* dst, unsigned char* scratch,
                                      unsigned long long* lsum, int batch, int h, int w, const int* order, int n_ops,
                                      const double* factors, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CLSLAM_REQUIRE(order && factors && n_ops >= 0 && n_ops <= 8, "color_jitter_u8: bad args");
    for (int k = 0; k < n_ops; ++k) CLSLAM_REQUIRE(order[k] >= 0 && order[k] <= 3, "color_jitter_u8: unknown op %d", order[k]);
    CLSLAM_REQUIRE(n_ops == 0 || (factors[3] >= -0.5 && factors[3] <= 0.5), "color_jitter_u8: hue_factor outside [-0.5, 0.5]");
    if (batch == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(src && dst && scratch && lsum, "color_jitter_u8: null pointer");
    const size_t total = (size_t)batch * h * w;
    CLSLAM_REQUIRE(total < ((size_t)1 << 30), "color_jitter_u8: image too large for 32-bit indexing");
    if (!total) return CLSLAM_OK;
    const unsigned blocks = (unsigned)std::min<size_t>(4096, (total + 255) / 256);
    if (n_ops == 0) {
        hipMemcpyAsync(dst, src, total * 3, hipMemcpyDeviceToDevice, stream);
        return check_launch("color_jitter_u8");
    }
    const unsigned char* cur = src;
    for (int k = 0; k < n_ops; ++k) {
        unsigned char* out = ((n_ops - 1 - k) % 2 == 0) ? dst : scratch;     // the last op writes dst
        const int op = order[k];
        if (op == 3) {
            const int shift = ((int)(factors[3] * 255.0) % 256 + 256) % 256;   // np.uint8(hue_factor * 255): truncate, wrap
            hipLaunchKernelGGL(jitter_hue_kernel, dim3(blocks), dim3(256), 0, stream, cur, out, (int)total, shift);
        } else {
            if (op == 1) {
                hipMemsetAsync(lsum, 0, sizeof(unsigned long long) * batch, stream);
                hipLaunchKernelGGL(jitter_lsum_kernel, dim3(std::min(64, cdiv(h * w, 256)), batch), dim3(256), 0, stream, cur, lsum,
                                   h * w);
            }
            hipLaunchKernelGGL(jitter_blend_kernel, dim3(blocks), dim3(256), 0, stream, cur, out, lsum, batch, h * w, op,
                               (float)factors[op]);   // Image.blend takes a C float
        }
        cur = out;
    }
    return check_launch("color_jitter_u8");
}

// =====================================================================================================================
// The replay buffer's colour jitter: torchvision's TENSOR code path on float images in [0, 1] (slam/replay_buffer.py:264-265,
// 281-283 after ToTensor; slam/slam.py:98 do_augmentation=True) -- functional_tensor.py of torchvision 0.11.1, operation by
// operation (oracle/jitter_tensor.py is the checker): _blend = (ratio * a + (1 - ratio) * b).clamp(0, 1) in float32, gray =
// 0.2989 r + 0.587 g + 0.114 b, contrast blends with the image's mean gray, hue = _rgb2hsv -> (h + f) % 1 -> _hsv2rgb.
// Contraction is off for this file: every product and sum rounds where torch's separate kernels round.
// One image = one (3, h, w) planar float plane set with ITS OWN op order and factors (a replayed sample draws one jitter for its
// three frames and four scales; the contrast mean is per image).  Two launches for any number of images: pass 1 applies the ops
// in front of `contrast` and leaves per-block sums of the gray value, pass 2 forms the mean (fixed order) and applies the chain.
namespace clslam {

struct JitterParams {        // per image, device memory: order[k] in {0 brightness, 1 contrast, 2 saturation, 3 hue, -1 end}
    int order[4];
    float f[4];              // factor as a C float, indexed by op id
    float omf[4];            // (float)(1.0 - factor): torch forms 1.0 - ratio in double before the multiply
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

__device__ __forceinline__ void jitter_hue(float& r, float& g, float& b, float hf) {
    // _rgb2hsv
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float crd = eqc ? 1.f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    const float hr = (maxc == r) ? (bc - gc) : 0.f;
    const float hg = ((maxc == g) && (maxc != r)) ? ((2.0f + rc) - bc) : 0.f;
    const float hb = ((maxc != g) && (maxc != r)) ? ((4.0f + gc) - rc) : 0.f;
    float h = (hr + hg) + hb;
    h = fmodf(h / 6.0f + 1.0f, 1.0f);
    // (h + hue_factor) % 1.0: torch.remainder = fmod, then + 1 when the sign differs from the divisor's
    float hh = fmodf(h + hf, 1.0f);
    if (hh != 0.f && hh < 0.f) hh += 1.0f;
    // _hsv2rgb
    const float v = maxc;
    const float h6 = hh * 6.0f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    int i = (int)fl;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - f * s));
    const float t = clamp01(v * (1.0f - (s * (1.0f - f))));
    i = ((i % 6) + 6) % 6;
    r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// ops [k0, k1) of the chain on one pixel; `mean` is used by the contrast op only
__device__ __forceinline__ void jitter_ops(const JitterParams& P, int k0, int k1, float& r, float& g, float& b, float mean) {
    for (int k = k0; k < k1; ++k) {
        const int op = P.order[k];
        if (op < 0) break;
        const float f = P.f[op], omf = P.omf[op];
        if (op == 0) {
            r = clamp01(f * r + omf * 0.f); g = clamp01(f * g + omf * 0.f); b = clamp01(f * b + omf * 0.f);
        } else if (op == 1) {
            const float m = omf * mean;
            r = clamp01(f * r + m); g = clamp01(f * g + m); b = clamp01(f * b + m);
        } else if (op == 2) {
            const float m = omf * gray_of(r, g, b);
            r = clamp01(f * r + m); g = clamp01(f * g + m); b = clamp01(f * b + m);
        } else {
            jitter_hue(r, g, b, f);
        }
    }
}

// blocks per image of the gray-sum pass (its partition fixes the summation order of the contrast mean)
__host__ __device__ inline int jitter_sum_blocks(int hw) {
    const int n = (hw + 1023) / 1024;
    return n < 1 ? 1 : (n > 64 ? 64 : n);
}

__device__ __forceinline__ int jitter_contrast_pos(const JitterParams& P) {
    for (int k = 0; k < 4; ++k) {
        if (P.order[k] < 0) break;
        if (P.order[k] == 1) return k;
    }
    return -1;
}

// grid (nblk, images).  partial[img][blk] = sum of the gray value in front of the contrast op over the block's pixels
__global__ __launch_bounds__(256) void jitter_f32_sum_kernel(const float* __restrict__ src, const JitterParams* __restrict__ params,
                                                             float* __restrict__ partial, int hw) {
    __shared__ float red[4];
    const int img = blockIdx.y;
    const JitterParams P = params[img];
    const int kc = jitter_contrast_pos(P);
    if (kc < 0) return;
    const float* base = src + (size_t)img * 3 * hw;
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        float r = base[i], g = base[hw + i], b = base[2 * hw + i];
        jitter_ops(P, 0, kc, r, g, b, 0.f);
        acc += gray_of(r, g, b);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)img * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void jitter_f32_apply_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               const JitterParams* __restrict__ params, const float* __restrict__ partial,
                                                               int nblk_sum, int hw) {
    __shared__ float s_mean;
    const int img = blockIdx.y;
    const JitterParams P = params[img];
    if (threadIdx.x == 0) {
        float m = 0.f;
        if (jitter_contrast_pos(P) >= 0) {
            for (int k = 0; k < nblk_sum; ++k) m += partial[(size_t)img * nblk_sum + k];     // fixed order
            m = m / (float)hw;
        }
        s_mean = m;
    }
    __syncthreads();
    const float mean = s_mean;
    const float* base = src + (size_t)img * 3 * hw;
    float* out = dst + (size_t)img * 3 * hw;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        float r = base[i], g = base[hw + i], b = base[2 * hw + i];
        jitter_ops(P, 0, 4, r, g, b, mean);
        out[i] = r; out[hw + i] = g; out[2 * hw + i] = b;
    }
}

}  // namespace clslam

extern "C" int clslam_color_jitter_f32_blocks(int h, int w) { return clslam::jitter_sum_blocks(h * w); }

extern "C" int clslam_color_jitter_f32(const float* src, float* dst, const void* params, float* partial, int n_images, int h, int w,
                                       void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images == 0 || h * w == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(src && dst && params && partial, "color_jitter_f32: null pointer");
    CLSLAM_REQUIRE(n_images > 0 && n_images <= 65535 && h > 0 && w > 0, "color_jitter_f32: bad geometry");
    const int nblk = clslam_color_jitter_f32_blocks(h, w);
    hipLaunchKernelGGL(clslam::jitter_f32_sum_kernel, dim3(nblk, n_images), dim3(256), 0, stream, src, (const clslam::JitterParams*)params,
                       partial, h * w);
    const int nb2 = std::max(1, std::min(256, clslam::cdiv(h * w, 512)));
    hipLaunchKernelGGL(clslam::jitter_f32_apply_kernel, dim3(nb2, n_images), dim3(256), 0, stream, src, dst,
                       (const clslam::JitterParams*)params, partial, nblk, h * w);
    return clslam::check_launch("color_jitter_f32");
}

// =====================================================================================================================
// Frame store: replayed samples served from HBM instead of from their PNGs.  When ReplayBuffer.add (slam/replay_buffer.py:82-184)
// sees a sample, that sample already holds the un-augmented pyramid `_get` later rebuilds from the image files
// (replay_buffer.py:270-279 runs the chain of datasets/kitti.py:249-259, datasets/utils.py:154-171): every value is fl32(b / 255) of
// a byte b, and b = round(x * 255) recovers it.  A slot keeps those bytes: per frame and level one planar (3, h, w) block at a
// fixed, 16-byte aligned offset.  clslam_store_pack fills a slot from float planes; clslam_store_gather_jitter turns slots back
// into the rgb / rgb_aug rows of the minibatch (ToTensor with u8_to_planar_kernel's arithmetic, then the chain of
// clslam_color_jitter_f32 with ITS summation order for the contrast mean: bitwise the same rgb_aug).
namespace clslam {

__device__ __forceinline__ unsigned store_byte(float x, unsigned& bad) {
    const float q = fminf(fmaxf(rintf(x * 255.f), 0.f), 255.f);       // NaN -> 0 (and counted below)
    const unsigned char b = (unsigned char)q;
    bad += ((float)b / 255.f != x) ? 1u : 0u;
    return b;
}

// grid (blocks, planes).  One plane = the 3 * h * w floats of one frame at one level.
__global__ __launch_bounds__(256) void store_pack_kernel(clslam_store_pack_desc d, unsigned char* __restrict__ slot,
                                                         unsigned long long* __restrict__ inexact) {
    const int pl = blockIdx.y;
    const float* __restrict__ src = d.plane[pl];
    unsigned char* __restrict__ dst = slot + d.offset[pl];
    const int n = d.count[pl];
    const int nvec = (((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0) ? n >> 2 : 0;
    unsigned bad = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        const unsigned b0 = store_byte(v.x, bad), b1 = store_byte(v.y, bad), b2 = store_byte(v.z, bad), b3 = store_byte(v.w, bad);
        reinterpret_cast<unsigned*>(dst)[i] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
    for (int i = 4 * nvec + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = (unsigned char)store_byte(src[i], bad);
    const float total = wave_sum((float)bad);          // small integers: exact
    if ((threadIdx.x & 63) == 0 && total > 0.f) atomicAdd(inexact, (unsigned long long)total);
}

struct GatherImage {
    const unsigned char* bytes;     // the (3, h, w) block of this image and level, nullptr: not served from the store
    int hw, nblk, table;            // pixels, blocks of the sum pass, index into the descriptor's tables
};

__device__ __forceinline__ GatherImage gather_image(const clslam_store_gather_desc& d, const unsigned char* store,
                                                    const int* slot_idx, int img, int li) {
    GatherImage g;
    const int slot = slot_idx[img];
    g.table = (img % d.n_frames) * d.n_levels + li;
    g.hw = d.h[li] * d.w[li];
    g.nblk = jitter_sum_blocks(g.hw);
    g.bytes = (slot < 0 || slot >= d.capacity) ? nullptr : store + (size_t)slot * d.slot_bytes + d.offset[g.table];
    return g;
}

// grid (max sum blocks, images, levels); partial[level][image][64].  The partition of clslam_color_jitter_f32's sum pass: block b
// of nblk, thread t takes the pixels b * 256 + t + k * nblk * 256.
__global__ __launch_bounds__(256) void store_gather_sum_kernel(clslam_store_gather_desc d, const unsigned char* __restrict__ store,
                                                               const int* __restrict__ slot_idx,
                                                               const JitterParams* __restrict__ params, float* __restrict__ partial,
                                                               int n_images) {
    __shared__ float red[4];
    const int img = blockIdx.y, li = blockIdx.z;
    const GatherImage g = gather_image(d, store, slot_idx, img, li);
    if (!g.bytes || (int)blockIdx.x >= g.nblk) return;
    const JitterParams P = params[img];
    const int kc = jitter_contrast_pos(P);
    if (kc < 0) return;
    const int hw = g.hw;
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += g.nblk * 256) {
        float r = (float)g.bytes[i] / 255.f, gg = (float)g.bytes[hw + i] / 255.f, b = (float)g.bytes[2 * hw + i] / 255.f;
        jitter_ops(P, 0, kc, r, gg, b, 0.f);
        acc += gray_of(r, gg, b);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[((size_t)li * n_images + img) * 64 + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (blocks, images, levels).  Four pixels per thread (one dword of bytes per colour plane in, one float4 per plane out)
// where the block and both rows are aligned for it, one pixel per thread for the rest.
__global__ __launch_bounds__(256) void store_gather_apply_kernel(clslam_store_gather_desc d, const unsigned char* __restrict__ store,
                                                                 const int* __restrict__ slot_idx,
                                                                 const JitterParams* __restrict__ params,
                                                                 const float* __restrict__ partial, int n_images, int row0) {
    __shared__ float s_mean;
    const int img = blockIdx.y, li = blockIdx.z;
    const GatherImage g = gather_image(d, store, slot_idx, img, li);
    const int hw = g.hw;
    if (!g.bytes || (int)blockIdx.x * 256 >= hw) return;
    const bool jitter = d.aug[g.table] != nullptr;
    JitterParams P;
    P.order[0] = -1;
    if (jitter) P = params[img];
    if (threadIdx.x == 0) {
        float m = 0.f;
        if (jitter && jitter_contrast_pos(P) >= 0) {
            const float* part = partial + ((size_t)li * n_images + img) * 64;
            for (int k = 0; k < g.nblk; ++k) m += part[k];     // fixed order
            m = m / (float)hw;
        }
        s_mean = m;
    }
    __syncthreads();
    const float mean = s_mean;
    const size_t row = (size_t)(row0 + img / d.n_frames) * (size_t)d.stride[g.table];
    float* __restrict__ rgb = d.rgb[g.table] + row;
    float* __restrict__ aug = jitter ? d.aug[g.table] + row : nullptr;
    const bool aligned = (hw & 3) == 0 && ((uintptr_t)g.bytes & 3) == 0 && ((uintptr_t)rgb & 15) == 0 && ((uintptr_t)aug & 15) == 0;
    const int nvec = aligned ? hw >> 2 : 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) {
        const unsigned R = reinterpret_cast<const unsigned*>(g.bytes)[i], G = reinterpret_cast<const unsigned*>(g.bytes + hw)[i],
                       B = reinterpret_cast<const unsigned*>(g.bytes + 2 * hw)[i];
        float r[4], gg[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = (float)((R >> (8 * j)) & 255u) / 255.f;
            gg[j] = (float)((G >> (8 * j)) & 255u) / 255.f;
            b[j] = (float)((B >> (8 * j)) & 255u) / 255.f;
        }
        reinterpret_cast<float4*>(rgb)[i] = make_float4(r[0], r[1], r[2], r[3]);
        reinterpret_cast<float4*>(rgb + hw)[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
        reinterpret_cast<float4*>(rgb + 2 * hw)[i] = make_float4(b[0], b[1], b[2], b[3]);
        if (!jitter) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) jitter_ops(P, 0, 4, r[j], gg[j], b[j], mean);
        reinterpret_cast<float4*>(aug)[i] = make_float4(r[0], r[1], r[2], r[3]);
        reinterpret_cast<float4*>(aug + hw)[i] = make_float4(gg[0], gg[1], gg[2], gg[3]);
        reinterpret_cast<float4*>(aug + 2 * hw)[i] = make_float4(b[0], b[1], b[2], b[3]);
    }
    for (int i = 4 * nvec + blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        float r = (float)g.bytes[i] / 255.f, gg = (float)g.bytes[hw + i] / 255.f, b = (float)g.bytes[2 * hw + i] / 255.f;
        rgb[i] = r; rgb[hw + i] = gg; rgb[2 * hw + i] = b;
        if (!jitter) continue;
        jitter_ops(P, 0, 4, r, gg, b, mean);
        aug[i] = r; aug[hw + i] = gg; aug[2 * hw + i] = b;
    }
}

}  // namespace clslam

extern "C" int clslam_store_pack(const clslam_store_pack_desc* desc, unsigned char* slot, unsigned long long* inexact, void* stream) {
    CLSLAM_REQUIRE(desc && slot && inexact, "store_pack: null pointer");
    CLSLAM_REQUIRE(desc->n_planes >= 0 && desc->n_planes <= CLSLAM_STORE_MAX_PLANES, "store_pack: %d planes (at most %d)",
                   desc->n_planes, CLSLAM_STORE_MAX_PLANES);
    int most = 0;
    for (int k = 0; k < desc->n_planes; ++k) {
        CLSLAM_REQUIRE(desc->plane[k] && desc->offset[k] >= 0 && desc->count[k] > 0, "store_pack: bad plane %d", k);
        most = std::max(most, desc->count[k]);
    }
    if (desc->n_planes == 0) return CLSLAM_OK;
    const int blocks = std::max(1, std::min(256, clslam::cdiv(most, 4 * 256)));
    hipLaunchKernelGGL(clslam::store_pack_kernel, dim3(blocks, desc->n_planes), dim3(256), 0, (hipStream_t)stream, *desc, slot, inexact);
    return clslam::check_launch("store_pack");
}

extern "C" int clslam_store_gather_jitter(const clslam_store_gather_desc* desc, const unsigned char* store, const int* slot_idx,
                                          const void* params, float* partial, int n_images, int row0, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(desc && store && slot_idx, "store_gather_jitter: null pointer");
    CLSLAM_REQUIRE(n_images > 0 && n_images <= 65535 && row0 >= 0, "store_gather_jitter: bad geometry");
    CLSLAM_REQUIRE(desc->n_frames >= 1 && desc->n_levels >= 1 && desc->n_frames * desc->n_levels <= CLSLAM_STORE_MAX_PLANES,
                   "store_gather_jitter: %d frames x %d levels (at most %d planes)", desc->n_frames, desc->n_levels,
                   CLSLAM_STORE_MAX_PLANES);
    CLSLAM_REQUIRE(n_images % desc->n_frames == 0 && desc->capacity >= 1 && desc->slot_bytes > 0,
                   "store_gather_jitter: %d images are no whole samples of %d frames, or an empty store", n_images, desc->n_frames);
    bool jitter = false;
    int most = 1, nblk = 1;
    for (int li = 0; li < desc->n_levels; ++li) {
        CLSLAM_REQUIRE(desc->h[li] > 0 && desc->w[li] > 0 && (size_t)desc->h[li] * desc->w[li] < ((size_t)1 << 29),
                       "store_gather_jitter: bad size of level %d", li);
        most = std::max(most, desc->h[li] * desc->w[li]);
        nblk = std::max(nblk, clslam::jitter_sum_blocks(desc->h[li] * desc->w[li]));
    }
    for (int t = 0; t < desc->n_frames * desc->n_levels; ++t) {
        CLSLAM_REQUIRE(desc->rgb[t] && desc->offset[t] >= 0 && desc->stride[t] > 0, "store_gather_jitter: bad table entry %d", t);
        jitter = jitter || desc->aug[t];
    }
    CLSLAM_REQUIRE(!jitter || (params && partial), "store_gather_jitter: rgb_aug rows without parameters or scratch");
    if (jitter)
        hipLaunchKernelGGL(clslam::store_gather_sum_kernel, dim3(nblk, n_images, desc->n_levels), dim3(256), 0, stream, *desc, store,
                           slot_idx, (const clslam::JitterParams*)params, partial, n_images);
    const int nb2 = std::max(1, std::min(256, clslam::cdiv(most, 4 * 256)));
    hipLaunchKernelGGL(clslam::store_gather_apply_kernel, dim3(nb2, n_images, desc->n_levels), dim3(256), 0, stream, *desc, store,
                       slot_idx, (const clslam::JitterParams*)params, partial, n_images, row0);
    return clslam::check_launch("store_gather_jitter");
}

// =====================================================================================================================
// Online ingest: the driver's own sample (slam/slam.py:141, datasets/kitti.py:231-317) from a ring of per-frame uint8 pyramids.
// A frame's pyramid is built ONCE, one launch per level (clslam_resize_level_u8), into its ring slot; a sample is then one launch
// (clslam_ring_gather) that turns the slots of its frames into the float planes of the sample dict.
namespace clslam {

// One pyramid level, both Pillow passes in one kernel.  A workgroup owns RL_TH output rows x RL_TW output columns.  It runs the
// horizontal pass for the input rows its vertical taps reach and keeps the result in LDS AS BYTES (Pillow rounds and clips to
// uint8 between the passes), RL_ROWS rows at a time; the vertical pass accumulates from LDS.  A tile whose vertical taps span
// more than RL_ROWS input rows (ratios far above 2) takes several rounds: the int32 accumulator lives across them, and integer
// sums do not depend on the order.  At the pyramid's 2:1 a tile reaches 15 * 2 + 13 = 43 rows: one round.
// LDS per workgroup: RL_ROWS * RL_TW * 3 = 2304 bytes.  Arithmetic: resize_pass_u8_kernel's, tap for tap.
constexpr int RL_TH = 16, RL_TW = 16, RL_ROWS = 48;

// bh / kh == nullptr: no horizontal pass (in_w == ow); bv / kv == nullptr: no vertical pass (in_h == oh).
__global__ __launch_bounds__(256) void resize_level_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                              long long pitch, const int* __restrict__ bh, const int* __restrict__ kh,
                                                              int ksh, const int* __restrict__ bv, const int* __restrict__ kv, int ksv,
                                                              int in_h, int in_w, int oh, int ow) {
    __shared__ unsigned char mid[RL_ROWS * RL_TW * 3];
    const int tid = threadIdx.x, tx = tid % RL_TW, ty = tid / RL_TW;
    const int x0 = blockIdx.x * RL_TW, y0 = blockIdx.y * RL_TH, b = blockIdx.z;
    const int x = x0 + tx, y = y0 + ty;
    const bool live = x < ow && y < oh;
    const int ylast = min(y0 + RL_TH, oh) - 1;
    // input rows of this tile (the plan's windows move monotonically with the output index)
    const int row_lo = bv ? bv[2 * y0] : y0;
    const int row_hi = bv ? bv[2 * ylast] + bv[2 * ylast + 1] : ylast + 1;
    const int vfirst = live ? (bv ? bv[2 * y] : y) : 0, vn = live ? (bv ? bv[2 * y + 1] : 1) : 0;
    const int* vk = (bv && live) ? kv + (size_t)y * ksv : nullptr;
    const int cols = min(RL_TW, ow - x0);
    const unsigned char* img = src + (size_t)b * in_h * in_w * 3;
    int acc[3] = {1 << (RS_PRECISION_BITS - 1), 1 << (RS_PRECISION_BITS - 1), 1 << (RS_PRECISION_BITS - 1)};
    for (int r0 = row_lo; r0 < row_hi; r0 += RL_ROWS) {
        const int rows = min(RL_ROWS, row_hi - r0);
        // horizontal pass: rows x cols intermediate pixels, column-fastest over the threads
        for (int i = tid; i < rows * cols; i += 256) {
            const int r = i / cols, c = i - r * cols;
            const int ox = x0 + c;
            const unsigned char* line = img + (size_t)(r0 + r) * in_w * 3;
            unsigned char* m = mid + (r * RL_TW + c) * 3;
            if (!bh) {
                m[0] = line[ox * 3]; m[1] = line[ox * 3 + 1]; m[2] = line[ox * 3 + 2];
                continue;
            }
            const int first = bh[2 * ox], n = bh[2 * ox + 1];
            const int* k = kh + (size_t)ox * ksh;
            const unsigned char* p = line + (size_t)first * 3;
            int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < n; ++t) {
                const int w = k[t];
                a0 += (int)p[0] * w; a1 += (int)p[1] * w; a2 += (int)p[2] * w;
                p += 3;
            }
            m[0] = (unsigned char)min(max(a0 >> RS_PRECISION_BITS, 0), 255);
            m[1] = (unsigned char)min(max(a1 >> RS_PRECISION_BITS, 0), 255);
            m[2] = (unsigned char)min(max(a2 >> RS_PRECISION_BITS, 0), 255);
        }
        __syncthreads();
        // vertical pass: the taps of this thread's output row that fall into [r0, r0 + rows)
        const int t_lo = max(0, r0 - vfirst), t_hi = min(vn, r0 + rows - vfirst);
        for (int t = t_lo; t < t_hi; ++t) {
            const unsigned char* m = mid + ((vfirst + t - r0) * RL_TW + tx) * 3;
            if (!vk) {
                acc[0] = m[0]; acc[1] = m[1]; acc[2] = m[2];
                continue;
            }
            const int w = vk[t];
            acc[0] += (int)m[0] * w; acc[1] += (int)m[1] * w; acc[2] += (int)m[2] * w;
        }
        __syncthreads();                     // the next round overwrites mid
    }
    if (!live) return;
    unsigned char* o = dst + ((size_t)b * oh + y) * (size_t)pitch + (size_t)x * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)(bv ? min(max(acc[c] >> RS_PRECISION_BITS, 0), 255) : acc[c]);
}

// grid (blocks, frames, levels).  The slot keeps a level INTERLEAVED (h, w, 3), as the level kernel wrote it; every byte is read
// once and goes to both planar destinations.  Four pixels per thread (three dwords in, three float4 per destination out) where
// the level and both destinations are aligned for it, one pixel per thread otherwise.
__global__ __launch_bounds__(256) void ring_gather_kernel(clslam_ring_gather_desc d, const unsigned char* __restrict__ ring) {
    const int fi = blockIdx.y, li = blockIdx.z;
    const int hw = d.h[li] * d.w[li];
    if ((int)blockIdx.x * 256 >= hw) return;
    const int table = fi * d.n_levels + li;
    const unsigned char* __restrict__ bytes = ring + (size_t)d.slot[fi] * (size_t)d.slot_bytes + (size_t)d.offset[li];
    float* __restrict__ rgb = d.rgb[table];
    float* __restrict__ aug = d.aug[table];
    const bool aligned = (hw & 3) == 0 && ((uintptr_t)bytes & 3) == 0 && ((uintptr_t)rgb & 15) == 0 && ((uintptr_t)aug & 15) == 0;
    const int nvec = aligned ? hw >> 2 : 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) {
        const unsigned* q = reinterpret_cast<const unsigned*>(bytes) + 3 * (size_t)i;
        const unsigned q0 = q[0], q1 = q[1], q2 = q[2];            // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        const float r0 = (float)(q0 & 255u) / 255.f, g0 = (float)((q0 >> 8) & 255u) / 255.f, b0 = (float)((q0 >> 16) & 255u) / 255.f;
        const float r1 = (float)(q0 >> 24) / 255.f, g1 = (float)(q1 & 255u) / 255.f, b1 = (float)((q1 >> 8) & 255u) / 255.f;
        const float r2 = (float)((q1 >> 16) & 255u) / 255.f, g2 = (float)(q1 >> 24) / 255.f, b2 = (float)(q2 & 255u) / 255.f;
        const float r3 = (float)((q2 >> 8) & 255u) / 255.f, g3 = (float)((q2 >> 16) & 255u) / 255.f, b3 = (float)(q2 >> 24) / 255.f;
        const float4 R = make_float4(r0, r1, r2, r3), G = make_float4(g0, g1, g2, g3), B = make_float4(b0, b1, b2, b3);
        reinterpret_cast<float4*>(rgb)[i] = R;
        reinterpret_cast<float4*>(rgb + hw)[i] = G;
        reinterpret_cast<float4*>(rgb + 2 * hw)[i] = B;
        reinterpret_cast<float4*>(aug)[i] = R;
        reinterpret_cast<float4*>(aug + hw)[i] = G;
        reinterpret_cast<float4*>(aug + 2 * hw)[i] = B;
    }
    for (int i = 4 * nvec + blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        const unsigned char* p = bytes + (size_t)i * 3;
        const float r = (float)p[0] / 255.f, g = (float)p[1] / 255.f, b = (float)p[2] / 255.f;
        rgb[i] = r; rgb[hw + i] = g; rgb[2 * hw + i] = b;
        aug[i] = r; aug[hw + i] = g; aug[2 * hw + i] = b;
    }
}

}  // namespace clslam

extern "C" int clslam_resize_level_u8(const unsigned char* src, unsigned char* dst, long long dst_pitch, const int* bounds_h,
                                      const int* coeffs_h, int ksize_h, const int* bounds_v, const int* coeffs_v, int ksize_v,
                                      int batch, int in_h, int in_w, int ch, int out_h, int out_w, void* stream) {
    CLSLAM_REQUIRE(batch >= 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, "resize_level_u8: bad geometry (%d images, %d x %d -> %d x %d)",
                   batch, in_h, in_w, out_h, out_w);
    CLSLAM_REQUIRE(ch == 3, "resize_level_u8: %d channels (interleaved RGB only)", ch);
    if (batch == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(src && dst, "resize_level_u8: null pointer");
    CLSLAM_REQUIRE(dst_pitch >= (long long)out_w * 3, "resize_level_u8: a row pitch of %lld bytes is shorter than a row of %d pixels",
                   dst_pitch, out_w);
    CLSLAM_REQUIRE(in_w == out_w || (bounds_h && coeffs_h && ksize_h > 0), "resize_level_u8: width %d -> %d without a tap plan", in_w, out_w);
    CLSLAM_REQUIRE(in_h == out_h || (bounds_v && coeffs_v && ksize_v > 0), "resize_level_u8: height %d -> %d without a tap plan", in_h, out_h);
    CLSLAM_REQUIRE(batch <= 65535 && cdiv(out_h, RL_TH) <= 65535 && (size_t)batch * in_h * in_w < ((size_t)1 << 31) / 3 &&
                       (size_t)batch * out_h * (size_t)dst_pitch < ((size_t)1 << 40),
                   "resize_level_u8: image too large");
    const bool hpass = in_w != out_w, vpass = in_h != out_h;
    hipLaunchKernelGGL(resize_level_u8_kernel, dim3(cdiv(out_w, RL_TW), cdiv(out_h, RL_TH), batch), dim3(256), 0, (hipStream_t)stream, src,
                       dst, dst_pitch, hpass ? bounds_h : nullptr, hpass ? coeffs_h : nullptr, ksize_h, vpass ? bounds_v : nullptr,
                       vpass ? coeffs_v : nullptr, ksize_v, in_h, in_w, out_h, out_w);
    return check_launch("resize_level_u8");
}

extern "C" int clslam_ring_gather(const clslam_ring_gather_desc* desc, const unsigned char* ring, void* stream) {
    CLSLAM_REQUIRE(desc && ring, "ring_gather: null pointer");
    CLSLAM_REQUIRE(desc->n_frames >= 1 && desc->n_levels >= 1 && desc->n_frames * desc->n_levels <= CLSLAM_STORE_MAX_PLANES,
                   "ring_gather: %d frames x %d levels (at most %d planes)", desc->n_frames, desc->n_levels, CLSLAM_STORE_MAX_PLANES);
    CLSLAM_REQUIRE(desc->capacity >= 1 && desc->slot_bytes > 0, "ring_gather: an empty ring");
    int most = 1;
    for (int li = 0; li < desc->n_levels; ++li) {
        CLSLAM_REQUIRE(desc->h[li] > 0 && desc->w[li] > 0 && (size_t)desc->h[li] * desc->w[li] < ((size_t)1 << 29),
                       "ring_gather: bad size of level %d", li);
        CLSLAM_REQUIRE(desc->offset[li] >= 0 && desc->offset[li] + 3ll * desc->h[li] * desc->w[li] <= desc->slot_bytes,
                       "ring_gather: level %d leaves the slot", li);
        most = std::max(most, desc->h[li] * desc->w[li]);
    }
    for (int fi = 0; fi < desc->n_frames; ++fi)
        CLSLAM_REQUIRE(desc->slot[fi] >= 0 && desc->slot[fi] < desc->capacity, "ring_gather: frame %d in slot %d of a ring of %d", fi,
                       desc->slot[fi], desc->capacity);
    for (int t = 0; t < desc->n_frames * desc->n_levels; ++t)
        CLSLAM_REQUIRE(desc->rgb[t] && desc->aug[t] && desc->rgb[t] != desc->aug[t], "ring_gather: bad destination of table entry %d", t);
    const int blocks = std::max(1, std::min(256, clslam::cdiv(most, 4 * 256)));
    hipLaunchKernelGGL(clslam::ring_gather_kernel, dim3(blocks, desc->n_frames, desc->n_levels), dim3(256), 0, (hipStream_t)stream, *desc,
                       ring);
    return clslam::check_launch("ring_gather");
}
