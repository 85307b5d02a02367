// What the convolution kernels share (conv_fwd.hip, conv_patch.hip, conv_sk.hip, conv_wino.hip, conv_bwd.hip): the operand block
// of a launch, the geometry predicates of the picker and the dispatchers, the timed launch, the MFMA accumulator row mapping
// and the fused epilogue of the kernels whose lanes run along the output channels.
#pragma once
#include "common.h"

#include <type_traits>

namespace clslam {

// ---- operands of one convolution launch, as every forward kernel receives them ----------------
// Packed (4-byte aligned, 116 bytes): as a plain base the struct would end in four bytes of padding, the ints of the structs
// derived from it would start at byte 120, and the kernel-argument block would have a hole nobody reads -- hipcc then fetches the
// arguments of the patch kernels with seven scalar loads instead of three.  Every pointer still sits on an 8-byte boundary of the
// kernel-argument block, but the type no longer says so: read and assign the members, never bind a reference or a pointer to one.
// A struct that derives from it pins its layout with CLSLAM_FOLLOWS_CONV_OPERANDS(Type, its first own field).
struct __attribute__((packed, aligned(4))) ConvOperands {
    const float* __restrict__ src_a;
    const float* __restrict__ src_b;
    const float* __restrict__ wgt;
    const float* __restrict__ scale;
    const float* __restrict__ shift;
    const float* __restrict__ residual;
    const float* __restrict__ actgrad_src;
    float* __restrict__ out;
    int actgrad_kind;
    int B, Hi, Wi, Ca, Cb, Ho, Wo, Cout;
    int pad, pad_mode, ups, act;
};
static_assert(sizeof(ConvOperands) == 116, "the fields of a derived struct follow at byte 116, without a gap");

// (offsetof into a struct with a base class is what clang warns about and supports)
#define CLSLAM_FOLLOWS_CONV_OPERANDS(Type, field)                                                                  \
    _Pragma("clang diagnostic push") _Pragma("clang diagnostic ignored \"-Winvalid-offsetof\"")                    \
    static_assert(__builtin_offsetof(Type, field) == sizeof(ConvOperands), #Type ": gap behind the shared operands"); \
    _Pragma("clang diagnostic pop")

inline ConvOperands conv_operands(const clslam_conv_desc* d) {
    ConvOperands k;
    k.src_a = d->src_a; k.src_b = d->src_b; k.wgt = d->weight; k.scale = d->scale; k.shift = d->shift;
    k.residual = d->residual; k.actgrad_src = d->actgrad_src; k.out = d->out; k.actgrad_kind = d->actgrad_kind;
    k.B = d->batch; k.Hi = d->in_h; k.Wi = d->in_w; k.Ca = d->ch_a; k.Cb = d->ch_b; k.Ho = d->out_h; k.Wo = d->out_w;
    k.Cout = d->ch_out; k.pad = d->pad; k.pad_mode = d->pad_mode; k.ups = d->upsample_a; k.act = d->act;
    return k;
}

// ---- geometry predicates ---------------------------------------------------------------------
// the output size is the one the input size, kernel size, stride and padding give
inline bool conv_size_consistent(const clslam_conv_desc* d) {
    return d->stride >= 1 && d->out_h == (d->in_h + 2 * d->pad - d->ksize) / d->stride + 1 &&
           d->out_w == (d->in_w + 2 * d->pad - d->ksize) / d->stride + 1;
}

// a 3x3 convolution of the given stride with a consistent output size: what the patch, stream-K and Winograd kernels serve
inline bool same_size_3x3(const clslam_conv_desc* d, int stride) {
    return d->ksize == 3 && d->stride == stride && conv_size_consistent(d);
}

// ---- timed launch ----------------------------------------------------------------------------
// While the measurement hook is armed (profile_next_events, common.h) the launch carries its own start / stop events.
template <typename F, typename Arg>
inline void conv_launch(F kernel, int nblk, int threads, hipStream_t stream, const Arg& k) {
#if CLSLAM_DEVICE_BUILD
    hipEvent_t e0, e1;
    if (profile_next_events(&e0, &e1)) {
        hipExtLaunchKernelGGL(kernel, dim3(nblk), dim3(threads), 0, stream, e0, e1, 0, k);
        return;
    }
#endif
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(threads), 0, stream, k);
}

// ---- MFMA accumulator layout -----------------------------------------------------------------
// row of an MF x MF accumulator tile that register r of this lane holds (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32);
// the column is lane % MF
template <int MF>
__device__ __forceinline__ int acc_row(int lane, int r) {
    if constexpr (MF == 32) return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    else return 4 * (lane >> 4) + r;
}

// ---- fused epilogue: BN / bias, residual, activation, activation gradient, NHWC store ----------
// For the kernels whose lanes run along the output channels (conv_igemm_kernel, conv3x3_patch_kernel); the persistent kernels
// (conv_sk.hip, conv_wino.hip, wgrad_patch.hip) hold four consecutive channels of one pixel per lane and have a float4 form.
//
//   out = act(acc * scale + shift + residual) * act_grad(actgrad_src)
//
// over the lane's TM x TN x NACC accumulator slots.  acc_at(i, j, r) is the raw accumulator of slot (tile row i, tile column j,
// register r), element(i, j, r, ok) its offset in out / residual / actgrad_src CLAMPED into the tensor, with ok = the slot is a
// real output.  sc / sh are the lane's scale and shift per tile column.  PRE_RES: the caller has fetched the residual already
// (pre_res[(i * TN + j) * NACC + r], zeros where there is none; without PRE_RES a one-element dummy).  A0, A1, A2: the order in
// which the activation is tested.
//
// Three straight-line phases: (1) the optional operands (residual, activation-gradient source) of ALL the lane's elements
// loaded back to back from clamped (always valid) addresses, (2) every value computed with the activation switch OUTSIDE the
// element loop, (3) all stores back to back.  The element-by-element form (load? - value - load? - store per element, the
// activation's branches in between) made hipcc put an `s_waitcnt vmcnt(0)` in front of every load and store: eight serial
// memory round trips per workgroup, ~5 us of its ~11 us life on the 16-channel layers (round 5).
template <int TM, int TN, int NACC, bool PRE_RES, int A0, int A1, int A2, class AccAt, class Element>
__device__ __forceinline__ void fused_epilogue(const ConvOperands& p, const float (&sc)[TN], const float (&sh)[TN],
                                               const float (&pre_res)[PRE_RES ? TM * TN * NACC : 1], const AccAt& acc_at,
                                               const Element& element) {
    float vals[TM][TN][NACC], resq[TM][TN][NACC], agq[TM][TN][NACC];
    const bool has_res = !PRE_RES && p.residual != nullptr, has_ag = p.actgrad_src != nullptr;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < NACC; ++r) {
                if constexpr (PRE_RES) resq[i][j][r] = pre_res[(i * TN + j) * NACC + r];
                else resq[i][j][r] = 0.f;
                agq[i][j][r] = 1.f;
            }
    if (has_res) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < NACC; ++r) { bool ok; resq[i][j][r] = p.residual[element(i, j, r, ok)]; }
    }
    if (has_ag) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < NACC; ++r) { bool ok; agq[i][j][r] = p.actgrad_src[element(i, j, r, ok)]; }
    }
    auto values = [&](auto act_tag) {
        constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < NACC; ++r) {
                    float v = acc_at(i, j, r) * sc[j] + sh[j];
                    v += resq[i][j][r];
                    vals[i][j][r] = ACT < 0 ? apply_act(v, p.act) : apply_act(v, ACT);
                }
    };
    if (p.act == A0) values(std::integral_constant<int, A0>{});
    else if (p.act == A1) values(std::integral_constant<int, A1>{});
    else if (p.act == A2) values(std::integral_constant<int, A2>{});
    else values(std::integral_constant<int, -1>{});
    if (has_ag) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < NACC; ++r) vals[i][j][r] *= act_grad_from_output(agq[i][j][r], p.actgrad_kind);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < NACC; ++r) {
                bool ok;
                const size_t o = element(i, j, r, ok);
                if (ok) p.out[o] = vals[i][j][r];
            }
}

}  // namespace clslam
