"""TEST INFRASTRUCTURE: a plain restatement of the convolution family of cl-slam_amd/csrc (conv_fwd.hip, conv_patch.hip,
conv_sk.hip, conv_wino.hip, conv_bwd.hip, wgrad_patch.hip), from the formula at the head of conv_fwd.hip:

    out[m][n] = act( scale[n] * sum_{tap,c} G(m,tap,c) * W[n][tap][c] + shift[n] (+ residual[m][n]) ) (* act'(actgrad_src))

    gather          G: nearest-2x upsampling of source A, channel concat with source B, zero / reflect padding (any pad: the
                    data-gradient convolutions run on the zero-padded domain with pad = 2)
    conv_forward    the direct form (F.conv2d over the gathered input) or the F(2x2,3x3) Winograd form, + the epilogue
    conv_winograd   the Winograd form alone: V = B^T d B, U = G g G^T, M = sum_c U V, Y = A^T M A (Lavin & Gray 2016)
    conv_backward   dW, the bias gradient and d (pre-activation of source A) by autograd through the direct form: the pool
                    of an upsampled source and the fold of the reflect border are whatever autograd makes of them
    fold            the fold / pool / activation-gradient step alone on a given padded-domain gradient
    transpose_flip  the weights of the data-gradient convolution

Everything is loop-free torch evaluated in `dtype`: float64 is the reference, float32 the yardstick ("what the same formula
loses in the kernel's own number format").  Tensors are NHWC activations and (Cout, k*k, Cin) weights, like the library's.
Nothing here runs on the device."""
import torch
import torch.nn.functional as F

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_ELU, ACT_HSWISH, ACT_HSIGMOID = 0, 1, 2, 3, 4
PAD_ZERO, PAD_REFLECT = 0, 1


def _nchw(t, dtype):
    return None if t is None else t.to(dtype).permute(0, 3, 1, 2)


def act_fn(v, act):
    if act == ACT_HSWISH:                       # common.h apply_act: v * clamp(v + 3, 0, 6) / 6
        return v * torch.clamp(v + 3, 0, 6) / 6
    if act == ACT_HSIGMOID:
        return torch.clamp(v + 3, 0, 6) / 6
    return F.relu(v) if act == ACT_RELU else F.elu(v) if act == ACT_ELU else v


def act_grad_from_output(y, act):
    """derivative of the activation expressed through its OUTPUT (common.h)"""
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == ACT_ELU:
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    return torch.ones_like(y)


def gather(xa, xb=None, *, pad=1, pad_mode=PAD_ZERO, ups=False):
    """NCHW in, NCHW out: upsample A, concat B, pad"""
    x = F.interpolate(xa, scale_factor=2, mode='nearest') if ups else xa
    if xb is not None:
        x = torch.cat([x, xb], 1)
    if pad > 0:
        x = F.pad(x, (pad,) * 4, mode='reflect' if pad_mode == PAD_REFLECT else 'constant')
    return x


def _w_oihw(w, ksize, dtype):
    return w.to(dtype).reshape(w.shape[0], ksize, ksize, -1).permute(0, 3, 1, 2)


# F(2x2,3x3): the transform matrices of Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", section 4.1
_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def conv_winograd(x, w):
    """x: the gathered (padded) input NCHW, w OIHW 3x3, one dtype -> the stride-1 'valid' convolution, tile by tile"""
    dt = x.dtype
    Bt, G, At = (torch.tensor(m, dtype=dt) for m in (_BT, _G, _AT))
    B, C, Hp, Wp = x.shape
    Ho, Wo = Hp - 2, Wp - 2
    th, tw = (Ho + 1) // 2, (Wo + 1) // 2
    x = F.pad(x, (0, 2 * tw + 2 - Wp, 0, 2 * th + 2 - Hp))
    d = x.unfold(2, 4, 2).unfold(3, 4, 2)                               # (B, C, th, tw, 4, 4)
    V = torch.einsum('ik,bcyxkl,jl->bcyxij', Bt, d, Bt)
    U = torch.einsum('ik,ockl,jl->ocij', G, w, G)
    M = torch.einsum('bcyxij,ocij->boyxij', V, U)
    Y = torch.einsum('ik,boyxkl,jl->boyxij', At, M, At)                 # (B, O, th, tw, 2, 2)
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], 2 * th, 2 * tw)[:, :, :Ho, :Wo]


def conv_forward(xa, w, *, xb=None, scale=None, shift=None, residual=None, ksize=3, stride=1, pad=None, pad_mode=PAD_ZERO,
                 ups=False, act=ACT_NONE, actgrad_src=None, actgrad_kind=ACT_NONE, dtype=F64, form='direct'):
    """NHWC tensors as ops.conv2d takes them -> NHWC output in `dtype`; form = 'direct' | 'winograd'"""
    pad = ksize // 2 if pad is None else pad
    x = gather(_nchw(xa, dtype), _nchw(xb, dtype), pad=pad, pad_mode=pad_mode, ups=ups)
    wk = _w_oihw(w, ksize, dtype)
    if form == 'winograd':
        assert ksize == 3 and stride == 1
        y = conv_winograd(x, wk)
    else:
        y = F.conv2d(x, wk, stride=stride)
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(dtype).view(1, -1, 1, 1)
    if residual is not None:
        y = y + _nchw(residual, dtype)
    y = act_fn(y, act)
    if actgrad_src is not None:
        y = y * act_grad_from_output(_nchw(actgrad_src, dtype), actgrad_kind)
    return y.permute(0, 2, 3, 1).contiguous()


def transpose_flip(w, ch_in_sel=None):
    """(Cout, taps, Cin) -> (Cin_sel, taps, Cout), taps reversed: the weights of the data-gradient convolution"""
    sel = w.shape[2] if ch_in_sel is None else ch_in_sel
    return w[:, :, :sel].flip(1).permute(2, 1, 0).contiguous()


def conv_backward(xa, w, dz, *, xb=None, ksize=3, stride=1, pad=None, pad_mode=PAD_ZERO, ups=False, act_a=ACT_NONE, dtype=F64):
    """xa: source A as stored (the OUTPUT of its producer's activation `act_a`), dz: d loss / d (pre-activation output) NHWC.
    -> dW (Cout, k*k, Cin), dbias (Cout), d (pre-activation of source A) NHWC = autograd's d xa times act_a'(xa)"""
    pad = ksize // 2 if pad is None else pad
    a = _nchw(xa, dtype).detach().clone().requires_grad_(True)
    wk = w.to(dtype).detach().clone().requires_grad_(True)
    y = F.conv2d(gather(a, _nchw(xb, dtype), pad=pad, pad_mode=pad_mode, ups=ups), _w_oihw(wk, ksize, dtype), stride=stride)
    y.backward(_nchw(dz, dtype))
    dpre = a.grad * act_grad_from_output(a.detach(), act_a)
    return wk.grad, dz.to(dtype).sum((0, 1, 2)), dpre.permute(0, 2, 3, 1).contiguous()


def fold(dxp, yout, *, border=1, pool=False, act=ACT_NONE, dtype=F64):
    """dxp (B, h + 2 border, w + 2 border, C): a gradient on the reflect-padded domain of (the upsampled, if pool) yout
    -> d (pre-activation of yout) = [pool 2x2 of] [the border folded back] times act'(yout), and its per-channel sums"""
    y = _nchw(yout, dtype)
    a = torch.zeros_like(y).requires_grad_(True)          # the gather is linear: its transpose is what autograd applies
    gather(a, pad=border, pad_mode=PAD_REFLECT, ups=pool).backward(_nchw(dxp, dtype))
    dpre = (a.grad * act_grad_from_output(y, act)).permute(0, 2, 3, 1).contiguous()
    return dpre, dpre.sum((0, 1, 2))


def macs(B, Ho, Wo, Cout, ksize, Cin):
    return B * Ho * Wo * Cout * ksize * ksize * Cin
