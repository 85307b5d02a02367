"""TEST INFRASTRUCTURE: a plain restatement of the encoder entry and of the two output heads of cl-slam_amd/csrc
(encoder_ops.hip, heads.hip, the disp_dz / disp_w path of fold_act_grad in conv_bwd.hip), from the formulas in the header
comments of those files and the lines of the reference network they cite:

    stem            relu(scale * conv7x7_s2_p3((cat(img_a, img_b) - 0.45) / 0.225) + shift): the padding is zero padding of the
                    NORMALISED tensor (resnet_encoder.py:117-120), NHWC output
    pack_weight     packed[pass][co][k] = w[co][pass * 3 + k / 49][k % 49] for k < 147, two zero columns per row of 149
    maxpool         3x3, stride 2, pad 1: a tap outside the image is no tap (resnet_encoder.py:121)
    dispconv        sigmoid(bias + conv3x3(reflection_pad1(x))) to one channel (depth_decoder.py:67-69, layers.py:28-48)
    dispconv_dxp    its data gradient on the padded domain: dxp[P] = sum_tap dz[P - tap] * w[tap]
    fold            the adjoint of the reflection padding: padded row 0 lands on row 1, padded row H + 1 on row H - 2
    dispconv_wgrad  dw[tap][c] = sum_pixels dz * xpad(tap shifted), db = sum dz
    pose_head       mean over the pixels -> 12x256 matvec + bias -> x 0.01 (pose_decoder.py:44-54: the 1x1 conv and the mean
                    commute)
    pose_head_bwd   dz1 = relu'(x) * (0.01 dpose w2) / HW, dw2 = s * (0.01 dpose)^T mean, db2 = s * sum_n 0.01 dpose

Everything is loop-free torch evaluated in `dtype`: float64 is the reference, float32 the yardstick ("what the same formula
loses in the kernel's own number format").  Activations are NHWC, the disparity filter is (9, C) = [tap][c].  Nothing here runs
on the device."""
import torch
import torch.nn.functional as F

STEM_K, STEM_LDW = 147, 149


def stem(imgs, w, scale, shift, dtype):
    """imgs: one or two planar (B,3,H,W) images; w OIHW (64, 3 n_img, 7, 7) -> (B,Ho,Wo,64)"""
    x = (torch.cat([i.to(dtype) for i in imgs], 1) - 0.45) / 0.225
    y = F.conv2d(x, w.to(dtype), stride=2, padding=3)
    y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


def pack_weight(w):
    """(64, 3 n_img, 7, 7) -> flat (n_img * 64 * 149): one slab of [64][149] per group of three input channels"""
    n_img = w.shape[1] // 3
    slab = w.reshape(64, n_img, STEM_K).permute(1, 0, 2)
    return F.pad(slab, (0, STEM_LDW - STEM_K)).reshape(-1).contiguous()


def maxpool(x, dtype):
    """NHWC -> NHWC; max_pool2d pads with "no tap" (-inf)"""
    return F.max_pool2d(x.to(dtype).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def _filter(w, dtype):
    """(9, C) [tap][c] -> (1, C, 3, 3)"""
    C = w.shape[1]
    return w.to(dtype).view(3, 3, C).permute(2, 0, 1).unsqueeze(0)


def _reflect_pad(x, dtype):
    return F.pad(x.to(dtype).permute(0, 3, 1, 2), (1, 1, 1, 1), mode='reflect')


def dispconv(x, w, bias, dtype):
    """x (B,H,W,C), w (9,C), bias (1,) -> (B,H,W)"""
    return torch.sigmoid(F.conv2d(_reflect_pad(x, dtype), _filter(w, dtype), bias.to(dtype)))[:, 0].contiguous()


def dispconv_dxp(dz, w, dtype):
    """dz (B,H,W) -> the gradient with respect to the reflection-PADDED input, (B,H+2,W+2,C)"""
    return F.conv_transpose2d(dz.to(dtype).unsqueeze(1), _filter(w, dtype)).permute(0, 2, 3, 1).contiguous()


def fold(dxp):
    """(B,H+2,W+2,C) padded-domain gradient -> (B,H,W,C): every padded position added to the pixel it mirrors"""
    B, Hp, Wp, C = dxp.shape
    H, W = Hp - 2, Wp - 2

    def mirror(n):
        i = torch.arange(-1, n + 1)
        return torch.where(i < 0, -i, torch.where(i > n - 1, 2 * (n - 1) - i, i))

    rows = torch.zeros(B, H, Wp, C, dtype=dxp.dtype).index_add_(1, mirror(H), dxp)
    return torch.zeros(B, H, W, C, dtype=dxp.dtype).index_add_(2, mirror(W), rows)


def dispconv_dx(dz, w, dtype):
    return fold(dispconv_dxp(dz, w, dtype))


def dispconv_wgrad(dz, x, dtype):
    """dz (B,H,W), x (B,H,W,C) -> dw (9, C), db ()"""
    B, H, W, C = x.shape
    xp = _reflect_pad(x, dtype)                                            # (B,C,H+2,W+2)
    win = torch.stack([xp[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 0)     # (9,B,C,H,W)
    g = dz.to(dtype)
    return torch.einsum('tbcyx,byx->tc', win, g), g.sum()


def pose_head(x, w2, b2, dtype):
    """x (N,H,W,256) -> mean (N,256), pose (N,12)"""
    N = x.shape[0]
    mean = x.to(dtype).reshape(N, -1, 256).mean(1)
    return mean, 0.01 * (mean @ w2.to(dtype).t() + b2.to(dtype))


def pose_head_bwd(dpose, x, w2, mean, grad_scale, dtype):
    """mean is an INPUT (what the forward pass stored) -> dz1 (N,H,W,256), dw2 (12,256), db2 (12,)"""
    N, H, W, _ = x.shape
    g = 0.01 * dpose.to(dtype)
    dmean = (g @ w2.to(dtype)) / (H * W)
    dz1 = torch.where(x.to(dtype) > 0, dmean.view(N, 1, 1, 256).expand(N, H, W, 256), torch.zeros((), dtype=dtype))
    return dz1.contiguous(), grad_scale * (g.t() @ mean.to(dtype)), grad_scale * g.sum(0)
