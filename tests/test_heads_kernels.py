"""The two output heads one kernel at a time: dispconv_fwd, dispconv_bwd_data, dispconv_wgrad (+ reduce_partials),
pose_head_fwd and pose_head_bwd of csrc/heads.hip and the fused head-gradient path of fold_act_grad (disp_dz / disp_w,
csrc/conv_bwd.hip) through their `ops` wrappers, on inputs this file constructs and buffers pre-filled with NaN, against the
float64 restatement of tests/heads_reference.py.  Conventions as documented at the top of tests/test_loss_kernels.py and
tests/test_conv_layers.py; every output lies in a buffer with a tail of 64 sentinel floats that must come back untouched.

Inputs: unit-variance noise times a per-input-channel gain over two decades; a spread over two decades per output channel: the
filter columns for the data gradients (channel of dx), the image amplitudes for the disparity and dz, the rows of w2 / the
columns of dpose for the pose head.  The pose head's x is a ReLU output with about 5 % exact zeros (one case: a channel that is
0 everywhere); dpose is non-zero in all 12 columns.  Seeds are integers derived from the shape.

Bounds, of three kinds:
  * identities: a second launch == the first; dispconv_bwd_data(accumulate=True) on a zeroed buffer == accumulate=False; a block
    of dispconv_wgrad that owns no pixel writes a partial row of exactly 0; pose_head_bwd's dz1 is exactly 0 where x <= 0, does
    not depend on grad_scale, and dw2 / db2 at grad_scale = 0.5, 0.25 are bitwise fp32(s * value at 1.0) (2 ulp at 1/3); a
    saturated sigmoid stays finite and inside [0, 1]; pose_head_fwd with N = 0 writes nothing;
  * derived, plain sums: |error| <= depth * 2^-24 * sum |term| (Higham, Accuracy and Stability, section 4.2), the depth read off
    the kernel's layout and stated in the test's docstring: pose_head_fwd's mean, db2, the bias partials of dispconv_wgrad;
  * measured: largest absolute error over the tensor and relative L2 per output channel (per channel of dx / dw, per image for
    the disparity, per output row for the pose head) against float64, at most 4 x the figure of the same restatement in torch
    float32 (formed first; median-channel fallback: test_conv_layers._measured).

Cases.  dispconv_fwd, per C in 16 / 32 / 64 / 128 (tiles 32x8, 32x4, 16x4, 8x4): 2x2 (both neighbours reflect onto the same
pixel), 3x5 with B = 2, exactly one tile, 2 x 2 tiles plus a ragged row and column; biases of +-30 on the 3x5 case.
dispconv_bwd_data and the plain fold after it: C = 16, 4 (one lane per pixel), 12 (256 / 3 lanes: not a divisor), 256; a grid
beyond the 4096-block cap on the device only.  The fused fold: 2x2, 3x4, 4x4 (no pixel takes the fast path), 5x5 (exactly one
does), 9x40, alone and on top of an upstream padded gradient.  dispconv_wgrad: the same channel counts, 130 pixels = 2 blocks of
65, and on the device only 131,841 pixels = 1024 blocks of 129 of which the last owns nothing.  Pose head: HW = 1, 2, 3, 5 (pixel
lanes without a pixel, a ragged last pass), the engine's 10 x 120 and the 4 x 8 of tests/test_heads_stem.py.

Measured figures (kernel | torch fp32, against float64), the worst case of each quantity; emu = kernel sources on the CPU
emulator, hip = gfx950 (printed per case with -s); sum rows = largest error as a fraction of the derived bound:
  quantity                              emu kernel | fp32   (ratio)        hip kernel | fp32   (ratio)
  dispconv_fwd disp max                   4.60e-07 |  2.15e-07 (2.14x)       4.84e-08 |  2.36e-08 (2.05x)
  dispconv_fwd disp per image rel L2      5.17e-08 |  2.64e-08 (1.96x)       5.17e-08 |  2.92e-08 (1.77x)
  bwd_data dxp max                        3.04e-06 |  1.04e-06 (2.92x)       3.04e-06 |  1.04e-06 (2.92x)
  bwd_data dxp channel rel L2             5.58e-08 |  4.57e-08 (1.22x)       5.58e-08 |  4.57e-08 (1.22x)
  bwd_data dxp += max                     1.49e-05 |  1.12e-05 (1.33x)       1.49e-05 |  1.12e-05 (1.33x)
  bwd_data dxp += channel rel L2          5.31e-08 |  4.49e-08 (1.18x)       5.31e-08 |  4.49e-08 (1.18x)
  bwd_data folded max                     3.87e-06 |  1.85e-06 (2.09x)       3.87e-06 |  1.85e-06 (2.09x)
  bwd_data folded channel rel L2          3.43e-07 |  2.15e-07 (1.60x)       3.43e-07 |  2.15e-07 (1.60x)
  fold+head alone max                     2.74e-05 |  1.54e-05 (1.78x)       2.74e-05 |  1.54e-05 (1.78x)
  fold+head alone channel rel L2          7.92e-08 |  6.53e-08 (1.21x)       7.92e-08 |  6.53e-08 (1.21x)
  fold+head on dxp max                    3.16e-05 |  1.63e-05 (1.94x)       3.16e-05 |  1.63e-05 (1.94x)
  fold+head on dxp channel rel L2         1.89e-07 |  1.16e-07 (1.63x)       1.89e-07 |  1.16e-07 (1.63x)
  wgrad dw max                            8.71e-06 |  2.73e-06 (3.19x)       8.65e-05 |  5.60e-05 (1.54x)
  wgrad dw channel rel L2                 2.15e-07 |  1.15e-07 (1.87x)       1.74e-07 |  7.90e-08 (2.20x)
  wgrad db per block sum error / bound    0.012                              0.027
  wgrad db sum error / derived bound      0.005                              0.005
  pose_head_fwd mean sum error / bound    0.379                              0.379
  pose_head_fwd pose max                  1.72e-08 |  1.19e-08 (1.45x)       2.46e-08 |  2.01e-08 (1.22x)
  pose_head_fwd pose per row rel L2       9.42e-08 |  8.21e-08 (1.15x)       1.05e-07 |  1.26e-07 (0.83x)
  pose_head_bwd dz1 max                   6.13e-11 |  6.13e-11 (1.00x)       6.13e-11 |  6.13e-11 (1.00x)
  pose_head_bwd dz1 per image rel L2      8.82e-08 |  8.82e-08 (1.00x)       8.83e-08 |  8.83e-08 (1.00x)
  pose_head_bwd dw2 max                   9.30e-08 |  9.30e-08 (1.00x)       9.30e-08 |  9.30e-08 (1.00x)
  pose_head_bwd dw2 per row rel L2        7.18e-08 |  7.18e-08 (1.00x)       7.18e-08 |  7.18e-08 (1.00x)
  pose_head_bwd db2 sum error / bound     0.357                              0.293
  (the case with the largest ratio; the hip column includes the device-only cases.  The backward pass of the pose head rounds
  in the order of torch's fp32 evaluation: the same figures.)

One-line mutations of the kernel sources (CPU emulator, scratch copies) and the test of this file that fails; "before" = whether
tests/test_heads_stem.py caught it on the emulator:
  heads.hip     pose_head_bwd: `* gscale` dropped from dw2
                     test_pose_head_bwd: all 6 cases                                                     before: no
  heads.hip     pose_head_bwd: `* gscale` dropped from db2
                     test_pose_head_bwd: all 6 cases                                                     before: no
  heads.hip     pose_head_fwd: `/ (float)HW` dropped from the mean
                     test_pose_head_fwd: the 5 cases with HW > 1                                         before: yes (through pose)
  heads.hip     pose_head_fwd stores `mean` before the division, pose_head_bwd divides what it reads (two lines: the pair stays
                consistent, only the `mean` output is wrong)
                     test_pose_head_fwd, test_pose_head_bwd: the 5 cases with HW > 1 each                before: no (mean never asserted)
  heads.hip     pose_head_bwd: `xv.x > 0.f` -> `>= 0.f`
                     test_pose_head_bwd: all 6 cases (dz1 is not 0 at x == 0)                            before: yes (half of its x are exact zeros)
  heads.hip     pose_head_fwd: `p += 4` -> `p += 3`
                     test_pose_head_fwd[2-5], [10-120], [4-8] (HW <= 3: every lane has at most one pixel)  before: yes
  heads.hip     dispconv_wgrad_kernel: reflect_idx -> a clamp (rows and columns)
                     test_dispconv_wgrad: all 6 cases                                                    before: yes
  conv_bwd.hip  fold fast path: `dw[8 - t]` -> `dw[t]`
                     test_fold_with_the_head_gradient[5-5-*], [9-40-*] (no fast-path pixel below 5x5)    before: yes
  conv_bwd.hip  fold border path: `dw[(2 - ky) * 3 + (2 - kx)]` -> `dw[ky * 3 + kx]`
                     test_fold_with_the_head_gradient: 3x4, 4x4, 5x5, 9x40 (2x2: see below)              before: yes
                     (at 2x2 every pixel folds all nine taps of every dz: the flipped filter gives the same sum -- equivalent there)
  heads.hip     dispconv_bwd_data_kernel: `accumulate` ignored
                     test_dispconv_bwd_data: all 4 cases                                                 before: yes
  Fixed with this file: clslam_pose_head_fwd refused N = 0 ("pose_head_fwd: null", an empty tensor has no storage) instead of
  returning at once like the other entry points: test_pose_head_fwd_without_images_is_a_no_op.
"""
import pytest
import torch

import heads_reference as R
from clslam_hip import ops
from emu_util import BACKENDS, use_backend
from test_conv_layers import _flush, _measured, _sum_bound
from test_stem_kernels import GPU_ONLY, _decades, guarded

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
BOTH = ((F64, F32))


def _cdiv(a, b):
    return -(-a // b)


def _head_inputs(seed, B, H, W, C, spread_w):
    """x (B,H,W,C), w (9,C), dz (B,H,W): per-input-channel gain over two decades on x, image amplitudes over two decades on x and
    dz; spread_w: the filter columns carry the two decades of the channels of dx, else the filter is normalised to z ~ N(0, 1) at
    amplitude 1"""
    g = torch.Generator().manual_seed(seed)
    gain, amp = _decades(g, C), _decades(g, B).view(B, 1, 1)
    x = (torch.randn(B, H, W, C, generator=g) * gain * amp.unsqueeze(-1)).contiguous()
    w = torch.randn(9, C, generator=g) / 3.0
    w = (w * _decades(g, C) if spread_w else w / (C ** 0.5 * float(gain.square().mean().sqrt()))).contiguous()
    dz = (torch.randn(B, H, W, generator=g) * amp).contiguous()
    return x, w, dz


# ---- dispconv_fwd ---------------------------------------------------------------------------------------------------------------
FWD_TILES = {16: (32, 8), 32: (32, 4), 64: (16, 4), 128: (8, 4)}


def _fwd_cases():
    cases = []
    for C, (tw, th) in FWD_TILES.items():
        for B, H, W, sat in ((1, 2, 2, False), (2, 3, 5, True), (1, th, tw, False), (1, 2 * th + 1, 2 * tw + 1, False)):
            cases.append(pytest.param(B, H, W, C, sat, id=f'B{B}-{H}x{W}x{C}'))
    return cases


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,C,sat', _fwd_cases())
def test_dispconv_fwd(backend, B, H, W, C, sat, capsys):
    """per image: largest error and relative L2 of the disparity; with biases of +30 and -30 (sat) also finite and in [0, 1]"""
    dev = use_backend(backend)
    x, w, _ = _head_inputs(100 * C + 10 * H + W, B, H, W, C, False)
    xd, wd = x.to(dev), w.to(dev)
    for bv in (0.3, 30.0, -30.0) if sat else (0.3,):
        bias = torch.tensor([bv])
        ref64, ref32 = (R.dispconv(x, w, bias, dt) for dt in BOTH)
        assert ref64.shape == (B, H, W)
        outs = []
        for _ in range(2):
            out, tail_ok = guarded((B, H, W), dev)
            ops.dispconv_fwd(xd, wd, bias.to(dev), out)
            tail_ok()
            outs.append(out.cpu())
        assert not torch.isnan(outs[0]).any(), 'a pixel was not written'
        assert bool(((outs[0] >= 0) & (outs[0] <= 1)).all())
        per_image = lambda t: t.permute(1, 2, 0)      # noqa: E731
        _measured(backend, f'dispconv_fwd B{B} {H}x{W}x{C} bias {bv:+.1f}', 'disp', per_image(outs[0]), per_image(ref64), per_image(ref32))
        assert torch.equal(outs[0], outs[1])
    _flush(capsys)


# ---- dispconv_bwd_data + the plain fold -----------------------------------------------------------------------------------------
def _bwd_data_check(backend, B, H, W, C, capsys):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(7000 + 10 * H + W + C)
    _, w, dz = _head_inputs(200 * C + 10 * H + W, B, H, W, C, True)
    base = torch.randn(B, H + 2, W + 2, C, generator=g).contiguous()
    dxp64, dxp32 = (R.dispconv_dxp(dz, w, dt) for dt in BOTH)
    dx64, dx32 = R.fold(dxp64), R.fold(dxp32)
    acc64, acc32 = base.double() + dxp64, base + dxp32
    assert dxp64.shape == (B, H + 2, W + 2, C)
    dzd, wd = dz.to(dev), w.to(dev)
    name = f'bwd_data B{B} {H}x{W}x{C}'

    def launch(fill, accumulate):
        dxp, tail_ok = guarded((B, H + 2, W + 2, C), dev)
        if fill is not None:
            dxp.copy_(fill)
        ops.dispconv_bwd_data(dzd, wd, dxp, C, accumulate=accumulate)
        tail_ok()
        return dxp

    plain = launch(None, False)
    got = plain.cpu()
    assert not torch.isnan(got).any(), 'a padded position was not written'
    _measured(backend, name, 'dxp', got, dxp64, dxp32)
    assert torch.equal(got, launch(None, False).cpu())
    assert torch.equal(got, launch(torch.zeros_like(base), True).cpu()), 'accumulate on a zeroed buffer differs from overwrite'
    _measured(backend, name, 'dxp +=', launch(base, True).cpu(), acc64, acc32)
    dx, tail_ok = guarded((B, H, W, C), dev)
    ops.fold_act_grad(plain, None, dx, h=H, w=W, ch=C, border=1, pool=False, act=0)
    tail_ok()
    assert not torch.isnan(dx.cpu()).any()
    _measured(backend, name, 'folded', dx.cpu(), dx64, dx32)
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,C', [(2, 2, 2, 16), (1, 3, 4, 4), (1, 5, 6, 12), (2, 9, 11, 256)])
def test_dispconv_bwd_data(backend, B, H, W, C, capsys):
    """the padded-domain gradient overwriting a NaN buffer and accumulating onto a non-zero one, and clslam_fold_act_grad on it"""
    _bwd_data_check(backend, B, H, W, C, capsys)


@pytest.mark.parametrize('backend', GPU_ONLY)
def test_dispconv_bwd_data_beyond_the_grid_cap(backend, capsys):
    """(1,190,350,64): 192 x 352 x 16 = 1,081,344 quads > 4096 x 256: the grid-stride loop runs a second, ragged time"""
    assert 192 * 352 * 16 == 1081344 > 4096 * 256
    _bwd_data_check(backend, 1, 190, 350, 64, capsys)


# ---- fold_act_grad with the fused head gradient ---------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('C', [16, 128])
@pytest.mark.parametrize('H,W', [(2, 2), (3, 4), (4, 4), (5, 5), (9, 40)])
def test_fold_with_the_head_gradient(backend, H, W, C, capsys):
    """B = 2.  The fast path needs 2 <= y <= H - 3 and 2 <= x <= W - 3: nobody up to 4x4, pixel (2, 2) alone at 5x5."""
    dev = use_backend(backend)
    B = 2
    fast = max(0, H - 4) * max(0, W - 4)
    assert fast == {(2, 2): 0, (3, 4): 0, (4, 4): 0, (5, 5): 1, (9, 40): 180}[H, W]
    g = torch.Generator().manual_seed(9000 + 10 * H + W + C)
    _, w, dz = _head_inputs(300 * C + 10 * H + W, B, H, W, C, True)
    up = (torch.randn(B, H + 2, W + 2, C, generator=g) * _decades(g, C)).contiguous()
    name = f'fold+head {H}x{W}x{C}'
    dzd, wd, upd = dz.to(dev), w.to(dev), up.to(dev)
    for what, src, srcd in (('alone', None, None), ('on dxp', up, upd)):
        ref64, ref32 = (R.fold(R.dispconv_dxp(dz, w, dt) + (0 if src is None else src.to(dt))) for dt in BOTH)
        outs = []
        for _ in range(2):
            dx, tail_ok = guarded((B, H, W, C), dev)
            ops.fold_act_grad(srcd, None, dx, h=H, w=W, ch=C, border=1, pool=False, act=0, disp_dz=dzd, disp_w=wd)
            tail_ok()
            outs.append(dx.cpu())
        assert not torch.isnan(outs[0]).any(), 'a pixel was not written'
        _measured(backend, name, what, outs[0], ref64, ref32)
        assert torch.equal(outs[0], outs[1])
    _flush(capsys)


# ---- dispconv_wgrad + reduce_partials -------------------------------------------------------------------------------------------
def _wgrad_check(backend, B, H, W, C, capsys):
    dev = use_backend(backend)
    x, _, dz = _head_inputs(400 * C + 10 * H + W, B, H, W, C, False)
    pixels = B * H * W
    nb = ops.dispconv_wgrad_blocks(pixels)
    assert nb == max(1, min(1024, _cdiv(pixels, 128)))
    ppb, lanes, n = _cdiv(pixels, nb), 256 // (C // 4), 9 * C + 1
    dw64, _ = R.dispconv_wgrad(dz, x, F64)
    dw32, _ = R.dispconv_wgrad(dz, x, F32)
    name = f'wgrad B{B} {H}x{W}x{C} ({nb} x {ppb})'
    xd, dzd = x.to(dev), dz.to(dev)
    outs = []
    for _ in range(2):
        part, tail_ok = guarded((nb * n,), dev)              # exactly dispconv_wgrad_blocks(...) * (9C + 1) floats
        ops.dispconv_wgrad(dzd, xd, part)
        tail_ok()
        gw, gw_ok = guarded((n,), dev)
        ops.reduce_partials(part, gw, n, nb)
        gw_ok()
        outs.append((part.cpu().view(nb, n), gw.cpu()))
    part, gw = outs[0]
    assert not torch.isnan(part).any(), 'a partial was not written'
    owned = torch.zeros(nb * ppb, dtype=F32)
    owned[:pixels] = dz.reshape(-1)
    owned = owned.view(nb, ppb)                                    # row = the pixels of a block, zero where it owns none
    for blk in range(nb):
        if blk * ppb >= pixels:
            assert bool((part[blk] == 0).all()), ('a block without pixels wrote a non-zero partial', blk)
    _sum_bound(backend, name, 'db blocks', part[:, 9 * C], owned.t(), _cdiv(ppb, lanes) + lanes)
    _sum_bound(backend, name, 'db', gw[9 * C:], dz.reshape(-1, 1), _cdiv(ppb, lanes) + lanes + _cdiv(nb, 4) + 16)
    _measured(backend, name, 'dw', gw[:9 * C].view(9, C), dw64, dw32)
    assert torch.equal(part, outs[1][0]) and torch.equal(gw, outs[1][1])
    _flush(capsys)
    return part


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,C', [(1, 2, 2, 16), (2, 7, 9, 64), (1, 5, 6, 12), (1, 4, 4, 4), (1, 6, 5, 256), (1, 10, 13, 32)])
def test_dispconv_wgrad(backend, B, H, W, C, capsys):
    """A block's bias partial is a plain sum: a pixel lane (256 / (C / 4) of them) adds ceil(pixels per block / lanes) values,
    thread 0 then adds the lanes one after the other: depth = ceil(ppb / lanes) + lanes; reduce_partials adds
    ceil(blocks / 4) + 16 (tests/test_conv_layers.py).  dw per channel c against 4 x fp32.  (1,10,13,32): 130 pixels = 2 blocks
    of 65."""
    if (B, H, W) == (1, 10, 13):
        assert ops.dispconv_wgrad_blocks(130) == 2
    _wgrad_check(backend, B, H, W, C, capsys)


@pytest.mark.parametrize('backend', GPU_ONLY)
def test_dispconv_wgrad_with_an_empty_block(backend, capsys):
    """(1,257,513,16): 131,841 pixels -> 1024 blocks of 129; block 1022 owns 3 pixels, block 1023 none: its row is exactly 0"""
    assert 257 * 513 == 131841 and _cdiv(131841, 1024) == 129 and 1023 * 129 > 131841 > 1022 * 129
    part = _wgrad_check(backend, 1, 257, 513, 16, capsys)
    assert part.shape[0] == 1024 and bool((part[1023] == 0).all())


# ---- pose head ------------------------------------------------------------------------------------------------------------------
POSE_SHAPES = {(1, 1): (1, 1), (2, 2): (1, 2), (3, 3): (1, 3), (2, 5): (1, 5), (10, 120): (6, 20), (4, 8): (2, 4)}


def _pose_inputs(N, HW):
    H, W = POSE_SHAPES[N, HW]
    g = torch.Generator().manual_seed(500 * N + HW)
    gain = _decades(g, 256)
    x = (torch.relu(torch.randn(N, H, W, 256, generator=g) + 1.645) * gain).contiguous()       # P(N(0,1) < -1.645) = 5 %
    if (N, HW) == (2, 5):
        x[..., 17] = 0.0                                                                       # a channel that is 0 everywhere
    rows = _decades(g, 12)
    # x >= 0, so a filter row with a common-mode part (as a trained one has) makes pose[n][o] a well-conditioned sum: at N = 1 an
    # output row is ONE number, and a row that cancels to a fraction of its terms would compare two single draws of that noise
    w2 = ((1.0 + torch.randn(12, 256, generator=g)) * rows.view(12, 1) / (256 * float(gain.mean()))).contiguous()
    b2 = (0.1 * rows * torch.randn(12, generator=g)).contiguous()
    dpose = (torch.randn(N, 12, generator=g) * _decades(g, 12)).contiguous()
    assert bool((dpose != 0).all())
    return x, w2, b2, dpose


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('N,HW', list(POSE_SHAPES))
def test_pose_head_fwd(backend, N, HW, capsys):
    """mean: four pixel lanes add ceil(HW / 4) values each, three additions combine them, one division: depth = ceil(HW / 4) + 4.
    pose per output row against 4 x fp32."""
    dev = use_backend(backend)
    x, w2, b2, _ = _pose_inputs(N, HW)
    zeros = float((x == 0).double().mean())
    assert 0.02 < zeros < 0.09, zeros
    (_, p64), (_, p32) = (R.pose_head(x, w2, b2, dt) for dt in BOTH)
    outs = []
    for _ in range(2):
        mean, mean_ok = guarded((N, 256), dev)
        pose, pose_ok = guarded((N, 12), dev)
        ops.pose_head_fwd(x.to(dev), w2.to(dev), b2.to(dev), mean, pose)
        mean_ok(), pose_ok()
        outs.append((mean.cpu(), pose.cpu()))
    mean, pose = outs[0]
    assert not torch.isnan(mean).any() and not torch.isnan(pose).any()
    for n in range(N):
        _sum_bound(backend, f'pose_head_fwd N{N} HW{HW}', f'mean n{n}', mean[n].double() * HW, x[n].reshape(HW, 256), _cdiv(HW, 4) + 4)
    _measured(backend, f'pose_head_fwd N{N} HW{HW}', 'pose', pose, p64, p32)
    assert torch.equal(mean, outs[1][0]) and torch.equal(pose, outs[1][1])
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
def test_pose_head_fwd_without_images_is_a_no_op(backend):
    dev = use_backend(backend)
    _, w2, b2, _ = _pose_inputs(4, 8)
    mean, mean_ok = guarded((1, 256), dev)
    pose, pose_ok = guarded((1, 12), dev)
    ops.pose_head_fwd(torch.zeros(0, 2, 2, 256, device=dev), w2.to(dev), b2.to(dev), mean, pose)
    mean_ok(), pose_ok()
    assert bool(torch.isnan(mean.cpu()).all()) and bool(torch.isnan(pose.cpu()).all())


def _ulp(t):
    t = t.float().abs()
    return (torch.nextafter(t, torch.full_like(t, float('inf'))) - t).double()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('N,HW', list(POSE_SHAPES))
def test_pose_head_bwd(backend, N, HW, capsys):
    """`mean` is an input: the float64 mean rounded to fp32, not pose_head_fwd's output.  dz1 per image, dw2 per output row
    against 4 x fp32; dz1 exactly 0 where x <= 0.  (dz1[n][p][c] takes one value per (n, c), a 12-term dot product over terms of
    both signs spread over four decades: a channel of dz1 is N numbers -- one at N = 1 -- of heavy-tailed conditioning, an image
    is 256 of them.)  db2[o] = s * sum_n 0.01 dpose[n][o]: the constant 0.01f, the product, N
    additions and the scale: depth N + 3.  grad_scale = 1, 0.5, 0.25, 1/3: dz1 does not move, dw2 / db2 are the values at 1.0 times
    s, bitwise for the powers of two, within 2 ulp for 1/3 (one rounding of s, one of the product)."""
    dev = use_backend(backend)
    x, w2, _, dpose = _pose_inputs(N, HW)
    H, W = POSE_SHAPES[N, HW]
    mean = R.pose_head(x, w2, torch.zeros(12), F64)[0].float().contiguous()
    xd, w2d, dpd, md = x.to(dev), w2.to(dev), dpose.to(dev), mean.to(dev)
    name = f'pose_head_bwd N{N} HW{HW}'

    def launch(s):
        dz1, a_ok = guarded((N, H, W, 256), dev)
        dw2, b_ok = guarded((12, 256), dev)
        db2, c_ok = guarded((12,), dev)
        if s is None:
            ops.pose_head_bwd(dpd, xd, w2d, md, dz1, dw2, db2)
        else:
            ops.pose_head_bwd(dpd, xd, w2d, md, dz1, dw2, db2, grad_scale=s)
        a_ok(), b_ok(), c_ok()
        got = dz1.cpu(), dw2.cpu(), db2.cpu()
        assert not any(bool(torch.isnan(t).any()) for t in got), 'an output element was not written'
        return got

    def against_float64(got, s, tag):
        ref64, ref32 = (R.pose_head_bwd(dpose, x, w2, mean, s, dt) for dt in BOTH)
        per_image = lambda t: t.permute(1, 2, 3, 0)      # noqa: E731
        _measured(backend, name, f'dz1{tag}', per_image(got[0]), per_image(ref64[0]), per_image(ref32[0]))
        _measured(backend, name, f'dw2{tag}', got[1].t(), ref64[1].t(), ref32[1].t())
        _sum_bound(backend, name, f'db2{tag}', got[2], s * 0.01 * dpose.double(), N + 3)

    one = launch(None)
    against_float64(one, 1.0, '')
    assert bool((one[0][x <= 0] == 0).all()), "relu'(0) must be 0"
    assert bool((one[0][x > 0] != 0).any())
    for s in (1.0, 0.5, 0.25, 1.0 / 3.0):
        got = launch(s)
        assert torch.equal(got[0], one[0]), ('dz1 depends on grad_scale', s)
        if s == 1.0 / 3.0:
            against_float64(got, s, ' s=1/3')
            for k in (1, 2):
                want = one[k].double() / 3.0
                assert bool(((got[k].double() - want).abs() <= 2 * _ulp(want)).all()), (('dw2', 'db2')[k - 1], s)
        else:
            assert torch.equal(got[1], one[1] * s) and torch.equal(got[2], one[2] * s), ('dw2 / db2 are not s * the value at 1.0', s)
    _flush(capsys)
