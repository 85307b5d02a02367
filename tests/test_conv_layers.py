"""The convolution family (csrc/conv_fwd.hip, conv_patch.hip, conv_sk.hip, conv_wino.hip, conv_bwd.hip, wgrad_patch.hip) at the
shapes the engine really launches, against the float64 restatement of tests/conv_reference.py.  Conventions as documented at
the top of tests/test_loss_kernels.py.

Layer table.  LAYERS is every distinct conv2d the engine launches for one adaptation step, written out from
clslam_hip/engine.py (Engine.pack / _encoder / _depth_decoder / _pose_decoder / _backward_depth_decoder /
_backward_pose_decoder): both ResNet-18 encoders (the pose encoder on 2B images), the depth and the pose decoder, forward and
data gradient (on the zero-padded domain, pad = 2, for the reflect-padded depth decoder; same-size with the fused activation
gradient for the pose decoder).  The weight gradients are the trainable forward rows (TRAINABLE).  A row is resolved at 192x640
and 384x1280 by geometry().  test_layer_table_is_what_the_engine_launches holds the table to the engine (ops.profile_begin()
around one adapt(steps=1) at 192x640, B = 1 and 5); PICKS records what clslam_conv2d_pick_config returns per row and
test_picker_coverage holds it to the picker, so a changed threshold or a new dispatch case fails until it is covered here.
The picker asks for the device's CU count (Winograd units per workgroup): the emulator build reports the MI355X's 256.

Cases.  Real shapes (GPU): every forward / dgrad row at B = 1 and 5 with config = -1, the engine's zeroed 32 MiB workspace, its
cu_limit and weight_wino wherever pack() makes one -- and once more with neither where the picker then decides otherwise (the
only way it returns configuration 22).  Twins (emulator and GPU): the row's Cin, Ca / Cb split and epilogue on
_twin_geometry() -- B = 1, Cout cut, the wide rows cropped -- inside the multiply-accumulate budget of the largest case
tests/test_conv.py runs on the emulator (EMU_BUDGET, computed from its case lists), with the configuration the picker returns
for the full row forced: 512-channel reductions, stream-K hand-offs over all 32 chunks of a tile (one unit per workgroup:
31 contributors), Winograd over 64 stages.  Nothing sets CLSLAM_SPLITK / CLSLAM_SK_GROUPS: the launchers' own counts.
launch_patch() has no built-in split-K heuristic (ksplit = 1 unless CLSLAM_SPLITK is set, conv_patch.hip), so with the
engine's environment the split-K instantiations of 20-23 are never launched; their counters are still checked for zero.

Inputs: unit-variance noise times a per-input-channel gain spread over two decades, a per-output-channel spread over two decades
(BatchNorm scale of the encoder rows, filter rows elsewhere, dz of the backward), zero-mean pre-activations (both signs under
ReLU / ELU); seeds are integers derived from the row's index.

Bounds.  Every output is compared in two metrics, no element left out: the largest absolute error over the tensor, and the
relative L2 per output channel (per output channel of dW for the weight gradients).  The yardstick is the SAME restatement
evaluated in torch float32 on the same inputs (the Winograd form for configuration 40, the direct form otherwise), formed
before the kernel's output is read; the kernel is allowed 4 x that figure in the same metric: the tensor's maximum, the worst
channel against the worst channel, and every channel against 4 x its own fp32 figure -- or 4 x the median channel's where fp32
happens to land nearly exactly on a channel (one channel's fp32 error is a single draw and can be arbitrarily close to zero;
the median channel is what the format loses typically).  Identities are bitwise: a second launch on the same workspace, the
transposed weights, a fallback launch == the tiled launch it is served by.
Derived instead of measured:
  * plain sums (colsum, reduce_partials, the fused bias sums of fold_act_grad): |error| <= depth * 2^-24 * sum |term| where
    depth bounds the additions any term passes through in the kernel's layout (Higham, Accuracy and Stability, section 4.2);
  * weight gradients launched with fewer splits than the engine's.  dW[n][tap][c] is a dot product over all M = B Ho Wo
    pixels; a workgroup accumulates its share along ONE fp32 chain of M / splits products.  The engine's launch (target 512)
    keeps the chains short (128 pixels for upconv_3_0 at B = 5) and torch's fp32 kernel blocks the sum; the unsplit launch
    (wgrad_splits(desc, 1) = 1) runs one chain over all M pixels (614400 for upconv_0_1 at B = 5).  Rounding errors of a
    chain grow like the square root of its length, a property of the summation order asked for, not a fault.  So a launch
    with fewer splits than the engine's is allowed 4 x sqrt(engine's splits / its splits) x the fp32 figure, every other
    launch 4 x; and every launch is held, element by element, to the textbook |error| <= chain * 2^-24 * sum_m |dz| |G|
    (Higham, section 3.1), chain = ceil(M / splits) + ceil(splits / 4) + 16.  On the emulator twins the unsplit launch is
    therefore held at 4 x sqrt(splits of target 512), not at 4 x: it measures 4.3x-7.6x the fp32 figure there, and 25x on
    gfx950 at the real shapes (upconv_0_0 at B = 5: 253 splits against 1, allowed 4 x sqrt(253) = 64x).
    _ragged_target() adds the nearest target below the engine's whose split count does not divide the chunks / tiles (last
    split short, chains as long as the engine's, held at 4 x): a split count that divides them does not see a wrong
    rounding of chunks per split.

Measured figures (kernel | torch fp32, against float64), emu = kernel sources on the CPU emulator (twins), hip = gfx950 (real
shapes and twins): the worst case of each quantity over all cases (every row is printed per case when the tests run with -s).
"cfg N" = forward / dgrad launches served by configuration N; sum / dot rows = largest error as a fraction of the derived bound.
  quantity                                     emu kernel | fp32   (ratio)        hip kernel | fp32   (ratio)
  cfg 2 channel rel L2                         1.85e-07 |  1.83e-07 (1.01x)       3.95e-07 |  3.61e-07 (1.09x)
  cfg 2 max                                    2.31e-05 |  1.55e-05 (1.49x)       2.12e-05 |  1.55e-05 (1.37x)
  cfg 20 channel rel L2                        6.85e-07 |  6.07e-07 (1.13x)       3.58e-07 |  2.39e-07 (1.50x)
  cfg 20 max                                   3.14e-05 |  2.27e-05 (1.38x)       2.04e-05 |  1.05e-05 (1.94x)
  cfg 21 channel rel L2                        3.03e-07 |  3.79e-07 (0.80x)       2.71e-07 |  2.39e-07 (1.13x)
  cfg 21 max                                   2.53e-05 |  2.86e-05 (0.88x)       8.71e-06 |  7.05e-06 (1.24x)
  cfg 22 channel rel L2                        1.33e-06 |  1.63e-06 (0.82x)       1.33e-06 |  1.63e-06 (0.82x)
  cfg 22 max                                   2.43e-05 |  3.02e-05 (0.80x)       2.43e-05 |  3.02e-05 (0.80x)
  cfg 23 channel rel L2                        3.56e-07 |  5.18e-07 (0.69x)       8.40e-07 |  1.13e-06 (0.74x)
  cfg 23 max                                   2.51e-05 |  3.96e-05 (0.63x)       5.31e-05 |  6.84e-05 (0.78x)
  cfg 30 channel rel L2                        2.58e-07 |  5.34e-07 (0.48x)       4.73e-07 |  5.05e-07 (0.94x)
  cfg 30 max                                   1.05e-05 |  2.17e-05 (0.48x)       3.13e-05 |  3.73e-05 (0.84x)
  cfg 31 channel rel L2                        3.20e-07 |  1.33e-06 (0.24x)       6.05e-07 |  1.30e-06 (0.47x)
  cfg 31 max                                   6.83e-06 |  3.42e-05 (0.20x)       1.21e-05 |  3.72e-05 (0.33x)
  cfg 32 channel rel L2                        3.28e-07 |  1.19e-06 (0.28x)       8.23e-07 |  1.13e-06 (0.73x)
  cfg 32 max                                   6.94e-06 |  3.28e-05 (0.21x)       3.83e-05 |  6.84e-05 (0.56x)
  cfg 33 channel rel L2                        1.33e-06 |  2.20e-06 (0.60x)       1.13e-06 |  1.54e-06 (0.73x)
  cfg 33 max                                   3.17e-05 |  4.50e-05 (0.70x)       3.20e-05 |  4.98e-05 (0.64x)
  cfg 40 channel rel L2                        1.33e-06 |  1.58e-06 (0.84x)       2.87e-07 |  2.88e-07 (1.00x)
  cfg 40 max                                   3.22e-05 |  3.98e-05 (0.81x)       1.99e-05 |  1.89e-05 (1.05x)
  wgrad channel rel L2                         3.10e-07 |  2.03e-07 (1.53x)       1.97e-07 |  1.13e-07 (1.74x)
  wgrad dot error / derived bound              0.055                              0.055
  wgrad max                                    9.45e-04 |  5.55e-04 (1.70x)       7.69e-04 |  3.59e-04 (2.14x)
  colsum sum error / derived bound             0.019                              0.021
  reduce sum error / derived bound             0.156                              0.170
  wgpatch0 channel rel L2                      1.78e-07 |  2.03e-07 (0.88x)       2.14e-07 |  2.33e-07 (0.92x)
  wgpatch0 dot error / derived bound           0.002                              0.002
  wgpatch0 max                                 2.74e-03 |  2.90e-03 (0.94x)       2.74e-03 |  2.90e-03 (0.94x)
  wgpatch1 channel rel L2                      1.98e-07 |  1.52e-07 (1.30x)       1.98e-07 |  1.52e-07 (1.30x)
  wgpatch1 dot error / derived bound           0.006                              0.012
  wgpatch1 max                                 1.57e-03 |  1.08e-03 (1.45x)       1.57e-03 |  1.08e-03 (1.45x)
  fold act1 channel rel L2                     8.46e-08 |  6.11e-08 (1.38x)       8.46e-08 |  6.11e-08 (1.38x)
  fold act1 max                                3.58e-07 |  2.98e-07 (1.20x)       1.67e-06 |  9.09e-07 (1.84x)
  fold act2 channel rel L2                     7.91e-08 |  6.24e-08 (1.27x)       7.91e-08 |  6.24e-08 (1.27x)
  fold act2 max                                1.02e-06 |  6.03e-07 (1.69x)       1.67e-06 |  9.09e-07 (1.84x)
  fold bias sum error / derived bound          0.039                              0.039
  dgrad fuse channel rel L2                    6.84e-07 |  5.12e-07 (1.34x)       6.84e-07 |  5.12e-07 (1.34x)
  dgrad fuse max                               9.64e-06 |  8.18e-06 (1.18x)       9.64e-06 |  8.18e-06 (1.18x)
  dgrad+fold channel rel L2                    2.02e-07 |  1.24e-07 (1.63x)       2.49e-07 |  1.41e-07 (1.77x)
  dgrad+fold max                               2.62e-06 |  1.14e-06 (2.30x)       2.62e-06 |  1.14e-06 (2.30x)
  unsplit reduce sum error / derived bound     0.000                              0.000
  unsplit wgpatch0 channel rel L2              4.47e-07 |  2.03e-07 (2.20x)       4.32e-06 |  7.22e-07 (5.98x)
  unsplit wgpatch0 dot error / derived bound   0.003                              0.003
  unsplit wgpatch0 max                         4.38e-03 |  1.64e-03 (2.67x)       3.60e-01 |  4.89e-02 (7.36x)
  unsplit wgpatch1 channel rel L2              2.54e-07 |  1.52e-07 (1.67x)       5.67e-07 |  2.53e-07 (2.24x)
  unsplit wgpatch1 dot error / derived bound   0.016                              0.017
  unsplit wgpatch1 max                         4.85e-04 |  3.18e-04 (1.53x)       8.89e-03 |  4.95e-03 (1.80x)
  unsplit wgrad channel rel L2                 8.64e-07 |  2.03e-07 (4.26x)       2.24e-05 |  1.67e-06 (13.41x)
  unsplit wgrad dot error / derived bound      0.048                              0.048
  unsplit wgrad max                            1.25e-02 |  1.64e-03 (7.62x)       6.77e-01 |  2.68e-02 (25.26x)

One-line mutations of the kernel sources (CPU emulator, scratch copies) and the test that fails; "before" = whether
tests/test_conv.py and tests/test_conv_bwd.py as they stood caught it on the emulator:
  conv_sk.hip    `min(base + q, ncon - 1)` -> `min(base + q, 3)`: a contributor slab past the fourth re-read as the fourth
                     test_forward_twin[denc.layer3.0.conv2-cfg33] (+ cfg 31 / 32 twins)              before: yes (33 with 16 groups)
  conv_fwd.hip   pick_stream_k: `units128 >= 1280 ? 32 : 33` -> `>= 640`
                     test_picker_coverage (a penc row is no longer what PICKS records)               before: no
  conv_fwd.hip   pick_stream_k: band_fits `<= 544` -> `<= 500` (the 13 x 41 band of the 6x20 stride-2 run no longer "fits")
                     test_picker_coverage (a denc row is no longer what PICKS records)               before: no
  conv_fwd.hip   picker / dispatch: a new `case 7:` in the switch of clslam_conv2d
                     test_picker_coverage (neither picked nor in EXPLICIT_ONLY: [7])                 before: no
  conv_fwd.hip   stream-K fallback of clslam_conv2d: `if (rc == CLSLAM_OK || d->config >= 0) return rc;` -> `return rc;`
                     test_fallbacks_of_conv2d[ddec.upconv_4_0-5-33]                                  before: no
  conv_fwd.hip   Winograd fallback: the same line of the Winograd block
                     test_fallbacks_of_conv2d[denc.layer4.1.conv1-5-40]                              before: yes
  conv_patch.hip dispatch: configs 24 / 25 refuse `Cin % 64 != 0` instead of `% 32`
                     tests/test_conv.py::test_conv2d_matches_torch (the new 32-channel cases of 24 / 25) before: no (24 / 25 never launched)
  conv_patch.hip `offB = (...) * p.Cb` -> `* p.Ca`: skip source addressed with the wrong channel count
                     test_forward_twin[ddec.upconv_1_1-cfg21] (32 + 64 channels)                     before: yes
  conv_wino.hip  picker: units per workgroup `d->ch_a / 8` -> `/ 4`
                     test_picker_coverage (a denc row is no longer what PICKS records)               before: no
  conv_wino.hip  `has_res = p.residual != nullptr` -> `... && p.Cin < 256`: residual dropped from 256 channels on
                     test_forward_twin[denc.layer3.0.conv2-cfg40], [denc.layer4.0.conv2-cfg40]       before: no (Cin <= 64 there)
  conv_bwd.hip   `chunks_per_split = cdiv(chunks, splits)` -> `chunks / splits`: the pixels of a short last split dropped
                     test_backward_twin[ddec.upconv_4_1, 3_0, 3_1] (ragged target)                      before: yes
                     (a target whose split count divides the chunks does not see this mutation: _ragged_target() exists for
                      that reason)
  wgrad_patch.hip `tiles_per_split = cdiv(ntiles, splits)` -> `ntiles / splits`
                     test_backward_twin[ddec.upconv_4_1, 3_0, 3_1] (ragged target)                      before: no
                     (the same: invisible to split counts that divide the tiles)
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import conv_reference as R
from clslam_hip import _lib, ops
from conv_reference import ACT_ELU, ACT_RELU, PAD_REFLECT
from emu_util import BACKENDS, use_backend

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
NAN = float('nan')

NUM_CH_ENC = (64, 64, 128, 256, 512)
NUM_CH_DEC = (16, 32, 64, 128, 256)
NONE, RELU, ELU = 0, 1, 2
ZERO, REFLECT = 0, 1


def _row(name, net, kind, div, ca, cb, cout, k=3, stride=1, pad=None, pad_mode=ZERO, ups=False, act=NONE, bn=False, bias=False,
         resid=False, wino=False, actgrad=NONE):
    return dict(name=name, net=net, kind=kind, div=div, ca=ca, cb=cb, cout=cout, k=k, stride=stride,
                pad=k // 2 if pad is None else pad, pad_mode=pad_mode, ups=ups, act=act, bn=bn, bias=bias, resid=resid, wino=wino,
                actgrad=actgrad)


def _layer_table():
    rows = []
    # both ResNet-18 encoders (Engine.pack / Engine._encoder): per stage li the entry block (stride 2 from stage 2 on, with the 1x1
    # stride-2 downsample) and the second block; folded BatchNorm = scale + shift, weight_wino wherever pack() made one
    for net in ('denc', 'penc'):
        for li, (cin, cout) in enumerate(((64, 64), (64, 128), (128, 256), (256, 512)), start=1):
            din, dout = (4, 4) if li == 1 else (2 << li - 1, 2 << li)
            s = 1 if li == 1 else 2
            rows.append(_row(f'{net}.layer{li}.0.conv1', net, 'fwd', din, cin, 0, cout, stride=s, act=RELU, bn=True, wino=s == 1))
            if s == 2:
                rows.append(_row(f'{net}.layer{li}.0.downsample', net, 'fwd', din, cin, 0, cout, k=1, stride=2, bn=True))
            rows.append(_row(f'{net}.layer{li}.0.conv2', net, 'fwd', dout, cout, 0, cout, act=RELU, bn=True, resid=True, wino=True))
            rows.append(_row(f'{net}.layer{li}.1.conv1', net, 'fwd', dout, cout, 0, cout, act=RELU, bn=True, wino=True))
            rows.append(_row(f'{net}.layer{li}.1.conv2', net, 'fwd', dout, cout, 0, cout, act=RELU, bn=True, resid=True, wino=True))
    # depth decoder (Engine._depth_decoder): upconv_i_0 at the resolution of level i + 1, upconv_i_1 on up(x[i,0]) ++ skip
    for i in range(4, -1, -1):
        cin0 = NUM_CH_ENC[-1] if i == 4 else NUM_CH_DEC[i + 1]
        ci = NUM_CH_DEC[i]
        rows.append(_row(f'ddec.upconv_{i}_0', 'ddec', 'fwd', 2 << i, cin0, 0, ci, pad_mode=REFLECT, act=ELU, bias=True))
        rows.append(_row(f'ddec.upconv_{i}_1', 'ddec', 'fwd', 1 << i, ci, NUM_CH_ENC[i - 1] if i > 0 else 0, ci, pad_mode=REFLECT,
                         ups=True, act=ELU, bias=True))
    # pose decoder (Engine._pose_decoder), 2B images
    rows.append(_row('pdec.squeeze', 'pdec', 'fwd', 32, 512, 0, 256, k=1, act=RELU, bias=True))
    rows.append(_row('pdec.pose_0', 'pdec', 'fwd', 32, 256, 0, 256, act=RELU, bias=True))
    rows.append(_row('pdec.pose_1', 'pdec', 'fwd', 32, 256, 0, 256, act=RELU, bias=True))
    # data gradients (Engine._backward_depth_decoder): dz -> the zero-padded domain (pad = 2) with the flipped / transposed weights
    for i in range(5):
        ci = NUM_CH_DEC[i]
        rows.append(_row(f'ddec.dgrad_{i}_1', 'ddec', 'dgrad', 1 << i, ci, 0, ci, pad=2))
        if i < 4:
            rows.append(_row(f'ddec.dgrad_{i}_0', 'ddec', 'dgrad', 2 << i, ci, 0, NUM_CH_DEC[i + 1], pad=2))
    # ... and of the pose decoder (Engine._backward_pose_decoder): same-size convolution with the fused activation gradient
    rows.append(_row('pdec.dgrad_pose_1', 'pdec', 'dgrad', 32, 256, 0, 256, actgrad=RELU))
    rows.append(_row('pdec.dgrad_pose_0', 'pdec', 'dgrad', 32, 256, 0, 256, actgrad=RELU))
    return rows


LAYERS = _layer_table()
SIZES = ((192, 640), (384, 1280))
DEVICE_CUS = 256


def geometry(row, H, W, B):
    """-> dict(batch, Hi, Wi, Ho, Wo): Hi x Wi is the gathered input (after the upsampling of source A)"""
    n = B * (2 if row['net'] in ('penc', 'pdec') else 1)
    Hi, Wi = H // row['div'], W // row['div']
    Ho = (Hi + 2 * row['pad'] - row['k']) // row['stride'] + 1
    Wo = (Wi + 2 * row['pad'] - row['k']) // row['stride'] + 1
    return dict(batch=n, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo)


def cu_limit(row, B):
    """Engine.cu_limit: the two encoders share the chip 3/8 : 5/8 while they run side by side (2 <= B <= 16)"""
    if row['net'] in ('denc', 'penc') and 2 <= B <= 16:
        return DEVICE_CUS * (3 if row['net'] == 'denc' else 5) // 8
    return 0


# clslam_conv2d_pick_config per row: (engine variant @192x640 B = 1..5, @384x1280, bare variant @192x640, @384x1280); the engine
# variant = zeroed workspace + weight_wino where Engine.pack() makes one, bare = neither (test_picker_coverage holds it current)
PICKS = {
    'denc.layer1.0.conv1'       : ((21, 21, 21, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'denc.layer1.0.conv2'       : ((21, 21, 21, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'denc.layer1.1.conv1'       : ((21, 21, 21, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'denc.layer1.1.conv2'       : ((21, 21, 21, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'denc.layer2.0.conv1'       : ((23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23)),
    'denc.layer2.0.downsample'  : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'denc.layer2.0.conv2'       : ((21, 21, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 21), (21, 21, 20, 20, 20)),
    'denc.layer2.1.conv1'       : ((21, 21, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 21), (21, 21, 20, 20, 20)),
    'denc.layer2.1.conv2'       : ((21, 21, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 21), (21, 21, 20, 20, 20)),
    'denc.layer3.0.conv1'       : ((23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23)),
    'denc.layer3.0.downsample'  : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'denc.layer3.0.conv2'       : ((33, 33, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 21), (21, 20, 21, 21, 20)),
    'denc.layer3.1.conv1'       : ((33, 33, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 21), (21, 20, 21, 21, 20)),
    'denc.layer3.1.conv2'       : ((33, 33, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 21), (21, 20, 21, 21, 20)),
    'denc.layer4.0.conv1'       : ((31, 31, 31, 32, 32), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23)),
    'denc.layer4.0.downsample'  : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'denc.layer4.0.conv2'       : ((33, 40, 40, 40, 40), (33, 40, 40, 40, 40), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'denc.layer4.1.conv1'       : ((33, 40, 40, 40, 40), (33, 40, 40, 40, 40), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'denc.layer4.1.conv2'       : ((33, 40, 40, 40, 40), (33, 40, 40, 40, 40), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'penc.layer1.0.conv1'       : ((21, 21, 40, 40, 40), (20, 40, 40, 40, 40), (21, 21, 20, 20, 20), (20, 20, 20, 20, 20)),
    'penc.layer1.0.conv2'       : ((21, 21, 40, 40, 40), (20, 40, 40, 40, 40), (21, 21, 20, 20, 20), (20, 20, 20, 20, 20)),
    'penc.layer1.1.conv1'       : ((21, 21, 40, 40, 40), (20, 40, 40, 40, 40), (21, 21, 20, 20, 20), (20, 20, 20, 20, 20)),
    'penc.layer1.1.conv2'       : ((21, 21, 40, 40, 40), (20, 40, 40, 40, 40), (21, 21, 20, 20, 20), (20, 20, 20, 20, 20)),
    'penc.layer2.0.conv1'       : ((23, 23, 23, 23, 30), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23)),
    'penc.layer2.0.downsample'  : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'penc.layer2.0.conv2'       : ((21, 21, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'penc.layer2.1.conv1'       : ((21, 21, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'penc.layer2.1.conv2'       : ((21, 21, 40, 40, 40), (21, 40, 40, 40, 40), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'penc.layer3.0.conv1'       : ((23, 23, 23, 23, 23), (23, 23, 23, 23, 30), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23)),
    'penc.layer3.0.downsample'  : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'penc.layer3.0.conv2'       : ((33, 33, 40, 40, 40), (40, 40, 40, 40, 40), (21, 21, 21, 21, 21), (20, 21, 20, 20, 20)),
    'penc.layer3.1.conv1'       : ((33, 33, 40, 40, 40), (40, 40, 40, 40, 40), (21, 21, 21, 21, 21), (20, 21, 20, 20, 20)),
    'penc.layer3.1.conv2'       : ((33, 33, 40, 40, 40), (40, 40, 40, 40, 40), (21, 21, 21, 21, 21), (20, 21, 20, 20, 20)),
    'penc.layer4.0.conv1'       : ((31, 32, 32, 32, 32), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23), (23, 23, 23, 23, 23)),
    'penc.layer4.0.downsample'  : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'penc.layer4.0.conv2'       : ((33, 40, 40, 40, 40), (40, 40, 40, 40, 40), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'penc.layer4.1.conv1'       : ((33, 40, 40, 40, 40), (40, 40, 40, 40, 40), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'penc.layer4.1.conv2'       : ((33, 40, 40, 40, 40), (40, 40, 40, 40, 40), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'ddec.upconv_4_0'           : ((33, 33, 33, 33, 33), (33, 33, 32, 32, 32), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'ddec.upconv_4_1'           : ((33, 33, 32, 32, 32), (21, 20, 30, 30, 30), (21, 21, 21, 21, 21), (21, 20, 21, 21, 20)),
    'ddec.upconv_3_0'           : ((33, 33, 33, 33, 33), (21, 21, 30, 30, 30), (21, 21, 21, 21, 21), (21, 21, 21, 21, 21)),
    'ddec.upconv_3_1'           : ((21, 21, 30, 30, 30), (21, 21, 20, 20, 20), (21, 21, 21, 21, 21), (21, 21, 20, 20, 20)),
    'ddec.upconv_2_0'           : ((21, 21, 21, 21, 21), (21, 21, 21, 21, 20), (21, 21, 21, 21, 21), (21, 21, 21, 21, 20)),
    'ddec.upconv_2_1'           : ((21, 21, 21, 21, 20), (21, 20, 20, 20, 20), (21, 21, 21, 21, 20), (21, 20, 20, 20, 20)),
    'ddec.upconv_1_0'           : ((21, 21, 21, 21, 21), (21, 21, 20, 20, 20), (21, 21, 21, 21, 21), (21, 21, 20, 20, 20)),
    'ddec.upconv_1_1'           : ((21, 21, 20, 20, 20), (20, 20, 20, 20, 20), (21, 21, 20, 20, 20), (20, 20, 20, 20, 20)),
    'ddec.upconv_0_0'           : ((20, 20, 20, 20, 20), (20, 20, 20, 20, 20), (20, 20, 20, 20, 20), (20, 20, 20, 20, 20)),
    'ddec.upconv_0_1'           : ((20, 20, 20, 20, 20), (20, 20, 20, 20, 20), (20, 20, 20, 20, 20), (20, 20, 20, 20, 20)),
    'pdec.squeeze'              : (( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2), ( 2,  2,  2,  2,  2)),
    'pdec.pose_0'               : ((33, 33, 33, 33, 33), (33, 33, 21, 21, 32), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'pdec.pose_1'               : ((33, 33, 33, 33, 33), (33, 33, 21, 21, 32), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'ddec.dgrad_0_1'            : ((20, 20, 20, 20, 20), (20, 20, 20, 20, 20), (20, 20, 20, 20, 20), (20, 20, 20, 20, 20)),
    'ddec.dgrad_0_0'            : ((21, 20, 20, 20, 20), (20, 20, 20, 20, 20), (21, 20, 20, 20, 20), (20, 20, 20, 20, 20)),
    'ddec.dgrad_1_1'            : ((21, 20, 20, 20, 20), (20, 20, 20, 20, 20), (21, 20, 20, 20, 20), (20, 20, 20, 20, 20)),
    'ddec.dgrad_1_0'            : ((21, 21, 21, 21, 21), (20, 20, 20, 20, 20), (21, 21, 21, 21, 21), (20, 20, 20, 20, 20)),
    'ddec.dgrad_2_1'            : ((21, 21, 21, 21, 21), (20, 20, 20, 20, 20), (21, 21, 21, 21, 21), (20, 20, 20, 20, 20)),
    'ddec.dgrad_2_0'            : ((21, 21, 21, 21, 21), (21, 21, 21, 21, 21), (21, 21, 21, 21, 21), (21, 21, 21, 21, 21)),
    'ddec.dgrad_3_1'            : ((21, 21, 21, 21, 21), (21, 21, 21, 21, 21), (21, 21, 21, 21, 21), (21, 21, 21, 21, 21)),
    'ddec.dgrad_3_0'            : ((21, 21, 21, 21, 20), (21, 21, 21, 21, 21), (21, 21, 21, 21, 20), (21, 21, 21, 21, 21)),
    'ddec.dgrad_4_1'            : ((33, 33, 33, 21, 20), (21, 30, 30, 30, 30), (21, 21, 21, 21, 20), (21, 21, 21, 21, 21)),
    'pdec.dgrad_pose_1'         : ((33, 33, 33, 33, 33), (33, 33, 21, 21, 32), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
    'pdec.dgrad_pose_0'         : ((33, 33, 33, 33, 33), (33, 33, 21, 21, 32), (22, 22, 22, 22, 22), (21, 21, 21, 21, 21)),
}


# ---- which configurations exist, and which of them only an explicit request reaches ---------------------------------------------
# every `case` of the three dispatch switches (clslam_conv2d, conv3x3_patch_dispatch, conv3x3_sk_dispatch) + Winograd
DISPATCH_CONFIGS = set(range(0, 7)) | set(range(10, 27)) | set(range(30, 38)) | {40}
# never returned by clslam_conv2d_pick_config over the sweep of test_picker_coverage: tests/test_conv.py forces them
EXPLICIT_ONLY = [0, 1, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 24, 25, 26, 34, 35, 36, 37]
SPLITK_CAPABLE = (20, 21, 22, 23)          # launch_patch<..., SKOK = true>
STREAMK = tuple(range(30, 38))
ENGINE_WS_BYTES = 32 << 20                 # Engine.CONV_WS_BYTES


def _variants(row):
    """(workspace, weight_wino) as the sweep passes them; the first one is what the engine does"""
    return [(True, True), (False, False)] + ([(True, False), (False, True)] if row['wino'] else [])


def _pick(row, H, W, B, ws=True, wino=True, config=-1, g=None, cout=None, cu=None, ws_bytes=ENGINE_WS_BYTES):
    """clslam_conv2d_pick_config on a descriptor of the row's geometry (or of g / cout / cu where given): the picker reads no
    memory, only whether the pointers are set"""
    g = geometry(row, H, W, B) if g is None else g
    d = _lib.ConvDesc(1, 1 if row['cb'] else None, 1, None, None, None, 1, g['batch'], g['Hi'], g['Wi'], row['ca'], row['cb'],
                      g['Ho'], g['Wo'], row['cout'] if cout is None else cout, row['k'], row['stride'], row['pad'], row['pad_mode'], int(row['ups']),
                      row['act'], config, 1 if row['actgrad'] else None, row['actgrad'], 1 if ws else None,
                      ws_bytes if ws else 0, 1 if (wino and row['wino']) else None, cu_limit(row, B) if cu is None else cu)
    return _lib.get_lib().cdll.clslam_conv2d_pick_config(C.byref(d))


def _table_pick(row, size_index, B, ws=True, wino=True):
    """PICKS, for the two variants it records"""
    eng = ws and (wino or not row['wino'])
    bare = not ws and (not wino or not row['wino'])
    assert eng or bare
    return PICKS[row['name']][(0 if eng else 2) + size_index][B - 1]


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _case_key(row, g, cfg, ws, cout=None):
    return (g['batch'], g['Hi'], g['Wi'], row['ca'], row['cb'], row['cout'] if cout is None else cout, row['k'], row['stride'],
            row['pad'], row['pad_mode'], row['ups'], row['act'], row['bn'], row['bias'], row['resid'], row['actgrad'], cfg, ws)


def _real_cases():
    """every forward / dgrad row at 192x640, B = 1 and 5 (2B for the pose rows), as the engine launches it; the same row without
    workspace and transformed filter where the picker then decides otherwise.  Rows that launch the same thing (both encoders at
    B = 1, the second block of a stage) are one case."""
    H, W = SIZES[0]
    cases, seen = [], set()
    for row in LAYERS:
        for B in (1, 5):
            for ws, wino in ((True, True), (False, False)):
                cfg = _table_pick(row, 0, B, ws, wino)
                if not ws and cfg == _table_pick(row, 0, B):
                    continue
                g = geometry(row, H, W, B)
                key = _case_key(row, g, cfg, ws) + (cu_limit(row, B) if cfg >= 30 else 0,)
                if key in seen:
                    continue
                seen.add(key)
                cases.append(pytest.param(row, B, ws, cfg, id=f"{row['name']}-B{B}-{'engine' if ws else 'bare'}-cfg{cfg}"))
    return cases


def _emu_budget():
    """multiply-accumulates of the largest case tests/test_conv.py runs on the emulator"""
    import test_conv as T
    m = 0
    for B, H, W, Ca, Cb, Cout, k, stride, *_ in T.CASES:
        pad = k // 2
        m = max(m, R.macs(B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, Cout, k, Ca + Cb))
    for B, H, W, Ca, Cb, Cout, stride, *_ in T.SPLITK_CASES:
        m = max(m, R.macs(B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout, 3, Ca + Cb))
    for B, H, W, Ca, Cb, Cout, stride, *_ in T.STREAMK_CASES:
        pad = 2 if (H, W) == (14, 44) else 1          # as test_conv2d_stream_k sets it: the case tuple carries no pad
        m = max(m, R.macs(B, (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1, Cout, 3, Ca + Cb))
    for B, H, W, Cin, Cout, pad, *_ in T.WINO_CASES:
        m = max(m, R.macs(B, H + 2 * pad - 2, W + 2 * pad - 2, Cout, 3, Cin))
    return m


EMU_BUDGET = _emu_budget()


def _twin_geometry(row, H, W, cfg=None):
    """The emulator twin of a row: B = 1, the row's Cin and Ca / Cb split, the output size class kept.
    Rows up to 80 pixels wide (6x20, 12x40, 24x80) stay as they are; wider ones are cropped to 8 + (h mod 8) rows of
    32 + (w mod 16) pixels of the INPUT (64 + (w mod 32) under stride 2), which keeps the width modulo 16 and the ragged right /
    bottom tiles.  Cout is cut to the largest multiple of 16 inside two channel tiles of 64 that fits the budget; a row that is
    over the budget even with 16 channels (256 input channels and more at 24x80, 512 at 12x40 with an upsampled source) loses
    rows first (8 + (h mod 8), full width), then takes the crop of the wide rows."""
    g = geometry(row, H, W, 1)
    k, s, pad = row['k'], row['stride'], row['pad']

    def out(hi, wi):
        return (hi + 2 * pad - k) // s + 1, (wi + 2 * pad - k) // s + 1

    def crop_h(hi):
        return min(hi, (8 + hi % 8) * s)

    def crop_w(wi):
        return min(wi, (32 + wi % 16) if s == 1 else (64 + wi % 32))

    hi, wi = g['Hi'], g['Wi']
    shapes = [(crop_h(hi), crop_w(wi))] if g['Wo'] > 84 else [(hi, wi), (crop_h(hi), wi), (crop_h(hi), crop_w(wi))]
    cin = row['ca'] + row['cb']
    for hi, wi in shapes:
        ho, wo = out(hi, wi)
        cout = min(row['cout'], 128, EMU_BUDGET // R.macs(1, ho, wo, 16, k, cin) * 16)
        if cfg == 40:
            cout = min(cout, 64)          # a Winograd (region, stage) unit is 64 channels wide
        if cout >= 16:
            return dict(batch=1, Hi=hi, Wi=wi, Ho=ho, Wo=wo), cout
    raise AssertionError(('no twin inside the budget', row['name']))


def _twin_cases():
    """one twin per (row geometry, configuration) the picker returns for the row at 192x640: B = 1..5, every variant"""
    H, W = SIZES[0]
    cases, seen = [], set()
    for row in LAYERS:
        for B in range(1, 6):
            for ws, wino in ((True, True), (False, False)):
                cfg = _table_pick(row, 0, B, ws, wino)
                g, cout = _twin_geometry(row, H, W, cfg)
                key = _case_key(row, g, cfg, True, cout)
                if key in seen:
                    continue
                seen.add(key)
                cases.append(pytest.param(row, cfg, id=f"{row['name']}-cfg{cfg}"))
    return cases


REAL_CASES = _real_cases()
TWIN_CASES = _twin_cases()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _decades(g, n):
    """n gains spread log-uniformly over two decades (0.1 ... 10), the extremes always present"""
    e = torch.rand(n, generator=g) * 2 - 1
    e[0], e[n - 1] = -1.0, 1.0
    return (10.0 ** e)[torch.randperm(n, generator=g)]


def _make_inputs(seed, row, g, cout):
    """unit-variance noise times a per-input-channel gain over two decades; a per-output-channel spread over two decades in the
    BatchNorm scale (encoder rows) or in the filter rows (the others); zero-mean pre-activations, i.e. both signs under the
    activation; source A doubles as the activation-gradient source of the pose data gradients"""
    gen = torch.Generator().manual_seed(seed)
    ca, cb, k = row['ca'], row['cb'], row['k']
    cin = ca + cb
    gain = _decades(gen, cin)
    ha, wa = (g['Hi'] // 2, g['Wi'] // 2) if row['ups'] else (g['Hi'], g['Wi'])
    t = SimpleNamespace()
    t.xa = (torch.randn(g['batch'], ha, wa, ca, generator=gen) * gain[:ca]).contiguous()
    t.xb = (torch.randn(g['batch'], g['Hi'], g['Wi'], cb, generator=gen) * gain[ca:]).contiguous() if cb else None
    t.w = torch.randn(cout, k * k, cin, generator=gen) / (k * cin ** 0.5 * float(gain.square().mean().sqrt()))
    spread = _decades(gen, cout)
    t.scale = spread.contiguous() if row['bn'] else None
    if not row['bn']:
        t.w = t.w * spread.view(-1, 1, 1)
    t.w = t.w.contiguous()
    t.shift = (0.1 * spread * torch.randn(cout, generator=gen)).contiguous() if (row['bn'] or row['bias']) else None
    t.res = (torch.randn(g['batch'], g['Ho'], g['Wo'], cout, generator=gen) * spread).contiguous() if row['resid'] else None
    t.ag = (torch.randn(g['batch'], g['Ho'], g['Wo'], cout, generator=gen)).contiguous() if row['actgrad'] else None
    return t


def _reference(row, t, dtype, form='direct'):
    return R.conv_forward(t.xa, t.w, xb=t.xb, scale=t.scale, shift=t.shift, residual=t.res, ksize=row['k'], stride=row['stride'],
                          pad=row['pad'], pad_mode=row['pad_mode'], ups=row['ups'], act=row['act'], actgrad_src=t.ag,
                          actgrad_kind=row['actgrad'], dtype=dtype, form=form)


def _launch(dev, row, t, out, cfg, ws, u, cu=0):
    d = lambda v: None if v is None else v.to(dev)   # noqa: E731
    if not hasattr(t, 'dev') or t.dev[0] != dev:
        t.dev = (dev, {k: d(getattr(t, k)) for k in ('xa', 'xb', 'w', 'scale', 'shift', 'res', 'ag')})
    v = t.dev[1]
    ops.conv2d(v['xa'], v['w'], out, src_b=v['xb'], scale=v['scale'], shift=v['shift'], residual=v['res'], ksize=row['k'],
               stride=row['stride'], pad=row['pad'], pad_mode=row['pad_mode'], upsample_a=row['ups'], act=row['act'], config=cfg,
               actgrad_src=v['ag'], actgrad_kind=row['actgrad'], workspace=ws, weight_wino=u, cu_limit=cu)
    return out


# ---- comparison -----------------------------------------------------------------------------------------------------------------
ROWS = []


def _measured(backend, name, what, got, ref64, ref32, check=True, factor=4.0):
    """largest absolute error over the tensor, and relative L2 PER OUTPUT CHANNEL (last axis; the first for a weight gradient,
    which the caller moves last): the kernel is allowed 4 x the figure of the fp32 restatement in each -- the worst channel of
    the kernel against the worst channel of fp32, and every single channel against 4 x ITS fp32 figure or, where fp32 happens
    to be nearly exact on a channel, 4 x the median channel's.  The fp32 figures are formed before the kernel's output is read.
    factor: 4, times sqrt(chain / the engine's chain) for a weight gradient launched with fewer splits (module docstring)."""
    ref64 = ref64.detach().double()
    d32 = ref32.detach().double() - ref64
    e32 = float(d32.abs().max())
    nref = ref64.reshape(-1, ref64.shape[-1]).norm(dim=0).clamp_min(1e-300)
    c32 = d32.reshape(-1, ref64.shape[-1]).norm(dim=0) / nref
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), (name, what, 'non-finite output')
    dk = got - ref64
    ek = float(dk.abs().max())
    ck = dk.reshape(-1, ref64.shape[-1]).norm(dim=0) / nref
    allow = factor * torch.maximum(c32, c32.median())
    worst = int((ck / allow.clamp_min(1e-300)).argmax())
    ROWS.append(f'  [{backend}] {name:<44} {what:<10} max {ek:9.2e} | {e32:9.2e} ({ek / max(e32, 1e-300):5.2f}x)   '
                f'channel rel L2 {float(ck.max()):9.2e} | {float(c32.max()):9.2e} ({float(ck.max()) / max(float(c32.max()), 1e-300):5.2f}x)'
                f'  worst channel {worst}: {float(ck[worst]):9.2e} | {float(c32[worst]):9.2e}')
    if check:
        assert ek <= factor * e32, (name, what, 'max', ek, e32, factor)
        assert float(ck.max()) <= factor * float(c32.max()), (name, what, 'worst channel', float(ck.max()), float(c32.max()))
        assert bool((ck <= allow).all()), (name, what, 'channel', worst, float(ck[worst]), float(c32[worst]), float(c32.median()))
    return ek, e32


def _sum_bound(backend, name, what, got, terms, depth):
    """a column sum of fp32 terms, whatever its order: no term passes through more than `depth` additions, so
    |error| <= depth * 2^-24 * sum |term| to first order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)"""
    terms = terms.detach().cpu().double().reshape(-1, terms.shape[-1])
    got = got.detach().cpu().double().reshape(-1)
    assert torch.isfinite(got).all(), (name, what, 'non-finite output')
    err = (got - terms.sum(0)).abs()
    bound = depth * U * terms.abs().sum(0)
    e32 = (terms.float().sum(0).double() - terms.sum(0)).abs()
    worst = int((err / bound.clamp_min(1e-300)).argmax())
    ROWS.append(f'  [{backend}] {name:<44} {what:<10} sum error / bound {float(err[worst] / bound[worst].clamp_min(1e-300)):6.3f} '
                f'(depth {depth})   max {float(err.max()):9.2e} | {float(e32.max()):9.2e}')
    assert bool((err <= bound).all()), (name, what, worst, float(err[worst]), float(bound[worst]))


def _chain_bound(backend, name, what, got, ref64, abs64, chain):
    """a dot product accumulated in fp32 along one chain of `chain` additions (+ the reduction of the splits):
    |error| <= chain * 2^-24 * sum |term| element by element (Higham, section 3.1); abs64 = the same sum over |terms|"""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), (name, what, 'non-finite output')
    err, bound = (got - ref64.double()).abs(), chain * U * abs64.double()
    ROWS.append(f'  [{backend}] {name:<44} {what:<10} dot error / bound {float((err / bound.clamp_min(1e-300)).max()):6.3f} (chain {chain})')
    assert bool((err <= bound).all()), (name, what, float((err / bound.clamp_min(1e-300)).max()))


def _flush(capsys):
    with capsys.disabled():
        print()
        while ROWS:
            print(ROWS.pop(0))


def _workspace(dev, nbytes=ENGINE_WS_BYTES):
    return torch.zeros(nbytes, dtype=torch.uint8, device=dev)


def _forward_checks(backend, dev, name, row, g, cout, cfg, ws, cu, seed, capsys, picked=None):
    """(a) against float64, (b) a second launch on the same workspace bitwise, (c) counters / flags back at zero, (d) no NaN left"""
    t = _make_inputs(seed, row, g, cout)
    ref64 = _reference(row, t, F64)
    ref32 = _reference(row, t, F32, 'winograd' if cfg == 40 else 'direct')
    u = ops.wino_weight_transform(t.w.to(dev)) if (row['wino'] and (ws is not None or cfg == 40)) else None
    outs = []
    for _ in range(2):
        out = torch.full((g['batch'], g['Ho'], g['Wo'], cout), NAN, device=dev)
        _launch(dev, row, t, out, cfg if picked is None else -1, ws, u, cu)
        outs.append(out.cpu())
    assert not torch.isnan(outs[0]).any(), (name, 'an output element was not written')
    _measured(backend, name, f'cfg {cfg}', outs[0], ref64, ref32)
    assert torch.equal(outs[0], outs[1]), (name, 'second launch on the same workspace differs')
    if ws is not None and cfg != 40:
        assert int(ws[:65536].view(torch.int32).abs().sum()) == 0, (name, 'split-K counters / stream-K flags not reset')
    if picked is not None and cfg >= 30:
        # served by the picked persistent kernel, not quietly by a fallback: the tiled kernels sum in another order
        tiled = _launch(dev, row, t, torch.full_like(outs[0], NAN, device=dev), -2, ws, u, cu).cpu()
        assert not torch.equal(outs[0], tiled), (name, 'bitwise the tiled launch: the picked kernel did not run')
    _flush(capsys)
    return t, outs[0]


# ---- the table against the engine -----------------------------------------------------------------------------------------------
def _desc_string(row, g):
    return f"B{g['batch']} {g['Hi']}x{g['Wi']} {row['ca']}+{row['cb']}->{row['cout']} k{row['k']} s{row['stride']} pad{row['pad']}"


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 5])
def test_layer_table_is_what_the_engine_launches(B, capsys):
    """ops.profile_begin() around one adapt(steps=1) at 192x640: the set of (geometry, picked configuration) of the conv2d
    launches is the set of the table's forward and dgrad rows with the configurations PICKS records."""
    from clslam_hip import synth
    from predictor_util import make_predictor
    use_backend('hip')
    H, W = SIZES[0]
    p = make_predictor(H, W, B)
    batch = synth.make_batch(B, H, W, seed=3)
    p.set_tie_break_noise(synth.make_noise(B, H, W, seed=4))
    ops.profile_begin()
    try:
        p.adapt(None, {k: v.clone() for k, v in batch.items()}, steps=1)
        torch.cuda.synchronize()
    finally:
        got = ops.profile_end()
    launched = {(desc, cfg) for kind, cfg, _, _, desc, _ in got if kind == 'conv'}
    nconv = sum(kind == 'conv' for kind, *_ in got)
    table = {(_desc_string(row, geometry(row, H, W, B)), _table_pick(row, 0, B)) for row in LAYERS}
    with capsys.disabled():
        print(f'\n  B = {B}: {nconv} conv2d launches, {len(launched)} distinct; table {len(LAYERS)} rows, {len(table)} distinct')
    assert launched == table, (sorted(launched - table), sorted(table - launched))


# ---- the picker (host only) -----------------------------------------------------------------------------------------------------
def test_picker_coverage():
    """clslam_conv2d_pick_config over the table x B = 1..5 (2B for the pose rows) x both sizes x workspace present / absent x
    weight_wino present / absent, on the emulator build (the picker is host code; nothing is launched; the emulator reports
    the MI355X's 256 CUs).  PICKS is what it returns for the engine's variant and for the bare one; every configuration
    returned anywhere has a real-shape GPU case and an emulator twin in this file; every other configuration of the dispatch
    switches is in EXPLICIT_ONLY.  A changed threshold or a new dispatch case fails here until someone covers it."""
    use_backend('emu')
    returned = set()
    for si, (H, W) in enumerate(SIZES):
        for row in LAYERS:
            for B in range(1, 6):
                for ws, wino in _variants(row):
                    cfg = _pick(row, H, W, B, ws, wino)
                    returned.add(cfg)
                    if (ws, wino) in ((True, True), (False, False)):
                        assert cfg == _table_pick(row, si, B, ws, wino), (row['name'], (H, W), B, ws, wino, cfg)
                    # the tiled-only request of the two fallbacks of clslam_conv2d never returns a persistent kernel
                    assert _pick(row, H, W, B, ws, wino, config=-2) < 30
    gpu = {c.values[3] for c in REAL_CASES}
    twins = {c.values[1] for c in TWIN_CASES}
    assert returned <= gpu, ('picked somewhere, no real-shape GPU case', sorted(returned - gpu))
    assert returned <= twins, ('picked somewhere, no emulator twin', sorted(returned - twins))
    assert returned.isdisjoint(EXPLICIT_ONLY), sorted(returned & set(EXPLICIT_ONLY))
    assert returned | set(EXPLICIT_ONLY) == _dispatch_cases(), (
        'dispatch cases neither picked nor listed in EXPLICIT_ONLY / listed but gone', sorted(_dispatch_cases() ^ (returned | set(EXPLICIT_ONLY))))


def _dispatch_cases():
    """the `case N:` labels of the three dispatch switches, read from the kernel sources, + 40 (dispatched by an `if`)"""
    import re
    from emu_util import ROOT
    found = set()
    for f, fn in (('conv_fwd.hip', 'int clslam_conv2d(const'), ('conv_patch.hip', 'int conv3x3_patch_dispatch('), ('conv_sk.hip', 'int conv3x3_sk_dispatch(')):
        src = (ROOT / 'cl-slam_amd' / 'csrc' / f).read_text()
        body = src[src.index(fn):]
        body = body[body.index('switch (cfg)'):]
        found |= {int(m) for m in re.findall(r'case (\d+):', body[:body.index('default:')])}
    assert found == DISPATCH_CONFIGS - {40}, sorted(found ^ (DISPATCH_CONFIGS - {40}))
    return found | {40}


def test_twins_stay_inside_the_emulator_budget():
    for c in TWIN_CASES:
        row, cfg = c.values
        g, cout = _twin_geometry(row, *SIZES[0], cfg)
        assert R.macs(1, g['Ho'], g['Wo'], cout, row['k'], row['ca'] + row['cb']) <= EMU_BUDGET, (c.id, EMU_BUDGET)
        assert (g['Wo'] - geometry(row, *SIZES[0], 1)['Wo']) % 16 == 0, c.id


# ---- forward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('row,B,with_ws,cfg', REAL_CASES)
def test_forward_at_the_real_shape(row, B, with_ws, cfg, capsys, monkeypatch):
    """config = -1 with the engine's 32 MiB zeroed workspace, its cu_limit and the transformed filter where pack() makes one (or
    with neither): the library picks what PICKS records, and the result passes (a)-(d) of _forward_checks"""
    dev = use_backend('hip')
    monkeypatch.setattr(ops, '_CONV_WORKSPACES', {})
    g = geometry(row, *SIZES[0], B)
    assert _pick(row, *SIZES[0], B, with_ws, with_ws) == cfg
    ws = _workspace(dev) if with_ws else None
    name = f"{row['name']} B{B} {'ws' if with_ws else 'bare'}"
    _forward_checks('hip', dev, name, row, g, row['cout'], cfg, ws, cu_limit(row, B), 1000 + LAYERS.index(row) * 10 + B, capsys,
                    picked=cfg)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('row,cfg', TWIN_CASES)
def test_forward_twin(row, cfg, backend, capsys, monkeypatch):
    """the row's reduction (Cin, Ca / Cb split, epilogue) on _twin_geometry with the configuration the picker returns for the
    full row FORCED; workspace present, no CLSLAM_SPLITK / CLSLAM_SK_GROUPS: the launchers' own split and group counts"""
    dev = use_backend(backend)
    monkeypatch.setattr(ops, '_CONV_WORKSPACES', {})
    for env in ('CLSLAM_SPLITK', 'CLSLAM_SK_GROUPS', 'CLSLAM_WINO_GROUPS'):
        monkeypatch.delenv(env, raising=False)
    g, cout = _twin_geometry(row, *SIZES[0], cfg)
    _forward_checks(backend, dev, f"twin {row['name']} {g['Hi']}x{g['Wi']}->{cout}", row, g, cout, cfg, _workspace(dev), 0,
                    2000 + LAYERS.index(row) * 50 + cfg, capsys)


def _by_name(name):
    return next(r for r in LAYERS if r['name'] == name)


FALLBACKS = [('denc.layer4.1.conv1', 5, 40), ('ddec.upconv_4_0', 5, 33)]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,B,cfg', FALLBACKS)
def test_fallbacks_of_conv2d(name, B, cfg, backend, capsys, monkeypatch):
    """Both fallbacks of clslam_conv2d on a real row (the emulator takes the row's twin): an 80 KiB workspace holds the flag
    region and a quarter of a Winograd slab / one stream-K slab where every workgroup needs its own, which the automatically picked Winograd / stream-K launch is documented to refuse
    (include/clslam_hip.h: 64 KiB + one slab per workgroup).  The launch is then served by the tiled kernels -- bitwise the
    result of config = -2 -- and passes the comparison against float64; the explicit request still fails with the library's
    message."""
    dev = use_backend(backend)
    monkeypatch.setattr(ops, '_CONV_WORKSPACES', {})
    row = _by_name(name)
    if backend == 'hip':
        g, cout, cu = geometry(row, *SIZES[0], B), row['cout'], cu_limit(row, B)
    else:           # the twin, on two CUs' worth of workgroups: the picker then makes the same choice as for the full row
        (g, cout), cu = _twin_geometry(row, *SIZES[0], cfg), 2
    assert _pick(row, 0, 0, 0, g=g, cout=cout, cu=cu, ws_bytes=80 << 10) == cfg
    t = _make_inputs(77, row, g, cout)
    ref64, ref32 = _reference(row, t, F64), _reference(row, t, F32)
    small = _workspace(dev, 80 << 10)
    u = ops.wino_weight_transform(t.w.to(dev)) if row['wino'] else None
    shape = (g['batch'], g['Ho'], g['Wo'], cout)
    auto = _launch(dev, row, t, torch.full(shape, NAN, device=dev), -1, small, u, cu)
    tiled = _launch(dev, row, t, torch.full(shape, NAN, device=dev), -2, small, u, cu)
    assert torch.equal(auto, tiled)
    _measured(backend, f'fallback {name}', f'cfg {cfg}', auto, ref64, ref32)
    assert int(small[:65536].view(torch.int32).abs().sum()) == 0
    with pytest.raises(Exception, match='workspace'):
        _launch(dev, row, t, torch.full(shape, NAN, device=dev), cfg, small, u, cu)
    _flush(capsys)


# ---- backward -------------------------------------------------------------------------------------------------------------------
TRAINABLE = [r for r in LAYERS if r['kind'] == 'fwd' and r['net'] in ('ddec', 'pdec')]
WGRAD_TARGET = 512          # clslam_hip.engine.WGRAD_TARGET_BLOCKS (Engine._wgrad)
FROZEN_SOURCE = ('ddec.upconv_4_0', 'pdec.squeeze')     # their source is an encoder feature: the engine takes no data gradient


def _backward_inputs(seed, row, g, cout):
    """source A = act(noise x gain): the OUTPUT of its producer's activation (ELU in the depth decoder, ReLU in the pose
    decoder), so that d pre-activation carries act'; dz with a per-output-channel spread over two decades"""
    t = _make_inputs(seed, row, g, cout)
    gen = torch.Generator().manual_seed(seed + 1)
    t.xa = R.act_fn(t.xa, row['act']).contiguous()
    t.dz = (torch.randn(g['batch'], g['Ho'], g['Wo'], cout, generator=gen) * _decades(gen, cout)).contiguous()
    return t


def _wgp_tiles(B, H, W, deep):
    """pixel tiles of clslam_conv_wgrad_patch (wgp_pixel_tile, wgrad_patch.hip): 8x16, or the exact deep-stage tiles"""
    if deep and W == 40 and H % 4 == 0:
        return B * (H // 4)
    if deep and (H, W) == (6, 20):
        return B
    return B * -(-H // 8) * -(-W // 16)


def _ragged_target(splits_of, units):
    """the target nearest below the engine's for which the library's own split count does not divide the units (32-pixel
    chunks / pixel tiles): the last split is short, the chains about as long as the engine's.  None where no such count
    exists (fewer than three units)."""
    for tb in range(WGRAD_TARGET, 1, -1):
        sp = splits_of(tb)
        if 1 < sp < units and units % sp:
            return tb
    return None


def _backward_checks(backend, dev, name, row, g, cout, seed, capsys, monkeypatch):
    t = _backward_inputs(seed, row, g, cout)
    k, ca, cb, act = row['k'], row['ca'], row['cb'], row['act']
    B, H, W = g['batch'], g['Ho'], g['Wo']
    kw = dict(xb=t.xb, ksize=k, pad=row['pad'], pad_mode=row['pad_mode'], ups=row['ups'], act_a=act)
    dw64, db64, dpre64 = R.conv_backward(t.xa, t.w, t.dz, dtype=F64, **kw)
    dw32, db32, dpre32 = R.conv_backward(t.xa, t.w, t.dz, dtype=F32, **kw)
    dwabs = R.conv_backward(t.xa.abs(), t.w, t.dz.abs(), dtype=F64, **dict(kw, xb=None if t.xb is None else t.xb.abs()))[0]      # sum |dz| |G|: the gather keeps |.|
    last = lambda v: v.reshape(cout, -1).t()      # noqa: E731 -- per output channel of dW
    M = B * H * W
    d = lambda v: None if v is None else v.to(dev)   # noqa: E731
    xa, xb, w, dz = d(t.xa), d(t.xb), d(t.w), d(t.dz)
    n = t.w.numel()
    desc = ops.conv_desc(xa, (B, H, W, cout), src_b=xb, ksize=k, pad=row['pad'], pad_mode=row['pad_mode'], upsample_a=row['ups'])

    def reduced(partial, splits):
        dw = torch.full((n,), NAN, device=dev)
        ops.reduce_partials(partial, dw, n, splits)
        return dw.cpu().view_as(t.w)

    # ---- weight gradient: the gather kernel at the engine's target and unsplit, the patch kernel where it applies ----------
    # Every launch is held to 4 x the fp32 figure times sqrt(its chain / the engine's chain) where it has fewer splits than the
    # engine's (rounding errors of a chain grow like the square root of its length), and to the derived chain bound.
    engine_splits = ops.wgrad_splits(desc, WGRAD_TARGET)
    for target in (WGRAD_TARGET, 1, _ragged_target(lambda tb: ops.wgrad_splits(desc, tb), -(-M // 32))):
        if target is None:
            continue
        splits = ops.wgrad_splits(desc, target)
        partial = torch.full((splits * n,), NAN, device=dev)
        ops.conv_wgrad(desc, dz, partial, splits)
        _measured(backend, name, f'wgrad/{splits}', last(reduced(partial, splits)), last(dw64), last(dw32),
                  factor=4 * max(1.0, engine_splits / splits) ** 0.5)
        _chain_bound(backend, name, f'wgrad/{splits}', reduced(partial, splits), dw64, dwabs, -(-M // splits) + -(-splits // 4) + 16)
        # reduce_partials on its own: 256 / 64 or 256 / 16 split lanes, then the lanes (reduce_partials_kernel)
        _sum_bound(backend, name, f'reduce/{splits}', reduced(partial, splits).reshape(-1), partial.view(splits, n), -(-splits // 4) + 16)
    for deep in ('0', '1'):
        monkeypatch.setenv('CLSLAM_WGRAD_DEEP_TILES', deep)
        if not ops.wgrad_patch_supported(desc) or (deep == '1' and g['Wo'] > 40):
            continue
        ntiles = _wgp_tiles(B, H, W, deep == '1')
        engine_splits = ops.wgrad_patch_splits(desc, WGRAD_TARGET)
        for target in (WGRAD_TARGET, 1, _ragged_target(lambda tb: ops.wgrad_patch_splits(desc, tb), ntiles)):
            if target is None:
                continue
            splits = ops.wgrad_patch_splits(desc, target)
            partial = torch.full((splits * n,), NAN, device=dev)
            ops.conv_wgrad_patch(desc, dz, partial, splits)
            _measured(backend, name, f'wgpatch{deep}/{splits}', last(reduced(partial, splits)), last(dw64), last(dw32),
                      factor=4 * max(1.0, engine_splits / splits) ** 0.5)
            _chain_bound(backend, name, f'wgpatch{deep}/{splits}', reduced(partial, splits), dw64, dwabs, -(-M // splits) + -(-splits // 4) + 16)
    monkeypatch.delenv('CLSLAM_WGRAD_DEEP_TILES')
    # ---- bias gradient: column sums of dz ---------------------------------------------------------------------------------
    rows = B * H * W
    nb = ops.colsum_blocks(rows)
    part = torch.full((nb * cout,), NAN, device=dev)
    ops.colsum(dz, part, rows, cout)
    db = torch.full((cout,), NAN, device=dev)
    ops.reduce_partials(part, db, cout, nb)
    _sum_bound(backend, name, 'colsum', db, t.dz, -(-rows // nb) + -(-nb // 4) + 16)       # a block's rows, then reduce_partials
    # ---- data gradient w.r.t. the pre-activation of source A --------------------------------------------------------------
    if row['name'] in FROZEN_SOURCE:
        _flush(capsys)
        return
    taps = k * k
    wt = torch.full((ca, taps, cout), NAN, device=dev)
    ops.weight_transpose(w, wt, ch_in_sel=ca)
    assert torch.equal(wt.cpu(), R.transpose_flip(t.w, ca))
    if k == 3 and row['pad_mode'] == PAD_REFLECT:
        dxp = torch.full((B, H + 2, W + 2, ca), NAN, device=dev)
        ops.conv2d(dz, wt, dxp, ksize=3, pad=2, workspace=_workspace(dev))
        ha, wa = (H // 2, W // 2) if row['ups'] else (H, W)
        dpre = torch.full((B, ha, wa, ca), NAN, device=dev)
        nbf = ops.fold_blocks(B, H, W, ca, row['ups'])
        bpart = torch.full((nbf * ca,), NAN, device=dev)
        ops.fold_act_grad(dxp, xa, dpre, h=H, w=W, ch=ca, border=1, pool=row['ups'], act=act, bias_partial=bpart)
        _measured(backend, name, 'dgrad+fold', dpre.cpu(), dpre64, dpre32)
        bsum = torch.full((ca,), NAN, device=dev)
        ops.reduce_partials(bpart, bsum, ca, nbf)
        _sum_bound(backend, name, 'fold bias', bsum, dpre, -(-B * ha * wa // nbf) + -(-nbf // 4) + 16)    # the kernel's own dz summed
        # fold_act_grad on a padded-domain gradient of this file's own (not the convolution's output), ELU and ReLU
        gen = torch.Generator().manual_seed(seed + 2)
        own = torch.randn(B, H + 2, W + 2, ca, generator=gen)
        for a in (act, ACT_RELU if act == ACT_ELU else ACT_ELU):
            f64, s64 = R.fold(own, t.xa, pool=row['ups'], act=a, dtype=F64)
            f32, s32 = R.fold(own, t.xa, pool=row['ups'], act=a, dtype=F32)
            ops.fold_act_grad(d(own), xa, dpre.fill_(NAN), h=H, w=W, ch=ca, border=1, pool=row['ups'], act=a, bias_partial=bpart.fill_(NAN))
            _measured(backend, name, f'fold act{a}', dpre.cpu(), f64, f32)
            ops.reduce_partials(bpart, bsum.fill_(NAN), ca, nbf)
            _sum_bound(backend, name, f'fold{a} bias', bsum, dpre, -(-B * ha * wa // nbf) + -(-nbf // 4) + 16)
    else:
        dpre = torch.full((B, H, W, ca), NAN, device=dev)
        ops.conv2d(dz, wt, dpre, ksize=k, pad=k // 2, actgrad_src=xa, actgrad_kind=act, workspace=_workspace(dev))
        _measured(backend, name, 'dgrad fused', dpre.cpu(), dpre64, dpre32)
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('splits,n', [(1, 4608), (2, 1000), (19, 36864), (60, 2304), (512, 2304), (384, 16), (7, 18)])
def test_reduce_partials_on_generated_partials(splits, n, backend, capsys):
    """clslam_reduce_partials on partials this file makes: noise with a per-column gain over two decades, split counts of the
    engine's plans (the gather kernel's 19 / 60 / 512, a bias with 384 fold blocks) and n that is not a multiple of 16"""
    dev = use_backend(backend)
    gen = torch.Generator().manual_seed(5000 + splits)
    part = (torch.randn(splits, n, generator=gen) * _decades(gen, n)).contiguous()
    out = torch.full((n,), NAN, device=dev)
    ops.reduce_partials(part.to(dev).reshape(-1), out, n, splits)
    _sum_bound(backend, f'generated {splits} x {n}', 'reduce', out, part, -(-splits // 4) + 16)
    _flush(capsys)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('row', [pytest.param(r, id=r['name']) for r in TRAINABLE])
def test_backward_at_the_real_shape(row, B, capsys, monkeypatch):
    dev = use_backend('hip')
    monkeypatch.setattr(ops, '_CONV_WORKSPACES', {})
    g = geometry(row, *SIZES[0], B)
    _backward_checks('hip', dev, f"{row['name']} B{B}", row, g, row['cout'], 3000 + LAYERS.index(row) * 10 + B, capsys, monkeypatch)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('row', [pytest.param(r, id=r['name']) for r in TRAINABLE])
def test_backward_twin(row, backend, capsys, monkeypatch):
    dev = use_backend(backend)
    monkeypatch.setattr(ops, '_CONV_WORKSPACES', {})
    g, cout = _twin_geometry(row, *SIZES[0])
    cout = max(32, cout // 32 * 32) if row['cout'] >= 32 else cout        # keep the row's 32- / 64-wide weight-gradient tiles
    _backward_checks(backend, dev, f"twin {row['name']} {g['Hi']}x{g['Wi']}->{cout}", row, g, cout, 4000 + LAYERS.index(row), capsys,
                     monkeypatch)
