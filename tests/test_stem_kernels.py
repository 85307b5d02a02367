"""The encoder entry one kernel at a time: stem_pack_weight, stem_conv and maxpool3x3s2 of csrc/encoder_ops.hip through their
`ops` wrappers, on inputs this file constructs and buffers pre-filled with NaN, against the float64 restatement of
tests/heads_reference.py.  Conventions as documented at the top of tests/test_loss_kernels.py and tests/test_conv_layers.py;
every output lies in a buffer with a tail of 64 sentinel floats that must come back untouched.

Inputs.  Images uniform in [0, 1] (every image and every batch element its own draw); stem filters: unit-variance noise times a
per-input-channel gain over two decades; BatchNorm scales over two decades, every third one negative, shifts of the size of the
scaled convolution so that pre-activations lie on both sides of 0.  The max-pool is run on all-negative values, on mixed signs
with 5 % of the entries -inf, and on non-negative values: only the last one is what the stem produces, and only the first two
tell "no tap" from a tap of 0.  Seeds are integers derived from the shape.

Bounds.
  * identities: the max-pool == the float64 maximum of the same fp32 inputs, as values; stem_pack_weight == the restated layout
    bitwise, both pad columns of every row exactly 0; a second launch == the first; the images of a larger buffer that a launch
    into a batch-offset slice does not own stay NaN;
  * measured: stem_conv against float64, largest absolute error over the tensor and relative L2 per output channel, at most 4 x
    the figure of the same restatement in torch float32 (formed first; median-channel fallback, test_conv_layers._measured).

Cases (n_img, B, H, W).  (1,1,20,36): one partial tile of the 8x16 output tile; (1,3,33,70): odd H, 3 x 3 tiles with a ragged last
row and column, b > 0; (2,3,20,36): the second image with B = 3, every batch element of img_b distinct; (2,2,17,33) into images
1..2 of a 4-image buffer as the engine does; (1,1,7,7): Ho = Wo = 4, every output touches the zero padding; the engine's
192x640 with (2, 5) on the device only.  Max-pool (B,H,W,C): odd and even extents, one pixel, C = 4 (one quad) to 128;
(4,255,257,64) on the device only: 1,056,768 output quads, more than 4096 blocks x 256 threads, so that the grid-stride loop runs
a second, ragged time.

Measured figures (kernel | torch fp32, against float64), the worst case of each quantity; emu = kernel sources on the CPU
emulator, hip = gfx950 (printed per case with -s):
  quantity                              emu kernel | fp32   (ratio)        hip kernel | fp32   (ratio)
  stem_conv max                           7.97e-06 |  3.60e-06 (2.21x)       7.97e-06 |  3.60e-06 (2.21x)
  stem_conv channel rel L2                6.73e-07 |  5.21e-07 (1.29x)       1.26e-06 |  9.14e-07 (1.38x)
  (the case with the largest ratio; the hip column includes the 192x640 case.  Max-pool and stem_pack_weight are identities.)

One-line mutations of the kernel sources (CPU emulator, scratch copies) and the test of this file that fails; "before" = whether
tests/test_heads_stem.py caught it on the emulator:
  encoder_ops.hip  maxpool: a tap outside the image contributes 0 instead of repeating an inside tap
                     test_maxpool: the 5 negative and the 5 mixed cases                                 before: no
  encoder_ops.hip  maxpool: `float4 m = v[4]` -> `m = 0`
                     test_maxpool: the 5 negative and the 5 mixed cases                                 before: no
  encoder_ops.hip  stem: `img_b + ((size_t)b * 3 + (cc - 3))` -> `img_b + (cc - 3)` (b dropped)
                     test_stem_conv[2-3-20-36], test_stem_conv_into_a_batch_offset_slice                before: no (B = 1 there)
  encoder_ops.hip  stem: out-of-image patch value `0.f` -> `(0.f - 0.45f) / 0.225f` (the normalised raw zero)
                     test_stem_conv: all 4 cases, test_stem_conv_into_a_batch_offset_slice              before: yes
  encoder_ops.hip  stem_pack_kernel: the `k < ST_K` guard removed (emulator only: reads past the weights)
                     test_stem_pack_weight[1], [2] (a pad column is not 0); the 5 stem_conv cases       before: yes (through the stem)
"""
import pytest
import torch

import heads_reference as R
from clslam_hip import _lib, ops
from emu_util import BACKENDS, use_backend
from test_conv_layers import _flush, _measured

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
TAIL, SENTINEL = 64, -12345.0
GPU_ONLY = [pytest.param('hip', id='hip', marks=pytest.mark.gpu)]


def guarded(shape, dev, fill=NAN):
    """-> (tensor of `shape` filled with `fill`, check()): the tensor is the head of a buffer whose last TAIL floats hold a
    sentinel; check() asserts that they still do"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + TAIL,), fill, device=dev)
    buf[n:] = SENTINEL

    def check():
        assert bool((buf[n:] == SENTINEL).all()), 'the launch wrote past the end of its output'

    return buf[:n].view(shape), check


def _decades(g, n):
    """n gains spread log-uniformly over two decades (0.1 ... 10), the extremes always present"""
    e = torch.rand(n, generator=g) * 2 - 1
    if n > 1:
        e[0], e[n - 1] = -1.0, 1.0
    return (10.0 ** e)[torch.randperm(n, generator=g)]


# ---- stem_pack_weight -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n_img', [1, 2])
def test_stem_pack_weight(backend, n_img):
    """bitwise the restated layout; the two pad columns of all 64 n_img rows exactly 0 (the MFMA loop multiplies column 147 with a
    patch element), written into a NaN buffer; ops.stem_pack_weight returns the same"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(40 + n_img)
    w = (torch.randn(64, 3 * n_img, 7, 7, generator=g) + 3.0).contiguous()          # no zero among the weights
    want = R.pack_weight(w)
    n = _lib.get_lib().cdll.clslam_stem_packed_size(n_img)
    assert n == want.numel() == n_img * 64 * R.STEM_LDW
    outs, wd = [], w.to(dev)
    for _ in range(2):
        packed, tail_ok = guarded((n,), dev)
        _lib.get_lib().call('clslam_stem_pack_weight', ops._p(wd), ops._p(packed), n_img, ops._stream(packed))
        outs.append(packed.cpu())
        tail_ok()
    rows = outs[0].view(n_img * 64, R.STEM_LDW)
    assert bool((rows[:, R.STEM_K:] == 0).all()), 'a pad column is not 0'
    assert torch.equal(outs[0], want)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(ops.stem_pack_weight(w.to(dev)).cpu(), want)


# ---- stem_conv ------------------------------------------------------------------------------------------------------------------
def _stem_inputs(n_img, B, H, W):
    g = torch.Generator().manual_seed(1000 * n_img + 100 * B + H + W)
    imgs = [torch.rand(B, 3, H, W, generator=g).contiguous() for _ in range(n_img)]
    cin = 3 * n_img
    gain = _decades(g, cin)
    w = (torch.randn(64, cin, 7, 7, generator=g) * gain.view(1, -1, 1, 1) / (7 * cin ** 0.5 * float(gain.square().mean().sqrt()))).contiguous()
    scale = _decades(g, 64)
    scale[torch.randperm(64, generator=g)[:21]] *= -1.0                 # a third of the BatchNorm scales negative
    shift = (0.7 * scale.abs() * torch.randn(64, generator=g)).contiguous()
    return imgs, w, scale.contiguous(), shift


def _stem_check(backend, n_img, B, H, W, capsys, slot=None):
    dev = use_backend(backend)
    imgs, w, scale, shift = _stem_inputs(n_img, B, H, W)
    ref64, ref32 = R.stem(imgs, w, scale, shift, F64), R.stem(imgs, w, scale, shift, F32)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert ref64.shape == (B, Ho, Wo, 64)
    pre_sign = float((ref64 > 0).double().mean())
    assert 0.2 < pre_sign < 0.8, ('pre-activations are not on both sides of 0', pre_sign)
    if n_img == 2:
        assert all(not torch.equal(imgs[1][a], imgs[1][b]) for a in range(B) for b in range(a))
    packed = ops.stem_pack_weight(w.to(dev))
    d = [i.to(dev) for i in imgs]
    outs = []
    for _ in range(2):
        nbuf, first = (B, 0) if slot is None else slot
        buf, tail_ok = guarded((nbuf, Ho, Wo, 64), dev)
        ops.stem_conv(d[0], d[1] if n_img == 2 else None, packed, scale.to(dev), shift.to(dev), buf[first:first + B])
        tail_ok()
        host = buf.cpu()
        outs.append(host[first:first + B])
        others = torch.cat([host[:first], host[first + B:]])
        assert bool(torch.isnan(others).all()), 'an image outside the batch-offset slice was written'
    assert not torch.isnan(outs[0]).any(), 'an output element was not written'
    _measured(backend, f'stem n_img={n_img} B{B} {H}x{W}', 'stem', outs[0], ref64, ref32)
    assert torch.equal(outs[0], outs[1])
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n_img,B,H,W', [(1, 1, 20, 36), (1, 3, 33, 70), (2, 3, 20, 36), (1, 1, 7, 7)])
def test_stem_conv(backend, n_img, B, H, W, capsys):
    _stem_check(backend, n_img, B, H, W, capsys)


@pytest.mark.parametrize('backend', BACKENDS)
def test_stem_conv_into_a_batch_offset_slice(backend, capsys):
    """(2, 2, 17, 33) into images 1..2 of a 4-image buffer (Engine: the pose stem of a chunk of frames): images 0 and 3 stay NaN"""
    _stem_check(backend, 2, 2, 17, 33, capsys, slot=(4, 1))


@pytest.mark.parametrize('backend', GPU_ONLY)
def test_stem_conv_at_the_real_shape(backend, capsys):
    """192 x 640, two images, B = 5: 12 x 20 tiles per batch element, the launch the pose encoder makes"""
    _stem_check(backend, 2, 5, 192, 640, capsys)


# ---- maxpool3x3s2 ---------------------------------------------------------------------------------------------------------------
def _pool_input(kind, B, H, W, C):
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C + len(kind))
    x = torch.randn(B, H, W, C, generator=g) * _decades(g, C)
    if kind == 'negative':
        x = -x.abs() - 0.01
    elif kind == 'mixed':
        x[torch.rand(B, H, W, C, generator=g) < 0.05] = float('-inf')
    else:
        x = x.clamp_min(0.0)
    return x.contiguous()


def _pool_check(backend, kind, B, H, W, C):
    dev = use_backend(backend)
    x = _pool_input(kind, B, H, W, C)
    ref64 = R.maxpool(x, F64)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert ref64.shape == (B, Ho, Wo, C)
    if kind == 'negative':
        assert bool((ref64 < 0).all())
    outs = []
    for _ in range(2):
        out, tail_ok = guarded((B, Ho, Wo, C), dev)
        ops.maxpool3x3s2(x.to(dev), out)
        tail_ok()
        outs.append(out.cpu())
    assert not torch.isnan(outs[0]).any(), 'an output element was not written'
    assert torch.equal(outs[0].double(), ref64), int((outs[0].double() != ref64).sum())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', ['negative', 'mixed', 'nonneg'])
@pytest.mark.parametrize('B,H,W,C', [(2, 5, 7, 4), (1, 6, 9, 64), (3, 8, 8, 20), (1, 1, 1, 8), (1, 2, 3, 128)])
def test_maxpool(backend, kind, B, H, W, C):
    """== the float64 maximum over the taps inside the image.  Odd extents have a padded last row / column, even ones do not;
    1x1: eight of nine taps lie outside; 2x3: one output row whose windows start outside"""
    _pool_check(backend, kind, B, H, W, C)


@pytest.mark.parametrize('backend', GPU_ONLY)
@pytest.mark.parametrize('kind', ['negative', 'mixed', 'nonneg'])
def test_maxpool_beyond_the_grid_cap(backend, kind):
    """(4,255,257,64): 4 x 128 x 129 x 16 = 1,056,768 output quads > 4096 x 256 = 1,048,576 threads: 8192 threads take a second
    pass of the grid-stride loop, the others do not"""
    B, H, W, C = 4, 255, 257, 64
    assert B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 4) == 1056768 > 4096 * 256
    _pool_check(backend, kind, B, H, W, C)
