"""The loop-closure encoder one kernel at a time: the entry points of csrc/lcd_ops.hip through their `ops` wrappers (mbv3_stem,
dwconv, global_avgpool, se_gate, channel_scale), the encoder's pointwise convolutions through ops.conv2d, and one forward of
clslam_hip.lcd.MobileNetV3SmallHIP stage by stage -- on buffers pre-filled with NaN, against the float64 restatement of
tests/lcd_reference.py (tests/conv_reference.py for the pointwise rows, oracle/mobilenet.py in float64 for the stages).
Conventions as documented at the top of tests/test_conv_layers.py and tests/test_loss_kernels.py.

Inputs: unit-variance noise times a per-channel gain spread over two decades, BatchNorm scales over two decades, zero-mean
pre-activations.  Wherever a hardswish / hardsigmoid follows, a band of channels has scale 0 (se_gate: zero weights), so that
its pre-activation is exactly its shift: -3, 0 and +3 themselves, the fp32 neighbours of -3 and +3 on both sides, and -40 / +40
far outside; three more channels have scale 1e-3 around -3, 0, +3 (values scattered within a few 1e-3 of the breakpoints).
Seeds are integers derived from the case index.

Bounds.  Largest absolute error over the tensor and relative L2 per channel against float64, at most 4 x the figure of the same
restatement in torch float32 on the same inputs (formed first; median-channel fallback).  Stem and depthwise outputs are
compared twice, the border (every output whose window reaches into the padding) and the interior separately, so that a border
error cannot hide in a tensor-wide norm.  The average pool is a plain sum: |error| <= depth * 2^-24 * sum |term|, depth counted
from the kernel's layout: ceil(chunk_px / 16) additions of a pixel lane + 16 of the lane combine + the chain over the chunks
+ 2 (the rounded 1 / HW and the product, or the division).  channel_scale is one multiply: bitwise x * gate in fp32.  The
zero-padded channels of lcd.py are exact: gate 0.5 = hardsigmoid(0), activations 0.

Pointwise rows.  POINTWISE is every distinct (Cin padded, Cout padded, activation, residual) clslam_conv2d serves for the
encoder, derived from lcd.SETTINGS and lcd._p16; test_pointwise_rows_are_what_the_encoder_launches records the ops.conv2d calls
of one MobileNetV3SmallHIP._forward (22 of them: 10 expansions, 11 projections, the head) and holds the list, and the padded widths named when this file was written
(16, 32, 48, 80, 96, 128, 144, 240, 288, 576), to it: a changed SETTINGS fails there until this file is looked at again.

Measured figures (kernel | torch fp32, against float64), the worst case of each quantity; emu = kernel sources on the CPU
emulator, hip = gfx950 (printed per case with -s); sum rows = largest error as a fraction of the derived bound:
  quantity                              emu kernel | fp32   (ratio)        hip kernel | fp32   (ratio)
  stem border max                         1.93e-06 |  1.16e-06 (1.66x)       9.35e-07 |  9.35e-07 (1.00x)
  stem border channel rel L2              7.71e-05 |  7.71e-05 (1.00x)       7.71e-05 |  7.71e-05 (1.00x)
  stem interior max                       3.73e-06 |  3.24e-06 (1.15x)       3.73e-06 |  3.24e-06 (1.15x)
  stem interior channel rel L2            5.62e-05 |  5.62e-05 (1.00x)       5.62e-05 |  5.62e-05 (1.00x)
  dwconv border max                       2.14e-06 |  2.14e-06 (1.00x)       5.13e-06 |  2.46e-06 (2.09x)
  dwconv border channel rel L2            8.41e-08 |  8.41e-08 (1.00x)       1.26e-07 |  1.08e-07 (1.17x)
  dwconv interior max                     2.71e-06 |  2.71e-06 (1.00x)       4.05e-06 |  2.71e-06 (1.49x)
  dwconv interior channel rel L2          8.57e-08 |  8.57e-08 (1.00x)       1.16e-07 |  8.57e-08 (1.35x)
  avgpool sum error / derived bound      0.194                              0.194
  se_gate max                             1.19e-07 |  1.45e-07 (0.82x)       1.19e-07 |  1.77e-07 (0.67x)
  se_gate channel rel L2                  9.37e-05 |  9.37e-05 (1.00x)       9.37e-05 |  9.37e-05 (1.00x)
  pointwise max                           2.83e-05 |  1.12e-05 (2.53x)       2.83e-05 |  1.87e-05 (1.51x)
  pointwise channel rel L2                5.81e-07 |  4.68e-07 (1.24x)       5.93e-07 |  3.84e-07 (1.54x)
  encoder stages max                      6.25e-06 |  3.20e-06 (1.95x)       3.84e-06 |  3.20e-06 (1.20x)
  encoder stages channel rel L2           3.98e-07 |  3.59e-07 (1.11x)       3.95e-07 |  3.59e-07 (1.10x)
  encoder features max                    4.43e-06 |  3.30e-06 (1.34x)       2.99e-06 |  3.30e-06 (0.90x)
  encoder features channel rel L2         3.20e-06 |  2.63e-06 (1.22x)       3.20e-06 |  2.63e-06 (1.22x)

One-line mutations of the kernel sources (CPU emulator, scratch copies) and the test that fails; "before" = whether
tests/test_lcd_encoder.py as it stood caught it on the emulator:
  lcd_ops.hip  dwconv_kernel `iy >= H` -> `iy > H` (emulator only: on the device this reads past the image)
                     test_dwconv: 30 of the 32 cases; test_encoder_stage_by_stage                         before: yes
  lcd_ops.hip  global_avgpool_kernel `p1 = min(HW, p0 + chunk_px)` -> `p0 + chunk_px - 1`
                     test_global_avgpool: all 42 cases; test_encoder_stage_by_stage                      before: yes
  lcd_ops.hip  se_gate_kernel store guard `c < C` -> `c < C - 1`
                     test_se_gate: all 8 cases (the last gate stays NaN); test_encoder_stage_by_stage    before: yes
  common.h     apply_act HSWISH clamp `6.f` -> `5.f`
                     test_mbv3_stem (4), test_dwconv (the 16 hardswish cases), test_pointwise_row (the
                     hardswish rows), test_encoder_stage_by_stage                                        before: yes
  "before: yes" for all four: the end-to-end test's 1e-4 bar did see them at its two image sizes; what it cannot do is say
  which kernel, border or channel is wrong, and its bar is 100 x the fp32 figures held here.
"""
import pytest
import torch

import conv_reference as R
import lcd_reference as L
from clslam_hip import lcd, ops
from emu_util import BACKENDS, use_backend
from test_conv_layers import EMU_BUDGET, ROWS, U, _flush, _measured, _sum_bound

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
NONE, RELU, HSWISH, HSIGMOID = L.ACT_NONE, L.ACT_RELU, L.ACT_HSWISH, L.ACT_HSIGMOID


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _decades(g, n):
    """n gains spread log-uniformly over two decades (0.1 ... 10), the extremes always present"""
    e = torch.rand(n, generator=g) * 2 - 1
    if n > 1:
        e[0], e[n - 1] = -1.0, 1.0
    return (10.0 ** e)[torch.randperm(n, generator=g)]


def _next(v, up):
    return float(torch.nextafter(torch.tensor(v, dtype=F32), torch.tensor(float('inf') if up else float('-inf'), dtype=F32)))


BAND_EXACT = [-3.0, 3.0, 0.0, _next(-3.0, False), _next(-3.0, True), _next(3.0, False), _next(3.0, True), -40.0, 40.0]
BAND_NEAR = [-3.0, 0.0, 3.0]


def _band(C):
    """(channels with scale 0, their shifts), (channels with scale 1e-3, their shifts): the last channels of the tensor, at most
    half of them"""
    ne = min(len(BAND_EXACT), C // 2 - len(BAND_NEAR))
    ce = list(range(C - ne, C))
    cn = list(range(C - ne - len(BAND_NEAR), C - ne))
    return (ce, BAND_EXACT[:ne]), (cn, BAND_NEAR)


def _affine(g, C, banded):
    scale = _decades(g, C)
    shift = 0.1 * scale * torch.randn(C, generator=g)
    if banded:
        (ce, ve), (cn, vn) = _band(C)
        scale[ce], shift[ce] = 0.0, torch.tensor(ve)
        scale[cn], shift[cn] = 1e-3, torch.tensor(vn)
    return scale.contiguous(), shift.contiguous()


def _border_mask(H, W, Ho, Wo, K, stride):
    """(Ho, Wo) bool: the window of the output pixel reaches into the padding (pad = K // 2)"""
    pad = K // 2
    oy, ox = torch.arange(Ho), torch.arange(Wo)
    by = (oy * stride - pad < 0) | (oy * stride - pad + K - 1 > H - 1)
    bx = (ox * stride - pad < 0) | (ox * stride - pad + K - 1 > W - 1)
    return by.view(-1, 1) | bx.view(1, -1)


def _border_and_interior(backend, name, got, ref64, ref32, mask):
    assert not torch.isnan(got).any(), (name, 'an output element was not written')
    for what, m in (('border', mask), ('interior', ~mask)):
        if bool(m.any()):
            _measured(backend, name, what, got[:, m], ref64[:, m], ref32[:, m])


# ---- mbv3_stem ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W', [(1, 7, 9), (2, 8, 10), (1, 9, 8), (2, 33, 47)])
def test_mbv3_stem(backend, B, H, W, capsys):
    """odd and even extents (an even extent has no padded last row / column, an odd one has); 2 x 17 x 24 outputs = four
    workgroups"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(10 * H + W)
    img = torch.rand(B, 3, H, W, generator=g)
    w = (torch.randn(16, 3, 3, 3, generator=g) / 27 ** 0.5).contiguous()
    scale, shift = _affine(g, 16, True)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ref64, ref32 = L.stem(img, w, scale, shift, F64), L.stem(img, w, scale, shift, F32)
    assert ref64.shape == (B, Ho, Wo, 16)
    out = torch.full((B, Ho, Wo, 16), NAN, device=dev)
    ops.mbv3_stem(img.to(dev), w.to(dev), scale.to(dev), shift.to(dev), out)
    _border_and_interior(backend, f'stem B{B} {H}x{W}', out.cpu(), ref64, ref32, _border_mask(H, W, Ho, Wo, 3, 2))
    _flush(capsys)


# ---- dwconv ---------------------------------------------------------------------------------------------------------------------
def _dw_cases():
    cases = []
    for K in (3, 5):
        for stride in (1, 2):
            for act in (RELU, HSWISH):
                # B = 8 on the two smallest images: at 5x5 stride 2 their interior is one or two pixels, and a per-channel figure
                # of one or two numbers exceeds 4 x its fp32 twin by chance (6 % of the draws for two, more for one)
                shapes = [(2, 7, 9, 16), (8, 6, 5, 80), (8, 5, 8, 144)]
                if K == 5:
                    shapes += [(8, 2, 3, 16), (8, 3, 2, 80)]      # K / 2 is not smaller than the image: every tap row clips; B = 8:
                    #                                              a channel then still has 16 outputs at stride 2
                for B, H, W, C in shapes:
                    cases.append(pytest.param(K, stride, act, B, H, W, C, id=f'k{K}-s{stride}-act{act}-B{B}-{H}x{W}x{C}'))
    return cases


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('K,stride,act,B,H,W,C', _dw_cases())
def test_dwconv(backend, K, stride, act, B, H, W, C, capsys):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(K * 1000 + stride * 100 + act * 10 + H + C)
    x = (torch.randn(B, H, W, C, generator=g) * _decades(g, C)).contiguous()
    w = (torch.randn(K * K, C, generator=g) / (K * x.reshape(-1, C).std(0).clamp_min(1e-3))).contiguous()
    scale, shift = _affine(g, C, act == HSWISH)
    pad = K // 2
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    ref64, ref32 = (L.dwconv(x, w, scale, shift, K, stride, act, dt) for dt in (F64, F32))
    assert ref64.shape == (B, Ho, Wo, C)
    out = torch.full((B, Ho, Wo, C), NAN, device=dev)
    ops.dwconv(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), out, K, stride, act)
    _border_and_interior(backend, f'dwconv k{K} s{stride} act{act} B{B} {H}x{W}x{C}', out.cpu(), ref64, ref32,
                         _border_mask(H, W, Ho, Wo, K, stride))
    _flush(capsys)


# ---- global_avgpool -------------------------------------------------------------------------------------------------------------
POOL_HW = [1, 63, 64, 127, 128, 129, 64 * 64 + 1]
_POOL_INPUT = {}


def _pool_input(HW, C):
    if (HW, C) not in _POOL_INPUT:
        g = torch.Generator().manual_seed(HW * 7 + C)
        gain = _decades(g, C)
        _POOL_INPUT[HW, C] = ((torch.randn(2, HW, C, generator=g) + 100.0 * torch.randn(C, generator=g)) * gain).contiguous()
    return _POOL_INPUT[HW, C]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('with_partial', [False, True], ids=['direct', 'partial'])
@pytest.mark.parametrize('C', [16, 80, 576])
@pytest.mark.parametrize('HW', POOL_HW)
def test_global_avgpool(backend, HW, C, with_partial, capsys):
    """B = 2; HW = 1, 63, 64, 127: one chunk; 128, 129: two (129: a short second one); 4097: the cap of 64 chunks of 65 pixels,
    the last one 2 pixels.  C = 16: a quarter of a channel block; 80: a ragged second block; 576: nine blocks.  Every channel
    carries an offset of 100 standard deviations of its noise."""
    dev = use_backend(backend)
    x = _pool_input(HW, C)
    nch = ops.avgpool_chunks(HW) if with_partial else 1
    assert nch == max(1, min(64, HW // 64)) or not with_partial
    chunk_px = -(-HW // nch)
    depth = -(-chunk_px // 16) + 16 + (nch if nch > 1 else 0) + 2
    out = torch.full((2, C), NAN, device=dev)
    partial = torch.full((2 * nch * C,), NAN, device=dev) if with_partial else None
    ops.global_avgpool(x.to(dev), out, partial)
    got = out.cpu()
    assert not torch.isnan(got).any()
    for b in range(2):
        _sum_bound(backend, f'avgpool HW={HW} C={C} chunks={nch}', f'b{b}', got[b].double() * HW, x[b], depth)
    if with_partial and nch > 1:
        assert not torch.isnan(partial.cpu()).any(), 'a chunk sum was not written'
    _flush(capsys)


# ---- se_gate --------------------------------------------------------------------------------------------------------------------
SE_LAUNCHES = 16
SE_PAIRS = [(16, 8), (96, 24), (240, 64), (128, 32), (144, 40), (288, 72), (576, 144), (80, 256)]


def test_se_pairs_are_the_encoders():
    got = {(lcd._p16(exp), lcd._make_divisible(exp // 4, 8)) for _, _, exp, _, se, _, _ in lcd.SETTINGS if se}
    assert got == set(SE_PAIRS[:-1])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('C,S', SE_PAIRS)
def test_se_gate(backend, C, S, capsys):
    """B = 2, launched SE_LAUNCHES times on fresh pooled vectors with the same weights and compared as one (32, C) tensor: two
    gates per channel are too few for a per-channel figure (the ratio of two such errors exceeds 4 in 6 % of the draws even for
    identical error distributions).  Gate pre-activations have a standard deviation of 3 (both sides of -3 and +3); the band channels have zero w2 rows,
    so their pre-activation is exactly b2: -3, +3, 0, their neighbours, -40 / +40.  (128, 32) is lcd.py's padding of exp = 120:
    channels 120..127 have zero weights throughout and must come out as exactly hardsigmoid(0) = 0.5.  S = 256 is the limit."""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(C * 3 + S)
    gain = _decades(g, C)
    pools = (torch.randn(SE_LAUNCHES, 2, C, generator=g) * gain).contiguous()
    w1 = (torch.randn(S, C, generator=g) / (gain * C ** 0.5)).contiguous()
    b1 = (0.2 * torch.randn(S, generator=g)).contiguous()
    real = 120 if C == 128 else C
    if real < C:
        pools[..., real:] = 0.0
        w1[:, real:] = 0.0
    hid = L.se_hidden(pools.reshape(-1, C), w1, b1, F64)
    w2 = (torch.randn(C, S, generator=g) * 3.0 / float(hid.square().sum(1).mean().sqrt())).float()
    b2 = 0.5 * torch.randn(C, generator=g)
    (ce, ve), (cn, vn) = _band(real)
    w2[ce], b2[ce] = 0.0, torch.tensor(ve)
    w2[cn], b2[cn] = w2[cn] * 1e-3, torch.tensor(vn)
    if real < C:
        w2[real:], b2[real:] = 0.0, 0.0
    w2, b2 = w2.contiguous(), b2.contiguous()
    ref64, ref32 = (L.se_gate(pools.reshape(-1, C), w1, b1, w2, b2, dt) for dt in (F64, F32))
    pre = (hid @ w2.double().t() + b2.double())
    assert float((pre < -3).double().mean()) > 0.05 and float((pre > 3).double().mean()) > 0.05
    wd = [t.to(dev) for t in (w1, b1, w2, b2)]
    got = []
    for pool in pools:
        gate = torch.full((2, C), NAN, device=dev)
        ops.se_gate(pool.to(dev), *wd, gate)
        got.append(gate.cpu())
    got = torch.cat(got)
    assert not torch.isnan(got).any(), ('a gate was not written', torch.isnan(got).nonzero()[:4].tolist())
    _measured(backend, f'se_gate C={C} S={S}', 'gate', got, ref64, ref32)
    assert torch.equal(got[:, ce], ref32[:, ce]), 'a gate whose pre-activation is exactly its bias: one fp32 formula'
    if real < C:
        assert bool((got[:, real:] == 0.5).all()), 'zero-padded channels: hardsigmoid(0) = 0.5 exactly'
    _flush(capsys)


# ---- channel_scale --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,HW,C', [(2, 37, 16), (2, 13, 80), (2, 131073, 16)])
def test_channel_scale_is_one_multiply(backend, B, HW, C):
    """bitwise x * gate.  2 x 37 x 4 and 2 x 13 x 20 quads: a ragged last workgroup; 2 x 131073 x 4 quads = 8 more than the
    4096 x 256 threads of the capped grid: a second trip of the grid-stride loop for eight of them."""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(HW + C)
    x = (torch.randn(B, HW, C, generator=g) * _decades(g, C)).contiguous()
    gate = torch.rand(B, C, generator=g).contiguous()
    gate[0, 0], gate[1, C - 1] = 0.0, 1.0
    want = L.channel_scale(x, gate, F32)
    xd = x.to(dev)
    ops.channel_scale(xd, gate.to(dev))
    assert torch.equal(xd.cpu(), want)


# ---- the pointwise convolutions -------------------------------------------------------------------------------------------------
def _pointwise_table():
    """every distinct (Cin padded, Cout padded, act, residual) of the 1x1 convolutions of MobileNetV3SmallHIP._forward, in the
    order it launches them"""
    rows = []
    for cin, k, exp, cout, se, act, stride in lcd.SETTINGS:
        a = RELU if act == 'RE' else HSWISH
        if exp != cin:
            rows.append((lcd._p16(cin), lcd._p16(exp), a, False))
        rows.append((lcd._p16(exp), lcd._p16(cout), NONE, stride == 1 and cin == cout))
    rows.append((lcd._p16(96), 576, HSWISH, False))
    return rows


POINTWISE_LAUNCHES = _pointwise_table()
POINTWISE = list(dict.fromkeys(POINTWISE_LAUNCHES))
PW_H, PW_W = 5, 7                  # 35 pixels: ragged against a 64- and a 128-pixel tile


@pytest.mark.parametrize('backend', BACKENDS)
def test_pointwise_rows_are_what_the_encoder_launches(backend, monkeypatch):
    dev = use_backend(backend)
    from test_lcd_encoder import _weights
    enc = lcd.MobileNetV3SmallHIP(_weights()[1], dev)
    seen = []
    real = ops.conv2d

    def spy(src_a, weight, out, **kw):
        assert kw['ksize'] == 1 and kw['pad'] == 0 and kw.get('stride', 1) == 1 and kw.get('config', -1) == -1
        seen.append((src_a.shape[-1], out.shape[-1], kw['act'], kw.get('residual') is not None))
        return real(src_a, weight, out, **kw)

    monkeypatch.setattr(ops, 'conv2d', spy)
    enc._forward(torch.rand(1, 3, 17, 21).to(dev))
    assert seen == POINTWISE_LAUNCHES and len(seen) == 22        # 10 expansions, 11 projections, the head
    widths = {c for row in POINTWISE for c in row[:2]}
    assert widths == {16, 32, 48, 80, 96, 128, 144, 240, 288, 576}
    assert {(a, r) for _, _, a, r in POINTWISE} == {(RELU, False), (HSWISH, False), (NONE, False), (NONE, True)}
    assert all(R.macs(1, PW_H, PW_W, co, 1, ci) <= EMU_BUDGET for ci, co, _, _ in POINTWISE)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('cin,cout,act,resid', POINTWISE, ids=[f'{ci}-{co}-act{a}-{"res" if r else "nores"}' for ci, co, a, r in POINTWISE])
def test_pointwise_row(backend, cin, cout, act, resid, capsys):
    """B = 1, 5 x 7 pixels, config = -1 (the library picks, as for the encoder), folded BatchNorm scale / shift with the
    breakpoint band under hardswish, the residual under ACT_NONE"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(POINTWISE.index((cin, cout, act, resid)) + 50)
    gain = _decades(g, cin)
    x = (torch.randn(1, PW_H, PW_W, cin, generator=g) * gain).contiguous()
    w = (torch.randn(cout, 1, cin, generator=g) / (cin ** 0.5 * float(gain.square().mean().sqrt()))).contiguous()
    scale, shift = _affine(g, cout, act == HSWISH)
    res = (torch.randn(1, PW_H, PW_W, cout, generator=g) * _decades(g, cout)).contiguous() if resid else None
    ref64, ref32 = (R.conv_forward(x, w, scale=scale, shift=shift, residual=res, ksize=1, pad=0, act=act, dtype=dt)
                    for dt in (F64, F32))
    out = torch.full((1, PW_H, PW_W, cout), NAN, device=dev)
    ops.conv2d(x.to(dev), w.to(dev), out, scale=scale.to(dev), shift=shift.to(dev), residual=None if res is None else res.to(dev),
               ksize=1, pad=0, act=act, config=-1)
    got = out.cpu()
    assert not torch.isnan(got).any(), 'an output element was not written'
    _measured(backend, f'pointwise {cin}->{cout} act{act} res{int(resid)}', 'out', got, ref64, ref32)
    _flush(capsys)


ENC_FORWARDS = 8


# ---- the encoder, stage by stage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_encoder_stage_by_stage(backend, capsys):
    """B = 2 at 33 x 47: 17 x 24, 9 x 12, 5 x 6, 3 x 3, 2 x 2 -- an odd extent at every stride-2 stage; ENC_FORWARDS forwards on
    fresh images, every stage compared as one tensor over all of them (the pooled features of one forward are two numbers per
    channel, too few for a per-channel figure).  The buffers
    MobileNetV3SmallHIP keeps (stem, the output of every block, head) and the pooled features against
    oracle.mobilenet.MobileNetV3SmallFeatures.features[i] in float64, yardstick the same module in float32; padded channels
    are stripped and must be exactly zero."""
    dev = use_backend(backend)
    from oracle.mobilenet import MobileNetV3SmallFeatures  # noqa: F401
    from test_lcd_encoder import _weights
    m32, sd = _weights()
    m64 = _weights()[0].double()
    m32.eval(), m64.eval()
    B, H, W = 2, 33, 47
    mean, std = torch.tensor(L.MEAN).view(1, 3, 1, 1), torch.tensor(L.STD).view(1, 3, 1, 1)
    names = ['stem'] + [f'o{bi}' for bi in range(len(lcd.SETTINGS))] + ['head']
    real_ch = [16] + [s[3] for s in lcd.SETTINGS] + [576]
    enc = lcd.MobileNetV3SmallHIP(sd, dev)
    real_buf = enc._buf

    def nan_buf(key, *shape):                   # the activation buffers are allocated on first use: pre-fill them with NaN
        fresh = (key,) + shape not in enc._bufs
        t = real_buf(key, *shape)
        if fresh:
            t.fill_(NAN)
        return t
    enc._buf = nan_buf
    got, stages = [[] for _ in range(14)], {F64: [[] for _ in range(14)], F32: [[] for _ in range(14)]}
    gen = torch.Generator().manual_seed(77)
    for _ in range(ENC_FORWARDS):
        img = torch.rand(B, 3, H, W, generator=gen)
        with torch.no_grad():
            for dt, m in ((F64, m64), (F32, m32)):
                x = (img.to(dt) - mean.to(dt)) / std.to(dt)
                for i, layer in enumerate(m.features):
                    x = layer(x)
                    stages[dt][i].append(x.permute(0, 2, 3, 1).contiguous())
                stages[dt][13].append(x.mean((2, 3)))
        feat = enc._forward(img.to(dev))
        bufs = {k[0]: v for k, v in enc._bufs.items()}
        for i, (name, c) in enumerate(zip(names, real_ch)):
            t = bufs[name].cpu()
            assert t.shape[:3] == stages[F64][i][-1].shape[:3] and t.shape[3] == lcd._p16(c), (name, t.shape)
            assert bool((t[..., c:] == 0).all()), (name, 'padded channels are not exactly zero')
            got[i].append(t[..., :c].clone())
        got[13].append(feat.cpu())
    assert len(names) == 13 == len(m64.features)
    for i, name in enumerate(names + ['features']):
        _measured(backend, f'encoder {name}', f'stage {i}', torch.cat(got[i]), torch.cat(stages[F64][i]), torch.cat(stages[F32][i]))
    _flush(capsys)
