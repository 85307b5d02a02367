"""Opt-in "intended" smoothness: DepthPosePrediction(..., reference_quirks=False) computes the per-sample
edge-aware term of monodepth2 instead of the reference's flattened-batch behaviour (dpp.py:1148-1176).  Checked against the
oracle's `smooth_loss_intended` branch: every loss scalar at 1e-4, the gradients of all trainable tensors as full tensors,
and the term really differs from the default (parity) mode -- at 64 x 64 and at 64 x 128 (a square shape cannot tell the x
normaliser or stride from the y one).  The smoothness gradient ALONE: two engines that differ only in disparity_smoothness
(0.1 and 0) run the same forward, so the difference of their disparity-logit gradients is what smooth_intended_bwd added,
compared with the float64 restatement of tests/loss_reference.py without the 3e-2 the photometric term needs."""
import math

import pytest
import torch

import loss_reference as R
from clslam_hip import synth
from clslam_hip.engine import TrainableLayout
from emu_util import BACKENDS, use_backend
from helpers import make_oracle
from predictor_util import make_predictor

H, W, B = 64, 64, 2


@pytest.mark.parametrize('backend', BACKENDS)
def test_intended_smoothness_matches_oracle(backend):
    _matches_oracle(backend, H, W)


@pytest.mark.parametrize('backend', BACKENDS)
def test_intended_smoothness_matches_oracle_nonsquare(backend):
    _matches_oracle(backend, 64, 128)


def _matches_oracle(backend, H, W):
    use_backend(backend)
    batch = synth.make_batch(B, H, W, seed=7)
    noise = synth.make_noise(B, H, W, seed=17)
    # a smoothness weight large enough for the term to matter in the gradients (the shipped 1e-3 is ~1e-3 of the loss)
    p = make_predictor(H, W, B, reference_quirks=False, disparity_smoothness=0.1)
    o = make_oracle(H, W, B, reference_quirks=False, disparity_smoothness=0.1)
    p.set_tie_break_noise(noise)
    out, losses = p.adapt(None, {k: v.clone() for k, v in batch.items()}, steps=1)
    o.set_adapt()
    oo, ol = o.process_batch(batch, noise, None)
    o.optimizer.zero_grad()
    ol['loss'].backward()
    for k, v in ol.items():
        assert abs(float(losses[k]) - float(v.detach())) <= 1e-4 * max(abs(float(v.detach())), 1e-4), (k, float(losses[k]), float(v.detach()))
    assert float(ol['reg_loss/scale_0'].detach()) > 0.01 * float(ol['loss'].detach())       # the term is not negligible here
    eng = p.engine
    eng.wait_training()
    worst = 0.0
    for name, off, shape in eng.layout.entries:
        model, key = name.split('/', 1)
        ref = dict(o.models[model].named_parameters())[key].grad
        got = TrainableLayout.to_reference(eng.g[off:off + math.prod(shape)], shape).cpu()
        err = float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))
        worst = max(worst, err)
        assert err < 3e-2, (name, err)          # full tensors; the bound carries the photometric term's selection flips
    # the default (parity) mode computes something else
    q = make_predictor(H, W, B, disparity_smoothness=0.1)
    q.set_tie_break_noise(noise)
    _, lq = q.adapt(None, {k: v.clone() for k, v in batch.items()}, steps=1)
    assert abs(float(lq['smooth_loss/scale_0']) - float(losses['smooth_loss/scale_0'])) > 1e-3 * abs(float(losses['smooth_loss/scale_0']))


@pytest.mark.parametrize('backend', BACKENDS)
def test_intended_smoothness_gradient_alone(backend, capsys):
    """One adapt step at 64 x 128, B = 2, of two predictors with the same weights, batch and noise, disparity_smoothness 0.1
    and 0: the disparities are the same bits, and dz_disp of the first is fl32(dz_disp of the second + the smoothness
    gradient) -- smooth_intended_bwd adds 0 at weight 0.  So the difference of the two (exact in float64) is the smoothness
    gradient up to the rounding of that one addition, 2^-24 max |dz| (derived), and is held to the float64 restatement on the
    engine's own disparities within that + the kernel-level bound of tests/test_loss_kernels.py: 4 x the error of the same
    restatement in fp32 (formed before the difference is looked at), per scale, every pixel."""
    use_backend(backend)
    H, W = 64, 128
    batch = synth.make_batch(B, H, W, seed=7)
    noise = synth.make_noise(B, H, W, seed=17)
    got = []
    for weight in (0.1, 0.0):
        p = make_predictor(H, W, B, reference_quirks=False, disparity_smoothness=weight)
        p.set_tie_break_noise(noise)
        p.adapt(None, {k: v.clone() for k, v in batch.items()}, steps=1)
        p.engine.wait_training()
        ws = p.engine._ws[B]
        got.append(([d.detach().cpu().clone() for d in ws.disp], [d.detach().cpu().clone() for d in ws.train.dz_disp],
                    ws.ctx.sample_w.detach().cpu().clone()))
    (disp, dz_a, sw), (disp_0, dz_0, _) = got
    assert all(torch.equal(a, b) for a, b in zip(disp, disp_0))          # the forward does not depend on the weight
    rgb0 = [batch['rgb', 0, s].float() for s in range(4)]
    r64 = R.smooth_intended_backward(disp, rgb0, sw, 0.1)
    r32 = R.smooth_intended_backward(disp, rgb0, sw, 0.1, torch.float32)
    lines = []
    for s in range(4):
        e32 = float((r32[s].double() - r64[s]).abs().max())
        diff = dz_a[s].double() - dz_0[s].double()
        ek = float((diff - r64[s]).abs().max())
        add = 2.0 ** -24 * float(dz_a[s].abs().max())
        lines.append(f'  [{backend}] smoothness gradient alone s{s}: {ek:9.2e} | fp32 {e32:9.2e} + addition {add:9.2e}   (|ref| max '
                     f'{float(r64[s].abs().max()):.2e}, |dz| max {float(dz_a[s].abs().max()):.2e})')
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    for s in range(4):
        assert float(r64[s].abs().max()) > 1e-3 * float(dz_a[s].abs().max())           # the term is visible in dz
        e32 = float((r32[s].double() - r64[s]).abs().max())
        ek = float((dz_a[s].double() - dz_0[s].double() - r64[s]).abs().max())
        assert ek <= 2.0 ** -24 * float(dz_a[s].abs().max()) + 4 * e32, (s, ek, e32)
