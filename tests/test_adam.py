"""Fused Adam kernel vs torch.optim.Adam (the optimizer the reference constructs at dpp.py:203)."""
import math

import pytest
import torch

from clslam_hip import ops
from emu_util import BACKENDS, use_backend
from helpers import rel_err


@pytest.mark.parametrize('backend', BACKENDS)
def test_adam_matches_torch(backend):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(0)
    n = 4099
    p = torch.randn(n, generator=g)
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([ref], 1e-4)
    w = p.clone().to(dev)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-6, 0, (1,), generator=g)))
        ref.grad = grad.clone()
        opt.step()
        ops.adam_step(w, grad.to(dev), m, v, 1e-4, step)
        # <= 1 ulp of the parameter (|p| < 4) -- the update itself is lr-sized (1e-4)
        assert float((w.cpu() - ref.detach()).abs().max()) <= 4.8e-7
    st = opt.state[ref]
    assert rel_err(m.cpu(), st['exp_avg']) < 1e-6
    assert rel_err(v.cpu(), st['exp_avg_sq']) < 1e-6


def _adam64(p, g, m, v, lr, t, b1=0.9, b2=0.999, eps=1e-8):
    """the formula of csrc/adam_dev.h's header comment in float64, 1 - beta^t formed in double"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('step', [1, 10, 1000, 20000, 100000])
def test_adam_bias_correction_at_late_steps(backend, step):
    """One update at step t on moments that are already non-zero (an adaptation that has been running): the parameter within 1 ulp
    of the float64 formula (|p| < 4: 4.8e-7, as above), the moments to 1e-6."""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(100 + step % 97)
    n = 4099
    p = torch.randn(n, generator=g).clamp(-3.9, 3.9)
    grad = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 0, (n,), generator=g).float()
    m0 = torch.randn(n, generator=g) * grad.abs()
    v0 = (torch.rand(n, generator=g) + 0.1) * grad.square()
    rp, rm, rv = _adam64(p, grad, m0, v0, 1e-4, step)
    w, m, v = p.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev)
    ops.adam_step(w, grad.to(dev), m, v, 1e-4, step)
    assert float((w.cpu().double() - rp).abs().max()) <= 4.8e-7
    assert rel_err(m.cpu(), rm) < 1e-6
    assert rel_err(v.cpu(), rv) < 1e-6
    assert not torch.equal(w.cpu(), p)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('scale', [0.2, 3.0, 1.0 / 3.0])
def test_adam_grad_scale_is_the_premultiplied_gradient(backend, scale):
    """grad_scale = s is bitwise grad_scale = 1 on the gradient multiplied by s in fp32 (vector body and scalar tail)"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(7)
    n = 1027
    p, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    m0, v0 = torch.randn(n, generator=g) * 1e-3, torch.rand(n, generator=g) * 1e-4
    res = []
    for gr, s in ((grad, scale), (grad * torch.tensor(scale, dtype=torch.float32), 1.0)):
        w, m, v = p.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev)
        ops.adam_step(w, gr.to(dev), m, v, 1e-4, 3, grad_scale=s)
        res.append((w.cpu(), m.cpu(), v.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], p)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2048 * 256 * 4 + 4 * 256 * 3 + 3])
def test_adam_every_tensor_length(backend, n):
    """the float4 body / scalar tail split at every n mod 4, and one n beyond 2048 blocks x 256 threads x 4 elements, where the
    grid-stride loop wraps: every element updated exactly once (same bounds as above), guard elements around it untouched"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(n % 1000)
    p, grad = torch.randn(n + 8, generator=g).clamp(-3.9, 3.9), torch.randn(n + 8, generator=g) * 1e-3
    m0, v0 = torch.randn(n + 8, generator=g) * 1e-3, torch.rand(n + 8, generator=g) * 1e-6
    rp, rm, rv = _adam64(p, grad, m0, v0, 1e-4, 2)
    w, m, v = p.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev)
    ops.adam_step(w[4:4 + n], grad.to(dev)[4:4 + n], m[4:4 + n], v[4:4 + n], 1e-4, 2)
    w, m, v = w.cpu(), m.cpu(), v.cpu()
    for got, old in ((w, p), (m, m0), (v, v0)):
        assert torch.equal(got[:4], old[:4]) and torch.equal(got[4 + n:], old[4 + n:])
    assert float((w[4:4 + n].double() - rp[4:4 + n]).abs().max()) <= 4.8e-7
    assert rel_err(m[4:4 + n], rm[4:4 + n]) < 1e-6
    assert rel_err(v[4:4 + n], rv[4:4 + n]) < 1e-6
    assert bool((m[4:4 + n] != m0[4:4 + n]).all())          # no element skipped (the first moment always moves: g != m)


@pytest.mark.parametrize('backend', BACKENDS)
def test_reduce_multi_sums_in_double_and_adam_guard_skips_the_update(backend):
    """The two launches behind every training step, on one item: clslam_reduce_multi sums the split partials in double, in split
    order, and rounds once; clslam_adam_step with a NaN guard (the step's loss) leaves weights and moments alone, with a finite
    guard it updates them."""
    dev = use_backend(backend)
    n, splits = 1024, 3
    part = torch.randn(splits, n, generator=torch.Generator().manual_seed(1)).to(dev)
    g, w = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    table = ops.make_reduce_table([(part, g, n, splits)], dev)
    ops.reduce_multi(table, 1, g)
    ops.adam_step(w, g, m, v, 1e-4, 1, guard=torch.full((1,), float('nan'), device=dev))
    pd = part.cpu().double()          # the split partials are summed in double, in split order, and rounded once
    assert torch.equal(g.cpu(), ((pd[0] + pd[1]) + pd[2]).float())
    assert torch.equal(w.cpu(), torch.ones(n)) and not m.any() and not v.any()
    ops.adam_step(w, g, m, v, 1e-4, 1, guard=torch.zeros(1, device=dev))
    w2, m2, v2 = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ops.adam_step(w2, g, m2, v2, 1e-4, 1)
    assert torch.equal(w, w2) and torch.equal(m, m2) and torch.equal(v, v2)
    assert not torch.equal(w.cpu(), torch.ones(n)) and bool(m.any()) and bool(v.any())
