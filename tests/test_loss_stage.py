"""View synthesis + photometric/smoothness/velocity loss, forward and backward, against the oracle
(autograd gives the reference gradients w.r.t. the disparity logits and the pose-decoder output)."""
import pytest
import torch

from clslam_hip import ops, synth
from emu_util import BACKENDS, use_backend
from helpers import make_oracle, rel_err
from oracle import functional as OF


def _run_loss_stage(dev, inputs, disp, pose, noise, sample_w, smooth_w, H, W, min_depth, max_depth, train=True, pyramid=False):
    """Sequence the loss-stage kernels exactly as the engine does (kept small and explicit here so
    the kernels are tested in isolation from the network)."""
    B = disp[0].shape[0]
    t = lambda v: v.detach().contiguous().to(dev)
    K, Kinv = t(inputs['camera_matrix', 0]), t(inputs['inv_camera_matrix', 0])
    src = {f: t(inputs['rgb', f, 0]) for f in (-1, 0, 1)}
    pose_d = t(pose)
    T = torch.empty(2, B, 4, 4, device=dev)
    P = torch.empty(2, B, 3, 4, device=dev)
    ops.pose_to_proj(pose_d, K, T, P)
    depth = torch.empty(4, B, H, W, device=dev)
    warped = torch.empty(4, 2, B, 3, H, W, device=dev)
    disp_d = [t(d) for d in disp]
    if pyramid:
        ops.warp_fwd_pyramid(disp_d, src[-1], src[1], Kinv, P, depth, warped, min_depth, max_depth)
    else:
        for s in range(4):
            ops.warp_fwd(disp_d[s], src[-1], src[1], Kinv, P, depth[s], warped[s], min_depth, max_depth)
    idsrc = torch.stack([src[-1], src[1]]).contiguous()
    idmap = torch.empty(2, B, H, W, device=dev)
    ops.photo_map(idsrc, src[0], idmap, None, 2 * B, B, H, W)
    rpmap = torch.empty(4, 2, B, H, W, device=dev)
    coef = torch.empty(4, 2, B, 9, H, W, device=dev) if train else None
    nblk = ops.automask_blocks(H, W)
    partial = torch.empty(4, B, nblk, device=dev)
    sel = torch.empty(4, B, H, W, dtype=torch.uint8, device=dev)
    means = torch.empty(4, B, ops.disp_mean_chunks(), device=dev)
    if pyramid:   # the engine's path: fused map+automask (selected-frame coefficients), LDS-tiled backward
        noise_all = torch.stack([t(noise[s]) for s in range(4)]).contiguous() if noise is not None else None
        coef_sel = torch.empty(4, B, 9, H, W, device=dev) if train else None
        ops.photo_automask_pyramid(warped, src[0], idmap, noise_all, sel, coef_sel, partial, B, H, W)
        ops.disp_mean_pyramid(disp_d, means, H, W)
    else:
        for s in range(4):
            ops.photo_map(warped[s], src[0], rpmap[s], coef[s] if train else None, 2 * B, B, H, W)
            ops.automask(idmap, t(noise[s]) if noise is not None else None, rpmap[s], sel[s], partial[s], B, H, W)
            ops.disp_mean(disp_d[s], means[s])
    n_smooth = 0 if smooth_w is None else smooth_w.numel()
    losses = torch.empty(18, device=dev)
    aux = torch.zeros(4, 2 + 2 * max(n_smooth, 1), device=dev)[:, :2 + 2 * n_smooth].contiguous()
    d0, d1 = inputs['relative_distance', 0].to(dev), inputs['relative_distance', 1].to(dev)
    rgb0 = [t(inputs['rgb', 0, s]) for s in range(4)]
    ops.loss_finalize([partial[s] for s in range(4)], disp_d, rgb0, [means[s] for s in range(4)], pose_d, d0, d1,
                      t(sample_w), t(smooth_w) if n_smooth else None, losses, aux if n_smooth else None, B, nblk, H, W,
                      n_smooth, 1e-3, 0.05)
    out = dict(T=T, P=P, depth=depth, warped=warped, losses=losses, sel=sel, partial=partial)
    if not train:
        return out
    dz = []
    if pyramid:
        nb2 = ops.loss_bwd2_blocks(H, W)
        dp_partial = torch.empty(4, B, nb2, 24, dtype=torch.float64, device=dev)
        ddisp_all = torch.empty(4, B, H, W, device=dev)
        ops.loss_bwd2_pyramid(disp_d, sel, coef_sel, warped, src[0], src[-1], src[1], Kinv, P, t(sample_w), ddisp_all, dp_partial,
                              min_depth, max_depth)
        dz = [torch.empty_like(d) for d in disp_d]
        ops.disp_grad_pyramid(ddisp_all, disp_d, aux if n_smooth else None, n_smooth, dz, H, W)
    else:
        nb2 = ops.warp_bwd_blocks(H, W)
        dp_partial = torch.empty(4, B, nb2, 24, dtype=torch.float64, device=dev)
        dpred = torch.empty(2, B, 3, H, W, device=dev)
        ddisp_up = torch.empty(B, H, W, device=dev)
        for s in range(4):
            ops.photo_grad(sel[s], coef[s], warped[s], src[0], t(sample_w), dpred, B, H, W)
            ops.warp_bwd(dpred, disp_d[s], src[-1], src[1], Kinv, P, ddisp_up, dp_partial[s], min_depth, max_depth)
            g = torch.empty_like(disp_d[s])
            ops.disp_grad(ddisp_up, disp_d[s], aux[s] if n_smooth else None, n_smooth, g, H, W)
            dz.append(g)
    dpose = torch.empty(2 * B, 12, device=dev)
    ops.pose_bwd(dp_partial, 4, nb2, pose_d, K, d0, d1, t(sample_w), 0.05, dpose)
    out.update(dz=dz, dpose=dpose)
    return out


def _compute_loss(p, inputs, outputs, noise, sw, smw):
    """the oracle's loss; with smoothness weights other than the sample weights (the kernels take the two separately, the
    oracle one vector) the smoothness term is re-weighted: loss += sum_s 1e-3 / 2^s / 4 * ((smw - sw) . smooth_s)"""
    losses = p.compute_loss(inputs, outputs, noise, sw)
    if smw is sw:
        return losses
    total = losses['loss']
    for s in range(4):
        disp = outputs['disp', s]
        norm = disp / (disp.mean(2, True).mean(3, True) + 1e-7)
        sm = (OF.smooth_loss_reference(norm, inputs['rgb', 0, s]) * smw).sum()
        reg = 1e-3 / 2 ** s * sm
        total = total + (reg - losses[f'reg_loss/scale_{s}']) / 4
        losses[f'smooth_loss/scale_{s}'], losses[f'reg_loss/scale_{s}'] = sm, reg
        losses[f'depth_loss/scale_{s}'] = losses[f'reprojection_loss/scale_{s}'] + reg
    losses['loss'] = total
    return losses


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('pyramid', [False, True])
@pytest.mark.parametrize('B,H,W,max_depth,aligned,weights', [
    pytest.param(2, 32, 64, None, False, None, id='2-32-64-None-False'), pytest.param(3, 64, 128, None, True, None, id='3-64-128-None-True'),
    pytest.param(1, 32, 64, 80.0, True, None, id='1-32-64-80.0-True'),
    # sample weights that differ between the samples, and smoothness weights that differ from them
    pytest.param(3, 32, 64, None, True, ((0.5, 0.3, 0.2), (0.2, 0.1, 0.7)), id='3-32-64-nonuniform-weights'),
    # a width of 32 mod 64: the image edge inside a tile of every tiled kernel
    pytest.param(2, 32, 96, None, True, None, id='2-32-96-None-True')])
def test_loss_stage_matches_oracle(backend, B, H, W, max_depth, aligned, weights, pyramid):
    dev = use_backend(backend)
    torch.manual_seed(3)
    inputs = synth.make_batch(B, H, W, seed=5)
    noise = synth.make_noise(B, H, W, seed=2)
    # smooth random disparity logits and small poses
    z = [(torch.randn(B, 1, H >> s, W >> s) * 0.6).requires_grad_(True) for s in range(4)]
    pose = torch.randn(2 * B, 12) * (0.002 if aligned else 0.02)
    if aligned:
        # translations that roughly undo the synthetic horizontal shift between the frames, so
        # that many pixels pick a reprojection in the min (the gradient test then has teeth)
        z = [(v.detach() * 0.3).requires_grad_(True) for v in z]
        for b in range(B):
            shift = 2.0 + 4.0 * float(synth.hash_uniform(8, 5 * 1000 + b + 31)[0])
            depth0 = (0.1 / 0.5) if max_depth is None else 1.0 / (1 / max_depth + (10 - 1 / max_depth) * 0.5)
            tx = -shift * depth0 / (0.58 * W)
            pose[b, 3] += tx
            pose[B + b, 3] += tx
    pose.requires_grad_(True)
    p = make_oracle(H, W, B, max_depth=max_depth)
    outputs = {}
    for s in range(4):
        outputs['disp', s] = torch.sigmoid(z[s])
    Tm = {}
    for fi, f in enumerate((-1, 1)):
        aa = pose[fi * B:(fi + 1) * B, 0:3].unsqueeze(1)
        tr = pose[fi * B:(fi + 1) * B, 3:6].unsqueeze(1)
        outputs['axis_angle', 0, f], outputs['translation', 0, f] = aa, tr
        Tm[f] = OF.transformation_from_parameters(aa, tr, invert=f < 0)
        outputs['cam_T_cam', 0, f] = Tm[f]
    src = {f: inputs['rgb', f, 0] for f in (-1, 1)}
    for s in range(4):
        depth, warped = OF.reconstruct(outputs['disp', s], Tm, inputs['camera_matrix', 0], inputs['inv_camera_matrix', 0],
                                       src, H, W, 0.1, max_depth)
        outputs['depth', s] = depth
        for f in (-1, 1):
            outputs['rgb', f, s] = warped[f]
    sw = smw = torch.ones(B) / B
    if weights is not None:
        sw, smw = torch.tensor(weights[0]), torch.tensor(weights[1])
    losses = _compute_loss(p, inputs, outputs, noise, sw, smw)
    losses['loss'].backward()

    got = _run_loss_stage(dev, inputs, [outputs['disp', s].squeeze(1) for s in range(4)], pose, noise, sw, smw, H, W, 0.1,
                          max_depth, pyramid=pyramid)
    for fi, f in enumerate((-1, 1)):
        assert rel_err(got['T'][fi].cpu(), Tm[f].detach()) < 1e-6
    for s in range(4):
        assert rel_err(got['depth'][s].cpu(), outputs['depth', s].detach().squeeze(1)) < 1e-5
        for fi, f in enumerate((-1, 1)):
            assert rel_err(got['warped'][s, fi].cpu(), outputs['rgb', f, s].detach()) < 2e-5, (s, f)
    L = got['losses'].cpu()
    for s in range(4):
        for j, name in enumerate(('reprojection_loss', 'smooth_loss', 'reg_loss', 'depth_loss')):
            ref = float(losses[f'{name}/scale_{s}'])
            assert abs(float(L[s * 4 + j]) - ref) <= 2e-5 * max(abs(ref), 1e-3), (name, s, float(L[s * 4 + j]), ref)
    assert abs(float(L[16]) - float(losses['velocity_loss'])) <= 1e-5 * abs(float(losses['velocity_loss']))
    assert abs(float(L[17]) - float(losses['loss'])) <= 1e-5 * abs(float(losses['loss']))
    # gradients: fraction of pixels choosing a reprojection must be non-trivial for the test to bite
    frac = float((got['sel'].cpu() >= 2).float().mean())
    assert frac > (0.2 if aligned else 0.002), frac
    # A near-tie in the 4-way min can resolve differently at fp32 round-off (the warp itself is
    # ~1e-6 away from torch's normalise->grid_sample->unnormalise round trip).  Such a pixel changes
    # the gradient of its 3x3 neighbourhood and of the pose.  Detect it against the oracle's argmin,
    # require it to be a genuine near-tie, and only then loosen the gradient tolerance.
    flipped = {}
    for s in range(4):
        rp = torch.cat([OF.reprojection_loss(outputs['rgb', f, s].detach(), inputs['rgb', 0, 0]) for f in (-1, 1)], 1)
        idl = torch.cat([OF.reprojection_loss(inputs['rgb', f, 0], inputs['rgb', 0, 0]) for f in (-1, 1)], 1) + noise[s]
        comb = torch.cat((idl, rp), 1)
        ours = got['sel'][s].cpu().long()
        mism = (comb.argmin(1) != ours).nonzero()
        assert len(mism) <= 3, (s, len(mism))
        for m in mism:
            v = comb[m[0], :, m[1], m[2]]
            assert abs(float(v.min() - v[ours[m[0], m[1], m[2]]])) < 1e-5, v.tolist()
        flipped[s] = len(mism)
    any_flip = sum(flipped.values()) > 0
    for s in range(4):
        zg = z[s].grad.squeeze(1)
        diff = (got['dz'][s].cpu() - zg).abs()
        if flipped[s] == 0:
            assert float(diff.max() / zg.abs().max()) < 2e-4, (s, float(diff.max() / zg.abs().max()))
        else:
            assert float(diff.double().norm() / zg.double().norm()) < 5e-2, s
    pg = pose.grad
    assert rel_err(got['dpose'].cpu()[:, :6], pg[:, :6]) < (2e-2 if any_flip else 2e-4)
    assert float(got['dpose'].cpu()[:, 6:].abs().max()) == 0.0


@pytest.mark.parametrize('backend', BACKENDS)
def test_in_kernel_tie_break_noise(backend):
    """dpp.py:1055-1056 inside the kernel (Philox4x32-10 + Box-Muller): N(0, 1e-5) per identity channel, reproducible per
    (seed, draw offset), fresh per offset; the fused photometric/automask kernel fed by the generator selects exactly
    what it selects when the same stream is injected as a tensor."""
    dev = use_backend(backend)
    n = 200000
    a = ops.tie_break_noise(torch.empty(n, 2, device=dev), seed=1234567, offset=3).cpu()
    b = ops.tie_break_noise(torch.empty(n, 2, device=dev), seed=1234567, offset=3).cpu()
    c = ops.tie_break_noise(torch.empty(n, 2, device=dev), seed=1234567, offset=4).cpu()
    assert torch.equal(a, b) and not torch.equal(a, c)
    z = a.double() / 1e-5
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1) < 0.01
    assert abs(float((z ** 4).mean()) - 3) < 0.1                                   # kurtosis of a normal
    assert abs(float((z[:, 0] * z[:, 1]).mean())) < 0.01 and abs(float((z * (c.double() / 1e-5)).mean())) < 0.01
    assert float(z.abs().max()) < 6.5
    # the fused kernel: generator == injected tensor of the same stream
    B, H, W = 2, 24, 80
    g = torch.Generator().manual_seed(3)
    tgt = torch.rand(B, 3, H, W, generator=g)
    warped = (tgt[None, None] + 0.002 * torch.randn(4, 2, B, 3, H, W, generator=g)).clamp(0, 1).contiguous()
    idmap = 0.0005 + 1e-5 * torch.rand(2, B, H, W, generator=g)                    # near-ties decided by the noise
    stream = ops.tie_break_noise(torch.empty(4 * B * H * W, 2, device=dev), seed=99, offset=7)
    noise = stream.view(4, B, H * W, 2).permute(0, 1, 3, 2).reshape(4, B, 2, H, W).contiguous()
    nblk = ops.automask_blocks(H, W)
    outs = []
    for mode in ('rng', 'tensor', 'none'):
        sel = torch.zeros(4, B, H, W, dtype=torch.uint8, device=dev)
        coef = torch.zeros(4, B, 9, H, W, device=dev)
        partial = torch.zeros(4, B, nblk, device=dev)
        if mode == 'rng':
            ops.photo_automask_pyramid_rng(warped.to(dev), tgt.to(dev), idmap.to(dev), 99, 7, sel, coef, partial, B, H, W)
        else:
            ops.photo_automask_pyramid(warped.to(dev), tgt.to(dev), idmap.to(dev), noise if mode == 'tensor' else None, sel, coef,
                                       partial, B, H, W)
        outs.append((sel.cpu(), partial.cpu(), coef.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert not torch.equal(outs[0][0], outs[2][0])                                 # the noise does decide near-ties

