"""TEST INFRASTRUCTURE: the loss under mask_dynamic=True (dpp.py:1063-1090 and 1148-1176) restated in loop-free torch, in
`dtype` (float64 the reference, float32 the yardstick), with torch.masked_select itself where the reference uses it -- the
flattening of the batch that makes smoothness term i the i-th static element of the cropped gradient planes is
masked_select's own here, not a re-derivation.  Builds on tests/loss_reference.py (photo maps, autograd backward)."""
import torch

import loss_reference as R

F64 = torch.float64


def static(mask):
    """dpp.py:1066-1067 / 1081-1082: a pixel is static iff (1 - m) is non-zero, i.e. m != 1"""
    return (1 - mask).type(torch.bool)


def reprojection(to_optimize, mask0):
    """to_optimize (B,H,W) the per-pixel minimum, mask0 (B,1,H,W) -> the mean over the static pixels of the whole minibatch"""
    return torch.masked_select(to_optimize, static(mask0).squeeze()).mean()


def _edge_terms(norm, img):
    gx = (norm[:, :, :, :-1] - norm[:, :, :, 1:]).abs() * torch.exp(-(img[:, :, :, :-1] - img[:, :, :, 1:]).abs().mean(1, keepdim=True))
    gy = (norm[:, :, :-1, :] - norm[:, :, 1:, :]).abs() * torch.exp(-(img[:, :, :-1, :] - img[:, :, 1:, :]).abs().mean(1, keepdim=True))
    return gx, gy


def smooth_quirk(norm, img, mask):
    """norm (B,1,h,w) normalised disparity, img (B,3,h,w), mask (B,1,h,w) float -> (B,) terms as dpp.py:1157-1176 forms them:
    both gradient planes go through masked_select (which flattens the batch), element i of each is broadcast over mask[i]
    by a second masked_select and averaged.  IndexError when the minibatch has fewer than B static elements."""
    st = static(mask)
    gx, gy = _edge_terms(norm, img)
    fx, fy = torch.masked_select(gx, st[..., :-1]), torch.masked_select(gy, st[..., :-1, :])
    out = []
    for i in range(norm.shape[0]):
        out.append(torch.masked_select(fx[i], st[i, :, :, :-1]).mean() + torch.masked_select(fy[i], st[i, :, :-1, :]).mean())
    return torch.stack(out)


def smooth_intended(norm, img, mask):
    """per sample: masked mean of the x terms over mask[b,:,:,:-1] + masked mean of the y terms over mask[b,:,:-1,:]"""
    st = static(mask)
    gx, gy = _edge_terms(norm, img)
    return torch.stack([torch.masked_select(gx[b], st[b, :, :, :-1]).mean() + torch.masked_select(gy[b], st[b, :, :-1, :]).mean()
                        for b in range(norm.shape[0])])


def quirk_positions(mask, B):
    """pixel indices y * w + x (and the sample they lie in) of the first B static elements of the cropped x plane and of the
    cropped y plane in masked_select's flat order: (2, n <= B) each"""
    st = static(mask)
    _, _, h, w = st.shape
    out = []
    for crop in (st[..., :-1], st[..., :-1, :]):
        idx = torch.nonzero(crop.reshape(-1))[:B, 0]
        cw = crop.shape[-1]
        per = crop.shape[-2] * cw
        b, r = idx // per, idx % per
        out.append((b, (r // cw) * w + r % cw))
    return out


def losses(to_opt, masks, disps, rgb0, pose, dist0, dist1, sample_w, smooth_scale, vel_scale, quirks=True, dtype=F64):
    """the 18 scalars (per scale reprojection, smooth, reg, depth; velocity; total).  to_opt[s] (B,H,W), masks[s] (B,1,h,w)"""
    B = sample_w.shape[0]
    sw = sample_w.to(dtype)
    out = torch.zeros(18, dtype=dtype)
    total = 0
    for s in range(4):
        rl = reprojection(to_opt[s].to(dtype), masks[0])
        d = disps[s].to(dtype)[:, None]
        norm = d / (d.mean(2, True).mean(3, True) + 1e-7)
        fn = smooth_quirk if quirks else smooth_intended
        sm = (fn(norm, rgb0[s].to(dtype), masks[s]) * sw).sum()
        reg = smooth_scale / 2 ** s * sm
        out[4 * s:4 * s + 4] = torch.stack([rl, sm, reg, rl + reg])
        total = total + rl + reg
    total = total / 4
    if vel_scale and vel_scale > 0:
        p = pose.to(dtype)
        vel = (vel_scale * R.OF.velocity_loss(p[:B, 3:6], p[B:2 * B, 3:6], dist0, dist1).to(dtype) * sw).sum()
        out[16] = vel
        total = total + vel
    out[17] = total
    return out


def photo_backward(sel, coef_sel, warped, target, mask0, dtype=F64):
    """dL / d warped (2,B,3,H,W) of one scale, L = sum over the static pixels of the selected reprojection map / N_static / 4:
    loss_reference.photo_backward with the dynamic pixels' selection removed and every sample weighted H W / N_static"""
    B, _, H, W = target.shape
    st = static(mask0)[:, 0]
    n = int(st.sum())
    sel_m = torch.where(st, sel, torch.full_like(sel, 255))
    return R.photo_backward(sel_m, coef_sel, warped, target, torch.full((B,), H * W / n, dtype=F64), dtype)


def disp_backward(ddisp_up, disp_s, rgb0_s, mask_s, H, W, sample_w, smooth_scale, scale, quirks=True, dtype=F64):
    """dL / dz (B,h,w), disp = sigmoid(z): L = <ddisp_up, upsample(disp)> + smooth_scale / 2^scale / 4 * sum_b w_b smooth_b.
    The forward VALUE of disp is the given tensor to the bit (loss_reference.smooth_intended_backward says why)."""
    d = disp_s.to(dtype)
    z = torch.log(d / (1 - d)).requires_grad_(True)
    sg = torch.sigmoid(z)
    disp = d + (sg - sg.detach())
    L = (R.upsample(disp, H, W) * ddisp_up.to(dtype)).sum()
    n = disp / (disp.mean((1, 2), keepdim=True) + 1e-7)
    fn = smooth_quirk if quirks else smooth_intended
    L = L + smooth_scale / 2 ** scale / 4 * (fn(n[:, None], rgb0_s.to(dtype), mask_s) * sample_w.to(dtype)).sum()
    g, = torch.autograd.grad(L, z)
    return g
