"""TEST INFRASTRUCTURE: what tests/loss_reference.py lacks for the pair loss of predict_from_images (dpp.py:602-620 with
scales = (0,)): one source frame, two candidates, the seven loss scalars.  Same rules as that file: loop-free torch in
`dtype` (float64 the reference, float32 the yardstick), decisions (cell, clip, SSIM clamp) imposed through arguments,
nothing runs on the device."""
import torch

import loss_reference as R
from oracle import functional as OF

F64 = torch.float64


def view_and_maps(disp, src, target, Kinv, P, min_depth, max_depth, dtype=F64, cell=None, flag=None):
    """disp (B,H,W) scale-0 disparity of the target, src / target (B,3,H,W), P (B,3,4) -> depth (B,H,W), warped (B,3,H,W) on
    the imposed cells (default: this evaluation's own), maps (2,B,H,W) = [identity map, reprojection map] on the imposed
    clamp flags (2B,3,H,W) ordered [warped, src]; the own decisions and their margins as loss_reference returns them"""
    B, H, W = disp.shape
    P2 = torch.stack([P, P])
    w = R.warp_fwd(disp, src, src, Kinv, P2, H, W, min_depth, max_depth, dtype=dtype, cell=cell)
    warped = w['warped'][0]
    pm = R.photo_map(torch.cat([warped, src.to(dtype)]), target, dtype, flag)
    maps = torch.stack([pm['map'][B:], pm['map'][:B]])
    return dict(depth=w['depth'], warped=warped, maps=maps, cell=w['cell'], margins=w['margins'], ix=w['ix'], iy=w['iy'],
                flag=pm['flag'], flag_margin=pm['flag_margin'], raw=pm['raw'])


def select(maps, noise, dtype=F64):
    """maps (2,B,H,W) = [identity, reprojection], noise (B,1,H,W) or None -> candidates (2,B,H,W) = [identity + noise,
    reprojection], sel (B,H,W) (1: the reprojection is strictly smaller), the gap between the two"""
    c0 = maps[0].to(dtype) + (0 if noise is None else noise[:, 0].to(dtype))
    c = torch.stack([c0, maps[1].to(dtype)])
    return c, (c[1] < c[0]).long(), (c[1] - c[0]).abs()


def finalize(partial, disp, rgb0, pose, dist, sample_w, smooth_w, intended, H, W, smooth_scale, vel_scale, dtype=F64, chunks=32):
    """the seven scalars: reprojection, smooth, reg, depth_loss/scale_0, depth_loss (/ 4), velocity, loss.
    partial (B,nblk) block sums of the minimum; smoothness: the flattened terms of dpp.py:1148-1176 weighted by smooth_w
    (intended False) or the per-sample term weighted by sample_w (intended True); velocity: one frame."""
    sw = sample_w.to(dtype)
    d = disp.to(dtype)
    rl = ((partial.to(dtype).sum(1) / (H * W)) * sw).sum()
    sm = torch.zeros((), dtype=dtype)
    if intended:
        n = d / (d.mean((1, 2), keepdim=True) + 1e-7)
        sm = (OF.smooth_loss_intended(n[:, None], rgb0.to(dtype)) * sw).sum()
    elif smooth_w is not None and smooth_w.numel():
        n0 = d[0] / (d[0].mean() + 1e-7)
        dx, dy, term = R._smooth_terms(n0, rgb0[0].to(dtype), smooth_w.numel(), smooth_w.to(dtype))
        sm = term(dx, dy).sum()
    reg = smooth_scale * sm
    out = torch.zeros(7, dtype=dtype)
    out[0], out[1], out[2], out[3], out[4] = rl, sm, reg, rl + reg, (rl + reg) / 4
    total = out[4].clone()
    if vel_scale and vel_scale > 0:
        t = pose.to(dtype)[:, 3:6]
        out[5] = (vel_scale * (t.norm(dim=1) - dist.to(dtype).abs()).abs() * sw).sum()
        total = total + out[5]
    out[6] = total
    return out
