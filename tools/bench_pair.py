#!/usr/bin/env python
"""Latency of predict_from_images at 192x640, N = 1, device outputs (as_numpy=False), with return_loss off and on, beside the
composition a caller had to write before: predict_from_image x 2 + predict_pose.  Per variant: warm-up, then BLOCKS blocks
of CALLS calls, each call synchronised; the median block and the range of the blocks are reported.  With return_loss the loss
scalars are read back (they are numpy by contract), so that variant includes one 28-byte device-to-host copy.

    python tools/bench_pair.py [--out profiles/pair_loss.txt]      # timing
    python tools/bench_pair.py --kernels fused|chain               # a few launches of the loss kernels alone, for a kernel trace

--kernels runs only the scale-0 loss stage on fixed inputs: `fused` = pair_loss + pair_loss_finalize, `chain` = what the
library offered before: warp_fwd (the frame in both source slots), photo_map x 2, a two-way minimum by torch."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'cl-slam_amd'))
import bench  # noqa: E402
from clslam_hip import ops, synth  # noqa: E402

H, W = 192, 640
WARMUP, CALLS, BLOCKS = 20, 50, 7


def blocks(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / CALLS * 1e3)
    return statistics.median(out), min(out), max(out)


def kernels(which: str) -> None:
    dev = torch.device('cuda')
    b = {k: v.to(dev) for k, v in synth.make_batch(1, H, W, seed=0).items()}
    src, tgt = b['rgb', -1, 0].contiguous(), b['rgb', 0, 0].contiguous()
    disp = (0.2 + 0.6 * torch.rand(1, H, W, device=dev)).contiguous()
    K, Kinv = b['camera_matrix', 0].contiguous(), b['inv_camera_matrix', 0].contiguous()
    pose = torch.zeros(2, 12, device=dev)
    pose[:, 3] = 0.05
    T, P = torch.empty(2, 1, 4, 4, device=dev), torch.empty(2, 1, 3, 4, device=dev)
    ops.pose_to_proj(pose, K, T, P)
    noise = (1e-5 * torch.randn(1, 1, H, W, device=dev)).contiguous()
    partial = torch.empty(1, ops.automask_blocks(H, W), device=dev)
    losses, scratch = torch.empty(7, device=dev), torch.empty(ops.pair_loss_scratch(1), device=dev)
    sw = torch.ones(1, device=dev)
    depth, warped = torch.empty(1, H, W, device=dev), torch.empty(2, 1, 3, H, W, device=dev)
    rp, idm = torch.empty(1, H, W, device=dev), torch.empty(1, H, W, device=dev)
    for _ in range(12):
        if which == 'fused':
            ops.pair_loss(disp, src, tgt, Kinv, P[0].contiguous(), noise, partial, 0.1, None)
            ops.pair_loss_finalize(partial, disp, tgt, pose[:1].contiguous(), None, sw, sw, False, scratch, losses, 1e-3, 0.0)
        else:
            ops.warp_fwd(disp, src, src, Kinv, P, depth, warped, 0.1, None)
            ops.photo_map(warped[0], tgt, rp, None, 1, 1, H, W)
            ops.photo_map(src, tgt, idm, None, 1, 1, H, W)
            torch.minimum(idm + noise[:, 0], rp).mean()
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels', choices=['fused', 'chain'], default=None)
    args = ap.parse_args()
    if args.kernels:
        kernels(args.kernels)
        return
    p = bench.build_predictor(H, W, 1)
    b = {k: v.cuda() for k, v in synth.make_batch(1, H, W, seed=0).items()}
    i0, i1 = b['rgb', -1, 0], b['rgb', 0, 0]
    cal = dict(camera_matrix=b['camera_matrix', 0], inv_camera_matrix=b['inv_camera_matrix', 0], relative_distance=b['relative_distance', 0])
    rows = [('predict_from_image x 2 + predict_pose (before)', lambda: (p.predict_from_image(i0, as_numpy=False), p.predict_from_image(i1, as_numpy=False),
                                                                        p.predict_pose(i0, i1, as_numpy=False))),
            ('predict_from_images(return_loss=False)', lambda: p.predict_from_images(i0, i1, as_numpy=False)),
            ('predict_from_images(return_loss=True)', lambda: p.predict_from_images(i0, i1, as_numpy=False, return_loss=True, **cal))]
    lines = [f'predict_from_images, {H}x{W}, N = 1, device outputs; ms per synchronised call: median of {BLOCKS} blocks of {CALLS} calls '
             f'(min .. max of the blocks), {WARMUP} warm-up calls; {torch.cuda.get_device_name(0)}']
    for name, fn in rows:
        med, lo, hi = blocks(fn)
        lines.append(f'  {name:52s} {med:7.3f}  ({lo:.3f} .. {hi:.3f})')
    # bytes the fused loss kernel moves, from the shapes: disparity + source + target read once, the partials written
    nbytes = (1 + 3 + 3) * H * W * 4 + ops.automask_blocks(H, W) * 4
    lines.append(f'  fused loss kernel: {nbytes} bytes by the shapes (disparity, source, target read once; {ops.automask_blocks(H, W)} partials written)')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + '\n')


if __name__ == '__main__':
    main()
