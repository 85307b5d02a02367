"""Depth-error metrics of one frame, 192x640 prediction against a 376x1241 ground truth with 5 % valid pixels:
  (a) what a user does without the device evaluator: outputs['depth', 0][0].cpu().numpy() (and the ground truth's) plus the
      float32 numpy restatement of calc_depth_error on the host (tests/depth_eval_reference.py, dtype=float32);
  (b) clslam_hip.depth_eval.calc_depth_error on the device tensors (kernels + the 40-byte read-back);
  (c) the kernels alone, by events around ops.depth_metrics (no read-back).
Both in one process: warm-up, then `--blocks` blocks of `--reps` calls each; per leg the median over the blocks of the block's
mean per call, with the smallest and largest block.  Prints one JSON line.

    python tools/bench_depth_eval.py [--blocks 9] [--reps 20]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / 'cl-slam_amd', ROOT / 'tests'):
    sys.path.insert(0, str(p))

import depth_eval_reference as R                      # noqa: E402
from clslam_hip import depth_eval, ops                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    h, w, hg, wg, lo, hi = 192, 640, 376, 1241, 0.1, 80.0
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    pred = (3 + 57 * (0.5 + 0.3 * np.sin(5 * xx + yy) + 0.2 * np.cos(7 * yy))).astype(np.float32)
    gt = R.resample(pred.astype(np.float64), hg, wg, np.float64) * np.exp(rng.uniform(np.log(0.5), np.log(2.2), (hg, wg)))
    gt = (np.round(gt / 0.01) * 0.01).astype(np.float32)
    gt[rng.random((hg, wg)) >= 0.05] = 0.0
    # the planes as the predictor hands them out: (B,1,H,W) on the device
    depth_dev = torch.from_numpy(pred).to(dev)[None, None].contiguous()
    gt_dev = torch.from_numpy(gt).to(dev)[None, None].contiguous()

    def host_leg():
        r = R.evaluate(depth_dev[0].squeeze().cpu().numpy(), gt_dev[0].squeeze().cpu().numpy(), lo, hi, dtype=np.float32)
        return {k: float(r[k]) for k in R.KEYS}

    def device_leg():
        return depth_eval.calc_depth_error(depth_dev[0], gt_dev[0], min_depth=lo, max_depth=hi)

    out = torch.empty(1, 10, device=dev)

    def kernels_leg():
        ops.depth_metrics(depth_dev[0], gt_dev[0], lo, hi, out=out)

    a, b = host_leg(), device_leg()
    agree = max(abs(a[k] - b[k]) / max(abs(a[k]), 1e-30) for k in R.KEYS)

    def timed(fn, events=False):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        per_block = []
        for _ in range(args.blocks):
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                per_block.append(e0.elapsed_time(e1) / args.reps)
            else:
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                per_block.append((time.perf_counter() - t0) * 1e3 / args.reps)
        return {'median_ms': float(np.median(per_block)), 'min_ms': float(min(per_block)), 'max_ms': float(max(per_block))}

    res = {'shape': f'{h}x{w}->{hg}x{wg}', 'valid_pixels': int((gt > lo).sum()), 'blocks': args.blocks, 'reps': args.reps,
           'host_numpy_fp32': timed(host_leg), 'device_calc_depth_error': timed(device_leg),
           'device_kernels_only': timed(kernels_leg, events=True), 'largest_relative_difference_of_the_two': agree,
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
