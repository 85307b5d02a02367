#!/usr/bin/env python
"""calc_error on a 4541-pose trajectory (KITTI 00's length; the seeded drive of tests/traj_eval_reference.py, tiled), each leg
timed ONCE after a warm-up call that loads the library:
  (a) clslam_hip.traj_eval.calc_error on two lists of 4x4 arrays (upload included),
  (b) the same on poses already on the device,
  (c) the float64 numpy restatement of the reference (tests/traj_eval_reference.calc_error) on this host.

    python tools/bench_traj_eval.py
"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / 'cl-slam_amd'), str(ROOT / 'tests')]

import torch  # noqa: E402

import traj_eval_reference as R  # noqa: E402
from clslam_hip import traj_eval  # noqa: E402


def main() -> None:
    pred, gt = R.make_fixture(1000, 0)
    pred, gt = R.tile(pred, 4541), R.tile(gt, 4541)
    P, G = list(pred), list(gt)
    traj_eval.calc_error(P[:20], G[:20])
    torch.cuda.synchronize()
    t = time.perf_counter()
    a = traj_eval.calc_error(P, G)
    t_lists = time.perf_counter() - t
    pd, gd = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    torch.cuda.synchronize()
    t = time.perf_counter()
    b = traj_eval.calc_error(pd, gd)
    t_device = time.perf_counter() - t
    t = time.perf_counter()
    c = R.calc_error(P, G)
    t_twin = time.perf_counter() - t
    print(f'calc_error, 4541 poses: lists of 4x4 {t_lists * 1e3:.2f} ms | device-resident {t_device * 1e3:.2f} ms | '
          f'numpy twin {t_twin * 1e3:.1f} ms | same text: {a == c and b == c}')
    print(a)


if __name__ == '__main__':
    main()
