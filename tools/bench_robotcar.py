"""RobotCar raw frames at 960x1280 (the stereo/centre frame size): the fused rectify kernel alone, fused against demosaic +
undistort, one frame against the scipy / numpy restatement on this host's CPU, and where the time of undistort_images goes.

Kernel rows: device events around `--reps` back-to-back calls on prepared device tensors, `--blocks` such blocks after a warm-up, the
median block per call with the smallest and largest.  `must move` = the table (16 B per pixel, once per launch) + per frame 1 B read
and 3 B written per pixel; the rate is set against the 6.29 TB/s a float4 copy reaches on this GPU.  The two-kernel
row also converts the float64 result to uint8 (torch, on the device), as a caller of the two kernels has to.  The offline pass runs
on `--frames` synthetic raw PNGs (a smooth scene with sensor noise under a gbrg mosaic) in a temporary directory: its stages one
after the other on `--workers` threads, then undistort_images itself (a host clock around the call).  Results are checked against
each other before anything is timed.  Writes the report to `--out` and prints one JSON line.

    python tools/bench_robotcar.py [--out profiles/robotcar_rectify.txt] [--frames 32] [--workers 16]
"""
import argparse
import json
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / 'cl-slam_amd', ROOT / 'tests'):
    sys.path.insert(0, str(p))

import robotcar_reference as ref                       # noqa: E402
from clslam_hip import ops, robotcar                   # noqa: E402

H, W = 960, 1280
COPY_TB_S = 6.29


def scene(n, seed=0):
    """n raw frames: smooth shapes that drift from frame to frame, sensor noise, sampled through a gbrg mosaic"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    r_m, g_m, b_m = ref.masks((H, W), 'gbrg')
    frames = []
    for i in range(n):
        rgb = [127 + 100 * np.sin((xx + 7 * i) / (40 + 25 * c)) * np.cos((yy - 3 * i) / (55 - 10 * c)) for c in range(3)]
        cfa = rgb[0] * r_m + rgb[1] * g_m + rgb[2] * b_m + rng.normal(0, 2.0, (H, W))
        frames.append(np.clip(cfa, 0, 255).astype(np.uint8))
    return np.stack(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'robotcar_rectify.txt'))
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lut_np, outside = ref.make_lut(H, W, seed=0, k1=0.05, shift=0.37)
    raw = scene(max(args.frames, 8))
    lut = torch.from_numpy(lut_np).to(dev)
    lines = [f'RobotCar raw frames, MI355X, {H}x{W}, pattern gbrg, {100 * outside:.1f} % of the table outside the image '
             '(tools/bench_robotcar.py)', '']

    def two_kernels(cfa):
        return (ops.undistort_lut(ops.demosaic_bilinear(cfa, 'gbrg'), lut).to(torch.int64) & 255).to(torch.uint8)

    def block_times(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            per_call.append(e0.elapsed_time(e1) / args.reps * 1e3)          # us
        return float(np.median(per_call)), min(per_call), max(per_call)

    # ---- results first: fused == two kernels == the CPU restatement (frame 0) ----
    d8 = torch.from_numpy(raw[:8]).to(dev)
    fused8 = ops.robotcar_rectify(d8, lut, 'gbrg')
    assert torch.equal(fused8, two_kernels(d8)), 'fused and two-kernel results differ'
    t0 = time.perf_counter()
    cpu = ref.load_image(raw[0], lut_np, 'gbrg')
    cpu_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(fused8[0].cpu().numpy(), cpu), 'the kernel and the CPU restatement differ'
    lines += ['0. Checked before timing: fused == demosaic + undistort on 8 frames, and frame 0 == the scipy / numpy restatement, byte for byte.', '']

    # ---- 1. kernels ----
    result = {'cpu_frame_ms': cpu_ms}
    lines += [f'1. Kernels (device events, us per call: median of {args.blocks} blocks of {args.reps} calls (min .. max), {args.warmup} warm-up calls)',
              f'   {"":44s} {"us / call":>10s}  {"(min .. max)":>20s}  {"us / frame":>10s}  {"must move":>10s}  {"rate":>10s}  of copy']
    for n in (1, 8):
        cfa = d8[:n].contiguous()
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        rows = [('clslam_robotcar_rectify (fused)', lambda: ops.robotcar_rectify(cfa, lut, 'gbrg', out=out)),
                ('demosaic + undistort + cast (three launches)', lambda: two_kernels(cfa))]
        for name, fn in rows:
            med, lo, hi = block_times(fn)
            mb = H * W * (16 + 4 * n) / 1e6
            tbs = mb / med                                               # MB / us = TB/s
            fused = name.startswith('clslam_robotcar')
            lines.append(f'   N = {n}  {name:44s} {med:10.1f}  ({lo:8.1f} .. {hi:8.1f})  {med / n:10.1f}  '
                         + (f'{mb:7.1f} MB  {tbs:5.2f} TB/s  {100 * tbs / COPY_TB_S:5.1f} %' if fused else f'{"":10s}  {"":10s}'))
            result[f'{"fused" if fused else "two_kernel"}_us_n{n}'] = med
    lines += [f'   (the two-kernel path also writes and re-reads a float64 image, {H * W * 24 / 1e6:.1f} MB per frame each way)',
              f'   fused against the two kernels: {result["two_kernel_us_n1"] / result["fused_us_n1"]:.1f} x at N = 1, '
              f'{result["two_kernel_us_n8"] / result["fused_us_n8"]:.1f} x at N = 8', '']

    # ---- 2. one frame on the CPU ----
    lines += ['2. One frame on this host\'s CPU: masks, three scipy.ndimage.convolve, three map_coordinates(order=1), the uint8 cast '
              '(tests/robotcar_reference.py load_image), one thread, timed once',
              f'   {cpu_ms:10.1f} ms   ({cpu_ms * 1e3 / result["fused_us_n1"]:.0f} x the fused kernel at N = 1)', '']

    # ---- 3. the offline pass ----
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        models, centre = tmp / 'models', tmp / 'seq' / 'stereo' / 'centre'
        models.mkdir()
        centre.mkdir(parents=True)
        (models / 'stereo_narrow_left.txt').write_text('983.044006 983.044006 643.646973 493.378998\n0 0 1 0\n1 0 0 0\n0 1 0 0\n0 0 0 1\n')
        np.stack([lut_np[1].ravel(), lut_np[0].ravel()]).tofile(models / 'stereo_narrow_left_distortion_lut.bin')
        files = []
        for i in range(args.frames):
            files.append(centre / f'{1400000000000000 + i}.png')
            Image.fromarray(raw[i]).save(files[-1])
        model = robotcar.CameraModel(models, centre)
        model.rectify(raw[:args.batch])                                      # warm-up: the table's upload, the first launch

        def decode(path):
            with Image.open(path) as im:
                return np.array(im)
        with ThreadPoolExecutor(max_workers=args.workers) as pool:
            t0 = time.perf_counter()
            decoded = list(pool.map(decode, files))
            t_dec = time.perf_counter() - t0
            t0 = time.perf_counter()
            rect = [model.rectify(np.stack(decoded[i:i + args.batch])) for i in range(0, len(files), args.batch)]
            torch.cuda.synchronize()
            t_gpu = time.perf_counter() - t0
            rect = np.concatenate(rect)
            (tmp / 'enc').mkdir()
            t0 = time.perf_counter()
            list(pool.map(lambda a: Image.fromarray(a[1]).save(tmp / 'enc' / f'{a[0]}.png'), enumerate(rect)))
            t_enc = time.perf_counter() - t0
        old = robotcar.FRAME_SLICE
        robotcar.FRAME_SLICE = slice(0, None)
        try:
            t0 = time.perf_counter()
            robotcar.undistort_images(str(centre), str(models), data_path_out=str(tmp / 'out'), batch=args.batch, workers=args.workers)
            t_all = time.perf_counter() - t0
        finally:
            robotcar.FRAME_SLICE = old
        assert np.array_equal(np.array(Image.open(tmp / 'out' / files[0].name)), cpu)
    F = args.frames
    lines += [f'3. undistort_images on {F} synthetic raw PNGs, batch = {args.batch}, {args.workers} threads (host clock, ms per frame)',
              f'   PNG decode (all frames, the pool)                       {t_dec / F * 1e3:8.2f}',
              f'   upload + fused kernel + download (batches, one thread)  {t_gpu / F * 1e3:8.2f}',
              f'   PNG encode (all frames, the pool)                       {t_enc / F * 1e3:8.2f}',
              f'   undistort_images, the stages overlapped                 {t_all / F * 1e3:8.2f}',
              f'   decode + encode are {100 * (t_dec + t_enc) / (t_dec + t_gpu + t_enc):.0f} % of the three stages; the kernel itself is '
              f'{result["fused_us_n8"] / 8 / 1e3:.3f} ms of a frame.', '']
    result.update(decode_ms=t_dec / F * 1e3, gpu_ms=t_gpu / F * 1e3, encode_ms=t_enc / F * 1e3, pass_ms=t_all / F * 1e3)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('\n'.join(lines))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
