"""PNG encoding on the device at 960x1280x3 (a rectified RobotCar frame): the launches' device time, the files' size against
Pillow and against zlib's Z_HUFFMAN_ONLY, and the offline pass undistort_images with both encoders.

Kernel rows: device events around `--reps` back-to-back ops.png_encode calls on a prepared device batch and output buffer (the
scratch allocation from torch's cache is inside), `--blocks` such blocks after a warm-up, the median block per call with the smallest
and largest.  `must move` per frame = the image read once and the filtered stream written (filter), read twice (plan, pack), the
output zeroed and written: 6 x the filtered size, set against the 6.29 TB/s a float4 copy reaches on this GPU.
Sizes: the device files of 8 frames against Pillow's default save of the same frames, and their deflate streams against
zlib.compressobj(strategy=Z_HUFFMAN_ONLY) of the very same filtered bytes (default level, so one block per zlib's buffer).
The pass: `--frames` synthetic raw PNGs (tools/bench_robotcar.py scene) in a temporary directory, undistort_images with each
encoder, alternating, `--passes` times each in this one session, a host clock around the call; the median per frame.  Every file of
the device encoder is decoded and compared with the Pillow encoder's before anything is timed.  Writes the report to `--out` and
prints one JSON line.

    python tools/bench_png.py [--out profiles/png_encode.txt] [--frames 32] [--workers 16]
"""
import argparse
import io
import json
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / 'cl-slam_amd', ROOT / 'tests', ROOT / 'tools'):
    sys.path.insert(0, str(p))

import png_reference as pref                           # noqa: E402
import robotcar_reference as ref                       # noqa: E402
from bench_robotcar import COPY_TB_S, H, W, scene      # noqa: E402
from clslam_hip import ops, png, robotcar              # noqa: E402

PARENT_PASS_MS = 24.79                                 # profiles/robotcar_rectify.txt section 3, the commit before this encoder


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'png_encode.txt'))
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lut_np, _ = ref.make_lut(H, W, seed=0, k1=0.05, shift=0.37)
    raw = scene(max(args.frames, 8))
    lut = torch.from_numpy(lut_np).to(dev)
    rgb8 = ops.robotcar_rectify(torch.from_numpy(raw[:8]).to(dev), lut, 'gbrg')
    lines = [f'PNG encoding on the device, MI355X, {H}x{W}x3 rectified frames (tools/bench_png.py)', '']

    # ---- results first ----
    files = png.encode_batch(rgb8)
    host8 = rgb8.cpu().numpy()
    for f, im in zip(files, host8):
        assert np.array_equal(np.array(Image.open(io.BytesIO(f))), im), 'a device file does not decode to its pixels'
    filtered0 = bytes(pref.filter_rows(host8[0])[0])
    pref.check_file(files[0], filtered0, H, W, 3)
    lines += ['0. Checked before timing: the 8 device files decode (Pillow) to their pixels; frame 0 inflates (zlib) to the numpy '
              'restatement of the filter, its chunk CRCs and Adler-32 equal zlib\'s.', '']

    # ---- 1. device time ----
    result = {}
    F = H * (1 + W * 3)
    lines += [f'1. ops.png_encode (memset, filter, plan, layout, pack, finish on one stream; device events, us per call: median of '
              f'{args.blocks} blocks of {args.reps} calls (min .. max), {args.warmup} warm-up calls)',
              f'   {"":8s} {"us / call":>10s}  {"(min .. max)":>22s}  {"us / frame":>10s}  {"must move":>10s}  {"rate":>10s}  of copy']
    for n in (1, 8):
        batch = rgb8[:n].contiguous()
        out = torch.empty(n, (ops.png_bound(H, W, 3) + 3) & ~3, dtype=torch.uint8, device=dev)
        for _ in range(args.warmup):
            ops.png_encode(batch, out=out)
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                ops.png_encode(batch, out=out)
            e1.record()
            e1.synchronize()
            per_call.append(e0.elapsed_time(e1) / args.reps * 1e3)
        med, lo, hi = float(np.median(per_call)), min(per_call), max(per_call)
        mb = 6 * F * n / 1e6
        lines.append(f'   N = {n}    {med:10.1f}  ({lo:9.1f} .. {hi:9.1f})  {med / n:10.1f}  {mb:7.1f} MB  {mb / med:5.2f} TB/s  '
                     f'{100 * mb / med / COPY_TB_S:5.1f} %')
        result[f'encode_us_n{n}'] = med
    lines.append('')

    # ---- 2. sizes ----
    pil_sizes, huff_sizes = [], []
    for im in host8:
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format='PNG')
        pil_sizes.append(len(buf.getvalue()))
        c = zlib.compressobj(strategy=zlib.Z_HUFFMAN_ONLY)
        filt = bytes(pref.filter_rows(im)[0])
        huff_sizes.append(len(c.compress(filt) + c.flush()))
    dev_sizes = [len(f) for f in files]
    dev_z = [len(f) - 57 for f in files]
    result.update(device_bytes=float(np.mean(dev_sizes)), pillow_bytes=float(np.mean(pil_sizes)), raw_bytes=H * W * 3,
                  size_vs_pillow=float(np.sum(dev_sizes) / np.sum(pil_sizes)), size_vs_huffman_only=float(np.sum(dev_z) / np.sum(huff_sizes)))
    lines += ['2. File size, mean of 8 frames (bytes)',
              f'   pixels                                              {H * W * 3:10d}',
              f'   device encoder (adaptive filter, Huffman only)      {np.mean(dev_sizes):10.0f}   {np.mean(dev_sizes) / (H * W * 3):.3f} of the pixels',
              f'   Pillow default save (zlib level 6 with LZ77)        {np.mean(pil_sizes):10.0f}   the device files are {result["size_vs_pillow"]:.3f} x these',
              f'   zlib stream, device / zlib Z_HUFFMAN_ONLY on the same filtered bytes: {np.mean(dev_z):.0f} / {np.mean(huff_sizes):.0f} = '
              f'{result["size_vs_huffman_only"]:.4f}',
              '   The device files are LARGER than Pillow\'s: there is no LZ77 matching.' if result['size_vs_pillow'] > 1 else
              '   The device files are not larger than Pillow\'s on these frames.', '']

    # ---- 3. the offline pass ----
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        models, centre = tmp / 'models', tmp / 'seq' / 'stereo' / 'centre'
        models.mkdir()
        centre.mkdir(parents=True)
        (models / 'stereo_narrow_left.txt').write_text('983.044006 983.044006 643.646973 493.378998\n0 0 1 0\n1 0 0 0\n0 1 0 0\n0 0 0 1\n')
        np.stack([lut_np[1].ravel(), lut_np[0].ravel()]).tofile(models / 'stereo_narrow_left_distortion_lut.bin')
        names = []
        for i in range(args.frames):
            names.append(f'{1400000000000000 + i}.png')
            Image.fromarray(raw[i]).save(centre / names[-1])
        old = robotcar.FRAME_SLICE
        robotcar.FRAME_SLICE = slice(0, None)
        times = {'pillow': [], 'device': []}
        try:
            for k in range(args.passes + 1):                             # pass 0 warms up and is compared, not timed
                for enc in ('pillow', 'device'):
                    out = tmp / f'{enc}{k}'
                    t0 = time.perf_counter()
                    robotcar.undistort_images(str(centre), str(models), data_path_out=str(out), batch=args.batch, workers=args.workers,
                                              encoder=enc)
                    if k:
                        times[enc].append((time.perf_counter() - t0) / args.frames * 1e3)
            for name in names:
                assert np.array_equal(np.array(Image.open(tmp / 'pillow0' / name)), np.array(Image.open(tmp / 'device0' / name)))
        finally:
            robotcar.FRAME_SLICE = old
    t_pil, t_dev = float(np.median(times['pillow'])), float(np.median(times['device']))
    result.update(pass_pillow_ms=t_pil, pass_device_ms=t_dev)
    lines += [f'3. undistort_images on {args.frames} synthetic raw PNGs, batch = {args.batch}, {args.workers} threads, the two encoders '
              f'alternating in one session (host clock, ms per frame: median of {args.passes} passes, all passes)',
              f'   encoder=\'pillow\' (the default)   {t_pil:8.2f}   {" ".join(f"{t:.2f}" for t in times["pillow"])}',
              f'   encoder=\'device\'                 {t_dev:8.2f}   {" ".join(f"{t:.2f}" for t in times["device"])}',
              f'   the commit before this encoder   {PARENT_PASS_MS:8.2f}   (profiles/robotcar_rectify.txt, another session)',
              f'   The device encoder makes the pass {t_pil / t_dev:.1f} x faster than the Pillow encoder here; the files on disk are '
              f'{result["size_vs_pillow"]:.2f} x the size.' if t_dev < t_pil else
              f'   The device encoder does NOT make the pass faster than the Pillow encoder here ({t_dev:.2f} against {t_pil:.2f} ms).', '']
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('\n'.join(lines))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
