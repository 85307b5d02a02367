"""The dense map at 192x640 with `--frames` frames (200: 24.6 M points, 590 MB) of synthetic planes resident in HBM:
  add_frame      one frame's planes -> its camera-frame cloud appended to the map (per frame, over a whole fill of the map);
  world_points   the whole map posed into the world (24 B/point read + 24 B/point written);
  render         one z-buffered view of the whole map, poses applied on the fly (24 B/point read).
Each as the API call (host clock around work that ends in a synchronise) and, for the two map-wide ones, as the kernels alone
(events around ops.pcl_transform / ops.pcl_to_image on prepared device arguments): warm-up, then `--blocks` timed blocks, the
median block with the smallest and largest; achieved bytes/s over the bytes the work must move.  The comparison is the
vectorised float64 numpy restatement of the same work on the host (tests/mapping_reference.py), timed once; the reference's own
shape of pcl_to_image, one Python iteration per point, is timed at one frame only.  Prints one JSON line.

    python tools/bench_map.py [--frames 200] [--blocks 7] [--no-host]
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

import mapping_reference as R                          # noqa: E402
from clslam_hip import mapping, ops                    # noqa: E402

H, W = 192, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    F, npx = args.frames, H * W
    K, inv = R.camera(H, W)
    poses = np.stack([R.frame_pose(f) for f in range(F)])
    gen = torch.Generator(device=dev).manual_seed(0)
    depth = 3 + 57 * torch.rand(F, 1, H, W, device=dev, generator=gen) ** 2
    image = torch.rand(F, 3, H, W, device=dev, generator=gen)
    inv_K = torch.from_numpy(inv).to(dev)[None].contiguous()
    M = F * npx

    m = mapping.DenseMap(capacity=M)

    def fill():
        m.clear()
        for f in range(F):
            m.add_frame(f, depth[f:f + 1], image[f:f + 1], inv_K)

    pose_list = list(poses)
    view = poses[F // 2]

    def timed(fn, reps, events=False):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        per_block = []
        for _ in range(args.blocks):
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                per_block.append(e0.elapsed_time(e1) / reps)
            else:
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                per_block.append((time.perf_counter() - t0) * 1e3 / reps)
        return {'median_ms': float(np.median(per_block)), 'min_ms': float(min(per_block)), 'max_ms': float(max(per_block))}

    def with_rate(t, nbytes):
        t['bytes'] = int(nbytes)
        t['TB_per_s'] = nbytes / (t['median_ms'] * 1e-3) / 1e12
        return t

    res = {'shape': f'{H}x{W}', 'frames': F, 'points': M, 'blocks': args.blocks, 'device': torch.cuda.get_device_name(0)}
    t = timed(fill, 1)
    res['add_frame'] = with_rate({k: v / F for k, v in t.items()}, npx * (16 + 24))
    fill()
    res['world_points'] = with_rate(timed(lambda: m.world_points(pose_list), args.reps), 48 * M)
    res['render'] = with_rate(timed(lambda: m.render(pose_list, view, K, (H, W)), args.reps), 24 * M)
    # the kernels alone
    pts, offsets = m.points, torch.from_numpy(m.offsets).to(dev)
    T = torch.from_numpy(poses).to(dev)
    Tv = torch.from_numpy(np.linalg.inv(view) @ poses).to(dev)
    Kd = torch.from_numpy(K).to(dev)
    out = torch.empty_like(pts)
    res['transform_kernel'] = with_rate(timed(lambda: ops.pcl_transform(pts, offsets, T, out=out), args.reps, events=True), 48 * M)
    res['splat_resolve_kernels'] = with_rate(timed(lambda: ops.pcl_to_image(pts, Kd, (H, W), offsets=offsets, poses=Tv), args.reps,
                                                   events=True), 24 * M)
    res['backproject_kernels'] = with_rate(timed(lambda: ops.pcl_backproject(depth[:1], inv_K, image[:1], out=out, narrow=False),
                                                 20, events=True), npx * (16 + 24))
    image_dev, index = ops.pcl_to_image(pts, Kd, (H, W), offsets=offsets, poses=Tv, return_index=True)
    res['render_occupied_pixels'] = int((index >= 0).sum())
    if not args.no_host:
        d0, i0 = depth[0, 0].cpu().numpy(), image[0].cpu().numpy()
        t0 = time.perf_counter()
        cloud0 = R.backproject(d0, inv, i0)['points'].astype(np.float32)
        res['host_numpy_add_frame_ms'] = (time.perf_counter() - t0) * 1e3
        host_pts, host_off = pts.cpu().numpy(), m.offsets
        t0 = time.perf_counter()
        xyz, _ = R.transform(host_pts, host_off, poses)
        res['host_numpy_world_points_ms'] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        seen, _ = R.transform(host_pts, host_off, np.linalg.inv(view) @ poses)
        z = R.zbuffer(np.concatenate([seen.astype(np.float32), host_pts[:, 3:]], axis=1), K, (H, W))
        res['host_numpy_render_ms'] = (time.perf_counter() - t0) * 1e3
        res['render_pixels_differing_from_host'] = int((z['index'] != index.cpu().numpy()).sum())
        t0 = time.perf_counter()
        R.pcl_to_image_loop(cloud0, K, (H, W))
        res['host_python_loop_one_frame_ms'] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(res))


if __name__ == '__main__':
    main()
