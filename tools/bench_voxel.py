"""The voxel-grid filter over the dense map at 192x640 with `--frames` frames (200: 24.6 M points, 590 MB) resident in HBM, posed
on the fly (DenseMap.world_points(poses, voxel_size)), at voxel sizes of 0.05, 0.2 and 1.0 m.  The scene is that of
tests/mapping_reference.py (depth 3 + 57 r^2, KITTI-like K, 0.8 m forward and 0.03 rad of yaw per frame), built on the device.

Per size: the API call (host clock around a call that ends in a synchronise) and the kernels alone (events around the two library
calls, clslam_pcl_voxel_sort and clslam_pcl_voxel_reduce, on prepared arguments; the 32-byte read-back between them is outside):
warm-up, then `--blocks` timed blocks, the median block with the smallest and largest.  `must move`: 36 B/point for the keys (24
read, 12 written), 32 B/point per radix pass that runs (8 read by the histogram, 12 read and 12 written by the scatter),
16 B/point for the two sweeps over the sorted keys, 28 B/point gathered by the reduction and 28 B per cell written; the rate is set
against the 6.29 TB/s a float4 copy reaches on this GPU.  The comparison is the vectorised numpy restatement
(np.unique on the keys, np.add.at in float64) of the same work on the host, timed once.  Prints one JSON line.

    python tools/bench_voxel.py [--frames 200] [--blocks 7] [--no-host]
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
import voxel_reference as V                            # noqa: E402
from clslam_hip import _lib, mapping, ops              # noqa: E402

H, W = 192, 640
COPY_TB_S = 6.29


def host_voxel(world, size):
    """np.unique on the keys, np.add.at of the float64 rows: -> (rows (V,6) float32, counts)"""
    k, keep = V.keys(world, size)
    uniq, inverse, counts = np.unique(k[keep], return_inverse=True, return_counts=True)
    sums = np.zeros((len(uniq), 6))
    np.add.at(sums, inverse, world[keep].astype(np.float64))
    return (sums / counts[:, None]).astype(np.float32), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--sizes', type=float, nargs='+', default=[0.05, 0.2, 1.0])
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    F, npx = args.frames, H * W
    _, inv = R.camera(H, W)
    poses = np.stack([R.frame_pose(f) for f in range(F)])
    gen = torch.Generator(device=dev).manual_seed(0)
    depth = 3 + 57 * torch.rand(F, 1, H, W, device=dev, generator=gen) ** 2
    image = torch.rand(F, 3, H, W, device=dev, generator=gen)
    inv_K = torch.from_numpy(inv).to(dev)[None].contiguous()
    M = F * npx
    m = mapping.DenseMap(capacity=M)
    for f in range(F):
        m.add_frame(f, depth[f:f + 1], image[f:f + 1], inv_K)
    del depth, image
    pose_list = list(poses)
    pts, offsets = m.points, torch.from_numpy(m.offsets).to(dev)
    T = torch.from_numpy(poses).to(dev)
    lib = _lib.get_lib()
    scratch = torch.empty(ops.pcl_voxel_scratch(M), dtype=torch.int64, device=dev)

    def block_times(fn, reps, events):
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
        return per_block

    def stats(per_block):
        return {'median_ms': float(np.median(per_block)), 'min_ms': float(min(per_block)), 'max_ms': float(max(per_block))}

    res = {'shape': f'{H}x{W}', 'frames': F, 'points': M, 'blocks': args.blocks, 'device': torch.cuda.get_device_name(0),
           'scratch_bytes': int(scratch.numel() * 8), 'copy_TB_per_s': COPY_TB_S, 'sizes': {}}
    stream = torch.cuda.current_stream(dev).cuda_stream
    for size in args.sizes:
        rows, counts, info = ops.pcl_voxel_downsample(pts, size, offsets=offsets, poses=T, return_info=True)
        cells = info['cells']
        out_rows, out_counts = torch.empty_like(rows), torch.empty_like(counts)

        def sort():
            lib.call('clslam_pcl_voxel_sort', pts.data_ptr(), offsets.data_ptr(), T.data_ptr(), F, M, float(size), 1, scratch.data_ptr(),
                     stream)

        def reduce():
            lib.call('clslam_pcl_voxel_reduce', pts.data_ptr(), offsets.data_ptr(), T.data_ptr(), F, M, scratch.data_ptr(),
                     out_rows.data_ptr(), out_counts.data_ptr(), cells, stream)

        r = {'cells': cells, 'passes': info['passes'], 'dropped': info['dropped'], 'largest_cell': int(counts.max()),
             'cells_of_one': int((counts == 1).sum())}
        r['api'] = stats(block_times(lambda: m.world_points(pose_list, size), args.reps, events=False))
        s, d = block_times(sort, args.reps, events=True), block_times(reduce, args.reps, events=True)
        r['sort_kernels'], r['reduce_kernel'] = stats(s), stats(d)
        r['kernels'] = stats([a + b for a, b in zip(s, d)])
        assert torch.equal(out_rows.view(torch.int32), rows.view(torch.int32)) and torch.equal(out_counts, counts)
        moved = M * (36 + 32 * info['passes'] + 16 + 28) + cells * 28
        r['bytes'] = int(moved)
        r['TB_per_s'] = moved / (r['kernels']['median_ms'] * 1e-3) / 1e12
        r['of_copy_rate'] = r['TB_per_s'] / COPY_TB_S
        if not args.no_host:
            world = m.world_points(pose_list).cpu().numpy()
            t0 = time.perf_counter()
            host_rows, host_counts = host_voxel(world, size)
            r['host_numpy_ms'] = (time.perf_counter() - t0) * 1e3
            del world
            r['counts_equal_host'] = bool(np.array_equal(host_counts, counts.cpu().numpy()))
            r['rows_differing_from_host_bitwise'] = int((host_rows.view(np.uint32) != rows.cpu().numpy().view(np.uint32)).any(axis=1).sum())
        res['sizes'][str(size)] = r
        del rows, counts, out_rows, out_counts
    print(json.dumps(res))


if __name__ == '__main__':
    main()
