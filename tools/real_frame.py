#!/usr/bin/env python
"""The REAL adaptation frame of the SLAM loop, timed end to end on one MI355X (review r4 item 2): descriptor pass
(slam.py:143-147) + replay `get` of K samples (slam/replay_buffer.py:186-235,263-291: PNG -> LANCZOS pyramid -> ToTensor ->
colour jitter, per sample and frame) + concatenation with the online sample + adapt() + read-back of the pose and the losses
(slam.py:181-188), with the replay samples built
  (a) the reference's way: on the host with Pillow + torch CPU ops, then uploaded inside adapt(), and
  (b) by clslam_hip.ingest.ReplaySampleBuilder: PNG decode on the host (optionally cached), one uint8 upload, pyramid + jitter
      on the GPU, concatenation on the GPU, and
  (c) by the same builder with a frame store (store_bytes > 0, no host cache): every sample was added from the pyramid the online
      path holds at `add` time, `get` is two launches over bytes in HBM, cat_dict fills row 0.  Reported warm (steady state) and
      for the first frames after a restart (store empty: every sample is a miss, decoded and packed).
    python tools/real_frame.py [frames=40] [K=4] [modes: comma-separated substrings, default all]
    python tools/real_frame.py [frames=40] [K=4] online
The `online` mode times what stands in FRONT of all that, `online_data = next(self.online_dataloader_iter)` (slam.py:141), and the
whole frame behind it (replay from the frame store, mode (c)), on one tree of KITTI-sized PNGs, three runs each:
  (y) the parent's path: a dataset whose __getitem__ is datasets/kitti.py:231-317 (three PNGs, three LANCZOS chains, 24 ToTensor
      planes, with Pillow) behind DataLoader(batch_size=1, num_workers=0), and
  (t) clslam_hip.ingest.OnlineSampleBuilder installed on the same dataset object: its first frame and its steady state.
KITTI-sized PNGs (376x1241) are written to a temporary directory first.  Measurement tool (no parity claim: the parity of (b)
is tests/test_replay_ingest.py); the host-side jitter in (a) is a plain torch restatement good enough for timing."""
import pickle
import random
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'cl-slam_amd')); sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from PIL import Image  # noqa: E402
import bench  # noqa: E402
from clslam_hip import ingest, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 40
K = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ONLY = sys.argv[3].split(',') if len(sys.argv) > 3 else None
H, W, RAW_H, RAW_W, STORE = 192, 640, 376, 1241, 12
FRAMES, SCALES = (0, -1, 1), (0, 1, 2, 3)
work = Path(tempfile.mkdtemp())
rng = np.random.default_rng(0)
base = synth.make_batch(1, H, W, seed=0)
files = []
for i in range(STORE):
    sample = {k: v.clone() for k, v in base.items() if k[0] not in ('rgb', 'rgb_aug')}
    for f in FRAMES:
        img = (rng.random((RAW_H // 8, RAW_W // 8, 3)) * 255).astype(np.uint8)
        img = np.asarray(Image.fromarray(img).resize((RAW_W, RAW_H), Image.BICUBIC))
        png = work / f's{i}_{f}.png'
        Image.fromarray(img).save(png)
        sample['rgb', f] = png
    fn = work / f'kitti_{i:05}.pkl'
    with open(fn, 'wb') as fh:
        pickle.dump(sample, fh)
    files.append(fn)


def gray(x):
    return (0.2989 * x[..., 0:1, :, :] + 0.587 * x[..., 1:2, :, :] + 0.114 * x[..., 2:3, :, :])


def host_jitter(x, order, f):        # timing stand-in for torchvision's tensor ops on the CPU
    for op in order:
        if op == 0:
            x = (f[0] * x).clamp(0, 1)
        elif op == 1:
            x = (f[1] * x + (1 - f[1]) * gray(x).mean(dim=(-3, -2, -1), keepdim=True)).clamp(0, 1)
        elif op == 2:
            x = (f[2] * x + (1 - f[2]) * gray(x)).clamp(0, 1)
        else:                        # hue: HSV round trip (same operation count as functional_tensor.adjust_hue)
            mx, mn = x.max(-3).values, x.min(-3).values
            cr = mx - mn
            s = cr / torch.where(cr == 0, torch.ones_like(mx), mx)
            d = torch.where(cr == 0, torch.ones_like(cr), cr)
            r, g, b = x.unbind(-3)
            rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
            h = (mx == r) * (bc - gc) + ((mx == g) & (mx != r)) * (2 + rc - bc) + ((mx != g) & (mx != r)) * (4 + gc - rc)
            h = (torch.fmod(h / 6 + 1, 1) + f[3]) % 1.0
            i = torch.floor(h * 6); ff = h * 6 - i; i = i.to(torch.int64) % 6
            p_, q_, t_ = (mx * (1 - s)).clamp(0, 1), (mx * (1 - ff * s)).clamp(0, 1), (mx * (1 - s * (1 - ff))).clamp(0, 1)
            sel = lambda *c: torch.stack(c, -3).gather(-3, i.unsqueeze(-3)).squeeze(-3)     # noqa: E731
            x = torch.stack((sel(mx, q_, p_, p_, t_, mx), sel(t_, mx, mx, q_, p_, p_), sel(p_, p_, t_, mx, mx, q_)), -3)
    return x


def reference_get(fns):
    """slam/replay_buffer.py:263-291 on the host, K samples concatenated like `get` does"""
    out = None
    for fn in fns:
        order, f = ingest.draw_color_jitter()
        with open(fn, 'rb') as fh:
            data = pickle.load(fh)
        for frame in FRAMES:
            rgb = Image.open(data['rgb', frame]).convert('RGB')
            for s in SCALES:
                rgb = rgb.resize((W >> s, H >> s), Image.LANCZOS)
                t = torch.from_numpy(np.asarray(rgb, dtype=np.float32).transpose(2, 0, 1) / 255.0).unsqueeze(0)
                data['rgb', frame, s] = t
                data['rgb_aug', frame, s] = host_jitter(t, order, f)
            del data['rgb', frame]
        out = data if out is None else {k: torch.cat([out[k], data[k]]) for k in out}
    return out


p = bench.build_predictor(H, W, 1 + K)
p.optimizer.param_groups[0]['lr'] = 1e-6
dev = p.device
online_host = {k: v.pin_memory() for k, v in synth.make_batch(1, H, W, seed=3).items()}
builders = {'gpu ingest, PNGs decoded in one thread': ingest.ReplaySampleBuilder(H, W, SCALES, FRAMES, dev, decode_threads=1),
            'gpu ingest': ingest.ReplaySampleBuilder(H, W, SCALES, FRAMES, dev),            # 16 decode threads (default)
            'gpu ingest, decoded frames cached': ingest.ReplaySampleBuilder(H, W, SCALES, FRAMES, dev, cache_frames=3 * STORE)}
STORE_MODE = 'gpu ingest, frame store'
STORE_BYTES = STORE * ingest.FrameStore(H, W, SCALES, FRAMES, device=dev).slot_bytes


def store_builder(fill):
    b = ingest.ReplaySampleBuilder(H, W, SCALES, FRAMES, dev, store_bytes=STORE_BYTES)
    if fill:            # what replay_buffer.add sees: the online sample's own pyramid, host tensors
        for fn in files:
            data = builders['gpu ingest'].get_many([fn])[0]
            b.store.add_sample(fn, {k: v.cpu() for k, v in data.items() if k[0] == 'rgb'})
        assert b.store.inexact_pixels() == 0 and len(b.store) == STORE
    return b


builders[STORE_MODE] = store_builder(fill=True)
pick = np.random.default_rng(1)


DETAIL = {}
ONLINE_SOURCE = None          # `online` mode: where the frame's online sample comes from
NEXT_MS = []


def frame(mode, detail=False):
    sync = torch.cuda.synchronize if detail else (lambda: None)
    tick = time.perf_counter
    ta = tick()
    if ONLINE_SOURCE is None:
        online = dict(online_host)
    else:
        online = next(ONLINE_SOURCE)                                                                # slam.py:141
        NEXT_MS.append((tick() - ta) * 1e3)
    feat = p.models['depth_encoder'](online['rgb', 0, 0].to(dev))[4].mean(-1).mean(-1).cpu()      # slam.py:143-147
    sync()
    fns = [files[i] for i in pick.choice(STORE, K, replace=False)]
    t0 = time.perf_counter()
    if mode == 'reference get (host)':
        replay = reference_get(fns)
        t1 = time.perf_counter()
        training = {k: torch.cat([online[k], replay[k]]) for k in online if k in replay}              # slam.py:300-309
    else:
        if builders[mode].store is not None:
            replay = builders[mode].get_batch(fns)
        else:
            datas = builders[mode].get_many(fns)
            replay = {k: torch.cat([d[k] for d in datas]) for k in datas[0]}
        t1 = time.perf_counter()
        training = ingest.cat_dict(online, replay, dev)
    sync()
    t2 = tick()
    out, losses = p.adapt(None, training, steps=1)
    sync()
    t3 = tick()
    T = out['cam_T_cam', 0, 1][0, :].squeeze().cpu().numpy()
    vals = {k: float(v) for k, v in losses.items()}
    assert vals['loss'] == vals['loss'] and abs(T).max() < 1e3 and feat.shape == (1, 512)
    if detail:
        for name, v in (('descriptor', t0 - ta), ('get', t1 - t0), ('cat', t2 - t1), ('adapt', t3 - t2), ('read-back', tick() - t3)):
            DETAIL[name] = DETAIL.get(name, 0.0) + v
    return t1 - t0


class KittiShaped:
    """datasets/kitti.py:231-317 with Pillow (torchvision's Resize(LANCZOS) / ToTensor of PIL images are these calls), as far as the
    driver's configuration uses it; the camera matrices are synth's, so that its samples join the stored ones"""

    def __init__(self, root, n_files):
        self.frame_ids, self.scales, self.height, self.width = sorted(FRAMES), SCALES, H, W
        self.do_augmentation, self.views, self.with_depth, self.with_mask, self.include_poses = False, ('left',), False, False, True
        self.left_img_filenames = []
        for i in range(n_files):
            img = (rng.random((RAW_H // 8, RAW_W // 8, 3)) * 255).astype(np.uint8)
            self.left_img_filenames.append(root / f'{i:06}.png')
            Image.fromarray(img).resize((RAW_W, RAW_H), Image.BICUBIC).save(self.left_img_filenames[-1])
        self.camera_matrix = np.eye(4, dtype=np.float32)
        self.relative_distances = [0.] + [0.8] * (n_files - 1)
        self.global_poses = [np.eye(4, dtype=np.float32)] * n_files
        self.relative_poses = np.stack(self.global_poses)

    def __len__(self):
        return len(self.left_img_filenames) - 2

    def _scale_camera_matrix(self, camera_matrix, scale):
        k, kinv = synth.camera_matrices(H, W, scale)
        return np.asarray(k), np.asarray(kinv, dtype=np.float32)

    def _pre_getitem(self, index):
        if index < 0 or index >= len(self):
            raise IndexError()
        return self.left_img_filenames, [], index + 1, False, False

    def __getitem__(self, index):
        names, _, index, _, _ = self._pre_getitem(index)
        item, planes = {'index': index}, {}
        for f in self.frame_ids:
            rgb = Image.open(names[index + f]).convert('RGB')
            for s in self.scales:
                rgb = rgb.resize((W >> s, H >> s), Image.LANCZOS)
                planes['rgb', f, s] = rgb
        for s in range(len(self.scales)):
            k, kinv = self._scale_camera_matrix(self.camera_matrix, s)
            item['camera_matrix', s], item['inv_camera_matrix', s] = torch.from_numpy(k.copy()), torch.from_numpy(kinv.copy())
        for f in self.frame_ids[1:]:
            item['relative_distance', f] = self.relative_distances[index + f]
        for f in self.frame_ids[1:]:
            item['relative_pose', f] = torch.from_numpy(self.relative_poses[index + f][None].copy())
            item['absolute_pose', f] = torch.from_numpy(self.global_poses[index + f][None].copy())
        for kind in ('rgb', 'rgb_aug'):
            for (_, f, s), img in planes.items():
                item[kind, f, s] = torch.from_numpy(np.asarray(img).transpose(2, 0, 1).copy()).to(torch.float32).div(255)
        return item


def online_mode():
    global ONLINE_SOURCE
    from types import SimpleNamespace
    from torch.utils.data import DataLoader
    tree = work / 'image_2'
    tree.mkdir()
    ds = KittiShaped(tree, N + 3)
    print(f'online sample + real frame @{H}x{W} ({RAW_H}x{RAW_W} PNGs), K = {K} replay samples from the frame store, 3 runs of 1 + {N} frames')
    for _ in range(STORE):                                    # warm the step and the store up on the synthetic online sample
        frame(STORE_MODE)
    results = {}
    for name in ('DataLoader(num_workers=0), host __getitem__', 'OnlineSampleBuilder'):
        for run in range(3):
            slam = SimpleNamespace(online_dataset=ds, online_dataloader_iter=iter(DataLoader(ds, batch_size=1, num_workers=0)))
            builder = ingest.OnlineSampleBuilder(ds, dev).install(slam) if name == 'OnlineSampleBuilder' else None
            ONLINE_SOURCE = slam.online_dataloader_iter
            NEXT_MS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frame(STORE_MODE)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(N):
                frame(STORE_MODE)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            results.setdefault(name, []).append((NEXT_MS[0], (t1 - t0) * 1e3, sum(NEXT_MS[1:]) / N, (t2 - t1) / N * 1e3))
            if builder is not None:
                builder.close()
                ds.__class__ = KittiShaped                     # the next run starts from the dataset's own class again
        ONLINE_SOURCE = None
    for name, runs in results.items():
        for label, col in (('first frame : next()', 0), ('first frame : whole frame', 1), ('steady state: next()', 2),
                           ('steady state: whole frame', 3)):
            v = [r[col] for r in runs]
            print(f'  {name:44s} {label:26s}: {sorted(v)[1]:8.2f} ms  (3 runs: {min(v):.2f} .. {max(v):.2f})')
    # the share of the one new PNG per frame: its decode alone, on this host thread
    t0 = time.perf_counter()
    for fn in ds.left_img_filenames[:10]:
        np.asarray(Image.open(fn).convert('RGB'))
    print(f'  decode of one {RAW_H}x{RAW_W} PNG, one thread: {(time.perf_counter() - t0) / 10 * 1e3:.2f} ms')


if ONLY == ['online']:
    online_mode()
    sys.exit(0)

print(f'real frame @{H}x{W}, K = {K} replay samples from a store of {STORE} ({RAW_H}x{RAW_W} PNGs), {N} frames per mode')
for mode in ('reference get (host)', 'gpu ingest, PNGs decoded in one thread', 'gpu ingest', 'gpu ingest, decoded frames cached',
             STORE_MODE):
    if ONLY is not None and not any(o in mode for o in ONLY):
        continue
    random.seed(0)
    for _ in range(3 if mode == 'reference get (host)' else STORE):        # warm-up (and fill the decoded-frame cache)
        frame(mode)
    torch.cuda.synchronize()
    n = max(4, N // 4) if mode == 'reference get (host)' else N
    t0 = time.perf_counter()
    tg = 0.0
    for _ in range(n):
        tg += frame(mode)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n * 1e3
    print(f'  {mode:36s}: {dt:8.2f} ms per frame  ({1e3 / dt:6.1f} frames/s)   of which `get`: {tg / n * 1e3:7.2f} ms')
    if mode != 'reference get (host)':
        DETAIL.clear()
        for _ in range(10):
            frame(mode, detail=True)
        print('      stage by stage, a synchronize between the stages (ms):', {k: round(v / 10 * 1e3, 2) for k, v in DETAIL.items()})

if ONLY is None or any(o in STORE_MODE for o in ONLY):
    # first sight after a restart: the store is empty, every one of the K samples is decoded, built by the PNG path and packed.
    # One builder; its first frame (tap plans, decode pool, the store's allocation: once per process) is not counted.
    first = 'first sight after restart'
    builders[first] = store_builder(fill=False)
    frame(first)
    tf = tg = 0.0
    for _ in range(5):
        for fn in files:
            builders[first].store.drop(fn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tg += frame(first)
        torch.cuda.synchronize()
        tf += time.perf_counter() - t0
    builders[first].close()
    print(f'  {STORE_MODE + ", " + first:36s}: {tf / 5 * 1e3:8.2f} ms per frame  (5 frames, each on an empty store)   of which `get`: '
          f'{tg / 5 * 1e3:7.2f} ms')
