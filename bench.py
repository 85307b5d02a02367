#!/usr/bin/env python
"""Headline benchmark: online-adaptation frames/sec of the depth/pose hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--replay R] [--height 192 --width 640]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one `DepthPosePrediction.adapt(online, training, steps=1)`: forward of both networks,
view synthesis + loss, hand-written backward, fused Adam -- on a synthetic minibatch of 1 online
triplet + R replayed triplets that is already resident in HBM when the timed region starts (bench contract), followed by
what slam/slam.py:181-188 does with the result every frame: the online sample's pose and every loss scalar read back to
the host (`--no-readback` leaves that out), on the product's DEFAULT boundary -- outputs and losses are device tensors
exactly like the reference's (`--host-outputs` times the opt-in host-output path instead).  The PCIe-inclusive frame of SURVEY.md 8(d) (pinned host minibatch -> H2D
inside adapt()) is measured by the same run with `--full` and reported under `also.end_to_end`; by the contract it is never `value`.
N = 1 runs BASELINE config 3 (R = 4, B = 5, the configuration the 30 frames/s target is quoted on);
`--replay R` selects another replay count (R = 0 is BASELINE config 2).
N > 1 shards a minibatch data-parallel with ONE sum-all-reduce of the flat gradient arena per step over
RCCL/xGMI.  By default every rank gets the N = 1 shard size, 1+R triplets (rank 0: the online triplet + R
replayed ones, the others 1+R replayed ones; B = N*(1+R), K = B-1), so per-GPU work is exactly fixed as N
grows ("weak").  `--total-replay K` instead shards a minibatch of 1+K triplets as evenly as possible
(`--gpus 8 --total-replay 32` is BASELINE config 4: shards 5,4,4,4,4,4,4,4).  `value` counts frames of
(1+R) triplets: value = steps/s * B/(1+R), so N = 1 is plain frames/s.

Rank 0 prints ONE JSON line (contract in the task description).  A plain run sets up, warms up (`--warmup W` steps), times
EXACTLY `--steps K` steps (one timed block; `--blocks n` repeats it and reports the median block), writes the last timed step's
outputs if `--dump-outputs DIR` is given, and prints that line.  Everything else is measured only with `--full`:
`roofline` (dominant kernel: the fp32-MFMA conv, algorithmic FLOPs / the launches' own start-stop HIP events --
hipExtLaunchKernel timestamps taken by the library, the duration rocprofv3 reports -- vs the 157.3 TFLOP/s fp32 matrix peak),
`cpu_baseline` (the oracle's torch-CPU restatement of the same step, timed on this box's host cores on a bounded sample),
`repeated_blocks` (the timed block run 25 more times: spread and bitwise replica check), `also` (the reference's 5-step frame and
the end-to-end frame) and, with N > 1, `gradient_exchange`.

`--dump-outputs DIR` writes what the caller of the timed path receives from its last step -- every tensor of the outputs dict
adapt() returns, every loss scalar and, with `--lcd`, the loop-closure feature -- as DIR/<name>.npy (float32; the key's parts
joined by '_', loss keys prefixed `loss_`).  An array larger than the per-array cap (64 MB in all) is written as a fixed sample
of its flattened elements: the same seeded indices for the same shape, so two builds compare output for output.  The inputs
(weights, minibatch, tie-break noise) are seeded: the same arguments give the same inputs in every run.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / 'cl-slam_amd'))
sys.path.insert(0, str(ROOT))
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import torch  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4_f32
REPEAT_BLOCKS = 25              # --full: extra timed blocks for the spread of the headline statistic


def build_predictor(H, W, B_cfg, host_outputs=False):
    from types import SimpleNamespace
    from clslam_hip import synth
    from depth_pose_prediction import Config, DepthPosePrediction
    ds = SimpleNamespace(dataset='Kitti', config_file=Path('x.yaml'), dataset_path=None, scales=(0, 1, 2, 3), height=H,
                         width=W, frame_ids=(0, -1, 1))
    cfg = Config(config_file=Path('x.yaml'), train_set='all', val_set=0, resnet_depth=18, resnet_pose=18,
                 resnet_pretrained=False, scales=(0, 1, 2, 3), learning_rate=1e-4, scheduler_step_size=15,
                 batch_size=B_cfg, num_workers=0, num_epochs=1, min_depth=0.1, max_depth=None, disparity_smoothness=1e-3,
                 velocity_loss_scaling=0.05, mask_dynamic=False, log_path=Path('/tmp/clslam_bench'), save_frequency=-1,
                 save_val_depth=False, save_val_depth_batches=0, multiple_gpus=False, gpu_ids=None,
                 load_weights_folder=None, use_wandb=False)
    # host_outputs: the opt-in fast path of the product (pose + losses handed out as host tensors staged behind the forward,
    # DepthPosePrediction(host_pose_output=True) / CLSLAM_HOST_POSE=1); False = the reference's behaviour (device tensors)
    p = DepthPosePrediction(ds, cfg, host_pose_output=host_outputs)
    for name, m in p.models.items():  # random-init weights of the reference architecture (closed form)
        m.load_state_dict(synth.fill_state_dict(torch.nn.Module.state_dict(m), 0, name))
    p.is_trained = True
    return p


def cpu_baseline(H, W, B, budget_s=25.0):
    """The oracle (torch-CPU port of the reference step, validated against the reference's golden
    vectors) on this host's cores; bounded sample.  torch's default of one thread per hardware thread is far
    from the best setting on a many-core host (measured on the MI355X box: 3.9 s/step with 128 threads, 0.59 s
    with 32), so a short sweep picks the thread count first and the baseline is timed at the fastest one."""
    from clslam_hip import synth
    from oracle import OraclePredictor
    default_threads = torch.get_num_threads()
    o = OraclePredictor(H, W, B)
    for name, m in o.models.items():
        m.load_state_dict(synth.fill_state_dict(m.state_dict(), 0, name))
    batch = synth.make_batch(B, H, W, seed=0)
    t_all = time.time()

    def one():
        t0 = time.time()
        o.adapt(batch, steps=1)
        return time.time() - t0
    sweep = {}
    for n in sorted({min(default_threads, c) for c in (8, 16, 32, 64)} | {default_threads}):
        if time.time() - t_all > 0.6 * budget_s and sweep:
            break
        torch.set_num_threads(n)
        one()                                    # warm-up at this setting
        sweep[n] = one()
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    times = [sweep[best]]
    while len(times) < 5 and (time.time() - t_all) < budget_s:
        times.append(one())
    torch.set_num_threads(default_threads)
    times.sort()
    med = times[len(times) // 2]
    return {'value': round(1.0 / med, 4), 'unit': 'frames/s', 'cores': best, 'kind': 'port',
            # BASELINE.md section 3 asks for N = 8 threads and N = all hardware threads as well: single steps of the sweep
            'frames_per_s_at_8_threads': round(1.0 / sweep[8], 4) if 8 in sweep else None,
            'frames_per_s_at_all_threads': round(1.0 / sweep[default_threads], 4) if default_threads in sweep else None,
            'all_threads': default_threads,
            'sample': f'{len(times)} adapt steps of the same B={B} {H}x{W} minibatch, torch {torch.__version__} CPU fp32, '
                      f'median {med:.3f} s/step at {best} threads (sweep s/step: '
                      + ', '.join(f'{n}: {t:.2f}' for n, t in sweep.items()) + ')'}


DUMP_MAX_BYTES = 64 << 20       # all arrays of --dump-outputs together
DUMP_MAX_ELEMS = 1 << 19        # per array (2 MB of float32); a larger output is written as a seeded sample of its elements


def dump_outputs(out_dir, outputs, losses, lcd_feature=None):
    """The last timed step's results as out_dir/<name>.npy in float32 (float64 stays float64).  Arrays above the per-array cap
    are flattened and sampled at indices drawn from a generator seeded with 0: a function of the array's size only."""
    import re
    import numpy as np

    def name_of(key):
        parts = key if isinstance(key, tuple) else (key,)
        return re.sub(r'[^A-Za-z0-9_.-]', '_', '_'.join(str(x) for x in parts))
    arrays = {name_of(k): v for k, v in outputs.items() if isinstance(v, torch.Tensor)}
    arrays.update({'loss_' + name_of(k): v for k, v in losses.items() if isinstance(v, torch.Tensor)})
    if lcd_feature is not None:
        arrays['lcd_feature'] = lcd_feature
    # the small arrays (pose, losses, features) whole; the 64 MB that remain shared by the large ones (8 bytes per element:
    # float64 at worst)
    small = [t for t in arrays.values() if t.numel() <= 4096]
    budget = DUMP_MAX_BYTES - sum(8 * t.numel() for t in small)
    cap = max(4096, min(DUMP_MAX_ELEMS, budget // (8 * max(1, len(arrays) - len(small)))))
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    total, sampled = 0, []
    for name, t in sorted(arrays.items()):
        a = t.detach().to('cpu', torch.float64 if t.dtype == torch.float64 else torch.float32)
        if a.numel() > cap:
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:cap].sort().values
            a = a.reshape(-1)[idx]
            sampled.append(name)
        a = a.numpy()
        np.save(out_dir / f'{name}.npy', a)
        total += a.nbytes
    assert total <= DUMP_MAX_BYTES, total
    return {'dir': str(out_dir), 'arrays': len(arrays), 'bytes': total, 'sampled': sampled, 'sample_elements': cap}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)      # 0.33 s timed at 3.2 ms per step
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=1, help='how many times the timed block of `steps` steps is repeated; the median '
                    'block is reported (ms_per_step), min / max beside it')
    ap.add_argument('--full', action='store_true', help='also measure everything beside the headline: roofline pass, CPU baseline, '
                    'repeated blocks, 5-step and end-to-end frames, per-rank gradient exchange (off: only the timed steps)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write the outputs of the last timed step as DIR/<name>.npy')
    ap.add_argument('--replay', type=int, default=4, help='replay triplets of the N=1 minibatch; every rank gets 1+replay triplets')
    ap.add_argument('--total-replay', type=int, default=None, help='shard a minibatch of 1+K triplets over the ranks instead '
                    '(8 GPUs, K=32: BASELINE config 4)')
    ap.add_argument('--adapt-steps', type=int, default=1, help='optimizer steps per adapt() call (S); the headline metric is '
                    'S=1, the reference\'s config_adapt.yaml runs S=5')
    ap.add_argument('--height', type=int, default=192)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--random-images', action='store_true', help='uniform-random image content instead of the smooth synthetic '
                    'frames (SURVEY.md 8d: the photometric min / mask then flips per pixel -- worst case for the loss stage)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-readback', action='store_true', help='do not read the pose and the loss scalars back to the host inside '
                    'the timed region of `value` (slam.py:181-188 does, every frame)')
    ap.add_argument('--host-outputs', action='store_true', help='time the product\'s OPT-IN host-output path (host_pose_output=True: '
                    'pose + losses handed out as host tensors staged behind the forward) instead of the default boundary '
                    '(device tensors like the reference; the training step runs detached on the engine\'s stream)')
    ap.add_argument('--device-outputs', action='store_true', help='(default since round 4; kept for old command lines)')
    ap.add_argument('--lcd', action='store_true', help='BASELINE config 5: the loop-closure encoder forward on rgb(+1, 0) of the online '
                    'frame inside every timed frame (slam.py:223 -> loop_closure_detection.py:41-51); closed-form weights, '
                    'parity of that encoder is UNPINNED (DESIGN.md)')
    ap.add_argument('--no-also', action='store_true', help='skip the extra adapt(steps=5) timing (profiling runs)')
    ap.add_argument('--backend', default='nccl', help='torch.distributed backend for --gpus > 1 (nccl = RCCL; gloo lets two '
                    'ranks share one GPU for a functional check of the sharded path)')
    ap.add_argument('--dump-convs', action='store_true', help='per-launch conv timings to stderr')
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit('--steps must be at least 1')
    H, W, N = args.height, args.width, args.gpus

    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != N:
        raise SystemExit(f'--gpus {N} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {N}')
    if args.backend != 'nccl':
        local_rank %= torch.cuda.device_count()      # functional check: ranks may share a GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    dist = None
    if N > 1:
        import torch.distributed as dist
        if args.backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)
        else:
            dist.init_process_group(args.backend)

    FRAME_TRIPLETS = 1 + args.replay   # a "frame" = the N=1 minibatch: 1 online + R replay triplets
    B = N * FRAME_TRIPLETS if args.total_replay is None else 1 + args.total_replay
    K = B - 1
    # contiguous shards, rank 0 holds the online sample (+ the remainder)
    base, rem = divmod(B, N)
    counts = [base + (1 if r < rem else 0) for r in range(N)]
    offset = sum(counts[:rank])
    Bl = counts[rank]

    from clslam_hip import _lib, ops, synth
    build_id = _lib.build_id()
    torch.manual_seed(1 + rank)          # the tie-break noise is drawn on the device: same trajectory every run
    p = build_predictor(H, W, B if N == 1 else max(Bl, 1), host_outputs=args.host_outputs)   # (a rank may hold no sample: --total-replay K < N-1)
    if N > 1:
        p.enable_data_parallel(B, offset)
    full = synth.make_batch(B, H, W, seed=0)
    if args.random_images:
        g = torch.Generator().manual_seed(1234)
        for k in list(full):
            if k[0] in ('rgb', 'rgb_aug'):
                full[k] = torch.rand(full[k].shape, generator=g)
    shard = {k: v[offset:offset + Bl].contiguous() for k, v in full.items()}
    batch = {k: v.to(dev) for k, v in shard.items()}
    if args.random_images:
        # training the untrained synthetic network on noise is degenerate (the disparity collapses to 0 within tens of steps
        # and the reference's NaN guard fires, dpp.py:1115): the timing run keeps the weights in place -- same kernels, lr ~ 0
        p.optimizer.param_groups[0]['lr'] = 1e-12

    S = args.adapt_steps

    def consume(outputs, losses):
        """what slam/slam.py:182-192 reads back after every adapt(): the online sample's pose and the loss scalars"""
        T = outputs['cam_T_cam', 0, 1][0, :].squeeze().cpu().detach().numpy()
        vals = {k: float(v.squeeze().cpu().detach().numpy()) for k, v in losses.items()}
        return T, vals

    lcd_enc = None
    if args.lcd and rank == 0:
        from clslam_hip import lcd as lcd_mod
        from loop_closure_detection import FeatureEncoder
        lcd_enc = FeatureEncoder(dev, weights=lcd_mod.synthetic_state_dict())
        lcd_image = batch['rgb', 1, 0][0]

    # The synthetic network is UNTRAINED (closed-form weights): trained over and over on one minibatch its disparity saturates
    # within ~25 optimizer steps and, a few dozen steps later, one scale collapses to disp ~ 1e-20 -- depth = min_depth / disp
    # (utils.py:120-142 with max_depth None) and its derivative -min_depth / disp^2 overflow fp32, the gradient turns NaN in the
    # reference's arithmetic as much as here, and the NaN guard of dpp.py:1115-1118 ends the run (tools/diag_nan.py,
    # profiles/r05_degenerate_minibatch.txt: step 43 of this minibatch).  A benchmark that repeats its timed block 25 times
    # would walk into that, so the trainable state (weights, both Adam moments, step count) goes back to its post-warmup value
    # every RESTORE_EVERY optimizer steps: three device-to-device copies (54 MB, ~25 us) ordered on the stream like any
    # other work of the caller -- inside the timed region when a block is longer than that, i.e. counted against the result.
    RESTORE_EVERY = 20
    state0 = None
    since_restore = [0]

    def snapshot_state():
        nonlocal state0
        eng = p.engine
        state0 = (eng.w.clone(), eng.m.clone(), eng.v.clone(), eng.adam_step_count, torch.cuda.default_generators[dev.index].get_offset())
        since_restore[0] = 0

    def restore_state():
        eng = p.engine
        eng.install_weights(state0[0], state0[3])
        eng.m.copy_(state0[1])
        eng.v.copy_(state0[2])
        # the tie-break noise (dpp.py:1055-1056) is drawn from the device generator's Philox stream: same draws again
        torch.cuda.default_generators[dev.index].set_offset(state0[4])
        since_restore[0] = 0

    def train(data, steps):
        if state0 is not None and since_restore[0] + steps > RESTORE_EVERY:
            restore_state()
        since_restore[0] += steps
        return p.adapt(None, data, steps=steps)

    last_lcd = [None]

    def step():
        out = train(batch, S)
        if not args.no_readback:
            consume(*out)
        if lcd_enc is not None:      # slam.py:223: after the pose has been read back, on the rank that holds the online frame
            last_lcd[0] = lcd_enc(lcd_image)
        return out

    def sync():
        if N > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    snapshot_state()
    # The timed region of the contract -- barrier + synchronize, EXACTLY `steps` steps, barrier + synchronize, MAX over ranks -- is
    # run `blocks` times back to back (default 1) and the MEDIAN block is reported; min / max are printed beside it.  `steps` x
    # `ms_per_step` describes one block.  (One 65 ms block moved by +-1 % from run to run: time enough steps, or look at the
    # spread of `repeated_blocks` under --full.)
    def timed_blocks(n_blocks):
        block_s, block_end_loss = [], []
        for _ in range(n_blocks):
            restore_state()          # every block times the same `steps` optimizer steps
            sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                outputs, losses = step()
            sync()
            dt = time.perf_counter() - t0
            if N > 1:
                t = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            block_s.append(dt)
            block_end_loss.append(float(losses['loss']))
        # the blocks are replicas of one another down to the last bit (same state, same minibatch, same noise draws, fixed
        # summation orders) -- reported, not asserted: `blocks_identical` false would mean the restore above is not ordered
        ordered = sorted(block_s)
        return ordered, len(set(block_end_loss)) == 1, outputs, losses

    ordered, blocks_identical, outputs, losses = timed_blocks(max(1, args.blocks))
    dt = ordered[len(ordered) // 2]
    ms = dt / args.steps * 1e3
    ms_min, ms_max = ordered[0] / args.steps * 1e3, ordered[-1] / args.steps * 1e3
    value = (args.steps / dt) * (B / FRAME_TRIPLETS)
    dumped = None
    if args.dump_outputs and rank == 0:
        # the last timed step's results, before any further step (--full's extra passes) can replace them
        dumped = dump_outputs(args.dump_outputs, outputs, losses, last_lcd[0])
    loss_last = float(losses['loss'])

    # ---- --full: the timed block 25 more times (spread of the headline's statistic, replica check of the restore) ---------
    repeated = None
    if args.full:
        r_ordered, r_identical, _, r_losses = timed_blocks(REPEAT_BLOCKS)
        repeated = {'blocks': REPEAT_BLOCKS, 'steps_per_block': args.steps,
                    'ms_per_step_median': round(r_ordered[len(r_ordered) // 2] / args.steps * 1e3, 3),
                    'ms_per_step_min': round(r_ordered[0] / args.steps * 1e3, 3),
                    'ms_per_step_max': round(r_ordered[-1] / args.steps * 1e3, 3),
                    'blocks_identical': r_identical and float(r_losses['loss']) == loss_last}

    # ---- SURVEY.md 8(d)'s end-to-end frame: pinned host batch -> adapt() (H2D inside) -> pose + losses on the host -------
    e2e = None
    if args.full and rank == 0 and N == 1 and not args.no_also:
        host = {k: v.pin_memory() for k, v in shard.items()}

        def frame():
            out = train(dict(host), S)     # a fresh dict per frame: adapt() moves its entries in place
            r = consume(*out)
            if lcd_enc is not None:
                lcd_enc(host['rgb', 1, 0][0])
            return r

        def timed(groups_n):
            frame()
            groups = []
            for _ in range(groups_n):
                sync()
                t0 = time.perf_counter()
                for _ in range(10):
                    frame()
                sync()
                groups.append((time.perf_counter() - t0) / 10 * 1e3)
            return sorted(groups)[len(groups) // 2]
        for _ in range(2):
            frame()
        ms_e2e = timed(3)
        # the same frame on the other boundary (opt-in host outputs <-> reference-default device outputs)
        prev = p.host_pose_output
        p.host_pose_output = not prev
        ms_other = timed(3)
        p.host_pose_output = prev
        # ... and with the training step on the caller's stream (rounds 1-3: the first .cpu() waits for backward + Adam),
        # on both boundaries (host outputs + caller's stream = round 3's opt-in fast path, for same-box comparison)
        p.engine.detached_training = False
        ms_attached = timed(3)
        p.host_pose_output = not prev
        ms_attached_other = timed(3)
        p.host_pose_output = prev
        p.engine.detached_training = True
        ms_att_dev, ms_att_host = (ms_attached_other, ms_attached) if prev else (ms_attached, ms_attached_other)
        # the box's own host -> device rate for this dict (the frame is partly PCIe time and the boxes of the pool differ)
        big = torch.empty(64 << 20, dtype=torch.uint8).pin_memory()
        dbig = torch.empty_like(big, device=dev)
        dbig.copy_(big, non_blocking=True)
        sync()
        t0 = time.perf_counter()
        for _ in range(5):
            dbig.copy_(big, non_blocking=True)
        sync()
        h2d_gbs = 5 * big.numel() / (time.perf_counter() - t0) / 1e9
        up = [k for k in host if isinstance(host[k], torch.Tensor)] if p.upload_all_inputs else [k for k in p.UPLOAD_FIRST + p.UPLOAD_REST if k in host]
        ms_dev, ms_host = (ms_other, ms_e2e) if prev else (ms_e2e, ms_other)
        e2e = {'ms_per_frame': round(ms_e2e, 3), 'frames_per_s': round(1e3 / ms_e2e, 2),
               'boundary': 'opt-in host outputs' if prev else 'reference default (device outputs)',
               'h2d_mbytes_per_frame': round(sum(host[k].numel() * host[k].element_size() for k in up) / 1e6, 2),
               'h2d_tensors': len(up), 'of_tensors_in_sample_dict': len(host),
               'ms_per_frame_with_device_outputs': round(ms_dev, 3),
               'ms_per_frame_with_host_outputs': round(ms_host, 3),
               'ms_per_frame_step_on_callers_stream': {'device_outputs': round(ms_att_dev, 3), 'host_outputs_r03_fast_path': round(ms_att_host, 3)},
               'h2d_gbytes_per_s_of_this_box': round(h2d_gbs, 1),
               'includes': 'H2D of the whole sample dict from pinned host memory (dpp.py:916-917; copy stream, network inputs '
                           'first, entries the path never reads last), adapt(), cam_T_cam[0] and the loss scalars on the host '
                           '(slam.py:181-188)' + (', loop-closure encoder forward (slam.py:223)' if lcd_enc is not None else '')}

    also = None
    if args.full and N == 1 and S == 1 and not args.no_also:
        # the reference's shipped configuration (config_adapt.yaml:53, adaptation_epochs: 5): five optimizer steps
        # per incoming frame; steps 2..5 keep the frozen encoders' features (engine.forward reuse_frozen).
        # Best of three groups of six calls (a reported extra, not the headline: one noisy group should not move it).
        for _ in range(2):
            train(batch, 5)
        groups = []
        for _ in range(3):
            sync()
            t0 = time.perf_counter()
            for _ in range(6):
                train(batch, 5)
            sync()
            groups.append((time.perf_counter() - t0) / 6 * 1e3)
        ms5 = min(groups)
        groups.sort()
        also = {'adapt_steps_per_frame': 5, 'ms_per_frame': round(ms5, 3), 'frames_per_s': round(1e3 / ms5, 2),
                'ms_per_optimizer_step': round(ms5 / 5, 3),
                'statistic': 'BEST of 3 groups of 6 calls (the headline `value` is the MEDIAN of its timed blocks)',
                'ms_per_frame_median_group': round(groups[1], 3), 'ms_per_frame_worst_group': round(groups[2], 3)}

    # ---- multi-GPU diagnosis (outside the timed region): every rank times its three bucket all-reduces on the tail stream ------
    exchange = None
    if args.full and N > 1:
        eng = p.engine
        reports = []
        for _ in range(5):
            eng.time_exchange = True
            eng.exchange_events, eng.exchange_main_done = [], None
            step()
            sync()
            eng.time_exchange = False
            r = eng.exchange_report()
            if r is not None:
                reports.append(r)
        mine = None
        if reports:
            reports.sort(key=lambda r: r['allreduce_ms'])
            mine = dict(reports[len(reports) // 2], rank=rank, steps_sampled=len(reports))      # the median step of this rank
        gathered = [None] * N
        dist.all_gather_object(gathered, mine)
        if rank == 0:
            exchange = {'per_rank': gathered,
                        'note': 'events around each bucket\'s all-reduce on the tail stream (median of 5 extra steps per rank); exposed_ms = '
                                'exchange still running after the backward\'s own last kernel; a world of ranks sharing ONE GPU (gloo '
                                'functional check) measures the host round trip of the collective, not xGMI'}
            for g in gathered:
                print(f'# rank {g and g["rank"]}: {g}', file=sys.stderr)

    # ---- roofline of the dominant kernel (instrumented extra step, outside the timed region) ------
    roof = None
    if args.full and rank != 0 and N > 1:
        step(); step()          # the two extra (collective) steps of rank 0's instrumented pass below
    if args.full and rank == 0:
        # serial launch order for this pass: with the pose / wgrad side streams active several kernels share
        # the GPU and a launch's own duration is not its kernel's efficiency
        p.engine.use_side_stream = False
        step()
        torch.cuda.synchronize()
        ops.profile_begin()
        step()
        torch.cuda.synchronize()
        agg = {}
        for kind, cfg, flops, secs, desc, nbytes in ops.profile_end():
            if args.dump_convs:
                us = secs * 1e6
                print(f'# conv cfg{cfg:3d} {desc:40s} {flops / 1e9:7.2f} GF {us:8.1f} us {flops / us / 1e6:6.1f} TF', file=sys.stderr)
            a = agg.setdefault((kind, cfg), [0.0, 0.0, 0, 0.0])
            a[0] += flops
            a[1] += secs
            a[2] += 1
            a[3] += nbytes
        p.engine.use_side_stream = True
        # kernel names as rocprofv3 prints them (template arguments TH, TW, BN, BK, MF, WGM, RUN, LDPAD, S, SK)
        patch = {10: '8, 16, 64, 16, 32, 2, false, 4, 1', 11: '8, 16, 32, 16, 32, 4, false, 4, 1', 12: '8, 16, 16, 16, 16, 4, false, 4, 1',
                 13: '4, 16, 64, 16, 32, 2, false, 4, 1', 14: '8, 16, 16, 32, 16, 4, false, 4, 1', 15: '16, 16, 16, 16, 16, 4, false, 4, 1',
                 16: '8, 16, 32, 16, 16, 4, false, 4, 1', 17: '4, 16, 16, 16, 16, 4, false, 4, 1', 18: '4, 16, 16, 16, 16, 4, true, 4, 1',
                 19: '8, 16, 16, 16, 16, 4, true, 4, 1', 20: '8, 16, 16, 16, 16, 4, false, 8, 1', 21: '4, 16, 16, 16, 16, 4, false, 8, 1',
                 22: '4, 16, 16, 16, 16, 4, true, 8, 1', 23: '4, 16, 16, 16, 16, 4, false, 8, 2', 24: '4, 16, 16, 32, 16, 4, true, 8, 1',
                 25: '4, 16, 16, 32, 16, 4, false, 8, 1', 26: '4, 8, 32, 16, 16, 2, false, 8, 1'}
        names = {0: 'conv_igemm_kernel<128, 64, 32, 32, 2>', 1: 'conv_igemm_kernel<64, 64, 32, 32, 2>',
                 2: 'conv_igemm_kernel<32, 32, 32, 16, 2>', 3: 'conv_igemm_kernel<64, 32, 32, 16, 2>',
                 4: 'conv_igemm_kernel<128, 16, 16, 16, 4>', 5: 'conv_igemm_kernel<64, 32, 16, 16, 2>',
                 6: 'conv_igemm_kernel<128, 16, 32, 16, 4>'}
        names.update({k: f'conv3x3_patch_kernel<{v}, false>' for k, v in patch.items()})
        # stream-K kernels (template arguments TH, TW, RUN, S, BN, NWM, NWN; the stride-2 layers use S = 2)
        names.update({30: 'conv3x3_sk_kernel<8, 16, false, 1, 64, 4, 2>', 31: 'conv3x3_sk_kernel<4, 16, false, 1, 64, 4, 2>',
                      32: 'conv3x3_sk_kernel<8, 16, true, 1, 64, 4, 2>', 33: 'conv3x3_sk_kernel<4, 16, true, 1, 64, 4, 2>',
                      34: 'conv3x3_sk_kernel<8, 16, false, 1, 32, 4, 1>', 35: 'conv3x3_sk_kernel<4, 16, false, 1, 32, 2, 2>',
                      36: 'conv3x3_sk_kernel<4, 16, true, 1, 32, 2, 2>', 37: 'conv3x3_sk_kernel<8, 16, true, 1, 32, 4, 1>'})
        # Winograd F(2x2,3x3) kernels (conv_wino.hip): 16 MFMA MACs per 2x2 output tile and input channel instead of 36
        names.update({40: 'conv3x3_wino8_kernel'})
        (kind, cfg), (fl, tt, cnt, nb) = max(agg.items(), key=lambda kv: kv[1][1])
        all_fl = sum(a[0] for a in agg.values())
        all_t = sum(a[1] for a in agg.values())
        # L2-miss bytes per launch of this kernel from the committed rocprofv3 PMC passes (profiles/pmc_traffic.json, written by
        # tools/measure_round.sh) -- only if those passes ran on THIS build of the kernels (same source id), else null
        traffic, traffic_note = None, None
        try:
            pmc = json.load(open(ROOT / 'profiles' / 'pmc_traffic.json'))
            if pmc.get('_build_id') == build_id:
                traffic = pmc[names[cfg]]['traffic_bytes_per_launch']
                traffic_note = ('2 x FETCH_SIZE + WRITE_SIZE (MI355X_MICROARCH.md); calibrated in round 6 (profiles/r06_pmc_calibration.txt): '
                                'FETCH_SIZE is exact, not half, for 64-B segment reads -- lower bound FETCH + WRITE = '
                                f"{pmc[names[cfg]].get('traffic_bytes_per_launch_lower_bound')} bytes")
            else:
                traffic_note = f"profiles/pmc_traffic.json was taken on build {pmc.get('_build_id')}, this is {build_id}"
        except Exception as e:
            traffic_note = f'no counter entry: {type(e).__name__}'
        roof = {'bound': 'mfma', 'achieved': round(fl / tt / 1e12, 2), 'peak': FP32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                'frac': round(fl / tt / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4), 'traffic': traffic, 'traffic_note': traffic_note,
                'algorithmic_bytes_per_launch_avg': round(nb / cnt),
                'kernel': names[cfg], 'launches_per_step': cnt,
                'avg_launch_us': round(tt / cnt * 1e6, 2), 'flops_per_launch_avg': fl / cnt,
                'all_conv_launches': {'achieved': round(all_fl / all_t / 1e12, 2), 'time_ms_per_step': round(all_t * 1e3, 3),
                                      'gflop_per_step': round(all_fl / 1e9, 2)}}
        if cfg == 40:
            # `achieved` counts the ALGORITHMIC flops of the convolution (2 * M * Cout * 9 * Cin), as for every other
            # kernel; this kernel EXECUTES 16/36 of them on the matrix pipe -- both fractions are stated
            roof['algorithm'] = 'Winograd F(2x2,3x3): 16/36 of the direct MFMA count'
            roof['pass_note'] = ('instrumented pass: serial launch order, every launch alone on the WHOLE chip (no cu_limit) -- there the depth '
                                 "encoder's layer1-3 at 5 images fall below the kernel's 8 units per workgroup and run on the direct kernel; in "
                                 'the TIMED step all 26 stride-1 3x3 encoder convolutions are Winograd launches, 13 on 5/8 of the chip (pose net) '
                                 'beside 13 on 3/8 (depth net): profiles/r06_timeline_one_step.txt')
            roof['executed_mfma_tflops'] = round(fl / tt / 1e12 * 16 / 36, 2)
            roof['executed_mfma_frac'] = round(fl / tt / 1e12 * 16 / 36 / FP32_MFMA_PEAK_TFLOPS, 4)
        # the dominant DIRECT kernel beside it (rounds 1-4's roofline row), and how the launches split
        direct = [(kv[0][1], kv[1]) for kv in agg.items() if kv[0][1] != 40]
        if direct and cfg == 40:
            dcfg, (dfl, dtt, dcnt, dnb) = max(direct, key=lambda kv: kv[1][1])
            roof['dominant_direct_kernel'] = {'kernel': names[dcfg], 'achieved': round(dfl / dtt / 1e12, 2),
                                              'frac': round(dfl / dtt / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4), 'launches_per_step': dcnt,
                                              'avg_launch_us': round(dtt / dcnt * 1e6, 2)}
        wfl = sum(a[0] for (k_, c_), a in agg.items() if c_ == 40)
        wt = sum(a[1] for (k_, c_), a in agg.items() if c_ == 40)
        roof['all_conv_launches']['winograd'] = {'launches': sum(a[2] for (k_, c_), a in agg.items() if c_ == 40),
                                                 'gflop_per_step': round(wfl / 1e9, 2), 'time_ms_per_step': round(wt * 1e3, 3)}
    cpu = None
    if args.full and rank == 0 and N == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(H, W, B)
    if rank == 0:
        line = {
            'metric': 'online-adapt frames/sec @192x640 (1 triplet + K replay)',
            'value': round(value, 3), 'unit': 'frames/s', 'n_gpus': N, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(ms, 3), 'ms_per_step_min': round(ms_min, 3), 'ms_per_step_max': round(ms_max, 3),
            'timed_blocks': len(ordered), 'blocks_identical': blocks_identical, 'state_restored_every_steps': RESTORE_EVERY, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': 'f32', 'data': 'synthetic (uniform-random images, lr 1e-12)' if args.random_images else 'synthetic',
            'config': {'workload': f'DepthPosePrediction.adapt(steps={S}), {H}x{W}, 1 online + K={K} replay triplets '
                                   f'(global batch {B}); ResNet-18 depth+pose nets, closed-form random-init weights; '
                                   f'a frame = {FRAME_TRIPLETS} triplets (value = steps/s * B/{FRAME_TRIPLETS})',
                       'global_batch': B, 'replay_k': K, 'height': H, 'width': W, 'adapt_steps_per_frame': S,
                       'parallelism': f'dp{N}' if N > 1 else 'single', 'shards': counts,
                       # by-sample sharding cannot beat the largest shard: the speed-up over one GPU is capped at B / max(shard)
                       'shard_imbalance_speedup_cap': round(B / max(counts), 2),
                       'timed_region': 'minibatch resident in HBM -> adapt() -> ' + ('nothing read back' if args.no_readback else
                                       'cam_T_cam[0] and every loss scalar on the host (slam.py:181-188)'),
                       'boundary': 'opt-in host-output path (host_pose_output=True): pose + losses handed out as host tensors '
                                   'staged behind the forward' if args.host_outputs else
                                   'reference default: outputs and losses are device tensors; the training step runs detached on '
                                   'the engine stream (the read-back waits for the forward + 3 launches)',
                       'lcd_encoder_in_frame': bool(args.lcd),
                       'loss': loss_last},
            'build_id': build_id,
            'roofline': roof, 'cpu_baseline': cpu, 'full': bool(args.full),
        }
        if repeated is not None:
            line['repeated_blocks'] = repeated
        if dumped is not None:
            line['dumped_outputs'] = dumped
        if exchange is not None:
            line['gradient_exchange'] = exchange
        if also is not None:
            line['also'] = also
        if e2e is not None:
            line.setdefault('also', {})['end_to_end'] = e2e
            # SURVEY.md 8(d) defines the metric WITH the host -> device upload of the sample dict: stated at top level beside `value`
            # (which, by the bench contract, starts with the minibatch resident in HBM)
            line['value_end_to_end'] = e2e['frames_per_s']
            line['ms_per_frame_end_to_end'] = e2e['ms_per_frame']
        print(json.dumps(line), flush=True)
    if N > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
