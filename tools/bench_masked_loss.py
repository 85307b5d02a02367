#!/usr/bin/env python
"""Step time of adapt() with mask_dynamic=True beside mask_dynamic=False: 192 x 640, one online + K replay triplets, the same
synthetic minibatch and weights, masks with 30 % dynamic pixels (synth.make_masks).  Device-resident inputs, in-kernel
tie-break noise, `blocks` timed blocks of `steps` steps each per configuration, interleaved; prints the median and the
spread of the blocks and one JSON line.  The loss stage of the unmasked step is hidden under the side streams' work
(DESIGN.md); the comparison says whether the masked one (a locate pass, a second finalize, a gradient kernel more) still is.

    python tools/bench_masked_loss.py [--replay 4] [--steps 50] [--blocks 5] [--out profiles/masked_loss.txt]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / 'cl-slam_amd', ROOT / 'tests'):
    sys.path.insert(0, str(p))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--replay', type=int, default=4)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--height', type=int, default=192)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from clslam_hip import synth
    from predictor_util import make_predictor
    assert torch.cuda.is_available(), 'needs an MI355X'
    B, H, W = 1 + a.replay, a.height, a.width
    batch = {k: v.cuda() for k, v in synth.make_batch(B, H, W, seed=3).items()}
    batch.update({k: v.cuda() for k, v in synth.make_masks(B, H, W, seed=5, dynamic=0.3).items()})
    preds = {name: make_predictor(H, W, B, mask_dynamic=flag) for name, flag in (('unmasked', False), ('masked', True))}

    # the synthetic network is untrained and degenerates when it is trained on one minibatch for dozens of steps (bench.py says
    # why): the trainable state goes back to its post-warmup value every RESTORE_EVERY steps, inside the timed region
    RESTORE_EVERY = 20
    state = {}

    def restore(name, p):
        w, m, v, count = state[name]
        p.engine.install_weights(w, count)
        p.engine.m.copy_(m)
        p.engine.v.copy_(v)

    def block(name, p, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            if name in state and i % RESTORE_EVERY == 0:
                restore(name, p)
            _, losses = p.adapt(None, dict(batch), steps=1)
            float(losses['loss'])                   # the read-back the driver does every frame
        p.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for name, p in preds.items():
        block(name, p, a.warmup)
        p.synchronize()
        state[name] = (p.engine.w.clone(), p.engine.m.clone(), p.engine.v.clone(), p.engine.adam_step_count)
    times = {name: [] for name in preds}
    for _ in range(a.blocks):
        for name, p in preds.items():
            times[name].append(block(name, p, a.steps))
    res = {'height': H, 'width': W, 'batch': B, 'steps': a.steps, 'blocks': a.blocks}
    lines = [f'adapt() step time, {H} x {W}, 1 + {a.replay} triplets, {a.blocks} blocks of {a.steps} steps (ms per step)']
    for name, ts in times.items():
        res[name + '_ms'] = statistics.median(ts)
        res[name + '_blocks_ms'] = [round(t, 4) for t in ts]
        lines.append(f'  {name:<9} median {statistics.median(ts):.4f}   min {min(ts):.4f}   max {max(ts):.4f}')
    res['masked_minus_unmasked_ms'] = res['masked_ms'] - res['unmasked_ms']
    spread = max(max(ts) - min(ts) for ts in times.values())
    lines.append(f'  masked - unmasked = {res["masked_minus_unmasked_ms"]:+.4f} ms (spread of the blocks: {spread:.4f} ms)')
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + '\n' + json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
