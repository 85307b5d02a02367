#!/usr/bin/env python
"""Generate tests/golden/pair_b1.npz: predict_from_images(return_loss=True) of the REAL reference class (dpp.py:556-626) on
clslam_hip.synth weights and inputs at 64x128, N = 1, velocity_loss_scaling = 0 (with a positive scaling the reference raises
KeyError: 'index'), the tie-break noise injected through the torch.randn patch of make_golden.py.  Outputs only.

    python tests/golden/make_pair_golden.py

Runs where the reference checkout is present (see make_golden.py, whose stubs and builder are imported)."""
import shutil
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as MG  # noqa: E402

H, W, SEED_BATCH, SEED_NOISE = 64, 128, 7, 21


def main() -> None:
    sys.path.insert(0, str(MG.ROOT / 'cl-slam_amd'))
    from clslam_hip import synth
    MG.install_stubs()
    torch.set_num_threads(8)
    p = MG.build_reference(H, W, 1, HERE / '_tmp_log')
    p.velocity_loss_scaling = 0
    for name, m in p.models.items():
        m.load_state_dict(synth.fill_state_dict(m.state_dict(), 0, name))
    batch = synth.make_batch(1, H, W, seed=SEED_BATCH)
    noise = synth.make_noise(1, H, W, seed=SEED_NOISE)[0][:, :1].contiguous()          # (1,1,H,W), already x 1e-5
    orig = torch.randn

    def injected(*a, **k):
        shape = a[0] if len(a) == 1 and not isinstance(a[0], int) else a
        assert tuple(shape) == tuple(noise.shape), (shape, noise.shape)
        return noise / 1e-5          # the reference multiplies by 1e-5

    torch.randn = injected
    try:
        d0, d1, T, losses = p.predict_from_images(batch['rgb', -1, 0], batch['rgb', 0, 0], as_numpy=True, return_loss=True,
                                                  camera_matrix=batch['camera_matrix', 0], inv_camera_matrix=batch['inv_camera_matrix', 0],
                                                  relative_distance=batch['relative_distance', 0])
    finally:
        torch.randn = orig
    assert p.frame_ids == (0, -1, 1)
    rec = {'params': np.array([H, W, SEED_BATCH, SEED_NOISE], np.int64), 'depth_0': d0, 'depth_1': d1, 'transformation': T}
    for k, v in losses.items():
        rec['loss/' + k] = np.asarray(v)
    np.savez_compressed(HERE / 'pair_b1.npz', **rec)
    print('pair_b1', {k: float(v) for k, v in losses.items()}, d0.shape, T.shape)
    shutil.rmtree(HERE / '_tmp_log', ignore_errors=True)


if __name__ == '__main__':
    main()
