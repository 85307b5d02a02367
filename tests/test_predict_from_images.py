"""DepthPosePrediction.predict_from_images (dpp.py:556-626): two frames -> depth of both, the relative pose and, on request,
the photometric loss of the pair.  Golden vectors of the real reference class (tests/golden/make_pair_golden.py), consistency
with predict_from_image / predict_pose, shapes and errors, the velocity term, and a call behind a detached training step."""
import numpy as np
import pytest
import torch

from clslam_hip import synth
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend
from helpers import load_golden, rel_err
from predictor_util import make_predictor

H, W = 64, 128
TOL = 1e-4          # the project's parity bound for goldens (tests/test_predictor.py)
KEYS = ['reprojection_loss/scale_0', 'smooth_loss/scale_0', 'reg_loss/scale_0', 'depth_loss/scale_0', 'depth_loss', 'loss']


def _pair(batch, n=None):
    kw = dict(camera_matrix=batch['camera_matrix', 0][:n], inv_camera_matrix=batch['inv_camera_matrix', 0][:n],
              relative_distance=batch['relative_distance', 0][:n])
    return batch['rgb', -1, 0][:n].clone(), batch['rgb', 0, 0][:n].clone(), kw


def test_the_method_exists():
    from depth_pose_prediction import DepthPosePrediction
    assert hasattr(DepthPosePrediction, 'predict_from_images')


@pytest.mark.parametrize('backend', BACKENDS)
def test_matches_reference_golden(backend):
    """depth_0, depth_1, the transformation and every loss key of the reference's call (N = 1, velocity_loss_scaling = 0,
    injected tie-break noise) within 1e-4 relative; the dictionary has the reference's keys in its order, as 0-d numpy."""
    use_backend(backend)
    g = load_golden('pair_b1')
    _, _, sb, sn = (int(v) for v in g['params'])
    p = make_predictor(H, W, 1, velocity_loss_scaling=0)
    batch = synth.make_batch(1, H, W, seed=sb)
    p.set_tie_break_noise(synth.make_noise(1, H, W, seed=sn))
    i0, i1, kw = _pair(batch)
    d0, d1, T, losses = p.predict_from_images(i0, i1, return_loss=True, **kw)
    assert d0.shape == (H, W) and d1.shape == (H, W) and T.shape == (4, 4) and d0.dtype == np.float32
    assert rel_err(d0, g['depth_0']) < TOL and rel_err(d1, g['depth_1']) < TOL and rel_err(T, g['transformation']) < TOL
    assert list(losses.keys()) == KEYS
    for k in KEYS:
        assert isinstance(losses[k], np.ndarray) and losses[k].shape == ()
        assert abs(float(losses[k]) - float(g['loss/' + k])) <= TOL * abs(float(g['loss/' + k])), (k, float(losses[k]), float(g['loss/' + k]))
    assert float(losses['depth_loss']) == float(losses['depth_loss/scale_0']) / 4
    assert p.frame_ids == (0, -1, 1)
    # without the loss: three values, the same numbers
    e0, e1, T2 = p.predict_from_images(i0, i1)
    assert np.array_equal(e0, d0) and np.array_equal(e1, d1) and np.array_equal(T2, T)


@pytest.mark.parametrize('backend', BACKENDS)
def test_consistent_with_the_single_frame_calls(backend):
    """The transformation is predict_pose's bit for bit (N = 1: the same kernels on the same share of the chip).  The depths come
    from ONE depth-network pass over both frames, predict_from_image's from a pass over one: another batch size, so the
    persistent convolution kernels may split their sums differently -- they are held to the 1e-4 relative bound the
    stand-alone encoder outputs are held to (tests/test_predictor.py), not to the bit.  3-D inputs, device outputs."""
    dev = use_backend(backend)
    p = make_predictor(H, W, 1)
    batch = synth.make_batch(1, H, W, seed=9)
    i0, i1, _ = _pair(batch)
    d0, d1, T = p.predict_from_images(i0[0], i1[0])                      # (3,H,W) inputs gain a batch dimension
    assert d0.shape == (H, W) and T.shape == (4, 4)
    Tp, _ = p.predict_pose(i0, i1)
    assert np.array_equal(T, Tp)
    for d, img in ((d0, i0), (d1, i1)):
        assert rel_err(d, p.predict_from_image(img)) < TOL
    t0, t1, Tt = p.predict_from_images(i0, i1, as_numpy=False)
    assert all(isinstance(v, torch.Tensor) and v.device.type == dev.type for v in (t0, t1, Tt))
    assert t0.shape == (1, 1, H, W) and t1.shape == (1, 1, H, W) and Tt.shape == (1, 4, 4)
    assert np.array_equal(t0[0, 0].cpu().numpy(), d0) and np.array_equal(Tt[0].cpu().numpy(), T)
    assert p.frame_ids == (0, -1, 1)
    p.is_trained = False
    with pytest.warns(RuntimeWarning, match='not been trained'):
        p.predict_from_images(i0, i1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_batch_weights_and_errors(backend):
    """N = batch_size: every pair weighs 1 / batch_size, so the reprojection loss is the mean of the per-pair values (each from
    an N = 1 call, where the single pair sees the sum of the weights = 1); depths of another batch size: 1e-4 relative, so
    the losses too.  N outside {1, batch_size} raises the class's broadcasting error; missing calibration a ValueError;
    another resolution a ClslamError."""
    use_backend(backend)
    B = 2
    p = make_predictor(H, W, B, velocity_loss_scaling=0)
    batch = synth.make_batch(3, H, W, seed=4)
    noise = synth.make_noise(3, H, W, seed=5)[0][:, :1].contiguous()
    i0, i1, kw = _pair(batch, B)
    p.set_tie_break_noise(noise[:B])
    d0, d1, T, losses = p.predict_from_images(i0, i1, return_loss=True, **kw)
    assert d0.shape == (B, H, W) and T.shape == (B, 4, 4)
    single = []
    for b in range(B):
        p.set_tie_break_noise({0: noise[b:b + 1]})
        kb = {k: v[b:b + 1] for k, v in kw.items()}
        e0, _, Tb, lb = p.predict_from_images(i0[b:b + 1], i1[b:b + 1], return_loss=True, **kb)
        assert rel_err(e0, d0[b]) < TOL and rel_err(Tb, T[b]) < TOL
        single.append(float(lb['reprojection_loss/scale_0']))
    want = sum(single) / B
    assert abs(float(losses['reprojection_loss/scale_0']) - want) <= TOL * want
    j0, j1, kw3 = _pair(batch, 3)
    p.set_tie_break_noise(None)
    with pytest.raises(RuntimeError, match='must match the size of tensor'):
        p.predict_from_images(j0, j1, return_loss=True, **kw3)
    assert p.predict_from_images(j0, j1)[0].shape == (3, H, W)          # without the loss any N goes
    with pytest.raises(ValueError, match='camera_matrix'):
        p.predict_from_images(i0, i1, return_loss=True)
    with pytest.raises(ClslamError, match='must be'):
        p.predict_from_images(i0[..., :64], i1[..., :64])
    assert p.frame_ids == (0, -1, 1)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('quirks', [True, False])
def test_velocity_term_and_smoothness_modes(backend, quirks):
    """velocity_loss_scaling > 0 (the reference raises KeyError there): 'velocity_loss' = scaling * | |t| - |distance| | of the
    returned transformation's translation, 'loss' = 'depth_loss' + 'velocity_loss'; the tie-break noise comes from the engine's
    draw counter (no tensor set): two calls differ from each other by less than the noise can move a mean.  Both smoothness
    modes: the smooth term against the restatement on the returned depth's disparity."""
    use_backend(backend)
    p = make_predictor(H, W, 1, reference_quirks=quirks)
    batch = synth.make_batch(1, H, W, seed=6)
    i0, i1, kw = _pair(batch)
    d0, d1, T, losses = p.predict_from_images(i0, i1, return_loss=True, **kw)
    assert list(losses.keys()) == KEYS[:5] + ['velocity_loss', 'loss']
    t = np.linalg.norm(T[:3, 3].astype(np.float64))
    want = 0.05 * abs(t - abs(float(kw['relative_distance'][0])))
    assert want > 0 and abs(float(losses['velocity_loss']) - want) <= 1e-6 * want
    assert abs(float(losses['loss']) - (float(losses['depth_loss']) + float(losses['velocity_loss']))) <= 2e-7 * float(losses['loss'])
    assert float(losses['depth_loss']) == float(losses['depth_loss/scale_0']) / 4
    import pair_loss_reference as PR
    disp = torch.from_numpy(0.1 / d1.astype(np.float64))[None]          # min_depth / depth (max_depth None)
    z = torch.zeros(1, 1)
    ref = PR.finalize(z, disp, i1, torch.zeros(1, 12), None, torch.ones(1), torch.ones(1), not quirks, H, W, 1e-3, 0.0)
    assert abs(float(losses['smooth_loss/scale_0']) - float(ref[1])) <= 1e-4 * float(ref[1])
    with pytest.raises(ValueError, match='relative_distance'):
        p.predict_from_images(i0, i1, return_loss=True, camera_matrix=kw['camera_matrix'], inv_camera_matrix=kw['inv_camera_matrix'])
    again = p.predict_from_images(i0, i1, return_loss=True, **kw)[3]
    assert abs(float(again['reprojection_loss/scale_0']) - float(losses['reprojection_loss/scale_0'])) <= 1e-4


@pytest.mark.gpu
def test_behind_a_detached_training_step():
    """A call right behind a training adapt() whose backward + optimizer step are still in flight on the engine's stream
    returns the values of the POST-step weights: the same bits as the call repeated after the device has drained, and not
    those of the call before the step."""
    use_backend('hip')
    B = 2
    p = make_predictor(H, W, B)
    eng = p.engine
    assert eng.detached_ok()
    batch = synth.make_batch(B, H, W, seed=5)
    i0, i1, _ = _pair(batch, 1)
    i0, i1 = i0.cuda(), i1.cuda()
    before = p.predict_from_images(i0, i1, as_numpy=False)
    p.adapt({k: v.clone() for k, v in batch.items()}, {k: v.clone() for k, v in batch.items()})
    assert eng._train_done is not None                      # the step went out detached
    during = p.predict_from_images(i0, i1, as_numpy=False)
    torch.cuda.synchronize()
    after = p.predict_from_images(i0, i1, as_numpy=False)
    for a, b in zip(during, after):
        assert torch.equal(a, b)
    assert not torch.equal(before[1], after[1]) and not torch.equal(before[2], after[2])
