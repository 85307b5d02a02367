"""The public face of the depth-error metrics: clslam_hip.depth_eval.calc_depth_error / depth_error_async,
DepthPosePrediction.compute_depth_error and predict_from_image (slam/utils.py:389-442, dpp.py:344-468, 538-554).

Bounds: those of tests/test_depth_metrics.py (depth_eval_reference.bounds), per sample, carried to what the evaluator returns:
an average over samples may differ by the average of the samples' bounds; a1..a3 by the average share of pixels in the 1e-5
band around the threshold (plus the rounding of a count / n to fp32); the median of the ratios by the largest bound of a ratio.
"""
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import depth_eval_reference as R
from clslam_hip import depth_eval, synth
from emu_util import BACKENDS, use_backend
from predictor_util import make_config, make_predictor

H, W, HG, WG = 64, 128, 70, 150
U = 2.0 ** -24


def _scene(seed=3, h=24, w=80, hg=47, wg=155):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(3.0, 60.0, (h, w)).astype(np.float32)
    base = R.resample(pred.astype(np.float64), hg, wg, np.float64)
    gt = (base * np.exp(rng.uniform(np.log(0.5), np.log(2.2), (hg, wg)))).astype(np.float32)
    gt[rng.random((hg, wg)) < 0.4] = 0.0
    return pred, gt


@pytest.mark.parametrize('backend', BACKENDS)
def test_calc_depth_error_accepts_numpy_host_and_device_inputs(backend):
    dev = use_backend(backend)
    pred, gt = _scene()
    a = depth_eval.calc_depth_error(pred, gt, min_depth=0.1, max_depth=80.0)
    b = depth_eval.calc_depth_error(torch.from_numpy(pred), torch.from_numpy(gt), min_depth=0.1, max_depth=80.0)
    c = depth_eval.calc_depth_error(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), min_depth=0.1, max_depth=80.0)
    assert list(a) == ['abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3', 'rmse', 'rmse_log']      # utils.py:431-440
    assert all(type(v) is float for v in a.values())
    assert a == b == c
    r64, r32 = R.evaluate(pred, gt, 0.1, 80.0), R.evaluate(pred, gt, 0.1, 80.0, dtype=np.float32)
    tol = R.bounds(r64, r32)
    for k in R.SUMS:
        assert abs(a[k] - float(r64[k])) <= tol[k], k
    for k in ('a1', 'a2', 'a3'):
        assert abs(a[k] - r64[k]) <= tol['band'][k].sum() / r64['n'] + U
    # the driver's shapes (slam.py:264-270 squeezes (1,H,W) planes); median_scaling=False is passed through
    d = depth_eval.calc_depth_error(pred[None], gt[None, None], median_scaling=False, min_depth=0.1, max_depth=80.0)
    assert abs(d['abs_diff'] - float(R.evaluate(pred, gt, 0.1, 80.0, median_scaling=False)['abs_diff'])) < 1e-4
    with pytest.raises(Exception, match='min_depth'):
        depth_eval.calc_depth_error(pred, gt)
    with pytest.raises(Exception, match='one image'):
        depth_eval.calc_depth_error(np.stack([pred, pred]), np.stack([gt, gt]), min_depth=0.1)
    h = depth_eval.depth_error_async(np.stack([pred, pred]), np.stack([gt, gt]), min_depth=0.1, max_depth=80.0)
    assert h.result() == [a, a] and h.done() and h.rows().shape == (2, 10) and h.rows()[0, 9] == r64['n']


def _samples(p, dev):
    """three single-image samples; the ground truth follows the predictor's own depth (min_depth / disp, resampled), scaled and
    perturbed per pixel, dense at 70x150"""
    out = []
    for i in range(3):
        batch = synth.make_batch(1, H, W, seed=40 + i)
        with torch.no_grad():
            disp = p.predict({k: v.clone() for k, v in batch.items()})['disp', 0][0, 0].cpu().numpy()
        rng = np.random.default_rng(i)
        depth = np.float32(p.min_depth) / disp.astype(np.float64)
        gt = ((7 + 3 * i) * R.resample(depth, HG, WG, np.float64) * np.exp(rng.uniform(np.log(0.5), np.log(2.2), (HG, WG))))
        sample = {('rgb_aug', 0, 0): batch['rgb_aug', 0, 0].clone(), ('depth', 0, -1): torch.from_numpy(gt.astype(np.float32))[None, None]}
        out.append((sample, disp))
    return out


@pytest.mark.parametrize('backend', BACKENDS)
def test_compute_depth_error_with_a_data_loader(backend, capsys):
    dev = use_backend(backend)
    p = make_predictor(H, W, 1)
    samples = _samples(p, dev)
    r64 = [R.evaluate(d, s['depth', 0, -1][0, 0].numpy(), p.min_depth, p.max_depth, from_disp=True) for s, d in samples]
    r32 = [R.evaluate(d, s['depth', 0, -1][0, 0].numpy(), p.min_depth, p.max_depth, from_disp=True, dtype=np.float32)
           for s, d in samples]
    tols = [R.bounds(a, b) for a, b in zip(r64, r32)]
    assert all(r['n'] == HG * WG for r in r64)
    capsys.readouterr()
    got = p.compute_depth_error(data_loader=[s for s, _ in samples])
    printed = capsys.readouterr().out.splitlines()
    assert list(got) == list(R.KEYS) + ['med_scaling'] and all(type(v) is float for v in got.values())
    for k in R.SUMS:
        ref, tol = np.mean([float(r[k]) for r in r64]), np.mean([t[k] for t in tols])
        print(f'[compute_depth_error {backend}] {k:<9} err {abs(got[k] - ref):.3e} bound {tol:.3e}')
        assert abs(got[k] - ref) <= tol, k
    for k in ('a1', 'a2', 'a3'):
        ref = np.mean([r[k] for r in r64])
        assert abs(got[k] - ref) <= np.mean([t['band'][k].sum() / r['n'] for t, r in zip(tols, r64)]) + U, k
    med64 = float(np.median([float(r['ratio']) for r in r64]))
    assert abs(got['med_scaling'] - med64) <= max(t['ratio'] for t in tols)
    # dpp.py:457-466: the print format
    assert printed[:8] == [f'{k:<8}: {got[k]:>6.3f}' for k in R.KEYS]
    assert printed[8].startswith(f'Scaling ratios | med: {got["med_scaling"]:.3f} | std: ') and len(printed) == 9
    # without median scaling there is no med_scaling key and nothing more is printed with print_results=False
    capsys.readouterr()
    quiet = p.compute_depth_error(median_scaling=False, print_results=False, data_loader=[samples[0][0]])
    assert list(quiet) == list(R.KEYS) and capsys.readouterr().out == ''
    ref = float(R.evaluate(samples[0][1], samples[0][0]['depth', 0, -1][0, 0].numpy(), p.min_depth, p.max_depth,
                           median_scaling=False, from_disp=True)['abs_rel'])
    assert abs(quiet['abs_rel'] - ref) <= 1e-5 * ref
    # a sample without a valid pixel is not dropped: the averages are NaN
    empty = dict(samples[0][0])
    empty['depth', 0, -1] = torch.zeros(1, 1, HG, WG)
    nan = p.compute_depth_error(print_results=False, data_loader=[samples[1][0], empty])
    assert all(np.isnan(nan[k]) for k in R.KEYS)


@pytest.mark.parametrize('backend', BACKENDS)
def test_compute_depth_error_unsupported_dataset(backend):
    use_backend(backend)
    from depth_pose_prediction import DepthPosePrediction
    ds = SimpleNamespace(dataset='RobotCar', config_file=Path('x.yaml'), dataset_path=None, scales=(0, 1, 2, 3), height=H, width=W,
                         frame_ids=(0, -1, 1))
    p = DepthPosePrediction(ds, make_config(1, train_set='a', val_set='b'))
    p.is_trained = True
    with pytest.warns(RuntimeWarning, match='Unsupported dataset: RobotCar'):
        assert p.compute_depth_error() == {}


@pytest.mark.parametrize('backend', BACKENDS)
def test_predict_from_image(backend):
    dev = use_backend(backend)
    p = make_predictor(H, W, 1, max_depth=80.0)
    batch = synth.make_batch(1, H, W, seed=9)
    image = batch['rgb_aug', 0, 0].clone()
    with torch.no_grad():
        ref = p.predict({k: v.clone() for k, v in batch.items()})
    a = p.predict_from_image(image[0])                             # (3,H,W), numpy (dpp.py:551-553: squeezed)
    b = p.predict_from_image(image, as_numpy=False)                # (1,3,H,W), tensor on the device, unsqueezed
    assert isinstance(a, np.ndarray) and a.shape == (H, W) and a.dtype == np.float32
    assert isinstance(b, torch.Tensor) and b.shape == (1, 1, H, W) and b.device.type == dev.type
    assert np.array_equal(a, b[0, 0].cpu().numpy())
    from depth_pose_prediction.utils import disp_to_depth
    # the same kernels on the same weights: predict()'s disparity bitwise, through the reference's disp_to_depth
    assert np.array_equal(a, disp_to_depth(ref['disp', 0], p.min_depth, p.max_depth)[0, 0].cpu().numpy())
    # predict()'s own depth plane comes out of the warp kernel's arithmetic: the same number up to fp32 rounding of
    # 1 / (min_disp + (max_disp - min_disp) * disp) (three operations)
    assert np.allclose(a, ref['depth', 0][0, 0].cpu().numpy(), rtol=8 * U, atol=0)
    p.is_trained = False
    with pytest.warns(RuntimeWarning, match='not been trained'):
        p.predict_from_image(image)


@pytest.mark.gpu
def test_depth_error_async_during_a_training_adapt():
    """The metric of the frame is enqueued on the caller's stream right behind a detached training adapt(): its event
    completes without anything having waited for the step (engine.wait_training is not called), and the values are those of the
    synchronous call on the same planes."""
    dev = use_backend('hip')
    B = 2
    p = make_predictor(H, W, B, max_depth=80.0)
    eng = p.engine
    assert eng.detached_ok()
    batch = synth.make_batch(B, H, W, seed=5)
    rng = np.random.default_rng(0)
    gt = torch.from_numpy(rng.uniform(0.0, 90.0, (B, HG, WG)).astype(np.float32)).to(dev)
    p.adapt({k: v.clone() for k, v in batch.items()}, {k: v.clone() for k, v in batch.items()})      # warm-up: allocations, packing
    torch.cuda.synchronize()
    calls = []
    orig = eng.wait_training
    eng.wait_training = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        outputs, _ = p.adapt({k: v.clone() for k, v in batch.items()}, {k: v.clone() for k, v in batch.items()})
        step_done = eng._train_done
        assert step_done is not None                                   # the step went out detached, on the engine's stream
        before = len(calls)
        depth = outputs['depth', 0]
        handle = depth_eval.depth_error_async(depth, gt, min_depth=p.min_depth, max_depth=p.max_depth)
        assert handle.stream.cuda_stream == torch.cuda.current_stream().cuda_stream != eng.main_stream.cuda_stream
        handle.event.synchronize()                                     # ordered behind the output planes only
        assert handle.event.query() and handle.done()
        rows = handle.rows().copy()
        assert len(calls) == before                                    # nothing in between waited for backward + Adam
    finally:
        eng.wait_training = orig
    torch.cuda.synchronize()
    assert step_done.query()
    sync = [depth_eval.calc_depth_error(depth[i], gt[i], min_depth=p.min_depth, max_depth=p.max_depth) for i in range(B)]
    assert handle.result() == sync
    assert [depth_eval.as_dict(r) for r in rows] == sync
    r64 = R.evaluate(depth[0, 0].cpu().numpy(), gt[0].cpu().numpy(), p.min_depth, p.max_depth)
    assert rows[0, 9] == r64['n'] and abs(sync[0]['abs_rel'] - float(r64['abs_rel'])) <= 1e-5 * float(r64['abs_rel'])
