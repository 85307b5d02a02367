"""The public face of the trajectory and pose-error metrics: clslam_hip.traj_eval (calc_error and the reference's other names,
trajectory_metrics, pose_pair_error_async), DepthPosePrediction.compute_pose_error and validate (slam/utils.py:129-383,
slam.py:257-259, dpp.py:321-342, 470-525).

Bounds: those of tests/test_traj_metrics.py -- an array of errors may deviate from the longdouble truth by 4 x the float64
twin's largest deviation; what the reference prints with four decimals is compared as text against tests/golden/traj_eval.npz.
"""
import copy
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import traj_eval_reference as R
from clslam_hip import synth, traj_eval
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend
from predictor_util import make_config, make_predictor

H, W = 64, 128
GOLDEN = np.load(Path(__file__).resolve().parent / 'golden' / 'traj_eval.npz')


def _lists():
    pred, gt = R.make_fixture(1000, 0)
    return [p.copy() for p in pred], [g.copy() for g in gt]


@pytest.mark.parametrize('backend', BACKENDS)
def test_calc_error_returns_the_reference_text(backend):
    use_backend(backend)
    pred, gt = _lists()
    assert traj_eval.calc_error(pred, gt) == str(GOLDEN['log_plain'])
    assert traj_eval.calc_error(pred, gt, optimize_scale=True) == str(GOLDEN['log_scaled'])
    assert 'Scaling: ' in str(GOLDEN['log_scaled']) and '\nScaling' in str(GOLDEN['log_scaled'])
    assert str(GOLDEN['log_scaled']).startswith('-' * 10 + ' MEDIAN\nScaling: ' + repr(float(GOLDEN['scaling'])) + '-' * 10 + '\n')


@pytest.mark.parametrize('backend', BACKENDS)
def test_inputs_of_every_kind_agree(backend):
    dev = use_backend(backend)
    pred, gt = R.make_fixture(1000, 0)
    a = traj_eval.trajectory_metrics([p for p in pred], [g for g in gt])                      # lists of 4x4
    b = traj_eval.trajectory_metrics(pred, gt)                                                # (N,4,4) arrays
    c = traj_eval.trajectory_metrics(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()))
    d = traj_eval.trajectory_metrics(torch.from_numpy(pred.copy()).to(dev), torch.from_numpy(gt.copy()).to(dev))
    assert list(a) == ['t_err', 'r_err', 'n_segments', 'ate', 'rpe_trans', 'rpe_rot', 'scaling', 'path_length']
    assert type(a['n_segments']) is int and a['n_segments'] == 440
    assert all(type(v) is float for k, v in a.items() if k != 'n_segments')
    assert a == b == c == d
    h = traj_eval.trajectory_metrics_async(pred, gt, optimize_scale=True)
    assert h.result()['scaling'] == a['scaling'] and h.done() and h.device_result.shape == (8,)
    assert h.device_result.device.type == dev.type and h.result()['t_err'] != a['t_err']
    # fp32 is accepted (converted to fp64): the metrics of the rounded poses
    p32, g32 = pred.astype(np.float32), gt.astype(np.float32)
    e = traj_eval.trajectory_metrics(torch.from_numpy(p32).to(dev), g32)
    assert e == traj_eval.trajectory_metrics(p32.astype(np.float64), g32.astype(np.float64))
    assert abs(e['ate'] - a['ate']) < 1e-3 and e['n_segments'] in (439, 440, 441)
    # what the reference would answer with an IndexError or a silent truncation
    with pytest.raises(ClslamError, match='1000 poses.*999'):
        traj_eval.calc_error(list(pred), list(gt[:999]))
    with pytest.raises(ClslamError, match='4x4'):
        traj_eval.calc_error(list(pred[:3]) + [np.eye(3)], list(gt[:4]))
    with pytest.raises(ClslamError):
        traj_eval.trajectory_metrics(pred[:, :3], gt)
    with pytest.raises(ClslamError):
        traj_eval.pose_pair_error_async(pred[:4], gt[:3])


@pytest.mark.parametrize('backend', BACKENDS)
def test_reference_names(backend):
    use_backend(backend)
    pred, gt = _lists()
    twin, truth = R.evaluate(pred, gt), R.evaluate(pred, gt, hp=True)
    # calc_sequence_errors: the rows that have a last frame, in the reference's order and layout
    rows = traj_eval.calc_sequence_errors(pred, gt)
    ref = GOLDEN['sequence_errors']
    assert isinstance(rows, list) and len(rows) == len(ref) == 440 and all(isinstance(r, list) and len(r) == 5 for r in rows)
    assert all(type(r[0]) is int and type(r[3]) is int and type(r[1]) is float for r in rows)
    got = np.asarray(rows, dtype=np.float64)
    assert np.array_equal(got[:, [0, 3, 4]], ref[:, [0, 3, 4]])                              # first_frame, length, speed: exactly
    ok = twin['segments'][:, 5] >= 0
    for col in (1, 2):
        e_twin = R.element_bound(ref[:, col], truth['segments'][ok, col])
        assert 0 < e_twin and R.element_bound(got[:, col], truth['segments'][ok, col]) <= 4 * e_twin
    # the two host-only averages
    seg = traj_eval.compute_segment_error(rows)
    assert list(seg) == list(R.LENGTHS) and all(len(v) == 2 for v in seg.values())
    for length in R.LENGTHS:
        sel = got[:, 3] == length
        assert seg[length] == [float(np.mean(got[sel, 2])), float(np.mean(got[sel, 1]))]
    assert traj_eval.compute_segment_error(rows[:1])[800] == [] and traj_eval.compute_overall_err([]) == (0, 0)
    t_err, r_err = traj_eval.compute_overall_err(rows)
    m = traj_eval.trajectory_metrics(pred, gt)
    # two sums of the same 440 non-negative terms in different orders: each within 440 x 2^-53 relative of the exact sum
    assert abs(t_err - m['t_err']) <= 440 * 2.0**-52 * t_err and abs(r_err - m['r_err']) <= 440 * 2.0**-52 * r_err
    # ATE, RPE: Python floats, the metrics dict's numbers
    ate, rpe = traj_eval.compute_ATE(pred, gt), traj_eval.compute_RPE(pred, gt)
    assert type(ate) is float and ate == m['ate'] and rpe == (m['rpe_trans'], m['rpe_rot'])
    assert f'{ate:.4f}' == f'{float(GOLDEN["ate"]):.4f}' and f'{rpe[0]:.6f}' == f'{GOLDEN["rpe"][0]:.6f}'
    # distances: a list that starts at 0
    dist = traj_eval.trajectory_distances(gt)
    assert isinstance(dist, list) and len(dist) == 1000 and dist[0] == 0 and dist[-1] == m['path_length']
    assert np.abs(np.asarray(dist) - GOLDEN['dist']).max() <= 2 * 1000 * 2.0**-52 * dist[-1]      # each within n 2^-52 path of the truth
    assert traj_eval.last_frame_from_segment_length(dist, 0, 100) == R.last_frame_linear(GOLDEN['dist'], 0, 100) > 0
    assert traj_eval.last_frame_from_segment_length(dist, 990, 100) == -1
    assert traj_eval.last_frame_from_segment_length([0, 1, 2, 3], 1, 1) == 3
    # scale_optimization: the list of 4x4 (translations only, the input untouched) and the (N,2) trajectory
    before = copy.deepcopy(pred)
    scaled, scaling = traj_eval.scale_optimization(pred, gt)
    assert scaling == float(GOLDEN['scaling']) and isinstance(scaled, list) and scaled[0].shape == (4, 4)
    assert all(np.array_equal(a, b) for a, b in zip(pred, before))
    assert np.array_equal(np.asarray([p[:3, 3] for p in scaled]), GOLDEN['scaled_xyz'])
    assert all(np.array_equal(s[:3, :3], p[:3, :3]) for s, p in zip(scaled, pred))
    xz_p = np.ascontiguousarray(np.asarray(pred)[:, [0, 2], 3])
    xz_g = np.ascontiguousarray(np.asarray(gt)[:, [0, 2], 3])
    scaled2, scaling2 = traj_eval.scale_optimization(xz_p, xz_g)
    assert scaling2 == float(GOLDEN['scaling_2d']) and np.array_equal(scaled2, GOLDEN['scaled_2d'])
    assert traj_eval.scale_lse_solver(xz_p, xz_g) == scaling2
    with pytest.raises(ClslamError):
        traj_eval.scale_optimization(np.zeros((4, 3)), np.zeros((4, 3)))
    # one 4x4
    e = np.linalg.inv(gt[7]) @ pred[7]
    # inv(I) @ e is e exactly: three squares, two sums and a root (a fused multiply-add rounds differently), one arccos
    t_ref, r_ref = float(R.translation_error(e)), float(R.rotation_error(e))
    assert abs(traj_eval.translation_error(e) - t_ref) <= 4 * 2.0**-52 * t_ref and type(traj_eval.rotation_error(e)) is float
    assert abs(traj_eval.rotation_error(e) - r_ref) <= 2.0**-52
    assert abs(traj_eval.rotation_error(np.diag([1.0, -3.0, -3.0, 1.0])) - np.pi) <= 2.0**-51     # the clamp: d = -3 -> -1


def _pair_bound(got, a, b, inverted):
    twin, truth = R.pair_errors(a, b, inverted), R.pair_errors(a, b, inverted, hp=True)
    for col in (0, 1):
        e_twin = R.element_bound(twin[:, col], truth[:, col])
        e_k = R.element_bound(got[:, col], truth[:, col])
        print(f'[pose_pair_error] column {col}: kernel {e_k:.3e} | twin {e_twin:.3e}')
        assert 0 < e_twin and e_k <= 4 * e_twin
    return truth


@pytest.mark.parametrize('backend', BACKENDS)
def test_pose_pair_error_on_the_predictors_own_output(backend):
    dev = use_backend(backend)
    p = make_predictor(H, W, 2)
    batch = synth.make_batch(2, H, W, seed=6)
    outputs, _ = p.adapt({k: v.clone() for k, v in batch.items()}, None)
    T = outputs['cam_T_cam', 0, 1]
    assert T.shape == (2, 4, 4) and T.dtype is torch.float32
    rng = np.random.default_rng(0)
    gt = T.cpu().double().numpy().copy()
    gt[:, :3, 3] += rng.normal(0, 0.05, (2, 3))
    gt[:, :3, :3] = gt[:, :3, :3] @ R._rot_y(0.01)
    for inverted in (False, True):
        h = traj_eval.pose_pair_error_async(T, torch.from_numpy(gt), pred_inverted=inverted)
        assert h.device_result.shape == (2, 2) and h.device_result.device.type == dev.type and h.device_result.dtype is torch.float64
        got = h.result()
        assert got.shape == (2, 2) and h.done()
        _pair_bound(got, T.cpu().double().numpy(), gt, inverted)
    one = traj_eval.pose_pair_error_async(T[:1], gt[0]).result()                            # the per-frame form: (1,4,4) and (4,4)
    assert one.shape == (1, 2) and np.array_equal(one[0], traj_eval.pose_pair_error_async(T, gt).result()[0])


def _pose_samples(p):
    out = []
    for i in range(3):
        batch = synth.make_batch(1, H, W, seed=50 + i)
        i0, i1 = batch['rgb_aug', -1, 0].clone(), batch['rgb_aug', 0, 0].clone()
        pred, _ = p.predict_pose(i0.clone(), i1.clone(), as_numpy=False)
        pred = pred.reshape(4, 4).cpu().double().numpy()
        gt = np.linalg.inv(pred)                                                             # dpp.py:505: the prediction is inverted first
        gt[:3, 3] += 0.02 * (i + 1)
        gt[:3, :3] = gt[:3, :3] @ R._rot_x(0.004 * (i + 1))
        out.append(({('rgb_aug', -1, 0): i0, ('rgb_aug', 0, 0): i1, ('relative_pose', 0): torch.from_numpy(gt.astype(np.float32))[None]},
                    pred))
    return out


@pytest.mark.parametrize('backend', BACKENDS)
def test_compute_pose_error_with_a_data_loader(backend, capsys):
    use_backend(backend)
    p = make_predictor(H, W, 1)
    samples = _pose_samples(p)
    a = np.stack([pred for _, pred in samples])
    b = np.stack([s['relative_pose', 0][0].double().numpy() for s, _ in samples])
    twin, truth = R.pair_errors(a, b, True), R.pair_errors(a, b, True, hp=True)
    capsys.readouterr()
    got = p.compute_pose_error(data_loader=[s for s, _ in samples])
    printed = capsys.readouterr().out.splitlines()
    assert list(got) == ['rpe_trans', 'rpe_rot'] and all(type(v) is float for v in got.values())
    deg = R.HP(180) / R.HP(np.pi)
    e_trans = R.element_bound(twin[:, 0], truth[:, 0])
    e_rot = R.element_bound(np.asarray(twin[:, 1], dtype=R.HP) * deg, truth[:, 1] * deg)
    assert e_trans > 0 and e_rot > 0
    err_t = abs(float(R.HP(got['rpe_trans']) - truth[:, 0].mean()))
    err_r = abs(float(R.HP(got['rpe_rot']) - (truth[:, 1] * deg).mean()))
    print(f'[compute_pose_error {backend}] trans {err_t:.3e} (4 x twin {4 * e_trans:.3e}) rot {err_r:.3e} deg (4 x twin {4 * e_rot:.3e})')
    assert err_t <= 4 * e_trans and err_r <= 4 * e_rot
    assert 0.01 < got['rpe_trans'] < 0.2 and 0.1 < got['rpe_rot'] < 1.0
    assert printed == [f'{k:<8}: {got[k]:>6.3f}' for k in ('rpe_trans', 'rpe_rot')]              # dpp.py:521-523
    capsys.readouterr()
    assert p.compute_pose_error(print_results=False, data_loader=[samples[0][0]])['rpe_trans'] > 0 and capsys.readouterr().out == ''
    many = p.compute_pose_error(print_results=False, data_loader=[s for s, _ in samples] * 30)  # the device buffer grows past 64 rows
    assert abs(many['rpe_trans'] - got['rpe_trans']) <= 1e-12 and abs(many['rpe_rot'] - got['rpe_rot']) <= 1e-10
    p.is_trained = False
    with pytest.warns(RuntimeWarning, match='not been trained'):
        p.compute_pose_error(print_results=False, data_loader=[samples[0][0]])


@pytest.mark.parametrize('backend', BACKENDS)
def test_compute_pose_error_unsupported_dataset(backend):
    use_backend(backend)
    from depth_pose_prediction import DepthPosePrediction
    ds = SimpleNamespace(dataset='RobotCar', config_file=Path('x.yaml'), dataset_path=None, scales=(0, 1, 2, 3), height=H, width=W,
                         frame_ids=(0, -1, 1))
    p = DepthPosePrediction(ds, make_config(1, train_set='a', val_set='b'))
    p.is_trained = True
    with pytest.warns(RuntimeWarning, match='Unsupported dataset: RobotCar'):
        assert p.compute_pose_error() == {}


def _state(p):
    w = {f'{name}.{k}': v.detach().clone() for name, m in p.models.items() for k, v in torch.nn.Module.state_dict(m).items()}
    o = copy.deepcopy(p.optimizer.state_dict())
    return w, o


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize('backend', BACKENDS)
def test_validate(backend):
    use_backend(backend)
    p = make_predictor(H, W, 2)
    noise = synth.make_noise(2, H, W, seed=7)                     # the tie-break noise of the loss is drawn anew per forward: pin it
    p.set_tie_break_noise(noise)
    batches = [synth.make_batch(2, H, W, seed=70 + i) for i in range(2)]
    clone = lambda b: {k: v.clone() for k, v in b.items()}      # noqa: E731
    expect = float(np.mean([float(p.adapt(clone(b), None)[1]['loss']) for b in batches]))
    w0, o0 = _state(p)
    with warnings.catch_warnings(record=True) as rec:             # trained, nothing to save: neither warning
        warnings.simplefilter('always')
        got = p.validate(data_loader=[clone(b) for b in batches])
    assert not [r for r in rec if 'save_val_depth' in str(r.message) or 'not been trained' in str(r.message)]
    assert type(got) is float and got == expect and np.isfinite(got)
    w1, o1 = _state(p)
    assert _same(w0, w1) and _same(o0, o1)
    with pytest.raises(NotImplementedError):
        p.train()
    with pytest.raises(ValueError, match='empty'):
        p.validate(data_loader=[])
    q = make_predictor(H, W, 2, save_val_depth=True, save_val_depth_batches=1)
    q.set_tie_break_noise(noise)
    with pytest.warns(RuntimeWarning, match='save_val_depth') as rec:
        assert q.validate(data_loader=[clone(b) for b in batches]) == expect
    assert len([r for r in rec if 'save_val_depth' in str(r.message)]) == 1          # once, not per batch
    q.is_trained = False
    with pytest.warns(RuntimeWarning, match='not been trained'):
        q.validate(data_loader=[clone(batches[0])])


@pytest.mark.gpu
def test_pose_pair_error_async_during_a_training_adapt():
    """The per-frame relative pose error is enqueued on the caller's stream right behind a detached training adapt(): its event
    completes without anything having waited for the step, and the values are those of the same call after the step."""
    dev = use_backend('hip')
    B = 2
    p = make_predictor(H, W, B, host_pose_output=False)
    eng = p.engine
    assert eng.detached_ok()
    batch = synth.make_batch(B, H, W, seed=5)
    clone = lambda: {k: v.clone() for k, v in batch.items()}     # noqa: E731
    gt = torch.eye(4, dtype=torch.float64).repeat(1, 1, 1)
    p.adapt(clone(), clone())                                     # warm-up: allocations, packing
    torch.cuda.synchronize()
    calls = []
    orig = eng.wait_training
    eng.wait_training = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        outputs, _ = p.adapt(clone(), clone())
        step_done = eng._train_done
        assert step_done is not None
        before = len(calls)
        T = outputs['cam_T_cam', 0, 1]
        assert T.is_cuda
        handle = traj_eval.pose_pair_error_async(T[:1], gt)
        assert handle.stream.cuda_stream == torch.cuda.current_stream().cuda_stream != eng.main_stream.cuda_stream
        handle.event.synchronize()
        assert handle.done()
        rows = handle.result().copy()
        assert len(calls) == before                               # nothing in between waited for backward + Adam
    finally:
        eng.wait_training = orig
    torch.cuda.synchronize()
    assert step_done.query() and dev.type == 'cuda'
    again = traj_eval.pose_pair_error_async(T[:1], gt).result()
    assert rows.shape == (1, 2) and np.array_equal(rows, again)
    e = T[0].cpu().double().numpy()                               # inv(I) @ T = T: the errors of the prediction itself
    assert abs(rows[0, 0] - float(R.translation_error(e))) <= 4 * 2.0**-52 * rows[0, 0]
    assert abs(rows[0, 1] - float(R.rotation_error(e))) <= 2.0**-52
