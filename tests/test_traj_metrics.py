"""ops.traj_metrics / ops.pose_pair_error (csrc/traj_eval.hip) against tests/traj_eval_reference.py, on the CPU emulator and on
gfx950.  The twin is the float64 restatement of slam/utils.py:129-383 (pinned to the real module by tests/golden/traj_eval.npz),
the truth the same formulae in numpy.longdouble.

Bounds (every figure of the twin is formed before the kernel's output is read; every figure is printed with -s):
  * decisions, exactly: last_frame, first_frame, length, speed of all ceil(n/10)*8 rows (the -1 rows included) and n_segments
    equal the twin's.  The fixture is first shown, on the twin alone, to keep every dist[i] at least 1e-6 m away from every
    dist[first] + length, so no decision is a matter of rounding.
  * dist: |dist_k - dist_truth| <= n * 2^-52 * path_length (each addition rounds once, the step norms round to half an ulp:
    derived, not measured).
  * per-segment rot / trans errors, RPE pair errors, pose_pair_error rows (both a_inverted): per array, the largest absolute
    deviation from the truth <= 4 x the twin's largest deviation (asserted non-zero first).
  * the scalar means (ave_t_err, ave_r_err, rpe_trans, rpe_rot, the mean square under ate), the project's rule for sums as
    tests/test_depth_metrics.py states it: the twin's error is taken PER TERM, and the kernel's mean may differ from the truth's
    mean by 4 x the mean of those errors plus the final rounding, 2 x 2^-53 relative.  ate = sqrt(mean): the bound of the mean
    divided by 2 * ate, plus the rounding of the square root.
  * scaling: the twin's, bitwise (the kernel adds in np.sum's order).
"""
import functools

import numpy as np
import pytest
import torch

import traj_eval_reference as R
from clslam_hip import _lib, ops
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

U52 = 2.0 ** -52


# ---- references, computed once ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name, optimize_scale=False):
    pred, gt = _inputs(name)
    return R.evaluate(pred, gt, optimize_scale), R.evaluate(pred, gt, optimize_scale, hp=True)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    pred, gt = R.make_fixture(1000, 0)
    if name == 'fixture':
        return pred, gt
    if name == 'tiled':                                     # KITTI 00's length: 5 scan blocks, 18 blocks of terms, 15 of segments
        return R.tile(pred, 4541), R.tile(gt, 4541)
    if name == 'stationary':                                # 50 frames standing still at frame 299: ties in dist
        idx = np.concatenate([np.arange(300), np.full(50, 299), np.arange(300, 950)])
        return pred[idx], gt[idx]
    if name == 'same':                                      # pred = gt
        return gt, gt
    if name == 'double':                                    # pred = gt with translations times two
        p = gt.copy()
        p[:, :3, 3] *= 2.0
        return p, gt
    raise KeyError(name)


def _launch(dev, pred, gt, optimize_scale=False):
    """-> out (8,), segments (S,6), dist (n,), pairs (n-1,2) as numpy"""
    p = torch.from_numpy(np.array(pred, dtype=np.float64)).to(dev)          # (a copy: the cached fixture is read-only)
    g = torch.from_numpy(np.array(gt, dtype=np.float64)).to(dev)
    n = p.shape[0]
    seg = torch.full((ops.traj_segments(n), 6), 7.0, dtype=torch.float64, device=dev)
    dist = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    pairs = torch.full((max(n - 1, 0), 2), 7.0, dtype=torch.float64, device=dev)
    out = ops.traj_metrics(p, g, optimize_scale, segments=seg, dist=dist, pairs=pairs)
    assert out.device.type == dev.type and out.shape == (8,) and out.dtype is torch.float64
    return out.cpu().numpy(), seg.cpu().numpy(), dist.cpu().numpy(), pairs.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _row(backend, case, what, kernel, twin, bound=None):
    print(f'[traj_metrics {backend}] {case:<22} {what:<20} kernel {kernel:.3e} | twin {twin:.3e}'
          + (f' ({kernel / twin:.2f}x)' if twin > 0 else '') + (f' bound {bound:.3e}' if bound is not None else ''))


def _dev(a, truth):
    d = np.abs(np.asarray(a, dtype=R.HP) - truth)
    return float(np.nanmax(d)) if d.size else 0.0


def _check_decisions(case, seg, out, twin):
    ts = twin['segments']
    for col, what in ((0, 'first_frame'), (3, 'length'), (5, 'last_frame'), (4, 'speed')):
        assert np.array_equal(seg[:, col], ts[:, col], equal_nan=True), (case, what)
    assert np.array_equal(np.isnan(seg[:, 1:3]), np.isnan(ts[:, 1:3])), case
    assert out[2] == twin['n_segments'], (case, out[2], twin['n_segments'])


def _check_elements(backend, case, what, kernel, twin, truth):
    e_twin = _dev(twin, truth)
    assert e_twin > 0, (case, what)
    e_k = _dev(kernel, truth)
    _row(backend, case, what + ' max', e_k, e_twin)
    assert e_k <= 4 * e_twin, (case, what, e_k, e_twin)


def _check_mean(backend, case, what, kernel, twin_terms, truth_terms, truth_mean, twin_mean):
    tol = R.mean_bound(twin_terms, truth_terms, truth_mean)
    err = abs(float(R.HP(kernel) - truth_mean))
    _row(backend, case, what, err, abs(float(R.HP(twin_mean) - truth_mean)), tol)
    assert err <= tol, (case, what, err, tol)
    return tol


def _check_all(backend, case, out, seg, dist, pairs, twin, truth, elements=True):
    n = len(twin['dist'])
    assert R.decision_margin(twin['dist']) >= 1e-6                                          # on the twin alone
    assert np.array_equal(twin['segments'][:, 5], truth['segments'][:, 5])
    _check_decisions(case, seg, out, twin)
    # dist
    e_dist = _dev(dist, truth['dist'])
    _row(backend, case, 'dist max', e_dist, _dev(twin['dist'], truth['dist']), n * U52 * float(truth['path_length']))
    assert e_dist <= n * U52 * float(truth['path_length'])
    assert (np.diff(dist) >= 0).all() and out[7] == dist[-1]
    ok = seg[:, 5] >= 0
    if elements:
        _check_elements(backend, case, 'segment rot', seg[ok, 1], twin['segments'][ok, 1], truth['segments'][ok, 1])
        _check_elements(backend, case, 'segment trans', seg[ok, 2], twin['segments'][ok, 2], truth['segments'][ok, 2])
        _check_elements(backend, case, 'rpe pair trans', pairs[:, 0], twin['pairs'][:, 0], truth['pairs'][:, 0])
        _check_elements(backend, case, 'rpe pair rot', pairs[:, 1], twin['pairs'][:, 1], truth['pairs'][:, 1])
    # means
    _check_mean(backend, case, 'ave_t_err', out[0], twin['segments'][ok, 2], truth['segments'][ok, 2], truth['t_err'], twin['t_err'])
    _check_mean(backend, case, 'ave_r_err', out[1], twin['segments'][ok, 1], truth['segments'][ok, 1], truth['r_err'], twin['r_err'])
    _check_mean(backend, case, 'rpe_trans', out[4], twin['pairs'][:, 0], truth['pairs'][:, 0], truth['rpe_trans'], twin['rpe_trans'])
    _check_mean(backend, case, 'rpe_rot', out[5], twin['pairs'][:, 1], truth['pairs'][:, 1], truth['rpe_rot'], twin['rpe_rot'])
    ms_truth = truth['ate_sq'].mean()
    tol_ms = R.mean_bound(twin['ate_sq'], truth['ate_sq'], ms_truth)
    tol_ate = tol_ms / (2 * float(truth['ate'])) + U52 * float(truth['ate'])
    err = abs(float(R.HP(out[3]) - truth['ate']))
    _row(backend, case, 'ate', err, abs(float(R.HP(twin['ate']) - truth['ate'])), tol_ate)
    assert err <= tol_ate
    assert _bits(out[6]) == _bits(twin['scaling'])


# ---- the twin itself ----------------------------------------------------------------------------------------------------
def test_twin_is_the_reference_to_the_last_bit():
    g = np.load(R.__file__.replace('traj_eval_reference.py', 'golden/traj_eval.npz'))
    pred, gt = R.make_fixture(1000, 0)
    assert np.array_equal(_bits(pred), _bits(g['pred'])) and np.array_equal(_bits(gt), _bits(g['gt']))
    twin, _ = _reference('fixture')
    scaled, _ = _reference('fixture', True)
    assert R.format_log(twin, False) == str(g['log_plain']) and R.format_log(scaled, True) == str(g['log_scaled'])
    assert np.array_equal(_bits(np.asarray(R.sequence_errors(twin), dtype=np.float64)), _bits(g['sequence_errors']))
    assert np.array_equal(_bits(np.asarray(R.sequence_errors(scaled), dtype=np.float64)), _bits(g['sequence_errors_scaled']))
    assert np.array_equal(_bits(twin['dist']), _bits(g['dist']))
    assert _bits(twin['ate']) == _bits(g['ate']) and _bits(twin['scaling']) == _bits(g['scaling'])
    assert np.array_equal(_bits([twin['rpe_trans'], twin['rpe_rot']]), _bits(g['rpe']))
    assert np.array_equal(_bits([twin['t_err'], twin['r_err']]), _bits(g['overall']))
    # the searchsorted restatement is the reference's linear scan
    first, length, last = R.segment_frames(twin['dist'])
    assert [R.last_frame_linear(twin['dist'], int(f), int(l)) for f, l in zip(first, length)] == list(last)
    assert (last >= 0).sum() == 440 and (last < 0).sum() == 360 and set(length[last >= 0]) == set(R.LENGTHS)


# ---- the fixture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('optimize_scale', [False, True], ids=['plain', 'scaled'])
def test_fixture(backend, optimize_scale):
    dev = use_backend(backend)
    pred, gt = _inputs('fixture')
    twin, truth = _reference('fixture', optimize_scale)
    out, seg, dist, pairs = _launch(dev, pred, gt, optimize_scale)
    _check_all(backend, f'fixture scale={int(optimize_scale)}', out, seg, dist, pairs, twin, truth)
    if optimize_scale:                                      # only the sequence errors see the scaled translations (utils.py:374,378)
        plain = _launch(dev, pred, gt, False)
        assert _bits(out[3]) == _bits(plain[0][3]) and np.array_equal(_bits(out[4:8]), _bits(plain[0][4:8]))
        assert np.array_equal(_bits(pairs), _bits(plain[3])) and out[0] != plain[0][0]


@pytest.mark.parametrize('backend', BACKENDS)
def test_stationary_stretch(backend):
    dev = use_backend(backend)
    pred, gt = _inputs('stationary')
    twin, truth = _reference('stationary')
    out, seg, dist, pairs = _launch(dev, pred, gt)
    assert (np.diff(dist)[299:349] == 0).all()              # ties in dist
    _check_all(backend, 'stationary', out, seg, dist, pairs, twin, truth)


@pytest.mark.parametrize('backend', BACKENDS)
def test_kitti_length(backend):
    """4541 poses: several blocks in the scan, the terms, the segments and the partials of the finalising block; decisions against
    the searchsorted restatement, the sums at their bounds"""
    dev = use_backend(backend)
    pred, gt = _inputs('tiled')
    twin, truth = _reference('tiled')
    out, seg, dist, pairs = _launch(dev, pred, gt)
    assert twin['n_segments'] > 2500
    _check_all(backend, 'tiled 4541', out, seg, dist, pairs, twin, truth, elements=False)


# ---- pose_pair_error ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('a_inverted', [False, True], ids=['plain', 'inverted'])
def test_pose_pair_error(backend, a_inverted):
    """the relative motions of the fixture, 999 pairs (four blocks, the last one partly filled)"""
    dev = use_backend(backend)
    pred, gt = _inputs('fixture')
    a = np.stack([np.linalg.inv(pred[i]) @ pred[i + 1] for i in range(999)])
    b = np.stack([np.linalg.inv(gt[i]) @ gt[i + 1] for i in range(999)])
    if a_inverted:
        a = np.stack([np.linalg.inv(m) for m in a])         # inverted once more by the kernel: not the same bits, the same pose
    twin, truth = R.pair_errors(a, b, a_inverted), R.pair_errors(a, b, a_inverted, hp=True)
    out = ops.pose_pair_error(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), a_inverted=a_inverted)
    assert out.shape == (999, 2) and out.dtype is torch.float64
    k = out.cpu().numpy()
    _check_elements(backend, f'pair inverted={int(a_inverted)}', 'trans', k[:, 0], twin[:, 0], truth[:, 0])
    _check_elements(backend, f'pair inverted={int(a_inverted)}', 'rot', k[:, 1], twin[:, 1], truth[:, 1])
    again = ops.pose_pair_error(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), a_inverted=a_inverted)
    assert np.array_equal(_bits(k), _bits(again.cpu().numpy()))
    # a batch of none
    empty = ops.pose_pair_error(torch.zeros(0, 4, 4, dtype=torch.float64, device=dev), torch.zeros(0, 4, 4, dtype=torch.float64, device=dev))
    assert empty.shape == (0, 2)


# ---- exact cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_shift_by_3_4_0_gives_ate_5(backend):
    dev = use_backend(backend)
    _, gt = _inputs('fixture')
    gt = gt.copy()
    gt[:, :3, 3] = np.round(gt[:, :3, 3] * 1024.0) / 1024.0      # translations on a 2^-10 grid: the shift below is exact
    pred = gt.copy()
    pred[:, :3, 3] += np.array([3.0, 4.0, 0.0])
    assert np.array_equal(gt[:, :3, 3] - pred[:, :3, 3], np.broadcast_to([-3.0, -4.0, 0.0], (1000, 3)))
    out, _, _, _ = _launch(dev, pred, gt)
    assert out[3] == 5.0


@pytest.mark.parametrize('backend', BACKENDS)
def test_translations_times_two(backend):
    """scaling == 0.5 exactly (a power of two commutes with rounding); with optimize_scale the scaled prediction IS gt, so the
    sequence errors are those of pred = gt -- bitwise the launch on (gt, gt), and within the element bound of the truth --
    while ATE and RPE are those of the unscaled input"""
    dev = use_backend(backend)
    pred, gt = _inputs('double')
    plain = _launch(dev, pred, gt, False)
    scaled = _launch(dev, pred, gt, True)
    same = _launch(dev, gt, gt, False)
    assert plain[0][6] == 0.5 and scaled[0][6] == 0.5 and same[0][6] == 1.0
    assert np.array_equal(_bits(scaled[1]), _bits(same[1])) and np.array_equal(_bits(scaled[0][:3]), _bits(same[0][:3]))
    assert np.array_equal(_bits(scaled[0][3:6]), _bits(plain[0][3:6])) and np.array_equal(_bits(scaled[3]), _bits(plain[3]))
    assert plain[0][0] > 0.5                                 # unscaled: every segment is off by its own length
    twin, truth = _reference('same')
    ok = same[1][:, 5] >= 0
    _check_decisions('double', scaled[1], scaled[0], twin)
    _check_elements(backend, 'pred = gt', 'segment rot', scaled[1][ok, 1], twin['segments'][ok, 1], truth['segments'][ok, 1])
    _check_elements(backend, 'pred = gt', 'segment trans', scaled[1][ok, 2], twin['segments'][ok, 2], truth['segments'][ok, 2])


# ---- edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', [1, 2, 9, 11, 61])
def test_short_trajectories_have_no_segment(backend, n):
    """1, 2, 9, 11 poses and a 60 m path: (0, 0) and no segment; the rows of a first frame that is the last pose (n = 11: frame
    10; n = 1, 61) exist and say -1; RPE is NaN for one pose"""
    dev = use_backend(backend)
    pred, gt = R.make_fixture(n, 3)
    twin = R.evaluate(pred, gt)
    out, seg, dist, pairs = _launch(dev, pred, gt)
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0 and twin['n_segments'] == 0
    assert seg.shape == ((n + 9) // 10 * 8, 6) and (seg[:, 5] == -1).all() and np.isnan(seg[:, [1, 2, 4]]).all()
    _check_decisions(f'n={n}', seg, out, twin)
    assert dist[0] == 0.0 and abs(dist[-1] - twin['path_length']) <= n * U52 * twin['path_length'] and out[7] == dist[-1]
    if n == 61:
        assert 55.0 < out[7] < 65.0
    if n == 1:
        assert np.isnan(out[4]) and np.isnan(out[5]) and pairs.shape == (0, 2)
    else:
        assert pairs.shape == (n - 1, 2) and np.isfinite(out[3:6]).all()
    assert _bits(out[6]) == _bits(twin['scaling'])


@pytest.mark.parametrize('backend', BACKENDS)
def test_segment_start_at_the_last_frame_of_a_long_run(backend):
    dev = use_backend(backend)
    pred, gt = _inputs('fixture')
    pred, gt = pred[:991], gt[:991]                          # first_frame 990 is the last pose
    twin = R.evaluate(pred, gt)
    out, seg, _, _ = _launch(dev, pred, gt)
    assert seg.shape == (800, 6) and (seg[-8:, 0] == 990).all() and (seg[-8:, 5] == -1).all()
    _check_decisions('n=991', seg, out, twin)


@pytest.mark.parametrize('backend', BACKENDS)
def test_no_pose_at_all(backend):
    dev = use_backend(backend)
    z = torch.zeros(0, 4, 4, dtype=torch.float64, device=dev)
    out = ops.traj_metrics(z, z).cpu().numpy()
    assert (out[[0, 1, 2, 7]] == 0).all() and np.isnan(out[3:7]).all()


@pytest.mark.parametrize('backend', BACKENDS)
def test_two_launches_are_bitwise_equal(backend):
    dev = use_backend(backend)
    pred, gt = _inputs('tiled')
    a, b = _launch(dev, pred, gt, True), _launch(dev, pred, gt, True)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    p, g = torch.from_numpy(pred.copy()).to(dev), torch.from_numpy(gt.copy()).to(dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    assert ops.traj_metrics(p, g, True, out=out) is out                  # without the optional outputs too
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(a[0]))


@pytest.mark.parametrize('backend', BACKENDS)
def test_argument_checks(backend):
    dev = use_backend(backend)
    lib = _lib.get_lib()
    p = torch.eye(4, dtype=torch.float64, device=dev).repeat(3, 1, 1)
    with pytest.raises(ClslamError):
        ops.traj_metrics(p.float(), p)
    with pytest.raises(ClslamError):
        ops.traj_metrics(p, p[:2])
    with pytest.raises(ClslamError):
        ops.traj_metrics(p[:, :3], p)
    with pytest.raises(ClslamError):
        ops.traj_metrics(p, p, out=torch.empty(7, dtype=torch.float64, device=dev))
    with pytest.raises(ClslamError):
        ops.traj_metrics(p, p, segments=torch.empty(8, 5, dtype=torch.float64, device=dev))
    with pytest.raises(ClslamError):
        ops.pose_pair_error(p, p[:2])
    with pytest.raises(ClslamError):
        ops.pose_pair_error(p, p.float())
    with pytest.raises(ClslamError):
        ops.pose_pair_error(p, p, out=torch.empty(3, 3, dtype=torch.float64, device=dev))
    if dev.type == 'cuda':
        with pytest.raises(ClslamError):
            ops.traj_metrics(p.cpu(), p.cpu())
    # the C ABI's own checks, with the library's message
    out = torch.empty(8, dtype=torch.float64, device=dev)
    scratch = torch.empty(ops.traj_metrics_scratch(3), dtype=torch.float64, device=dev)
    P, O, S = p.data_ptr(), out.data_ptr(), scratch.data_ptr()
    with pytest.raises(ClslamError, match='traj_metrics: null pointer'):
        lib.call('clslam_traj_metrics', None, P, 3, 0, O, None, None, S, None)
    with pytest.raises(ClslamError, match='traj_metrics: null pointer'):
        lib.call('clslam_traj_metrics', P, P, 3, 0, None, None, None, S, None)
    with pytest.raises(ClslamError, match='traj_metrics: null pointer'):
        lib.call('clslam_traj_metrics', P, P, 3, 0, O, None, None, None, None)
    with pytest.raises(ClslamError, match='traj_metrics: n must be'):
        lib.call('clslam_traj_metrics', P, P, -1, 0, O, None, None, S, None)
    with pytest.raises(ClslamError, match='traj_metrics: n must be'):
        lib.call('clslam_traj_metrics', P, P, _lib.TRAJ_MAX_POSES + 1, 0, O, None, None, S, None)
    assert ops.traj_metrics_scratch(_lib.TRAJ_MAX_POSES + 1) == 0 and ops.traj_metrics_scratch(-1) == 0
    assert ops.traj_metrics_scratch(_lib.TRAJ_MAX_POSES) > 0 and ops.traj_metrics_scratch(0) > 0
    with pytest.raises(ClslamError, match='pose_pair_error: negative n'):
        lib.call('clslam_pose_pair_error', P, P, -1, 0, O, None)
    with pytest.raises(ClslamError, match='pose_pair_error: null pointer'):
        lib.call('clslam_pose_pair_error', P, None, 3, 0, O, None)
    lib.call('clslam_pose_pair_error', None, None, 0, 0, None, None)    # n = 0: a no-op
