"""ops.depth_metrics (csrc/depth_eval.hip) against the float64 restatement of tests/depth_eval_reference.py, on the CPU emulator
and on gfx950.

Bounds (every fp32 figure is formed before the kernel's output is read; every figure is printed with -s):
  * identities, bitwise: an equal-size resample is `pred`; n is the reference count; the ground-truth median is np.median of
    the masked fp32 values (the kernel does not transform them); the prediction median is np.median of the kernel's OWN
    resampled values (its optional `resampled` output), which separates the selection from the interpolation's rounding; the
    ratio is the fp32 quotient of the kernel's two medians; a batch equals its single-image launches; two launches are equal.
  * resampled plane: largest absolute error against float64 over the masked pixels <= 4 x the fp32 twin's.
  * the five sums (abs_diff, abs_rel, sq_rel, rmse, rmse_log), the project's rule for a sum of non-negative terms as
    tests/test_loss_kernels.py applies it to tile sums: the twin's error is taken PER TERM, e_i = |term32_i - term64_i| on the
    twin's own scaled and clamped prediction, and the kernel's mean may differ from the float64 mean by 4 x mean(e_i) plus the
    final rounding of the result to fp32, 2 x 2^-24 relative (the kernel accumulates in double, so the n x 2^-24 allowance of
    an fp32 summation is not claimed).  The twin's SCALAR error is not used as the yardstick: it is the sum of the same e_i
    with their signs plus the rounding of np.mean's fp32 pairwise sum, which cancels to anywhere between 0 and a few ulp of
    the result by chance, and the kernel's own ~1 ulp would be compared with that chance figure.  It is printed next to the
    kernel's.  rmse and rmse_log are square roots of such means: the bound of the mean is propagated through sqrt.
  * a1..a3: the kernel's count must be the count of the fp32 formula on the kernel's own resampled values and ratio, exactly;
    pixel by pixel that decision must equal the float64 one except where the float64 `thresh` lies within 1e-5 relative of
    the threshold; the inputs are built so that at most 0.1 % of n lie in that band (asserted on the float64 reference first);
    every differing pixel is counted and must lie in the band.
"""
import numpy as np
import pytest
import torch

import depth_eval_reference as R
from clslam_hip import ops
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

SUMS = R.SUMS
COL = {k: i for i, k in enumerate(R.KEYS)}


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _smooth(rng, h, w, lo, hi):
    """a smooth positive field with grain, float32"""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    a, b, c = rng.uniform(1, 4, 3)
    f = 0.5 + 0.25 * np.sin(a * xx * 3 + b * yy) + 0.2 * np.cos(c * yy * 4 - xx) + 0.05 * (rng.random((h, w)) - 0.5)
    f = (f - f.min()) / (f.max() - f.min())
    return (lo + (hi - lo) * f).astype(np.float32)


def _scene(seed, h, w, hg, wg, valid=1.0, lo=3.0, hi=60.0, quantise=None):
    """prediction (h,w) and a ground truth (hg,wg) that is the resampled prediction times a per-pixel factor in [0.5, 2.2]
    (thresh spreads continuously over the three thresholds), invalid pixels 0"""
    rng = np.random.default_rng(seed)
    pred = _smooth(rng, h, w, lo, hi)
    base = R.resample(pred.astype(np.float64), hg, wg, np.float64)
    gt = (base * np.exp(rng.uniform(np.log(0.5), np.log(2.2), (hg, wg)))).astype(np.float32)
    if quantise:
        gt = (np.round(gt / quantise) * quantise).astype(np.float32)
    if valid < 1.0:
        gt[rng.random((hg, wg)) >= valid] = 0.0
    return pred, gt


def _launch(dev, pred, gt, lo, hi, **kw):
    """pred (N,h,w), gt (N,hg,wg) numpy -> out (N,10), resampled (N,hg,wg), medians (N,2) as numpy"""
    pred, gt = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(gt, np.float32)
    rs = torch.full(gt.shape, float('nan'), device=dev)
    med = torch.full((gt.shape[0], 2), float('nan'), device=dev)
    out = ops.depth_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), lo, hi, resampled=rs, medians=med, **kw)
    assert out.device.type == dev.type and out.shape == (gt.shape[0], 10)
    return out.cpu().numpy(), rs.cpu().numpy(), med.cpu().numpy()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _row(backend, case, what, kernel, fp32):
    print(f'[depth_metrics {backend}] {case:<34} {what:<22} kernel {kernel:.3e} | fp32 {fp32:.3e}'
          + (f' ({kernel / fp32:.2f}x)' if fp32 > 0 else ''))


def _check_image(backend, case, pred, gt, lo, hi, out, rs, med, scaling=True, from_disp=False):
    """every check of one image; pred (h,w), gt (hg,wg), out (10,), rs (hg,wg), med (2,)"""
    r64 = R.evaluate(pred, gt, lo, hi, scaling, from_disp)
    r32 = R.evaluate(pred, gt, lo, hi, scaling, from_disp, dtype=np.float32)
    n, m = r64['n'], r64['mask']
    assert out[9] == n, (out[9], n)                                               # exactly the reference count
    if n == 0:
        assert np.isnan(out[:9]).all()
        return r64
    # fp32 figures first ------------------------------------------------------------------------------------------------
    e32_res = float(np.abs(r32['resampled'][m].astype(np.float64) - r64['resampled'][m]).max())
    tol = R.bounds(r64, r32)
    e32 = {k: abs(float(r32[k]) - float(r64[k])) for k in SUMS}
    band = tol['band']
    for k in band:
        assert band[k].sum() <= 1e-3 * n, (case, k, int(band[k].sum()), n)        # the float64 reference itself, before the kernel
    # the kernel ----------------------------------------------------------------------------------------------------------
    ek = float(np.abs(rs[m].astype(np.float64) - r64['resampled'][m]).max())
    _row(backend, case, 'resampled max', ek, e32_res)
    assert ek <= 4 * e32_res, (case, ek, e32_res)
    if scaling:
        assert _bits(med[0]) == _bits(np.median(gt[m])), (case, med[0], np.median(gt[m]))
        assert _bits(med[1]) == _bits(np.median(rs[m])), (case, med[1], np.median(rs[m]))
        assert _bits(out[8]) == _bits(np.float32(med[0]) / np.float32(med[1]))
        er, er32 = abs(float(out[8]) - float(r64['ratio'])), abs(float(r32['ratio']) - float(r64['ratio']))
        _row(backend, case, 'ratio', er, er32)
        assert er <= tol['ratio']
    else:
        assert out[8] == 1.0
    for k in SUMS:
        err = abs(float(out[COL[k]]) - float(r64[k]))
        _row(backend, case, k, err, e32[k])
        print(f'{"":<60} bound {tol[k]:.3e}')
        assert err <= tol[k], (case, k, err, tol[k])
    # thresholds: the kernel's decision rebuilt from its own resampled values and ratio, pixel by pixel
    pk = rs[m] * out[8] if scaling else rs[m].copy()
    pk = np.maximum(pk, np.float32(lo))
    if hi is not None:
        pk = np.minimum(pk, np.float32(hi))
    gk = gt[m]
    tk = np.maximum(gk / pk, pk / gk)
    assert tk.dtype == np.float32
    for k, t in zip(('a1', 'a2', 'a3'), R.THRESHOLDS):
        dec = tk < np.float32(t)
        assert round(float(out[COL[k]]) * n) == int(dec.sum()), (case, k, float(out[COL[k]]) * n, int(dec.sum()))
        differ = dec != (r64['thresh'] < t)
        print(f'[depth_metrics {backend}] {case:<34} {k} differing {int(differ.sum())} in band {int(band[k].sum())} of {n}')
        assert not (differ & ~band[k]).any(), (case, k, int((differ & ~band[k]).sum()))
    return r64


# ---- resample geometry ------------------------------------------------------------------------------------------------------
GEOMETRY = [(24, 80, 47, 155), (32, 96, 32, 96), (48, 160, 30, 100), (8, 8, 9, 200)]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('h,w,hg,wg', GEOMETRY, ids=[f'{a}x{b}-{c}x{d}' for a, b, c, d in GEOMETRY])
def test_resample_geometry(backend, h, w, hg, wg):
    """non-integer ratios with both borders clamping, the identity, shrinking (no antialiasing), one axis nearly untouched"""
    dev = use_backend(backend)
    pred, gt = _scene(h * 1000 + wg, h, w, hg, wg)
    x0, _ = R.linear_coords(wg, w)
    y0, _ = R.linear_coords(hg, h)
    if hg > h and wg > w:                                                               # enlarging: the first and last source coordinates lie outside
        assert x0[0] == 0 and x0[-1] == w - 1 and y0[0] == 0 and y0[-1] == h - 1       # both borders take the clamped cell
    out, rs, med = _launch(dev, pred[None], gt[None], 0.1, 1000.0)
    assert out[0, 9] == hg * wg                                                         # dense: every pixel is compared
    if (h, w) == (hg, wg):
        assert np.array_equal(_bits(rs[0]), _bits(pred))
    _check_image(backend, f'geometry {h}x{w}->{hg}x{wg}', pred, gt, 0.1, 1000.0, out[0], rs[0], med[0])


# ---- mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('hi', [80.0, None], ids=['max80', 'maxNone'])
def test_mask_edges(backend, hi):
    """ground truth exactly at min_depth and at max_depth is excluded (both comparisons strict); max_depth=None has no upper
    bound and no upper clamp; n is the reference count"""
    dev = use_backend(backend)
    lo = 0.1
    pred, gt = _scene(7, 20, 64, 33, 101, lo=2.0, hi=70.0)
    flat = gt.reshape(-1)
    flat[::7] = np.float32(lo)
    flat[3::11] = np.float32(80.0)
    flat[5::13] = np.nextafter(np.float32(lo), np.float32(1))
    flat[6::17] = np.nextafter(np.float32(80.0), np.float32(0))
    flat[8::19] = 95.0
    out, rs, med = _launch(dev, pred[None], gt[None], lo, hi)
    r = _check_image(backend, f'mask edges max={hi}', pred, gt, lo, hi, out[0], rs[0], med[0])
    expect = (gt > np.float32(lo)) & ((gt < np.float32(80.0)) if hi is not None else True)
    assert r['n'] == int(expect.sum()) == out[0, 9]
    assert (rs[0][~expect] == 0).all()
    if hi is None:
        assert float(r['pred'].max()) > 80.0


# ---- order statistics -------------------------------------------------------------------------------------------------------
def _sparse_gt(hg, wg, values, seed=0):
    gt = np.zeros(hg * wg, np.float32)
    idx = np.random.default_rng(seed).choice(hg * wg, len(values), replace=False)
    gt[idx] = values
    return gt.reshape(hg, wg)


ORDER = ['odd', 'even', 'one', 'two', 'zero', 'all_equal', 'quantised', 'lowest_bit', 'lowest_bit_pair', 'cross_block']


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', ORDER)
def test_order_statistics(backend, kind):
    dev = use_backend(backend)
    rng = np.random.default_rng(ORDER.index(kind))
    h, w, hg, wg = 16, 48, 37, 111
    pred = _smooth(rng, h, w, 3.0, 60.0)
    if kind in ('odd', 'even', 'one', 'two', 'zero'):
        n = {'odd': 1001, 'even': 1000, 'one': 1, 'two': 2, 'zero': 0}[kind]
        gt = _sparse_gt(hg, wg, rng.uniform(2.0, 70.0, n).astype(np.float32))
    elif kind == 'all_equal':
        gt = np.full((hg, wg), 12.34, np.float32)
    elif kind == 'quantised':
        gt = (np.round(rng.uniform(10.0, 10.45, (hg, wg)) / 0.01) * 0.01).astype(np.float32)      # <= 46 distinct values, 4107 pixels
        assert len(np.unique(gt)) < 50
    elif kind == 'lowest_bit':
        a = np.float32(17.3)
        gt = np.where(rng.random((hg, wg)) < 0.5, a, np.nextafter(a, np.float32(100))).astype(np.float32)
        gt.reshape(-1)[0] = 0.0                                                             # n even: the two middle elements
    elif kind == 'lowest_bit_pair':
        a = np.float32(17.3)
        gt = _sparse_gt(hg, wg, np.array([a, np.nextafter(a, np.float32(100))], np.float32))
    else:
        h, w, hg, wg = 40, 120, 120, 400                                                    # 47 blocks: the cross-block merge
        pred, gt = _scene(11, h, w, hg, wg)
    out, rs, med = _launch(dev, pred[None], gt[None], 0.1, 80.0)
    r = _check_image(backend, f'order {kind}', pred, gt, 0.1, 80.0, out[0], rs[0], med[0])
    if kind == 'zero':
        assert r['n'] == 0 and np.isnan(out[0, :9]).all() and out[0, 9] == 0 and np.isnan(med).all()
    if kind == 'lowest_bit_pair':
        assert out[0, 9] == 2
    if kind == 'all_equal':
        assert _bits(med[0, 0]) == _bits(np.float32(12.34))


# ---- sparse batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_sparse_batch_equals_single_launches(backend):
    """5 % valid at random positions, three images with different n (one of them empty of valid pixels in its upper half)
    in one launch == the three single-image launches, bitwise"""
    dev = use_backend(backend)
    h, w, hg, wg = 24, 80, 61, 203
    scenes = [_scene(20 + i, h, w, hg, wg, valid=v) for i, v in enumerate((0.05, 0.03, 0.08))]
    scenes[1][1][: hg // 2] = 0.0
    pred, gt = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    out, rs, med = _launch(dev, pred, gt, 0.1, 80.0)
    assert len({int(v) for v in out[:, 9]}) == 3
    for i in range(3):
        o1, r1, m1 = _launch(dev, pred[i:i + 1], gt[i:i + 1], 0.1, 80.0)
        assert np.array_equal(_bits(o1[0]), _bits(out[i])) and np.array_equal(_bits(r1[0]), _bits(rs[i]))
        assert np.array_equal(_bits(m1[0]), _bits(med[i]))
        _check_image(backend, f'sparse batch image {i}', pred[i], gt[i], 0.1, 80.0, out[i], rs[i], med[i])


# ---- modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_without_median_scaling(backend):
    dev = use_backend(backend)
    pred, gt = _scene(31, 24, 80, 47, 155, valid=0.6)
    pred = (pred * np.float32(1.3)).astype(np.float32)             # off-scale on purpose: the unscaled errors differ from the scaled
    out, rs, med = _launch(dev, pred[None], gt[None], 0.1, 80.0, median_scaling=False)
    _check_image(backend, 'no median scaling', pred, gt, 0.1, 80.0, out[0], rs[0], med[0], scaling=False)
    scaled, _, _ = _launch(dev, pred[None], gt[None], 0.1, 80.0)
    assert abs(scaled[0, 0] - out[0, 0]) > 1e-3 * out[0, 0]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('hi', [100.0, None], ids=['max100', 'maxNone'])
def test_from_disparity(backend, hi):
    """sigmoid disparities down to 0.01 and up to 1.0 (depth = min_depth / disp per tap, then the interpolation); the ground truth
    follows the depth, so median scaling finds a ratio near 50"""
    dev = use_backend(backend)
    rng = np.random.default_rng(41)
    h, w, hg, wg = 24, 80, 47, 155
    disp = _smooth(rng, h, w, 0.01, 1.0)
    disp[0, :5], disp[-1, -5:] = 0.01, 1.0
    depth = np.float32(0.1) / disp.astype(np.float64)
    gt = (50 * R.resample(depth, hg, wg, np.float64) * np.exp(rng.uniform(np.log(0.5), np.log(2.2), (hg, wg)))).astype(np.float32)
    gt[rng.random((hg, wg)) < 0.3] = 0.0
    out, rs, med = _launch(dev, disp[None], gt[None], 0.1, hi, from_disp=True)
    _check_image(backend, f'from disparity max={hi}', disp, gt, 0.1, hi, out[0], rs[0], med[0], from_disp=True)
    assert 40 < out[0, 8] < 60


@pytest.mark.parametrize('backend', BACKENDS)
def test_two_launches_are_bitwise_equal(backend):
    dev = use_backend(backend)
    scenes = [_scene(50 + i, 40, 120, 120, 400, valid=v) for i, v in enumerate((1.0, 0.4))]
    pred, gt = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    a, b = _launch(dev, pred, gt, 0.1, 80.0), _launch(dev, pred, gt, 0.1, 80.0)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    out = torch.empty(2, 10, device=dev)
    assert ops.depth_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), 0.1, 80.0, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(a[0]))                  # without the optional outputs too


@pytest.mark.parametrize('backend', BACKENDS)
def test_real_size(backend):
    """the network's 192x640 plane against a KITTI-sized 376x1241 ground truth, 5 % valid, quantised to centimetres"""
    dev = use_backend(backend)
    pred, gt = _scene(61, 192, 640, 376, 1241, valid=0.05, quantise=0.01)
    out, rs, med = _launch(dev, pred[None], gt[None], 0.1, 80.0)
    _check_image(backend, 'real size', pred, gt, 0.1, 80.0, out[0], rs[0], med[0])


@pytest.mark.parametrize('backend', BACKENDS)
def test_argument_checks(backend):
    dev = use_backend(backend)
    p, g = torch.ones(1, 4, 6, device=dev), torch.ones(1, 5, 7, device=dev)
    with pytest.raises(ClslamError):
        ops.depth_metrics(p.double(), g, 0.1, 80.0)
    with pytest.raises(ClslamError):
        ops.depth_metrics(p[0], g, 0.1, 80.0)
    with pytest.raises(ClslamError):
        ops.depth_metrics(p, torch.ones(2, 5, 7, device=dev), 0.1, 80.0)
    with pytest.raises(ClslamError):
        ops.depth_metrics(p, g, None, 80.0)
    with pytest.raises(ClslamError):
        ops.depth_metrics(p, g, 0.1, 80.0, out=torch.empty(1, 8, device=dev))
    with pytest.raises(ClslamError):
        ops.depth_metrics(p.transpose(1, 2), g, 0.1, 80.0)
    if dev.type == 'cuda':
        with pytest.raises(ClslamError):
            ops.depth_metrics(p.cpu(), g.cpu(), 0.1, 80.0)
    assert ops.depth_metrics(p[:0], g[:0], 0.1, 80.0).shape == (0, 10)
