"""Restatement of the depth-error evaluation (slam/utils.py:389-442; dpp.py:396-440 with disp_to_depth(disp, min_depth, None)
in front), written from the rules in include/clslam_hip.h, in numpy.

``evaluate(pred, gt, ..., dtype=np.float64)`` is the reference proper: the fp32 inputs are taken as exact and every operation
after them runs in float64.  ``dtype=np.float32`` is its twin: the arithmetic numpy does in the reference, where the arrays are
float32 and np.mean / np.median stay in float32.  What both share are the DECISIONS the rule makes in single precision and the
inputs as the kernel receives them: the source coordinate of the resampling is narrowed to float32 and its floor and fraction
are taken there (OpenCV's INTER_LINEAR on float images), and min_depth / max_depth are float32 numbers (numpy compares and
divides a float32 array with a Python float in float32).

OpenCV is not installed where this project is developed, so the resampling rule is restated, not compared against cv2.resize.
"""
import numpy as np

KEYS = ('abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3', 'rmse', 'rmse_log')      # utils.py:431-440, the kernel's order
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)                                           # exact in float32


def linear_coords(dst: int, src: int):
    """cell (int64) and fraction (float32) of every destination index: (d + 0.5) * (src / dst) - 0.5 in double, narrowed to
    float32; floor; cell < 0 -> (0, 0); cell >= src - 1 -> (src - 1, 0)"""
    scale = float(src) / float(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    cell = np.floor(f)
    frac = (f - cell).astype(np.float32)
    cell = cell.astype(np.int64)
    low, high = cell < 0, cell >= src - 1
    cell = np.where(low, 0, np.where(high, src - 1, cell))
    frac = np.where(low | high, np.float32(0), frac).astype(np.float32)
    return cell, frac


def resample(depth: np.ndarray, hg: int, wg: int, dtype) -> np.ndarray:
    """depth (h,w) of `dtype` -> (hg,wg): horizontal pass (1-fx)*a + fx*b on the two rows, then the vertical pass"""
    h, w = depth.shape
    x0, fx = linear_coords(wg, w)
    y0, fy = linear_coords(hg, h)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = fx.astype(dtype)[None, :], fy.astype(dtype)[:, None]
    one = dtype(1)
    rows = (one - fx) * depth[:, x0] + fx * depth[:, x1]                  # (h, wg)
    return (one - fy) * rows[y0] + fy * rows[y1]


def median(v: np.ndarray):
    """np.median: middle element, or the mean of the two middle elements (in v's dtype)"""
    return np.median(v)


def evaluate(pred, gt, min_depth, max_depth, median_scaling=True, from_disp=False, dtype=np.float64):
    """one image: pred (h,w), gt (hg,wg) float32 arrays.  -> dict with the intermediate planes and the metrics in `dtype`"""
    pred = np.asarray(pred, dtype=np.float32)
    gt32 = np.asarray(gt, dtype=np.float32)
    lo = np.float32(min_depth)
    hi = None if max_depth is None else np.float32(max_depth)
    depth = pred.astype(dtype)
    if from_disp:
        depth = dtype(lo) / depth
    res = resample(depth, gt32.shape[0], gt32.shape[1], dtype)
    mask = gt32 > lo
    if hi is not None:
        mask &= gt32 < hi
    n = int(mask.sum())
    out = {'resampled': res, 'mask': mask, 'n': n}
    if n == 0:
        out.update({k: float('nan') for k in KEYS}, ratio=float('nan'), med_gt=float('nan'), med_pred=float('nan'))
        return out
    g = gt32[mask].astype(dtype)
    p = res[mask].astype(dtype)
    ratio = dtype(1)
    if median_scaling:
        out['med_gt'], out['med_pred'] = median(g), median(p)
        ratio = dtype(out['med_gt'] / out['med_pred'])
        p = p * ratio
    p = np.maximum(p, dtype(lo))
    if hi is not None:
        p = np.minimum(p, dtype(hi))
    thresh = np.maximum(g / p, p / g)
    d = g - p
    dl = np.log(g) - np.log(p)
    out.update(ratio=ratio, pred=p, gt=g, thresh=thresh,
               abs_diff=np.mean(np.abs(d)), abs_rel=np.mean(np.abs(d) / g), sq_rel=np.mean(d ** 2 / g),
               rmse=np.sqrt(np.mean(d ** 2)), rmse_log=np.sqrt(np.mean(dl ** 2)))
    for k, t in zip(('a1', 'a2', 'a3'), THRESHOLDS):
        out[k + '_count'] = int((thresh < dtype(t)).sum())
        out[k] = out[k + '_count'] / n                                   # np.mean of a bool array is a float64 mean
    return out


def vector(r) -> np.ndarray:
    """the kernel's 10 outputs of one image, float64"""
    return np.array([float(r[k]) for k in KEYS] + [float(r['ratio']), float(r['n'])])


U = 2.0 ** -24
SUMS = ('abs_diff', 'abs_rel', 'sq_rel', 'rmse', 'rmse_log')
_TERMS = {'abs_diff': lambda g, p: np.abs(g - p), 'abs_rel': lambda g, p: np.abs(g - p) / g, 'sq_rel': lambda g, p: (g - p) ** 2 / g,
          'rmse': lambda g, p: (g - p) ** 2, 'rmse_log': lambda g, p: (np.log(g) - np.log(p)) ** 2}


def bounds(r64, r32):
    """What a fp32 evaluation may differ from r64 by, from the float64 result and its fp32 twin alone (n > 0):
    SUMS: 4 x the mean of the twin's per-term errors |term32_i - term64_i| (on its own scaled, clamped prediction) + the final
          rounding of the result to fp32 (2 x 2^-24 relative); for the two roots the bound of the mean carried through sqrt;
    'ratio': 4 x the twin's error + the final rounding;
    'band': per threshold, the pixels whose float64 thresh lies within 1e-5 relative of it (where a fp32 decision may differ)."""
    tol = {}
    for k in SUMS:
        t_mean = 4 * float(np.abs(_TERMS[k](r32['gt'], r32['pred']).astype(np.float64) - _TERMS[k](r64['gt'], r64['pred'])).mean())
        ref = float(r64[k])
        if k.startswith('rmse'):        # the mean may move by t_mean either way: the larger of the two distances of the roots
            mean = ref * ref
            tol[k] = max(np.sqrt(mean + t_mean) - ref, ref - np.sqrt(max(mean - t_mean, 0.0))) + 2 * U * ref
        else:
            tol[k] = t_mean + 2 * U * ref
    tol['ratio'] = 4 * abs(float(r32['ratio']) - float(r64['ratio'])) + 2 * U * float(r64['ratio'])
    tol['band'] = {k: np.abs(r64['thresh'] / t - 1) <= 1e-5 for k, t in zip(('a1', 'a2', 'a3'), THRESHOLDS)}
    return tol
