"""numpy restatements of the frame-panel rules of include/clslam_hip.h "Frame panels" (csrc/viz.hip), for the tests.

The colour tables come from tests/golden/viz_colormap.npz (recorded from matplotlib by tests/golden/make_viz_golden.py)."""
import functools
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'viz_colormap.npz'
GT_COLOUR, PRED_COLOUR = (31, 119, 180), (255, 127, 14)           # matplotlib's C0 and C1
PIX_CLAMP = 2 ** 30


@functools.lru_cache(maxsize=None)
def table(cmap: str) -> np.ndarray:
    """(256,3) uint8"""
    with np.load(GOLDEN) as z:
        return z[cmap].copy()


def order_key(x: np.ndarray) -> np.ndarray:
    """the monotone uint32 key of float32 values: unsigned order of the keys = order of the values, -0 below +0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def depth_range(plane, q: float = 95.0):
    """-> (vmin, vmax, m): the project's rule.  Only finite values; order statistics by key; the percentile interpolated in
    float64 and rounded once to float32."""
    x = np.asarray(plane, np.float32).ravel()
    fin = x[np.isfinite(x)]
    m = fin.size
    if m == 0:
        return np.float32(np.nan), np.float32(np.nan), 0
    a = fin[np.argsort(order_key(fin), kind='stable')]
    pos = float(q) / 100 * (m - 1)
    k = int(np.floor(pos))
    g = pos - k
    lo, hi = np.float64(a[k]), np.float64(a[min(k + 1, m - 1)])
    return a[0], np.float32(lo + (hi - lo) * g), m


def colorize(plane, vmin, vmax, cmap: str = 'magma_r') -> np.ndarray:
    """(…,H,W) float32 -> (…,H,W,3) uint8, matplotlib's arithmetic (include/clslam_hip.h, CMAP)"""
    x = np.asarray(plane, np.float32)
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    lut = table(cmap)
    with np.errstate(all='ignore'):
        if vmin == vmax:
            idx = np.zeros(x.shape, np.int64)
            bad = np.isnan(x)
        else:
            r = (x.astype(np.float64) - np.float64(vmin)).astype(np.float32)           # Normalize: float64 scalars, stored as float32
            xa = (r.astype(np.float64) / (np.float64(vmax) - np.float64(vmin))).astype(np.float32) * np.float32(256)
            bad = np.isnan(xa)
            idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.trunc(np.where(bad | np.isinf(xa), 0, xa)))).astype(np.int64)
    out = lut[np.clip(idx, 0, 255)]
    out[bad] = 0
    return out


def to_bytes(x) -> np.ndarray:
    """trunc(clamp(x, 0, 1) * 255 + 0.5) in x's own precision, NaN -> 0; uint8 unchanged"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.copy()
    t = x.dtype.type
    with np.errstate(invalid='ignore'):
        c = np.where(x > 0, np.where(x > 1, t(1), x), t(0)).astype(x.dtype)
    return (c * t(255) + t(0.5)).astype(x.dtype).astype(np.uint8)


def image_row(image, chw: bool = False) -> np.ndarray:
    """(3,H,W) with chw else (H,W,3) -> (H,W,3) uint8"""
    b = to_bytes(image)
    return np.ascontiguousarray(np.moveaxis(b, 0, -1)) if chw else b


def _floordiv(a: int, b: int) -> int:
    return a // b                                      # Python's integer division floors


def _pixel(t: float) -> int:
    return int(min(max(np.floor(t), -PIX_CLAMP), PIX_CLAMP))


def segment_pixels(u0: int, v0: int, u1: int, v1: int, h: int, w: int, brute: bool = False):
    """the pixels of the segment rule that lie inside the h x w row, as a set of (u, v).  Python integers throughout.  Without
    `brute` only the k whose MAJOR coordinate (start +- k, exactly) is inside the row are visited."""
    du, dv = u1 - u0, v1 - v0
    n = max(abs(du), abs(dv))
    if n == 0:
        return {(u0, v0)} if 0 <= u0 < w and 0 <= v0 < h else set()
    ks = range(n + 1)
    if not brute:
        a0, d, size = (u0, du, w) if abs(du) >= abs(dv) else (v0, dv, h)
        lo, hi = (-a0, size - 1 - a0) if d > 0 else (a0 - (size - 1), a0)
        ks = range(max(lo, 0), min(hi, n) + 1)
    out = set()
    for k in ks:
        u, v = u0 + _floordiv(2 * k * du + n, 2 * n), v0 + _floordiv(2 * k * dv + n, 2 * n)
        if 0 <= u < w and 0 <= v < h:
            out.add((u, v))
    return out


def polyline_pixels(xz, h: int, w: int, xlim, ylim, brute: bool = False):
    xz = np.zeros((0, 2)) if xz is None else np.asarray(xz, np.float64).reshape(-1, 2)
    x0, xs, y1, ys = float(xlim[0]), float(xlim[1]) - float(xlim[0]), float(ylim[1]), float(ylim[1]) - float(ylim[0])
    out = set()
    nv = xz.shape[0]
    for s in range(1 if nv == 1 else max(nv - 1, 0)):
        a, b = xz[s], xz[s if nv == 1 else s + 1]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        with np.errstate(over='ignore'):
            p = [_pixel((a[0] - x0) / xs * w), _pixel((y1 - a[1]) / ys * h), _pixel((b[0] - x0) / xs * w), _pixel((y1 - b[1]) / ys * h)]
        out |= segment_pixels(*p, h, w, brute)
    return out


def trajectory_row(gt_xz, pred_xz, shape, xlim=(-400, 15), ylim=(-60, 160), brute: bool = False) -> np.ndarray:
    h, w = shape
    out = np.full((h, w, 3), 255, np.uint8)
    for line, colour in ((gt_xz, GT_COLOUR), (pred_xz, PRED_COLOUR)):          # pred over gt
        for u, v in polyline_pixels(line, h, w, xlim, ylim, brute):
            out[v, u] = colour
    return out


def frame_panel(image, depth, image_pcl=None, gt_xz=None, pred_xz=None, cmap='magma_r', q=95.0, xlim=(-400, 15), ylim=(-60, 160)):
    """-> (panel (rows*H, W, 3) uint8, vmax): image (3,H,W) float32 or (H,W,3); depth (H,W)"""
    depth = np.asarray(depth, np.float32)
    depth = depth.reshape(depth.shape[-2:])
    image = np.asarray(image)
    vmin, vmax, _ = depth_range(depth, q)
    rows = [image_row(image, chw=image.shape[0] == 3 and image.shape[-1] != 3), colorize(depth, vmin, vmax, cmap)]
    if image_pcl is not None:
        rows.append(image_row(np.asarray(image_pcl)))
    if gt_xz is not None or pred_xz is not None:
        rows.append(trajectory_row(gt_xz, pred_xz, depth.shape, xlim, ylim))
    return np.concatenate(rows, 0), vmax
