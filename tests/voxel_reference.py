"""Restatement of the voxel-grid filter (include/clslam_hip.h, clslam_pcl_voxel_*) in float64 numpy with exact sums, and of the
reference's point-cloud writer (slam/utils.py:61-73 save_point_cloud with MeshlabInf.add_points / write, slam/meshlab.py:116-139,
159-206, and norm_range_01, :209-229) as the plain Python ``%`` loop it is.

The cell index is floor(double(c) / voxel_size): one IEEE division and one floor, which numpy performs with the same bits as the
kernel, so keys, order and counts are compared bitwise.  The per-cell sums are math.fsum: the correctly rounded sum of the members'
fp32 values.
"""
import math

import numpy as np

BIAS = 1 << 20


def cell_indices(points, voxel_size):
    """(M,6) float32 -> ((M,3) float64 indices ix, iy, iz (NaN where the row is dropped), (M,) bool kept).  A row with any
    non-finite value among its six is dropped."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 6)
    keep = np.isfinite(points).all(axis=1)
    with np.errstate(all='ignore'):
        idx = np.floor(points[:, :3].astype(np.float64) / np.float64(voxel_size))
    idx[~keep] = np.nan
    return idx, keep


def out_of_range(points, voxel_size):
    idx, keep = cell_indices(points, voxel_size)
    with np.errstate(invalid='ignore'):
        return int((keep & ((idx < -BIAS) | (idx > BIAS - 1)).any(axis=1)).sum())


def keys(points, voxel_size):
    """-> ((M,) uint64 keys, (M,) bool kept); the keys of dropped rows are 0"""
    idx, keep = cell_indices(points, voxel_size)
    assert out_of_range(points, voxel_size) == 0
    i = np.where(keep[:, None], idx, 0).astype(np.int64) + BIAS
    k = (i[:, 2].astype(np.uint64) << np.uint64(42)) | (i[:, 1].astype(np.uint64) << np.uint64(21)) | i[:, 0].astype(np.uint64)
    return np.where(keep, k, np.uint64(0)), keep


def voxel(points, voxel_size, min_points=1):
    """-> dict: 'keys' (V,) uint64 ascending, 'counts' (V,) int32, 'mean' (V,6) float64 = fsum of the members / n, 'abs_sum'
    (V,6) float64 = fsum of the members' absolute values (S of the bound), 'members': list of index arrays (ascending)"""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 6)
    k, keep = keys(points, voxel_size)
    cand = np.flatnonzero(keep)
    order = cand[np.argsort(k[cand], kind='stable')]
    uniq, first, cnt = np.unique(k[order], return_index=True, return_counts=True)
    out = {'keys': [], 'counts': [], 'mean': [], 'abs_sum': [], 'members': []}
    for u, a, n in zip(uniq, first, cnt):
        if n < min_points:
            continue
        m = order[a:a + n]
        vals = points[m].astype(np.float64)
        out['keys'].append(u)
        out['counts'].append(n)
        out['mean'].append([math.fsum(vals[:, c]) / float(n) for c in range(6)])
        out['abs_sum'].append([math.fsum(np.abs(vals[:, c])) for c in range(6)])
        out['members'].append(m)
    return {'keys': np.asarray(out['keys'], dtype=np.uint64), 'counts': np.asarray(out['counts'], dtype=np.int32),
            'mean': np.asarray(out['mean'], dtype=np.float64).reshape(-1, 6),
            'abs_sum': np.asarray(out['abs_sum'], dtype=np.float64).reshape(-1, 6), 'members': out['members']}


def value_bound(ref):
    """per value: one rounding to fp32 of the mean, plus any fixed fp64 summation order and the division"""
    return 2.0 ** -24 * np.abs(ref['mean']) + 2.0 ** -52 * ref['abs_sum']


def row_keys(rows, voxel_size):
    """the keys of output rows.  The mean of a cell lies in the cell only up to its rounding at a face, so the tests assert on
    these where the rows are exact: cells of one member and hand-made points."""
    return keys(rows, voxel_size)[0]


# ---- the writer ---------------------------------------------------------------------------------------------------------------
def norm_range_01(v):
    if np.all(np.isnan(v)):
        return v
    lo, hi = np.nanmin(v), np.nanmax(v)
    d = hi - lo
    if d < np.finfo(type(lo)).eps:
        d = 1
    return np.clip((v - lo) / d, 0, 1)


def obj_text(pcl):
    """the text MeshlabInf().add_points(pcl); .write(f) produces (false_color=False, no faces, identity global transformation)"""
    xyz = np.asarray(pcl).copy()
    if xyz.ndim == 1:
        xyz = xyz.reshape(1, -1)
    xyz = xyz[~np.any(np.isnan(xyz), axis=1), :]
    assert xyz.shape[1] == 6
    xyzrgb = np.vstack((np.zeros((0, 6)), xyz))
    xyzrgb[:, 3:] = norm_range_01(xyzrgb[:, 3:])
    xyzrgb[:, 3:] += 1 - np.max(xyzrgb[:, 3:])
    T = np.eye(4)
    out = ['# OBJ file\n']
    for i in range(xyzrgb.shape[0]):
        x = xyzrgb[i, :]
        x[:3] = T[:3, :3] @ x[:3] + T[:3, -1]
        out.append('v %.4f %.4f %.4f %.4f %.4f %.4f\n' % (x[0], x[1], x[2], x[3], x[4], x[5]))
    return ''.join(out)
