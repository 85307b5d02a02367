"""Restatement of the voxel-grid filter (include/clslam_hip.h, clslam_pcl_voxel_*) in float64 numpy with exact sums, and of the
reference's point-cloud writer (slam/utils.py:61-73 save_point_cloud with MeshlabInf.add_points / write, slam/meshlab.py:116-139,
159-206, and norm_range_01, :209-229) as the plain Python ``%`` loop it is.

The cell index is floor(double(c) / voxel_size): one IEEE division and one floor, which numpy performs with the same bits as the
kernel, so keys, order and counts are compared bitwise.  The per-cell sums are math.fsum: the correctly rounded sum of the members'
fp32 values.  For clouds of 10^5 .. 10^7 points there are lattice clouds, on which every sum is exact, and voxel_exact.
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


# ---- exact clouds -------------------------------------------------------------------------------------------------------------
# On a lattice cloud (coordinates integer multiples of 2^-6 with |c| <= 16, colours integer multiples of 2^-8 in [0, 1]) and a
# voxel_size that is a power of two, the division and the floor are exact and every fp64 partial sum of up to 2^32 members is an
# integer multiple of 2^-8 below 2^36 (2^44 units, under 2^53): exact, in any order.  float32(sum / n) is then the one value a
# correct filter returns, and the rows are compared bitwise at sizes math.fsum could not reach.
def lattice_cloud(m, seed=0, lo=(-512, -512, -512), hi=(512, 512, 512), top=None):
    """(m,6) float32: coordinates drawn uniformly from the integers [lo, hi) (either may be an array that broadcasts to (m,3)),
    times 2^-6; colours from the integers [0, 256], times 2^-8.  One integers() call per array; rows are independent, so the
    cloud is shuffled as it stands.  top = (n, voxel_size): the cell that ends at max(hi) on every axis -- the largest key of
    the cloud, the end of the sorted order -- gets exactly n members, at random rows."""
    rng = np.random.default_rng(seed)
    q = rng.integers(lo, hi, (m, 3), dtype=np.int16)
    c = rng.integers(0, 257, (m, 3), dtype=np.int16)
    if top is not None:
        n, vs = top
        end = np.broadcast_to(np.asarray(hi), (m, 3)).max(axis=0)
        side = int(round(vs * 64))
        assert side >= 1 and side == vs * 64 and n <= side ** 3 and (end % side == 0).all()
        inside = (q >= end - side).all(axis=1)
        q[inside, 0] -= side                                                           # the neighbouring cell
        rows = rng.choice(m, n, replace=False)
        q[rows] = end - 1 - np.stack(np.unravel_index(rng.choice(side ** 3, n, replace=False), (side,) * 3), axis=1)
    pts = np.empty((m, 6), np.float32)
    pts[:, :3] = q
    pts[:, 3:] = c
    pts[:, :3] *= np.float32(2.0 ** -6)
    pts[:, 3:] *= np.float32(2.0 ** -8)
    return pts


def is_lattice(points, voxel_size):
    """the premise of voxel_exact, on the finite rows: multiples of 2^-6 within [-16, 16], of 2^-8 within [0, 1], and a
    voxel_size that is a power of two no finer than the lattice"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 6)
    p = p[np.isfinite(p).all(axis=1)]
    mant, _ = math.frexp(voxel_size)
    return bool(mant == 0.5 and voxel_size >= 2.0 ** -6 and (p[:, :3] * 64 == np.rint(p[:, :3] * 64)).all() and
                (np.abs(p[:, :3]) <= 16).all() and (p[:, 3:] * 256 == np.rint(p[:, 3:] * 256)).all() and
                (p[:, 3:] >= 0).all() and (p[:, 3:] <= 1).all())


def _compact(k):
    """the cells numbered inside the box the keys span, z-major as the keys are: (ids, size of the box); ids order as the keys do"""
    mask = np.uint64((1 << 21) - 1)
    ids, size = np.zeros(k.shape, np.int64), 1
    for shift in (42, 21, 0):
        i = ((k >> np.uint64(shift)) & mask).astype(np.int64)
        lo, span = int(i.min()), int(i.max()) - int(i.min()) + 1
        ids = ids * span + (i - lo)
        size *= span
    return ids, size


def voxel_exact(points, voxel_size, min_points=1, method=None):
    """voxel() for lattice clouds, vectorised.  -> dict: 'keys' (V,) uint64 ascending, 'counts' (V,) int32, 'rows' (V,6) float32 =
    float32(sum / n) with exact fp64 sums (+0.0 for a zero sum: the filter adds to +0.0), of the cells with at least min_points
    members; 'all_keys' / 'all_counts': every cell, the runs of the sorted order; 'dropped': the rows with a non-finite value.
    The sums are formed twice, over each cell's members in ascending and in descending row order, and asserted bit-equal: if they
    were not exact, the order would show.  method 'sort': a stable argsort of the keys and np.add.reduceat; 'bincount': np.bincount
    over the cell's number inside the box the cloud spans (at most 2^22 cells); None: 'sort' up to 2^21 points."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 6)
    assert is_lattice(points, voxel_size)
    k, keep = keys(points, voxel_size)
    cand = np.flatnonzero(keep)
    dropped = len(points) - len(cand)
    if len(cand) == 0:
        none = np.zeros(0, np.uint64), np.zeros(0, np.int32)
        return {'keys': none[0], 'counts': none[1], 'rows': np.zeros((0, 6), np.float32), 'all_keys': none[0],
                'all_counts': none[1], 'dropped': dropped}
    kc = k[cand]
    assert len(cand) <= 1 << 32                                                        # sums below 2^32 * 2^12 units of 2^-8
    if method is None:
        method = 'sort' if len(cand) <= 1 << 21 else 'bincount'
    if method == 'bincount':
        ids, size = _compact(kc)
        assert size <= 1 << 22, size
        cnt = np.bincount(ids, minlength=size)
        fwd = np.stack([np.bincount(ids, weights=points[cand, c], minlength=size) for c in range(6)], axis=1)
        rev = np.stack([np.bincount(ids[::-1], weights=points[cand[::-1], c], minlength=size) for c in range(6)], axis=1)
        occupied = np.flatnonzero(cnt)
        rep = np.zeros(size, np.int64)
        rep[ids] = np.arange(len(ids))                                                 # any member: they share the key
        uniq, cnt, fwd, rev = kc[rep[occupied]], cnt[occupied], fwd[occupied], rev[occupied]
    else:
        order = np.argsort(kc, kind='stable')
        back = (len(kc) - 1 - np.argsort(kc[::-1], kind='stable'))                     # the same cells, members descending
        uniq, first, cnt = np.unique(kc[order], return_index=True, return_counts=True)
        vals = points[cand].astype(np.float64)
        fwd, rev = np.add.reduceat(vals[order], first, axis=0), np.add.reduceat(vals[back], first, axis=0)
    fwd, rev = fwd + 0.0, rev + 0.0
    assert np.array_equal(fwd.view(np.uint64), rev.view(np.uint64)), 'the sums depend on the order: not exact'
    assert (np.diff(uniq.astype(np.uint64)) > 0).all() if len(uniq) > 1 else True
    rows = (fwd / cnt[:, None].astype(np.float64)).astype(np.float32)
    sel = cnt >= min_points
    return {'keys': uniq[sel], 'counts': cnt[sel].astype(np.int32), 'rows': rows[sel], 'all_keys': uniq,
            'all_counts': cnt.astype(np.int64),
            'dropped': dropped}


def radix_trace(points, voxel_size):
    """what the sort of include/clslam_hip.h does to these rows, pass by pass: [(pass, digits)] for every pass that runs, digits
    (M,) uint8 in the order of the keys when the pass starts.  A pass runs if its 4 bits vary among the kept rows' keys; the last
    one also if rows are dropped (key 2^63), to move them behind the cells."""
    k, keep = keys(points, voxel_size)
    k = np.where(keep, k, np.uint64(1) << np.uint64(63))
    if not keep.any():
        return []
    varies = int(np.bitwise_or.reduce(k[keep]) & np.bitwise_or.reduce(~k[keep]))
    out = []
    for p in range(16):
        if not ((varies >> (4 * p)) & 15 or (p == 15 and not keep.all())):
            continue
        d = ((k >> np.uint64(4 * p)) & np.uint64(15)).astype(np.uint8)
        out.append((p, d))
        k = k[np.argsort(d, kind='stable')]
    return out


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
