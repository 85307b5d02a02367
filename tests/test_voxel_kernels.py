"""ops.pcl_voxel_downsample (csrc/mapping.hip, clslam_pcl_voxel_*) against the float64 restatement of tests/voxel_reference.py, on
the CPU emulator and on gfx950.  Every figure is printed with -s.

Sizes.  The sort's tile is T = 1024 keys (the key kernel's block takes 1024 points too, the reduction 256 cells); a thread adds up
to 32 members of a cell itself and a wave takes a longer run, 64 members per step.

Bounds.  Membership, order and counts are exact: the cell index is one IEEE fp64 division and one floor on both sides.  Per value
|out - ref| <= 2^-24 |ref| + 2^-52 S, ref = the fsum mean, S = the fsum of the members' absolute values: the one rounding to fp32,
plus any fixed fp64 summation order and the division.  The output carries no keys; where a case's means are exact in fp32 (cell
faces, hand-made points) the keys of the output rows are compared as well.
"""
import functools

import numpy as np
import pytest
import torch

import mapping_reference as R
import voxel_reference as V
from clslam_hip import ops
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

T = 1024


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)


@functools.lru_cache(maxsize=None)
def _cloud(m, seed=0):
    """m points: the first two share a cell of 0.5 m and the third is alone far away; of the rest, half crowd into
    [-1.5, 1.5]^3 and half are spread over [-8, 8]^3 (mostly alone in their cells at 0.5 m).  Colours uniform."""
    rng = np.random.default_rng(1000 + 7 * m + seed)
    pts = np.empty((m, 6), np.float32)
    crowd = rng.random(m) < 0.5
    pts[:, :3] = np.where(crowd[:, None], rng.uniform(-1.5, 1.5, (m, 3)), rng.uniform(-8, 8, (m, 3)))
    pts[:, 3:] = rng.random((m, 3))
    head = np.array([[0.1, 0.1, 0.1], [0.2, 0.3, 0.4], [7.6, -7.7, 7.8]], np.float32)
    pts[:min(m, 3), :3] = head[:min(m, 3)]
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _ref(m, vs, min_points=1, seed=0):
    return V.voxel(_cloud(m, seed), vs, min_points)


def _run(dev, pts, vs, **kw):
    kw = {k: (_t(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    rows, counts, info = ops.pcl_voxel_downsample(_t(np.asarray(pts, np.float32).reshape(-1, 6), dev), vs, return_info=True, **kw)
    assert rows.dtype == torch.float32 and counts.dtype == torch.int32 and rows.device.type == dev.type == counts.device.type
    assert rows.shape == (counts.shape[0], 6)
    return rows.cpu().numpy(), counts.cpu().numpy(), info


def _has_work(ref):
    """the reference itself, before the kernel: a pass-through would not pass"""
    assert (ref['counts'] >= 2).any() and (ref['counts'] == 1).any(), np.bincount(ref['counts'])[:4]


def _check(backend, case, rows, counts, ref):
    assert np.array_equal(counts, ref['counts']), (case, len(counts), len(ref['counts']))
    err = np.abs(rows.astype(np.float64) - ref['mean'])
    bound = V.value_bound(ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'[voxel {backend}] {case}: {len(counts)} cells, largest {int(counts.max()) if len(counts) else 0}, '
          f'single {int((counts == 1).sum())}, max err / bound {ratio:.3f}')
    assert (err <= bound).all(), case


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('m', [0, 1, T - 1, T, T + 1, 3 * T + 517])
def test_sizes(backend, m):
    dev = use_backend(backend)
    ref = _ref(m, 0.5)
    if m >= 3:
        _has_work(ref)
    rows, counts, info = _run(dev, _cloud(m), 0.5)
    assert rows.shape == (len(ref['counts']), 6) and info['cells'] == len(counts) and info['dropped'] == 0
    _check(backend, f'M = {m}', rows, counts, ref)
    if m == 1:
        assert np.array_equal(_bits(rows[0]), _bits(_cloud(1)[0])) and counts.tolist() == [1]    # the mean of one is itself


@pytest.mark.parametrize('backend', BACKENDS)
def test_runs_across_tiles_and_long_runs(backend):
    """in sorted order: 1000 cells of one point, a cell of 100 (positions 1000 .. 1099: across the tile boundary at 1024), cells of
    32, 33, 64 and 65 (the last the thread sums itself, the first a wave takes, one and two wave steps), one of 700 (more than the
    256 threads of a block), then 300 single cells; the input is shuffled"""
    dev = use_backend(backend)
    rng = np.random.default_rng(5)
    cells = [(x, 0, 0, 1) for x in range(1000)] + [(0, 1, 0, 100), (1, 1, 0, 32), (2, 1, 0, 33), (3, 1, 0, 64), (4, 1, 0, 65),
                                                      (5, 1, 0, 700)] + [(x, 2, 0, 1) for x in range(300)]
    pts = np.concatenate([np.concatenate([(np.array([x, y, z]) + rng.random((n, 3))) * 0.25, rng.random((n, 3))], axis=1)
                          for x, y, z, n in cells]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    ref = V.voxel(pts, 0.25)
    assert ref['counts'].tolist() == [n for *_, n in cells]                                     # the reference first
    _has_work(ref)
    rows, counts, _ = _run(dev, pts, 0.25)
    _check(backend, 'runs', rows, counts, ref)


# ---- key arithmetic -----------------------------------------------------------------------------------------------------------
def _row(x, y, z, c=0.5):
    return [x, y, z, c, c / 2, c / 4]


@pytest.mark.parametrize('backend', BACKENDS)
def test_floor_and_faces(backend):
    dev = use_backend(backend)
    # floor, not truncation: -0.05 / 0.1 is cell -1, with -0.01; 0.05 is cell 0
    pts = np.asarray([_row(0.05, 0.05, 0.05), _row(-0.05, 0.05, 0.05), _row(-0.01, 0.05, 0.05), _row(-0.15, -0.15, -0.15)], np.float32)
    ref = V.voxel(pts, 0.1)
    assert ref['counts'].tolist() == [1, 2, 1] and [m.tolist() for m in ref['members']] == [[3], [1, 2], [0]]
    rows, counts, _ = _run(dev, pts, 0.1)
    _check(backend, 'negative coordinates', rows, counts, ref)
    # exactly on faces with voxel_size 0.25 (the division is exact): 0.5 opens cell 2, the fp32 number below it closes cell 1;
    # -0.25 opens cell -1, -0.0 and 0.0 share cell 0
    below = np.nextafter(np.float32(0.5), np.float32(0))
    xs = [0.5, below, 0.25, -0.25, np.nextafter(np.float32(-0.25), np.float32(-1)), -0.0, 0.0, 0.75 - 2.0 ** -20]
    pts = np.asarray([_row(x, 0.125, 0.125, 0.25 + 0.0625 * i) for i, x in enumerate(xs)], np.float32)
    ref = V.voxel(pts, 0.25)
    want = [-2, -1, 0, 1, 2]
    assert ((ref['keys'] & np.uint64((1 << 21) - 1)).astype(np.int64) - V.BIAS).tolist() == want
    assert ref['counts'].tolist() == [1, 1, 2, 2, 2]
    rows, counts, _ = _run(dev, pts, 0.25)
    _check(backend, 'faces', rows, counts, ref)
    # keys that differ in one index only, from each axis: x orders first, then y, then z
    pts = np.asarray([_row(0.5, 0.5, 1.5, 1), _row(0.5, 1.5, 0.5, 2), _row(1.5, 0.5, 0.5, 3), _row(0.5, 0.5, 0.5, 4),
                      _row(0.5, 0.5, -0.5, 5), _row(0.5, -0.5, 0.5, 6), _row(-0.5, 0.5, 0.5, 7)], np.float32)
    ref = V.voxel(pts, 1.0)
    rows, counts, _ = _run(dev, pts, 1.0)
    _check(backend, 'one axis', rows, counts, ref)
    assert rows[:, 3].tolist() == [5, 6, 7, 4, 3, 2, 1]                                         # single members: exact rows
    assert np.array_equal(V.row_keys(rows, 1.0), ref['keys'])


@pytest.mark.parametrize('backend', BACKENDS)
def test_index_range(backend):
    """indices -2^20 and 2^20 - 1 are cells like any other; one beyond either end, on any axis, raises"""
    dev = use_backend(backend)
    lo, hi = -float(1 << 20), float((1 << 20) - 1) + 0.5
    ends = np.asarray([_row(lo, 0.5, 0.5, 1), _row(hi, 0.5, 0.5, 2), _row(0.5, lo, 0.5, 3), _row(0.5, hi, 0.5, 4),
                       _row(0.5, 0.5, lo, 5), _row(0.5, 0.5, hi, 6), _row(hi, hi, hi, 7), _row(lo, lo, lo, 8), _row(lo, lo, lo, 9)],
                      np.float32)
    assert ends[1, 0] == hi                                                                     # exact in fp32
    ref = V.voxel(ends, 1.0)
    assert len(ref['counts']) == 8 and ref['keys'][0] == 0 and ref['keys'][-1] == np.uint64((1 << 63) - 1)
    rows, counts, _ = _run(dev, ends, 1.0)
    _check(backend, 'ends of the range', rows, counts, ref)
    assert np.array_equal(V.row_keys(rows[counts == 1], 1.0), ref['keys'][ref['counts'] == 1])
    for axis in range(3):
        for c in (lo - 0.5, float(1 << 20)):
            bad = np.asarray([_row(0.5, 0.5, 0.5), _row(0.5, 0.5, 0.5)], np.float32)
            bad[1, axis] = c
            assert V.out_of_range(bad, 1.0) == 1
            with pytest.raises(ClslamError, match='2\\^20'):
                _run(dev, bad, 1.0)
    with pytest.raises(ClslamError):
        _run(dev, _cloud(100), 1e-30)                                                           # every index overflows


def _passes(ref_keys):
    varies = np.bitwise_or.reduce(ref_keys) & np.bitwise_or.reduce(~ref_keys)
    return sum(1 for p in range(16) if (int(varies) >> (4 * p)) & 15)


@pytest.mark.parametrize('backend', BACKENDS)
def test_skipped_passes(backend):
    """cells 0 .. 15 on every axis: the keys differ in bits 0-3, 21-24 and 42-45, five digits of 4 bits, so eleven passes are
    skipped; the same points moved by -8 cells straddle zero, every bit below 63 varies and all sixteen passes run.  The move is
    exact (coordinates in 64ths) and keeps the order of the cells: the counts are the same sequence."""
    dev = use_backend(backend)
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.integers(0, 16 * 64, (2500, 3)) / 64.0, rng.random((2500, 3))], axis=1).astype(np.float32)
    moved = pts.copy()
    moved[:, :3] -= 8.0
    ref, ref_moved = V.voxel(pts, 1.0), V.voxel(moved, 1.0)
    _has_work(ref)
    assert _passes(ref['keys']) == 5 and _passes(ref_moved['keys']) == 16
    assert np.array_equal(ref['counts'], ref_moved['counts'])
    rows, counts, info = _run(dev, pts, 1.0)
    rows_m, counts_m, info_m = _run(dev, moved, 1.0)
    print(f'[voxel {backend}] radix passes: {info["passes"]} and {info_m["passes"]} of 16')
    assert info['passes'] == 5 and info_m['passes'] == 16
    _check(backend, 'five passes', rows, counts, ref)
    _check(backend, 'sixteen passes', rows_m, counts_m, ref_moved)
    assert np.array_equal(counts, counts_m) and np.array_equal(_bits(rows[:, 3:]), _bits(rows_m[:, 3:]))
    one = np.repeat(pts[:1], 300, axis=0)                                                       # one cell: nothing to sort
    rows, counts, info = _run(dev, one, 1.0)
    assert info['passes'] == 0 and counts.tolist() == [300] and np.array_equal(_bits(rows[0]), _bits(one[0]))


# ---- determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_determinism(backend):
    dev = use_backend(backend)
    m = 3 * T + 517
    pts, ref = _cloud(m), _ref(m, 0.5)
    a = _run(dev, pts, 0.5)
    b = _run(dev, pts, 0.5)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    shuffled = pts[np.random.default_rng(3).permutation(m)]                                     # the members of every cell reordered
    c = _run(dev, shuffled, 0.5)
    assert np.array_equal(c[1], a[1])
    _check(backend, 'shuffled', c[0], c[1], ref)                                                # the same cells, sums in another order
    assert np.array_equal(_bits(c[0][c[1] == 1]), _bits(a[0][a[1] == 1]))


# ---- fused poses --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames():
    s = R.scene(24, 40, 3, seed=24 * 40 + 3)
    clouds = [R.backproject(s['depth'][f, 0], s['inv_K'][f], s['image'][f])['points'].astype(np.float32) for f in range(3)]
    sizes = [len(clouds[0]), 0, len(clouds[1]), len(clouds[2])]                                # an empty segment
    poses = np.stack([s['poses'][0], s['poses'][1], s['poses'][1], np.full((4, 4), np.nan)])   # and one without a pose
    return np.concatenate(clouds), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), poses


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('vs', [0.5, 2.0])
def test_fused_poses(backend, vs):
    dev = use_backend(backend)
    pts, offsets, poses = _frames()
    world = ops.pcl_transform(_t(pts, dev), offsets, _t(poses, dev))
    ref = V.voxel(world.cpu().numpy(), vs)
    _has_work(ref)
    assert sum(len(m) for m in ref['members']) == offsets[3]                                    # the NaN-posed frame is gone
    two = ops.pcl_voxel_downsample(world, vs)
    _check(backend, f'24x40x3 at {vs}', two[0].cpu().numpy(), two[1].cpu().numpy(), ref)
    rows, counts, info = _run(dev, pts, vs, offsets=offsets, poses=poses)
    assert info['dropped'] == offsets[4] - offsets[3]
    assert np.array_equal(_bits(rows), _bits(two[0].cpu().numpy())) and np.array_equal(counts, two[1].cpu().numpy())


# ---- dropped rows, min_points, arguments --------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_dropped_rows(backend):
    dev = use_backend(backend)
    m = T + 1
    pts = _cloud(m).copy()
    hit = [(0, 0, np.nan), (1, 5, np.nan), (2, 2, np.inf), (700, 4, -np.inf), (T - 1, 1, np.nan), (T, 3, np.inf)]
    for r, c, v in hit:
        pts[r, c] = v
    clean = np.delete(pts, [r for r, _, _ in hit], axis=0)
    ref = V.voxel(pts, 0.5)
    assert np.array_equal(ref['counts'], V.voxel(clean, 0.5)['counts']) and ref['counts'].sum() == m - len(hit)
    _has_work(ref)
    rows, counts, info = _run(dev, pts, 0.5)
    assert info['dropped'] == len(hit) and np.isfinite(rows).all()
    _check(backend, 'dropped', rows, counts, ref)
    rows, counts, info = _run(dev, np.full((5, 6), np.nan, np.float32), 0.5)                    # nothing left
    assert rows.shape == (0, 6) and counts.shape == (0,) and info['dropped'] == 5 and info['passes'] == 0


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('min_points', [2, 3])
def test_min_points(backend, min_points):
    dev = use_backend(backend)
    m = 3 * T + 517
    every, ref = _ref(m, 0.5), _ref(m, 0.5, min_points)
    _has_work(every)
    assert 0 < len(ref['counts']) < len(every['counts']) and ref['counts'].min() == min_points
    rows, counts, _ = _run(dev, _cloud(m), 0.5, min_points=min_points)
    _check(backend, f'min_points {min_points}', rows, counts, ref)
    all_rows, all_counts, _ = _run(dev, _cloud(m), 0.5)
    assert np.array_equal(_bits(rows), _bits(all_rows[all_counts >= min_points]))               # the same rows, fewer of them


@pytest.mark.parametrize('backend', BACKENDS)
def test_argument_checks(backend):
    dev = use_backend(backend)
    p = _t(_cloud(100), dev)
    pts, offsets, poses = _frames()
    for bad in (lambda: ops.pcl_voxel_downsample(p, 0.0), lambda: ops.pcl_voxel_downsample(p, -1.0),
                lambda: ops.pcl_voxel_downsample(p, float('nan')), lambda: ops.pcl_voxel_downsample(p, float('inf')),
                lambda: ops.pcl_voxel_downsample(p, 0.5, min_points=0), lambda: ops.pcl_voxel_downsample(p[:, :5], 0.5),
                lambda: ops.pcl_voxel_downsample(p.double(), 0.5), lambda: ops.pcl_voxel_downsample(p, 0.5, poses=_t(poses, dev)),
                lambda: ops.pcl_voxel_downsample(_t(pts, dev), 0.5, offsets=offsets[:-1], poses=_t(poses, dev))):
        with pytest.raises(ClslamError):
            bad()
    rows, counts = ops.pcl_voxel_downsample(p[:0], 0.5)                                         # M = 0: no launch
    assert rows.shape == (0, 6) and counts.shape == (0,) and counts.dtype == torch.int32
