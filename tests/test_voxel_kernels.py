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


# ---- the sizes at which the scans go multi-level --------------------------------------------------------------------------------
# Exact clouds (voxel_reference.lattice_cloud): rows and counts are compared bitwise with voxel_exact, the keys of the rows of
# one-member cells with the reference's.  Every condition a case is there for is asserted on the reference before the kernel runs.
#
# Measured, seconds per case, CPU emulator | MI355X (the whole test: cloud, reference, conditions, kernel, comparison):
#   test_scan_levels        65,536: 1.4 | 0.32     65,537: 0.3 | 0.03     262,147: 0.8 | 0.13     1,048,577: (4.5) | 0.56
#   test_scan_levels_dropped_rows 0.3 | 0.04    test_scan_levels_min_points 0.6 | 0.05 each    test_scan_levels_fused_poses 0.6 | 0.04
#   test_determinism_multi_level  1.2 | 0.11       test_scan_sums_two_per_thread  (30) | 6.4, nearly all of it on the host
# (65,536 also runs the fsum reference on a prefix.)  The slowest emulator case of this file before these took 0.4 s
# (test_determinism); 262,147 points take twice that, so no row was moved: every row is on the backends the table of sizes names.
# The figures in brackets are runs outside the suite: 1,048,577 and 16,777,217 points are device-only.
LEVEL_CASES = [pytest.param(m, b, id=f'{m}-{b}', marks=[pytest.mark.gpu] if b == 'hip' else [])
               for m, bs in ((65536, ('emu', 'hip')), (65537, ('emu', 'hip')), (262147, ('emu', 'hip')), (1048577, ('hip',)))
               for b in bs]


@functools.lru_cache(maxsize=None)
def _lattice(m, **kw):
    """x in [-2, 8), y and z in [-8, 8): every axis straddles the bias, so every key bit below 63 varies.  x is off centre for
    pass 5 (bit 20 of ix + 2^20, then iy's lowest three): it finds the keys ordered by ix's low 20 bits, the cells from 0 on in
    front of those below 0, and digit 15 needs ix >= 0 -- with a fifth of the rows below 0 the others reach tile 49 of 65."""
    pts = V.lattice_cloud(m, seed=m, **{'lo': (-128, -512, -512), **kw})
    pts.setflags(write=False)
    return pts


def _scan_conditions(pts, vs):
    """-> the number of radix passes that run.  Asserted for each of them, on the keys in the order that pass finds them (the
    scatter reads gbase = hist[g] + sums[g / 1024] with g = digit * tiles + tile): where the histogram fills more than one scan
    block, digit 15 occurs in a tile with 15 * tiles + tile >= 1024 and the sums entry it reads is not zero -- a second level
    that returned zeros, or sums[0], would misplace those keys.  Two passes cannot hold digit 15 in any cloud within 2^19 cells of
    the origin: pass 15 (bits 60-63: bit 63 is clear in every cell key) and pass 10 (bits 40-43 start with bits 19 and 20 of
    iy + 2^20, which are 01 below the bias and 10 from it on).  There the same is asserted of the largest digit that occurs
    instead, if its entries lie beyond the first scan block at all."""
    m = len(pts)
    tiles = -(-m // T)
    n_sums = -(-16 * tiles // T)
    trace = V.radix_trace(pts, vs)
    tile = np.arange(m) // T
    for p, d in trace:
        if n_sums == 1:
            continue
        g = d.astype(np.int64) * tiles + tile
        top = 15 if p not in (10, 15) else int(d.max())
        late = (d == top) & (g >= T)
        if top == 15 or top * tiles + tiles - 1 >= T:
            assert late.any(), (p, top)
            assert g.min() < (g[late] // T).min() * T, p                                   # keys in front of that scan block
    return len(trace)


def _check_exact(backend, case, out, ref, vs, passes):
    rows, counts, info = out
    print(f'[voxel {backend}] {case}: {len(ref["counts"])} cells, largest {int(ref["counts"].max())}, single '
          f'{int((ref["counts"] == 1).sum())}, dropped {ref["dropped"]}, passes {passes}; kernel: {info}')
    assert info['cells'] == len(ref['counts']) == len(counts), case
    assert info['dropped'] == ref['dropped'] and info['passes'] == passes, case
    assert np.array_equal(counts, ref['counts']), case
    assert np.array_equal(_bits(rows), _bits(ref['rows'])), case
    one = ref['counts'] == 1
    assert np.array_equal(V.row_keys(rows[one], vs), ref['keys'][one]), case                # exact rows lie in their cells


def _every_cell(ref):
    return {'counts': ref['all_counts']}


@pytest.mark.parametrize('m,backend', LEVEL_CASES)
def test_scan_levels(m, backend):
    """pcl_voxel_scatter_kernel's `gbase[t] = hist[g] + sums[g / kVxTile]`, pcl_voxel_scan_kernel as more than one block and
    pcl_voxel_scan_sums_kernel over more than one value; at 1,048,577 also pcl_voxel_heads_kernel's `sums[blockIdx.x / kVxTile]`.
      65,536     n_hist == 1024: one scan block, exactly full; every tile full (the 16-byte loads in every tile)
      65,537     n_sums == 2; the last tile holds one key; the second scan block holds 16 live entries
      262,147    n_sums == 5, 257 tiles, a partial last tile
      1,048,577  1025 tiles: head_sums == 2, the heads kernel reads sums[1]; n_sums == 17.  Only tile 1024 reads sums[1], and it
                 holds one key, the largest: that cell is given exactly one member, so position 1024 * 1024 is a run head and
                 the heads before it make sums[1] non-zero (both asserted on the reference)
    The cloud is _lattice's: x in [-2, 8) (off centre for pass 5, see there), y and z in [-8, 8), so the cell indices straddle
    the 2^20 bias on every axis, every key bit below 63 varies and all 16 passes run.  Times: the table above LEVEL_CASES."""
    dev = use_backend(backend)
    vs = 0.25
    pts = _lattice(m, top=(1, vs)) if m > T * T else _lattice(m)
    tiles = -(-m // T)
    n_sums, head_sums = -(-16 * tiles // T), -(-tiles // T)
    assert (n_sums, head_sums, m % T) == {65536: (1, 1, 0), 65537: (2, 1, 1), 262147: (5, 1, 3), 1048577: (17, 2, 1)}[m]
    ref = V.voxel_exact(pts, vs)
    _has_work(ref)
    passes = _scan_conditions(pts, vs)
    assert passes == 16 == _passes(ref['keys'])
    if head_sums > 1:                                # a head whose block reads sums[1], and heads in front of it
        start = np.cumsum(ref['all_counts']) - ref['all_counts']
        assert (start >= T * T).any() and (start < T * T).any() and start[-1] == m - 1
    if m == 65536:                                   # voxel_exact against the fsum reference, where that one is affordable
        few, slow = V.voxel_exact(pts[:4096], vs), V.voxel(pts[:4096], vs)
        _has_work(few)
        assert np.array_equal(few['keys'], slow['keys']) and np.array_equal(few['counts'], slow['counts'])
        assert np.array_equal(_bits(few['rows']), _bits(slow['mean'].astype(np.float32)))
        other = V.voxel_exact(pts, vs, method='bincount')                                # and its two forms against each other
        assert all(np.array_equal(ref[k], other[k]) for k in ('keys', 'counts', 'all_counts'))
        assert np.array_equal(_bits(ref['rows']), _bits(other['rows']))
    _check_exact(backend, f'M = {m}', _run(dev, pts, vs), ref, vs, passes)


def _dropped_cloud(m):
    """z below 0 only: without the dropped rows the last pass would not run.  About 1 % of the rows get a NaN or an infinity in
    one of their six values, among them the last two rows: the last tile of the input is nothing but a dropped row."""
    rng = np.random.default_rng(77)
    clean = _lattice(m, hi=(512, 512, 0))
    pts = clean.copy()
    hit = np.unique(np.concatenate([rng.choice(m, m // 100, replace=False), [0, T - 1, T, m - 2, m - 1]]))
    pts[hit, rng.integers(0, 6, len(hit))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(hit))
    return clean, pts, len(hit)


@pytest.mark.parametrize('backend', BACKENDS)
def test_scan_levels_dropped_rows(backend):
    """65,537 points (n_sums == 2: the scatter's `sums[g / kVxTile]`) of which 1 % are dropped: `dropped` is not zero, the last
    pass runs only to move them (digit 8 against the cells' one digit), and mv < M in pcl_voxel_heads_kernel and
    pcl_voxel_reduce_kernel.  Times: the table above LEVEL_CASES."""
    dev = use_backend(backend)
    m, vs = 65537, 0.25
    clean, pts, n_hit = _dropped_cloud(m)
    ref = V.voxel_exact(pts, vs)
    _has_work(ref)
    assert ref['dropped'] == n_hit >= m // 100 and ref['all_counts'].sum() == m - n_hit
    assert not np.isfinite(pts[m - 1]).all() and not np.isfinite(pts[0]).all()
    assert 15 not in [p for p, _ in V.radix_trace(clean, vs)] and V.radix_trace(pts, vs)[-1][0] == 15
    passes = _scan_conditions(pts, vs)
    assert passes == _passes(ref['keys']) + 1 == 13
    out = _run(dev, pts, vs)
    assert np.isfinite(out[0]).all()
    _check_exact(backend, 'dropped rows', out, ref, vs, passes)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('min_points', [2, 3])
def test_scan_levels_min_points(backend, min_points):
    """vx_head's `K[i + min_points - 1]` across tile and scan-block boundaries, at 65,537 points (n_sums == 2).  The cell of the
    largest key holds exactly min_points members, so its run starts before position 65,536 = 64 * 1024 and ends on it: the head
    in the last full tile reads the one key of the last tile.  Times: the table above LEVEL_CASES."""
    dev = use_backend(backend)
    m, vs = 65537, 0.5
    pts = _lattice(m, top=(min_points, vs))
    every, ref = V.voxel_exact(pts, vs), V.voxel_exact(pts, vs, min_points)
    _has_work(_every_cell(ref))                      # of every cell: no cell of one member survives min_points >= 2
    assert 0 < len(ref['counts']) < len(every['counts']) and ref['counts'].min() == min_points
    start = np.cumsum(every['all_counts']) - every['all_counts']
    last = start + every['all_counts'] - 1
    straddles = [(int(a), int(b)) for a, b, n in zip(start, last, every['all_counts'])
                 if n >= min_points and any(a < T * k <= b for k in range(64, m // T + 1))]
    assert (m - min_points, m - 1) in straddles, straddles
    assert sum(1 for a, b in zip(start, last) if a // T != b // T) > 10                       # and runs across tile boundaries
    passes = _scan_conditions(pts, vs)
    assert passes == 16
    out = _run(dev, pts, vs, min_points=min_points)
    _check_exact(backend, f'min_points {min_points}', out, ref, vs, passes)
    all_rows, all_counts, _ = _run(dev, pts, vs)
    assert np.array_equal(_bits(out[0]), _bits(all_rows[all_counts >= min_points]))               # the same rows, fewer of them


def _signed_permutations():
    """five poses that keep a lattice cloud on the lattice, exactly: an axis permutation with sign flips, and a translation in
    64ths that is zero on no axis (so no coordinate comes out as -0.0)"""
    perms = [((0, 1, 2), (1, -1, 1)), ((1, 2, 0), (-1, 1, 1)), ((0, 2, 1), (1, -1, 1)), ((2, 0, 1), (-1, -1, 1)),
             ((1, 0, 2), (-1, -1, -1))]
    shifts = [(37, -101, 5), (-64, 3, 200), (1, 1, -1), (255, -256, 77), (-130, 64, -9)]  # the third keeps x where _lattice put it
    out = []
    for (perm, sign), shift in zip(perms, shifts):
        P = np.eye(4)
        P[:3, :3] = 0
        for r in range(3):
            P[r, perm[r]] = sign[r]
        P[:3, 3] = np.asarray(shift) / 64.0
        out.append(P)
    return np.stack(out)


@pytest.mark.parametrize('backend', BACKENDS)
def test_scan_levels_fused_poses(backend):
    """65,537 points (n_sums == 2: the scatter's `sums[g / kVxTile]`) in five segments with boundaries at 0, 1, 65,536 and 65,537:
    an empty first segment, one point, 65,535 points, an empty segment whose pose is NaN, and the one point of the last tile.  The
    poses are signed axis permutations with translations in 64ths: pose_apply is exact, the posed cloud stays on the lattice, and
    the fused result equals the reference on the posed points and the filter of the transformed cloud, bitwise.  Times: the
    table above LEVEL_CASES."""
    dev = use_backend(backend)
    m, vs = 65537, 0.25
    pts = _lattice(m)
    offsets = np.array([0, 0, 1, 65536, 65536, 65537], np.int64)
    poses = _signed_permutations()
    poses[3] = np.nan
    posed = pts.copy()
    for f in range(5):
        a, b = offsets[f], offsets[f + 1]
        if b > a:
            posed[a:b, :3] = (pts[a:b, :3].astype(np.float64) @ poses[f][:3, :3].T + poses[f][:3, 3]).astype(np.float32)
    assert V.is_lattice(posed, vs) and not np.signbit(posed[posed == 0]).any()
    ref = V.voxel_exact(posed, vs)
    _has_work(ref)
    passes = _scan_conditions(posed, vs)
    assert passes == 16
    world = ops.pcl_transform(_t(pts, dev), offsets, _t(poses, dev))
    assert np.array_equal(_bits(world.cpu().numpy()), _bits(posed))
    two = ops.pcl_voxel_downsample(world, vs, return_info=True)
    _check_exact(backend, 'transformed, then filtered', (two[0].cpu().numpy(), two[1].cpu().numpy(), two[2]), ref, vs, passes)
    _check_exact(backend, 'fused poses', _run(dev, pts, vs, offsets=offsets, poses=poses), ref, vs, passes)


@pytest.mark.parametrize('backend', BACKENDS)
def test_determinism_multi_level(backend):
    """two runs of the 262,147-point case (n_sums == 5: the scatter's `sums[g / kVxTile]` in 257 blocks that run in any order) are
    bit-equal, and equal to the reference.  Times: the table above LEVEL_CASES."""
    dev = use_backend(backend)
    m, vs = 262147, 0.25
    pts = _lattice(m)
    ref = V.voxel_exact(pts, vs)
    _has_work(ref)
    passes = _scan_conditions(pts, vs)
    a = _run(dev, pts, vs)
    b = _run(dev, pts, vs)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    _check_exact(backend, 'second run', b, ref, vs, passes)


@pytest.mark.gpu
def test_scan_sums_two_per_thread():
    """pcl_voxel_scan_sums_kernel's `per = ceil(n / 256)` at per == 2: 16,777,217 points are 16,385 tiles and n_sums == 257, so
    thread t scans sums 2 t and 2 t + 1, thread 128 takes the one that is left and the `lo` / `hi` clamp leaves the threads from
    129 on empty.  (The heads' second level has 17 sums here.)  0.4 GB of cloud and as much scratch on the device; on the host the
    process peaks at 2.2 GB (the cloud, and the float64 cell indices the reference forms from it).  The cloud straddles the bias
    in x only: x in [-8, 8), y in [0, 2), z in [-0.5, 0) for all but some 4,000 rows with z in [-8, 0), which are mostly alone in
    their cells -- the keys vary in the digits 0-5, 10 and 11, eight passes.  Host time is the cost (the table above LEVEL_CASES):
    the cloud is one integers() call per array and the reference np.bincount over the 64 x 8 x 32 cells of the box."""
    dev = use_backend('hip')
    m, vs = (1 << 24) + 1, 0.25
    tiles = -(-m // T)
    assert -(-16 * tiles // T) == 257 and -(-257 // 256) == 2 and min(129 * 2, 257) == 257
    lo = np.empty((m, 3), np.int16)                  # per row for z only; int16 bounds, 0.1 GB
    lo[:] = (-512, 0, -32)
    lo[np.random.default_rng(3).choice(m, 4000, replace=False), 2] = -512
    pts = V.lattice_cloud(m, seed=m, lo=lo, hi=(512, 128, 0))
    del lo
    ref = V.voxel_exact(pts, vs)
    _has_work(ref)
    passes = _scan_conditions(pts, vs)
    assert passes == 8 == _passes(ref['keys'])
    try:
        _check_exact('hip', f'M = {m}', _run(dev, pts, vs), ref, vs, passes)
    finally:
        torch.cuda.empty_cache()


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
