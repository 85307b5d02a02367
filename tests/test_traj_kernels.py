"""The kernels of cl-slam_amd/csrc/traj_eval.hip (ops.traj_metrics, ops.pose_pair_error) at the places the smooth fixture of
tests/test_traj_metrics.py keeps away from: exact ties in the segment search, every row exchange of the 4x4 inverse, the clamp of
the rotation error, non-finite poses, the sizes at which a launch gains a block or a kernel, every shape of numpy's summation
tree, and the documented maximum of 2^20 poses.  Twin and truth are those of tests/traj_eval_reference.py; the helpers and the
full check (_check_all) are the ones of tests/test_traj_metrics.py, imported, not copied.  Every figure of the twin is formed
before the kernel's output is read; figures are printed with -s.

Bounds.  None is new:
  * decisions (first_frame, length, last_frame, speed, the NaN rows, n_segments): the twin's, exactly.
  * ties: translations on a 0.5 m grid make every partial sum of the steps exact, so dist is the twin's bit for bit and
    dist[first + 200 k] == dist[first] + 100 k holds exactly; the twin's linear scan is asserted to step over the tie (and over a
    whole run of equal dist) before the kernel is looked at.
  * pose_pair_error on general matrices: per output column, the largest deviation from the longdouble truth <= 4 x the float64
    twin's (R.pair_errors: np.linalg.inv and @), the twin's asserted non-zero first.  The eight fixed motions M and the random ones
    turn by 0.3 .. 2.5 rad, where acos is well conditioned: nearer 0 or pi the rotation column's error is that of one
    rounding of d amplified by 1 / sin, and which of kernel and twin rounds worse there is chance.  cond_2 <= 10 is asserted for
    every matrix that is inverted.
  * a tie of two column maxima: integer matrices for which the documented rule (the FIRST row of the largest |a[r][k]|) makes
    every operation of the elimination exact in binary64 (asserted against rational arithmetic), while the last such row does not
    (asserted with R.lu_inverse(tie='last')): the translation error is then the correctly rounded square root of an exact sum,
    and is asserted bitwise.
  * clamp: d = 1.25 -> exactly 0.0; d = -2.25 and d = -1 -> within one ulp of np.pi (acos is not promised correctly rounded).
  * launch boundaries: the whole _check_all of tests/test_traj_metrics.py (its docstring states the bounds), elements included.
  * scaling: np.sum(X * Y) / np.sum(X ** 2) by numpy itself, bitwise.  The inputs span 10^-3 .. 10^3 with random signs; a strict
    left-to-right sum is first shown to give other bits than np.sum at more than 90 % of the lengths above 8.
  * 2^20 poses: dist within n * 2^-52 * path_length of the longdouble cumulative sum, ATE within R.mean_bound, scaling bitwise,
    last_frame equal to np.searchsorted(twin dist, limit, 'right') on the rows whose margin on the twin is >= 1e-6 (the share of
    rows left out is asserted <= 0.1 % on the twin first).

Pivot paths.  b = P D for the 24 row permutations P of a matrix D that is strictly diagonally dominant by columns (so are its
Schur complements: the pivot of column k is always D's row k, wherever P put it).  R.lu_inverse, a plain-Python restatement of
"first row of the largest |a[r][k]|", finds 24 different pivot sequences that cover every (k, p):
(0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3).

Defect found.  test_the_documented_maximum failed on gfx950 at the scaling: the kernel added the 3n products in ONE pairwise tree,
but np.sum is one tree only up to numpy's buffer size of 8192 elements; a longer array is summed piece by piece, 8192 elements
at a time, and the sums of the pieces are added to the result in order.  Beyond 2730 poses the factor was therefore not the
reference's to the last bit (at 2^20 poses it differed in the last digit: 0.9994321281848471 for 0.9994321281848473); the 4541
poses of tests/test_traj_metrics.py agreed by chance (mutation (q) below still passes that file).  Fixed in traj_eval.hip
(kTePiece: the leaf kernel descends the tree of its piece, the tree kernel adds the pieces up);
test_scale_sums_in_numpy_order[beyond one 8192-element piece] holds it on both backends, with inputs drawn until a single tree
gives other bits than np.sum in both sums (R.pairwise_tree_sum).

Measured (emu | hip).  Largest ratio kernel / twin of an element deviation: 24 permutations x 8 motions 1.09 | 1.00 (plain), 0.58 |
0.52 (inverted); 513 random 1.10 | 1.47; launch boundaries 1.98 (n = 682, segment trans) | 2.04 (n = 320, rpe pair trans).  dist at
the boundaries: at most 0.01 of its bound.  Ties, clamp (0.0; pi within one ulp), poisoned rows, the tied maxima and the
scaling at all 149 lengths: exact on both.  2^20 poses on gfx950: dist off by 5.4e-10 m (twin 1.1e-7, bound 1.2e-4), ATE off
by 2.5e-16 (bound 2.8e-15), no row within 1e-6 m of a decision, so all 838864 rows are compared; the launch takes 18 - 24 ms
(first launch, allocation of the scratch included), the references 0.3 s, the whole case 0.33 s.  No other case of this file takes
more than 0.5 s on either backend; the whole file runs in 4 s on the emulator.

One-line mutations of a scratch copy of traj_eval.hip (CPU emulator, never committed), the tests of this file that fail, and
whether tests/test_traj_metrics.py alone fails ("old: ..."):
  (a) `dist[mid] > limit` -> `>=`                 test_segment_search_on_exact_ties (all four)                        old: passes
  (b) `lo = first + 1` -> `lo = first`            NO test fails, and none can: dist[first] > dist[first] + length is false for
          every length >= 100 (and for a NaN), so the search takes the same path one step later.  Equivalent.
  (c) the swap of `b` dropped in inv4             test_inverse_on_every_pivot_path (all four), test_pivot_tie_takes_the_first_row,
          test_launch_boundaries[2048, 2049]                                                                         old: fails
          (so the smooth fixture does exchange rows)
  (d) `v > best` -> `v >= best`                   test_pivot_tie_takes_the_first_row only: equivalent on the 24 permutations and
          on every other input here, which have no two equal column maxima                                           old: passes
  (e) the swap of `a` (or of `b`) applied to row r + 1     as (c)                                                    old: fails
  (f) the upper clamp removed                     test_rotation_error_clamp, test_traj_metrics_poisoned_pose_stays_in_its_rows,
          test_launch_boundaries[320, 682, 683, 1023, 1024] (d > 1 by rounding somewhere: NaN)                       old: passes
  (g) the lower clamp removed                     test_rotation_error_clamp                                          old: passes
  (h) `h - h % 8` -> `h`                          test_scale_sums_in_numpy_order (all), most sizes of test_launch_boundaries,
          test_traj_metrics_poisoned_pose_stays_in_its_rows (leaf slots left unwritten)                              old: fails
  (i) `i < n - n % 8` -> `i < n`                  test_scale_sums_in_numpy_order (all), most of test_launch_boundaries    old: fails
  (j) `n > kTeLeaf` -> `n >= kTeLeaf` (leaves)    test_scale_sums_in_numpy_order[65-130, 170-175, splits, beyond],
          test_launch_boundaries[682, 683]                                                        old: test_kitti_length only
  (k) `n <= kTeLeaf` -> `n < kTeLeaf` (tree)      the same ranges, test_launch_boundaries[682]  old: kitti_length, two_launches
  (l) `if (nscan > 1)` -> `if (nscan > 2)`        test_segment_search_on_exact_ties (all four), test_launch_boundaries[1025, 2048]
                                                                                                                     old: passes
  (m) `off += totals[b]` for b <= blockIdx.x      test_segment_search_on_exact_ties (all four), test_launch_boundaries (8 sizes)
                                                                                                                     old: fails
  (n) thread 0's exclusive scan made inclusive    test_segment_search_on_exact_ties, test_launch_boundaries (all)    old: fails
  (o) `row[5] >= 0.0` -> `> 0.0` in the finalize  NO test fails, and none can: row[5] is -1 or a last frame, and a last frame is
          at least first + 1 >= 1.  Equivalent.
  (p) `n - 1` -> `n` in the RPE mean              test_launch_boundaries (all twelve)                                old: fails
  (q) the pieces of the scale removed (kTePiece = 2^30: the kernel as it was)
                                                  test_scale_sums_in_numpy_order[beyond one 8192-element piece] (and
          test_the_documented_maximum on gfx950)                                                                     old: passes
  (r) `b += kTeThreads` -> `b += 1` in the finalize     test_launch_boundaries from 257 poses on (ten sizes)         old: fails
"""
import functools
import itertools
import math
import time
from fractions import Fraction

import numpy as np
import pytest
import torch

import test_traj_metrics as T
import traj_eval_reference as R
from clslam_hip import _lib, ops
from emu_util import BACKENDS, use_backend

U52 = 2.0 ** -52
SENTINEL = 7.0


def _pair_launch(dev, a, b, a_inverted=False):
    out = torch.full((len(a), 2), SENTINEL, dtype=torch.float64, device=dev)
    got = ops.pose_pair_error(torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(dev),
                              torch.from_numpy(np.array(b, dtype=np.float64, order='C')).to(dev), a_inverted=a_inverted, out=out)
    assert got is out
    return out.cpu().numpy()


def _rigid(axis, angle, t):
    """Rodrigues: the pose that turns by `angle` about `axis` and moves by t"""
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    m[:3, 3] = t
    return m


# ---- 1. exact ties in the segment search -------------------------------------------------------------------------------------
TIE_CASES = {'every row a tie': (1700, None), 'standstill on the tie': (1700, 400), 'standstill across scan blocks': (1700, 1000),
             'a tie at the last frame': (1601, None)}
STANDSTILL = 50


@functools.lru_cache(maxsize=None)
def _tie_case(name):
    """gt on the z axis in steps of exactly 0.5 m, with 50 steps of 0 behind frame `still`; pred = gt shifted.  Everything that
    can be asserted on the twin alone is asserted here."""
    n, still = TIE_CASES[name]
    moving = np.ones(n, dtype=bool)
    moving[0] = False
    if still is not None:
        moving[still + 1:still + 1 + STANDSTILL] = False
    z = 0.5 * np.cumsum(moving)                                                          # exact
    xyz = np.zeros((n, 3))
    xyz[:, 2] = z
    gt = R.poses_from_xyz(xyz)
    pred = gt.copy()
    pred[:, :3, 3] += np.array([3.0, 4.0, 0.0])
    twin = R.evaluate(pred, gt)
    dist = twin['dist']
    assert np.array_equal(T._bits(dist), T._bits(z))                                    # every dist a multiple of 0.5, exactly
    first, length, last = R.segment_frames(dist)
    limit = dist[first] + length
    linear = np.array([R.last_frame_linear(dist, int(f), int(l)) for f, l in zip(first, length)])
    assert np.array_equal(linear, last) and np.array_equal(twin['segments'][:, 5], last)
    assert n != 1700 or set(length[last >= 0]) == set(R.LENGTHS)
    tie = np.isin(limit, dist)
    if still is None:                                                                # dist[first + 200 k] == dist[first] + 100 k
        j = first + 2 * length.astype(np.int64)
        inside = j < n
        assert np.array_equal(T._bits(dist[j[inside]]), T._bits(limit[inside])) and tie[inside].all() and not tie[~inside].any()
        assert np.array_equal(last[inside], np.where(j[inside] + 1 < n, j[inside] + 1, -1))
        assert (last[~inside] == -1).all() and inside.sum() > 500
        if name == 'a tie at the last frame':
            assert (j == n - 1).sum() == 8 and (last[j == n - 1] == -1).all()
    else:                                                                                # the tie is a run of 51 equal dist
        on_run = limit == dist[still]
        assert on_run.sum() >= 2 and (dist[still:still + STANDSTILL + 1] == dist[still]).all()
        assert (last[on_run] == still + STANDSTILL + 1).all() and dist[still + STANDSTILL + 1] > dist[still]
        assert tie.sum() > 500
    return pred, gt, twin


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', list(TIE_CASES))
def test_segment_search_on_exact_ties(backend, name):
    """`dist[mid] > limit` must be strict (slam/utils.py:185-188): the frame AT the limit is not the last frame, the next one
    that moved is -- also when the frames at the limit are a standstill of 51, inside one scan block or across two"""
    dev = use_backend(backend)
    pred, gt, twin = _tie_case(name)
    out, seg, dist, _ = T._launch(dev, pred, gt)
    assert np.array_equal(T._bits(dist), T._bits(twin['dist'])) and out[7] == dist[-1]   # exact sums: no rounding anywhere
    T._check_decisions(name, seg, out, twin)
    print(f'[traj_kernels {backend}] {name:<30} rows {len(seg)}, with a last frame {int(out[2])}')


# ---- 2. every pivot path of inv4 -----------------------------------------------------------------------------------------------
DOMINANT = np.array([[4.1, -0.9, 1.3, 0.7],
                     [1.2, 5.3, -0.8, -1.1],
                     [-0.7, 1.4, 6.2, 0.9],
                     [0.9, -1.6, 1.7, 7.3]])
# eight motions, so that the twin's largest deviation is a maximum over 192 rows and not the luck of 24
MOTIONS = np.stack([_rigid(axis, angle, t) for axis, angle, t in (
    ([1.0, 2.0, 3.0], 1.1, [0.7, -1.3, 2.1]), ([-2.0, 1.0, 0.5], 0.3, [-0.4, 0.9, 0.2]), ([0.3, -1.0, 2.0], 0.6, [1.9, 0.3, -0.8]),
    ([1.0, 0.0, 0.0], 0.9, [0.1, 0.2, 0.3]), ([0.0, 1.0, 0.1], 1.4, [-2.2, 1.1, 0.6]), ([1.0, 1.0, -1.0], 1.8, [0.5, -0.5, 1.5]),
    ([-1.0, 3.0, 2.0], 2.2, [3.1, -0.7, 0.4]), ([2.0, -1.0, 1.0], 2.5, [-0.9, -1.7, 0.8]))])
ALL_PIVOTS = {(k, p) for k in range(3) for p in range(k, 4)}


@functools.lru_cache(maxsize=None)
def _permuted(a_inverted):
    D = DOMINANT
    off = np.abs(D).sum(axis=0) - np.abs(np.diag(D))
    assert (np.abs(np.diag(D)) > off).all() and (D[3, :3] != 0).all()                    # dominant by columns, a full last row
    assert np.linalg.cond(D) <= 10.0
    perms = list(itertools.permutations(range(4)))
    b = np.stack([D[list(p)] for p in perms])
    seqs = [tuple(R.lu_inverse(m)[1][:3]) for m in b]
    assert len(set(seqs)) == 24                                                          # a pivot sequence of its own for each P
    assert {(k, s[k]) for s in seqs for k in range(3)} == ALL_PIVOTS
    b = np.repeat(b, len(MOTIONS), axis=0)                                               # every P with every motion: 192 rows
    a = b @ np.tile(MOTIONS, (len(perms), 1, 1))
    if a_inverted:
        a = R.inv_hp(a).astype(np.float64)
    return a, b, R.pair_errors(a, b, a_inverted), R.pair_errors(a, b, a_inverted, hp=True)


@functools.lru_cache(maxsize=None)
def _random_general(a_inverted, n=513):
    rng = np.random.default_rng(11)
    q1 = np.linalg.qr(rng.normal(size=(n, 4, 4)))[0]
    q2 = np.linalg.qr(rng.normal(size=(n, 4, 4)))[0]
    b = (q1 * rng.uniform(1.0, 3.0, (n, 1, 4))) @ q2                                     # singular values in [1, 3]
    m = np.stack([_rigid(rng.normal(size=3), rng.uniform(0.3, 2.5), rng.uniform(-0.5, 0.5, 3)) for _ in range(n)])
    a = b @ m
    if a_inverted:
        a = R.inv_hp(a).astype(np.float64)
    assert np.linalg.cond(b).max() <= 10.0 and np.linalg.cond(a).max() <= 10.0
    return a, b, R.pair_errors(a, b, a_inverted), R.pair_errors(a, b, a_inverted, hp=True)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('a_inverted', [False, True], ids=['plain', 'inverted'])
@pytest.mark.parametrize('batch', ['24 permutations', '513 random'])
def test_inverse_on_every_pivot_path(backend, a_inverted, batch):
    """general 4x4 matrices through pose_pair_error: inv(b) @ a with b = P D for every row permutation P (each forces another
    sequence of row exchanges, on `a` and on the right-hand side alike), and 513 random ones (three blocks, one matrix in the
    last).  Rotation angles are 0.3 .. 2.5 rad, where acos is well conditioned (module docstring)."""
    dev = use_backend(backend)
    a, b, twin, truth = _permuted(a_inverted) if batch.startswith('24') else _random_general(a_inverted)
    k = _pair_launch(dev, a, b, a_inverted)
    case = f'{batch} inverted={int(a_inverted)}'
    T._check_elements(backend, case, 'trans', k[:, 0], twin[:, 0], truth[:, 0])
    T._check_elements(backend, case, 'rot', k[:, 1], twin[:, 1], truth[:, 1])


# Two equal maxima in column 0 (rows 0 and 2, 0 and 1, ...).  With the first of them as the pivot every operation is exact.
TIED_MAXIMA = [[[4, 4, -4, -2], [-2, 1, 2, -1], [4, 1, -3, 4], [-2, 3, -3, -1]],
               [[3, -2, 3, 1], [-2, 0, 2, -1], [3, 2, 3, -3], [0, 0, 4, 1]],
               [[4, -3, 1, 4], [2, -4, 1, 1], [4, 1, -3, -4], [0, -2, 2, -4]],
               [[-2, -1, -1, 4], [-1, -2, -1, -2], [-2, 3, 3, 1], [-1, -3, -4, 1]]]


def _rational_inverse(a):
    A = [[Fraction(int(x)) for x in row] + [Fraction(int(i == j)) for j in range(4)] for i, row in enumerate(a)]
    for k in range(4):
        p = next(r for r in range(k, 4) if A[r][k] != 0)
        A[k], A[p] = A[p], A[k]
        A[k] = [x / A[k][k] for x in A[k]]
        for r in range(4):
            if r != k:
                A[r] = [x - A[r][k] * y for x, y in zip(A[r], A[k])]
    return [row[4:] for row in A]


@pytest.mark.parametrize('backend', BACKENDS)
def test_pivot_tie_takes_the_first_row(backend):
    """`v > best` is strict: of two rows with the same |a[r][k]| the first is the pivot (LAPACK's rule too).  The 24 permutations
    have no tie, so these matrices are the only place where `>=` shows."""
    dev = use_backend(backend)
    expected = []
    for m in TIED_MAXIMA:
        col = [abs(r[0]) for r in m]
        assert col.count(max(col)) == 2 and np.linalg.cond(np.array(m, dtype=np.float64)) <= 10.0
        exact = _rational_inverse(m)
        first, p_first = R.lu_inverse(m, 'first')
        last, p_last = R.lu_inverse(m, 'last')
        assert p_first[0] != p_last[0]
        assert all(Fraction(first[i][j]) == exact[i][j] for i in range(4) for j in range(4))        # no rounding on this path
        sq = (first[0][3] ** 2 + first[1][3] ** 2) + first[2][3] ** 2
        assert Fraction(sq) == exact[0][3] ** 2 + exact[1][3] ** 2 + exact[2][3] ** 2
        expected.append(math.sqrt(sq))
        assert math.sqrt((last[0][3] ** 2 + last[1][3] ** 2) + last[2][3] ** 2) != expected[-1]    # the other rule is visible
    b = np.array(TIED_MAXIMA, dtype=np.float64)
    a = np.broadcast_to(np.eye(4), b.shape).copy()
    k = _pair_launch(dev, a, b)
    assert np.array_equal(T._bits(k[:, 0]), T._bits(expected)), (k[:, 0], expected)
    assert np.isfinite(k[:, 1]).all()


# ---- 3. the clamp and the non-finite cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_rotation_error_clamp(backend):
    dev = use_backend(backend)
    a = np.stack([np.diag([1.5, 1.0, 1.0, 1.0]), np.diag([-1.5, -1.0, -1.0, 1.0]), np.diag([-1.0, -1.0, 1.0, 1.0])])
    d = 0.5 * (a[:, 0, 0] + a[:, 1, 1] + a[:, 2, 2] - 1.0)
    assert list(d) == [1.25, -2.25, -1.0]
    k = _pair_launch(dev, a, np.broadcast_to(np.eye(4), a.shape))
    print(f'[traj_kernels {backend}] clamp: rot {k[:, 1]!r} trans {k[:, 0]!r}')
    assert k[0, 1] == 0.0 and k[0, 0] == 0.0 and not np.signbit(k[0]).any()
    for i in (1, 2):
        assert np.isfinite(k[i, 1]) and abs(k[i, 1] - np.pi) <= np.spacing(np.pi), (i, k[i, 1])


@pytest.mark.parametrize('backend', BACKENDS)
def test_pair_error_poisoned_poses_stay_in_their_rows(backend):
    """one NaN, or an all-zero (singular) matrix, wherever the kernel inverts -- b, or a with a_inverted -- gives non-finite
    outputs in that row (NaN for the NaN) and leaves the other rows bit for bit.  (A poisoned `a` that is NOT inverted reaches
    only the columns of the product it stands in: that is the reference's behaviour too and is not asserted here.)"""
    dev = use_backend(backend)
    pred, gt = R.make_fixture(300, 1, 4.0)
    a0, b0 = np.array(pred[:261]), np.array(gt[:261])                                    # two blocks; rows around the block edge
    for a_inverted in (False, True):
        clean = _pair_launch(dev, a0, b0, a_inverted)
        assert np.isfinite(clean).all()
        for kind in ('nan', 'zero'):
            a, b = a0.copy(), b0.copy()
            target = a if a_inverted else b
            rows = (3, 255, 256, 260)
            for r in rows:
                if kind == 'nan':
                    target[r, r % 4, (r + 1) % 4] = np.nan
                else:
                    target[r] = 0.0
            k = _pair_launch(dev, a, b, a_inverted)
            others = np.setdiff1d(np.arange(261), rows)
            assert np.array_equal(T._bits(k[others]), T._bits(clean[others])), (kind, a_inverted)
            assert not np.isfinite(k[list(rows)]).any(), (kind, a_inverted, k[list(rows)])
            if kind == 'nan':
                assert np.isnan(k[list(rows)]).all()


@functools.lru_cache(maxsize=None)
def _poison_case():
    pred, gt = R.make_fixture(300, 1, 4.0)
    first, _, last = R.segment_frames(R.distances(gt))
    both = sorted(set(first[last >= 0]) & set(last[last >= 0]))                  # a first frame of some rows, the last of others
    assert both and 0 < both[len(both) // 2] < 299
    return pred, gt, int(both[len(both) // 2])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', ['nan', 'zero'])
def test_traj_metrics_poisoned_pose_stays_in_its_rows(backend, kind):
    """the rotation block of ONE ground-truth pose holds a NaN / is all zero (its translation is intact, so dist is unchanged by
    design): the pair errors (i-1, i) and (i, i+1) are non-finite, every other pair, dist, the scaling and every segment that
    neither starts nor ends at frame i are those of the clean launch, bit for bit"""
    dev = use_backend(backend)
    pred, gt, i = _poison_case()
    clean = T._launch(dev, pred, gt)
    bad = np.array(gt)
    if kind == 'nan':
        bad[i, 1, 2] = np.nan
    else:
        bad[i, :3, :3] = 0.0
    out, seg, dist, pairs = T._launch(dev, pred, bad)
    c_out, c_seg, c_dist, c_pairs = clean
    assert np.isfinite(c_pairs).all() and np.isfinite(c_seg[c_seg[:, 5] >= 0]).all()
    others = np.setdiff1d(np.arange(299), [i - 1, i])
    assert np.array_equal(T._bits(pairs[others]), T._bits(c_pairs[others]))
    assert not np.isfinite(pairs[[i - 1, i]]).any(), pairs[[i - 1, i]]
    assert np.array_equal(T._bits(dist), T._bits(c_dist))
    assert T._bits(out[6]) == T._bits(c_out[6]) and T._bits(out[7]) == T._bits(c_out[7]) and out[2] == c_out[2]
    starts, ends = c_seg[:, 0] == i, c_seg[:, 5] == i
    assert starts.sum() == 8 and (c_seg[starts, 5] >= 0).any() and ends.any()
    untouched = ~(starts | ends)
    assert np.array_equal(T._bits(seg[untouched]), T._bits(c_seg[untouched]))
    assert np.array_equal(T._bits(seg[:, [0, 3, 4, 5]]), T._bits(c_seg[:, [0, 3, 4, 5]]))          # the decisions come from dist
    assert not np.isfinite(seg[starts & (c_seg[:, 5] >= 0)][:, 1:3]).any()


# ---- 4. launch boundaries ----------------------------------------------------------------------------------------------------
#   255/256/257   a second block of terms, a second partial in the finalize        320/321    segment rows 256 -> 264
#   682/683       leaf slots of the scale 256 -> 257 (3n = 2046 / 2049)            1023..1025 the scan totals kernel appears
#   2048/2049     a third scan block
BOUNDARY_SIZES = [255, 256, 257, 320, 321, 682, 683, 1023, 1024, 1025, 2048, 2049]


@functools.lru_cache(maxsize=None)
def _boundary(n):
    pred, gt = R.make_fixture(n, 5, 2.0)                                                  # 2 m a frame: 510 m at n = 255
    twin, truth = R.evaluate(pred, gt), R.evaluate(pred, gt, hp=True)
    ok = twin['segments'][:, 5] >= 0
    assert len(set(twin['segments'][ok, 3])) >= 3
    return pred, gt, twin, truth


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n', BOUNDARY_SIZES)
def test_launch_boundaries(backend, n):
    dev = use_backend(backend)
    pred, gt, twin, truth = _boundary(n)
    out, seg, dist, pairs = T._launch(dev, pred, gt)
    T._check_all(backend, f'n={n}', out, seg, dist, pairs, twin, truth)
    if n > 1024:
        assert (np.diff(dist) >= 0).all()
        for edge in range(1024, n, 1024):                                            # the offset of a block is the sum that ends
            assert dist[edge] >= dist[edge - 1] and dist[edge] > 0                       # the one before it
        assert T._dev(dist, truth['dist']) <= n * U52 * float(truth['path_length'])


# ---- 5. the summation tree of the scale, at every shape -------------------------------------------------------------------------
#   3n = 8190 | 8193, 8199 (a second piece of 1 and of 7 elements) | 13623 (KITTI 00) | 16383, 16386 | 24576 (three whole pieces) |
#   32769 (a fifth piece of one element)
TREE_RANGES = {'1-64': range(1, 65), '65-130': range(65, 131), '170-175': range(170, 176),
               'second and third splits': (341, 342, 343, 683, 1366),
               'beyond one 8192-element piece': (2730, 2731, 2733, 4541, 5461, 5462, 8192, 10923)}
PIECE = 8192                                                                             # numpy's buffer size (np.getbufsize())


def _left_to_right(v):
    s = 0.0
    for x in v.ravel().tolist():
        s += x
    return s


def _wide(n, seed):
    rng = np.random.default_rng(seed)
    return tuple(np.ascontiguousarray(rng.choice([-1.0, 1.0], (n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 3))) for _ in range(2))


def _one_tree_differs(X, Y):
    return (R.pairwise_tree_sum((X * Y).ravel()) != np.sum(X * Y)) and (R.pairwise_tree_sum((X ** 2).ravel()) != np.sum(X ** 2))


@functools.lru_cache(maxsize=None)
def _tree_inputs():
    """n -> X, Y (n,3) contiguous: random signs, magnitudes 10^-3 .. 10^3.  Shown first: the order of the additions is visible in
    the bits at more than 90 % of the lengths above 8; and beyond 8192 elements, where np.sum is no longer one pairwise tree but
    the pieces of numpy's buffered reduction added in order, the inputs are drawn until BOTH sums tell the two apart."""
    cases = {}
    for n in itertools.chain(*TREE_RANGES.values()):
        cases[n] = _wide(n, 1000 + n)
        if 3 * n > PIECE:
            cases[n] = next(c for c in (_wide(n, 1000 * k + n) for k in range(1, 40)) if _one_tree_differs(*c))
    long = [n for n in cases if 3 * n > 8]
    differs = [n for n in long if _left_to_right(cases[n][0] * cases[n][1]) != np.sum(cases[n][0] * cases[n][1])
               or _left_to_right(cases[n][0] ** 2) != np.sum(cases[n][0] ** 2)]
    print(f'[traj_kernels] summation order visible at {len(differs)} of {len(long)} lengths above 8')
    assert len(differs) >= 0.9 * len(long)
    assert np.getbufsize() == PIECE and sum(3 * n > PIECE for n in cases) == 7
    assert all(R.pairwise_tree_sum(cases[n][0].ravel()) == np.sum(cases[n][0]) for n in cases if 128 < 3 * n <= PIECE)
    return cases


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('which', list(TREE_RANGES))
def test_scale_sums_in_numpy_order(backend, which):
    dev = use_backend(backend)
    cases = _tree_inputs()
    wrong = []
    for n in TREE_RANGES[which]:
        X, Y = cases[n]
        want = np.sum(X * Y) / np.sum(X ** 2)                                            # numpy itself
        out = torch.full((8,), SENTINEL, dtype=torch.float64, device=dev)
        ops.traj_metrics(torch.from_numpy(R.poses_from_xyz(X)).to(dev), torch.from_numpy(R.poses_from_xyz(Y)).to(dev), out=out)
        got = out.cpu().numpy()[6]
        if T._bits(got) != T._bits(want):
            wrong.append((n, float(got), float(want)))
    total = len(TREE_RANGES[which])
    print(f'[traj_kernels {backend}] scaling bitwise at n in {which}: {total - len(wrong)} of {total}')
    assert not wrong, wrong


# ---- 6. the documented maximum -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_documented_maximum():
    """TRAJ_MAX_POSES = 2^20 poses in one launch: 1024 scan blocks, 4096 partials (sixteen per thread of the finalize), 838864
    segment rows, a summation tree over 3145728 elements.  Rotations are identity, so every reference is one vectorised numpy
    expression."""
    dev = use_backend('hip')
    n = _lib.TRAJ_MAX_POSES
    t0 = time.perf_counter()
    i = np.arange(n)
    s = 0.25 + 0.5 * ((i * 37 % 101) / 100.0)                                            # step lengths 0.25 .. 0.75 m
    th = i * (2 * np.pi / 5000.0)
    stepv = np.round(np.stack([s * np.cos(th), 0.02 * s, s * np.sin(th)], axis=1) * 1024.0) / 1024.0
    stepv[0] = 0.0
    Y = np.cumsum(stepv, axis=0)                                                         # a helix on a 2^-10 grid: exact
    assert np.array_equal(np.diff(Y, axis=0), stepv[1:])
    X = np.ascontiguousarray(Y + np.stack([3 + np.sin(i / 1000.0), 4 + np.cos(i / 777.0), 0.5 * np.sin(i / 5000.0)], axis=1))
    pred, gt = R.poses_from_xyz(X), R.poses_from_xyz(Y)
    # the twin and the truth
    norm = np.sqrt((stepv[:, 0] ** 2 + stepv[:, 1] ** 2) + stepv[:, 2] ** 2)
    dist_twin = np.cumsum(norm)
    hp = stepv.astype(R.HP)
    dist_truth = np.cumsum(np.sqrt(hp[:, 0] ** 2 + hp[:, 1] ** 2 + hp[:, 2] ** 2))
    scaling = np.sum(X * Y) / np.sum(X ** 2)
    sq_twin = np.sqrt(((Y - X) ** 2).sum(axis=1)) ** 2
    sq_truth = ((Y.astype(R.HP) - X.astype(R.HP)) ** 2).sum(axis=1)
    ate_truth = np.sqrt(sq_truth.mean())
    tol_ate = R.mean_bound(sq_twin, sq_truth, sq_truth.mean()) / (2 * float(ate_truth)) + U52 * float(ate_truth)
    first, length, last = R.segment_frames(dist_twin)
    keep = R.decision_margins(dist_twin) >= 1e-6
    left_out = int((~keep).sum())
    assert left_out <= 1e-3 * len(keep) and (last >= 0).sum() > 800000
    t_host = time.perf_counter() - t0
    # the launch
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    seg = torch.full((ops.traj_segments(n), 6), SENTINEL, dtype=torch.float64, device=dev)
    dist = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
    out = torch.full((8,), SENTINEL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.traj_metrics(p, g, out=out, segments=seg, dist=dist)
    torch.cuda.synchronize()
    t_kernel = time.perf_counter() - t0
    out, seg, dist = out.cpu().numpy(), seg.cpu().numpy(), dist.cpu().numpy()
    e_dist, b_dist = T._dev(dist, dist_truth), n * U52 * float(dist_truth[-1])
    e_ate = abs(float(R.HP(out[3]) - ate_truth))
    print(f'[traj_kernels hip] n = {n}: references {t_host:.2f} s, traj_metrics (first launch, scratch allocation included) '
          f'{t_kernel * 1e3:.1f} ms; rows left out {left_out} of {len(keep)}')
    T._row('hip', f'n={n}', 'dist max', e_dist, T._dev(dist_twin, dist_truth), b_dist)
    T._row('hip', f'n={n}', 'ate', e_ate, abs(float(R.HP(np.sqrt(sq_twin.mean())) - ate_truth)), tol_ate)
    assert T._bits(out[6]) == T._bits(scaling)
    assert e_dist <= b_dist and (np.diff(dist) >= 0).all() and out[7] == dist[-1]
    assert e_ate <= tol_ate
    assert np.array_equal(seg[:, 0], first) and np.array_equal(seg[:, 3], length)
    assert np.array_equal(seg[keep, 5], last[keep])
    assert out[2] == (seg[:, 5] >= 0).sum() and abs(out[2] - (last >= 0).sum()) <= left_out
