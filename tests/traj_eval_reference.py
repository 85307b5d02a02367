"""TEST INFRASTRUCTURE: the trajectory evaluators of the reference (slam/utils.py:129-383) restated in numpy, twice.

  the twin    float64, with the reference's own operations in the reference's own order (np.linalg.inv and `@` on one 4x4 at a
              time, np.linalg.norm, Python-loop accumulation, np.mean): tests/golden/traj_eval.npz pins it to the real module to
              the last bit.  It is the yardstick of the kernel-level tests.
  the truth   the same formulae in numpy.longdouble (64-bit significand on x86), batched; the 4x4 inverse is a Gauss-Jordan
              elimination with partial pivoting written out here, because LAPACK has no extended precision.

    evaluate(pred, gt, optimize_scale=False, hp=False) -> dict     everything one clslam_traj_metrics launch produces
    pair_errors(a, b, a_inverted, hp=False) -> (n,2)                clslam_pose_pair_error
    calc_error(pred, gt, optimize_scale=False) -> str               the reference's log text, from the twin
    make_fixture(n, seed) / tile(poses, n)                          the seeded drive of the tests and of the golden file

Nothing here runs on the device; the kernels are checked against it."""
import functools

import numpy as np

LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)
STEP = 10
HP = np.longdouble
OUT_KEYS = ('t_err', 'r_err', 'n_segments', 'ate', 'rpe_trans', 'rpe_rot', 'scaling', 'path_length')


# ---- the two error measures ---------------------------------------------------------------------------------------------
def rotation_error(m):
    d = 0.5 * (m[0, 0] + m[1, 1] + m[2, 2] - 1.0)
    return np.arccos(max(min(d, 1.0), -1.0))


def translation_error(m):
    dx, dy, dz = m[0, 3], m[1, 3], m[2, 3]
    return np.sqrt(dx**2 + dy**2 + dz**2)


def _errors_hp(M):
    """(N,4,4) longdouble -> (N,2) [translation_error, rotation_error]"""
    d = HP(0.5) * (M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2] - HP(1))
    rot = np.arccos(np.clip(d, HP(-1), HP(1)))
    tr = np.sqrt(M[:, 0, 3]**2 + M[:, 1, 3]**2 + M[:, 2, 3]**2)
    return np.stack([tr, rot], axis=1)


def inv_hp(A):
    """(N,4,4) longdouble -> the inverses, Gauss-Jordan with partial pivoting"""
    A = np.array(A, dtype=HP)
    N = len(A)
    B = np.broadcast_to(np.eye(4, dtype=HP), (N, 4, 4)).copy()
    idx = np.arange(N)
    for k in range(4):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        for X in (A, B):
            row = X[idx, k].copy()
            X[idx, k] = X[idx, p]
            X[idx, p] = row
        piv = A[:, k, k].copy()
        A[:, k] /= piv[:, None]
        B[:, k] /= piv[:, None]
        for r in range(4):
            if r != k:
                f = A[:, r, k].copy()
                A[:, r] -= f[:, None] * A[:, k]
                B[:, r] -= f[:, None] * B[:, k]
    return B


def _as_poses(x, dtype=np.float64):
    a = np.asarray(x, dtype=dtype)
    return a.reshape(-1, 4, 4)


# ---- distances and the segment decisions --------------------------------------------------------------------------------
def distances(gt, hp=False):
    """utils.py:164-172: the running sum of the step norms, (n,)"""
    gt = _as_poses(gt, HP if hp else np.float64)
    xyz = gt[:, :3, 3]
    dist = np.zeros(len(gt), dtype=gt.dtype)
    for i in range(1, len(gt)):
        step = xyz[i] - xyz[i - 1]
        dist[i] = dist[i - 1] + (np.sqrt(step[0]**2 + step[1]**2 + step[2]**2) if hp else np.linalg.norm(step))
    return dist


def last_frame_linear(dist, first, length):
    """utils.py:175-188 as written: the linear scan"""
    for i in range(first, len(dist)):
        if dist[i] > dist[first] + length:
            return i
    return -1


def segment_frames(dist):
    """-> first (S,), length (S,), last (S,) for S = ceil(n/10)*8 rows in the reference's loop order; the scan as one
    searchsorted per row (dist is non-decreasing: the first index right of dist[first] + length is the scan's answer)"""
    n = len(dist)
    first = np.repeat(np.arange(0, n, STEP), len(LENGTHS))
    length = np.tile(np.asarray(LENGTHS, dtype=np.float64), (n + STEP - 1) // STEP)
    if n == 0:
        return first, length, np.zeros(0, dtype=np.int64)
    last = np.searchsorted(dist, dist[first] + length.astype(dist.dtype), side='right')
    last = np.where(last >= n, -1, last)
    return first, length, last.astype(np.int64)


def decision_margins(dist):
    """per row, the smallest |dist[i] - (dist[first] + length)| over all frames"""
    first, length, _ = segment_frames(dist)
    limit = dist[first] + length
    j = np.clip(np.searchsorted(dist, limit), 1, len(dist) - 1)
    return np.minimum(np.abs(dist[j] - limit), np.abs(dist[j - 1] - limit))


def decision_margin(dist):
    """the smallest |dist[i] - (dist[first] + length)| over all rows and frames: how far the segment decisions are from rounding"""
    return float(decision_margins(dist).min())


def poses_from_xyz(xyz):
    """(n,3) -> (n,4,4) float64 poses with identity rotations"""
    xyz = np.asarray(xyz, dtype=np.float64)
    p = np.broadcast_to(np.eye(4), (len(xyz), 4, 4)).copy()
    p[:, :3, 3] = xyz
    return p


def lu_inverse(a, tie='first'):
    """A 4x4 inverse in plain Python floats (binary64, every operation rounded on its own), as csrc/traj_eval.hip documents its
    own: LU with partial pivoting on [A | I], the pivot of column k being the FIRST row r >= k of the largest |a[r][k]|
    (tie='last': the last such row -- a deliberately different rule, for the tests that show they can tell the two apart), then
    back substitution.  -> (inverse as a 4x4 list, [p0, p1, p2, p3] the pivot rows chosen)"""
    a = [[float(x) for x in row] for row in a]
    b = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    pivots = []
    for k in range(4):
        p, best = k, abs(a[k][k])
        for r in range(k + 1, 4):
            v = abs(a[r][k])
            if v > best or (tie == 'last' and v == best):
                best, p = v, r
        pivots.append(p)
        a[k], a[p] = a[p], a[k]
        b[k], b[p] = b[p], b[k]
        for r in range(k + 1, 4):
            f = a[r][k] / a[k][k]
            for j in range(k + 1, 4):
                a[r][j] -= f * a[k][j]
            for j in range(4):
                b[r][j] -= f * b[k][j]
    for k in range(3, -1, -1):
        for j in range(4):
            s = b[k][j]
            for c in range(k + 1, 4):
                s -= a[k][c] * b[c][j]
            b[k][j] = s / a[k][k]
    return b, pivots


# ---- one evaluation -----------------------------------------------------------------------------------------------------
def scale_factor(pred, gt, hp=False):
    dt = HP if hp else np.float64
    X, Y = _as_poses(pred, dt)[:, :3, 3], _as_poses(gt, dt)[:, :3, 3]
    return np.sum(X * Y) / np.sum(X**2)


def pairwise_tree_sum(a):
    """numpy's pairwise summation (pairwise_sum of its add loop) as ONE tree over a 1-D float64 array: more than 128 elements are
    split at half the length rounded down to a multiple of 8; a leaf of 8..128 runs eight interleaved accumulators, then the
    remainder one by one; fewer than 8 are added one by one.  np.sum IS this for up to 8192 elements (numpy's buffer size);
    beyond, numpy sums each 8192-element piece this way and adds the pieces in order -- so for longer arrays this function is
    NOT np.sum, and the tests use it to show that they can tell the two apart."""
    n = len(a)
    if n > 128:
        h = n // 2
        h -= h % 8
        return pairwise_tree_sum(a[:h]) + pairwise_tree_sum(a[h:])
    m = n - n % 8 if n >= 8 else 0
    res = np.float64(0.0)
    if m:
        r = a[:8].copy()
        for i in range(8, m, 8):
            r = r + a[i:i + 8]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[m:]:
        res = res + x
    return res


def pair_errors(a, b, a_inverted=False, hp=False):
    """(n,2) [translation_error, rotation_error] of inv(b_i) @ (inv(a_i) if a_inverted else a_i)"""
    if hp:
        a, b = _as_poses(a, HP), _as_poses(b, HP)
        if len(a) == 0:
            return np.zeros((0, 2), dtype=HP)
        return _errors_hp(inv_hp(b) @ (inv_hp(a) if a_inverted else a))
    a, b = _as_poses(a), _as_poses(b)
    out = np.zeros((len(a), 2))
    for i in range(len(a)):
        e = np.linalg.inv(b[i]) @ (np.linalg.inv(a[i]) if a_inverted else a[i])
        out[i] = translation_error(e), rotation_error(e)
    return out


def evaluate(pred, gt, optimize_scale=False, hp=False):
    dt = HP if hp else np.float64
    pred, gt = _as_poses(pred, dt), _as_poses(gt, dt)
    n = len(gt)
    r = {}
    with np.errstate(all='ignore'):
        r['scaling'] = scale_factor(pred, gt, hp) if n else dt(np.nan)
    scaled = pred
    if optimize_scale:
        scaled = pred.copy()
        scaled[:, :3, 3] *= r['scaling']
    dist = r['dist'] = distances(gt, hp)
    first, length, last = segment_frames(dist)
    seg = np.full((len(first), 6), np.nan, dtype=dt)
    seg[:, 0], seg[:, 3], seg[:, 5] = first, length, last
    ok = np.nonzero(last >= 0)[0]
    f, l = first[ok], last[ok]
    if hp:
        if len(ok):
            e = _errors_hp(inv_hp(inv_hp(scaled[f]) @ scaled[l]) @ (inv_hp(gt[f]) @ gt[l]))
            seg[ok, 1], seg[ok, 2] = e[:, 1] / length[ok], e[:, 0] / length[ok]
    else:
        for k, a, b in zip(ok, f, l):
            delta_gt = np.linalg.inv(gt[a]) @ gt[b]
            delta_pred = np.linalg.inv(scaled[a]) @ scaled[b]
            e = np.linalg.inv(delta_pred) @ delta_gt
            seg[k, 1], seg[k, 2] = rotation_error(e) / length[k], translation_error(e) / length[k]
    seg[ok, 4] = length[ok] / (0.1 * (l - f + 1))
    r['segments'], r['n_segments'] = seg, len(ok)
    if hp:
        r['t_err'] = seg[ok, 2].sum() / len(ok) if len(ok) else HP(0)
        r['r_err'] = seg[ok, 1].sum() / len(ok) if len(ok) else HP(0)
    else:                                                   # utils.py:292-314: a running Python sum in row order
        t_sum = r_sum = 0
        for k in ok:
            r_sum += seg[k, 1]
            t_sum += seg[k, 2]
        r['t_err'], r['r_err'] = (t_sum / len(ok), r_sum / len(ok)) if len(ok) else (0, 0)
    # ATE and RPE on the UNSCALED prediction (utils.py:374,378)
    if hp:
        r['ate_sq'] = ((gt[:, :3, 3] - pred[:, :3, 3])**2).sum(axis=1)
        r['pairs'] = (_errors_hp(inv_hp(inv_hp(gt[:-1]) @ gt[1:]) @ (inv_hp(pred[:-1]) @ pred[1:])) if n > 1
                      else np.zeros((0, 2), dtype=HP))
    else:
        errors = [np.sqrt(np.sum((g[:3, 3] - p[:3, 3])**2)) for p, g in zip(pred, gt)]
        r['ate_sq'] = np.asarray(errors, dtype=np.float64)**2
        pairs = np.zeros((max(n - 1, 0), 2))
        for i in range(n - 1):
            gt_rel = np.linalg.inv(gt[i]) @ gt[i + 1]
            pred_rel = np.linalg.inv(pred[i]) @ pred[i + 1]
            e = np.linalg.inv(gt_rel) @ pred_rel
            pairs[i] = translation_error(e), rotation_error(e)
        r['pairs'] = pairs
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            r['ate'] = np.sqrt(np.mean(r['ate_sq']))
            r['rpe_trans'], r['rpe_rot'] = np.mean(r['pairs'][:, 0]), np.mean(r['pairs'][:, 1])
    r['path_length'] = dist[-1] if n else dt(0)
    return r


def sequence_errors(r):
    """the reference's list layout: [first_frame, rot, trans, length, speed] of the rows that have a last frame"""
    return [[int(s[0]), s[1], s[2], int(s[3]), s[4]] for s in r['segments'] if s[5] >= 0]


def calc_error(pred, gt, optimize_scale=False):
    """utils.py:357-383 from the twin's numbers"""
    r = evaluate(pred, gt, optimize_scale)
    return format_log(r, optimize_scale)


def format_log(r, optimize_scale):
    log = ''
    if optimize_scale:
        log += '-' * 10 + ' MEDIAN\n'
        log += f'Scaling: {r["scaling"]}'
    log += '-' * 10 + '\n'
    log += f'Trans error (%):      {r["t_err"] * 100:.4f}\n'
    log += f'Rot error (deg/100m): {100 * r["r_err"] / np.pi * 180:.4f}\n'
    log += f'Abs traj RMSE (m):    {r["ate"]:.4f}\n'
    log += f'Rel pose error (m):   {r["rpe_trans"]:.4f}\n'
    log += f'Rel pose err (deg):   {r["rpe_rot"] * 180 / np.pi:.4f}\n'
    log += '-' * 10 + '\n'
    return log


# ---- bounds -------------------------------------------------------------------------------------------------------------
def element_bound(twin, truth):
    """largest absolute deviation of the twin from the truth over an array (NaN where both are NaN is no deviation)"""
    d = np.abs(np.asarray(twin, dtype=HP) - truth)
    return float(np.nanmax(d)) if d.size and not np.isnan(d).all() else 0.0


def mean_bound(twin_terms, truth_terms, truth_mean):
    """the project's rule for a sum (tests/test_depth_metrics.py): 4 x the mean of the twin's per-term errors plus the final
    rounding of the result, 2 x 2^-53 relative"""
    e = np.abs(np.asarray(twin_terms, dtype=HP) - truth_terms)
    return 4.0 * float(e.mean()) + 2.0**-52 * abs(float(truth_mean))


# ---- the fixture --------------------------------------------------------------------------------------------------------
def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


@functools.lru_cache(maxsize=None)
def make_fixture(n=1000, seed=0, mean_step=1.0):
    """-> pred, gt (n,4,4) float64.  gt: a smooth drive in camera axes (z forward): yaw a random walk of sigma 0.02 rad, pitch a
    gentle sinusoid, steps uniform in mean_step * [0.8, 1.2] m.  pred: gt's relative motions with a small rotation noise and a 2 %
    scale error, composed in float32 and cast back, so its rotation blocks are not orthonormal."""
    rng = np.random.default_rng(seed)
    yaw = np.cumsum(rng.normal(0.0, 0.02, n))
    pitch = 0.03 * np.sin(np.arange(n) * (2 * np.pi / 240.0))
    steps = mean_step * rng.uniform(0.8, 1.2, n)
    gt = np.zeros((n, 4, 4))
    gt[:, 3, 3] = 1.0
    pos = np.zeros(3)
    for i in range(n):
        R = _rot_y(yaw[i] - yaw[0]) @ _rot_x(pitch[i])
        if i:
            pos = pos + R @ np.array([0.0, 0.0, steps[i]])
        gt[i, :3, :3], gt[i, :3, 3] = R, pos
    noise = rng.normal(0.0, 2e-3, (n, 3))
    pred32 = np.zeros((n, 4, 4), dtype=np.float32)
    pred32[0] = gt[0].astype(np.float32)
    for i in range(1, n):
        rel = np.linalg.inv(gt[i - 1]) @ gt[i]
        rel[:3, :3] = _rot_z(noise[i, 2]) @ _rot_y(noise[i, 1]) @ _rot_x(noise[i, 0]) @ rel[:3, :3]
        rel[:3, 3] *= 1.02
        pred32[i] = pred32[i - 1] @ rel.astype(np.float32)
    pred = pred32.astype(np.float64)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


def tile(poses, n):
    """continue a trajectory that starts at the identity to n poses by replaying its own relative motions"""
    poses = np.asarray(poses, dtype=np.float64)
    m = len(poses)
    rel = [np.linalg.inv(poses[i - 1]) @ poses[i] for i in range(1, m)]
    out = np.zeros((n, 4, 4))
    out[:min(m, n)] = poses[:n]
    for k in range(m, n):
        out[k] = out[k - 1] @ rel[(k - m) % (m - 1)]
    return out
