"""The pose-graph kernels of csrc/pose_graph.hip one at a time (ops.pgo_edge_eval, pgo_build_system, pgo_solve,
pgo_update_score), each against a reference that is better than the kernel: numpy.longdouble for the chart, the Jacobians
and the scores, dense float64 algebra for the assembly, a direct sparse solve and a plain numpy PCG with an exact block-
tridiagonal preconditioner (tests/pgo_reference.py) for the solver.  Nothing here goes through a converged Levenberg run
except where it says so: a converged optimum forgives a wrong step and a weak preconditioner.

Every tolerance below is either an identity (bitwise), the fp64 figure its docstring derives, or 4x what the REFERENCE
alone achieves on the same input (computed in the test, before the kernel's result is looked at).  None was tuned to a
kernel result.  emu = the kernel sources on the CPU emulator (256-thread workgroup), hip = gfx950 (512 threads)."""
import numpy as np
import pytest
import torch

import pgo_reference as R
from emu_util import BACKENDS, use_backend

EPS = float(np.finfo(np.float64).eps)
CG_TOL = 1e-10


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


def _random_pose(rng, big=False):
    T = np.eye(4)
    T[:3, :3] = R._rot(*rng.uniform(-np.pi, np.pi, 3)) if big else R._rot(*rng.normal(0, 0.3, 3))
    T[:3, 3] = rng.normal(0, 3, 3)
    return T


def _edge_eval(device, X, ev, Z):
    from clslam_hip import ops
    n = len(ev)
    err, ja, jb = (torch.full((n, c), float('nan'), dtype=torch.float64, device=device) for c in (6, 36, 36))
    ops.pgo_edge_eval(_dev(X.reshape(-1, 16), device), _dev(np.asarray(ev, dtype=np.int32), device),
                      _dev(Z.reshape(-1, 16), device), err, ja, jb, 0)
    return err.cpu().numpy(), ja.cpu().numpy().reshape(n, 6, 6), jb.cpu().numpy().reshape(n, 6, 6)


# ---- 1. chart, error, Jacobians ------------------------------------------------------------------------------------------
# (w, x, y, z) before normalisation, the branch of the matrix -> quaternion conversion it must take (0: trace > 0, 1 + i:
# trace <= 0 with the largest diagonal entry at i), exact half turn?
_LOG_CASES = [
    ((0.9, 0.1, -0.3, 0.2), 0, False), ((-0.8, 0.3, 0.1, -0.4), 0, False), ((1.0, 0.0, 0.0, 0.0), 0, False),
    ((0.2, 0.9, 0.3, 0.2), 1, False), ((-0.2, 0.9, -0.3, 0.2), 1, False),
    ((0.3, 0.2, 0.9, -0.1), 2, False), ((-0.1, -0.2, 0.9, 0.3), 2, False),
    ((0.25, -0.3, 0.1, 0.9), 3, False), ((-0.3, 0.1, 0.3, -0.9), 3, False),
    ((0.0, 1.0, 0.0, 0.0), 1, True), ((0.0, 0.0, 1.0, 0.0), 2, True), ((0.0, 0.0, 0.0, 1.0), 3, True),
    ((0.0, 2.0, 2.0, 1.0), 1, True), ((0.0, 1.0, 3.0, -2.0), 2, True), ((0.0, -1.0, 2.0, 3.0), 3, True),
    # trace = 4 w^2 - 1 = +-5e-13: w = 0.5 (1 +- 2.5e-13), the rest of the norm on an oblique axis
    ((0.5 * (1 + 2.5e-13), 0.7, 0.1, 0.5), 0, False), ((0.5 * (1 - 2.5e-13), 0.7, 0.1, 0.5), 1, False),
    ((-0.5 * (1 + 2.5e-13), 0.1, 0.3, 0.8), 0, False), ((-0.5 * (1 - 2.5e-13), 0.1, 0.3, 0.8), 3, False),
]


def _log_case_pose(q, t):
    q = np.asarray(q, dtype=np.longdouble)
    if abs(abs(q[0]) - 0.5) < 1e-6:                    # the near-zero-trace cases: w is kept, xyz scaled to unit norm
        q = np.concatenate([q[:1], q[1:] * np.sqrt((1 - q[0] * q[0]) / (q[1:] * q[1:]).sum())])
    return R.quat_to_pose(q, t)


@pytest.mark.parametrize('backend', BACKENDS)
def test_log_known_answers(backend):
    """Z = I, Xi = I, Xj = [R(q) t]: the error is (t, sign(w) q_xyz), the expected value taken from q (formed in longdouble),
    never from log_mqt.  All four branches of iso_log (checked on the reference side with quat_branch), exact half turns
    about x, y, z and oblique axes (w = 0: the kernel keeps the sign in which the pivot component q_i is positive; the cases
    are written that way), trace within 1e-12 of 0 from both sides.
    Tolerance 1e-12 (the file's figure): R(q) is rounded to fp64 entry by entry (<= 1.1e-16 each); every branch recovers q
    from sums of <= 4 entries divided by 4 |q_pivot| >= 2 (pivot >= 0.5), so the error is a few 1e-16."""
    device = use_backend(backend)
    rng = np.random.default_rng(5)
    X, ev, expect = [np.eye(4)], [], []
    for q, branch, half in _LOG_CASES:
        t = rng.normal(0, 3, 3)
        T, qn = _log_case_pose(q, t)
        assert R.quat_branch(T[:3, :3]) == branch, (q, R.quat_branch(T[:3, :3]))
        tr = np.trace(T[:3, :3])
        if abs(abs(q[0]) - 0.5) < 1e-6:
            assert 0 < abs(tr) < 1e-12
        if half:
            assert qn[0] == 0.0 and np.array_equal(T[:3, :3], T[:3, :3].T) and qn[branch] > 0
        sign = -1.0 if qn[0] < 0 else 1.0
        expect.append(np.concatenate([t, sign * qn[1:]]))
        ev.append((0, len(X)))
        X.append(T)
    assert {b for _, b, _ in _LOG_CASES} == {0, 1, 2, 3}
    X, expect = np.stack(X), np.stack(expect)
    Z = np.tile(np.eye(4), (len(ev), 1, 1))
    err, _, _ = _edge_eval(device, X, ev, Z)
    print('known-answer log: max error', np.abs(err - expect).max())
    assert np.abs(err - expect).max() <= 1e-12


@pytest.mark.parametrize('backend', BACKENDS)
def test_log_random_frames(backend):
    """The same relative poses as Z^-1 Xi^-1 Xj with random Xi and Z (equal to the known pose up to rounding) against
    edge_error, 1e-12.  For the exact half turns the rounding of the three products decides the sign of w = +-1e-16, so q
    and -q are the same answer there and the quaternion part is compared up to that one global sign; everything else is
    compared as it is.  The reference must take every branch here too."""
    device = use_backend(backend)
    rng = np.random.default_rng(6)
    X, ev, Zs, halfs = [], [], [], []
    for q, _, half in _LOG_CASES:
        T, _ = _log_case_pose(q, rng.normal(0, 1, 3))
        Xi, Z = _random_pose(rng, big=True), _random_pose(rng, big=True)
        ev.append((len(X), len(X) + 1))
        X += [Xi, Xi @ Z @ T]
        Zs.append(Z); halfs.append(half)
    X, Zs, ev, halfs = np.stack(X), np.stack(Zs), np.array(ev), np.array(halfs)
    ref = R.edge_error(X[ev[:, 0]], X[ev[:, 1]], Zs)
    rel = R.inv(Zs) @ R.inv(X[ev[:, 0]]) @ X[ev[:, 1]]
    assert {R.quat_branch(M[:3, :3]) for M in rel} == {0, 1, 2, 3}
    err, _, _ = _edge_eval(device, X, ev, Zs)
    dq = np.abs(err[:, 3:] - ref[:, 3:]).max(axis=1)
    dq_flip = np.abs(err[:, 3:] + ref[:, 3:]).max(axis=1)
    dq = np.where(halfs, np.minimum(dq, dq_flip), dq)
    print('random-frame log: max error t', np.abs(err[:, :3] - ref[:, :3]).max(), 'q', dq.max())
    assert np.abs(err[:, :3] - ref[:, :3]).max() <= 1e-12 and dq.max() <= 1e-12


def _jacobian_edges():
    """24 random edges between poses with arbitrary rotations (the set test_pose_graph.py uses), every fourth within 1e-3 ..
    2e-2 rad of a half turn, plus 3 deliberately exact half turns (within 1e-5 rad: left out of the Jacobian check)"""
    rng = np.random.default_rng(7)
    n = 24
    X = [_random_pose(rng, big=True) for _ in range(n)]
    ev, Z = [], []
    for k in range(n):
        j = (k + 1 + k % 5) % n
        z = R.inv(X[k]) @ X[j] @ _random_pose(rng)
        if k % 4 == 0:
            flip = np.eye(4)
            flip[:3, :3] = R._rot(*np.roll([np.pi - 1e-3 * (1 + k), 0.0, 0.0], k // 4))
            z = R.inv(X[k]) @ X[j] @ flip
        ev.append((k, j)); Z.append(z)
    for axis in ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.0, 2.0, -1.0, 2.0)):
        T, _ = R.quat_to_pose(axis, rng.normal(0, 1, 3))
        ev.append((len(X), len(X) + 1)); Z.append(_random_pose(rng))
        X += [_random_pose(rng, big=True), None]
        X[-1] = X[-2] @ Z[-1] @ T
    return np.stack(X), np.array(ev), np.stack(Z), n


def _jacobian_floor(X, ev, Z, n):
    A64, B64 = R.jacobians(X[ev[:n, 0]], X[ev[:n, 1]], Z[:n])
    Ahp, Bhp = R.jacobians_hp(X[ev[:n, 0]], X[ev[:n, 1]], Z[:n])
    return float(max(np.abs(A64 - Ahp).max(), np.abs(B64 - Bhp).max())), Ahp, Bhp


@pytest.mark.parametrize('backend', BACKENDS)
def test_jacobians_against_longdouble(backend):
    """A, B of pgo_edge_eval against jacobians_hp (the central difference in longdouble end to end, step 2^-21).
    floor = max |R.jacobians - jacobians_hp| over the same edges: what an fp64 central difference at step 1e-6 loses to
    rounding (eps |e| / h; |e| is up to ~10 m here).  Measured on the host: 1.16e-9.  The kernel's tolerance is 4 x floor =
    4.6e-9 (it orders the products differently; 4x covers that and nothing more), computed from the reference at run time
    and required to stay below 1e-8 so that it cannot drift up unnoticed.  The test before this change allowed 1e-7.
    The 3 constructed exact half turns (relative rotation within 1e-5 rad of pi) are left out of the Jacobian check: the
    w >= 0 sign flip makes e discontinuous there and a central difference meaningless in both implementations.  Their error
    is checked (up to the sign of q, as in test_log_random_frames); every random edge, the 6 near-half-turn ones (1e-3 rad
    and more away) included, is in."""
    device = use_backend(backend)
    X, ev, Z, n = _jacobian_edges()
    rel = R.inv(Z) @ R.inv(X[ev[:, 0]]) @ X[ev[:, 1]]
    ang = np.array([2 * np.arcsin(min(1.0, abs(w))) for w in
                    [np.sqrt(max(0.0, 1 - (R.log_mqt(M[None])[0, 3:] ** 2).sum())) for M in rel]])   # distance from a half turn
    assert (ang[:n] > 1e-5).all() and (ang[n:] <= 1e-5).all() and (ang[:n] < 0.03).sum() >= 6
    floor, Ahp, Bhp = _jacobian_floor(X, ev, Z, n)
    tol = 4 * floor
    assert 1e-11 < floor and tol < 1e-8, floor
    err, A, B = _edge_eval(device, X, ev, Z)
    e_hp = R.edge_error_hp(X[ev[:, 0]], X[ev[:, 1]], Z).astype(np.float64)
    assert np.abs(err[:n] - e_hp[:n]).max() <= 1e-12
    dq = np.minimum(np.abs(err[n:, 3:] - e_hp[n:, 3:]).max(axis=1), np.abs(err[n:, 3:] + e_hp[n:, 3:]).max(axis=1))
    assert np.abs(err[n:, :3] - e_hp[n:, :3]).max() <= 1e-12 and dq.max() <= 1e-12
    dA, dB = np.abs(A[:n] - Ahp).max(), np.abs(B[:n] - Bhp).max()
    print(f'jacobians: fp64 reference floor {floor:.3g}, tolerance {tol:.3g}, kernel {float(dA):.3g} / {float(dB):.3g}')
    assert dA <= tol and dB <= tol


_NV_UPDATE = 2 * 512 + 3 + 40


def _update_inputs():
    """1067 slots (more than two passes of a 512-thread workgroup): fixed and isolated ones scattered among the active, the
    active index a random permutation (not monotone in the slot), increments with |qxyz|^2 > 1, = 1 exactly, just below 1"""
    rng = np.random.default_rng(12)
    nv = _NV_UPDATE
    X = np.stack([_random_pose(rng, big=True) for _ in range(nv)])
    X[0], X[1] = np.eye(4), np.eye(4)
    X[1][0, 3] = 2.0                                      # with Z = I, Omega = I: e = (2, 0, 0, 0, 0, 0), chi2 = 4 exactly
    kind = rng.choice(3, nv, p=[0.8, 0.1, 0.1])          # 0 active, 1 fixed, 2 isolated
    kind[:2] = 1
    kind[-3:] = (0, 1, 0)                                 # the last pass has both
    slots = np.nonzero(kind == 0)[0]
    act = np.full(nv, -1, dtype=np.int32)
    act[slots] = rng.permutation(len(slots)).astype(np.int32)
    na = len(slots)
    d = np.concatenate([rng.normal(0, 0.5, (na, 3)), rng.normal(0, 0.25, (na, 3))], axis=1)
    one = np.nextafter(1.0, 0.0)
    special = [(0.8, 0.5, 0.4), (0.9, 0.5, 0.1), (-0.7, 0.7, 0.3),            # |q|^2 > 1: identity rotation
               (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0),              # = 1 exactly: w = 0, a half turn
               # just below 1.  w = sqrt(1 - |q|^2) amplifies a rounding error of |q|^2 by 1 / (2 w): one nonzero
               # component squares to the same fp64 number however the sum is fused; the mixed ones keep w >= 1.4e-3, i.e.
               # an error of 1.1e-16 / 2.8e-3 = 4e-14 in w
               (one, 0.0, 0.0), (0.0, 0.0, -one), (0.6 * (1 - 1e-6), 0.8 * (1 - 1e-6), 0.0), (0.5, -0.5, np.sqrt(0.5) - 2e-6),
               (0.0, 0.0, 0.0)]
    d[:len(special), 3:] = special
    # edges: a chain over the non-isolated slots plus random pairs; edge 0 joins the two fixed slots 0 and 1
    live = np.nonzero(kind != 2)[0]
    ev = [(0, 1)] + [(live[k], live[k + 1]) for k in range(1, len(live) - 1)] + \
         [tuple(rng.choice(live[2:], 2, replace=False)) for _ in range(300)]
    ev = np.array(ev, dtype=np.int32)
    return X, kind, act, d, ev


@pytest.mark.parametrize('backend', BACKENDS)
def test_update_and_score(backend):
    """pgo_update_score with a delta, one launch, 1067 slots and 1300+ edges (three passes of every strided loop on both
    backends).  trial against R.oplus at 1e-12 (the existing figure: two 3x3 products and one orthonormalisation step of
    O(1) entries, errors of a few 1e-16 times |t| <= 15); fixed and isolated slots bitwise copies.
    The score against R.robust_chi2_hp (longdouble) evaluated at the kernel's own trial poses, with and without `robust`:
    1e-12 relative.  Derivation: e carries an absolute error of <= ~40 eps max|t| = 1e-13 (three 4x4 products), the edges
    here have |e| ~ 1, so each e^T Omega e is off by <= ~3e-13 relative, the terms are all positive and the tree sum adds
    log2(n) eps.  Reference-only check first: the float64 R.robust_chi2 itself must be within 2.5e-13 (a quarter of the
    bound) of the longdouble value.  Huber deltas put edges on both sides of s = delta^2 and edge 0 exactly on it."""
    device = use_backend(backend)
    from clslam_hip import ops
    X, kind, act, d, ev = _update_inputs()
    nv, ne = len(X), len(ev)
    rng = np.random.default_rng(13)
    noise = np.stack([R.exp_mqt(np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 0.1, 3)])[None])[0] for _ in range(ne)])
    Z = R.inv(X[ev[:, 0]]) @ X[ev[:, 1]] @ noise
    Z[0] = np.eye(4)
    L = rng.normal(size=(ne, 6, 6)) * 0.4 + np.eye(6)
    info = L @ np.swapaxes(L, 1, 2)
    info[0] = np.eye(6)
    delta = np.where(rng.random(ne) < 0.3, -1.0, rng.uniform(0.5, 4.0, ne))
    delta[0] = 2.0
    t = {k: _dev(v, device) for k, v in dict(est=X.reshape(-1, 16), act=act, d=d, ev=ev, meas=Z.reshape(-1, 16),
                                             info=info.reshape(-1, 36), delta=delta).items()}
    scal = torch.full((8,), float('nan'), dtype=torch.float64, device=device)
    trial = torch.full((nv, 16), float('nan'), dtype=torch.float64, device=device)
    ops.pgo_update_score(t['est'], trial, t['act'], nv, t['d'], t['ev'], t['meas'], t['info'], t['delta'], ne, 1, scal, 6, 0)
    ops.pgo_update_score(t['est'], trial, t['act'], nv, t['d'], t['ev'], t['meas'], t['info'], t['delta'], ne, 0, scal, 2, 0)
    ops.pgo_update_score(t['est'], trial, t['act'], nv, None, t['ev'], t['meas'], t['info'], t['delta'], ne, 1, scal, 4, 0)
    T = trial.cpu().numpy().reshape(-1, 4, 4)
    s = scal.cpu().numpy()
    assert np.isnan(s[[0, 1, 3, 5, 7]]).all()              # only the requested slots are written
    ref = X.copy()
    ref[act >= 0] = R.oplus(X[act >= 0], d[act[act >= 0]])
    assert np.allclose(R.exp_mqt(d[:1])[0, :3, :3], np.eye(3)) and (np.diff(act[act >= 0]) < 0).any()
    print('update: max |trial - oplus|', np.abs(T - ref).max())
    assert np.abs(T - ref).max() <= 1e-12
    assert np.array_equal(T[act < 0], X[act < 0]) and (kind[act < 0] > 0).all() and (kind == 1).any() and (kind == 2).any()
    # scores
    g = R.Graph(np.arange(nv), X, kind == 1, ev, Z, info, delta)
    for poses, robust, out in ((T, True, 6), (T, False, 2), (X, True, 4)):
        hp = R.robust_chi2_hp(g, poses, robust)
        s_terms = R.chi2_terms(g, poses)[1]
        if robust:
            on = s_terms[delta > 0] > delta[delta > 0] ** 2
            assert on.sum() > 50 and (~on).sum() > 50 and (poses is T or s_terms[0] == delta[0] ** 2 == 4.0)
        f64 = float(R.huber(s_terms, delta)[0].sum()) if robust else float(s_terms.sum())
        ref_only = abs(f64 - hp) / hp
        print(f'score[{out}]: kernel {s[out]!r}, longdouble {float(hp)!r}, float64 numpy off by {float(ref_only):.2g} relative')
        assert ref_only <= 2.5e-13
        assert abs(s[out] - hp) <= 1e-12 * hp


# ---- 2. assembly ---------------------------------------------------------------------------------------------------------
def _assembly_graph(variant):
    """Small graphs of every shape the contribution lists have to get right (see test_assembly)"""
    rng = np.random.default_rng(100 + variant)
    if variant == 3:                                      # 40 vertices, 3 loops, shuffled insertion
        d = R.make_graph(40, 3, seed=40, start_id=5, lap=28)
        d['insert'] = rng.permutation(40)
        d['delta'] = None
        return d
    n = 14
    ids = np.array([-9, -4, -1, 0, 3, 4, 10, 11, 12, 20, 33, 34, 50, 71])[:n]      # rising, non-contiguous, negative
    gt = np.stack([_random_pose(rng, big=True) for _ in range(n)])
    fixed = np.zeros(n, dtype=bool)
    iso = 9                                               # index 9 (id 20) is isolated: in no edge
    chain = [k for k in range(n) if k != iso]
    edges = [(chain[k], chain[k + 1]) for k in range(len(chain) - 1)]
    if variant == 0:
        fixed[0] = True
        edges += [(2, 3), (3, 2), (3, 2)]                 # with the chain's (2, 3): three and more between one pair, both ways
        edges += [(6, 5)]                                 # two, opposite directions
        edges += [(1, 8), (12, 4), (0, 13)]               # loops: earlier -> later, later -> earlier, from the fixed one
    elif variant == 1:
        fixed[[6, 13]] = True                             # fixed in the middle of the chain and as the `to` end of (12, 13)
        edges += [(2, 6), (8, 6), (6, 3)]                 # the fixed vertex at either end
        edges += [(1, 10), (11, 4), (4, 11)]
    else:
        fixed[[0, 5, 6]] = True                           # (5, 6): an edge whose two ends are both fixed, active ones around
        edges += [(5, 6), (6, 5), (3, 12), (12, 3), (7, 2)]
    edges = np.array(edges)
    m = len(edges)
    meas = np.stack([R.inv(gt[a]) @ gt[b] @ R._small_noise(rng, 0.05, 0.01) for a, b in edges])
    L = rng.normal(size=(m, 6, 6)) * 0.5 + 1.5 * np.eye(6)
    K = rng.normal(size=(m, 6, 6))
    info = L @ np.swapaxes(L, 1, 2) + 0.3 * (K - np.swapaxes(K, 1, 2))           # dense, deliberately asymmetric: the host
    info[::3] = L[::3] @ np.swapaxes(L[::3], 1, 2)                                # symmetrises, which leaves L L^T (definite)
    poses = np.stack([gt[k] if fixed[k] else gt[k] @ R._small_noise(rng, 0.15, 0.02) for k in range(n)])
    delta = np.where(np.arange(m) % 3 == 1, 0.8, -1.0)    # Huber on a third of the edges, some beyond the knee
    return {'ids': ids, 'poses': poses, 'fixed': fixed, 'edges': edges, 'meas': meas, 'info': info, 'delta': delta,
            'insert': rng.permutation(n)}


def _load(d):
    """into a PoseGraph, vertices in the order d['insert'] (slots are by insertion, the active order is by id)"""
    from clslam_hip.pose_graph import PoseGraph
    pg = PoseGraph()
    for k in d['insert']:
        assert pg.add_vertex(int(d['ids'][k]), d['poses'][k], bool(d['fixed'][k]))
    for k, (a, b) in enumerate(d['edges']):
        pg.add_edge(int(d['ids'][a]), int(d['ids'][b]), d['meas'][k], d['info'][k],
                    None if d['delta'] is None or d['delta'][k] <= 0 else float(d['delta'][k]))
    return pg


def _built_system(pg):
    """_sync_structure + _upload + _alloc_work + _build -> (H blocks, dense H, b, scal, structure arrays on the host)"""
    pg._sync_structure()
    ctx, stream = pg._ctx()
    with ctx:
        pg._upload()
        pg._alloc_work()
        pg._dev['H'].fill_(float('nan')); pg._dev['b'].fill_(float('nan')); pg._dev['scal'].fill_(float('nan'))
        pg._build(stream)
        na, nnzb = pg._na, pg._nnzb
        Hb = pg._dev['H'][:nnzb].cpu().numpy().reshape(nnzb, 6, 6).copy()
        b = pg._dev['b'][:na].cpu().numpy().reshape(-1).copy()
        scal = pg._read().copy()
        st = {k: v.cpu().numpy() for k, v in pg._sdev.items()}
    rows = np.repeat(np.arange(na), np.diff(st['rptr']))
    assert len(rows) == nnzb == len(st['col'])
    H = np.zeros((6 * na, 6 * na))
    seen = set()
    for q, (r, c) in enumerate(zip(rows, st['col'])):
        assert (r, c) not in seen
        seen.add((r, c))
        H[6 * r:6 * r + 6, 6 * c:6 * c + 6] = Hb[q]
    return Hb, H, b, scal, st, rows


@pytest.mark.parametrize('variant', [0, 1, 2, 3])
@pytest.mark.parametrize('backend', BACKENDS)
def test_assembly(backend, variant):
    """H, b and scal[0] (max diagonal) of pgo_build_system, driven through PoseGraph's host pattern code, against the dense
    R.linear_system.  Graphs: vertices inserted in an order that is not their id order; two, three and four edges between one
    pair in both directions; loop edges in both directions; the fixed vertex as the `to` end and in the middle of the
    chain (tri has -1 inside the matrix: asserted); an edge between two fixed vertices; an isolated vertex; negative and non-
    contiguous ids; dense asymmetric information matrices; Huber with edges beyond the knee.
    (a) Assembly alone: the per-edge records of pgo_linearize_kernel (A^T W A, A^T W B, B^T W B, A^T W e, B^T W e) are read
        back and summed on the host edge by edge, the way R.linear_system does and without the contribution lists:
        1e-12 * max|H| (only the order of <= 8 additions per entry differs: a few eps).  This is what a wrong or missing
        entry in cptr / contrib / diag breaks.  (Feeding pgo_edge_eval's Jacobians to R.linear_system instead does not give
        this: on gfx950 the two kernels compile the same device function with different fused multiply-adds, and their
        Jacobians differ by the rounding floor of (b) -- measured 6e-8 in H.)
    (b) With the reference's Jacobians the two sides differ by the Jacobians alone: kernel and numpy are each within
        4 x floor resp. floor of the longdouble Jacobians (test_jacobians_against_longdouble), so dJ <= 5 floor entrywise,
        and |dH| <= sum over the m edges of a block of (|dJ|^T |W| |J| + |J|^T |W| |dJ|) <= m * 2 * 6 * 6 * dJ * max|W| *
        max|J| per entry (36 products per entry, two terms); |db| <= m * 6 * dJ * max|W e|... bounded the same way with
        |e| in place of |J|.  The floor is measured on this graph's edges.  1e-12 * max|H| cannot hold here: dJ / |J| is
        ~1e-10.
    Identities from the fixed contribution order: block (r, c) is bitwise the transpose of block (c, r); two builds are
    bitwise equal; H's block pattern is exactly the reference's."""
    use_backend(backend)
    d = _assembly_graph(variant)
    pg = _load(d)
    Hb, H, b, scal, st, rows = _built_system(pg)
    g = R.Graph(d['ids'], d['poses'], d['fixed'], d['edges'], d['meas'], d['info'], d['delta'])
    act, H_ref, b_ref = R.linear_system(g, g.poses)
    na = len(act)
    assert pg._na == na and np.array_equal(pg._act_host[[pg._slot[int(i)] for i in d['ids'][act]]], np.arange(na))
    assert np.array_equal(H != 0, H_ref != 0)
    if variant in (1, 2):
        assert (st['tri'][1:, 0] < 0).any() and (st['tri'][:-1, 2] < 0).any()      # the band is broken inside the matrix
    if variant < 3:
        assert (g.delta > 0).any() and (R.chi2_terms(g, g.poses)[1][g.delta > 0] > 0.64).any()
        assert np.array_equal(pg.get_estimate(20), d['poses'][9])
    # (a) the kernel's own per-edge records, summed on the host (record layout: the kLin* offsets of pose_graph.hip)
    from clslam_hip import ops
    lin = pg._dev['lin'][:pg.ne].cpu().numpy()
    assert lin.shape[1] == ops.pgo_lin_stride()
    pos = np.full(len(g.ids), -1)
    pos[act] = np.arange(na)
    H_a, b_a = np.zeros_like(H), np.zeros_like(b)
    for k, (i, j) in enumerate(g.edges):
        pi, pj = pos[i], pos[j]
        Hii, Hij, Hjj = (lin[k, o:o + 36].reshape(6, 6) for o in (0, 36, 72))
        if pi >= 0:
            H_a[6 * pi:6 * pi + 6, 6 * pi:6 * pi + 6] += Hii; b_a[6 * pi:6 * pi + 6] += lin[k, 108:114]
        if pj >= 0:
            H_a[6 * pj:6 * pj + 6, 6 * pj:6 * pj + 6] += Hjj; b_a[6 * pj:6 * pj + 6] += lin[k, 114:120]
        if pi >= 0 and pj >= 0:
            H_a[6 * pi:6 * pi + 6, 6 * pj:6 * pj + 6] += Hij; H_a[6 * pj:6 * pj + 6, 6 * pi:6 * pi + 6] += Hij.T
    hmax = np.abs(H_ref).max()
    print(f'assembly[{variant}]: na {na}, max|H| {hmax:.3g}; own records: dH {np.abs(H - H_a).max():.3g}, db '
          f'{np.abs(b - b_a).max():.3g}; reference Jacobians: dH {np.abs(H - H_ref).max():.3g}, db {np.abs(b - b_ref).max():.3g}')
    assert np.abs(H - H_a).max() <= 1e-12 * hmax
    assert np.abs(b - b_a).max() <= 1e-12 * max(hmax, np.abs(b_ref).max())
    # (b) the reference's Jacobians
    Xi, Xj = g.poses[g.edges[:, 0]], g.poses[g.edges[:, 1]]
    A64, B64 = R.jacobians(Xi, Xj, g.meas)
    Ahp, Bhp = R.jacobians_hp(Xi, Xj, g.meas)
    floor = float(max(np.abs(A64 - Ahp).max(), np.abs(B64 - Bhp).max()))
    dJ = 5 * floor
    deg = np.bincount(g.edges.reshape(-1), minlength=len(g.ids)).max()
    e_ref, s_ref = R.chi2_terms(g, g.poses)
    W = g.info * R.huber(s_ref, g.delta)[1][:, None, None]
    jmax = max(np.abs(A64).max(), np.abs(B64).max())
    bound_H = deg * 2 * 36 * dJ * np.abs(W).max() * jmax
    bound_b = deg * 36 * dJ * np.abs(W).max() * np.abs(e_ref).max()
    print(f'   Jacobian floor {floor:.3g}, bound dH {bound_H:.3g} ({bound_H / hmax:.3g} of max|H|), db {bound_b:.3g}')
    assert bound_H <= 1e-6 * hmax
    assert np.abs(H - H_ref).max() <= bound_H and np.abs(b - b_ref).max() <= bound_b
    assert abs(scal[0] - H_ref.diagonal().max()) <= bound_H and scal[0] == H.diagonal().max()
    # identities
    where = {(r, c): q for q, (r, c) in enumerate(zip(rows, st['col']))}
    off = [(r, c) for (r, c) in where if r != c]
    assert off and all(np.array_equal(Hb[where[r, c]], Hb[where[c, r]].T) for r, c in off)
    Hb2, _, b2, scal2, _, _ = _built_system(pg)
    assert np.array_equal(Hb, Hb2) and np.array_equal(b, b2) and scal[0] == scal2[0]


@pytest.mark.parametrize('variant', [0, 1, 2, 3])
@pytest.mark.parametrize('backend', BACKENDS)
def test_assembly_graphs_optimize(backend, variant):
    """The same graphs through optimize() against R.lm: iterations, chi2 (1e-9 relative), poses (1e-6 m, 1e-7 rad), fixed and
    isolated vertices untouched -- test_pose_graph.py's _check; every solve converged below the cap."""
    use_backend(backend)
    from clslam_hip.pose_graph import CG_MAX_ITER
    d = _assembly_graph(variant)
    pg = _load(d)
    it = pg.optimize(10000)
    g = R.Graph(d['ids'], d['poses'], d['fixed'], d['edges'], d['meas'], d['info'], d['delta'])
    ref, st = R.lm(g)
    P = np.stack([pg.get_estimate(int(i)) for i in d['ids']])
    stats = pg.last_stats
    print(f'optimize[{variant}]: {it} iterations (reference {st["iterations"]}), chi2 {stats["chi2"]!r} / {st["chi2"]!r}, CG '
          f'{stats["cg_iterations"]}')
    assert it == st['iterations']
    assert abs(stats['chi2'] - st['chi2']) <= 1e-9 * st['chi2'] + 1e-20
    assert np.abs(P[:, :3, 3] - ref[:, :3, 3]).max() <= 1e-6
    assert (np.linalg.norm(P[:, :3, :3] - ref[:, :3, :3], axis=(1, 2)) / np.sqrt(2)).max() <= 1e-7
    still = d['fixed'].copy()
    used = np.zeros(len(still), dtype=bool); used[d['edges'].reshape(-1)] = True
    still |= ~used
    assert np.array_equal(P[still], d['poses'][still]) and np.array_equal(ref[still], d['poses'][still])
    assert max(stats['cg_iterations']) < CG_MAX_ITER and max(stats['cg_residual']) <= CG_TOL and stats['precond_failed'] == 0
    # rank argument: L off-band block pairs perturb the preconditioner by rank <= 12 L, so exact CG needs <= 12 L + 1
    # iterations; on these small systems fp64 CG keeps close to that (checked on the reference in test_solve_off_band)


# ---- 3. the linear solve -------------------------------------------------------------------------------------------------
_GUARD = 4096
_GUARD_BITS = 0x7FF8DEADBEEF0000        # a quiet NaN with a payload no computation produces


def _solve(device, S, lam, tol, max_iter):
    """pgo_solve on a host-built system; work is exactly clslam_pgo_solve_workspace(na) doubles followed by a guard region
    with a NaN pattern, which must be untouched afterwards (checked here, for every solve of this file)"""
    from clslam_hip import ops
    na = S['na']
    ws = ops.pgo_solve_workspace(na)
    assert ws >= 30 * na
    work = torch.full((ws + _GUARD,), float('nan'), dtype=torch.float64, device=device)
    guard = torch.full((_GUARD,), _GUARD_BITS, dtype=torch.int64)
    work[ws:] = guard.view(torch.float64).to(device)
    dpad = torch.full((6 * na + 64,), float('nan'), dtype=torch.float64, device=device)
    dpad[6 * na:] = guard[:64].view(torch.float64).to(device)
    scal = torch.full((8,), -7.0, dtype=torch.float64, device=device)
    ops.pgo_solve(_dev(S['H'], device), _dev(S['rptr'], device), _dev(S['col'], device), _dev(S['tri'], device),
                  _dev(S['b'], device), lam, na, tol, max_iter, dpad, work, scal, 0)
    assert torch.equal(work[ws:].cpu().view(torch.int64), guard), 'pgo_solve wrote past its workspace'
    assert torch.equal(dpad[6 * na:].cpu().view(torch.int64), guard[:64]), 'pgo_solve wrote past d'
    s = scal.cpu().numpy()
    assert (s[[0, 4, 6, 7]] == -7.0).all()
    return dpad[:6 * na].cpu().numpy().copy(), s


def _matrices(S, lam):
    import scipy.sparse as sp
    na = S['na']
    I = sp.identity(6 * na, format='csc')
    M = (R.bsr_matrix(S['H'], S['rptr'], S['col'], na) + lam * I).tocsc()
    P = (R.tri_part(S['H'], S['rptr'], S['col'], S['tri'], na) + lam * I).tocsc()
    return M, P


def _max_diag(S):
    return float(S['H'].reshape(-1, 6, 6)[S['diag']].diagonal(axis1=1, axis2=2).max())


_BAND_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1031, 4540]


@pytest.mark.parametrize('na', _BAND_SIZES)
@pytest.mark.parametrize('backend', BACKENDS)
def test_preconditioner_exact_on_band(backend, na):
    """Band only: the block-cyclic-reduction preconditioner is then the matrix, so PCG is a direct solve.  Three dampings:
    lambda = 0 with row 0 strongly anchored (100 J0^T J0), 1e-5 max diag (Levenberg's start), 1e3 max diag.
    Sizes around every power of two up to the workgroup sizes (256 emu, 512 hip) and twice that, and 4540.
    Required, with everything taken from the references first:
      * iterations <= the numpy PCG reference's (exact sparse-LU preconditioner, same stopping rule) + 1; the reference
        takes 1 or 2 (asserted <= 2: with an exact preconditioner the second only mops up rounding);
      * ||d - d_direct|| / ||d_direct|| <= 4 max(ref, eps cond): ref is the same distance for the numpy PCG, cond the
        2-norm condition number of H + lambda I (Lanczos on the host).  eps cond enters because the sparse-LU direct solve
        that serves as the truth is itself only that good; measured ref is between 0 and 2.3e-10 (lambda = 0, na = 4540,
        cond 5.8e9, eps cond 1.3e-6), always below eps cond;
      * the true residual in longdouble <= 4 max(tol, the reference's true residual);
      * the workspace guard is intact (in _solve), two solves are bitwise equal."""
    pytest.importorskip('scipy')
    import scipy.sparse.linalg as spl
    device = use_backend(backend)
    for case, (anchor, lam_rel) in enumerate(((100.0, 0.0), (0.0, 1e-5), (0.0, 1e3))):
        S = R.make_block_system(na, R.band_pairs(na), seed=na + 7 * case, anchor=anchor if na > 1 or anchor else 0.0)
        if na == 1 and anchor == 0.0:                 # a single vertex has no pair: its block comes from a fixed neighbour
            S = R.make_block_system(1, [], seed=na + 7 * case, anchor=1.0)
        lam = lam_rel * _max_diag(S)
        M, P = _matrices(S, lam)
        assert abs(M - P).max() == 0.0
        b = S['b'].reshape(-1)
        direct = spl.splu(M).solve(-b)
        cond = R.cond_spd(M)
        ref = R.pcg_reference(M, P, b, CG_TOL, 50)
        ref_err = float(np.linalg.norm(ref['d'] - direct) / np.linalg.norm(direct))
        ref_res = R.residual_hp(S['H'], S['rptr'], S['col'], na, lam, ref['d'], b)
        assert 1 <= ref['iterations'] <= 2 and ref_err <= 4 * EPS * cond
        d, s = _solve(device, S, lam, CG_TOL, 50)
        err = float(np.linalg.norm(d - direct) / np.linalg.norm(direct))
        res = R.residual_hp(S['H'], S['rptr'], S['col'], na, lam, d, b)
        print(f'band na {na} lambda {lam:.3g}: cond {cond:.3g}; reference {ref["iterations"]} it, err {ref_err:.3g}, true res '
              f'{ref_res:.3g}; kernel {int(s[1])} it, err {err:.3g}, true res {res:.3g}, scal[2] {s[2]:.3g}')
        assert s[5] == 0.0 and s[1] == int(s[1]) and 1 <= s[1] <= ref['iterations'] + 1
        assert err <= 4 * max(ref_err, EPS * cond)
        assert res <= 4 * max(CG_TOL, ref_res)
        d2, s2 = _solve(device, S, lam, CG_TOL, 50)
        assert np.array_equal(d, d2) and np.array_equal(s, s2)


def _off_band_system(kind):
    rng = np.random.default_rng(50 + len(kind))
    if kind == 'few':                                 # 3 off-band pairs in 60 blocks
        na, extra = 60, [(3, 40), (10, 55), (22, 25)]
    elif kind == 'many':                              # 40 random off-band pairs in 300 blocks: a second pass on the emulator
        na = 300
        extra = sorted({tuple(sorted(p)) for p in rng.integers(0, na, (60, 2)).tolist() if abs(p[0] - p[1]) > 1})[:40]
    elif kind == 'dense-row':                         # block 17 seen from 20 others
        na, extra = 80, [(17, k) for k in range(30, 70, 2)]
    else:                                             # 'large': 600 blocks (a second pass on hip too), 12 off-band pairs
        na = 600
        extra = [(int(a), int(a) + int(g)) for a, g in zip(rng.integers(0, 300, 12), rng.integers(5, 290, 12))]
    S = R.make_block_system(na, R.band_pairs(na) + list(extra), seed=len(kind), anchor=1.0)
    return S, len(extra)


@pytest.mark.parametrize('kind', ['few', 'many', 'dense-row', 'large'])
@pytest.mark.parametrize('backend', BACKENDS)
def test_solve_off_band(backend, kind):
    """Band plus off-band blocks (a few, many, one dense row, and 600 blocks) at lambda = 1e-5 max diag, tol 1e-10, cap 2000.
    From the numpy PCG reference alone, first: its iteration count n_ref, the spread of that count over 4 permuted
    summation orders, its true residual (longdouble) and the ratio of its recurrence residual to the true one; and the
    rank bound n_ref <= 12 L + 1 + 2 (L off-band pairs; +2 for the rounding mop-up seen on the band) where 12 L + 3 < n.
    Measured on the host: n_ref 38 / 70 / 13 / 120 for few / many / dense-row / large, spread 0 in all four, ratio 1.00.
    Required of the kernel:
      * |iterations - n_ref| margin: iterations <= n_ref + max(0.1 n_ref + 2, 4 spread) (the issue's 10 % + 2, or 4x the
        reference's own spread if that is larger);
      * true residual <= 4 max(tol, reference's true residual) as the cap is not reached;
      * scal[2] within a factor 4 max(1, reference's ratio) of the true residual, both directions, when above 1e-13;
      * scal[3] = d^T (lambda d - b) from the returned d in longdouble: 1e-12 relative, or 4x the relative error of the
        float64 numpy evaluation of the same expression if that is larger (measured: ~1e-16);
      * scal[1] an integer in [0, max_iter], scal[5] = 0, guard intact, two solves bitwise equal."""
    pytest.importorskip('scipy')
    device = use_backend(backend)
    S, L = _off_band_system(kind)
    na, tol, cap = S['na'], CG_TOL, 2000
    lam = 1e-5 * _max_diag(S)
    M, P = _matrices(S, lam)
    assert abs(M - P).max() > 0
    b = S['b'].reshape(-1)
    ref = R.pcg_reference(M, P, b, tol, cap)
    n_ref = ref['iterations']
    rng = np.random.default_rng(1)
    counts = [R.pcg_reference(M, P, b, tol, cap, perm=rng.permutation(6 * na))['iterations'] for _ in range(4)]
    spread = max(abs(c - n_ref) for c in counts)
    ref_true = R.residual_hp(S['H'], S['rptr'], S['col'], na, lam, ref['d'], b)
    ref_ratio = max(ref['residual'] / ref_true, ref_true / ref['residual'])
    assert 12 < n_ref < cap and ref['residual'] <= tol and ref_true <= 4 * tol
    if 12 * L + 3 < 6 * na:
        assert n_ref <= 12 * L + 3
    margin = max(0.1 * n_ref + 2, 4 * spread)
    d, s = _solve(device, S, lam, tol, cap)
    true = R.residual_hp(S['H'], S['rptr'], S['col'], na, lam, d, b)
    dh, bh = d.astype(R.HP), b.astype(R.HP)
    sc_hp = (dh * (R.HP(lam) * dh - bh)).sum()
    sc_ref_err = abs(float(d @ (lam * d - b)) - sc_hp) / abs(sc_hp)
    print(f'off-band {kind}: na {na}, L {L}; reference {n_ref} it (permuted {counts}), true res {ref_true:.3g}, ratio '
          f'{ref_ratio:.3g}; kernel {int(s[1])} it (margin {margin:.1f}), true res {true:.3g}, scal[2] {s[2]:.3g}, scal[3] '
          f'rel err {float(abs(s[3] - sc_hp) / abs(sc_hp)):.3g} (numpy {float(sc_ref_err):.3g})')
    assert s[1] == int(s[1]) and 0 <= s[1] <= cap and s[5] == 0.0
    assert abs(s[1] - n_ref) <= margin
    assert s[1] < cap and true <= 4 * max(tol, ref_true)
    f = 4 * max(1.0, ref_ratio)
    assert s[2] > 1e-13 and true / f <= s[2] <= true * f and s[2] <= tol
    assert abs(s[3] - sc_hp) <= max(1e-12, 4 * sc_ref_err) * abs(sc_hp)
    d2, s2 = _solve(device, S, lam, tol, cap)
    assert np.array_equal(d, d2) and np.array_equal(s, s2)


@pytest.mark.parametrize('backend', BACKENDS)
def test_solve_caps_and_corners(backend):
    """max_iter = 0: d = 0, scal[1] = 0.  max_iter = 3 on a system the reference needs more than 10 iterations for: scal[1] =
    3 and d equals the reference's third iterate to 1e-10 relative -- or 4x the distance between the reference's third
    iterates under two summation orders if that is larger (measured: 3e-15, so 1e-10 stands; it is a loose figure for
    three CG steps on a system of condition ~1e5, kept as the issue states it).  scal[2] there is the residual AFTER the
    third update: equal to the true residual of the returned d within the factor of test_solve_off_band.
    b = 0: d = 0, scal[2] = 0, all finite.  A zero diagonal block at lambda = 0 (an edge with zero information on a leaf
    vertex): scal[5] = 1, d = 0, all outputs finite.  tol = 0: runs to the cap (unless the residual reaches exactly 0) and
    returns finite values."""
    pytest.importorskip('scipy')
    device = use_backend(backend)
    S, _ = _off_band_system('few')
    na = S['na']
    lam = 1e-5 * _max_diag(S)
    M, P = _matrices(S, lam)
    b = S['b'].reshape(-1)
    d, s = _solve(device, S, lam, CG_TOL, 0)
    assert not d.any() and s[1] == 0 and s[5] == 0 and s[3] == 0 and s[2] == 1.0
    ref = R.pcg_reference(M, P, b, CG_TOL, 2000, iterates=True)
    assert ref['iterations'] > 10
    alt = R.pcg_reference(M, P, b, CG_TOL, 3, perm=np.random.default_rng(2).permutation(6 * na), iterates=True)
    third = ref['iterates'][2]
    ref_only = float(np.linalg.norm(alt['iterates'][2] - third) / np.linalg.norm(third))
    d, s = _solve(device, S, lam, CG_TOL, 3)
    err = float(np.linalg.norm(d - third) / np.linalg.norm(third))
    true = R.residual_hp(S['H'], S['rptr'], S['col'], na, lam, d, b)
    print(f'cap 3: reference-only {ref_only:.3g}, kernel {err:.3g}; scal[2] {s[2]:.6g}, true residual {true:.6g}')
    assert s[1] == 3 and s[5] == 0 and err <= max(1e-10, 4 * ref_only)
    assert true / 4 <= s[2] <= 4 * true and abs(s[2] - true) <= 1e-6 * true      # far above rounding: the two must coincide
    # b = 0
    Z = dict(S, b=np.zeros_like(S['b']))
    d, s = _solve(device, Z, lam, CG_TOL, 100)
    assert not d.any() and s[1] == 0 and s[2] == 0 and s[3] == 0 and s[5] == 0 and np.isfinite(s).all()
    # a zero diagonal block, lambda = 0
    for n0 in (1, 2, 6, 9, 300):
        Zs = R.make_block_system(n0, R.band_pairs(n0)[:-1], seed=3, anchor=1.0 if n0 > 1 else 0.0,
                                 zero_pairs=R.band_pairs(n0)[-1:])
        assert not Zs['H'].reshape(-1, 6, 6)[Zs['diag'][-1]].any()
        d, s = _solve(device, Zs, 0.0, CG_TOL, 100)
        assert s[5] == 1 and not d.any() and s[1] == 0 and np.isfinite(d).all() and np.isfinite(s).all(), n0
        d, s = _solve(device, Zs, 0.5, CG_TOL, 100)       # damped, the same system is definite
        assert s[5] == 0 and 1 <= s[1] <= 3 and d.any()
    # tol = 0
    for S0, lam0 in ((S, lam), (R.make_block_system(1, [], seed=1, anchor=1.0), 0.0),
                     (R.make_block_system(5, R.band_pairs(5), seed=1, anchor=1.0), 0.0),
                     (R.make_block_system(700, R.band_pairs(700), seed=1, anchor=1.0), 1e-3)):
        d, s = _solve(device, S0, lam0, 0.0, 40)
        print(f'tol 0, na {S0["na"]}: {int(s[1])} iterations, scal[2] {s[2]:.3g}')
        assert np.isfinite(d).all() and np.isfinite(s).all() and 1 <= s[1] <= 40 and (s[1] == 40 or s[2] == 0.0)
        # going on past the tol = 1e-10 stopping point must not leave it worse than that stop is allowed to be
        assert R.residual_hp(S0['H'], S0['rptr'], S0['col'], S0['na'], lam0, d, S0['b'].reshape(-1)) <= 4 * CG_TOL
