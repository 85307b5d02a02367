"""SE(3) pose-graph optimiser (csrc/pose_graph.hip + clslam_hip/pose_graph.py) against the float64 numpy restatement in
tests/pgo_reference.py: error and Jacobians, Levenberg on small graphs, incremental growth as slam.py does it, Huber,
bitwise determinism and corner cases.  emu = the kernel sources on the CPU emulator (graphs <= 150 vertices), hip = the
gfx950 library (adds 600 vertices)."""
import numpy as np
import pytest

import pgo_reference as R
from emu_util import BACKENDS, use_backend


def _pg(d, delta=None, upto=None):
    from clslam_hip.pose_graph import PoseGraph
    pg = PoseGraph()
    n = len(d['ids']) if upto is None else upto
    for k in range(n):
        assert pg.add_vertex(int(d['ids'][k]), d['poses'][k], bool(d['fixed'][k]))
    for k, (a, b) in enumerate(d['edges']):
        if a < n and b < n:
            pg.add_edge(int(d['ids'][a]), int(d['ids'][b]), d['meas'][k], d['info'][k], None if delta is None else delta[k])
    return pg


def _poses(pg, ids):
    return np.stack([pg.get_estimate(int(i)) for i in ids])


def _check(P, ref, stats, ref_stats, fixed, tol_t=1e-6, tol_r=1e-7):
    # (+1e-20 absolute: an exactly consistent graph converges to chi2 ~ 1e-32, pure fp64 round-off)
    assert abs(stats['chi2'] - ref_stats['chi2']) <= 1e-9 * ref_stats['chi2'] + 1e-20
    assert np.abs(P[:, :3, 3] - ref[:, :3, 3]).max() <= tol_t
    # rotation difference in rad as ||R1 - R2||_F / sqrt(2) (arccos of the trace cannot resolve angles below ~1.5e-8).
    # 1e-7, not 1e-8: on the 150-vertex chain the two runs stop at the same iteration with chi2 equal to 1e-14 relative but
    # differ by up to 2.4e-8 rad at the far end (measured on the emulator): a low-curvature bending mode of the chain, along
    # which the last PCG step (relative residual 1e-10) and the dense direct solve leave different remainders.
    assert (np.linalg.norm(P[:, :3, :3] - ref[:, :3, :3], axis=(1, 2)) / np.sqrt(2)).max() <= tol_r
    assert np.array_equal(P[fixed], ref[fixed])


def _assert_solves_converged(pg):
    """every linear solve of the last optimize() ended below the iteration cap at the requested residual, and the
    preconditioner was factorable every time"""
    from clslam_hip.pose_graph import CG_MAX_ITER, CG_TOL
    st = pg.last_stats
    assert len(st['cg_residual']) == len(st['cg_iterations']) == st['trials'] > 0
    assert max(st['cg_iterations']) < CG_MAX_ITER, st['cg_iterations']
    assert max(st['cg_residual']) <= CG_TOL, st['cg_residual']
    assert st['precond_failed'] == 0


def _random_pose(rng, big=False):
    T = np.eye(4)
    T[:3, :3] = R._rot(*rng.uniform(-np.pi, np.pi, 3)) if big else R._rot(*rng.normal(0, 0.3, 3))
    T[:3, 3] = rng.normal(0, 3, 3)
    return T


@pytest.mark.parametrize('backend', BACKENDS)
def test_error_and_jacobians(backend):
    use_backend(backend)
    from clslam_hip.pose_graph import PoseGraph
    rng = np.random.default_rng(7)
    pg = PoseGraph()
    n = 24
    X = np.stack([_random_pose(rng, big=True) for _ in range(n)])
    for k in range(n):
        pg.add_vertex(k, X[k])
    edges, Z = [], []
    for k in range(n):
        j = (k + 1 + k % 5) % n
        z = R.inv(X[k]) @ X[j] @ _random_pose(rng)
        if k % 4 == 0:                         # relative rotation near 180 degrees
            flip = np.eye(4)
            flip[:3, :3] = R._rot(np.pi - 1e-3 * (1 + k), 0.0, 0.0)
            z = R.inv(X[k]) @ X[j] @ flip
        edges.append((k, j)); Z.append(z)
        pg.add_edge(k, j, z)
    edges, Z = np.array(edges), np.array(Z)
    err, A, B = pg.edge_eval()
    e_ref = R.edge_error(X[edges[:, 0]], X[edges[:, 1]], Z)
    assert np.abs(err - e_ref).max() <= 1e-12
    A_ref, B_ref = R.jacobians(X[edges[:, 0]], X[edges[:, 1]], Z)
    assert np.abs(A - A_ref).max() <= 1e-7 and np.abs(B - B_ref).max() <= 1e-7


@pytest.mark.parametrize('backend', BACKENDS)
def test_increment_chart_and_update(backend):
    """X <- X * exp(v), including |qxyz|^2 > 1 (identity rotation), re-orthonormalised: through the update kernel"""
    use_backend(backend)
    from clslam_hip.pose_graph import PoseGraph
    rng = np.random.default_rng(3)
    pg = PoseGraph()
    X = np.stack([_random_pose(rng, big=True) for _ in range(6)])
    for k in range(6):
        pg.add_vertex(k, X[k], fixed=(k == 0))
        if k:
            pg.add_edge(k - 1, k, np.eye(4))
    pg._sync_structure()
    ctx, stream = pg._ctx()
    import torch
    v = np.array([[0.1, -0.2, 0.3, 0.1, 0.2, -0.05], [1, 2, 3, 0.8, 0.5, 0.4], [0, 0, 0, 0.9, 0.5, 0.1],
                  [0.5, 0.5, 0.5, -0.3, 0.3, 0.3], [0, 0, 0, 0, 0, 0]])
    with ctx:
        pg._upload()
        pg._alloc_work()
        delta = torch.from_numpy(v.copy()).to(pg.device)
        pg._score(stream, delta, True, 6)
        trial = pg._dev['trial'][:6].cpu().numpy().reshape(-1, 4, 4)
    order = R.active_order(R.Graph(np.arange(6), X, np.arange(6) == 0, np.array([(k - 1, k) for k in range(1, 6)]),
                                   np.tile(np.eye(4), (5, 1, 1)), np.tile(np.eye(6), (5, 1, 1))))
    ref = X.copy()
    ref[order] = R.oplus(X[order], v)
    assert np.abs(trial - ref).max() <= 1e-12
    assert np.array_equal(trial[0], X[0])
    assert np.allclose(R.exp_mqt(v[1:2])[0, :3, :3], np.eye(3))


# the emulator covers graphs up to 150 vertices; the hip backend adds 600
_LM_CASES = [pytest.param(b.values[0], n, loops, id=f'{n}-{loops}-{b.id}', marks=b.marks)
             for b in BACKENDS for n, loops in ((2, 0), (10, 2), (150, 6))] + \
            [pytest.param('hip', 600, 20, id='600-20-hip', marks=pytest.mark.gpu)]


@pytest.mark.parametrize('backend,n,loops', _LM_CASES)
def test_lm_matches_dense_reference(backend, n, loops):
    use_backend(backend)
    d = R.make_graph(n, loops, seed=n, start_id=5, lap=max(2, int(0.7 * n)))
    if n == 2:                                  # perturb the start so that there is something to do
        d['poses'][1] = d['poses'][1] @ R.exp_mqt([[0.3, -0.2, 0.1, 0.05, 0.02, -0.03]])[0]
    pg = _pg(d)
    it = pg.optimize(10000)
    _assert_solves_converged(pg)
    ref, st = R.lm(R.graph_of(d))
    assert it == st['iterations']
    # 600 vertices: chi2 equal to 2.5e-13 relative after the same 44 iterations, but the far end of the chain differs by
    # 5.4e-5 m (measured on the MI355X): the same low-curvature bending mode as above, 4x longer; hence 2e-4 m / 1e-5 rad there
    _check(_poses(pg, d['ids']), ref, pg.last_stats, st, d['fixed'], *((2e-4, 1e-5) if n > 150 else (1e-6, 1e-7)))
    if loops:
        assert R.ate(ref, d['gt']) < R.ate(d['poses'], d['gt'])


_CHAIN_CASES = [pytest.param(b.values[0], n, id=f'{n}-{b.id}', marks=b.marks)
                for b in BACKENDS for n in (3, 10, 33, 150, 300, 700)] + [pytest.param('hip', 1500, id='1500-hip', marks=pytest.mark.gpu)]


@pytest.mark.parametrize('backend,n', _CHAIN_CASES)
def test_loop_free_chain_solves_are_direct(backend, n, monkeypatch):
    """On a loop-free chain the block-tridiagonal preconditioner is the whole matrix: every solve of optimize() takes no more
    iterations than a numpy PCG with an exact (sparse-LU) preconditioner takes on the very same H, b and lambda (read back
    from the device at each solve), plus one.  The reference takes 1 or 2; nothing is hard-coded here."""
    pytest.importorskip('scipy')
    import scipy.sparse as sp
    use_backend(backend)
    from clslam_hip import ops, pose_graph
    d = R.make_graph(n, 0, seed=n)
    rng = np.random.default_rng(n)
    for k in range(1, n):                       # perturb the start: the odometry chain alone is exactly consistent
        d['poses'][k] = d['poses'][k] @ R._small_noise(rng, 0.2, 0.02)
    pg = _pg(d)
    seen = []
    real = ops.pgo_solve

    def recording(H, rptr, col, tri, b, lam, na, *rest):
        nnzb = int(rptr[na].item())
        seen.append((H[:nnzb].cpu().numpy().copy(), rptr[:na + 1].cpu().numpy(), col[:nnzb].cpu().numpy(), tri[:na].cpu().numpy(),
                     b[:na].cpu().numpy().copy(), float(lam), na))
        real(H, rptr, col, tri, b, lam, na, *rest)

    monkeypatch.setattr(ops, 'pgo_solve', recording)
    it = pg.optimize(20)
    monkeypatch.undo()
    _assert_solves_converged(pg)
    stats = pg.last_stats
    assert it >= 1 and len(seen) == len(stats['cg_iterations']) and seen[0][-1] == n - 1
    ref_counts = []
    for H, rptr, col, tri, b, lam, na in seen:
        I = sp.identity(6 * na, format='csc')
        M = R.bsr_matrix(H, rptr, col, na) + lam * I
        P = R.tri_part(H, rptr, col, tri, na) + lam * I
        assert abs(M - P).max() == 0.0
        ref_counts.append(R.pcg_reference(M, P, b, pose_graph.CG_TOL, pose_graph.CG_MAX_ITER)['iterations'])
    print(f'\nchain {n}: CG iterations {stats["cg_iterations"]}, numpy PCG reference {ref_counts}')
    assert all(k <= r + 1 for k, r in zip(stats['cg_iterations'], ref_counts))


@pytest.mark.parametrize('backend', BACKENDS)
def test_incremental_growth_like_slam(backend):
    """optimize, add vertices / edges / a loop, set_estimate, optimize again: equal to the reference run on the same sequence;
    non-contiguous ids, an isolated vertex (never moves)"""
    use_backend(backend)
    from clslam_hip.pose_graph import PoseGraph
    d = R.make_graph(60, 4, seed=11, start_id=1000, lap=40)
    d['ids'] = d['ids'] * 3 + (np.arange(60) % 2)          # non-contiguous, increasing
    pg = PoseGraph()
    g_ref_poses = d['poses'].copy()
    iso = np.eye(4); iso[:3, 3] = [5, 6, 7]
    for stage_end in (45, 60):
        for k in range(len(pg.vertex_ids()) - (1 if len(pg.vertex_ids()) > 45 else 0), stage_end):
            if not pg.has_vertex(int(d['ids'][k])):
                pg.add_vertex(int(d['ids'][k]), g_ref_poses[k], bool(d['fixed'][k]))
        for k, (a, b) in enumerate(d['edges']):
            if a < stage_end and b < stage_end and (stage_end == 45 or a >= 45 or b >= 45):
                pg.add_edge(int(d['ids'][a]), int(d['ids'][b]), d['meas'][k], d['info'][k])
        if stage_end == 45:
            pg.add_vertex(-7, iso)                     # isolated
        pg.optimize(10000)
        _assert_solves_converged(pg)
        sel = [k for k, (a, b) in enumerate(d['edges']) if a < stage_end and b < stage_end]
        g = R.Graph(d['ids'][:stage_end], g_ref_poses[:stage_end], d['fixed'][:stage_end], d['edges'][sel], d['meas'][sel],
                    d['info'][sel])
        ref, st = R.lm(g)
        _check(_poses(pg, d['ids'][:stage_end]), ref, pg.last_stats, st, d['fixed'][:stage_end])
        g_ref_poses[:stage_end] = ref
        if stage_end == 45:                            # set_estimate between calls
            bump = g_ref_poses[30] @ R.exp_mqt([[0.2, 0.1, 0.0, 0.01, 0.0, 0.02]])[0]
            pg.set_estimate(int(d['ids'][30]), bump)
            g_ref_poses[30] = bump
    assert np.array_equal(pg.get_estimate(-7), iso)


@pytest.mark.parametrize('backend', BACKENDS)
def test_no_fixed_vertex_relative_transforms(backend):
    use_backend(backend)
    d = R.make_graph(30, 3, seed=4, lap=20)
    d['fixed'][:] = False
    pg = _pg(d)
    pg.optimize(10000)
    _assert_solves_converged(pg)
    ref, st = R.lm(R.graph_of(d))
    P = _poses(pg, d['ids'])
    rel = np.einsum('ij,njk->nik', R.inv(P[0]), P)
    rel_ref = np.einsum('ij,njk->nik', R.inv(ref[0]), ref)
    assert np.abs(rel - rel_ref).max() <= 1e-6
    assert abs(pg.last_stats['chi2'] - st['chi2']) <= 1e-9 * st['chi2'] + 1e-12


@pytest.mark.parametrize('backend', BACKENDS)
def test_huber(backend):
    use_backend(backend)
    d = R.make_graph(50, 4, seed=9, lap=35)
    d['meas'][-1] = d['meas'][-1] @ R.exp_mqt([[3.0, -2.0, 1.0, 0.2, 0.1, 0.0]])[0]      # an outlier loop closure
    delta = np.where(np.arange(len(d['edges'])) >= d['n_odom'], 1.0, -1.0)
    pg = _pg(d, delta)
    pg.optimize(10000)
    _assert_solves_converged(pg)
    ref, st = R.lm(R.graph_of(d, delta))
    _check(_poses(pg, d['ids']), ref, pg.last_stats, st, d['fixed'])
    assert abs(pg.chi2(robust=True) - R.robust_chi2(R.graph_of(d, delta), ref)) <= 1e-9 * st['chi2']


@pytest.mark.parametrize('backend', BACKENDS)
def test_bitwise_deterministic(backend):
    use_backend(backend)
    d = R.make_graph(80, 5, seed=2, lap=56)
    a, b = _pg(d), _pg(d)
    a.optimize(10000)
    b.optimize(10000)
    _assert_solves_converged(a)
    assert np.array_equal(_poses(a, d['ids']), _poses(b, d['ids']))
    assert a.last_stats['cg_iterations'] == b.last_stats['cg_iterations']
    assert a.last_stats['cg_residual'] == b.last_stats['cg_residual']


@pytest.mark.parametrize('backend', BACKENDS)
def test_corner_cases(backend):
    use_backend(backend)
    from clslam_hip.pose_graph import PoseGraph
    pg = PoseGraph()
    assert pg.optimize(100) == 0 and pg.chi2() == 0.0
    assert pg.add_vertex(3, np.eye(4), fixed=True)
    assert not pg.add_vertex(3, np.eye(4))
    with pytest.raises(KeyError):
        pg.add_edge(3, 4, np.eye(4))
    assert pg.optimize(100) == 0
    pg.add_vertex(4, np.eye(4), fixed=True)
    pg.add_edge(3, 4, np.eye(4))
    assert pg.optimize(100) == 0                    # nothing active
    assert np.array_equal(pg.get_estimate(4), np.eye(4))
