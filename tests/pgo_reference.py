"""TEST INFRASTRUCTURE: an independent float64 numpy restatement of the SE(3) pose-graph conventions of
cl-slam_amd/csrc/pose_graph.hip (g2o types/slam3d: compact-quaternion chart, right-multiplied updates, toVectorMQT error,
Huber) and of g2o's Levenberg rule, plus a seeded KITTI-like graph generator.

    exp_mqt / log_mqt / oplus / edge_error / jacobians   batched over a leading axis
    lm(graph, max_iterations)                            dense (or scipy-sparse) Levenberg -> (poses, stats)
    make_graph(n, n_loops, seed, start_id)               ground truth, odometry start, odometry + loop edges
    jacobians_hp / edge_error_hp / robust_chi2_hp        the same in numpy.longdouble, for the kernel-level tests
    make_block_system / pcg_reference / ...              block-CSR SPD systems that do not come from a graph, and a plain
                                                         numpy PCG with an exact block-tridiagonal preconditioner

Nothing here runs on the device; the kernels are checked against it."""
import numpy as np

JAC_STEP = 1e-6
ODOM_COV = np.diag([1.0, 1.0, 0.1, 1.0, 1.0, 0.1])          # slam.py's odometry covariance (information = its inverse)


# ---- chart --------------------------------------------------------------------------------------------------------------
def exp_mqt(v, dtype=np.float64):
    """(n,6) (t, qxyz) -> (n,4,4); |qxyz|^2 > 1 gives the identity rotation"""
    v = np.atleast_2d(np.asarray(v, dtype=dtype))
    x, y, z = v[:, 3], v[:, 4], v[:, 5]
    w2 = 1.0 - (x * x + y * y + z * z)
    bad = w2 < 0
    w = np.sqrt(np.where(bad, 0.0, w2))
    x, y, z = (np.where(bad, 0.0, a) for a in (x, y, z))
    w = np.where(bad, 1.0, w)
    T = np.zeros((len(v), 4, 4), dtype=dtype)
    T[:, 0, 0] = 1 - 2 * (y * y + z * z); T[:, 0, 1] = 2 * (x * y - z * w); T[:, 0, 2] = 2 * (x * z + y * w)
    T[:, 1, 0] = 2 * (x * y + z * w); T[:, 1, 1] = 1 - 2 * (x * x + z * z); T[:, 1, 2] = 2 * (y * z - x * w)
    T[:, 2, 0] = 2 * (x * z - y * w); T[:, 2, 1] = 2 * (y * z + x * w); T[:, 2, 2] = 1 - 2 * (x * x + y * y)
    T[:, :3, 3] = v[:, :3]
    T[:, 3, 3] = 1.0
    return T


def _quat(R):
    """Eigen's matrix -> quaternion (x, y, z, w), one matrix"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, dtype=R.dtype)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def log_mqt(T, dtype=np.float64):
    """(n,4,4) -> (n,6) (t, xyz of the unit quaternion with w >= 0)"""
    T = np.asarray(T, dtype=dtype).reshape(-1, 4, 4)
    out = np.zeros((len(T), 6), dtype=dtype)
    for n, M in enumerate(T):
        q = _quat(M[:3, :3])
        q /= np.linalg.norm(q)
        if q[3] < 0:
            q = -q
        out[n, :3] = M[:3, 3]
        out[n, 3:] = q[:3]
    return out


def inv(T, dtype=np.float64):
    T = np.asarray(T, dtype=dtype)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum('...ij,...j->...i', Rt, T[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


def oplus(X, v):
    """X * exp(v), then R -= 0.5 R (R^T R - I) (g2o's approximateNearestOrthogonalMatrix)"""
    Y = np.asarray(X, dtype=np.float64).reshape(-1, 4, 4) @ exp_mqt(v)
    R = Y[:, :3, :3]
    E = np.swapaxes(R, 1, 2) @ R - np.eye(3)
    Y[:, :3, :3] = R - 0.5 * R @ E
    return Y


def edge_error(Xi, Xj, Z, dtype=np.float64):
    return log_mqt(inv(Z, dtype) @ inv(Xi, dtype) @ np.asarray(Xj, dtype=dtype), dtype)


def jacobians(Xi, Xj, Z, h=JAC_STEP, dtype=np.float64):
    """(A, B) (n,6,6): central differences of edge_error in the increments of Xi and Xj"""
    Xi, Xj, Z = (np.asarray(a, dtype=dtype).reshape(-1, 4, 4) for a in (Xi, Xj, Z))
    n = len(Xi)
    A, B = np.zeros((n, 6, 6), dtype=dtype), np.zeros((n, 6, 6), dtype=dtype)
    h = dtype(h)
    for k in range(6):
        v = np.zeros((n, 6), dtype=dtype)
        v[:, k] = h
        Ep, Em = exp_mqt(v, dtype), exp_mqt(-v, dtype)
        A[:, :, k] = (edge_error(Xi @ Ep, Xj, Z, dtype) - edge_error(Xi @ Em, Xj, Z, dtype)) / (2 * h)
        B[:, :, k] = (edge_error(Xi, Xj @ Ep, Z, dtype) - edge_error(Xi, Xj @ Em, Z, dtype)) / (2 * h)
    return A, B


# ---- the same in numpy.longdouble (x87 extended where the platform has it: eps 1.1e-19) ----------------------------------
HP = np.longdouble
HP_JAC_STEP = 2.0 ** -21        # ~eps_hp^(1/3): truncation (h^2 / 6 |e'''|) and rounding (eps_hp / h) both ~2e-13


def edge_error_hp(Xi, Xj, Z):
    return edge_error(Xi, Xj, Z, HP)


def jacobians_hp(Xi, Xj, Z, h=HP_JAC_STEP):
    """jacobians() carried out in numpy.longdouble end to end (the float64 inputs convert exactly), step for that precision"""
    return jacobians(Xi, Xj, Z, h, HP)


def quat_branch(Rm):
    """which branch of the matrix -> quaternion conversion a rotation takes: 0 for trace > 0, else 1 + the index of the
    largest diagonal entry"""
    Rm = np.asarray(Rm)
    if Rm[0, 0] + Rm[1, 1] + Rm[2, 2] > 0:
        return 0
    i = 0
    if Rm[1, 1] > Rm[0, 0]:
        i = 1
    if Rm[2, 2] > Rm[i, i]:
        i = 2
    return 1 + i


def quat_to_pose(q_wxyz, t=(0.0, 0.0, 0.0)):
    """[R(q) t] of a quaternion (w, x, y, z) (normalised here in longdouble), rounded to float64 once at the end"""
    q = np.asarray(q_wxyz, dtype=HP)
    q = q / np.sqrt((q * q).sum())
    w, x, y, z = q
    T = np.zeros((4, 4), dtype=HP)
    T[0, :3] = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)]
    T[1, :3] = [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)]
    T[2, :3] = [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    T[:3, 3] = np.asarray(t, dtype=HP)
    T[3, 3] = 1
    return T.astype(np.float64), q.astype(np.float64)


def huber(s, delta):
    """(rho, rho') per edge; delta <= 0: none"""
    s = np.asarray(s, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    use = (delta > 0) & (s > delta * delta)
    r = np.sqrt(np.where(use, s, 1.0))
    rho = np.where(use, 2 * delta * r - delta * delta, s)
    return rho, np.where(use, delta / r, 1.0)


# ---- graph and Levenberg ------------------------------------------------------------------------------------------------
class Graph:
    """ids (n,), poses (n,4,4), fixed (n,) bool, edges (m,2) indices into ids, meas (m,4,4), info (m,6,6), delta (m,) (<= 0: no Huber)"""

    def __init__(self, ids, poses, fixed, edges, meas, info, delta=None):
        self.ids = np.asarray(ids, dtype=np.int64)
        self.poses = np.asarray(poses, dtype=np.float64).copy()
        self.fixed = np.asarray(fixed, dtype=bool)
        self.edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        self.meas = np.asarray(meas, dtype=np.float64).reshape(-1, 4, 4)
        om = np.asarray(info, dtype=np.float64).reshape(-1, 6, 6)
        self.info = 0.5 * (om + np.swapaxes(om, 1, 2))
        self.delta = np.full(len(self.edges), -1.0) if delta is None else np.asarray(delta, dtype=np.float64)


def chi2_terms(g, poses):
    e = edge_error(poses[g.edges[:, 0]], poses[g.edges[:, 1]], g.meas)
    return e, np.einsum('ni,nij,nj->n', e, g.info, e)


def robust_chi2(g, poses):
    return float(huber(chi2_terms(g, poses)[1], g.delta)[0].sum())


def robust_chi2_hp(g, poses, robust=True):
    """sum(rho) (robust=False: the plain sum of e^T Omega e) with errors, quadratic forms and the sum in numpy.longdouble"""
    e = edge_error_hp(poses[g.edges[:, 0]], poses[g.edges[:, 1]], g.meas)
    s = np.einsum('ni,nij,nj->n', e, g.info.astype(HP), e)
    if not robust:
        return s.sum()
    d = g.delta.astype(HP)
    use = (d > 0) & (s > d * d)
    return np.where(use, 2 * d * np.sqrt(np.where(use, s, 1)) - d * d, s).sum()


def active_order(g):
    used = np.zeros(len(g.ids), dtype=bool)
    used[g.edges.reshape(-1)] = True
    act = np.nonzero(used & ~g.fixed)[0]
    return act[np.argsort(g.ids[act], kind='stable')]


def linear_system(g, poses, sparse=False, jac=None):
    """(active order, H, b); jac = (A, B) replaces this module's own Jacobians (to separate assembly from differentiation)"""
    act = active_order(g)
    na = len(act)
    pos = np.full(len(g.ids), -1)
    pos[act] = np.arange(na)
    Xi, Xj = poses[g.edges[:, 0]], poses[g.edges[:, 1]]
    e = edge_error(Xi, Xj, g.meas)
    A, B = jacobians(Xi, Xj, g.meas) if jac is None else jac
    s = np.einsum('ni,nij,nj->n', e, g.info, e)
    _, w = huber(s, g.delta)
    W = g.info * w[:, None, None]
    blocks = {}
    b = np.zeros(6 * na)

    def add(r, c, M):
        blocks[(r, c)] = blocks.get((r, c), 0) + M

    for k, (i, j) in enumerate(g.edges):
        pi, pj = pos[i], pos[j]
        if pi >= 0:
            add(pi, pi, A[k].T @ W[k] @ A[k]); b[6 * pi:6 * pi + 6] += A[k].T @ W[k] @ e[k]
        if pj >= 0:
            add(pj, pj, B[k].T @ W[k] @ B[k]); b[6 * pj:6 * pj + 6] += B[k].T @ W[k] @ e[k]
        if pi >= 0 and pj >= 0:
            add(pi, pj, A[k].T @ W[k] @ B[k]); add(pj, pi, B[k].T @ W[k] @ A[k])
    if sparse:
        import scipy.sparse as sp
        rows, cols, vals = [], [], []
        rr, cc = np.meshgrid(np.arange(6), np.arange(6), indexing='ij')
        for (r, c), M in blocks.items():
            rows.append(6 * r + rr.ravel()); cols.append(6 * c + cc.ravel()); vals.append(M.ravel())
        H = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * na, 6 * na))
    else:
        H = np.zeros((6 * na, 6 * na))
        for (r, c), M in blocks.items():
            H[6 * r:6 * r + 6, 6 * c:6 * c + 6] += M
    return act, H, b


def lm(g, max_iterations=10000, sparse=False, tau=1e-5, max_trials=10, min_rel_decrease=1e-12):
    """g2o's Levenberg on a copy of g.poses -> (poses, {'iterations', 'chi2'})"""
    poses = g.poses.copy()
    chi2 = robust_chi2(g, poses)
    lam, ni, it = None, 2.0, 0
    if len(g.edges) == 0 or len(active_order(g)) == 0:
        return poses, {'iterations': 0, 'chi2': chi2}
    if sparse:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
    while it < max_iterations:
        act, H, b = linear_system(g, poses, sparse=sparse)
        n = H.shape[0]
        if lam is None:
            lam = tau * float(H.diagonal().max())
        trials, rho, accepted, before = 0, -1.0, False, chi2
        while True:
            if sparse:
                d = spl.spsolve((H + lam * sp.identity(n, format='csr')).tocsc(), -b)
            else:
                d = np.linalg.solve(H + lam * np.eye(n), -b)
            trial = poses.copy()
            trial[act] = oplus(poses[act], d.reshape(-1, 6))
            new = robust_chi2(g, trial)
            rho = (chi2 - new) / (float(d @ (lam * d - b)) + 1e-3)
            if rho > 0 and np.isfinite(new):
                lam *= max(1 / 3, min(2 / 3, 1 - (2 * rho - 1) ** 3))
                ni, chi2, poses, accepted = 2.0, new, trial, True
            else:
                lam *= ni
                ni *= 2
            trials += 1
            if not (rho < 0 and trials < max_trials):
                break
        it += 1
        if trials == max_trials or rho == 0 or not np.isfinite(lam):
            break
        if accepted and before - chi2 < min_rel_decrease * before:
            break
    return poses, {'iterations': it, 'chi2': chi2}


# ---- KITTI-like generator -----------------------------------------------------------------------------------------------
def _rot(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp_, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp_], [0, 1, 0], [-sp_, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def _small_noise(rng, sig_t, sig_r):
    T = np.eye(4)
    T[:3, :3] = _rot(*(rng.normal(0, sig_r, 3)))
    T[:3, 3] = rng.normal(0, sig_t, 3)
    return T


def make_graph(n, n_loops, seed=0, start_id=0, lap=None, sig_t=0.05, sig_r=0.004, loop_sig_t=0.02, loop_sig_r=0.002):
    """A car driving laps of a closed loop (radius from the lap length, 1 m per frame, slight hills), noisy odometry chained
    from a fixed first pose at its ground truth, and n_loops revisit edges between frame i and frame i - lap.
    -> dict(ids, gt, poses (odometry start), fixed, edges, meas, info, odom_edges, loop_edges)"""
    rng = np.random.default_rng(seed)
    lap = lap or max(4, int(0.7 * n))
    radius = lap / (2 * np.pi)
    gt = np.zeros((n, 4, 4))
    for k in range(n):
        a = 2 * np.pi * k / lap
        gt[k] = np.eye(4)
        gt[k][:3, :3] = _rot(a + np.pi / 2, 0.02 * np.sin(3 * a), 0.01 * np.cos(2 * a))
        gt[k][:3, 3] = [radius * np.cos(a), radius * np.sin(a), 2.0 * np.sin(2 * a)]
    ids = np.arange(n, dtype=np.int64) + start_id
    odom_info = np.linalg.inv(ODOM_COV)
    edges, meas, info = [], [], []
    poses = np.zeros_like(gt)
    poses[0] = gt[0]
    for k in range(1, n):
        z = inv(gt[k - 1]) @ gt[k] @ _small_noise(rng, sig_t, sig_r)
        edges.append((k - 1, k)); meas.append(z); info.append(odom_info)
        poses[k] = poses[k - 1] @ z
    cand = np.arange(lap, n)
    n_odom = len(edges)
    if n_loops and len(cand):
        pick = cand[np.linspace(0, len(cand) - 1, min(n_loops, len(cand))).round().astype(int)]
        for i in pick:
            j = i - lap
            z = inv(gt[i]) @ gt[j] @ _small_noise(rng, loop_sig_t, loop_sig_r)
            edges.append((i, j)); meas.append(z); info.append(0.5 * odom_info)
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = True
    return {'ids': ids, 'gt': gt, 'poses': poses, 'fixed': fixed, 'edges': np.array(edges, dtype=np.int64).reshape(-1, 2),
            'meas': np.array(meas).reshape(-1, 4, 4), 'info': np.array(info).reshape(-1, 6, 6), 'n_odom': n_odom}


def graph_of(d, delta=None):
    return Graph(d['ids'], d['poses'], d['fixed'], d['edges'], d['meas'], d['info'], delta)


def ate(poses, gt):
    """root-mean-square translation error (no alignment: the first pose is fixed at its ground truth)"""
    return float(np.sqrt(np.mean(np.sum((np.asarray(poses)[:, :3, 3] - gt[:, :3, 3]) ** 2, axis=1))))


def rot_angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


# ---- block-CSR SPD systems without a graph, and the PCG reference ------------------------------------------------------
def band_pairs(na):
    return [(k, k + 1) for k in range(na - 1)]


def make_block_system(na, pairs, seed=0, anchor=0.0, zero_pairs=()):
    """H = sum over pairs (r, c) of J^T J with one 6x12 J per pair (every term PSD, as an edge's J^T W J is) in the solver's
    block-CSR layout.  J = D [-(Q1 + N1) | Q2 + N2]: Q orthogonal, D a positive diagonal in [0.5, 2], N Gaussian of size
    0.3 / sqrt(na) -- dense and different per pair, yet the chain's transfer matrices stay near orthogonal, so the
    condition number grows like na^2 and not exponentially.  anchor > 0 adds anchor * J0^T J0 (J0 6x6) to block (0, 0): the
    fixed neighbour that makes H definite without damping.  zero_pairs: pairs drawn with J = 0 (zero information).
    -> dict(H [nnzb][36], rptr, col, tri, diag, b [na][6], na)"""
    rng = np.random.default_rng(seed)
    blocks = {(r, r): np.zeros((6, 6)) for r in range(na)}
    jit = 0.3 / np.sqrt(na)
    for r, c in list(pairs) + list(zero_pairs):
        assert 0 <= r < na and 0 <= c < na and r != c
        Q1, Q2 = (np.linalg.qr(rng.normal(size=(6, 6)))[0] for _ in range(2))
        D = np.diag(rng.uniform(0.5, 2.0, 6))
        J = D @ np.hstack([-(Q1 + jit * rng.normal(size=(6, 6))), Q2 + jit * rng.normal(size=(6, 6))])
        if (r, c) in zero_pairs:
            J = 0.0 * J
        G = J.T @ J
        blocks[(r, r)] = blocks[(r, r)] + G[:6, :6]
        blocks[(c, c)] = blocks[(c, c)] + G[6:, 6:]
        blocks[(r, c)] = blocks.get((r, c), 0) + G[:6, 6:]
        blocks[(c, r)] = blocks.get((c, r), 0) + G[6:, :6]
    if anchor > 0:
        J0 = np.linalg.qr(rng.normal(size=(6, 6)))[0] @ np.diag(rng.uniform(0.5, 2.0, 6))
        blocks[(0, 0)] = blocks[(0, 0)] + anchor * J0.T @ J0
    keys = sorted(blocks)
    index = {k: q for q, k in enumerate(keys)}
    H = np.stack([blocks[k] for k in keys]).reshape(-1, 36)
    rows = np.array([k[0] for k in keys])
    col = np.array([k[1] for k in keys], dtype=np.int32)
    rptr = np.searchsorted(rows, np.arange(na + 1)).astype(np.int32)
    tri = np.array([[index.get((r, r - 1), -1), index[(r, r)], index.get((r, r + 1), -1)] for r in range(na)], dtype=np.int32)
    return {'H': H, 'rptr': rptr, 'col': col, 'tri': tri, 'diag': tri[:, 1].copy(), 'b': rng.normal(size=(na, 6)), 'na': na}


def bsr_matrix(H, rptr, col, na, keep=None):
    """scipy-sparse (csc) matrix of a block-CSR H; keep: the block indices to keep (the others are dropped)"""
    import scipy.sparse as sp
    H = np.asarray(H, dtype=np.float64).reshape(-1, 6, 6)
    rows = np.repeat(np.arange(na), np.diff(rptr))
    q = np.arange(len(col)) if keep is None else np.asarray(keep)
    rr, cc = np.meshgrid(np.arange(6), np.arange(6), indexing='ij')
    i = (6 * rows[q, None, None] + rr).ravel()
    j = (6 * np.asarray(col)[q, None, None] + cc).ravel()
    return sp.csc_matrix((H[q].ravel(), (i, j)), shape=(6 * na, 6 * na))


def tri_part(H, rptr, col, tri, na):
    """the block-tridiagonal part the solver's preconditioner keeps (tri's -1 entries are absent blocks)"""
    t = np.asarray(tri).reshape(-1)
    return bsr_matrix(H, rptr, col, na, keep=t[t >= 0])


def residual_hp(H, rptr, col, na, lam, d, b):
    """||(H + lam I) d + b|| / ||b|| in numpy.longdouble"""
    Hh = np.asarray(H).reshape(-1, 6, 6).astype(HP)
    dh, bh = np.asarray(d).reshape(na, 6).astype(HP), np.asarray(b).reshape(na, 6).astype(HP)
    rows = np.repeat(np.arange(na), np.diff(rptr))
    y = HP(lam) * dh + bh
    np.add.at(y, rows, np.einsum('qij,qj->qi', Hh, dh[np.asarray(col)]))
    return float(np.sqrt((y * y).sum() / (bh * bh).sum()))


def cond_spd(M):
    """2-norm condition number of a sparse SPD matrix from its extreme eigenvalues (Lanczos; shift-invert at 0 for the
    smallest); dense below 600 rows"""
    import scipy.sparse.linalg as spl
    n = M.shape[0]
    if n < 600:
        w = np.linalg.eigvalsh(M.toarray())
        return float(w[-1] / w[0])
    hi = spl.eigsh(M, k=1, which='LA', return_eigenvectors=False, tol=1e-6)[0]
    lo = spl.eigsh(M, k=1, sigma=0.0, which='LM', return_eigenvectors=False, tol=1e-6)[0]
    return float(hi / lo)


def pcg_reference(M, P, b, tol, max_iter, perm=None, iterates=False):
    """The solver's PCG restated in numpy: M d = -b from d = 0, preconditioner an exact sparse-LU solve with P, the same
    stopping rule (||r|| <= tol ||b||, tested after the update, or max_iter).  perm: evaluate every dot product and matrix-
    vector product with the unknowns in this order (a different summation order, the same arithmetic otherwise).
    -> dict(d, iterations, residual (the recurrence's ||r|| / ||b||), iterates [d after each iteration] if asked)"""
    import scipy.sparse.linalg as spl
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = len(b)
    M = M.tocsr()
    if perm is None:
        dot, mv = np.dot, lambda x: M @ x
    else:
        Mp = M[:, perm].tocsr()
        dot, mv = (lambda x, y: np.dot(x[perm], y[perm])), (lambda x: Mp @ x[perm])
    d, r = np.zeros(n), -b.copy()
    rhs2 = dot(r, r)
    rr, it, its = rhs2, 0, []
    if rhs2 > 0:
        lu = spl.splu(P.tocsc())
        z = lu.solve(r)
        p = z.copy()
        rz = dot(r, z)
        stop2 = tol * tol * rhs2
        while it < max_iter:
            q = mv(p)
            alpha = rz / dot(p, q)
            d = d + alpha * p
            r = r - alpha * q
            rr = dot(r, r)
            it += 1
            if iterates:
                its.append(d.copy())
            if not rr > stop2:
                break
            z = lu.solve(r)
            rz_new = dot(r, z)
            p = z + (rz_new / rz) * p
            rz = rz_new
    return {'d': d, 'iterations': it, 'residual': float(np.sqrt(rr / rhs2)) if rhs2 > 0 else 0.0, 'iterates': its}
