"""TEST INFRASTRUCTURE: an independent float64 numpy restatement of the SE(3) pose-graph conventions of
cl-slam_amd/csrc/pose_graph.hip (g2o types/slam3d: compact-quaternion chart, right-multiplied updates, toVectorMQT error,
Huber) and of g2o's Levenberg rule, plus a seeded KITTI-like graph generator.

    exp_mqt / log_mqt / oplus / edge_error / jacobians   batched over a leading axis
    lm(graph, max_iterations)                            dense (or scipy-sparse) Levenberg -> (poses, stats)
    make_graph(n, n_loops, seed, start_id)               ground truth, odometry start, odometry + loop edges

Nothing here runs on the device; the kernels are checked against it."""
import numpy as np

JAC_STEP = 1e-6
ODOM_COV = np.diag([1.0, 1.0, 0.1, 1.0, 1.0, 0.1])          # slam.py's odometry covariance (information = its inverse)


# ---- chart --------------------------------------------------------------------------------------------------------------
def exp_mqt(v):
    """(n,6) (t, qxyz) -> (n,4,4); |qxyz|^2 > 1 gives the identity rotation"""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    x, y, z = v[:, 3], v[:, 4], v[:, 5]
    w2 = 1.0 - (x * x + y * y + z * z)
    bad = w2 < 0
    w = np.sqrt(np.where(bad, 0.0, w2))
    x, y, z = (np.where(bad, 0.0, a) for a in (x, y, z))
    w = np.where(bad, 1.0, w)
    T = np.zeros((len(v), 4, 4))
    T[:, 0, 0] = 1 - 2 * (y * y + z * z); T[:, 0, 1] = 2 * (x * y - z * w); T[:, 0, 2] = 2 * (x * z + y * w)
    T[:, 1, 0] = 2 * (x * y + z * w); T[:, 1, 1] = 1 - 2 * (x * x + z * z); T[:, 1, 2] = 2 * (y * z - x * w)
    T[:, 2, 0] = 2 * (x * z - y * w); T[:, 2, 1] = 2 * (y * z + x * w); T[:, 2, 2] = 1 - 2 * (x * x + y * y)
    T[:, :3, 3] = v[:, :3]
    T[:, 3, 3] = 1.0
    return T


def _quat(R):
    """Eigen's matrix -> quaternion (x, y, z, w), one matrix"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
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


def log_mqt(T):
    """(n,4,4) -> (n,6) (t, xyz of the unit quaternion with w >= 0)"""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    out = np.zeros((len(T), 6))
    for n, M in enumerate(T):
        q = _quat(M[:3, :3])
        q /= np.linalg.norm(q)
        if q[3] < 0:
            q = -q
        out[n, :3] = M[:3, 3]
        out[n, 3:] = q[:3]
    return out


def inv(T):
    T = np.asarray(T, dtype=np.float64)
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


def edge_error(Xi, Xj, Z):
    return log_mqt(inv(Z) @ inv(Xi) @ Xj)


def jacobians(Xi, Xj, Z, h=JAC_STEP):
    """(A, B) (n,6,6): central differences of edge_error in the increments of Xi and Xj"""
    Xi, Xj, Z = (np.asarray(a, dtype=np.float64).reshape(-1, 4, 4) for a in (Xi, Xj, Z))
    n = len(Xi)
    A, B = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for k in range(6):
        v = np.zeros((n, 6))
        v[:, k] = h
        Ep, Em = exp_mqt(v), exp_mqt(-v)
        A[:, :, k] = (edge_error(Xi @ Ep, Xj, Z) - edge_error(Xi @ Em, Xj, Z)) / (2 * h)
        B[:, :, k] = (edge_error(Xi, Xj @ Ep, Z) - edge_error(Xi, Xj @ Em, Z)) / (2 * h)
    return A, B


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


def active_order(g):
    used = np.zeros(len(g.ids), dtype=bool)
    used[g.edges.reshape(-1)] = True
    act = np.nonzero(used & ~g.fixed)[0]
    return act[np.argsort(g.ids[act], kind='stable')]


def linear_system(g, poses, sparse=False):
    act = active_order(g)
    na = len(act)
    pos = np.full(len(g.ids), -1)
    pos[act] = np.arange(na)
    Xi, Xj = poses[g.edges[:, 0]], poses[g.edges[:, 1]]
    e = edge_error(Xi, Xj, g.meas)
    A, B = jacobians(Xi, Xj, g.meas)
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
