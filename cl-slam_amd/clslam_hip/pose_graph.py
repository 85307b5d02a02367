"""SE(3) pose graph on the MI355X: the storage and Levenberg control behind the ``g2o``-named module (cl-slam_amd/g2o), i.e.
the back end of the reference's slam/pose_graph_optimization.py (g2o.SparseOptimizer + BlockSolverSE3 +
OptimizationAlgorithmLevenberg over VertexSE3 / EdgeSE3) as slam/slam.py drives it (:110-115, :203-216, :241-246).

The linear algebra is csrc/pose_graph.hip (fp64; the chart, error, Huber and solver conventions are stated in its header).
This file keeps the graph in numpy arrays, mirrors it in fp64 device tensors (only what changed since the last optimize()
is uploaded) and runs g2o's Levenberg rule on the host with one small scalar read-back per trial step:

    lambda_0 = 1e-5 * max diag(H); the damping is H + lambda I
    rho = (chi2_old - chi2_new) / (d^T (lambda d + b_g2o) + 1e-3), b_g2o = -J^T W e (g2o's sign of b)
    success (rho > 0, chi2_new finite): lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2, the step is kept
    failure: lambda *= nu, nu *= 2, the step is dropped; up to 10 trials per iteration
    stop: 10 failed trials, rho == 0, a non-finite lambda, max_iterations, or (not in g2o) an accepted step whose chi2
          decrease is below 1e-12 * chi2 -- fp64 noise; without it optimize(10000) would run on long past convergence.

chi2 here is the robust sum(rho(e^T Omega e)) the Levenberg rule scores; chi2(robust=False) is the plain sum.
optimize() runs on a stream of its own and never synchronises the device or another stream; it copies the estimates back
to the host before it returns.  Only vertices that are not fixed and take part in at least one edge move (g2o's
initializeOptimization leaves the others out)."""
import contextlib
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, ops

CG_TOL = 1e-10          # PCG stop: ||r|| <= CG_TOL * ||b||
CG_MAX_ITER = 2000      # PCG iteration cap per solve
LM_MAX_TRIALS = 10      # g2o's maxTrialsAfterFailure
LM_TAU = 1e-5           # g2o's initial lambda factor
LM_MIN_REL_DECREASE = 1e-12


def _grow(a: np.ndarray, n: int) -> np.ndarray:
    if n <= a.shape[0]:
        return a
    out = np.zeros((max(n, 2 * a.shape[0]),) + a.shape[1:], dtype=a.dtype)
    out[:a.shape[0]] = a
    return out


class PoseGraph:
    def __init__(self, device=None) -> None:
        lib = _lib.get_lib()
        self.device = torch.device(device) if device is not None else torch.device(lib.device_type)
        self._slot: Dict[int, int] = {}                 # vertex id -> slot (insertion order)
        self._vid = np.zeros(64, dtype=np.int64)
        self._est = np.zeros((64, 4, 4))
        self._fixed = np.zeros(64, dtype=bool)
        self._ev = np.zeros((64, 2), dtype=np.int32)     # edge (from, to) slots
        self._meas = np.zeros((64, 4, 4))
        self._info = np.zeros((64, 6, 6))
        self._huber = np.zeros(64)
        self.nv = 0
        self.ne = 0
        # device mirror
        self._dev: Dict[str, torch.Tensor] = {}
        self._up_v = 0                                   # slots [0, _up_v) uploaded
        self._up_e = 0
        self._dirty_v: set = set()
        self._dirty_e: set = set()
        self._struct_dirty = True
        self._na = 0
        self._stream = None
        self.last_stats: dict = {}

    # -- graph edits (host, O(1) amortised) ----------------------------------------------------------------------------
    def has_vertex(self, vid: int) -> bool:
        return int(vid) in self._slot

    def add_vertex(self, vid: int, pose, fixed: bool = False) -> bool:
        vid = int(vid)
        if vid in self._slot:
            return False
        s = self.nv
        self._vid, self._est, self._fixed = _grow(self._vid, s + 1), _grow(self._est, s + 1), _grow(self._fixed, s + 1)
        self._vid[s] = vid
        self._est[s] = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        self._fixed[s] = bool(fixed)
        self._slot[vid] = s
        self.nv = s + 1
        self._struct_dirty = True
        return True

    def set_estimate(self, vid: int, pose) -> None:
        s = self._slot[int(vid)]
        self._est[s] = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        if s < self._up_v:
            self._dirty_v.add(s)

    def get_estimate(self, vid: int) -> np.ndarray:
        return self._est[self._slot[int(vid)]].copy()

    def set_fixed(self, vid: int, fixed: bool) -> None:
        s = self._slot[int(vid)]
        if bool(fixed) != bool(self._fixed[s]):
            self._fixed[s] = bool(fixed)
            self._struct_dirty = True

    def is_fixed(self, vid: int) -> bool:
        return bool(self._fixed[self._slot[int(vid)]])

    def vertex_ids(self) -> np.ndarray:
        """ids in insertion order"""
        return self._vid[:self.nv].copy()

    def add_edge(self, vid_from: int, vid_to: int, measurement, information=None, huber_delta: Optional[float] = None) -> int:
        """-> edge index; KeyError when a vertex is missing"""
        a, b = self._slot[int(vid_from)], self._slot[int(vid_to)]
        k = self.ne
        self._ev, self._meas, self._info, self._huber = (_grow(self._ev, k + 1), _grow(self._meas, k + 1), _grow(self._info, k + 1),
                                                         _grow(self._huber, k + 1))
        self._ev[k] = (a, b)
        self.ne = k + 1
        self.set_edge(k, measurement, np.eye(6) if information is None else information, huber_delta)
        self._struct_dirty = True
        return k

    def set_edge(self, k: int, measurement=None, information=None, huber_delta=False) -> None:
        """update edge k's measurement / information / Huber delta (None = no robust kernel; False = unchanged)"""
        if measurement is not None:
            self._meas[k] = np.asarray(measurement, dtype=np.float64).reshape(4, 4)
        if information is not None:
            om = np.asarray(information, dtype=np.float64).reshape(6, 6)
            self._info[k] = 0.5 * (om + om.T)
        if huber_delta is not False:
            self._huber[k] = -1.0 if huber_delta is None else float(huber_delta)
        if k < self._up_e:
            self._dirty_e.add(k)

    # -- device mirror ---------------------------------------------------------------------------------------------------
    def _ctx(self):
        if self.device.type == 'cuda':
            if self._stream is None:
                self._stream = torch.cuda.Stream(self.device)
            return torch.cuda.stream(self._stream), self._stream.cuda_stream
        return contextlib.nullcontext(), 0

    def _buf(self, name: str, rows: int, cols: int, dtype=torch.float64, keep: int = 0) -> torch.Tensor:
        """device tensor of at least `rows` rows (capacity doubles); the first `keep` rows survive a regrowth"""
        t = self._dev.get(name)
        if t is None or t.shape[0] < rows:
            n = max(rows, 64, 0 if t is None else 2 * t.shape[0])
            g = torch.empty((n, cols), dtype=dtype, device=self.device)
            if t is not None and keep:
                g[:keep] = t[:keep]
            self._dev[name] = t = g
        return t

    def _h2d(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _upload(self) -> None:
        nv, ne = self.nv, self.ne
        est = self._buf('est', nv, 16, keep=self._up_v)
        self._buf('trial', nv, 16)
        if nv > self._up_v:
            est[self._up_v:nv] = self._h2d(self._est[self._up_v:nv].reshape(-1, 16))
        if self._dirty_v:
            s = np.fromiter(sorted(self._dirty_v), dtype=np.int64)
            est[self._h2d(s)] = self._h2d(self._est[s].reshape(-1, 16))
        self._up_v, self._dirty_v = nv, set()
        names = (('ev', 2, torch.int32, lambda a, b: self._ev[a:b]), ('meas', 16, torch.float64, lambda a, b: self._meas[a:b].reshape(-1, 16)),
                 ('info', 36, torch.float64, lambda a, b: self._info[a:b].reshape(-1, 36)), ('huber', 1, torch.float64, lambda a, b: self._huber[a:b, None]))
        dirty = np.fromiter(sorted(self._dirty_e), dtype=np.int64) if self._dirty_e else None
        for name, cols, dt, rows in names:
            t = self._buf(name, ne, cols, dt, keep=self._up_e)
            if ne > self._up_e:
                t[self._up_e:ne] = self._h2d(rows(self._up_e, ne))
            if dirty is not None and name != 'ev':
                src = {'meas': self._meas[dirty].reshape(-1, 16), 'info': self._info[dirty].reshape(-1, 36), 'huber': self._huber[dirty, None]}[name]
                t[self._h2d(dirty)] = self._h2d(src)
        self._up_e, self._dirty_e = ne, set()

    def _sync_structure(self) -> None:
        """active set (not fixed, in >= 1 edge; ordered by vertex id) and the block-CSR pattern of H: rebuilt on the host only
        when vertices, edges or fixed flags changed since the last optimize()"""
        if not self._struct_dirty:
            return
        nv, ne = self.nv, self.ne
        ev = self._ev[:ne]
        used = np.zeros(nv, dtype=bool)
        used[ev.reshape(-1)] = True
        cand = np.nonzero(used & ~self._fixed[:nv])[0]
        cand = cand[np.argsort(self._vid[cand], kind='stable')]
        act = np.full(nv, -1, dtype=np.int32)
        act[cand] = np.arange(len(cand), dtype=np.int32)
        na = len(cand)
        self._act_host = act
        self._na = na
        dev = {'act': self._h2d(act if nv else np.zeros(1, np.int32))}
        if na:
            e = np.arange(ne, dtype=np.int64)
            ai, aj = act[ev[:, 0]].astype(np.int64), act[ev[:, 1]].astype(np.int64)
            mi, mj = ai >= 0, aj >= 0
            both = mi & mj
            rows = np.concatenate([ai[mi], aj[mj], ai[both], aj[both]])
            cols = np.concatenate([ai[mi], aj[mj], aj[both], ai[both]])
            code = np.concatenate([e[mi] * 4, e[mj] * 4 + 1, e[both] * 4 + 2, e[both] * 4 + 3])
            order = np.lexsort((code, cols, rows))
            rows, cols, code = rows[order], cols[order], code[order]
            key = rows * na + cols
            ukey, start = np.unique(key, return_index=True)
            nnzb = len(ukey)
            cptr = np.append(start, len(key)).astype(np.int32)
            urow, ucol = ukey // na, ukey % na
            rptr = np.searchsorted(urow, np.arange(na + 1)).astype(np.int32)

            def find(r, c):
                k = r * na + c
                p = np.searchsorted(ukey, k)
                ok = (c >= 0) & (c < na) & (p < nnzb)
                ok[ok] &= ukey[p[ok]] == k[ok]
                return np.where(ok, p, -1)

            r = np.arange(na, dtype=np.int64)
            diag = find(r, r)
            assert (diag >= 0).all()
            tri = np.stack([find(r, r - 1), diag, find(r, r + 1)], axis=1).astype(np.int32)
            dev.update(cptr=self._h2d(cptr), contrib=self._h2d(code.astype(np.int32)), diag=self._h2d(diag.astype(np.int32)),
                       rptr=self._h2d(rptr), col=self._h2d(ucol.astype(np.int32)), tri=self._h2d(tri))
            self._nnzb = nnzb
        self._sdev = dev
        self._struct_dirty = False

    # -- optimisation ---------------------------------------------------------------------------------------------------
    def _read(self) -> np.ndarray:
        return self._dev['scal'].cpu().numpy().reshape(-1)

    def _alloc_work(self) -> None:
        na, ne = self._na, self.ne
        self._buf('lin', ne, ops.pgo_lin_stride())
        self._buf('H', self._nnzb, 36)
        self._buf('b', na, 6)
        self._buf('delta', na, 6)
        self._buf('work', ops.pgo_solve_workspace(na), 1)
        self._buf('scal', 8, 1)

    def _build(self, stream) -> None:
        d, s = self._dev, self._sdev
        ops.pgo_build_system(d['est'], d['ev'], d['meas'], d['info'], d['huber'], self.ne, s['cptr'], s['contrib'], s['diag'],
                             self._nnzb, self._na, d['lin'], d['H'], d['b'], d['scal'], stream)

    def _score(self, stream, delta, robust: bool, out: int) -> None:
        d = self._dev
        ops.pgo_update_score(d['est'], d['trial'], self._sdev['act'], self.nv, delta, d['ev'], d['meas'], d['info'], d['huber'],
                             self.ne, robust, d['scal'], out, stream)

    def optimize(self, max_iterations: int) -> int:
        """g2o's Levenberg (module docstring) for at most max_iterations iterations -> iterations done"""
        stats = {'iterations': 0, 'cg_iterations': [], 'cg_residual': [], 'precond_failed': 0, 'chi2': None, 'lambda': None,
                 'trials': 0}
        self.last_stats = stats
        if max_iterations <= 0 or self.ne == 0:
            return 0
        ctx, stream = self._ctx()
        with ctx:
            self._sync_structure()
            if self._na == 0:
                return 0
            self._upload()
            self._alloc_work()
            d, s = self._dev, self._sdev
            self._score(stream, None, True, 4)
            lam, ni, chi2 = None, 2.0, None
            it = 0
            while it < max_iterations:
                self._build(stream)
                if lam is None:
                    r = self._read()
                    chi2, lam = float(r[4]), LM_TAU * float(r[0])
                trials, rho, accepted, chi2_before = 0, -1.0, False, chi2
                while True:
                    ops.pgo_solve(d['H'], s['rptr'], s['col'], s['tri'], d['b'], lam, self._na, CG_TOL, CG_MAX_ITER, d['delta'],
                                  d['work'], d['scal'], stream)
                    self._score(stream, d['delta'], True, 6)
                    r = self._read()
                    chi2_new = float(r[6])
                    stats['cg_iterations'].append(int(r[1]))
                    stats['cg_residual'].append(float(r[2]))     # the solver's own ||r|| / ||b|| where it stopped
                    stats['precond_failed'] += int(r[5] != 0.0)   # preconditioner not factorable: that solve returned d = 0
                    rho = (chi2 - chi2_new) / (float(r[3]) + 1e-3)
                    if rho > 0 and np.isfinite(chi2_new):
                        lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                        ni = 2.0
                        chi2 = chi2_new
                        d['est'], d['trial'] = d['trial'], d['est']
                        accepted = True
                    else:
                        lam *= ni
                        ni *= 2.0
                    trials += 1
                    if not (rho < 0 and trials < LM_MAX_TRIALS):
                        break
                it += 1
                stats['trials'] += trials
                if trials == LM_MAX_TRIALS or rho == 0 or not np.isfinite(lam):
                    break
                if accepted and chi2_before - chi2 < LM_MIN_REL_DECREASE * chi2_before:
                    break
            stats.update(iterations=it, chi2=chi2, **{'lambda': lam})
            self._est[:self.nv] = d['est'][:self.nv].cpu().numpy().reshape(-1, 4, 4)
        return it

    def chi2(self, robust: bool = False) -> float:
        """sum over edges of e^T Omega e at the current estimates (robust: of Huber rho)"""
        if self.ne == 0:
            return 0.0
        ctx, stream = self._ctx()
        with ctx:
            self._sync_structure()
            self._upload()
            self._buf('scal', 8, 1)
            self._score(stream, None, robust, 7)
            return float(self._read()[7])

    def gradient(self) -> np.ndarray:
        """b = J^T W e over the active vertices (rows in active order) at the current estimates"""
        ctx, stream = self._ctx()
        with ctx:
            self._sync_structure()
            if self._na == 0 or self.ne == 0:
                return np.zeros((0, 6))
            self._upload()
            self._alloc_work()
            self._build(stream)
            return self._dev['b'][:self._na].cpu().numpy().copy()

    def edge_eval(self, edges: Optional[List[int]] = None):
        """(err [n][6], jac_from [n][6][6], jac_to [n][6][6]) of the edges at the current estimates, on the device"""
        ctx, stream = self._ctx()
        with ctx:
            self._upload()
            idx = np.arange(self.ne) if edges is None else np.asarray(edges, dtype=np.int64)
            n = len(idx)
            if n == 0:
                return np.zeros((0, 6)), np.zeros((0, 6, 6)), np.zeros((0, 6, 6))
            ev = self._h2d(self._ev[idx])
            meas = self._h2d(self._meas[idx].reshape(-1, 16))
            err = torch.empty((n, 6), dtype=torch.float64, device=self.device)
            ja = torch.empty((n, 36), dtype=torch.float64, device=self.device)
            jb = torch.empty((n, 36), dtype=torch.float64, device=self.device)
            ops.pgo_edge_eval(self._dev['est'], ev, meas, err, ja, jb, stream)
            return err.cpu().numpy(), ja.cpu().numpy().reshape(n, 6, 6), jb.cpu().numpy().reshape(n, 6, 6)
