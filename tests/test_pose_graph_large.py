"""The KITTI-00-sized pose graph (4541 vertices, ~30 loop edges, slam.py's information matrices) on the MI355X:
convergence, ATE, chi2 against a float64 scipy-sparse host Levenberg, bitwise determinism; wall time printed only."""
import time

import numpy as np
import pytest

import pgo_reference as R

N, LOOPS = 4541, 30


def _load(d):
    from clslam_hip.pose_graph import PoseGraph
    pg = PoseGraph()
    for k in range(len(d['ids'])):
        pg.add_vertex(int(d['ids'][k]), d['poses'][k], bool(d['fixed'][k]))
    for k, (a, b) in enumerate(d['edges']):
        pg.add_edge(int(d['ids'][a]), int(d['ids'][b]), d['meas'][k], d['info'][k])
    return pg


@pytest.mark.gpu
def test_kitti_sized_graph():
    from emu_util import use_backend
    use_backend('hip')
    d = R.make_graph(N, LOOPS, seed=0, lap=300, sig_t=0.02, sig_r=3e-4)
    pg = _load(d)
    g0 = np.linalg.norm(pg.gradient())
    t = time.perf_counter()
    it = pg.optimize(10000)
    wall = time.perf_counter() - t
    g1 = np.linalg.norm(pg.gradient())
    P = np.stack([pg.get_estimate(int(i)) for i in d['ids']])
    stats = dict(pg.last_stats)
    print(f'\n4541-vertex graph: {it} LM iterations, {wall * 1e3:.1f} ms, CG iterations {stats["cg_iterations"]}, '
          f'CG relative residuals {["%.2g" % r for r in stats["cg_residual"]]}, preconditioner failures {stats["precond_failed"]}, '
          f'chi2 {stats["chi2"]:.6g}, |grad| {g0:.3g} -> {g1:.3g}, ATE {R.ate(d["poses"], d["gt"]):.3f} -> {R.ate(P, d["gt"]):.3f} m', flush=True)
    assert g1 <= 1e-8 * g0
    assert R.ate(P, d['gt']) < R.ate(d['poses'], d['gt'])
    again = _load(d)
    again.optimize(10000)
    assert np.array_equal(np.stack([again.get_estimate(int(i)) for i in d['ids']]), P)
    pytest.importorskip('scipy')
    ref, st = R.lm(R.graph_of(d), sparse=True)
    print(f'scipy host LM: {st["iterations"]} iterations, chi2 {st["chi2"]:.6g}', flush=True)
    assert abs(stats['chi2'] - st['chi2']) <= 1e-9 * st['chi2']
