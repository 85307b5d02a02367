#!/usr/bin/env python
"""Pin the SE(3) pose-graph conventions (cl-slam_amd/csrc/pose_graph.hip, tests/pgo_reference.py) against a REAL g2opy --
the moment one is importable (the reference builds it from its third_party/g2opy submodule).

    python tests/golden/make_pgo_golden.py

What it does when a real g2o imports (one that is NOT this repository's cl-slam_amd/g2o):
  runs the seeded synthetic graphs of tests/pgo_reference.make_graph (10 / 150 / 600 vertices) through g2opy configured
  as slam/pose_graph_optimization.py configures it (BlockSolverSE3 + LinearSolverCholmodSE3 + Levenberg), optimize(10000),
  and writes tests/golden/pgo_g2o.npz: per graph the generator arguments, g2o's optimised poses, its chi2 and the
  iteration count (data, no source).
Without a real g2o it prints PARITY UNPINNED and exits 3: nothing is faked."""
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / 'tests'))
sys.path = [p for p in sys.path if Path(p or '.').resolve() != (ROOT / 'cl-slam_amd').resolve()]

GRAPHS = [(10, 2, 10), (150, 6, 150), (600, 20, 600)]      # (n, loops, seed) as tests/test_pose_graph.py makes them


def real_g2o():
    try:
        g2o = importlib.import_module('g2o')
    except ImportError:
        return None
    f = Path(getattr(g2o, '__file__', '') or '')
    if not hasattr(g2o, 'SparseOptimizer') or (f and (ROOT / 'cl-slam_amd') in f.resolve().parents):
        return None
    return g2o


def run(g2o, d):
    opt = g2o.SparseOptimizer()
    opt.set_algorithm(g2o.OptimizationAlgorithmLevenberg(g2o.BlockSolverSE3(g2o.LinearSolverCholmodSE3())))
    for k, vid in enumerate(d['ids']):
        v = g2o.VertexSE3()
        v.set_id(int(vid))
        v.set_estimate(g2o.Isometry3d(d['poses'][k]))
        v.set_fixed(bool(d['fixed'][k]))
        opt.add_vertex(v)
    for k, (a, b) in enumerate(d['edges']):
        e = g2o.EdgeSE3()
        e.set_vertex(0, opt.vertex(int(d['ids'][a])))
        e.set_vertex(1, opt.vertex(int(d['ids'][b])))
        e.set_measurement(g2o.Isometry3d(d['meas'][k]))
        e.set_information(d['info'][k])
        opt.add_edge(e)
    opt.initialize_optimization()
    it = opt.optimize(10000)
    poses = np.stack([opt.vertex(int(v)).estimate().matrix() for v in d['ids']])
    return poses, float(opt.chi2()), int(it)


def main() -> int:
    g2o = real_g2o()
    if g2o is None:
        print('PARITY UNPINNED: no real g2o (g2opy) is importable here; tests/golden/pgo_g2o.npz not written')
        return 3
    import pgo_reference as R
    out = {}
    for n, loops, seed in GRAPHS:
        d = R.make_graph(n, loops, seed=seed, start_id=5, lap=max(2, int(0.7 * n)))
        poses, chi2, it = run(g2o, d)
        out[f'n{n}_args'] = np.array([n, loops, seed, 5, max(2, int(0.7 * n))])
        out[f'n{n}_poses'], out[f'n{n}_chi2'], out[f'n{n}_iterations'] = poses, np.array(chi2), np.array(it)
        print(f'{n} vertices: g2o {it} iterations, chi2 {chi2:.12g}')
    np.savez_compressed(OUT / 'pgo_g2o.npz', **out)
    print('wrote', OUT / 'pgo_g2o.npz')
    return 0


if __name__ == '__main__':
    sys.exit(main())
