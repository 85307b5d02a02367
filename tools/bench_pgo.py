#!/usr/bin/env python
"""Time PoseGraph.optimize() (csrc/pose_graph.hip) on a seeded KITTI-00-sized synthetic graph from tests/pgo_reference.py:
4541 vertices, 30 loop edges, slam.py's information matrices (inv(diag(1,1,.1,1,1,.1)), 0.5x for loop edges).

  cold    optimize(10000) from the pure-odometry start
  steady  a converged graph gets one more loop edge, then optimize(10000) again (what slam.py does at each loop closure)

Prints, per scenario: median wall time over --reps runs, LM iterations, CG iterations per LM trial, final chi2 and ATE;
with --scipy also a float64 scipy-sparse host Levenberg (same rule, direct solve) once per scenario.

    python tools/bench_pgo.py [--reps 5] [--scipy]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / 'cl-slam_amd'), str(ROOT / 'tests')]

import pgo_reference as R  # noqa: E402

N, LOOPS = 4541, 30


def _graph(d, n_edges):
    from clslam_hip.pose_graph import PoseGraph
    pg = PoseGraph()
    for k in range(len(d['ids'])):
        pg.add_vertex(int(d['ids'][k]), d['poses'][k], bool(d['fixed'][k]))
    for k in range(n_edges):
        a, b = d['edges'][k]
        pg.add_edge(int(d['ids'][a]), int(d['ids'][b]), d['meas'][k], d['info'][k])
    return pg


def _timed(pg):
    import torch
    t = time.perf_counter()
    it = pg.optimize(10000)         # returns after the estimates are back on the host
    torch.cuda.synchronize()
    return time.perf_counter() - t, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scipy', action='store_true')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_pgo.py measures the MI355X'
    d = R.make_graph(N, LOOPS, seed=0, lap=300, sig_t=0.02, sig_r=3e-4)
    ne = len(d['edges'])
    _timed(_graph(d, ne))           # warm-up: code objects, allocator
    out = {}
    for name in ('cold', 'steady'):
        times, res = [], None
        for _ in range(args.reps):
            if name == 'cold':
                pg = _graph(d, ne)
            else:
                pg = _graph(d, ne - 1)
                pg.optimize(10000)
                a, b = d['edges'][ne - 1]
                pg.add_edge(int(d['ids'][a]), int(d['ids'][b]), d['meas'][ne - 1], d['info'][ne - 1])
            dt, it = _timed(pg)
            times.append(dt)
            P = np.stack([pg.get_estimate(int(i)) for i in d['ids']])
            st = pg.last_stats
            res = {'lm_iterations': it, 'cg_per_trial': st['cg_iterations'], 'chi2': st['chi2'], 'ate_m': R.ate(P, d['gt'])}
        res['median_ms'] = 1e3 * float(np.median(times))
        res['all_ms'] = [round(1e3 * t, 3) for t in times]
        if args.scipy:
            try:
                import scipy  # noqa: F401
                g = R.graph_of(d)
                if name == 'steady':
                    g.edges, g.meas, g.info, g.delta = g.edges[:-1], g.meas[:-1], g.info[:-1], g.delta[:-1]
                    g.poses, _ = R.lm(g, sparse=True)
                    g = R.Graph(d['ids'], g.poses, d['fixed'], d['edges'], d['meas'], d['info'])
                t = time.perf_counter()
                ref, st = R.lm(g, sparse=True)
                res['scipy'] = {'ms': 1e3 * (time.perf_counter() - t), 'lm_iterations': st['iterations'], 'chi2': st['chi2'],
                                'ate_m': R.ate(ref, d['gt'])}
            except ImportError:
                res['scipy'] = None
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    out['odometry_ate_m'] = R.ate(d['poses'], d['gt'])
    print(json.dumps({'odometry_ate_m': out['odometry_ate_m'], 'vertices': N, 'edges': ne}))


if __name__ == '__main__':
    main()
