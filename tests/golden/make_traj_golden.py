#!/usr/bin/env python
"""Pin tests/traj_eval_reference.py (the float64 twin of the trajectory evaluators) against the REAL reference module.

    python tests/golden/make_traj_golden.py [reference root]

Imports slam/utils.py of the reference checkout (default: the `reference` directory next to this repository; cv2 and the
other packages it imports at module level come from tests/ref_stubs.py), runs calc_error, calc_sequence_errors, compute_ATE,
compute_RPE and scale_optimization on the seeded drive of traj_eval_reference.make_fixture(1000, 0) and writes
tests/golden/traj_eval.npz: the poses, the returned numbers and the log strings (data, no source).
Without the reference it prints PARITY UNPINNED and exits 3: nothing is faked."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / 'tests'))


def main() -> int:
    ref = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT.parent / 'reference'
    if not (ref / 'slam' / 'utils.py').exists():
        print(f'PARITY UNPINNED: no reference checkout at {ref}; tests/golden/traj_eval.npz not written')
        return 3
    import ref_stubs
    ref_stubs.install()
    # slam/utils.py and the slam/meshlab.py it imports, WITHOUT the package's __init__ (that pulls in the whole SLAM driver:
    # faiss, the networks): an empty package object that only knows where the reference's modules lie.  The one class utils.py
    # imports from depth_pose_prediction (never used on this path) comes from this repository's package.
    import importlib
    import types
    sys.path.insert(0, str(ROOT / 'cl-slam_amd'))
    pkg = types.ModuleType('slam')
    pkg.__path__ = [str(ref / 'slam')]
    sys.modules['slam'] = pkg
    U = importlib.import_module('slam.utils')
    import traj_eval_reference as R
    pred, gt = R.make_fixture(1000, 0)
    P, G = [p.copy() for p in pred], [g.copy() for g in gt]
    out = {'pred': pred, 'gt': gt}
    for flag, tag in ((False, 'plain'), (True, 'scaled')):
        out[f'log_{tag}'] = np.array(U.calc_error(P, G, optimize_scale=flag))
    out['sequence_errors'] = np.asarray(U.calc_sequence_errors(P, G), dtype=np.float64)
    scaled, scaling = U.scale_optimization(P, G)
    out['scaling'] = np.array(scaling)
    out['scaled_xyz'] = np.asarray([p[:3, 3] for p in scaled])
    out['sequence_errors_scaled'] = np.asarray(U.calc_sequence_errors(scaled, G), dtype=np.float64)
    out['overall'] = np.asarray(U.compute_overall_err(U.calc_sequence_errors(P, G)), dtype=np.float64)
    out['ate'] = np.array(U.compute_ATE(P, G))
    out['rpe'] = np.asarray(U.compute_RPE(P, G))
    out['dist'] = np.asarray(U.trajectory_distances(G), dtype=np.float64)
    xz_p, xz_g = np.ascontiguousarray(pred[:, [0, 2], 3]), np.ascontiguousarray(gt[:, [0, 2], 3])
    scaled2, scaling2 = U.scale_optimization(xz_p, xz_g)
    out['scaling_2d'], out['scaled_2d'] = np.array(scaling2), scaled2
    np.savez_compressed(OUT / 'traj_eval.npz', **out)
    print('wrote', OUT / 'traj_eval.npz', (OUT / 'traj_eval.npz').stat().st_size, 'bytes')
    print(out['log_plain'])
    print(out['log_scaled'])
    return 0


if __name__ == '__main__':
    sys.exit(main())
