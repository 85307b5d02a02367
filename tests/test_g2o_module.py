"""The g2o-named module (cl-slam_amd/g2o): it is what `import g2o` finds, it serves the reference's
slam/pose_graph_optimization.py unchanged (loaded by path where the reference checkout exists, with slam.py's call
sequence), and an independent twin of that sequence runs on the MI355X."""
import importlib.util
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np
import pytest

import pgo_reference as R

ROOT = Path(__file__).resolve().parents[1]
REF = Path('/root/reference')


def _fresh_g2o():
    """the package under cl-slam_amd/g2o, whatever another test put into sys.modules['g2o'] (tests/ref_stubs.py does)"""
    spec = importlib.util.spec_from_file_location('g2o', ROOT / 'cl-slam_amd' / 'g2o' / '__init__.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_import_g2o_resolves_to_this_package():
    import importlib
    saved = sys.modules.pop('g2o', None)
    try:
        g2o = importlib.import_module('g2o')
        assert Path(g2o.__file__).resolve() == (ROOT / 'cl-slam_amd' / 'g2o' / '__init__.py').resolve()
        assert g2o.__version__.endswith('clslam_hip')
    finally:
        sys.modules.pop('g2o', None)
        if saved is not None:
            sys.modules['g2o'] = saved


def test_api_subset_without_device():
    g2o = _fresh_g2o()
    m = np.eye(4); m[:3, 3] = [1, 2, 3]
    T = g2o.Isometry3d(m)
    assert np.array_equal(T.matrix(), m) and np.array_equal(T.t, [1, 2, 3]) and np.array_equal(T.translation(), [1, 2, 3])
    U = g2o.Isometry3d(R._rot(0.3, 0.1, -0.2), [0.5, 0, 1])
    assert np.allclose((U * U.inverse()).matrix(), np.eye(4))
    assert np.allclose((T * U).matrix(), m @ U.matrix()) and np.array_equal(U.rotation_matrix(), U.R)
    k = g2o.RobustKernelHuber()
    assert k.delta() == 1.0
    k.set_delta(2.5)
    assert k.delta() == 2.5
    for name in ('BlockSolverSE3', 'LinearSolverCholmodSE3', 'LinearSolverEigenSE3', 'LinearSolverPCGSE3',
                 'OptimizationAlgorithmLevenberg', 'ParameterSE3Offset'):
        getattr(g2o, name)()
    with pytest.raises(NotImplementedError):
        g2o.VertexPointXYZ()
    with pytest.raises(NotImplementedError):
        g2o.EdgeSE3PointXYZ()
    with pytest.raises(NotImplementedError):
        g2o.VertexSE2


def _drive_reference_pattern(pgo_cls, g2o, d):
    """slam.py's sequence: fixed start vertex, then per frame a vertex at the chained odometry pose + an odometry edge,
    loop edges with 0.5x the information at their frame, optimize(max_iterations=10000) after each loop closure"""
    cov = np.eye(6); cov[2, 2] = .1; cov[5, 5] = .1
    pg = pgo_cls()
    loops = {}
    for k in range(d['n_odom'], len(d['edges'])):
        i, j = d['edges'][k]
        loops.setdefault(int(i), []).append((int(j), d['meas'][k]))
    ids = d['ids']
    pg.add_vertex(int(ids[0]), d['gt'][0], fixed=True)
    n_opt = 0
    for k in range(1, len(ids)):
        z = d['meas'][k - 1]
        pose = pg.get_pose(pg.vertex_ids[-1]) @ z
        pg.add_vertex(int(ids[k]), pose)
        pg.add_edge((pg.vertex_ids[-2], int(ids[k])), z, information=np.linalg.inv(cov))
        for j, zl in loops.get(k, []):
            pg.get_transform(int(ids[k]), int(ids[j]))
            pg.add_edge((int(ids[k]), int(ids[j])), zl, information=.5 * np.linalg.inv(cov), is_loop_closure=True)
        if k in loops:
            pg.optimize(max_iterations=10000, verbose=False)
            n_opt += 1
    return pg, n_opt


def _dense_like_slam(d):
    """the dense reference driven through the same sequence (optimise after each loop frame, starting from the last result)"""
    n = len(d['ids'])
    poses = np.zeros((n, 4, 4))
    poses[0] = d['gt'][0]
    loop_frames = sorted({int(d['edges'][k][0]) for k in range(d['n_odom'], len(d['edges']))})
    done = 0
    for f in loop_frames + [n - 1]:
        for k in range(done + 1, f + 1):
            poses[k] = poses[k - 1] @ d['meas'][k - 1]
        done = f
        sel = [k for k, (a, b) in enumerate(d['edges']) if a <= f and b <= f]
        g = R.Graph(d['ids'][:f + 1], poses[:f + 1], d['fixed'][:f + 1], d['edges'][sel], d['meas'][sel], d['info'][sel])
        if f in loop_frames:
            poses[:f + 1], _ = R.lm(g)
    return poses


def _check_result(poses, d, ratio=0.65, tol_t=1e-6):
    ref = _dense_like_slam(d)
    ate_odom, ate_opt = R.ate(d['poses'], d['gt']), R.ate(poses, d['gt'])
    assert ate_opt < ratio * ate_odom, (ate_opt, ate_odom)      # measured 0.53-0.58 on the two CPU sequences
    assert np.abs(poses[:, :3, 3] - ref[:, :3, 3]).max() <= tol_t


@pytest.mark.skipif(not (REF / 'slam' / 'pose_graph_optimization.py').exists(), reason='reference checkout absent')
def test_reference_pose_graph_module_runs_unchanged(monkeypatch, tmp_path):
    from emu_util import use_backend
    use_backend('emu')
    g2o = _fresh_g2o()
    monkeypatch.setitem(sys.modules, 'g2o', g2o)
    monkeypatch.setitem(sys.modules, 'cv2', MagicMock())
    slam_pkg = type(sys)('slam')
    slam_pkg.__path__ = [str(REF / 'slam')]
    monkeypatch.setitem(sys.modules, 'slam', slam_pkg)
    for name in ('meshlab', 'pose_graph_optimization'):
        spec = importlib.util.spec_from_file_location(f'slam.{name}', REF / 'slam' / f'{name}.py')
        mod = importlib.util.module_from_spec(spec)
        monkeypatch.setitem(sys.modules, f'slam.{name}', mod)
        spec.loader.exec_module(mod)
    PGO = sys.modules['slam.pose_graph_optimization'].PoseGraphOptimization
    assert issubclass(PGO, g2o.SparseOptimizer)
    d = R.make_graph(90, 8, seed=21, start_id=0, lap=60)
    pg, n_opt = _drive_reference_pattern(PGO, g2o, d)
    assert n_opt == 8
    assert all(isinstance(v, g2o.VertexSE3) for v in pg.vertices().values())
    poses = np.stack(pg.get_all_poses())
    _check_result(poses, d)
    pg.visualize_in_meshlab(tmp_path / 'pose_graph.obj', verbose=False)
    assert np.allclose(pg.get_transform(0, 5), np.linalg.inv(poses[0]) @ poses[5])


class _SlamLikeGraph:
    """an independent restatement of the calling pattern (no reference code): a g2o.SparseOptimizer subclass"""

    @staticmethod
    def make(g2o):
        class G(g2o.SparseOptimizer):
            def __init__(self):
                self.edge_vertices = set()
                super().__init__()
                super().set_algorithm(g2o.OptimizationAlgorithmLevenberg(g2o.BlockSolverSE3(g2o.LinearSolverCholmodSE3())))
                p = g2o.ParameterSE3Offset()
                p.set_id(0)
                super().add_parameter(p)

            @property
            def vertex_ids(self):
                return sorted(self.vertices().keys())

            def optimize(self, max_iterations=1000, verbose=False):
                super().initialize_optimization()
                super().set_verbose(verbose)
                return super().optimize(max_iterations)

            def add_vertex(self, vertex_id, pose, fixed=False):
                v = g2o.VertexSE3()
                v.set_id(vertex_id)
                v.set_estimate(g2o.Isometry3d(pose))
                v.set_fixed(fixed)
                return super().add_vertex(v)

            def add_edge(self, vertices, measurement, information=np.eye(6), robust_kernel=None, is_loop_closure=False):
                self.edge_vertices.add(vertices)
                e = g2o.EdgeSE3()
                for i, v in enumerate(vertices):
                    e.set_vertex(i, self.vertex(v) if isinstance(v, int) else v)
                e.set_measurement(g2o.Isometry3d(measurement))
                e.set_information(information)
                if robust_kernel is not None:
                    e.set_robust_kernel(robust_kernel)
                return super().add_edge(e)

            def get_pose(self, vertex_id):
                return self.vertex(vertex_id).estimate().matrix()

            def get_all_poses(self):
                return [self.get_pose(i) for i in self.vertex_ids]

            def get_transform(self, a, b):
                return np.linalg.inv(self.get_pose(a)) @ self.get_pose(b)
        return G


@pytest.mark.gpu
def test_slam_sequence_on_the_gpu():
    from emu_util import use_backend
    use_backend('hip')
    g2o = _fresh_g2o()
    G = _SlamLikeGraph.make(g2o)
    d = R.make_graph(300, 8, seed=23, start_id=0, lap=200)
    pg, n_opt = _drive_reference_pattern(G, g2o, d)
    assert n_opt == 8
    # ATE only falls from 3.21 to 2.99 m here (measured): the first 100 frames have no revisit; the exact agreement with the
    # dense reference is the check that matters.  1e-5 m: the far end of the 300-frame chain differs by 1.4e-6 m with chi2
    # equal (measured), the low-curvature bending mode described in test_pose_graph.py
    _check_result(np.stack(pg.get_all_poses()), d, ratio=0.99, tol_t=1e-5)
    # g2o's return conventions
    assert pg.add_vertex(0, np.eye(4)) is False
    assert pg.add_edge((0, 10 ** 6), np.eye(4)) is False
    assert pg.vertex(10 ** 6) is None
    assert pg.chi2() > 0 and len(pg.edges()) == len(d['edges'])
    est = pg.vertex(5).estimate()
    m = est.matrix(); m[0, 3] += 100
    assert not np.array_equal(pg.vertex(5).estimate().matrix(), m)      # estimate() is a copy


def test_slam_sequence_on_the_emulator():
    from emu_util import use_backend
    use_backend('emu')
    g2o = _fresh_g2o()
    G = _SlamLikeGraph.make(g2o)
    d = R.make_graph(60, 6, seed=5, start_id=0, lap=40)
    pg, n_opt = _drive_reference_pattern(G, g2o, d)
    assert n_opt == 6
    _check_result(np.stack(pg.get_all_poses()), d)
    assert pg.add_vertex(0, np.eye(4)) is False
    assert pg.add_edge((0, 10 ** 6), np.eye(4)) is False
