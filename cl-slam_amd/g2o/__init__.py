"""``g2o``-named module over the MI355X SE(3) pose-graph optimiser (clslam_hip.pose_graph) -- the SUBSET of g2opy the
reference's back end uses, so that slam/pose_graph_optimization.py (:1-35, :55-77, :92-140: a g2o.SparseOptimizer
subclass) and slam/slam.py (:110-115, :203-216, :241-246, :272-277) run unchanged where g2opy (third_party/g2opy, a
hand-built extension) is not installed:

    SparseOptimizer: set_algorithm / add_parameter / initialize_optimization / set_verbose / optimize(n) -> iterations
                     add_vertex / add_edge (False on a duplicate id or a missing vertex) / vertices() / vertex(id) / edges() / chi2()
    VertexSE3:       set_id / id / set_estimate / estimate (a copy) / set_fixed / fixed
    EdgeSE3:         set_vertex / vertex / set_measurement / measurement / set_information / information / set_robust_kernel
    Isometry3d(4x4 | R, t): matrix / R / t / translation / rotation_matrix / inverse / *
    RobustKernelHuber(delta=1.0): set_delta / delta
    BlockSolverSE3, LinearSolverCholmodSE3 / LinearSolverEigenSE3 / LinearSolverPCGSE3, OptimizationAlgorithmLevenberg,
    ParameterSE3Offset: accepted, configure nothing

Whatever solver is configured, optimize() runs g2o's Levenberg rule on the host over an fp64 Gauss-Newton system solved on
the GPU by preconditioned conjugate gradients (block-tridiagonal preconditioner over consecutive vertex ids, block cyclic
reduction); conventions and the one extra stopping rule are in clslam_hip/pose_graph.py and csrc/pose_graph.hip.
This directory is only on sys.path when cl-slam_amd/ is; remove it to use an installed g2opy instead.  Anything outside
the subset (VertexPointXYZ, EdgeSE3PointXYZ, save / load, other types) raises NotImplementedError instead of guessing."""
from typing import Dict, Optional

import numpy as np

from clslam_hip.pose_graph import PoseGraph

__version__ = '0+clslam_hip'


class Isometry3d:
    def __init__(self, *args) -> None:
        if len(args) == 0:
            m = np.eye(4)
        elif len(args) == 1:
            a = args[0]
            m = a.matrix() if isinstance(a, Isometry3d) else np.asarray(a, dtype=np.float64)
            if m.shape != (4, 4):
                raise ValueError(f'Isometry3d needs a 4x4 matrix, got {m.shape}')
        elif len(args) == 2:
            m = np.eye(4)
            m[:3, :3] = np.asarray(args[0], dtype=np.float64).reshape(3, 3)
            m[:3, 3] = np.asarray(args[1], dtype=np.float64).reshape(3)
        else:
            raise NotImplementedError('Isometry3d(matrix) or Isometry3d(R, t) only')
        self._m = np.array(m, dtype=np.float64)

    def matrix(self) -> np.ndarray:
        return self._m.copy()

    @property
    def R(self) -> np.ndarray:
        return self._m[:3, :3].copy()

    @property
    def t(self) -> np.ndarray:
        return self._m[:3, 3].copy()

    def translation(self) -> np.ndarray:
        return self.t

    def rotation_matrix(self) -> np.ndarray:
        return self.R

    def inverse(self) -> 'Isometry3d':
        Rt = self._m[:3, :3].T
        return Isometry3d(Rt, -Rt @ self._m[:3, 3])

    def __mul__(self, other):
        if isinstance(other, Isometry3d):
            return Isometry3d(self._m @ other._m)
        p = np.asarray(other, dtype=np.float64)
        if p.shape == (3,):
            return self._m[:3, :3] @ p + self._m[:3, 3]
        return NotImplemented

    def __repr__(self) -> str:
        return f'Isometry3d({self._m!r})'


class _Config:
    """solver / parameter classes: accepted, configure nothing (see the module docstring for the solver that runs)"""

    def __init__(self, *args, **kwargs) -> None:
        self._id = 0

    def set_id(self, i: int) -> None:
        self._id = int(i)

    def id(self) -> int:
        return self._id


class BlockSolverSE3(_Config):
    pass


class LinearSolverCholmodSE3(_Config):
    pass


class LinearSolverEigenSE3(_Config):
    pass


class LinearSolverPCGSE3(_Config):
    pass


class OptimizationAlgorithmLevenberg(_Config):
    pass


class ParameterSE3Offset(_Config):
    pass


class RobustKernelHuber:
    def __init__(self, delta: float = 1.0) -> None:
        self._delta = float(delta)

    def set_delta(self, delta: float) -> None:
        self._delta = float(delta)

    def delta(self) -> float:
        return self._delta


class VertexSE3:
    def __init__(self) -> None:
        self._id = -1
        self._est = np.eye(4)
        self._fixed = False
        self._graph: Optional[PoseGraph] = None

    def set_id(self, i: int) -> None:
        if self._graph is not None:
            raise RuntimeError('cannot change the id of a vertex in an optimizer')
        self._id = int(i)

    def id(self) -> int:
        return self._id

    def set_estimate(self, est) -> None:
        m = est.matrix() if isinstance(est, Isometry3d) else np.asarray(est, dtype=np.float64).reshape(4, 4)
        if self._graph is not None:
            self._graph.set_estimate(self._id, m)
        else:
            self._est = np.array(m, dtype=np.float64)

    def estimate(self) -> Isometry3d:
        return Isometry3d(self._graph.get_estimate(self._id) if self._graph is not None else self._est)

    def set_fixed(self, fixed: bool) -> None:
        if self._graph is not None:
            self._graph.set_fixed(self._id, bool(fixed))
        else:
            self._fixed = bool(fixed)

    def fixed(self) -> bool:
        return self._graph.is_fixed(self._id) if self._graph is not None else self._fixed


class EdgeSE3:
    def __init__(self) -> None:
        self._v = [None, None]
        self._meas = np.eye(4)
        self._info = np.eye(6)
        self._kernel: Optional[RobustKernelHuber] = None
        self._graph: Optional[PoseGraph] = None
        self._index = -1

    def set_vertex(self, i: int, v) -> None:
        if i not in (0, 1):
            raise IndexError('EdgeSE3 has vertices 0 and 1')
        if v is not None and not isinstance(v, VertexSE3):
            raise NotImplementedError('EdgeSE3 connects VertexSE3 only')
        self._v[i] = v

    def vertex(self, i: int):
        return self._v[i]

    def vertices(self):
        return list(self._v)

    def set_measurement(self, m) -> None:
        self._meas = np.array(m.matrix() if isinstance(m, Isometry3d) else np.asarray(m, dtype=np.float64).reshape(4, 4))
        if self._graph is not None:
            self._graph.set_edge(self._index, measurement=self._meas)

    def measurement(self) -> Isometry3d:
        return Isometry3d(self._meas)

    def set_information(self, info) -> None:
        self._info = np.array(info, dtype=np.float64).reshape(6, 6)
        if self._graph is not None:
            self._graph.set_edge(self._index, information=self._info)

    def information(self) -> np.ndarray:
        return self._info.copy()

    def set_robust_kernel(self, kernel) -> None:
        if kernel is not None and not isinstance(kernel, RobustKernelHuber):
            raise NotImplementedError('only RobustKernelHuber is provided')
        self._kernel = kernel
        if self._graph is not None:
            self._graph.set_edge(self._index, huber_delta=None if kernel is None else kernel.delta())

    def robust_kernel(self):
        return self._kernel

    def set_parameter_id(self, *args) -> None:
        raise NotImplementedError('EdgeSE3 takes no parameters in this subset')


class SparseOptimizer:
    """g2o.SparseOptimizer over VertexSE3 / EdgeSE3.  Usable as a Python base class the way the reference subclasses it
    (attributes set before super().__init__(), its own vertex_ids property, super().optimize(n) / super().add_vertex(v))."""

    def __init__(self) -> None:
        self._graph = PoseGraph()
        self._vertices: Dict[int, VertexSE3] = {}
        self._edges = []
        self._verbose = False

    def set_algorithm(self, algorithm) -> None:
        pass

    def add_parameter(self, parameter) -> bool:
        return True

    def initialize_optimization(self, *args) -> bool:
        return True

    def set_verbose(self, verbose: bool) -> None:
        self._verbose = bool(verbose)

    def vertices(self) -> Dict[int, VertexSE3]:
        return self._vertices

    def vertex(self, i: int) -> Optional[VertexSE3]:
        return self._vertices.get(int(i))

    def edges(self):
        return list(self._edges)

    def add_vertex(self, v) -> bool:
        if not isinstance(v, VertexSE3):
            raise NotImplementedError(f'{type(v).__name__} is outside the g2o subset provided here (VertexSE3 only)')
        if v._graph is not None or v.id() in self._vertices:
            return False
        self._graph.add_vertex(v.id(), v._est, v._fixed)
        v._graph = self._graph
        self._vertices[v.id()] = v
        return True

    def add_edge(self, e) -> bool:
        if not isinstance(e, EdgeSE3):
            raise NotImplementedError(f'{type(e).__name__} is outside the g2o subset provided here (EdgeSE3 only)')
        a, b = e._v
        if e._graph is not None or a is None or b is None:
            return False
        if self._vertices.get(a.id()) is not a or self._vertices.get(b.id()) is not b:
            return False
        e._index = self._graph.add_edge(a.id(), b.id(), e._meas, e._info, None if e._kernel is None else e._kernel.delta())
        e._graph = self._graph
        self._edges.append(e)
        return True

    def optimize(self, iterations: int, online: bool = False) -> int:
        n = self._graph.optimize(int(iterations))
        if self._verbose:
            st = self._graph.last_stats
            print(f'g2o (clslam_hip): {n} Levenberg iterations, chi2 {st.get("chi2")}, CG iterations {st.get("cg_iterations")}')
        return n

    def chi2(self) -> float:
        return self._graph.chi2(robust=False)

    def active_robust_chi2(self) -> float:
        return self._graph.chi2(robust=True)

    def save(self, *args, **kwargs):
        raise NotImplementedError('the g2o file format is outside the subset provided here')

    load = save


class _Unsupported:
    _what = ''

    def __init__(self, *args, **kwargs) -> None:
        raise NotImplementedError(f'g2o.{self._what} is outside the subset provided here (slam.py does not use it)')


class VertexPointXYZ(_Unsupported):
    _what = 'VertexPointXYZ'


class EdgeSE3PointXYZ(_Unsupported):
    _what = 'EdgeSE3PointXYZ'


def __getattr__(name: str):
    if name[:1].isupper():                       # a g2o type or solver this subset does not provide
        raise NotImplementedError(f'g2o.{name} is outside the subset provided here')
    raise AttributeError(name)


__all__ = ['Isometry3d', 'SparseOptimizer', 'VertexSE3', 'EdgeSE3', 'RobustKernelHuber', 'BlockSolverSE3', 'LinearSolverCholmodSE3',
           'LinearSolverEigenSE3', 'LinearSolverPCGSE3', 'OptimizationAlgorithmLevenberg', 'ParameterSE3Offset', 'VertexPointXYZ',
           'EdgeSE3PointXYZ']
