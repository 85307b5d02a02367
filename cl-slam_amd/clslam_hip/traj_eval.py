"""Trajectory and pose-error metrics on the device: the reference's ``calc_error`` and the evaluators it is built from
(slam/utils.py:129-383) without OpenCV or matplotlib and without the Python loop over segments, and the per-frame relative pose
error of slam.py:257-259 / dpp.py:505-511 without pulling the predicted pose to the host first.

``calc_error(pred_poses, gt_poses, optimize_scale=False)`` has the reference's signature and returns the reference's text.
``trajectory_metrics`` returns the same numbers as a dict.  The reference's other names (``calc_sequence_errors``,
``compute_ATE``, ``compute_RPE``, ``scale_optimization``, ``trajectory_distances``, ``rotation_error``, ...) are thin wrappers
over the same kernels with the reference's return types, so ``from slam.utils import ...`` at slam.py:13 can point here.
Lists of 4x4 arrays and numpy arrays are uploaded; tensors on the device are used where they are; fp32 is converted to fp64
(all arithmetic is double, as numpy's is in the reference).

``trajectory_metrics_async`` / ``pose_pair_error_async`` enqueue the kernels on the CURRENT stream and stage the small result
to pinned host memory behind an event; ``.result()`` waits for that event only.  Right after a detached training ``adapt()``
the current stream is ordered behind the step's outputs but not behind its backward and optimizer step, so
``pose_pair_error_async(outputs['cam_T_cam', 0, 1][:1], online_data['relative_pose', 1])`` does not wait for them.
"""
import copy
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib, ops

KEYS = ('t_err', 'r_err', 'n_segments', 'ate', 'rpe_trans', 'rpe_rot', 'scaling', 'path_length')
SEQUENCE_LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)                      # utils.py:226


def _device_of(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    lib = _lib.get_lib()
    return torch.device('cuda', torch.cuda.current_device()) if lib.is_device else torch.device('cpu')


def _poses(x, name: str, device: torch.device) -> torch.Tensor:
    """-> (n,4,4) contiguous fp64 on `device`; a device tensor that already is one is passed through untouched"""
    if isinstance(x, (list, tuple)):
        for i, p in enumerate(x):
            if tuple(np.shape(p)) != (4, 4):
                raise _lib.ClslamError(f'{name}[{i}] must be a 4x4 pose, got shape {tuple(np.shape(p))}')
        if x and isinstance(x[0], torch.Tensor):
            x = torch.stack([p.to(device, torch.float64) for p in x])
        else:
            x = np.asarray(x, dtype=np.float64).reshape(-1, 4, 4)
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())      # (torch warns about read-only arrays; it is only read)
    if not isinstance(x, torch.Tensor):
        raise _lib.ClslamError(f'{name} must be a list of 4x4 arrays, a numpy array or a tensor, got {type(x).__name__}')
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or tuple(x.shape[1:]) != (4, 4):
        raise _lib.ClslamError(f'{name} must be (4, 4) or (n, 4, 4), got {tuple(x.shape)}')
    if x.device != device:
        x = x.to(device, non_blocking=True)
    if x.dtype is not torch.float64:
        x = x.double()
    return x.contiguous()


def _pair(pred, gt) -> Tuple[torch.Tensor, torch.Tensor]:
    dev = _device_of(pred, gt)
    p, g = _poses(pred, 'pred_poses', dev), _poses(gt, 'gt_poses', dev)
    if p.shape[0] != g.shape[0]:
        raise _lib.ClslamError(f'pred_poses holds {p.shape[0]} poses, gt_poses {g.shape[0]}')
    return p, g


class _Handle:
    """A small fp64 result on the device (`device_result`) and, behind `event`, in pinned host memory."""

    def __init__(self, device_result: torch.Tensor) -> None:
        self.device_result = device_result
        self.event = None
        self.stream = None
        if device_result.is_cuda:
            self.stream = torch.cuda.current_stream(device_result.device)
            self._host = torch.empty(device_result.shape, dtype=torch.float64, pin_memory=True)
            self._host.copy_(device_result, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record(self.stream)
        else:
            self._host = device_result

    def done(self) -> bool:
        return self.event is None or self.event.query()

    def rows(self) -> np.ndarray:
        """the result on the host (float64); waits for the staging event only"""
        if self.event is not None:
            self.event.synchronize()
        return self._host.numpy()


def as_dict(row) -> Dict[str, float]:
    """the (8,) result -> {'t_err', 'r_err', 'n_segments' (int), 'ate', 'rpe_trans', 'rpe_rot', 'scaling', 'path_length'}"""
    return {k: (int(row[i]) if k == 'n_segments' else float(row[i])) for i, k in enumerate(KEYS)}


class TrajectoryHandle(_Handle):
    def result(self) -> Dict[str, float]:
        return as_dict(self.rows())


class PairErrorHandle(_Handle):
    def result(self) -> np.ndarray:
        """(B,2) float64: [translation_error (m), rotation_error (rad)] per pair"""
        return self.rows()


def trajectory_metrics_async(pred, gt, optimize_scale: bool = False) -> TrajectoryHandle:
    p, g = _pair(pred, gt)
    return TrajectoryHandle(ops.traj_metrics(p, g, optimize_scale))


def trajectory_metrics(pred, gt, optimize_scale: bool = False) -> Dict[str, float]:
    return trajectory_metrics_async(pred, gt, optimize_scale).result()


def pose_pair_error_async(pred, gt, pred_inverted: bool = False) -> PairErrorHandle:
    """rows [translation_error, rotation_error (rad)] of inv(gt_i) @ pred_i (slam.py:257-259), or of inv(gt_i) @ inv(pred_i)
    with pred_inverted (dpp.py:505-511); (B,4,4) or (4,4) on any device"""
    p, g = _pair(pred, gt)
    return PairErrorHandle(ops.pose_pair_error(p, g, a_inverted=pred_inverted))


# ---- the reference's names (slam/utils.py:129-383) ------------------------------------------------------------------------
def format_error_log(m: Dict[str, float], optimize_scale: bool = False) -> str:
    """utils.py:357-383, character for character (no newline behind the scaling factor)"""
    log = ''
    if optimize_scale:
        log += '-' * 10 + ' MEDIAN\n'
        log += f'Scaling: {m["scaling"]}'
    log += '-' * 10 + '\n'
    log += f'Trans error (%):      {m["t_err"] * 100:.4f}' + '\n'
    log += f'Rot error (deg/100m): {100 * m["r_err"] / np.pi * 180:.4f}' + '\n'
    log += f'Abs traj RMSE (m):    {m["ate"]:.4f}' + '\n'
    log += f'Rel pose error (m):   {m["rpe_trans"]:.4f}' + '\n'
    log += f'Rel pose err (deg):   {m["rpe_rot"] * 180 / np.pi:.4f}' + '\n'
    log += '-' * 10 + '\n'
    return log


def calc_error(pred_poses, gt_poses, optimize_scale: bool = False) -> str:
    return format_error_log(trajectory_metrics(pred_poses, gt_poses, optimize_scale), optimize_scale)


def _with_outputs(pred, gt, optimize_scale=False, segments=False, dist=False):
    p, g = _pair(pred, gt)
    n = p.shape[0]
    seg = torch.empty(ops.traj_segments(n), 6, dtype=torch.float64, device=p.device) if segments else None
    d = torch.empty(n, dtype=torch.float64, device=p.device) if dist else None
    out = ops.traj_metrics(p, g, optimize_scale, segments=seg, dist=d)
    return out, seg, d


def calc_sequence_errors(pred_poses, gt_poses) -> List[list]:
    """utils.py:220-250: [first_frame, rot_error / length, trans_error / length, length, speed] per segment that is long enough"""
    _, seg, _ = _with_outputs(pred_poses, gt_poses, segments=True)
    rows = seg.cpu().numpy()
    return [[int(r[0]), float(r[1]), float(r[2]), int(r[3]), float(r[4])] for r in rows if r[5] >= 0]


def compute_segment_error(seq_errs) -> Dict[int, list]:
    """utils.py:253-289 (host only: an average per length over the rows of calc_sequence_errors)"""
    by_length = {length: [] for length in SEQUENCE_LENGTHS}
    for err in seq_errs:
        by_length[err[3]].append([err[2], err[1]])
    return {length: ([float(np.mean(np.asarray(v)[:, 0])), float(np.mean(np.asarray(v)[:, 1]))] if v else [])
            for length, v in by_length.items()}


def compute_overall_err(seq_err) -> Tuple[float, float]:
    """utils.py:292-314 (host only) -> (ave_t_err, ave_r_err); (0, 0) without a segment"""
    if len(seq_err) == 0:
        return 0, 0
    t_err = r_err = 0
    for item in seq_err:
        r_err += item[1]
        t_err += item[2]
    return t_err / len(seq_err), r_err / len(seq_err)


def compute_ATE(pred_poses, gt_poses) -> float:
    return trajectory_metrics(pred_poses, gt_poses)['ate']


def compute_RPE(pred_poses, gt_poses) -> Tuple[float, float]:
    m = trajectory_metrics(pred_poses, gt_poses)
    return m['rpe_trans'], m['rpe_rot']


def scale_lse_solver(X, Y) -> float:
    """utils.py:151-161 (host only: one numpy expression)"""
    X, Y = np.asarray(X), np.asarray(Y)
    return np.sum(X * Y) / np.sum(X**2)


def scale_optimization(pred_poses, gt_poses):
    """utils.py:129-148 -> (scaled copy, scaling): an (N,2) trajectory is scaled as a whole, a list of 4x4 poses in its
    translations only (the factor comes from the kernels)"""
    if isinstance(pred_poses, np.ndarray) and pred_poses.ndim == 2 and pred_poses.shape[1] == 2:
        scaling = scale_lse_solver(pred_poses, gt_poses)
        return scaling * pred_poses, scaling
    if isinstance(pred_poses, list) and len(pred_poses) and tuple(np.shape(pred_poses[0])) == (4, 4):
        scaling = np.float64(trajectory_metrics(pred_poses, gt_poses)['scaling'])
        scaled = copy.deepcopy(pred_poses)
        for p in scaled:
            p[:3, 3] *= scaling
        return scaled, scaling
    raise _lib.ClslamError('scale_optimization takes an (N, 2) array or a list of 4x4 poses')


def trajectory_distances(poses) -> List[float]:
    """utils.py:164-172: the path length up to every pose, a list that starts at 0"""
    dev = _device_of(poses)
    p = _poses(poses, 'poses', dev)
    _, _, d = _with_outputs(p, p, dist=True)
    return d.cpu().tolist()


def last_frame_from_segment_length(dist, first_frame: int, length: float) -> int:
    """utils.py:175-188 (host only): the first i >= first_frame with dist[i] > dist[first_frame] + length, or -1"""
    d = np.asarray(dist, dtype=np.float64)
    hit = np.nonzero(d[first_frame:] > d[first_frame] + length)[0]
    return int(first_frame + hit[0]) if hit.size else -1


def _one(pose_error) -> np.ndarray:
    dev = _device_of(pose_error)
    m = _poses(pose_error, 'pose_error', dev)
    if m.shape[0] != 1:
        raise _lib.ClslamError(f'one 4x4 matrix expected, got {tuple(m.shape)}')
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None]
    return PairErrorHandle(ops.pose_pair_error(m, eye)).rows()[0]          # inv(I) @ m is m, exactly


def rotation_error(pose_error) -> float:
    """utils.py:191-203 for one 4x4 (rad)"""
    return float(_one(pose_error)[1])


def translation_error(pose_error) -> float:
    """utils.py:206-217 for one 4x4"""
    return float(_one(pose_error)[0])
