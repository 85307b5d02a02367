"""Depth-error metrics on the device: the reference's ``calc_depth_error`` (slam/utils.py:389-442) without OpenCV and without
pulling the depth plane to the host.

``calc_depth_error(pred_depth, gt_depth, ...)`` has the reference's signature, key names and Python-float values.  Device
tensors are used where they are (no copy); numpy arrays and host tensors are uploaded, so the driver's call at slam.py:264-270
(``outputs['depth', 0][0].cpu().numpy()``, ``online_data['depth', 0, -1][0].cpu().numpy()``) keeps working -- and works
better with the ``.cpu().numpy()`` dropped: the result is one 40-byte read-back per image instead of a 491 KB plane.

``depth_error_async`` enqueues the kernels on the CURRENT stream and stages the (N,10) result to pinned host memory behind an
event; ``.result()`` waits for that event only.  Right after a detached training ``adapt()`` the current stream is ordered
behind the step's output planes but not behind its backward and optimizer step, so a per-frame metric does not wait for them.
"""
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from . import _lib, ops

KEYS = ('abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3', 'rmse', 'rmse_log')      # utils.py:431-440


def _planes(x, name: str, device: torch.device) -> torch.Tensor:
    """-> (N,rows,cols) contiguous fp32 on `device`; a device tensor that already is one is passed through untouched"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not isinstance(x, torch.Tensor):
        raise _lib.ClslamError(f'{name} must be a numpy array or a tensor, got {type(x).__name__}')
    if x.dim() < 2:
        raise _lib.ClslamError(f'{name} must have at least two dimensions, got {tuple(x.shape)}')
    if x.dim() == 4 and x.shape[1] == 1:            # (N,1,rows,cols): the predictor's output planes
        x = x[:, 0]
    elif x.dim() != 3:
        x = x.reshape(-1, x.shape[-2], x.shape[-1]) if x.dim() == 2 else x.squeeze()
        if x.dim() == 2:
            x = x[None]
    if x.dim() != 3:
        raise _lib.ClslamError(f'{name} must be (rows, cols), (N, rows, cols) or (N, 1, rows, cols), got {tuple(x.shape)}')
    if x.device != device:
        x = x.to(device, non_blocking=True)
    if x.dtype is not torch.float32:
        x = x.float()
    return x.contiguous()


def _device_of(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    lib = _lib.get_lib()
    return torch.device('cuda', torch.cuda.current_device()) if lib.is_device else torch.device('cpu')


def as_dict(row) -> Dict[str, float]:
    """one row of the (N,10) result -> the reference's dict (Python floats)"""
    return {k: float(row[i]) for i, k in enumerate(KEYS)}


class DepthErrorHandle:
    """The (N,10) result on the device (`device_result`) and, behind `event`, in pinned host memory."""

    def __init__(self, device_result: torch.Tensor) -> None:
        self.device_result = device_result
        self.event = None
        self.stream = None
        if device_result.is_cuda:
            self.stream = torch.cuda.current_stream(device_result.device)
            self._host = torch.empty(device_result.shape, dtype=torch.float32, pin_memory=True)
            self._host.copy_(device_result, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record(self.stream)
        else:
            self._host = device_result

    def done(self) -> bool:
        return self.event is None or self.event.query()

    def rows(self) -> np.ndarray:
        """(N,10) float32 on the host: [the 8 metrics, ratio, n] per image; waits for the staging event only"""
        if self.event is not None:
            self.event.synchronize()
        return self._host.numpy()

    def result(self) -> Union[Dict[str, float], List[Dict[str, float]]]:
        """the reference's dict for one image, a list of them for a batch"""
        rows = self.rows()
        return as_dict(rows[0]) if rows.shape[0] == 1 else [as_dict(r) for r in rows]


def depth_error_async(pred, gt, median_scaling: bool = True, min_depth: Optional[float] = None, max_depth: Optional[float] = None,
                      from_disp: bool = False) -> DepthErrorHandle:
    dev = _device_of(pred, gt)
    return DepthErrorHandle(ops.depth_metrics(_planes(pred, 'pred_depth', dev), _planes(gt, 'gt_depth', dev), min_depth, max_depth,
                                              median_scaling=median_scaling, from_disp=from_disp))


def calc_depth_error(pred_depth, gt_depth, median_scaling: bool = True, min_depth: Optional[float] = None,
                     max_depth: Optional[float] = None) -> Dict[str, float]:
    """slam/utils.py:389-442 for one image"""
    h = depth_error_async(pred_depth, gt_depth, median_scaling, min_depth, max_depth)
    if h.device_result.shape[0] != 1:
        raise _lib.ClslamError(f'calc_depth_error evaluates one image, got {h.device_result.shape[0]} (use depth_error_async)')
    return h.result()
