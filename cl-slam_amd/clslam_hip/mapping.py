"""The mapping half of the SLAM loop on the device: the reference's ``depth_to_pcl`` (slam/utils.py:25-38), ``accumulate_pcl``
(:76-82) and ``pcl_to_image`` (:41-58) without OpenCV, without the per-point Python loop and without pulling the depth and
colour planes to the host, and ``DenseMap``, a map that stays in HBM.

The three functions have the reference's names, argument order and defaults.  Device tensors are used where they are; numpy
arrays and host tensors are uploaded.  The result comes back as what went in: numpy in gives a numpy (M,6) or (rows,cols,3)
array out, which the reference's ``save_point_cloud`` / ``MeshlabInf`` and ``generate_figure`` take unchanged; a tensor in
gives a tensor on the same device out.  All results are float32.

``voxel_downsample`` reduces a cloud to one mean row per occupied grid cell (a radix sort of the cell keys on the device) and
``save_point_cloud`` is the reference's (slam/utils.py:61-73) with a trailing ``voxel_size``: the same bytes, written in seconds.

``DenseMap`` stores every frame's cloud in ITS CAMERA FRAME and poses it when it is read: after a loop-closure ``optimize()``
the whole map is re-posed from the corrected vertex poses by calling ``world_points`` / ``render`` again -- nothing is cached
across pose changes.

Differences from the reference, all on inputs it cannot handle or in representation only: ``pcl_to_image`` skips points with a
non-finite coordinate (the reference raises on ``int(nan)``); it returns float32 where the reference returns float64 zeros
filled with float32 colours (the same values); ``accumulate_pcl`` returns the float32 rounding of the reference's float64
coordinates.  The projection is OpenCV's ``projectPoints`` with zero rotation, translation and distortion restated from its
source (include/clslam_hip.h), not compared with cv2.
"""
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops


def _device_of(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    lib = _lib.get_lib()
    return torch.device('cuda', torch.cuda.current_device()) if lib.is_device else torch.device('cpu')


def _tensor(x, name: str, device: torch.device, dtype=torch.float32) -> torch.Tensor:
    """-> contiguous `dtype` on `device`; a device tensor that already is one is passed through untouched"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise _lib.ClslamError(f'{name} must be a numpy array or a tensor, got {type(x).__name__}')
    if x.dtype is not dtype:
        x = x.to(dtype)
    if x.device != device:
        x = x.to(device, non_blocking=True)
    return x.detach().contiguous()


def _like(result: torch.Tensor, given):
    """the result as what went in: numpy for numpy, else a tensor on the input's device"""
    if isinstance(given, np.ndarray):
        return result.cpu().numpy()
    return result if given.device == result.device else result.to(given.device)


def _planes(depth, image, inv_K, device, batch: Optional[int] = None, hw: Optional[Tuple[int, int]] = None):
    """-> depth (N,1,H,W), image (N,3,H,W), inv_K (N,4,4) on `device`"""
    depth, image, inv_K = _tensor(depth, 'depth', device), _tensor(image, 'image', device), _tensor(inv_K, 'inv_K', device)
    if hw is None:
        if depth.dim() < 2:
            raise _lib.ClslamError(f'depth must be (H,W), (1,H,W) or (N,1,H,W), got {tuple(depth.shape)}')
        hw = tuple(depth.shape[-2:])
    H, W = hw
    if H * W == 0 or depth.numel() % (H * W) or (batch is not None and depth.numel() != batch * H * W):
        raise _lib.ClslamError(f'depth {tuple(depth.shape)} does not hold {batch if batch is not None else "whole"} planes of {H}x{W}')
    N = depth.numel() // (H * W)
    if image.numel() != N * 3 * H * W:
        raise _lib.ClslamError(f'image {tuple(image.shape)} does not hold {N} colour planes of 3x{H}x{W}')
    if inv_K.numel() not in (16, N * 16) or tuple(inv_K.shape[-2:]) != (4, 4):
        raise _lib.ClslamError(f'inv_K must be (4,4) or ({N},4,4), got {tuple(inv_K.shape)}')
    inv_K = inv_K.reshape(-1, 4, 4)
    if inv_K.shape[0] != N:
        inv_K = inv_K.expand(N, 4, 4).contiguous()
    return depth.reshape(N, 1, H, W), image.reshape(N, 3, H, W), inv_K


def depth_to_pcl(backproject_depth, inv_camera_matrix, depth, image, batch_size: int = 1, dist_threshold: float = np.inf):
    """slam/utils.py:25-38: the (M,6) cloud [cam_x, cam_y, cam_z, r, g, b] of the pixels closer than dist_threshold, in pixel
    order.  `backproject_depth` is used for its height and width only (None: the depth plane's last two dimensions)."""
    dev = _device_of(depth, image, inv_camera_matrix)
    hw = None if backproject_depth is None else (int(backproject_depth.height), int(backproject_depth.width))
    d, im, ik = _planes(depth, image, inv_camera_matrix, dev, batch=batch_size, hw=hw)
    points, _ = ops.pcl_backproject(d, ik, im, dist_threshold)
    return _like(points, depth)


def _pose_stack(poses, device: torch.device) -> torch.Tensor:
    """a sequence of 4x4 (or one (F,4,4) array) -> (F,4,4) float64 on `device`"""
    if isinstance(poses, torch.Tensor):
        p = poses.detach().to(torch.float64).cpu().numpy()
    else:
        p = np.asarray([np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float64) for m in poses],
                       dtype=np.float64)
    p = p.reshape(-1, 4, 4) if p.size else np.zeros((0, 4, 4))
    return torch.from_numpy(np.ascontiguousarray(p)).to(device)


def accumulate_pcl(pcl_list, global_pose_list):
    """slam/utils.py:76-82: every cloud posed by its 4x4 pose (float64 arithmetic, rounded once to float32), concatenated"""
    pairs = list(zip(pcl_list, global_pose_list))
    if not pairs:
        raise _lib.ClslamError('accumulate_pcl: nothing to accumulate')          # np.concatenate of an empty list raises too
    dev = _device_of(*(c for c, _ in pairs))
    clouds = [_tensor(c, 'pcl', dev) for c, _ in pairs]
    for c in clouds:
        if c.dim() != 2 or c.shape[1] != 6:
            raise _lib.ClslamError(f'accumulate_pcl: a cloud must be (M, 6), got {tuple(c.shape)}')
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    points = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
    out = ops.pcl_transform(points, offsets, _pose_stack([p for _, p in pairs], dev))
    return _like(out, pairs[0][0])


def _camera(camera_matrix, device: torch.device) -> torch.Tensor:
    K = _tensor(camera_matrix, 'camera_matrix', device, torch.float64)
    if K.dim() != 2 or K.shape[0] < 3 or K.shape[1] < 3:
        raise _lib.ClslamError(f'camera_matrix must be at least 3x3, got {tuple(K.shape)}')
    return K[:3, :3].contiguous()


def pcl_to_image(pcl, camera_matrix, image_shape):
    """slam/utils.py:41-58: the (rows,cols,3) float32 view of the cloud from the origin -- per pixel the colour of the closest
    point (Euclidean distance; the lowest index among equal distances), 0 where nothing projects.  Points behind the camera
    project mirrored, as in the reference (DenseMap.render has min_z)."""
    dev = _device_of(pcl)
    points = _tensor(pcl, 'pcl', dev)
    return _like(ops.pcl_to_image(points, _camera(camera_matrix, dev), image_shape), pcl)


def _voxel_size(fn: str, voxel_size, min_points) -> None:
    try:
        ok = float(voxel_size) > 0.0 and np.isfinite(float(voxel_size))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise _lib.ClslamError(f'{fn}: voxel_size must be a finite number above 0, got {voxel_size!r}')
    if not isinstance(min_points, (int, np.integer)) or isinstance(min_points, bool) or min_points < 1:
        raise _lib.ClslamError(f'{fn}: min_points must be an integer of at least 1, got {min_points!r}')


def voxel_downsample(pcl, voxel_size, min_points: int = 1, return_counts: bool = False):
    """The voxel-grid filter: one (6,) row per cell of side `voxel_size` that holds at least `min_points` points of the (M,6)
    cloud -- the float64 mean of its members' coordinates and colours, rounded once to float32 -- in ascending order of
    (iz, iy, ix), i = floor(c / voxel_size).  Rows with a NaN or an infinity are dropped; a cell index beyond +-2^20 raises.
    return_counts adds the (V,) int32 number of members of every row."""
    fn = 'voxel_downsample'
    _voxel_size(fn, voxel_size, min_points)
    dev = _device_of(pcl)
    points = _tensor(pcl, 'pcl', dev)
    if points.dim() != 2 or points.shape[1] != 6:
        raise _lib.ClslamError(f'{fn}: a cloud must be (M, 6), got {tuple(points.shape)}')
    rows, counts = ops.pcl_voxel_downsample(points, voxel_size, min_points=int(min_points))
    return (_like(rows, pcl), _like(counts, pcl)) if return_counts else _like(rows, pcl)


OBJ_CHUNK = 1 << 16         # rows formatted by one % operation


def save_point_cloud(filename, pcl, global_pose_list=None, verbose: bool = True, voxel_size: Optional[float] = None) -> None:
    """slam/utils.py:61-73 with MeshlabInf.add_points / write (slam/meshlab.py:116-139, 159-206; false_color=False, no faces):
    `pcl` ((M,6) only: the 3- and 4-column clouds add_points paints grey are not taken) -- with `global_pose_list` a list of
    clouds, accumulated first -- written as "# OBJ file" and one
    "v x y z r g b" line per point with four decimals; rows with a NaN are dropped, the colours are normalised over the whole
    cloud (norm_range_01) and shifted so that their maximum is 1.  `voxel_size` thins the cloud with voxel_downsample first.
    Dropping, thinning and normalising run on the device; the rows cross to the host once, as float64, and are formatted
    OBJ_CHUNK rows at a time.  The bytes are the reference's for the same float32 cloud.  `verbose` is accepted for the
    signature's sake: writing a map takes seconds, not the minutes a progress bar is for."""
    fn = 'save_point_cloud'
    if voxel_size is not None:
        _voxel_size(fn, voxel_size, 1)
    if global_pose_list is not None:
        cloud = accumulate_pcl(pcl, global_pose_list)
    else:
        cloud = pcl
    dev = _device_of(cloud)
    points = _tensor(cloud, 'pcl', dev)
    if points.dim() == 1:
        points = points.reshape(1, -1)
    if points.dim() != 2 or points.shape[1] != 6:
        raise _lib.ClslamError(f'{fn}: a cloud must be (M, 6), got {tuple(points.shape)}')
    if voxel_size is not None:
        points, _ = ops.pcl_voxel_downsample(points, voxel_size)
    _write_obj(filename, points)


def _write_obj(filename, points: torch.Tensor) -> None:
    """(M,6) float32 on any device -> the reference's file"""
    rows = points[~torch.isnan(points).any(dim=1)].to(torch.float64)
    if rows.shape[0]:
        c = rows[:, 3:]
        lo, hi = c.min(), c.max()
        span = hi - lo
        span = torch.where(span < np.finfo(np.float64).eps, torch.ones_like(span), span)
        c = ((c - lo) / span).clamp(0.0, 1.0)
        c = c + (1.0 - c.max())
        # write() passes the coordinates through its identity global_transformation, 1 x + 0 y + 0 z + 0: -0.0 becomes 0.0, an
        # infinite coordinate stays and turns the row's other two into NaN (0 * inf)
        inf = torch.isinf(rows[:, :3])
        others = inf.sum(dim=1, keepdim=True) - inf.to(torch.int64)
        xyz = torch.where(others > 0, torch.full_like(rows[:, :3], float('nan')), rows[:, :3] + 0.0)
        rows = torch.cat([xyz, c], dim=1)
    host = rows.cpu().numpy()
    line = 'v %.4f %.4f %.4f %.4f %.4f %.4f\n'
    with open(filename, 'w', encoding='utf-8') as f:
        f.write('# OBJ file\n')
        for a in range(0, host.shape[0], OBJ_CHUNK):
            chunk = host[a:a + OBJ_CHUNK]
            f.write((line * chunk.shape[0]) % tuple(chunk.ravel().tolist()))


class DenseMap:
    """The dense coloured map on the device: one camera-frame cloud per frame in a geometrically grown buffer, host-side
    int64 segment offsets and step ids.

        dense_map.add_frame(step, outputs['depth', 0], inputs['rgb', 0, 0], inputs['inv_K', 0])     # after adapt(): no read-back
        cloud = dense_map.world_points(slam.pose_graph.get_all_poses())                               # (M,6) on the device
        view = dense_map.render(poses, poses[-1], K, (192, 640), exclude=step)                        # (rows,cols,3)
    """

    def __init__(self, device: Optional[torch.device] = None, capacity: int = 0, growth: float = 2.0) -> None:
        if growth <= 1.0:
            raise _lib.ClslamError('DenseMap: growth must be above 1')
        self.device = torch.device(device) if device is not None else _device_of()
        self.growth = float(growth)
        self.reallocations = 0
        self._buf = torch.empty(max(0, int(capacity)), 6, device=self.device)
        self._offsets: List[int] = [0]
        self._steps: List[int] = []
        self._pending = None           # (event or None, host tensor): the row count of the last frame, on its way

    # -- bookkeeping ------------------------------------------------------------------------------------------------------------
    def _settle(self) -> None:
        """take in the staged point count of the last thresholded frame (waits for its 8-byte copy only)"""
        if self._pending is None:
            return
        event, host = self._pending
        self._pending = None
        if event is not None:
            event.synchronize()
        self._offsets.append(self._offsets[-1] + int(host[0]))

    def __len__(self) -> int:
        return len(self._steps)

    @property
    def num_points(self) -> int:
        self._settle()
        return self._offsets[-1]

    @property
    def capacity(self) -> int:
        return self._buf.shape[0]

    @property
    def step_ids(self) -> List[int]:
        return list(self._steps)

    @property
    def offsets(self) -> np.ndarray:
        """(frames + 1) int64: frame k owns rows [offsets[k], offsets[k+1]) of `points`"""
        self._settle()
        return np.asarray(self._offsets, dtype=np.int64)

    @property
    def points(self) -> torch.Tensor:
        """the (M,6) camera-frame rows, a view of the buffer"""
        return self._buf[:self.num_points]

    def clear(self) -> None:
        self._pending = None
        self._offsets, self._steps = [0], []

    def _reserve(self, rows: int) -> None:
        if rows <= self._buf.shape[0]:
            return
        grown = torch.empty(max(rows, int(self._buf.shape[0] * self.growth)), 6, device=self.device)
        used = self._offsets[-1]
        if used:
            grown[:used].copy_(self._buf[:used])
        self._buf = grown
        self.reallocations += 1

    # -- filling ----------------------------------------------------------------------------------------------------------------
    def add_frame(self, step_id: int, depth, image, inv_K, dist_threshold: float = np.inf) -> None:
        """Append the cloud of ONE frame: sample 0 of depth (B,1,H,W) / image (B,3,H,W) / inv_K (B,4,4) as adapt() and the data
        loader return them (slam.py:180-182, 266 read [0] too), or a single (1,H,W) / (H,W) plane with its (3,H,W) image and
        (4,4) inv_K.  Device planes are read where they are; with an infinite threshold nothing comes back to the host, with a
        finite one the frame's point count does (8 bytes, staged through pinned memory behind an event)."""
        if step_id in self._steps:
            raise _lib.ClslamError(f'DenseMap: step {step_id} is already in the map')
        self._settle()
        pick = [x[:1] if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == rank else x
                for x, rank in ((depth, 4), (image, 4), (inv_K, 3))]
        d, im, ik = _planes(pick[0], pick[1], pick[2], self.device, batch=1)
        rows = d.shape[2] * d.shape[3]
        start = self._offsets[-1]
        self._reserve(start + rows)
        keep_all = bool(np.isinf(dist_threshold))
        _, off = ops.pcl_backproject(d, ik, im, dist_threshold, out=self._buf[start:], narrow=False)
        self._steps.append(step_id)
        if keep_all:
            self._offsets.append(start + rows)
        elif off.is_cuda:
            host = torch.empty(1, dtype=torch.int64, pin_memory=True)
            host.copy_(off[1:], non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self.device))
            self._pending = (event, host)
        else:
            self._pending = (None, off[1:])

    # -- reading ----------------------------------------------------------------------------------------------------------------
    def _frame_poses(self, poses, frames: Sequence[int]) -> np.ndarray:
        """(len(frames),4,4) float64 for the frames (indices into the map) from a {step_id: 4x4} mapping or a list aligned with
        the frames in insertion order (PoseGraphOptimization.get_all_poses() when every vertex went into the map)"""
        out = np.empty((len(frames), 4, 4), dtype=np.float64)
        is_map = isinstance(poses, Mapping)
        for i, k in enumerate(frames):
            step = self._steps[k]
            if (is_map and step not in poses) or (not is_map and k >= len(poses)):
                raise _lib.ClslamError(f'DenseMap: no pose for step {step} (frame {k} of the map)')
            m = poses[step] if is_map else poses[k]
            out[i] = np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float64).reshape(4, 4)
        return out

    def world_points(self, poses, voxel_size: Optional[float] = None, min_points: int = 1) -> torch.Tensor:
        """(M,6) device tensor: every frame's rows posed by ITS pose (world <- camera), in insertion order.  With a
        `voxel_size` the (V,6) voxel_downsample of that cloud instead -- the same bits, but the poses are applied inside the
        filter and no world copy of the map is made."""
        if voxel_size is not None:
            _voxel_size('DenseMap.world_points', voxel_size, min_points)
        frames = list(range(len(self)))
        T = torch.from_numpy(self._frame_poses(poses, frames)).to(self.device)
        if voxel_size is None:
            return ops.pcl_transform(self.points, self.offsets, T)
        return ops.pcl_voxel_downsample(self.points, voxel_size, offsets=self.offsets, poses=T, min_points=int(min_points))[0]

    def save(self, filename, poses, voxel_size: Optional[float] = None) -> None:
        """the posed map as the reference's OBJ point file (save_point_cloud), thinned to `voxel_size` if given"""
        _write_obj(filename, self.world_points(poses, voxel_size))

    def render(self, poses, view_pose, camera_matrix, image_shape, exclude=None, min_z: Optional[float] = None,
               return_dist: bool = False, return_index: bool = False):
        """The z-buffered (rows,cols,3) view of the map from `view_pose` (world <- camera): frame f is posed by
        inv(view_pose) . pose_f, composed in float64 on the host, inside the splat -- no world copy of the map is made.
        exclude: a step id or an iterable of them to leave out (the reference's 'Projected PCL (w/o current frame)' panel).
        min_z: cull points with z <= min_z in the view instead of projecting those behind the camera mirrored."""
        if exclude is None:
            skip = set()
        elif isinstance(exclude, Iterable) and not isinstance(exclude, (str, bytes)):
            skip = set(exclude)
        else:
            skip = {exclude}
        offsets = self.offsets
        frames = list(range(len(self)))
        kept = [k for k in frames if self._steps[k] not in skip]
        T = self._frame_poses(poses, kept)
        view_inv = np.linalg.inv(np.asarray(view_pose.detach().cpu() if isinstance(view_pose, torch.Tensor) else view_pose,
                                            dtype=np.float64).reshape(4, 4))
        full = np.full((len(frames), 4, 4), np.nan)       # a NaN pose gives non-finite coordinates: the splat skips the frame
        if kept:
            full[kept] = view_inv @ T
        K = _camera(camera_matrix, self.device)
        return ops.pcl_to_image(self.points, K, image_shape, offsets=offsets, poses=torch.from_numpy(full).to(self.device),
                                min_z=min_z, return_dist=return_dist, return_index=return_index)
