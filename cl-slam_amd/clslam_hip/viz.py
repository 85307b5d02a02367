"""Frame panels formed on the device (csrc/viz.hip, include/clslam_hip.h "Frame panels"): what slam/utils.py:85-121
``generate_figure`` and dpp.py:1197-1244 ``save_prediction`` draw with matplotlib, as uint8 RGB pixels and PNG files.

``depth_range(depth, q=95.0) -> (vmin, vmax)``          the smallest finite value and the q-th percentile of the finite values
``colorize(depth, cmap='magma_r', vmin=None, vmax=None, q=95.0)``     uint8 (…,H,W,3); None takes the plane's own range
``trajectory_image(gt_xz, pred_xz, shape, xlim, ylim)``               the x/z trajectory as 1-pixel lines on white, uint8 (H,W,3)
``frame_panel(image, depth, image_pcl=None, gt_xz=None, pred_xz=None, ...) -> (panel, vmax)``
                                                        the rows that were given, top to bottom in generate_figure's order
``generate_figure(batch_i, image, depth, image_pcl, gt_xz, pred_xz, save_figure=True, out_dir=...)``
                                                        the reference's call: writes {batch_i:05}.png through clslam_hip.png
``PanelWriter(out_dir, workers=2)``                     the same per frame without waiting: submit() enqueues the panel and its
                                                        PNG on the caller's stream, a pool thread writes the file

numpy in gives numpy out; a tensor in gives a tensor on the same device out (a CPU tensor is computed on the GPU and brought back).  Nothing between the caller's tensors and the PNG
bytes is read back; generate_figure's one synchronising read is the file's length.

Divergences from the reference's figure: only finite values enter the range (np.percentile answers NaN); the
percentile is interpolated in float64 and rounded once (numpy's float32 path differs in the last bits); there are no titles,
axes or legend -- the title's number is the returned vmax; lines are one pixel wide and not anti-aliased; a row is the depth
plane's H x W, image floats become bytes by trunc(clamp(x, 0, 1) * 255 + 0.5).
"""
import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import _lib, ops, png

XLIM, YLIM = (-400, 15), (-60, 160)                                   # utils.py:115-116
_EVENT_DEADLINE_S = 60.0


def _device(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device('cuda', torch.cuda.current_device()) if _lib.get_lib().is_device else torch.device('cpu')


def _home(*xs):
    """where the result goes: None (numpy) when no input is a tensor, else the device of the first tensor among the inputs -- a
    CPU tensor given to the device library is computed on the GPU and its result brought back"""
    for x in xs:
        if isinstance(x, torch.Tensor):
            return x.device
    return None


def _tensor(x, name: str, device: torch.device, dtype=None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = np.ascontiguousarray(x) if dtype is None else np.ascontiguousarray(x, dtype=dtype)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())
    if dtype is not None:
        want = torch.from_numpy(np.empty(0, dtype)).dtype
        if x.dtype is not want:
            x = x.to(want)
    if x.device != device:
        x = x.to(device, non_blocking=True)
    return x.contiguous()


def _planes(depth, device: torch.device):
    """-> ((N,H,W) contiguous fp32 on `device`, the caller's leading shape)"""
    t = _tensor(depth, 'depth', device, None if isinstance(depth, torch.Tensor) else np.float32)
    if t.dtype is not torch.float32:
        t = t.float()
    if t.dim() < 2 or t.dim() > 4 or (t.dim() == 4 and t.shape[1] != 1) or t.numel() == 0:
        raise _lib.ClslamError(f'depth must be a non-empty (H,W), (N,H,W) or (N,1,H,W) plane, got {tuple(t.shape)}')
    return t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous(), tuple(t.shape[:-2])


def _out(t: torch.Tensor, home):
    return t.cpu().numpy() if home is None else t.to(home)


def depth_range(depth, q: float = 95.0):
    """(H,W) -> scalars, (N,H,W) / (N,1,H,W) -> (N,): vmin = the smallest finite value (what imshow takes without vmin), vmax = the
    q-th percentile of the finite values (utils.py:100).  A plane without a finite value gives NaN for both."""
    planes, lead = _planes(depth, _device(depth))
    rng, _ = ops.viz_range(planes, q)
    vmin, vmax = (rng[:, 0], rng[:, 1]) if lead else (rng[0, 0], rng[0, 1])
    return _out(vmin, _home(depth)), _out(vmax, _home(depth))


def _range(planes: torch.Tensor, vmin, vmax, q: float) -> torch.Tensor:
    """(N,2) fp32 on the device: the planes' own range, a column replaced by what the caller passes (a number or one per plane)"""
    N = planes.shape[0]
    if vmin is None or vmax is None:
        rng, _ = ops.viz_range(planes, q)
    else:
        rng = torch.empty((N, 2), dtype=torch.float32, device=planes.device)
    for col, v in ((0, vmin), (1, vmax)):
        if v is not None:
            v = v.to(planes.device, torch.float32) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, np.float32)).to(planes.device)
            rng[:, col] = v.reshape(-1).expand(N) if v.numel() == 1 else v.reshape(N)
    return rng


def colorize(depth, cmap: str = 'magma_r', vmin=None, vmax=None, q: float = 95.0):
    """depth (…,H,W) -> uint8 (…,H,W,3) through 'magma_r' or 'magma' with matplotlib's arithmetic (dpp.py:1225 / utils.py:101);
    vmin / vmax None: depth_range of every plane"""
    planes, lead = _planes(depth, _device(depth, vmin, vmax))
    N, H, W = planes.shape
    out = ops.viz_compose([ops.viz_cmap_row(planes, _range(planes, vmin, vmax, q), cmap)], N, H, W)
    return _out(out.reshape(*lead, H, W, 3), _home(depth))


def _line(xz, name: str, device: torch.device):
    if xz is None:
        return None
    t = _tensor(xz, name, device, None if isinstance(xz, torch.Tensor) else np.float64)
    if t.dtype is not torch.float64:
        t = t.double()
    if t.numel() == 0:
        return None
    if t.dim() != 2 or t.shape[1] != 2:
        raise _lib.ClslamError(f'{name} must be an (N,2) array of (x, z) positions, got {tuple(t.shape)}')
    return t.contiguous()


def trajectory_image(gt_xz, pred_xz, shape, xlim=XLIM, ylim=YLIM):
    """uint8 (H,W,3): white, gt_xz in matplotlib's C0, pred_xz over it in C1, 1-pixel lines inside xlim x ylim (utils.py:113-116)"""
    dev = _device(gt_xz, pred_xz)
    H, W = int(shape[0]), int(shape[1])
    out = ops.viz_compose([ops.viz_traj_row(_line(gt_xz, 'gt_xz', dev), _line(pred_xz, 'pred_xz', dev), xlim, ylim)], 1, H, W)
    return _out(out[0], _home(gt_xz, pred_xz))


def _image_row(image, name: str, H: int, W: int, device: torch.device):
    """a (3,H,W) fp32 network input or an (H,W,3) fp32 / fp64 / uint8 image, with or without a leading 1"""
    t = _tensor(image, name, device)
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if tuple(t.shape) == (3, H, W) and t.dtype is torch.float32:
        return ops.viz_image_row(t[None], chw=True)
    if tuple(t.shape) == (H, W, 3) and t.dtype in (torch.float32, torch.float64, torch.uint8):
        return ops.viz_image_row(t[None])
    raise _lib.ClslamError(f'{name} must be (3,{H},{W}) float32 or ({H},{W},3) float32 / float64 / uint8 like the depth plane, got '
                           f'{tuple(t.shape)} {t.dtype}')


def _panel(image, depth, image_pcl, gt_xz, pred_xz, cmap, q, xlim, ylim):
    """-> (panel (rows*H, W, 3) uint8, range (1,2)) on the device"""
    dev = _device(image, depth, image_pcl, gt_xz, pred_xz)
    planes, _ = _planes(depth, dev)
    if planes.shape[0] != 1:
        raise _lib.ClslamError(f'a panel shows one depth plane, got {planes.shape[0]}')
    _, H, W = planes.shape
    rng, _ = ops.viz_range(planes, q)
    rows = [_image_row(image, 'image', H, W, dev), ops.viz_cmap_row(planes, rng, cmap)]
    if image_pcl is not None:
        rows.append(_image_row(image_pcl, 'image_pcl', H, W, dev))
    if gt_xz is not None or pred_xz is not None:
        rows.append(ops.viz_traj_row(_line(gt_xz, 'gt_xz', dev), _line(pred_xz, 'pred_xz', dev), xlim, ylim))
    return ops.viz_compose(rows, 1, H, W)[0], rng


def frame_panel(image, depth, image_pcl=None, gt_xz=None, pred_xz=None, cmap: str = 'magma_r', q: float = 95.0, xlim=XLIM, ylim=YLIM):
    """-> (panel, vmax): the rows that were given stacked top to bottom in generate_figure's order -- the frame, the depth plane
    through `cmap` up to its q-th percentile, the projected map, the trajectory -- each H x W of the depth plane, uint8
    (rows*H, W, 3).  One range computation and ONE composing launch.  There is no text: the title's number is vmax."""
    panel, rng = _panel(image, depth, image_pcl, gt_xz, pred_xz, cmap, q, xlim, ylim)
    home = _home(image, depth, image_pcl, gt_xz, pred_xz)
    return _out(panel, home), _out(rng[0, 1], home)


def generate_figure(batch_i, image, depth, image_pcl, gt_xz, pred_xz, save_figure: bool = True, out_dir='./figures/sequence_08'):
    """slam/utils.py:85-121 with one trailing keyword: writes out_dir/{batch_i:05}.png (the directory is created); with
    save_figure=False the panel is returned instead of a window being opened."""
    panel, _ = _panel(image, depth, image_pcl, gt_xz, pred_xz, 'magma_r', 95.0, XLIM, YLIM)
    if not save_figure:
        return _out(panel, _home(image, depth, image_pcl, gt_xz, pred_xz))
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    png.save(out_dir / f'{batch_i:05}.png', panel)
    return None


def _wait(event, deadline_s: float, what: str) -> None:
    """wait for a device event, with a deadline"""
    if event is None:
        return
    end = time.monotonic() + deadline_s
    while not event.query():
        if time.monotonic() > end:
            raise _lib.ClslamError(f'{what}: the device did not finish within {deadline_s:.0f} s')
        time.sleep(0.0002)


class PanelHandle:
    """One submitted panel: `.result()` waits (with a deadline) until its file is written and returns the path."""

    def __init__(self, future, path: Path) -> None:
        self._future, self.path = future, path

    def done(self) -> bool:
        return self._future.done()

    def result(self, timeout: float = 2 * _EVENT_DEADLINE_S) -> Path:
        self._future.result(timeout=timeout)
        return self.path


class PanelWriter:
    """generate_figure for every frame, beside the training step.  submit() enqueues the panel and its PNG on the caller's
    stream, stages the file buffer and its length to pinned host memory behind an event and returns; a pool thread waits for
    that event only and writes the file.  The caller's tensors may be overwritten (on the same stream) as soon as submit()
    returns, and nothing waits for work enqueued later, such as a detached training step's backward and Adam.

    At most `in_flight` frames are pending: the pinned staging buffers are a ring of that many slots, reused, and submit()
    waits (with the deadline) for the file that last used its slot -- the back-pressure of a disk slower than the driver.  The
    length is not known on the host when the copy is enqueued, so a slot holds and receives the PNG's worst-case size.  Handles
    of written files are dropped; the error of a failed one is kept and raised by close()."""

    def __init__(self, out_dir, workers: int = 2, deadline_s: float = _EVENT_DEADLINE_S, in_flight: int = 4) -> None:
        self.out_dir = Path(out_dir)
        self.out_dir.mkdir(parents=True, exist_ok=True)
        self.deadline_s = float(deadline_s)
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix='clslam-panel')
        self._slots = [{'host': None, 'length': None, 'handle': None} for _ in range(max(1, int(in_flight)))]
        self._next = 0
        self._failed = []

    def _retire(self, slot, wait: bool) -> None:
        """forget the slot's handle once its file is written (waiting for it first if asked to); keep it if it failed"""
        h = slot['handle']
        if h is None or not (wait or h.done()):
            return
        try:
            h.result(timeout=2 * self.deadline_s)
        except Exception:      # noqa: BLE001 -- raised again by close()
            self._failed.append(h)
        slot['handle'] = None

    def pending(self) -> int:
        """frames submitted whose file is not written yet"""
        for slot in self._slots:
            self._retire(slot, wait=False)
        return sum(slot['handle'] is not None for slot in self._slots)

    def submit(self, batch_i, image, depth, image_pcl=None, gt_xz=None, pred_xz=None) -> PanelHandle:
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        self._retire(slot, wait=True)                                          # its buffers are free again
        panel, _ = _panel(image, depth, image_pcl, gt_xz, pred_xz, 'magma_r', 95.0, XLIM, YLIM)
        files, lengths = ops.png_encode(panel[None])
        event = None
        if files.is_cuda:
            if slot['host'] is None or slot['host'].shape != files.shape:
                slot['host'] = torch.empty(files.shape, dtype=torch.uint8, pin_memory=True)
                slot['length'] = torch.empty(lengths.shape, dtype=torch.int32, pin_memory=True)
            host, host_len = slot['host'], slot['length']
            host.copy_(files, non_blocking=True)
            host_len.copy_(lengths, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(files.device))
        else:
            host, host_len = files, lengths
        path = self.out_dir / f'{batch_i:05}.png'

        def write():
            _wait(event, self.deadline_s, f'PanelWriter({path.name})')
            tmp = path.with_suffix('.png.part')
            with open(tmp, 'wb') as f:
                f.write(host[0, :int(host_len[0])].numpy().tobytes())
            os.replace(tmp, path)

        slot['handle'] = PanelHandle(self._pool.submit(write), path)
        return slot['handle']

    def close(self) -> None:
        """wait (with the deadline per file) until every submitted file is written; raises what a writer raised"""
        try:
            for slot in self._slots:
                self._retire(slot, wait=True)
        finally:
            self._pool.shutdown(wait=True)
        failed, self._failed = self._failed, []
        if failed:
            failed[0].result(timeout=0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
