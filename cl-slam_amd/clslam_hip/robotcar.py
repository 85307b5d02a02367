"""Oxford RobotCar raw frames on the device, behind the reference's names (datasets/robotcar.py:493-678).

RobotCar ships ``stereo/centre/<timestamp>.png`` as a one-channel Bayer mosaic seen through a distorting lens.  The reference
opens such a directory only after its offline pass (``undistort_images``: colour_demosaicing's bilinear demosaic, three
``scipy.ndimage.map_coordinates`` calls per frame over the camera model's look-up table, a PNG rewrite of the sequence on every
core) has rewritten it.  Here:

``CameraModel(models_dir, images_dir)``     the reference's attributes; the table is uploaded once, in (row, col) order
``demosaic(cfa, pattern)``                  float64 RGB of a mosaic (csrc/robotcar.hip, clslam_demosaic_bilinear)
``CameraModel.undistort(image)``            the table look-up of an (H,W,C) image (clslam_undistort_lut)
``load_image(path_or_u8, model, debayer)``  the reference's ``_load_image``; with a model, ONE fused launch
``undistort_images(...)``                   the offline pass, GPU work in batches, PNG decode / encode on a small thread pool;
                                            ``encoder='device'`` encodes on the GPU as well (clslam_hip.png)
``OnlineSampleBuilder(dataset, camera_model=model)`` (ingest.py) rectifies raw frames on their way into the ring: no offline pass.

numpy in gives numpy out, a tensor in gives a tensor (on the kernels' device) out.

What is restated and not compared: colour_demosaicing is not a dependency and was not at hand; its border is scipy.ndimage.convolve's
default, 'reflect', restated in ONE device function (robotcar.hip bayer_reflect); only the outermost pixel ring depends on it.
uint8 results are ``trunc(t) & 255``: the reference's ``astype(np.uint8)`` of a value above 255 (that ring again) is
platform-defined.  ``undistort`` of a uint8 ARRAY is defined the same way (float64 arithmetic, then that conversion), whereas
scipy handed a uint8 array rounds and saturates; the reference never does that, ``_load_image`` undistorts float64.
"""
import os
import re
from pathlib import Path

import numpy as np
import torch

from . import _lib, ops, png

BAYER_STEREO, BAYER_MONO = 'gbrg', 'rggb'                                  # robotcar.py:530-531
# robotcar.py:503: "the other photos are overexposed or taken when the car was not (yet) on the road"
FRAME_SLICE = slice(1112, -147)
_CAMERA = '(stereo|mono_(left|right|rear))'
# robotcar.py:647 + the directory's name BEFORE the offline pass renames it: a raw stereo/centre is the same camera
_SENSOR = '(left|center_distorted|centre_distorted|right|centre|center)'


def _device() -> torch.device:
    lib = _lib.get_lib()
    return torch.device('cuda', torch.cuda.current_device()) if lib.is_device else torch.device('cpu')


def _to_device(x):
    """-> (contiguous tensor on the kernels' device, was it numpy); a tensor that is already there stays where it is"""
    if isinstance(x, torch.Tensor):
        there = x.device.type == _lib.get_lib().device_type
        return (x if there else x.to(_device())).contiguous(), False
    a = np.ascontiguousarray(np.asarray(x))
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(_device()), True


def _back(t: torch.Tensor, as_numpy: bool):
    return t.cpu().numpy() if as_numpy else t


def _pattern_of(camera: str) -> str:
    return BAYER_STEREO if camera == 'stereo' else BAYER_MONO                  # robotcar.py:537-540


class CameraModel:
    """Intrinsics and undistortion table of a RobotCar camera (robotcar.py:553-678).

    camera, camera_sensor, focal_length, principal_point, G_camera_image, bilinear_lut: as in the reference.  images_dir names the
    camera by the reference's rules (:644-656); a stereo centre directory may carry its name from before or after the offline pass
    (``centre`` / ``centre_distorted``), both are stereo_narrow_left."""

    def __init__(self, models_dir, images_dir) -> None:
        self.camera = None
        self.camera_sensor = None
        self.focal_length = None
        self.principal_point = None
        self.G_camera_image = None
        self.bilinear_lut = None
        self._device_lut = {}                       # device -> (2, H*W) float64, rows (row, col)
        models_dir, images_dir = str(models_dir), str(images_dir)
        name = self._model_name(images_dir)
        with open(os.path.join(models_dir, name + '.txt'), 'r', encoding='utf-8') as f:            # :662-670
            vals = [float(x) for x in next(f).split()]
            self.focal_length = (vals[0], vals[1])
            self.principal_point = (vals[2], vals[3])
            self.G_camera_image = np.array([[float(x) for x in line.split()] for line in f])
        lut = np.fromfile(os.path.join(models_dir, name + '_distortion_lut.bin'), np.double)       # :676-678
        self.bilinear_lut = lut.reshape([2, lut.size // 2]).transpose()

    def _model_name(self, images_dir: str) -> str:
        found = re.search(_CAMERA, images_dir)
        if found is None:
            raise RuntimeError('Unknown camera model for given directory: ' + images_dir)
        self.camera = found.group(0)
        if self.camera != 'stereo':
            return self.camera
        found = re.search(_SENSOR, images_dir)
        self.camera_sensor = found.group(0) if found else None
        if self.camera_sensor == 'left':
            return 'stereo_wide_left'
        if self.camera_sensor == 'right':
            return 'stereo_wide_right'
        if self.camera_sensor in ('center_distorted', 'centre_distorted', 'centre', 'center'):
            return 'stereo_narrow_left'
        raise RuntimeError('Unknown camera model for given directory: ' + images_dir)

    @property
    def pattern(self) -> str:
        return _pattern_of(self.camera)

    def lut(self, height: int, width: int, device=None) -> torch.Tensor:
        """the (2, height, width) float64 table of (row, col) source coordinates on `device` (:631), uploaded on first use"""
        if height * width != self.bilinear_lut.shape[0]:
            raise ValueError('Incorrect image size for camera model')
        device = torch.device(device) if device is not None else _device()
        if device not in self._device_lut:
            rows_cols = np.ascontiguousarray(self.bilinear_lut[:, 1::-1].T)
            self._device_lut[device] = torch.from_numpy(rows_cols).to(device)
        return self._device_lut[device].view(2, height, width)

    def project(self, xyz, image_size):
        """Pinhole projection of a 3xn (or 4xn) cloud in the camera frame -> (uv (2,m) of the points in front of the camera and
        inside the image, their depths) (:584-615; host numpy, not a kernel)"""
        xyz = np.asarray(xyz)
        if xyz.shape[0] == 3:
            xyz = np.vstack((xyz, np.ones((1, xyz.shape[1]))))
        xyzw = np.linalg.solve(self.G_camera_image, xyz)
        xyzw = xyzw[:, xyzw[2] >= 0]
        uv = np.vstack((self.focal_length[0] * xyzw[0] / xyzw[2] + self.principal_point[0],
                        self.focal_length[1] * xyzw[1] / xyzw[2] + self.principal_point[1]))
        in_img = (uv[0] >= 0.5) & (uv[0] <= image_size[1]) & (uv[1] >= 0.5) & (uv[1] <= image_size[0])
        return uv[:, in_img], np.ravel(xyzw[2, in_img])

    def undistort(self, image):
        """(H,W,C) uint8 / float64 / float32 image, numpy or tensor -> the undistorted image of the same kind (:617-642)"""
        shape = tuple(image.shape)
        if len(shape) < 2 or shape[0] * shape[1] != self.bilinear_lut.shape[0]:
            raise ValueError('Incorrect image size for camera model')
        if len(shape) != 3:
            raise ValueError('Undistortion function only works with multi-channel images')
        t, as_numpy = _to_device(image)
        if t.dtype not in (torch.uint8, torch.float64, torch.float32):
            raise _lib.ClslamError(f'CameraModel.undistort: uint8, float64 or float32 images, got {t.dtype}')
        work = t.double() if t.dtype is torch.float32 else t
        out = ops.undistort_lut(work[None], self.lut(shape[0], shape[1], t.device))[0]
        return _back(out.to(t.dtype), as_numpy)

    def rectify(self, cfa, on_device: bool = False):
        """(H,W) or (N,H,W) uint8 raw mosaic -> (H,W,3) or (N,H,W,3) uint8 rectified RGB, one fused launch (_load_image, :522-548).
        on_device=True hands back the device tensor whatever came in (undistort_images' device encoder reads it there)."""
        shape = tuple(cfa.shape)
        if len(shape) not in (2, 3):
            raise ValueError(f'CameraModel.rectify: an (H,W) or (N,H,W) raw mosaic is expected, got {shape}')
        if shape[-2] * shape[-1] != self.bilinear_lut.shape[0]:
            raise ValueError('Incorrect image size for camera model')
        t, as_numpy = _to_device(cfa)
        out = ops.robotcar_rectify(t if t.dim() == 3 else t[None], self.lut(shape[-2], shape[-1], t.device), self.pattern)
        return _back(out if t.dim() == 3 else out[0], as_numpy and not on_device)


def demosaic(cfa, pattern):
    """(H,W) or (N,H,W) uint8 Bayer mosaic (numpy, PIL image or tensor) -> float64 RGB with a trailing axis of 3:
    colour_demosaicing.demosaicing_CFA_Bayer_bilinear (robotcar.py:544)"""
    if not isinstance(cfa, (torch.Tensor, np.ndarray)):
        cfa = np.asarray(cfa)
    if cfa.ndim not in (2, 3):
        raise ValueError(f'demosaic: an (H,W) or (N,H,W) mosaic is expected, got {tuple(cfa.shape)}')
    t, as_numpy = _to_device(cfa)
    out = ops.demosaic_bilinear(t if t.dim() == 3 else t[None], pattern)
    return _back(out if t.dim() == 3 else out[0], as_numpy)


def _u8(t: torch.Tensor) -> torch.Tensor:
    """float64 -> uint8 the way the kernels do: truncation toward zero, then the low byte"""
    return (t.to(torch.int64) & 255).to(torch.uint8)


def load_image(image_path, model=None, debayer=True):
    """The reference's ``_load_image`` (robotcar.py:522-548): a raw frame, given as a path or as the decoded uint8 array / tensor,
    demosaiced (``debayer``) and undistorted (``model``) -> uint8.  The pattern is gbrg for the stereo camera and rggb for the
    others; with no model the camera is read from the path."""
    is_path = isinstance(image_path, (str, os.PathLike))
    if model is not None:
        camera = model.camera
    elif is_path:
        camera = re.search(_CAMERA, str(image_path)).group(0)
    elif debayer:
        raise ValueError('load_image: a decoded frame needs a model to tell its Bayer pattern (or a path that names the camera)')
    else:
        camera = None
    if is_path:
        from PIL import Image
        with Image.open(image_path) as im:
            image_path = np.array(im)
    img, as_numpy = _to_device(image_path)
    if img.dtype is not torch.uint8:
        raise _lib.ClslamError(f'load_image: uint8 frames, got {img.dtype}')
    if debayer and img.dim() != 2:
        raise ValueError(f'load_image: debayer=True takes a one-channel mosaic, got {tuple(img.shape)}')
    if debayer and model is not None:
        return _back(model.rectify(img), as_numpy)
    if debayer:
        return _back(_u8(ops.demosaic_bilinear(img[None], _pattern_of(camera))[0]), as_numpy)
    if model is not None:
        return _back(model.undistort(img), as_numpy)
    return _back(img, as_numpy)


def _default_workers() -> int:
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 4


def undistort_images(data_path_in, models_path, data_path_out=None, batch: int = 8, workers=None, encoder: str = 'pillow') -> None:
    """The reference's offline pass (robotcar.py:493-517).  data_path_out=None is the reference: data_path_in is renamed to
    ``<data_path_in>_distorted`` and the rectified frames FRAME_SLICE of it are written under the old name; with data_path_out
    nothing is renamed and the frames are written there.  A frame whose output file exists is skipped.  `batch` frames go through
    one fused launch; PNG decode and encode run on `workers` threads (default: the CPUs this process may use, at most 16).
    encoder='pillow' (the default) writes the files with Pillow from a host copy of the rectified frames; encoder='device' keeps them
    on the device, where clslam_hip.png turns the batch into file bytes behind the fused launch on the same stream (literal-only
    deflate: larger files, the same pixels), and the threads only write those bytes."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    if encoder not in ('pillow', 'device'):
        raise ValueError(f"undistort_images: encoder must be 'pillow' or 'device', got {encoder!r}")
    batch = max(int(batch), 1)
    workers = _default_workers() if workers is None else max(int(workers), 1)
    if data_path_out is None:
        data_path_out = str(data_path_in)
        data_path_in = data_path_out.rstrip('/') + '_distorted'
        os.rename(data_path_out, data_path_in)
    Path(data_path_out).mkdir(parents=True, exist_ok=True)
    model = CameraModel(models_path, str(data_path_in))
    files = sorted(Path(data_path_in).glob('*.png'))[FRAME_SLICE]
    todo = [f for f in files if not (Path(data_path_out) / f.name).exists()]

    def decode(path):
        with Image.open(path) as im:
            return np.array(im)

    def encode(path, array):
        Image.fromarray(array).save(path)

    def write(path, data):
        with open(path, 'wb') as f:
            f.write(data)

    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix='clslam-robotcar-png') as pool:
        chunks = [todo[i:i + batch] for i in range(0, len(todo), batch)]
        decoding = [pool.submit(decode, f) for f in chunks[0]] if chunks else []
        encoding = []
        for ci, chunk in enumerate(chunks):
            raw = np.stack([f.result() for f in decoding])
            decoding = [pool.submit(decode, f) for f in chunks[ci + 1]] if ci + 1 < len(chunks) else []
            if encoder == 'device':
                blobs = png.encode_batch(model.rectify(raw, on_device=True))          # upload, launches, download of the files
            else:
                rgb = model.rectify(raw)                                 # upload, one launch, download
            while len(encoding) > 2 * workers:                           # the encoder is the slow stage: keep every thread fed,
                encoding.pop(0).result()                                 # and bound the rectified frames waiting for one
            if encoder == 'device':
                encoding += [pool.submit(write, Path(data_path_out) / f.name, blobs[i]) for i, f in enumerate(chunk)]
            else:
                encoding += [pool.submit(encode, Path(data_path_out) / f.name, rgb[i]) for i, f in enumerate(chunk)]
        for f in encoding:
            f.result()
