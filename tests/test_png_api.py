"""clslam_hip.png (encode, encode_batch, save), undistort_images(encoder=...) and the binding's answer to a library built before the
PNG entry points, on tiny generated frames and model files."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_reference as ref
import robotcar_reference as rc_ref
from emu_util import BACKENDS, use_backend

H, W = 12, 20


def _write_model(models, name, lut):
    """<name>.txt + <name>_distortion_lut.bin as the dataset's SDK ships them: the table's file holds all columns, then all rows"""
    models.mkdir(parents=True, exist_ok=True)
    g = np.eye(4)
    (models / f'{name}.txt').write_text('400.5 401.25 10.5 6.75\n' + '\n'.join(' '.join(repr(float(v)) for v in row) for row in g) + '\n')
    np.stack([lut[1].ravel(), lut[0].ravel()]).astype(np.double).tofile(models / f'{name}_distortion_lut.bin')


def _sequence(tmp_path, n=6):
    lut = rc_ref.edge_lut(H, W, seed=11)
    _write_model(tmp_path / 'models', 'stereo_narrow_left', lut)
    centre = tmp_path / 'seq' / 'stereo' / 'centre'
    centre.mkdir(parents=True)
    frames = np.random.default_rng(6).integers(0, 256, (n, H, W), dtype=np.uint8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(centre / f'{1400000000 + i}.png')
    return centre, [rc_ref.load_image(f, lut, 'gbrg') for f in frames]


@pytest.mark.parametrize('backend', BACKENDS)
def test_encode_save_and_batch(backend, tmp_path):
    from clslam_hip import png
    device = use_backend(backend)
    rng = np.random.default_rng(3)
    gray = (np.add.outer(np.arange(30), 2 * np.arange(41)) % 256).astype(np.uint8)
    rgb = rng.integers(0, 40, (30, 41, 3), dtype=np.uint8)
    for image in (gray, rgb):
        data = png.encode(image)
        assert isinstance(data, bytes) and np.array_equal(np.array(Image.open(io.BytesIO(data))), image)
        assert png.encode(torch.from_numpy(image).to(device)) == data                  # a tensor on the device: the same file
        assert png.encode(torch.from_numpy(image)) == data
        ref.check_file(data, bytes(ref.filter_rows(image)[0]), 30, 41, 1 if image.ndim == 2 else 3)
        fixed = png.encode(image, filter='paeth')
        ref.check_file(fixed, bytes(ref.filter_rows(image, 4)[0]), 30, 41, 1 if image.ndim == 2 else 3)
    png.save(tmp_path / 'a.png', rgb)
    assert np.array_equal(np.array(Image.open(tmp_path / 'a.png')), rgb)
    assert (tmp_path / 'a.png').read_bytes() == png.encode(rgb)
    images = np.stack([rgb, rgb[::-1], 255 - rgb])
    batch = png.encode_batch(images)
    assert batch == [png.encode(im) for im in images] and batch == png.encode_batch(torch.from_numpy(images.copy()).to(device))
    assert png.encode_batch(np.stack([gray, gray.T.copy().T])) == [png.encode(gray)] * 2


@pytest.mark.parametrize('backend', BACKENDS)
def test_other_dtypes_and_shapes_raise(backend):
    from clslam_hip import png
    from clslam_hip._lib import ClslamError
    use_backend(backend)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 5), np.uint16), np.zeros((4, 5, 2), np.uint8), np.zeros((4, 5, 4), np.uint8),
                np.zeros((5,), np.uint8), np.zeros((0, 5), np.uint8), torch.zeros(4, 5, dtype=torch.int16)):
        with pytest.raises(ClslamError):
            png.encode(bad)
    with pytest.raises(ClslamError):
        png.encode_batch(np.zeros((4, 5), np.uint8))
    with pytest.raises(ClslamError):
        png.encode_batch(np.zeros((2, 4, 5, 3, 1), np.uint8))
    with pytest.raises(ClslamError, match='filter'):
        png.encode(np.zeros((4, 5), np.uint8), filter='zip')
    assert png.encode(np.zeros((4, 5), np.uint8)[:, ::2])[:8] == ref.SIGNATURE            # a strided view is copied, not refused


@pytest.mark.parametrize('backend', BACKENDS)
def test_undistort_images_device_encoder(backend, tmp_path, monkeypatch):
    from clslam_hip import robotcar
    use_backend(backend)
    monkeypatch.setattr(robotcar, 'FRAME_SLICE', slice(0, None))
    centre, want = _sequence(tmp_path)
    names = sorted(p.name for p in centre.glob('*.png'))
    models = str(tmp_path / 'models')
    pil, dev = tmp_path / 'pillow', tmp_path / 'device'
    dev.mkdir()
    marker = np.full((2, 2, 3), 9, dtype=np.uint8)
    Image.fromarray(marker).save(dev / names[2])
    robotcar.undistort_images(str(centre), models, data_path_out=str(pil), batch=4, workers=2)
    robotcar.undistort_images(str(centre), models, data_path_out=str(dev), batch=4, workers=2, encoder='device')
    assert sorted(p.name for p in dev.glob('*.png')) == names and len(list(centre.glob('*.png'))) == 6
    for i, name in enumerate(names):
        a, b = np.array(Image.open(pil / name)), np.array(Image.open(dev / name))
        assert np.array_equal(a, want[i])
        assert np.array_equal(b, marker if i == 2 else a)                                # an existing output is skipped
        if i != 2:
            ref.check_file((dev / name).read_bytes(), bytes(ref.filter_rows(want[i])[0]), H, W, 3)
        # the default encoder is the same Pillow call as before
        buf = io.BytesIO()
        Image.fromarray(want[i]).save(buf, format='PNG')
        assert (pil / name).read_bytes() == buf.getvalue()


@pytest.mark.parametrize('backend', BACKENDS)
def test_an_unknown_encoder_is_refused_before_anything_is_renamed(backend, tmp_path):
    from clslam_hip import robotcar
    use_backend(backend)
    centre, _ = _sequence(tmp_path, n=2)
    with pytest.raises(ValueError, match='encoder'):
        robotcar.undistort_images(str(centre), str(tmp_path / 'models'), encoder='zip')
    assert centre.exists() and not (centre.parent / 'centre_distorted').exists()


@pytest.mark.parametrize('backend', BACKENDS)
def test_rectify_on_device_returns_the_tensor(backend, tmp_path):
    from clslam_hip import robotcar
    device = use_backend(backend)
    centre, want = _sequence(tmp_path, n=1)
    m = robotcar.CameraModel(str(tmp_path / 'models'), str(centre))
    raw = np.array(Image.open(next(centre.glob('*.png'))))
    assert isinstance(m.rectify(raw), np.ndarray)
    t = m.rectify(raw, on_device=True)
    assert isinstance(t, torch.Tensor) and t.device.type == device.type and np.array_equal(t.cpu().numpy(), want[0])


class _StaleLibrary:
    """a library built before the PNG entry points: every other symbol resolves"""

    def __init__(self, missing):
        self._missing = set(missing)

    def __getattr__(self, name):
        if name.startswith('_') or name in self._missing:
            raise AttributeError(name)

        class _Fn:
            restype = argtypes = None
        fn = _Fn()
        setattr(self, name, fn)
        return fn


def test_a_stale_library_is_named_by_its_missing_entry_point():
    from clslam_hip import _lib
    _lib.bind_entry_points(_StaleLibrary([]), 'lib.so')                               # complete: binds
    for name in ('clslam_png_encode', 'clslam_png_bound', 'clslam_png_scratch', 'clslam_png_filter', 'clslam_png_deflate'):
        with pytest.raises(_lib.ClslamError, match=name) as info:
            _lib.bind_entry_points(_StaleLibrary([name]), 'lib.so')
        assert 'rebuild' in str(info.value) and not isinstance(info.value, AttributeError)
