"""clslam_hip.robotcar (CameraModel, demosaic, load_image, undistort_images) and OnlineSampleBuilder(camera_model=...) against the
numpy / scipy restatement, on generated model files and tiny generated PNGs."""
import numpy as np
import pytest
import torch
from PIL import Image

import robotcar_reference as ref
from emu_util import BACKENDS, use_backend

H, W = 12, 20


def _write_model(models, name, lut):
    """<name>.txt + <name>_distortion_lut.bin as the dataset's SDK ships them: the table's file holds all columns, then all rows"""
    models.mkdir(parents=True, exist_ok=True)
    g = np.array([[0., 0., 1., 0.], [1., 0., 0., 0.], [0., 1., 0., 0.], [0., 0., 0., 1.]])
    (models / f'{name}.txt').write_text('400.5 401.25 10.5 6.75\n' + '\n'.join(' '.join(repr(float(v)) for v in row) for row in g) + '\n')
    np.stack([lut[1].ravel(), lut[0].ravel()]).astype(np.double).tofile(models / f'{name}_distortion_lut.bin')
    return g


def _raw_dir(root, n, seed=0):
    root.mkdir(parents=True, exist_ok=True)
    frames = np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(root / f'{1400000000 + i}.png')
    return frames


@pytest.fixture
def lut():
    return ref.edge_lut(H, W, seed=11)


@pytest.mark.parametrize('backend', BACKENDS)
def test_camera_model_names_and_attributes(backend, tmp_path, lut):
    from clslam_hip import robotcar
    use_backend(backend)
    models = tmp_path / 'models'
    g = _write_model(models, 'stereo_narrow_left', lut)
    _write_model(models, 'stereo_wide_left', lut)
    _write_model(models, 'mono_left', lut)
    m = robotcar.CameraModel(str(models), str(tmp_path / 'seq' / 'stereo' / 'centre_distorted'))
    assert (m.camera, m.camera_sensor) == ('stereo', 'centre_distorted')
    assert m.focal_length == (400.5, 401.25) and m.principal_point == (10.5, 6.75)
    assert np.array_equal(m.G_camera_image, g)
    assert m.bilinear_lut.shape == (H * W, 2)
    assert np.array_equal(m.bilinear_lut[:, 1::-1].T.reshape(2, H, W), lut)
    assert m.pattern == 'gbrg'
    assert np.array_equal(m.lut(H, W).cpu().numpy(), lut) and m.lut(H, W).data_ptr() == m.lut(H, W).data_ptr()
    assert robotcar.CameraModel(str(models), 'x/stereo/centre').camera_sensor == 'centre'           # the raw download's name
    left = robotcar.CameraModel(str(models), 'x/stereo/left')
    assert (left.camera, left.camera_sensor) == ('stereo', 'left')
    mono = robotcar.CameraModel(models, tmp_path / 'mono_left')
    assert (mono.camera, mono.camera_sensor, mono.pattern) == ('mono_left', None, 'rggb')
    with pytest.raises(FileNotFoundError):
        robotcar.CameraModel(str(models), 'x/stereo/right')                                           # stereo_wide_right.txt: not written
    with pytest.raises(RuntimeError, match='Unknown camera model'):
        robotcar.CameraModel(str(models), 'x/stereo/middle')
    uv, depth = m.project(np.array([[5.0, 5.0], [0.1, -0.01], [0.05, -0.01]]), (H, W))                  # x forward, y right, z down
    assert uv.shape == (2, 2) and depth.tolist() == [5.0, 5.0]
    assert np.allclose(uv[:, 0], [400.5 * 0.1 / 5 + 10.5, 401.25 * 0.05 / 5 + 6.75])


@pytest.mark.parametrize('backend', BACKENDS)
def test_undistort_and_demosaic_keep_the_callers_kind(backend, tmp_path, lut):
    from clslam_hip import robotcar
    device = use_backend(backend)
    _write_model(tmp_path, 'stereo_narrow_left', lut)
    m = robotcar.CameraModel(tmp_path, 'stereo/centre_distorted')
    rng = np.random.default_rng(2)
    cfa = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rgb = ref.demosaic(cfa, 'gbrg')
    got = robotcar.demosaic(cfa, 'gbrg')
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, rgb)
    assert np.array_equal(robotcar.demosaic(Image.fromarray(cfa), 'GBRG'), rgb)
    got = robotcar.demosaic(torch.from_numpy(cfa).to(device), 'gbrg')
    assert isinstance(got, torch.Tensor) and got.device.type == device.type and np.array_equal(got.cpu().numpy(), rgb)
    want = ref.undistort_f64(rgb, lut)
    got = m.undistort(rgb)
    assert isinstance(got, np.ndarray) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    got = m.undistort(torch.from_numpy(rgb).to(device))
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), want)
    u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(m.undistort(u8), ref.undistort(u8, lut))
    f32 = rgb.astype(np.float32)
    got = m.undistort(f32)
    assert got.dtype == np.float32 and np.array_equal(got, ref.undistort_f64(f32, lut).astype(np.float32))
    with pytest.raises(ValueError, match='Incorrect image size'):
        m.undistort(np.zeros((H, W + 1, 3)))
    with pytest.raises(ValueError, match='multi-channel'):
        m.undistort(np.zeros((H, W)))
    with pytest.raises(ValueError, match='pattern'):
        robotcar.demosaic(cfa, 'rgb')


@pytest.mark.parametrize('backend', BACKENDS)
def test_load_image(backend, tmp_path, lut):
    from clslam_hip import robotcar
    device = use_backend(backend)
    _write_model(tmp_path / 'models', 'stereo_narrow_left', lut)
    frames = _raw_dir(tmp_path / 'stereo' / 'centre_distorted', 1, seed=4)
    mono = _raw_dir(tmp_path / 'mono_rear', 1, seed=5)
    path = str(next((tmp_path / 'stereo' / 'centre_distorted').glob('*.png')))
    m = robotcar.CameraModel(str(tmp_path / 'models'), str(tmp_path / 'stereo' / 'centre_distorted'))
    want = ref.load_image(frames[0], lut, 'gbrg')
    got = robotcar.load_image(path, m)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want)
    assert np.array_equal(robotcar.load_image(frames[0], m), want)
    got = robotcar.load_image(torch.from_numpy(frames[0]).to(device), m)
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(robotcar.load_image(path), ref.to_u8(ref.demosaic(frames[0], 'gbrg')))                 # no model: by the path
    mono_path = str(next((tmp_path / 'mono_rear').glob('*.png')))
    assert np.array_equal(robotcar.load_image(mono_path), ref.to_u8(ref.demosaic(mono[0], 'rggb')))
    assert np.array_equal(robotcar.load_image(path, debayer=False), frames[0])
    with pytest.raises(ValueError, match='multi-channel'):
        robotcar.load_image(path, m, debayer=False)
    with pytest.raises(ValueError, match='needs a model'):
        robotcar.load_image(frames[0])


def _sequence(tmp_path, lut, n=6):
    _write_model(tmp_path / 'models', 'stereo_narrow_left', lut)
    centre = tmp_path / 'seq' / 'stereo' / 'centre'
    frames = _raw_dir(centre, n, seed=6)
    return centre, frames, [ref.load_image(f, lut, 'gbrg') for f in frames]


@pytest.mark.parametrize('backend', BACKENDS)
def test_undistort_images_reference_mode(backend, tmp_path, lut, monkeypatch):
    from clslam_hip import robotcar
    use_backend(backend)
    monkeypatch.setattr(robotcar, 'FRAME_SLICE', slice(1, -1))
    centre, frames, want = _sequence(tmp_path, lut)
    names = sorted(p.name for p in centre.glob('*.png'))
    robotcar.undistort_images(str(centre), str(tmp_path / 'models'), batch=3, workers=2)
    distorted = centre.parent / 'centre_distorted'
    assert sorted(p.name for p in distorted.glob('*.png')) == names                                  # renamed, untouched
    assert np.array_equal(np.array(Image.open(distorted / names[0])), frames[0])
    assert sorted(p.name for p in centre.glob('*.png')) == names[1:-1]                                # the slice
    for i in range(1, 5):
        assert np.array_equal(np.array(Image.open(centre / names[i])), want[i])


@pytest.mark.parametrize('backend', BACKENDS)
def test_undistort_images_into_another_directory_skips_what_exists(backend, tmp_path, lut, monkeypatch):
    from clslam_hip import robotcar
    use_backend(backend)
    monkeypatch.setattr(robotcar, 'FRAME_SLICE', slice(0, None))
    centre, frames, want = _sequence(tmp_path, lut)
    names = sorted(p.name for p in centre.glob('*.png'))
    out = tmp_path / 'rectified'
    out.mkdir()
    marker = np.full((2, 2, 3), 9, dtype=np.uint8)
    Image.fromarray(marker).save(out / names[2])
    robotcar.undistort_images(str(centre), str(tmp_path / 'models'), data_path_out=str(out), batch=4, workers=1)
    assert not (centre.parent / 'centre_distorted').exists() and len(list(centre.glob('*.png'))) == 6  # nothing renamed
    assert sorted(p.name for p in out.glob('*.png')) == names
    for i, name in enumerate(names):
        assert np.array_equal(np.array(Image.open(out / name)), marker if i == 2 else want[i])


def test_the_reference_slice_is_the_default():
    from clslam_hip import robotcar
    assert robotcar.FRAME_SLICE == slice(1112, -147)


class _RawDataset:
    """what OnlineSampleBuilder reads of a datasets.Robotcar object: file names, sizes, the camera matrix, distances"""

    def __init__(self, files, height=8, width=16):
        self.files, self.height, self.width = list(files), height, width
        self.frame_ids, self.scales = [0, -1, 1], (0, 1)
        self.camera_matrix = np.array([[0.77, 0, 0.5, 0], [0, 1.03, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        self.relative_distances = [0.5] * len(self.files)

    def __len__(self):
        return len(self.files) - 2

    def _scale_camera_matrix(self, camera_matrix, scale):
        scaled = camera_matrix.copy()
        scaled[0, :] *= self.width // (2**scale)
        scaled[1, :] *= self.height // (2**scale)
        return scaled, np.linalg.pinv(scaled)

    def _pre_getitem(self, index):
        return self.files, [], index + 1, False, False


@pytest.mark.parametrize('backend', BACKENDS)
def test_online_builder_rectifies_raw_frames_into_the_ring(backend, tmp_path, lut):
    from clslam_hip import ingest, robotcar
    device = use_backend(backend)
    centre, frames, want = _sequence(tmp_path, lut, n=4)
    raw_files = sorted(centre.glob('*.png'))
    rgb_dir = tmp_path / 'rectified'
    rgb_dir.mkdir()
    rgb_files = []
    for f, image in zip(raw_files, want):                              # what the offline pass would have written
        Image.fromarray(image).save(rgb_dir / f.name)
        rgb_files.append(rgb_dir / f.name)
    model = robotcar.CameraModel(tmp_path / 'models', centre)
    raw = ingest.OnlineSampleBuilder(_RawDataset(raw_files), device=device, camera_model=model)
    plain = ingest.OnlineSampleBuilder(_RawDataset(rgb_files), device=device)
    assert plain.camera_model is None
    try:
        for index in range(2):
            a, b = raw.sample(index), plain.sample(index)
            assert list(a) == list(b)
            for key in a:
                if isinstance(key, tuple) and key[0] in ('rgb', 'rgb_aug'):
                    assert torch.equal(a[key].cpu(), b[key].cpu()), key
        for f_raw, f_rgb in zip(raw_files[:3], rgb_files[:3]):
            for scale in (0, 1):
                assert torch.equal(raw.ring.level(str(f_raw), scale).cpu(), plain.ring.level(str(f_rgb), scale).cpu())
        with pytest.raises(ValueError, match='no one-channel'):
            ingest.OnlineSampleBuilder(_RawDataset(rgb_files), device=device, camera_model=model).sample(0)
    finally:
        raw.close()
        plain.close()
