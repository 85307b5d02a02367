"""mapping.voxel_downsample, DenseMap.world_points(voxel_size=...), mapping.save_point_cloud and DenseMap.save, on the CPU emulator
and on gfx950.  The files are compared byte for byte with the restated writer of tests/voxel_reference.py (the reference's
slam/meshlab.py imports cv2, which is not installed where this project is developed: no fixture written by the reference itself).
"""
import numpy as np
import pytest
import torch

import mapping_reference as R
import voxel_reference as V
from clslam_hip import mapping, ops
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

H, W, F = 24, 40, 3


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cloud(m=400, seed=2):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-2, 2, (m, 3)), rng.random((m, 3))], axis=1).astype(np.float32)
    pts[1, :3] = pts[0, :3]                                                      # two in one cell, whatever the size
    return pts


def _filled(dev, seed=9):
    s = R.scene(H, W, F, seed=seed)
    m = mapping.DenseMap()
    for f in range(F):
        m.add_frame(10 * f, torch.from_numpy(s['depth'][f:f + 1]).to(dev), torch.from_numpy(s['image'][f:f + 1]).to(dev),
                    torch.from_numpy(s['inv_K'][f:f + 1]).to(dev))
    return m, {10 * f: s['poses'][f] for f in range(F)}


@pytest.mark.parametrize('backend', BACKENDS)
def test_voxel_downsample_forms_and_errors(backend):
    dev = use_backend(backend)
    pts = _cloud()
    ref = V.voxel(pts, 0.5)
    assert (ref['counts'] >= 2).any() and (ref['counts'] == 1).any()
    out = mapping.voxel_downsample(pts, 0.5)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (len(ref['counts']), 6)
    assert (np.abs(out - ref['mean']) <= V.value_bound(ref)).all()
    rows, counts = mapping.voxel_downsample(pts, 0.5, return_counts=True)
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int32 and np.array_equal(counts, ref['counts'])
    assert np.array_equal(_bits(rows), _bits(out))
    for given in (torch.from_numpy(pts), torch.from_numpy(pts).to(dev)):
        rows, counts = mapping.voxel_downsample(given, 0.5, return_counts=True)
        assert isinstance(rows, torch.Tensor) and rows.device == given.device and counts.device == given.device
        assert np.array_equal(_bits(rows), _bits(out)) and np.array_equal(counts.cpu().numpy(), ref['counts'])
    two = mapping.voxel_downsample(pts, 0.5, min_points=2)
    assert np.array_equal(_bits(two), _bits(out[ref['counts'] >= 2]))
    for bad in (lambda: mapping.voxel_downsample(pts, 0.0), lambda: mapping.voxel_downsample(pts, -0.5),
                lambda: mapping.voxel_downsample(pts, float('nan')), lambda: mapping.voxel_downsample(pts, float('inf')),
                lambda: mapping.voxel_downsample(pts, None), lambda: mapping.voxel_downsample(pts, 0.5, min_points=0),
                lambda: mapping.voxel_downsample(pts, 0.5, min_points=1.5), lambda: mapping.voxel_downsample(pts[:, :5], 0.5),
                lambda: mapping.voxel_downsample(pts.reshape(-1), 0.5), lambda: mapping.voxel_downsample(pts * 1e9, 0.5),
                lambda: mapping.voxel_downsample('cloud', 0.5)):
        with pytest.raises(ClslamError):
            bad()
    assert mapping.voxel_downsample(pts[:0], 0.5).shape == (0, 6)


@pytest.mark.parametrize('backend', BACKENDS)
def test_world_points_with_and_without_a_voxel_size(backend):
    dev = use_backend(backend)
    m, poses = _filled(dev)
    T = torch.from_numpy(np.stack([poses[k] for k in m.step_ids])).to(dev)
    world = m.world_points(poses)
    assert np.array_equal(_bits(world), _bits(ops.pcl_transform(m.points, m.offsets, T)))       # as before, bitwise
    assert np.array_equal(_bits(m.world_points(poses, voxel_size=None, min_points=1)), _bits(world))
    for size, least in ((0.5, 1), (2.0, 2)):
        thin = m.world_points(poses, size, least)
        assert thin.device.type == dev.type and 0 < thin.shape[0] < world.shape[0]
        assert np.array_equal(_bits(thin), _bits(mapping.voxel_downsample(world, size, least)))
    # other poses, asked again: the new result, nothing kept from the last call
    moved = {k: R.frame_pose(3) @ P for k, P in poses.items()}
    again = m.world_points(moved, 0.5)
    want = mapping.voxel_downsample(m.world_points(moved), 0.5)
    assert np.array_equal(_bits(again), _bits(want)) and not np.array_equal(_bits(again), _bits(m.world_points(poses, 0.5)))
    for bad in (lambda: m.world_points(poses, 0.0), lambda: m.world_points(poses, float('nan')),
                lambda: m.world_points(poses, 0.5, min_points=0)):
        with pytest.raises(ClslamError):
            bad()


def _written(tmp_path, name, *args, **kw):
    path = tmp_path / name
    mapping.save_point_cloud(str(path), *args, **kw)
    return path.read_bytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_save_point_cloud_bytes(backend, tmp_path):
    dev = use_backend(backend)
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-30, 30, (50, 3)), 0.1 + 0.7 * rng.random((50, 3))], axis=1).astype(np.float32)
    pts[1, :3] = pts[0, :3] + 0.01
    pts[7, 4] = np.nan                                                           # a NaN row is left out, and out of the min / max
    pts[9, 0] = np.nan
    pts[11, :3] = [-0.00001, -0.0, 12345.67891]                                  # "-0.0000", and the sign of an exact zero
    assert np.nanmax(pts[:, 3:]) < 0.85                                          # the shift by 1 - max is visible
    want = V.obj_text(pts).encode()
    assert want.count(b'\n') == 49 and b' 1.0000' in want and b'v -0.0000 0.0000 12345.6787' in want
    for given in (pts, torch.from_numpy(pts), torch.from_numpy(pts).to(dev)):
        assert _written(tmp_path, 'plain.obj', given) == want
    assert _written(tmp_path, 'quiet.obj', pts, verbose=False) == want
    # a list of clouds with their poses: accumulated (float64, rounded once to float32), then written
    s = R.scene(H, W, F, seed=1)
    clouds = [pts[:20], pts[20:35], pts[35:]]
    world = mapping.accumulate_pcl(clouds, s['poses'])
    assert _written(tmp_path, 'posed.obj', clouds, s['poses']) == V.obj_text(world).encode()
    assert _written(tmp_path, 'posed.obj', clouds, global_pose_list=list(s['poses'])) == V.obj_text(world).encode()
    # thinned: the writer's text of the filter's rows
    for size in (0.5, 25.0):
        thin = mapping.voxel_downsample(world[~np.isnan(world).any(axis=1)], size)
        assert len(thin) < 48 if size == 25.0 else len(thin) == 47
        assert _written(tmp_path, 'thin.obj', clouds, s['poses'], voxel_size=size) == V.obj_text(thin).encode()
    assert _written(tmp_path, 'thin.obj', pts, voxel_size=25.0) == V.obj_text(mapping.voxel_downsample(pts, 25.0)).encode()
    # one colour everywhere: the span is below eps and becomes 1, every colour ends at 1
    flat = pts[:10].copy()
    flat[:, 3:] = 0.3
    got = _written(tmp_path, 'flat.obj', flat)
    assert got == V.obj_text(flat).encode() and got.count(b' 1.0000 1.0000 1.0000\n') == 9
    # infinite coordinates pass through the writer's identity transformation: the infinite one stays, 0 * inf makes the row's
    # other two NaN; two infinite ones leave three NaN
    odd = pts[:12].copy()
    odd[2, 0], odd[3, 1], odd[4, 2], odd[5, :2] = np.inf, -np.inf, np.inf, [np.inf, -np.inf]
    want_odd = V.obj_text(odd).encode()
    assert b'v inf nan nan ' in want_odd and b'v nan -inf nan ' in want_odd and b'v nan nan inf ' in want_odd
    assert b'v nan nan nan ' in want_odd and want_odd.count(b'\n') == 11
    for given in (odd, torch.from_numpy(odd).to(dev)):
        assert _written(tmp_path, 'odd.obj', given) == want_odd
    for value in (np.inf, -np.inf):                                              # an infinite colour: the reference's arithmetic
        hot = odd.copy()
        hot[6, 4] = value
        with np.errstate(all='ignore'):
            want_hot = V.obj_text(hot).encode()
        assert b'nan' in want_hot.split(b'\n')[1] and _written(tmp_path, 'hot.obj', hot) == want_hot
    # a single row given as a vector, an empty cloud, and more rows than one formatting chunk
    assert _written(tmp_path, 'one.obj', pts[0]) == V.obj_text(pts[0]).encode()
    assert _written(tmp_path, 'none.obj', pts[:0]) == b'# OBJ file\n'
    chunk, mapping.OBJ_CHUNK = mapping.OBJ_CHUNK, 16
    try:
        assert _written(tmp_path, 'chunks.obj', pts) == want
    finally:
        mapping.OBJ_CHUNK = chunk
    for bad in (lambda: mapping.save_point_cloud(str(tmp_path / 'x.obj'), pts[:, :5]),
                lambda: mapping.save_point_cloud(str(tmp_path / 'x.obj'), pts, voxel_size=0.0),
                lambda: mapping.save_point_cloud(str(tmp_path / 'x.obj'), pts, voxel_size=float('nan'))):
        with pytest.raises(ClslamError):
            bad()


@pytest.mark.parametrize('backend', BACKENDS)
def test_dense_map_save(backend, tmp_path):
    dev = use_backend(backend)
    m, poses = _filled(dev)
    path = tmp_path / 'map.obj'
    m.save(str(path), poses)
    world = m.world_points(poses).cpu().numpy()
    assert path.read_bytes() == V.obj_text(world).encode()
    m.save(str(path), poses, voxel_size=1.0)
    thin = m.world_points(poses, 1.0).cpu().numpy()
    assert 0 < len(thin) < len(world) and path.read_bytes() == V.obj_text(thin).encode()
