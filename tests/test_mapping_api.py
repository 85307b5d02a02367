"""The public face of the mapping kernels: clslam_hip.mapping.depth_to_pcl / accumulate_pcl / pcl_to_image (the reference's names,
argument order and defaults, slam/utils.py:25-82) and DenseMap.  Bounds: those of tests/test_mapping_kernels.py, carried to
what the functions return; everything else here is bitwise (the same kernels on the same inputs, whatever they arrive as)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mapping_reference as R
from clslam_hip import mapping
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

H, W, F = 24, 40, 3
U32 = 2.0 ** -24


def _scene(frames=F, seed=5):
    return R.scene(H, W, frames, seed=seed)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _forms(a, dev):
    """numpy, host tensor, device tensor"""
    return a, torch.from_numpy(np.array(a)), torch.from_numpy(np.array(a)).to(dev)


def _is_form(x, i, dev):
    if i == 0:
        return isinstance(x, np.ndarray) and x.dtype == np.float32
    return isinstance(x, torch.Tensor) and x.dtype is torch.float32 and x.device.type == ('cpu' if i == 1 else dev.type)


@pytest.mark.parametrize('backend', BACKENDS)
def test_reference_named_functions_accept_numpy_host_and_device_inputs(backend):
    dev = use_backend(backend)
    s = _scene()
    bp = SimpleNamespace(height=H, width=W)                                          # BackprojectDepth is used for its size only
    # depth_to_pcl ----------------------------------------------------------------------------------------------------------
    r64 = R.backproject(s['depth'][0, 0], s['inv_K'][0], s['image'][0], 17.3)
    r32 = R.backproject(s['depth'][0, 0], s['inv_K'][0], s['image'][0], 17.3, dtype=np.float32)
    e32 = float(np.abs(r32['cam'].astype(np.float64) - r64['cam']).max())
    assert not R.threshold_band(r64['norm'], r64['threshold']).any()
    clouds = []
    for i, (d, ik, im) in enumerate(zip(_forms(s['depth'][:1], dev), _forms(s['inv_K'][:1], dev), _forms(s['image'][:1], dev))):
        pcl = mapping.depth_to_pcl(bp, ik, d, im, dist_threshold=17.3)
        assert _is_form(pcl, i, dev) and tuple(pcl.shape) == (int(r64['keep'].sum()), 6)
        clouds.append(pcl)
    assert np.array_equal(_bits(clouds[0]), _bits(clouds[1])) and np.array_equal(_bits(clouds[0]), _bits(clouds[2]))
    assert np.abs(clouds[0][:, :3].astype(np.float64) - r64['points'][:, :3]).max() <= 4 * e32
    assert np.array_equal(_bits(clouds[0][:, 3:]), _bits(r64['colour'][r64['keep']]))
    everything = mapping.depth_to_pcl(bp, s['inv_K'][:1], s['depth'][:1], s['image'][:1])          # the defaults: batch 1, inf
    assert everything.shape == (H * W, 6)
    assert np.array_equal(_bits(mapping.depth_to_pcl(None, s['inv_K'][0], s['depth'][0, 0], s['image'][0])), _bits(everything))
    with pytest.raises(ClslamError):
        mapping.depth_to_pcl(bp, s['inv_K'], s['depth'], s['image'])                 # three planes, batch_size 1
    assert mapping.depth_to_pcl(bp, s['inv_K'], s['depth'], s['image'], batch_size=3).shape == (3 * H * W, 6)
    # accumulate_pcl: a list of clouds == the concatenation of the per-cloud references ----------------------------------
    pcl_list = [mapping.depth_to_pcl(bp, s['inv_K'][f], s['depth'][f], s['image'][f], dist_threshold=t)
                for f, t in zip(range(F), (17.3, np.inf, 40.1))]
    assert len({len(p) for p in pcl_list}) == 3
    ref = np.concatenate([R.accumulate([p], [T]) for p, T in zip(pcl_list, s['poses'])])
    mags = np.concatenate([R.transform(p, [0, len(p)], [T])[1] for p, T in zip(pcl_list, s['poses'])])
    acc = []
    for i in range(3):
        out = mapping.accumulate_pcl([_forms(p, dev)[i] for p in pcl_list], s['poses'])
        assert _is_form(out, i, dev) and tuple(out.shape) == ref.shape
        acc.append(out)
    assert np.array_equal(_bits(acc[0]), _bits(acc[1])) and np.array_equal(_bits(acc[0]), _bits(acc[2]))
    assert (np.abs(acc[0][:, :3].astype(np.float64) - ref[:, :3]) <= U32 * np.abs(ref[:, :3]) + 8 * 2.0 ** -53 * mags).all()
    assert np.array_equal(acc[0][:, 3:].astype(np.float64), ref[:, 3:])
    assert np.array_equal(_bits(mapping.accumulate_pcl(pcl_list, list(s['poses']))), _bits(acc[0]))   # a list of 4x4 arrays
    # pcl_to_image ----------------------------------------------------------------------------------------------------------
    z = R.zbuffer(acc[0], s['K'], (H, W))
    assert not R.close_calls(z).any()
    views = []
    for i in range(3):
        img = mapping.pcl_to_image(_forms(acc[0], dev)[i], s['K'], (H, W))
        assert _is_form(img, i, dev) and tuple(img.shape) == (H, W, 3)
        views.append(img)
    assert np.array_equal(_bits(views[0]), _bits(z['image']))
    assert np.array_equal(_bits(views[0]), _bits(views[1])) and np.array_equal(_bits(views[0]), _bits(views[2]))
    K4 = np.eye(4)
    K4[:3, :3] = s['K']
    assert np.array_equal(_bits(mapping.pcl_to_image(acc[0], torch.from_numpy(K4), (H, W))), _bits(views[0]))


def _fill(m, s, frames, thr=np.inf, dev=None):
    for f in frames:
        m.add_frame(10 * f, torch.from_numpy(s['depth'][f:f + 1]).to(dev), torch.from_numpy(s['image'][f:f + 1]).to(dev),
                    torch.from_numpy(s['inv_K'][f:f + 1]).to(dev), dist_threshold=thr)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('thr', [np.inf, 40.1], ids=['inf', '40.1'])
def test_dense_map(backend, thr):
    dev = use_backend(backend)
    n = 6
    s = _scene(n, seed=9)
    refs = [R.backproject(s['depth'][f, 0], s['inv_K'][f], s['image'][f], thr) for f in range(n)]
    assert not any(R.threshold_band(r['norm'], r['threshold']).any() for r in refs)
    m = mapping.DenseMap()
    assert len(m) == 0 and m.num_points == 0 and m.device.type == dev.type
    _fill(m, s, range(n), thr, dev)
    # it grew across reallocations and the contents survived: every frame's rows equal a one-frame launch, bitwise
    assert m.reallocations >= 3 and m.capacity >= m.num_points
    assert len(m) == n and m.step_ids == [10 * f for f in range(n)]
    counts = [int(r['keep'].sum()) for r in refs]
    assert np.array_equal(m.offsets, np.concatenate([[0], np.cumsum(counts)])) and m.num_points == sum(counts)
    bp = SimpleNamespace(height=H, width=W)
    single = [mapping.depth_to_pcl(bp, s['inv_K'][f], s['depth'][f], s['image'][f], dist_threshold=thr) for f in range(n)]
    assert np.array_equal(_bits(m.points), _bits(np.concatenate(single)))
    with pytest.raises(ClslamError):
        _fill(m, s, [2], thr, dev)                                                   # a step is added once
    # world_points: a mapping or the pose graph's list; changing the poses re-poses the map == a fresh map with the new poses
    poses = {10 * f: s['poses'][f] for f in range(n)}
    world = m.world_points(poses)
    assert world.device.type == dev.type and tuple(world.shape) == (m.num_points, 6)
    assert np.array_equal(_bits(world), _bits(mapping.accumulate_pcl(single, s['poses'])))
    assert np.array_equal(_bits(m.world_points(list(s['poses']))), _bits(world))
    moved = {k: R.frame_pose(3) @ T for k, T in poses.items()}
    fresh = mapping.DenseMap()
    _fill(fresh, s, range(n), thr, dev)
    assert np.array_equal(_bits(m.world_points(moved)), _bits(fresh.world_points(moved)))
    assert not np.array_equal(_bits(m.world_points(moved)), _bits(world))
    # a frame without a pose raises
    with pytest.raises(ClslamError, match='no pose'):
        m.world_points({k: v for k, v in poses.items() if k != 30})
    with pytest.raises(ClslamError, match='no pose'):
        m.render(list(s['poses'][:-1]), s['poses'][0], s['K'], (H, W))
    # render == the z-buffer of the cloud posed into the view; exclude == a map that never had the frame
    view = s['poses'][n - 1]
    image, dist, index = m.render(poses, view, s['K'], (H, W), return_dist=True, return_index=True)
    seen = mapping.accumulate_pcl(single, np.linalg.inv(view) @ s['poses'])
    z = R.zbuffer(seen, s['K'], (H, W))
    assert not R.close_calls(z).any()
    assert np.array_equal(index.cpu().numpy(), z['index']) and np.array_equal(_bits(image), _bits(z['image']))
    assert np.array_equal(_bits(m.render(poses, view, s['K'], (H, W))), _bits(image))
    without = mapping.DenseMap()
    _fill(without, s, [f for f in range(n) if f != n - 1], thr, dev)
    a = m.render(poses, view, s['K'], (H, W), exclude=10 * (n - 1), return_dist=True)
    b = without.render(poses, view, s['K'], (H, W), return_dist=True)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert not np.array_equal(_bits(a[0]), _bits(image))
    c = m.render(poses, view, s['K'], (H, W), exclude={10 * (n - 1), 0}, min_z=0.0)
    z2 = R.zbuffer(mapping.accumulate_pcl(single[1:-1], (np.linalg.inv(view) @ s['poses'])[1:-1]), s['K'], (H, W), min_z=0.0)
    assert not R.close_calls(z2).any() and np.array_equal(_bits(c), _bits(z2['image']))
    # clear() empties it; the buffer is kept
    cap = m.capacity
    m.clear()
    assert len(m) == 0 and m.num_points == 0 and m.capacity == cap and m.world_points({}).shape == (0, 6)
    assert (m.render({}, np.eye(4), s['K'], (H, W)) == 0).all()
    _fill(m, s, [1], thr, dev)
    assert np.array_equal(_bits(m.points), _bits(single[1]))


@pytest.mark.parametrize('backend', BACKENDS)
def test_add_frame_takes_sample_0_of_the_planes_adapt_returns(backend):
    """outputs['depth', 0] is (B,1,H,W), inputs['rgb', 0, 0] (B,3,H,W), inputs['inv_K', 0] (B,4,4): sample 0 only
    (slam.py:180-182, 266); single planes and numpy arrive at the same rows"""
    dev = use_backend(backend)
    s = _scene(3, seed=11)
    s['inv_K'][1:, 0, 0] *= 2                                                        # the other samples differ in every input
    d, im, ik = (torch.from_numpy(s[k]).to(dev) for k in ('depth', 'image', 'inv_K'))
    want = mapping.depth_to_pcl(None, s['inv_K'][0], s['depth'][0, 0], s['image'][0])
    m = mapping.DenseMap(capacity=10)
    m.add_frame(0, d, im, ik)
    m.add_frame(1, d[0], im[0], ik[0])
    m.add_frame(2, s['depth'][0, 0], s['image'][0], s['inv_K'][0])
    m.add_frame(3, d[1:], im[1:], ik[1:])
    assert m.num_points == 4 * H * W
    got = m.points.cpu().numpy().reshape(4, H * W, 6)
    assert all(np.array_equal(_bits(got[i]), _bits(want)) for i in range(3))
    assert np.array_equal(_bits(got[3]), _bits(mapping.depth_to_pcl(None, s['inv_K'][1], s['depth'][1, 0], s['image'][1])))
    assert not np.array_equal(_bits(got[3]), _bits(want))
    with pytest.raises(ClslamError):
        m.add_frame(4, d, im[:, :2], ik)
