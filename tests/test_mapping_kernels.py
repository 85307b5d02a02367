"""ops.pcl_backproject / pcl_transform / pcl_to_image (csrc/mapping.hip) against the float64 restatement of
tests/mapping_reference.py, on the CPU emulator and on gfx950.

Scenes: depth 3 + 57 r^2, KITTI-like K, frame f 0.8 f m forward with 0.03 f rad of yaw, at 8x16x2, 24x40x3 and 40x72x4 frames
(one backproject chunk; one chunk nearly full; three chunks of which the last is partial; the 11,520-point cloud of the third is
eleven and a quarter transform / splat blocks).  Every fp32-twin figure is formed before the kernel's output is read; every figure
is printed with -s.

Bounds:
  * backproject: kept rows in the reference's order; count and kept set equal the float64 reference's except inside the band
    |norm64 / threshold - 1| <= 2^-21 (one fp32 rounding of each of x, y, z, their squares, two sums and the root is below 8
    units of 2^-24), which may hold at most 0.1 % of the points (asserted on the reference first; the thresholds 17.3 and 40.1
    leave it empty); coordinates: largest absolute error against float64 <= 4 x the fp32 twin's; colours bitwise.
  * transform, per coordinate: |kernel - ref64| <= 2^-24 |ref64| + 8 x 2^-53 (|R| |xyz| + |t|): one rounding to fp32 plus the
    float64 evaluation (three products, three sums, and the reference's own).
  * splat: occupancy and pixel assignment bitwise (fp64, unfused); the winner equals the float64 reference's except where its two
    closest candidates differ by less than 2^-21 relative (at most 0.5 % of the occupied pixels, asserted on the reference first),
    and there it is one of the in-band candidates; colour = the winner's, bitwise; distance = the fp32 rounding of the winner's
    float64 norm within 1 fp32 ulp.
"""
import functools

import numpy as np
import pytest
import torch

import mapping_reference as R
from clslam_hip import ops
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

SCENES = [(8, 16, 2), (24, 40, 3), (40, 72, 4)]
SCENE_IDS = [f'{h}x{w}x{f}' for h, w, f in SCENES]
U32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _scene(h, w, frames):
    s = R.scene(h, w, frames, seed=h * w + frames)
    for v in s.values():
        v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _clouds(h, w, frames):
    """the frames' camera-frame clouds (float32 rounding of the float64 reference: exact fp32 inputs for transform and splat),
    their offsets"""
    s = _scene(h, w, frames)
    clouds = [R.backproject(s['depth'][f, 0], s['inv_K'][f], s['image'][f])['points'].astype(np.float32) for f in range(frames)]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.concatenate(clouds)
    pts.setflags(write=False)
    return pts, offsets


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a, order='C'))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _backproject(dev, s, thr=np.inf, frames=slice(None)):
    pts, off = ops.pcl_backproject(_t(s['depth'][frames], dev), _t(s['inv_K'][frames], dev), _t(s['image'][frames], dev), thr)
    assert pts.device.type == dev.type and off.dtype == torch.int64 and off.device.type == dev.type
    return pts.cpu().numpy(), off.cpu().numpy()


def _subsequence_mask(rows, all_rows):
    """rows is an ordered selection of all_rows (bitwise): -> the selection mask, or None if it is not one"""
    mask = np.zeros(len(all_rows), bool)
    a, b = _bits(rows), _bits(all_rows)
    j = 0
    for i in range(len(a)):
        while j < len(b) and not np.array_equal(a[i], b[j]):
            j += 1
        if j == len(b):
            return None
        mask[j] = True
        j += 1
    return mask


# ---- backproject --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('thr', [np.inf, 17.3, 40.1], ids=['inf', '17.3', '40.1'])
@pytest.mark.parametrize('h,w,frames', SCENES, ids=SCENE_IDS)
def test_backproject(backend, h, w, frames, thr):
    dev = use_backend(backend)
    s = _scene(h, w, frames)
    r64 = [R.backproject(s['depth'][f, 0], s['inv_K'][f], s['image'][f], thr) for f in range(frames)]
    r32 = [R.backproject(s['depth'][f, 0], s['inv_K'][f], s['image'][f], thr, dtype=np.float32) for f in range(frames)]
    e32 = max(float(np.abs(b['cam'].astype(np.float64) - a['cam']).max()) for a, b in zip(r64, r32))
    bands = [R.threshold_band(a['norm'], a['threshold']) for a in r64]
    for band in bands:                                                           # the reference itself, before the kernel
        assert band.sum() <= 1e-3 * h * w, int(band.sum())
    everything, off_all = _backproject(dev, s)
    assert np.array_equal(off_all, np.arange(frames + 1) * h * w) and everything.shape == (frames * h * w, 6)     # inf keeps H W
    pts, off = _backproject(dev, s, thr)
    assert off[0] == 0 and pts.shape == (off[-1], 6) and (np.diff(off) >= 0).all()
    worst = 0.0
    for f in range(frames):
        rows, all_rows = pts[off[f]:off[f + 1]], everything[f * h * w:(f + 1) * h * w]
        assert np.array_equal(_bits(all_rows[:, 3:]), _bits(r64[f]['colour']))       # colours bitwise, pixel order
        worst = max(worst, float(np.abs(all_rows[:, :3].astype(np.float64) - r64[f]['cam']).max()))
        mask = _subsequence_mask(rows, all_rows)                                     # order preserved, the same bits as keep-all
        assert mask is not None
        differ = mask != r64[f]['keep']
        print(f'[backproject {backend}] {h}x{w} frame {f} thr {thr}: kept {int(mask.sum())} (float64 {int(r64[f]["keep"].sum())}), '
              f'differing {int(differ.sum())}, in band {int(bands[f].sum())}')
        assert not (differ & ~bands[f]).any()
        if not bands[f].any():
            assert off[f + 1] - off[f] == r64[f]['keep'].sum()
    print(f'[backproject {backend}] {h}x{w}x{frames} coordinates max |err|: kernel {worst:.3e} | fp32 {e32:.3e} ({worst / e32:.2f}x)')
    assert worst <= 4 * e32
    # a batch equals its single-image launches, and two launches are equal, bitwise
    again, off2 = _backproject(dev, s, thr)
    assert np.array_equal(_bits(again), _bits(pts)) and np.array_equal(off2, off)
    for f in range(frames):
        one, o1 = _backproject(dev, s, thr, slice(f, f + 1))
        assert np.array_equal(o1, [0, off[f + 1] - off[f]]) and np.array_equal(_bits(one), _bits(pts[off[f]:off[f + 1]]))


@pytest.mark.parametrize('backend', BACKENDS)
def test_backproject_edges(backend):
    dev = use_backend(backend)
    s = _scene(24, 40, 3)
    pts, off = _backproject(dev, s, 0.0)                                             # nothing is closer than 0
    assert pts.shape == (0, 6) and np.array_equal(off, [0, 0, 0, 0])
    pts, off = _backproject(dev, s, 1e9)                                             # finite and beyond everything
    assert np.array_equal(off, np.arange(4) * 960)
    d = s['depth'].copy()
    d[1, 0, 3, 5] = np.nan                                                           # a NaN norm compares false: dropped
    pts, off = ops.pcl_backproject(_t(d, dev), _t(s['inv_K'], dev), _t(s['image'], dev), 1e9)
    assert off.cpu().tolist() == [0, 960, 1919, 2879]
    with pytest.raises(ClslamError):
        _backproject(dev, s, float('nan'))
    args = [_t(s[k], dev) for k in ('depth', 'inv_K', 'image')]
    with pytest.raises(ClslamError):
        ops.pcl_backproject(args[0][:, 0], args[1], args[2])                         # rank
    with pytest.raises(ClslamError):
        ops.pcl_backproject(args[0].double(), args[1], args[2])                      # dtype
    with pytest.raises(ClslamError):
        ops.pcl_backproject(args[0], args[1][:2], args[2])                           # batch mismatch
    with pytest.raises(ClslamError):
        ops.pcl_backproject(args[0][:, :, :0], args[1], args[2][:, :, :0])           # empty planes
    with pytest.raises(ClslamError):
        ops.pcl_backproject(*args, out=torch.empty(100, 6, device=dev))              # no room
    if dev.type == 'cuda':
        with pytest.raises(ClslamError):
            ops.pcl_backproject(args[0].cpu(), args[1], args[2])
    pts, off = ops.pcl_backproject(args[0][:0], args[1][:0], args[2][:0])            # N = 0: no launch
    assert pts.shape == (0, 6) and off.cpu().tolist() == [0]
    out = torch.full((3000, 6), -7.0, device=dev)
    full, off = ops.pcl_backproject(*args, 17.3, out=out, narrow=False)              # the caller's buffer, nothing read back
    assert full.data_ptr() == out.data_ptr() and full.shape == (3000, 6)
    assert (out[int(off[-1]):] == -7.0).all()                                        # nothing written past the kept rows


# ---- backproject: the one-block scan over more chunks than it has threads -----------------------------------------------------------
SCAN_PLANES = [(256, 1, 1, 256), (257, 1, 1, 257), (129, 1, 1025, 258), (86, 1, 2049, 258), (3, 192, 640, 360)]
SCAN_THR = 20.3


@functools.lru_cache(maxsize=None)
def _exact_planes(n, h, w):
    """n planes whose points are exact in fp32, so that float64 and the kernel agree to the bit.  inv_K of image i: focal length
    2^s with 2^s >= max(h, w), a principal point (cx, cy) of its own inside the plane; depths are eighths.  (px - cx) 2^-s has 12
    bits at most and |.| <= 1, a depth below 64 nine: the products are exact, and z = depth.  Image i is, by i % 4: mixed (depth
    1 .. 40: SCAN_THR keeps the pixels with depth * sqrt(u^2 + v^2 + 1) < 20.3, so pixels inside a chunk part ways), near (depth
    below 8: all kept), far (depth from 24: none kept), mixed."""
    rng = np.random.default_rng(1000 * n + h * w)
    s = int(np.ceil(np.log2(max(h, w, 2))))
    inv_K = np.zeros((n, 4, 4), np.float32)
    inv_K[:, 0, 0] = inv_K[:, 1, 1] = 2.0 ** -s
    inv_K[:, 0, 2] = -rng.integers(0, w, n) * 2.0 ** -s
    inv_K[:, 1, 2] = -rng.integers(0, h, n) * 2.0 ** -s
    inv_K[:, 2, 2] = inv_K[:, 3, 3] = 1
    kind = np.arange(n) % 4
    lo = np.where(kind == 1, 8, np.where(kind == 2, 192, 8))[:, None, None, None]
    hi = np.where(kind == 1, 64, np.where(kind == 2, 512, 320))[:, None, None, None]
    depth = (rng.integers(lo, hi, (n, 1, h, w)) / 8.0).astype(np.float32)
    out = {'depth': depth, 'inv_K': inv_K, 'image': rng.random((n, 3, h, w)).astype(np.float32)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _exact_reference(n, h, w, thr):
    """-> (rows (sum M,6) float32, offsets (n+1,), kept per chunk (n, chunks), pixels per chunk (chunks,)); the premises asserted:
    float64 coordinates that fp32 holds exactly, and no distance within 2^-21 of the threshold"""
    s = _exact_planes(n, h, w)
    rows, kept = [], []
    starts = np.arange(0, h * w, 1024)
    for f in range(n):
        r = R.backproject(s['depth'][f, 0], s['inv_K'][f], s['image'][f], thr)
        assert np.array_equal(r['cam'].astype(np.float32).astype(np.float64), r['cam'])
        assert not R.threshold_band(r['norm'], r['threshold']).any()
        rows.append(r['points'].astype(np.float32))
        kept.append(np.add.reduceat(r['keep'].astype(np.int64), starts))
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.concatenate(rows), offsets, np.stack(kept), np.diff(np.concatenate([starts, [h * w]]))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n,h,w,G', SCAN_PLANES, ids=[f'{n}x{h}x{w}' for n, h, w, _ in SCAN_PLANES])
def test_backproject_scan_beyond_one_chunk_per_thread(backend, n, h, w, G):
    """pcl_bp_scan_kernel: one block of 256 threads, thread t scans `per = ceil(G / 256)` chunk counts from `lo = min(t * per, G)`
    and writes offsets[g / chunks] where `g % chunks == 0` inside its loop.
      256 x (1x1)     G = 256  per == 1, every thread exactly one chunk
      257 x (1x1)     G = 257  per == 2, the threads from 129 on empty, every chunk an image of its own
      129 x (1x1025)  G = 258  chunks == 2: a thread's pair is one whole image
      86 x (1x2049)   G = 258  chunks == 3: image boundaries fall inside a thread's range
      3 x (192x640)   G = 360  the workload's own shape
    Rows bitwise and offsets exact against mapping_reference (exact planes: _exact_planes), with an infinite threshold (counts
    known without looking) and with one that keeps about half; there, chunks that keep nothing and chunks that keep everything,
    and whole images that keep nothing.  Measured, seconds per case in the order above, both thresholds and the reference together,
    CPU emulator | MI355X: 0.06 | 0.01, 0.07 | 0.01, 0.08 | 0.01, 0.08 | 0.05, 0.18 | 0.04."""
    dev = use_backend(backend)
    chunks = -(-h * w // 1024)
    assert n * chunks == G and -(-G // 256) == (1 if G <= 256 else 2)
    s = _exact_planes(n, h, w)
    for thr in (np.inf, SCAN_THR):
        rows, offsets, kept, size = _exact_reference(n, h, w, thr)
        if np.isinf(thr):
            assert np.array_equal(offsets, np.arange(n + 1) * h * w)
        else:
            share = offsets[-1] / (n * h * w)
            assert 0.25 <= share <= 0.75, share
            assert (kept == 0).any() and (kept == size).any() and (np.diff(offsets) == 0).any()
            if h * w > 1:
                assert ((kept > 0) & (kept < size)).any()                                # the threshold parts pixels inside a chunk
        pts, off = _backproject(dev, s, thr)
        print(f'[backproject scan {backend}] {n} x ({h}x{w}) thr {thr}: G = {G}, kept {int(offsets[-1])} of {n * h * w}, '
              f'chunks that keep nothing {int((kept == 0).sum())}, everything {int((kept == size).sum())}')
        assert np.array_equal(off, offsets)
        assert pts.shape == rows.shape and np.array_equal(_bits(pts), _bits(rows))


@pytest.mark.parametrize('backend', BACKENDS)
def test_backproject_scan_leaves_the_rest_of_the_buffer(backend):
    """pcl_bp_scan_kernel at `per == 2` (G = 258, 86 planes of 1x2049) with narrow=False: the rows up to offsets[-1] are the
    reference's and the rows past it keep the NaN pattern the buffer was filled with, bit for bit.  Measured: 0.04 s on the CPU
    emulator, under 0.005 s on the MI355X (the reference is the one of the case above)."""
    dev = use_backend(backend)
    n, h, w = 86, 1, 2049
    s = _exact_planes(n, h, w)
    rows, offsets, _, _ = _exact_reference(n, h, w, SCAN_THR)
    assert 0 < offsets[-1] < n * h * w - 1024
    fill = np.uint32(0x7fc0beef)
    out = torch.from_numpy(np.full((n * h * w + 5, 6), fill, np.uint32).view(np.float32)).to(dev)
    full, off = ops.pcl_backproject(_t(s['depth'], dev), _t(s['inv_K'], dev), _t(s['image'], dev), SCAN_THR, out=out, narrow=False)
    assert full.data_ptr() == out.data_ptr() and full.shape == out.shape and np.array_equal(off.cpu().numpy(), offsets)
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:offsets[-1]], _bits(rows)) and (got[offsets[-1]:] == fill).all()


# ---- transform ----------------------------------------------------------------------------------------------------------------
def _metre_poses(n, seed=1):
    """poses that differ by whole metres and by a yaw of 0.2 rad: a point posed with its neighbour's matrix is off by metres"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n):
        T = R.frame_pose(7 * f + 1)
        T[:3, 3] += [3.0 * f + 2, -2.0 * f - 1, 5.0 * f + 4]
        T[:3, :3] = T[:3, :3] @ np.linalg.qr(rng.normal(size=(3, 3)))[0]
        out.append(T)
    return np.stack(out)


def _check_transform(backend, case, pts, offsets, poses, dev):
    ref, mag = R.transform(pts, offsets, poses)
    bound = U32 * np.abs(ref) + 8 * 2.0 ** -53 * mag
    out = ops.pcl_transform(_t(pts, dev), _t(offsets, dev), _t(poses, dev)).cpu().numpy()
    assert out.shape == pts.shape
    if len(pts):
        err = np.abs(out[:, :3].astype(np.float64) - ref)
        print(f'[transform {backend}] {case}: {len(pts)} points, {len(offsets) - 1} segments, max err / bound {float((err / bound).max()):.3f}')
        assert (err <= bound).all()
    assert np.array_equal(_bits(out[:, 3:]), _bits(pts[:, 3:]))                      # colours bitwise
    return out


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('m', [1, 63, 64, 65, 11520])
def test_transform_sizes(backend, m):
    dev = use_backend(backend)
    pts = _clouds(40, 72, 4)[0][:m]
    assert len(pts) == m
    _check_transform(backend, f'one segment of {m}', pts, np.array([0, m]), _metre_poses(1), dev)
    ident = ops.pcl_transform(_t(pts, dev), [0, m], _t(np.eye(4)[None], dev)).cpu().numpy()
    assert np.array_equal(_bits(ident), _bits(pts))                                  # the identity pose returns the input bitwise


@pytest.mark.parametrize('backend', BACKENDS)
def test_transform_segments(backend):
    """one pose per segment, applied to exactly its points: frame clouds (boundaries at 2880 k, inside blocks of 1024 and inside
    tiles of 256), then empty first, middle and last segments, segments of one point, and a boundary on a block boundary"""
    dev = use_backend(backend)
    pts, offsets = _clouds(40, 72, 4)
    _check_transform(backend, 'frames', pts, offsets, _metre_poses(4), dev)
    ragged = np.array([0, 0, 1, 2, 2, 2, 700, 1024, 1025, 5000, 5000, 11520, 11520, 11520])
    _check_transform(backend, 'ragged', pts, ragged, _metre_poses(len(ragged) - 1), dev)
    few = np.array([0, 0, 3100, 3100])                                               # a little over three blocks, empty ends
    _check_transform(backend, 'empty ends', pts[:3100], few, _metre_poses(3), dev)
    assert ops.pcl_transform(_t(pts[:0], dev), [0, 0], _t(_metre_poses(1), dev)).shape == (0, 6)      # M = 0: no launch
    p, T = _t(pts, dev), _t(_metre_poses(4), dev)
    for bad in (lambda: ops.pcl_transform(p[:, :5], offsets, T), lambda: ops.pcl_transform(p.double(), offsets, T),
                lambda: ops.pcl_transform(p, offsets, T.float()), lambda: ops.pcl_transform(p, offsets[:-1], T),
                lambda: ops.pcl_transform(p, [0, 5, 3, 7, 11520], T), lambda: ops.pcl_transform(p, offsets, T[:, :3])):
        with pytest.raises(ClslamError):
            bad()


# ---- splat --------------------------------------------------------------------------------------------------------------------
def _render(dev, pts, K, shape, **kw):
    out = ops.pcl_to_image(_t(pts, dev), _t(K, dev), shape, return_dist=True, return_index=True,
                           **{k: (_t(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    return [o.cpu().numpy() for o in out]


def _check_splat(backend, case, pts, K, shape, image, dist, index, min_z=None, scene=True):
    z = R.zbuffer(pts, K, shape, min_z)
    close = R.close_calls(z)
    occupied = z['index'] >= 0
    if scene:               # (the hand-made clouds hold exact ties on purpose: their winners are asserted one by one)
        assert close.sum() <= 5e-3 * max(1, occupied.sum()), (case, int(close.sum()))  # the reference itself, before the kernel
    assert np.array_equal(index >= 0, occupied), case                                # occupancy: exact at every pixel
    differ = index != z['index']
    print(f'[splat {backend}] {case}: occupied {int(occupied.sum())}/{occupied.size}, contested {int((z["count"] > 1).sum())}, '
          f'close calls {int(close.sum())}, differing winners {int(differ.sum())}')
    assert not (differ & ~close).any(), case
    for p in np.flatnonzero(differ.reshape(-1)):
        assert index.reshape(-1)[p] in R.in_band_candidates(z, p), (case, p)
    win = index[occupied]
    assert np.array_equal(_bits(image[occupied]), _bits(pts[win, 3:])) and (image[~occupied] == 0).all(), case
    assert np.isposinf(dist[~occupied]).all()
    want = z['all_dist'][win]
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(dist[occupied].astype(np.float64) - want)
    if err.size:
        print(f'[splat {backend}] {case}: distance max err {float((err / ulp).max()):.3f} fp32 ulp')
    assert (err <= ulp).all(), case
    return z


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('h,w,frames', SCENES, ids=SCENE_IDS)
def test_splat_scenes(backend, h, w, frames):
    """every frame of the scene, posed, seen from frame 0's camera (frame 0 re-projects into its own pixels: u lands on or
    within an ulp of integers); then with the poses applied on the fly: index and colour planes bitwise equal"""
    dev = use_backend(backend)
    s = _scene(h, w, frames)
    pts, offsets = _clouds(h, w, frames)
    world = ops.pcl_transform(_t(pts, dev), offsets, _t(s['poses'], dev)).cpu().numpy()
    own = R.project(world[:h * w, :3], s['K'], h, w)
    print(f'[splat {backend}] {h}x{w}: frame 0 lands in its own pixel at {int((own == np.arange(h * w)).sum())}/{h * w} points')
    image, dist, index = _render(dev, world, s['K'], (h, w))
    _check_splat(backend, f'{h}x{w}x{frames}', world, s['K'], (h, w), image, dist, index)
    fly = _render(dev, pts, s['K'], (h, w), offsets=offsets, poses=s['poses'])
    assert np.array_equal(fly[2], index) and np.array_equal(_bits(fly[0]), _bits(image)) and np.array_equal(_bits(fly[1]), _bits(dist))
    # a cloud split into two launches, and into many, gives the same planes as one
    for chunk in (len(pts) // 2 + 1, 257):
        part = _render(dev, pts, s['K'], (h, w), offsets=offsets, poses=s['poses'], max_launch_points=chunk)
        assert np.array_equal(part[2], index) and np.array_equal(_bits(part[0]), _bits(image)) and np.array_equal(_bits(part[1]), _bits(dist))
    # a second view: from the last frame, culling what lies behind it
    view = np.linalg.inv(s['poses'][-1]) @ s['poses']
    image, dist, index = _render(dev, pts, s['K'], (h, w), offsets=offsets, poses=view, min_z=0.0)
    seen = ops.pcl_transform(_t(pts, dev), offsets, _t(view, dev)).cpu().numpy()
    _check_splat(backend, f'{h}x{w}x{frames} from the last frame', seen, s['K'], (h, w), image, dist, index, min_z=0.0)
    small = pts[:2000]                                                               # the vectorised z-buffer against the per-point loop
    assert np.array_equal(R.pcl_to_image_loop(small, s['K'], (h, w)).astype(np.float32), R.zbuffer(small, s['K'], (h, w))['image'])


def _row(x, y, z, c):
    return [x, y, z, c, c + 0.25, c + 0.5]


@pytest.mark.parametrize('backend', BACKENDS)
def test_splat_hand_made(backend):
    dev = use_backend(backend)
    K = np.array([[10.0, 0, 4.0], [0, 10.0, 3.0], [0, 0, 1]])
    rows, cols = 6, 8

    def render(points, shape=(rows, cols), **kw):
        points = np.asarray(points, dtype=np.float32).reshape(-1, 6)
        out = _render(dev, points, K, shape, **kw)
        _check_splat(backend, 'hand-made', points, K, shape, *out, min_z=kw.get('min_z'), scene=False)
        return out

    # two identical points: the lower index wins; the list reversed: the other copy
    a, b = _row(0.1, 0.1, 2.0, 1.0), _row(0.1, 0.1, 2.0, 2.0)
    image, dist, index = render([a, b])
    assert index[3, 4] == 0 and image[3, 4, 0] == 1.0 and (index >= 0).sum() == 1
    image, dist, index = render([b, a])
    assert index[3, 4] == 0 and image[3, 4, 0] == 2.0
    # the closer of two wins whatever the order; distance is the Euclidean norm, not z
    image, dist, index = render([_row(0.0, 0.0, 1.03, 3.0), _row(0.05, 0.04, 1.0, 4.0)])
    assert index[3, 4] == 1                                                          # |.| = 1.0021 < 1.03
    image, dist, index = render([_row(0.09, 0.09, 1.0, 3.0), _row(0.0, 0.0, 1.005, 4.0)])
    assert index[3, 4] == 1                                                          # z = 1 is nearer in z, |.| = 1.008 is not
    # borders: u = -0.5 is outside (floor, not truncation); u = cols exactly is outside; v = rows - 2^-40 is inside
    z = 1.0
    pts = [_row((-0.5 - 4.0) / 10, 0.0, z, 1.0), _row((cols - 4.0) / 10, 0.0, z, 2.0), _row(0.0, (rows - 2.0 ** -40 - 3.0) / 10, z, 3.0)]
    pix = R.project(np.asarray(pts, np.float32)[:, :3], K, rows, cols)
    image, dist, index = render(pts)
    print(f'[splat {backend}] borders: pixels {pix.tolist()}')
    assert np.array_equal(index >= 0, np.isin(np.arange(rows * cols), pix[pix >= 0]).reshape(rows, cols))
    # the three cases exactly: K is float64, so u = -0.5, u = cols and v = rows - 2^-40 are formed without a rounding
    K2 = np.array([[8.0, 0, 4.0], [0, 8.0, rows - 2.0 ** -40], [0, 0, 1]])
    exact = np.asarray([_row(-4.5 / 8, 0.0, 1.0, 1.0), _row((cols - 4.0) / 8, 0.0, 1.0, 2.0), _row(0.0, 0.0, 1.0, 3.0)], dtype=np.float32)
    assert R.project(exact[:, :3], K2, rows, cols).tolist() == [-1, -1, (rows - 1) * cols + 4]       # out, out, in
    out = _render(dev, exact, K2, (rows, cols))
    assert (out[2] >= 0).sum() == 1 and out[2][rows - 1, 4] == 2
    # behind the camera: mirrored in by default, culled with min_z = 0
    behind = [_row(0.1, 0.1, -2.0, 5.0)]
    image, dist, index = render(behind)
    assert index[2, 3] == 0                                                          # (-0.05 * 10 + 4, -0.05 * 10 + 3) = (3.5, 2.5)
    image, dist, index = render(behind, min_z=0.0)
    assert (index == -1).all() and (image == 0).all()
    # z = 0 projects as z = 1
    image, dist, index = render([_row(0.1, 0.2, 0.0, 6.0)])
    assert index[5, 5] == 0
    # NaN and +-inf coordinates are skipped
    bad = [_row(np.nan, 0, 1, 1.0), _row(0, np.inf, 1, 2.0), _row(0, 0, -np.inf, 3.0), _row(0, 0, np.nan, 4.0), _row(0.0, 0.0, 1.0, 5.0)]
    image, dist, index = render(bad)
    assert (index >= 0).sum() == 1 and index[3, 4] == 4
    # the 1-point and 0-point clouds, a 1x1 image
    image, dist, index = render([_row(0.0, 0.0, 1.0, 7.0)])
    assert index[3, 4] == 0 and dist[3, 4] == 1.0
    image, dist, index = render(np.zeros((0, 6)))
    assert (index == -1).all() and (image == 0).all() and np.isposinf(dist).all()
    K1 = np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1]])
    out = _render(dev, np.asarray([_row(0.2, 0.2, 1.0, 8.0), _row(0.7, 0.0, 1.0, 9.0), _row(0.1, 0.1, 0.9, 1.5)], np.float32), K1, (1, 1))
    assert out[0].shape == (1, 1, 3) and out[2][0, 0] == 2 and out[0][0, 0, 0] == 1.5
    # only the image unless asked for more
    assert isinstance(ops.pcl_to_image(_t(np.asarray([a], np.float32), dev), _t(K, dev), (rows, cols)), torch.Tensor)


@pytest.mark.parametrize('backend', BACKENDS)
def test_splat_argument_checks(backend):
    dev = use_backend(backend)
    pts, offsets = _clouds(8, 16, 2)
    p, K = _t(pts, dev), _t(R.camera(8, 16)[0], dev)
    T = _t(np.stack([np.eye(4)] * 2), dev)
    for bad in (lambda: ops.pcl_to_image(p[:, :5], K, (8, 16)), lambda: ops.pcl_to_image(p.double(), K, (8, 16)),
                lambda: ops.pcl_to_image(p, K.float(), (8, 16)), lambda: ops.pcl_to_image(p, K[:2], (8, 16)),
                lambda: ops.pcl_to_image(p, K, (0, 16)), lambda: ops.pcl_to_image(p, K, (8, 16), poses=T),
                lambda: ops.pcl_to_image(p, K, (8, 16), offsets=offsets[:-1], poses=T),
                lambda: ops.pcl_to_image(p, K, (8, 16), min_z=float('nan')),
                lambda: ops.pcl_to_image(p, K, (8, 16), max_launch_points=0)):
        with pytest.raises(ClslamError):
            bad()
    if dev.type == 'cuda':
        with pytest.raises(ClslamError):
            ops.pcl_to_image(p.cpu(), K, (8, 16))


@pytest.mark.gpu
def test_splat_past_two_to_the_31_floats():
    """a cloud whose float offsets pass 2^31 (358 M rows, 8.6 GB: NaN rows, which the splat skips, and three real points at the
    very end): the last rows are read, win, and come back with their 64-bit indices"""
    dev = use_backend('hip')
    m = (1 << 31) // 6 + 1000
    big = torch.empty(m, 6, device=dev)
    big.view(torch.int32).fill_(-1)                                                  # all bits set: NaN
    tail = np.asarray([_row(0.0, 0.0, 2.0, 1.0), _row(0.0, 0.0, 1.0, 2.0), _row(0.1, 0.0, 1.0, 3.0)], np.float32)
    big[m - 3:] = torch.from_numpy(tail).to(dev)
    K = np.array([[10.0, 0, 4.0], [0, 10.0, 3.0], [0, 0, 1]])
    offsets = [0, m - 2, m]
    poses = np.stack([np.eye(4), np.eye(4)])
    poses[1, 0, 3] = 0.15                                                            # the last two rows move to u = 5.5 and 6.5
    try:
        image, dist, index = ops.pcl_to_image(big, _t(K, dev), (6, 8), offsets=offsets, poses=_t(poses, dev), return_dist=True,
                                              return_index=True)
        index = index.cpu().numpy()
        assert (index >= 0).sum() == 3 and index[3, 4] == m - 3 and index[3, 5] == m - 2 and index[3, 6] == m - 1
        assert image[3, 6, 0].item() == 3.0 and dist[3, 4].item() == 2.0
        out = ops.pcl_transform(big, offsets, _t(poses, dev))
        assert np.array_equal(out[m - 3:].cpu().numpy()[:, 3:], tail[:, 3:]) and abs(out[m - 1, 0].item() - 0.25) < 1e-6
    finally:
        del big
        out = None
        torch.cuda.empty_cache()
