"""csrc/viz.hip one kernel at a time against tests/viz_reference.py (the numpy restatement of include/clslam_hip.h "Frame panels")
and the recorded matplotlib colours of tests/golden/viz_colormap.npz.  Every comparison is bit-equal unless it says otherwise."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import viz_reference as ref
from emu_util import BACKENDS, use_backend

sys.path.insert(0, str(Path(__file__).resolve().parent / 'golden'))
import make_viz_golden as golden  # noqa: E402

RANGE_SIZES = [(1, 1), (1, 2), (1, 3), (3, 7), (5, 51), (16, 16), (1, 257), (33, 67)]        # n = 1, 2, 3, 21, 255, 256, 257, 2211
QS = (0, 50, 95, 100)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _value_kinds(h, w, seed):
    """name -> (h,w) float32 plane"""
    rng = np.random.default_rng(seed)
    n = h * w
    smooth = (rng.random(n) ** 2 * 80).astype(np.float32)
    signed = (rng.normal(size=n) * 3).astype(np.float32)
    signed[rng.permutation(n)[:max(1, n // 8)]] = -0.0
    signed[rng.permutation(n)[:max(1, n // 8)]] = 0.0
    sprinkled = smooth.copy()
    bad = rng.permutation(n)[:max(1, n // 10)]
    sprinkled[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), bad.size)
    step = np.sort(smooth)                       # a[k] and a[k+1] one apart at q = 95: integers below the rank, one more above it
    k = int(np.floor(0.95 * (n - 1)))
    step[:k + 1], step[k + 1:] = 7.0, 8.0
    kinds = {'smooth': smooth, 'constant': np.full(n, 2.5, np.float32), 'integers': np.round(smooth), 'one_apart': rng.permutation(step),
             'signed_zeros': signed, 'sprinkled': sprinkled, 'all_nan': np.full(n, np.nan, np.float32)}
    return {name: v.reshape(h, w).astype(np.float32) for name, v in kinds.items()}


def _check_range(planes, q, got_range, got_count):
    for i, plane in enumerate(planes):
        vmin, vmax, m = ref.depth_range(plane, q)
        assert int(got_count[i]) == m
        assert _bits(got_range[i, 0]) == _bits(vmin) and _bits(got_range[i, 1]) == _bits(vmax), (i, q, got_range[i], vmin, vmax)
        if m == plane.size:                      # np.percentile itself, as a guard against a wrong rank: no non-finite value
            want = np.percentile(plane, q)
            assert abs(float(got_range[i, 1]) - float(want)) <= 1e-5 * abs(float(want)), (q, got_range[i, 1], want)
            assert got_range[i, 0] == plane.min()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', RANGE_SIZES, ids=lambda s: f'n{s[0] * s[1]}')
def test_range_sizes_and_value_kinds(backend, shape):
    from clslam_hip import ops
    device = use_backend(backend)
    kinds = _value_kinds(*shape, seed=shape[0] * 1000 + shape[1])
    planes = np.stack(list(kinds.values()))      # one call, seven planes of different contents
    for q in QS:
        rng, count = ops.viz_range(torch.from_numpy(planes).to(device), q)
        _check_range(planes, q, rng.cpu().numpy(), count.cpu().numpy())
    m21 = 0.95 * 20
    assert shape != (3, 7) or m21 == np.floor(m21)          # n = 21: the fraction g is exactly 0


@pytest.mark.parametrize('backend', BACKENDS)
def test_range_batch_of_three_and_degenerate_planes(backend):
    from clslam_hip import ops
    device = use_backend(backend)
    rng = np.random.default_rng(5)
    planes = np.stack([(rng.random((9, 31)) * 50).astype(np.float32), -(rng.random((9, 31)) * 5).astype(np.float32),
                       np.full((9, 31), np.nan, np.float32)])
    planes[2, 4, 4] = 3.25                       # one finite value: m = 1, vmin = vmax = it
    got, count = ops.viz_range(torch.from_numpy(planes).to(device), 95.0)
    _check_range(planes, 95.0, got.cpu().numpy(), count.cpu().numpy())
    assert count.tolist() == [279, 279, 1] and got[2].tolist() == [3.25, 3.25]
    empty, count = ops.viz_range(torch.full((1, 2, 2), float('inf'), device=device), 50.0)
    assert torch.isnan(empty).all() and count.tolist() == [0]


@pytest.mark.parametrize('backend', BACKENDS)
def test_range_refuses_bad_arguments(backend):
    from clslam_hip import ops
    from clslam_hip._lib import ClslamError
    device = use_backend(backend)
    x = torch.zeros((1, 2, 2), device=device)
    for q in (-1.0, 100.5, float('nan')):
        with pytest.raises(ClslamError, match='q must lie'):
            ops.viz_range(x, q)
    with pytest.raises(ClslamError, match='float32'):
        ops.viz_range(x.double())


@pytest.mark.gpu
def test_range_at_the_network_size_on_the_device():
    from clslam_hip import ops
    device = use_backend('hip')
    rng = np.random.default_rng(8)
    planes = np.stack([(rng.random((192, 640)) ** 2 * 80).astype(np.float32), np.round(rng.random((192, 640)) * 30).astype(np.float32)])
    planes[1, ::7, ::5] = np.nan
    for q in QS:
        got, count = ops.viz_range(torch.from_numpy(planes).to(device), q)
        _check_range(planes, q, got.cpu().numpy(), count.cpu().numpy())


# ---- colour map ------------------------------------------------------------------------------------------------------------------
def _golden():
    with np.load(ref.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('backend', BACKENDS)
def test_tables_of_the_golden_file_and_of_the_kernel(backend):
    """the recorded tables are matplotlib's, and the table in the kernel source is the recorded one, entry for entry"""
    from clslam_hip import ops
    device = use_backend(backend)
    g = _golden()
    assert g['magma_r'].shape == (256, 3) and g['magma_r'].dtype == np.uint8
    assert g['magma_r'][0].tolist() == [251, 252, 191] and g['magma_r'][-1].tolist() == [0, 0, 3]
    assert np.array_equal(g['magma'], g['magma_r'][::-1])
    ramp = torch.from_numpy(((np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)).reshape(1, 1, 256)).to(device)
    rng = torch.tensor([[0.0, 1.0]], dtype=torch.float32, device=device)         # xa = j + 0.5 exactly: entry j
    for cmap in ('magma', 'magma_r'):
        assert np.array_equal(ops.viz_compose([ops.viz_cmap_row(ramp, rng, cmap)], 1, 1, 256)[0, 0].cpu().numpy(), g[cmap]), cmap


@pytest.mark.parametrize('backend', BACKENDS)
def test_colour_map_against_recorded_matplotlib(backend):
    """every recorded case: W in {1, 5, 64, 67} x H in {1, 3, 33} x three ranges (one of them vmin == vmax), both maps; the planes
    hold vmin, vmax, their float32 neighbours, exact-integer xa, NaN and both infinities (make_viz_golden.colour_plane)"""
    from clslam_hip import ops
    device = use_backend(backend)
    g = _golden()
    seen = set()
    for name, x, vmin, vmax, cmap in golden.cases():
        h, w = x.shape
        if h * w >= 19:                          # room for every special value
            assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x == vmin).any() and (x == vmax).any()
        rng = torch.tensor([[vmin, vmax]], dtype=torch.float32, device=device)
        got = ops.viz_compose([ops.viz_cmap_row(torch.from_numpy(x[None]).to(device), rng, cmap)], 1, h, w)[0].cpu().numpy()
        assert np.array_equal(got, ref.colorize(x, vmin, vmax, cmap)), name
        want = g['rgb_' + name].copy()
        # imshow masks a NaN pixel whatever the range; Normalize alone gives it entry 0 when vmin == vmax: the kernel follows imshow
        want[np.isnan(x)] = 0
        assert np.array_equal(got, want), name
        seen.add((cmap, float(vmin) == float(vmax)))
    assert len(seen) == 4


def test_colour_map_live_against_matplotlib():
    matplotlib = pytest.importorskip('matplotlib')
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    from clslam_hip import ops
    device = use_backend('emu')
    x = golden.colour_plane(33, 67, np.float32(0.4), np.float32(55.5), seed=99)
    rng = torch.tensor([[0.4, 55.5]], dtype=torch.float32, device=device)
    for cmap in ('magma_r', 'magma'):
        got = ops.viz_compose([ops.viz_cmap_row(torch.from_numpy(x[None]).to(device), rng, cmap)], 1, 33, 67)[0].numpy()
        want = colormaps[cmap](Normalize(np.float32(0.4), np.float32(55.5))(x), bytes=True)[..., :3]
        assert np.array_equal(got, want), (cmap, matplotlib.__version__)


@pytest.mark.parametrize('backend', BACKENDS)
def test_destination_offset_stride_and_surroundings(backend):
    """two rows into the middle of a wider, taller destination of two images: the bytes around the rectangle stay as they were"""
    from clslam_hip import ops
    device = use_backend(backend)
    rng = np.random.default_rng(4)
    n, h, w = 2, 11, 13
    depth = (rng.random((n, h, w)) * 30).astype(np.float32)
    image = rng.random((n, h, w, 3)).astype(np.float32)
    rr = np.array([[2.0, 20.0], [5.0, 25.0]], np.float32)
    before = rng.integers(0, 256, (n, 40, 21, 3), dtype=np.uint8)
    dst = torch.from_numpy(before.copy()).to(device)
    view = dst[:, :, 4:, :]                      # wider rows behind a column offset: stride(1) = 63 > 3 * 13
    out = ops.viz_compose([ops.viz_cmap_row(torch.from_numpy(depth).to(device), torch.from_numpy(rr).to(device), 'magma'),
                           ops.viz_image_row(torch.from_numpy(image).to(device))], n, h, w, dst=view, row0=7)
    assert out.data_ptr() == view.data_ptr()
    want = before.copy()
    for i in range(n):
        want[i, 7:7 + h, 4:4 + w] = ref.colorize(depth[i], rr[i, 0], rr[i, 1], 'magma')
        want[i, 7 + h:7 + 2 * h, 4:4 + w] = ref.image_row(image[i])
    assert np.array_equal(dst.cpu().numpy(), want)


# ---- image rows ------------------------------------------------------------------------------------------------------------------
def _byte_values(dtype):
    t = np.dtype(dtype).type
    v = [t(b) / t(255) for b in range(256)] + [t(0), t(1), np.nextafter(t(0), t(-1)), np.nextafter(t(1), t(2)), t(-0.25), t(1.5),
                                               t(np.nan), t(np.inf), t(-np.inf), t(0.5), np.nextafter(t(0.5), t(0)), t(1) / t(510)]
    return np.array(v, dtype)


@pytest.mark.parametrize('backend', BACKENDS)
def test_image_rows_every_layout_and_dtype(backend):
    from clslam_hip import ops
    device = use_backend(backend)
    rng = np.random.default_rng(6)
    h, w = 9, 31                                 # 279 pixels x 3 channels: every value of _byte_values in every channel
    assert [int(b) for b in ref.to_bytes(_byte_values(np.float32)[:256])] == list(range(256))       # b from fl32(b / 255)
    for dtype in (np.float32, np.float64):
        vals = _byte_values(dtype)
        hwc = np.stack([rng.permutation(np.resize(vals, h * w)) for _ in range(3)], -1).reshape(1, h, w, 3)
        got = ops.viz_compose([ops.viz_image_row(torch.from_numpy(hwc).to(device))], 1, h, w)[0].cpu().numpy()
        assert np.array_equal(got, ref.image_row(hwc[0])), dtype
        if dtype is np.float32:
            chw = np.ascontiguousarray(np.moveaxis(hwc, -1, 1))
            got = ops.viz_compose([ops.viz_image_row(torch.from_numpy(chw).to(device), chw=True)], 1, h, w)[0].cpu().numpy()
            assert np.array_equal(got, ref.image_row(chw[0], chw=True)) and np.array_equal(got, ref.image_row(hwc[0]))
    u8 = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    assert np.array_equal(ops.viz_compose([ops.viz_image_row(torch.from_numpy(u8).to(device))], 2, h, w).cpu().numpy(), u8)


# ---- trajectory ------------------------------------------------------------------------------------------------------------------
LIMS = dict(xlim=(0.0, 67.0), ylim=(0.0, 33.0))          # 33x67: one unit per pixel, y upwards


def _lines():
    """name -> (gt, pred) in the units of LIMS"""
    nan = np.nan
    return {
        'point': ([[10.5, 10.5]], None),
        'horizontal': ([[3.5, 8.5], [60.5, 8.5]], [[60.5, 20.5], [3.5, 20.5]]),
        'vertical': ([[5.5, 2.5], [5.5, 30.5]], [[40.5, 30.5], [40.5, 2.5]]),
        'diagonals': ([[2.5, 2.5], [30.5, 30.5]], [[30.5, 2.5], [2.5, 30.5]]),
        'shallow': ([[1.5, 3.5], [64.5, 12.5]], [[64.5, 15.5], [1.5, 6.5]]),
        'steep': ([[20.5, 1.5], [27.5, 31.5]], [[37.5, 31.5], [30.5, 1.5]]),
        'outside': ([[-50.0, -20.0], [-10.0, -5.0]], [[100.0, 50.0], [300.0, 40.0]]),
        'crossing_borders': ([[-20.0, 10.0], [90.0, 25.0]], [[30.0, -15.0], [41.0, 60.0], [-9.0, 16.0], [70.0, -3.0]]),
        'far_vertices': ([[1e9, 16.0], [-1e9, 17.0], [5.0, 1e9], [8.0, -1e9]], [[1e300, 1e300], [10.0, 10.0], [-1e300, 20.0]]),
        'nan_between': ([[2.0, 2.0], [20.0, 9.0], [nan, 5.0], [40.0, 20.0], [60.0, 30.0], [np.inf, 3.0]], [[nan, nan]]),
        'pred_over_gt': ([[30.5, 2.5], [30.5, 30.5], [5.0, 5.0], [60.0, 28.0]], [[5.5, 16.5], [60.5, 16.5], [60.0, 5.0], [5.0, 28.0]]),
        'empty_and_pair': (np.zeros((0, 2)), [[12.0, 3.0], [14.0, 30.0]]),
        'none': (None, None),
    }


def test_the_reference_clipping_is_the_brute_force_rule():
    """viz_reference visits only the k inside the row on the major axis; where every k can be walked it gives the same pixels"""
    for name, (gt, pred) in _lines().items():
        if name == 'far_vertices':
            continue
        for shape in ((1, 1), (3, 5), (33, 67)):
            a = ref.trajectory_row(gt, pred, shape, **LIMS)
            assert np.array_equal(a, ref.trajectory_row(gt, pred, shape, brute=True, **LIMS)), (name, shape)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (33, 67)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_trajectory_rows(backend, shape):
    from clslam_hip import ops
    device = use_backend(backend)
    drawn = 0
    for name, (gt, pred) in _lines().items():
        args = [None if v is None else torch.from_numpy(np.asarray(v, np.float64).reshape(-1, 2)).to(device) for v in (gt, pred)]
        got = ops.viz_compose([ops.viz_traj_row(args[0], args[1], **LIMS)], 1, *shape)[0].cpu().numpy()
        want = ref.trajectory_row(gt, pred, shape, **LIMS)
        assert np.array_equal(got, want), name
        drawn += int((want != 255).any(-1).sum())
        if name == 'pred_over_gt' and shape == (33, 67):
            both = ref.polyline_pixels(gt, *shape, **LIMS) & ref.polyline_pixels(pred, *shape, **LIMS)
            assert both and all(tuple(got[v, u]) == ref.PRED_COLOUR for u, v in both)
        if name in ('outside', 'none'):
            assert (got == 255).all()
    assert drawn > 0


@pytest.mark.parametrize('backend', BACKENDS)
def test_trajectory_in_the_reference_limits_and_a_long_polyline(backend):
    """the default window of utils.py:115-116 and more segments than one block has threads"""
    from clslam_hip import ops
    device = use_backend(backend)
    rng = np.random.default_rng(12)
    gt = np.cumsum(rng.normal(size=(700, 2)) * 2.0, 0) + [-150.0, 40.0]
    pred = gt + np.cumsum(rng.normal(size=gt.shape) * 0.2, 0)
    got = ops.viz_compose([ops.viz_traj_row(torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device))], 1, 33, 67)[0]
    want = ref.trajectory_row(gt, pred, (33, 67))
    assert np.array_equal(got.cpu().numpy(), want) and (want != 255).any()


# ---- narrow bands: rows wider than 1024 pixels -------------------------------------------------------------------------------------
WIDE_H = 9                                                 # no multiple of 7 or of 2: the last band of every width below 4097 is partial
WIDE = [(1024, 8), (1025, 7), (2731, 2), (4096, 2), (4097, 1), (8192, 1)]
WIDE_IDS = [f'w{w}' for w, _ in WIDE]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('w,band', WIDE, ids=WIDE_IDS)
def test_wide_rows_colour_and_image(backend, w, band):
    """clslam_viz_compose's `band = max(1, min(8, 8192 / w))` below 8, down to one pixel row, and viz_compose_kernel's
    `ylo = blockIdx.x * band`, `yhi = min(h, ylo + band)`: a colour row and an HWC float32 image row in one call, into the middle
    of a taller destination with wider rows; the bytes around the rectangle stay as they were.  Measured: at most 0.02 s a case
    on the CPU emulator, under 0.005 s on the MI355X."""
    from clslam_hip import ops
    device = use_backend(backend)
    assert max(1, min(8, 8192 // w)) == band and (band == 1 or WIDE_H % band)
    rng = np.random.default_rng(w)
    n, h = 2, WIDE_H
    depth = (rng.random((n, h, w)) * 30).astype(np.float32)
    depth[:, ::4, ::97] = np.nan
    image = rng.random((n, h, w, 3)).astype(np.float32)
    rr = np.array([[2.0, 20.0], [5.0, 25.0]], np.float32)
    before = rng.integers(0, 256, (n, 5 + 2 * h + 3, w + 8, 3), dtype=np.uint8)
    dst = torch.from_numpy(before.copy()).to(device)
    view = dst[:, :, 4:, :]                      # stride(1) = 3 (w + 8) > 3 w
    out = ops.viz_compose([ops.viz_cmap_row(torch.from_numpy(depth).to(device), torch.from_numpy(rr).to(device)),
                           ops.viz_image_row(torch.from_numpy(image).to(device))], n, h, w, dst=view, row0=5)
    assert out.data_ptr() == view.data_ptr()
    want = before.copy()
    for i in range(n):
        want[i, 5:5 + h, 4:4 + w] = ref.colorize(depth[i], rr[i, 0], rr[i, 1], 'magma_r')
        want[i, 5 + h:5 + 2 * h, 4:4 + w] = ref.image_row(image[i])
    assert np.array_equal(dst.cpu().numpy(), want)


def _wide_lines(w):
    """(gt, pred) in a window of one unit per pixel, xlim = (0, w), ylim = (0, 9).  gt: a shallow x-major segment across the full
    width (w candidate k in every band: the bisection, also where a band is one pixel row), then, after a NaN vertex, a steep
    y-major one through every band.  pred: a polyline that crosses both, enters from beyond the left border and leaves beyond the
    right one."""
    nan = np.nan
    gt = [[0.5, 1.5], [w - 0.5, 7.5], [nan, nan], [w // 3 + 0.5, 0.5], [w // 3 + 3.5, 8.5]]
    pred = [[-100.5, 8.2], [w // 2 + 0.5, 0.7], [w // 2 + 2.5, 8.5], [w + 100.5, 1.2], [0.5, 7.5], [w - 0.5, 1.5]]
    return np.asarray(gt, np.float64), np.asarray(pred, np.float64)


def test_the_reference_clipping_is_the_brute_force_rule_on_a_wide_row():
    """the premise of test_wide_rows_trajectory: on a 9 x 1025 row, where every k of every segment can still be walked, the
    reference's clipping gives the pixels of the brute-force rule, for the very lines those cases draw"""
    gt, pred = _wide_lines(1025)
    lims = dict(xlim=(0.0, 1025.0), ylim=(0.0, float(WIDE_H)))
    a = ref.trajectory_row(gt, pred, (WIDE_H, 1025), **lims)
    assert np.array_equal(a, ref.trajectory_row(gt, pred, (WIDE_H, 1025), brute=True, **lims)) and (a != 255).any()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('w,band', WIDE, ids=WIDE_IDS)
def test_wide_rows_trajectory(backend, w, band):
    """vz_draw_segment's clip against a band of `band < 8` pixel rows (`ylo`, `yhi` from viz_compose_kernel), with `khi - klo >=
    kVzShortSegment` (the bisection) in a band of one row at w > 4096.  Measured: at most 0.13 s a case on the CPU emulator
    (most of it the reference's Python loop), 0.03 s on the MI355X."""
    from clslam_hip import ops
    device = use_backend(backend)
    assert max(1, min(8, 8192 // w)) == band
    h = WIDE_H
    gt, pred = _wide_lines(w)
    lims = dict(xlim=(0.0, float(w)), ylim=(0.0, float(h)))
    want = ref.trajectory_row(gt, pred, (h, w), **lims)
    shallow = ref.polyline_pixels(gt[:2], h, w, **lims)
    steep = ref.polyline_pixels(gt[3:], h, w, **lims)
    assert len(shallow) == w and len({v for _, v in shallow}) == 7 and len(steep) == h == len({v for _, v in steep})
    both = ref.polyline_pixels(gt, h, w, **lims) & ref.polyline_pixels(pred, h, w, **lims)
    assert both and (want == np.array(ref.GT_COLOUR, np.uint8)).all(-1).any(axis=1).all()        # gt shows in every pixel row
    row = ops.viz_traj_row(torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device), **lims)
    got = ops.viz_compose([row], 1, h, w)[0]
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    assert all(tuple(got[v, u]) == ref.PRED_COLOUR for u, v in both)


@pytest.mark.parametrize('backend', BACKENDS)
def test_compose_refuses_a_row_wider_than_8192(backend):
    """the width at which `8192 / w` would be 0 is refused, by the binding, which checks first, with '1 <= w <= 8192'"""
    from clslam_hip import ops
    from clslam_hip._lib import ClslamError
    device = use_backend(backend)
    plane = torch.zeros((1, 1, 8193), device=device)
    rng = torch.zeros((1, 2), device=device)
    with pytest.raises(ClslamError, match='1 <= w <= 8192'):
        ops.viz_compose([ops.viz_cmap_row(plane, rng)], 1, 1, 8193)
    assert ops.viz_compose([ops.viz_cmap_row(torch.zeros((1, 1, 8192), device=device), rng)], 1, 1, 8192).shape == (1, 1, 8192, 3)


@pytest.mark.parametrize('backend', BACKENDS)
def test_compose_refuses_bad_arguments(backend):
    from clslam_hip import ops
    from clslam_hip._lib import ClslamError
    device = use_backend(backend)
    plane = torch.zeros((1, 4, 6), device=device)
    rng = torch.zeros((1, 2), device=device)
    with pytest.raises(ClslamError, match='cmap must be'):
        ops.viz_compose([ops.viz_cmap_row(plane, rng, 'viridis')], 1, 4, 6)
    with pytest.raises(ClslamError, match='colour row must be'):
        ops.viz_compose([ops.viz_cmap_row(plane, rng)], 1, 4, 7)
    with pytest.raises(ClslamError, match='rows'):
        ops.viz_compose([ops.viz_cmap_row(plane, rng)] * 5, 1, 4, 6)
    with pytest.raises(ClslamError, match='dst must be'):
        ops.viz_compose([ops.viz_cmap_row(plane, rng)], 1, 4, 6, dst=torch.zeros((1, 4, 5, 3), dtype=torch.uint8, device=device))
    with pytest.raises(ClslamError, match='distinct ends'):
        ops.viz_compose([ops.viz_traj_row(None, None, xlim=(1.0, 1.0))], 1, 4, 6)
    with pytest.raises(ClslamError, match='float64'):
        ops.viz_compose([ops.viz_traj_row(torch.zeros((2, 2), device=device), None)], 1, 4, 6)


def test_the_symbols_are_listed():
    from clslam_hip import _lib
    assert {'clslam_viz_range', 'clslam_viz_range_scratch', 'clslam_viz_compose'} <= set(_lib.exported_symbols())
