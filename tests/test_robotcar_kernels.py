"""csrc/robotcar.hip one kernel at a time against the numpy / scipy restatement (tests/robotcar_reference.py): EXACT equality, the
float64 results bit for bit and the uint8 results byte for byte.

Sizes: 2x2 (every tap is border), 6x10, 37x67 (odd: the mosaic's last row and column have no partner), and 5x259 -- the kernels'
blocks are runs of BLOCK = 256 consecutive outputs of the flattened image (one direction only), so a width of BLOCK + 3 puts a block
edge inside every row, at another column each time, and leaves a partial last block (for pixels, for 3 and for 2 channels).
960x1280 (a RobotCar frame) runs through the fused kernel only.  N = 1 and N = 3: one table, frames not mixed."""
import numpy as np
import pytest
import torch

import robotcar_reference as ref
from emu_util import BACKENDS, use_backend

BLOCK = 256                     # kRcThreads
SIZES = [(2, 2), (6, 10), (37, 67), (5, BLOCK + 3)]
_CACHE = {}


def _mosaic(n, H, W, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)            # a copy: the cached references are read-only


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
        for a in (_CACHE[key] if isinstance(_CACHE[key], tuple) else (_CACHE[key],)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _CACHE[key]


def _guard(lut, expected):
    """a pass-through or an all-zero result must not pass: the table samples inside and outside, the reference is not constant"""
    H, W = lut.shape[1:]
    inside = (lut[0] >= 0) & (lut[0] <= H - 1) & (lut[1] >= 0) & (lut[1] <= W - 1)
    assert inside.any() and not inside.all()
    assert np.unique(expected).size > 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- demosaic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('pattern', ref.PATTERNS)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_demosaic_matches_the_reference_bit_for_bit(backend, size, n, pattern):
    from clslam_hip import ops
    device = use_backend(backend)
    cfa = _mosaic(n, *size)
    want = _cached(('dm', size, n, pattern), lambda: np.stack([ref.demosaic(f, pattern) for f in cfa]))
    got = ops.demosaic_bilinear(_dev(cfa, device), pattern).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.unique(want).size > 1
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize('backend', BACKENDS)
def test_demosaic_hand_made_4x4(backend):
    """rggb: R at (even, even), B at (odd, odd).  The four interior pixels, by hand:
       (1,1) is a B site: R = mean of its 4 diagonal R, G = mean of its 4 edge G, B = itself; (1,2) is a G site in a B row: R = mean
       of the R above and below, B = mean of the B left and right; and so on."""
    from clslam_hip import ops
    device = use_backend(backend)
    cfa = np.array([[10, 20, 30, 40],
                    [50, 60, 70, 80],
                    [90, 100, 110, 120],
                    [130, 140, 150, 160]], dtype=np.uint8)
    got = ops.demosaic_bilinear(_dev(cfa[None], device), 'rggb').cpu().numpy()[0]
    want = {(1, 1): ((10 + 30 + 90 + 110) / 4, (20 + 50 + 70 + 100) / 4, 60.0),
            (1, 2): ((30 + 110) / 2, 70.0, (60 + 80) / 2),
            (2, 1): ((90 + 110) / 2, 100.0, (60 + 140) / 2),
            (2, 2): (110.0, (70 + 100 + 120 + 150) / 4, (60 + 80 + 140 + 160) / 4)}
    for (y, x), rgb in want.items():
        assert tuple(got[y, x]) == rgb, (y, x)
    assert np.array_equal(got, ref.demosaic(cfa, 'rggb'))
    assert np.array_equal(got[1:3, 1:3], ref.demosaic(np.pad(cfa, 1, mode='edge'), 'bggr')[2:4, 2:4])    # interior: no border rule


# ---- undistort -------------------------------------------------------------------------------------------------------------
def _undistort_case(size, n, kind):
    H, W = size
    lut = ref.edge_lut(H, W, seed=3)
    rng = np.random.default_rng(5)
    if kind == 'f64':
        image = rng.uniform(0, 600, (n, H, W, 3))
    elif kind == 'u8':
        image = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    elif kind == 'u8c2':
        image = rng.integers(0, 256, (n, H, W, 2), dtype=np.uint8)
    else:
        image = np.full((n, H, W, 3), 255, dtype=np.uint8)
    return lut, image, np.stack([ref.undistort(f, lut) for f in image])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind', ['f64', 'u8', 'u8c2', 'flat255'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_undistort_equals_scipy(backend, size, n, kind):
    from clslam_hip import ops
    device = use_backend(backend)
    lut, image, want = _cached(('ud', size, n, kind), lambda: _undistort_case(size, n, kind))
    _guard(lut, want)
    got = ops.undistort_lut(_dev(image, device), _dev(lut, device)).cpu().numpy()
    assert got.dtype == image.dtype and got.shape == want.shape
    if kind == 'f64':
        assert np.array_equal(_bits(got), _bits(want))
    else:
        assert np.array_equal(got, want)


def test_scipy_lands_just_under_255_on_a_flat_image():
    """the weights of a sample do not always add up to 1 in floating point: scipy itself gives 254.99999999999997 -> 254 at some
    pixels of a flat 255 image, and the kernel reproduces those pixels (test_undistort_equals_scipy[flat255]) instead of mending them"""
    lut, _, want = _cached(('ud', (37, 67), 1, 'flat255'), lambda: _undistort_case((37, 67), 1, 'flat255'))
    assert (want == 254).any() and (want == 255).any()


def test_edge_lut_holds_every_special_coordinate():
    H, W = 37, 67
    lut = ref.edge_lut(H, W, seed=3)
    r, c = lut[0].ravel(), lut[1].ravel()
    pairs = set(zip(r.tolist(), c.tolist()))
    for p in [(0.0, 0.0), (H - 1.0, W - 1.0), (-1e-12, 0.0), (H - 1 + 1e-12, 0.0), (0.0, W - 1 + 1e-12), (-0.5, 0.0), (0.5, 0.5),
              (float(H // 2), float(W // 2)), (H // 2 - 0.5, float(W // 2))]:
        assert p in pairs, p
    assert 0.02 < ref.make_lut(H, W, seed=3)[1] < 0.5


# ---- fused -----------------------------------------------------------------------------------------------------------------
def _fused_case(size, n, pattern):
    H, W = size
    lut = ref.edge_lut(H, W, seed=7)
    cfa = _mosaic(n, H, W, seed=9)
    return lut, cfa, np.stack([ref.load_image(f, lut, pattern) for f in cfa])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('pattern', ['gbrg', 'rggb'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_rectify_equals_the_reference_and_the_two_kernels(backend, size, n, pattern):
    from clslam_hip import ops
    device = use_backend(backend)
    lut, cfa, want = _cached(('fu', size, n, pattern), lambda: _fused_case(size, n, pattern))
    _guard(lut, want)
    d_cfa, d_lut = _dev(cfa, device), _dev(lut, device)
    got = ops.robotcar_rectify(d_cfa, d_lut, pattern).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    two = ops.undistort_lut(ops.demosaic_bilinear(d_cfa, pattern), d_lut).cpu().numpy()
    assert np.array_equal(got, ref.to_u8(two))
    if n > 1:                                                            # one table for every frame, frames not mixed
        for i in range(n):
            assert np.array_equal(ops.robotcar_rectify(d_cfa[i:i + 1], d_lut, pattern).cpu().numpy()[0], want[i])


@pytest.mark.parametrize('backend', BACKENDS)
def test_rectify_full_frame(backend):
    from clslam_hip import ops
    device = use_backend(backend)
    lut, cfa, want = _cached(('fu', (960, 1280), 1, 'gbrg'), lambda: _fused_case((960, 1280), 1, 'gbrg'))
    _guard(lut, want)
    got = ops.robotcar_rectify(_dev(cfa, device), _dev(lut, device), 'gbrg').cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize('backend', BACKENDS)
def test_rectify_writes_into_an_unaligned_output(backend):
    """H * W odd and frame 1 of 2: the block's run starts off a 4-byte boundary, the byte-wise store path"""
    from clslam_hip import ops
    device = use_backend(backend)
    lut, cfa, want = _cached(('fu', (37, 67), 3, 'gbrg'), lambda: _fused_case((37, 67), 3, 'gbrg'))
    buf = torch.full((3 * 37 * 67 * 3 + 2,), 7, dtype=torch.uint8, device=device)
    out = buf[1:-1].view(3, 37, 67, 3)
    ops.robotcar_rectify(_dev(cfa, device), _dev(lut, device), 'gbrg', out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert int(buf[0]) == 7 and int(buf[-1]) == 7


# ---- errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_bad_arguments_raise_before_a_launch(backend):
    from clslam_hip import ops
    from clslam_hip._lib import ClslamError
    device = use_backend(backend)
    other = torch.device('meta')
    H, W = 6, 10
    cfa = _dev(_mosaic(1, H, W), device)
    rgb = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=device)
    lut = _dev(ref.make_lut(H, W)[0], device)
    with pytest.raises(ClslamError, match='lut must be'):
        ops.undistort_lut(rgb, _dev(ref.make_lut(H, W + 1)[0], device))
    with pytest.raises(ClslamError, match='lut must be'):
        ops.robotcar_rectify(cfa, lut[:, :, :-1], 'gbrg')
    with pytest.raises(ClslamError, match='rank 4'):
        ops.undistort_lut(rgb[0, :, :, 0], lut)
    with pytest.raises(ValueError, match='pattern'):
        ops.demosaic_bilinear(cfa, 'rgbg')
    with pytest.raises(ValueError, match='pattern'):
        ops.robotcar_rectify(cfa, lut, 'bayer')
    with pytest.raises(ClslamError, match='dtype'):
        ops.demosaic_bilinear(cfa.float(), 'rggb')
    with pytest.raises(ClslamError, match='dtype'):
        ops.undistort_lut(rgb.float(), lut)
    with pytest.raises(ClslamError, match='lut must be'):
        ops.undistort_lut(rgb, lut.float())
    with pytest.raises(ClslamError, match='lut on'):
        ops.undistort_lut(rgb, lut.to(other))
    with pytest.raises(ClslamError, match='lut on'):
        ops.robotcar_rectify(cfa, lut.to(other), 'gbrg')
    with pytest.raises(ClslamError, match='out must be'):
        ops.robotcar_rectify(cfa, lut, 'gbrg', out=torch.zeros(1, H, W, 3, dtype=torch.uint8, device=other))


def test_abi_is_114():
    from clslam_hip import _lib
    assert _lib.ABI_VERSION == 114
    assert {'clslam_demosaic_bilinear', 'clslam_undistort_lut', 'clslam_robotcar_rectify'} <= set(_lib.exported_symbols())
