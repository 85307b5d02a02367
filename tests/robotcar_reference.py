"""numpy / scipy restatement of the RobotCar raw-frame path (datasets/robotcar.py:522-548 _load_image, :617-642
CameraModel.undistort, and colour_demosaicing.demosaicing_CFA_Bayer_bilinear, which is not installed here and is restated from
its published definition: masks, then one scipy.ndimage.convolve per channel with the default border mode)."""
import numpy as np
from scipy.ndimage import convolve, map_coordinates

PATTERNS = ('rggb', 'bggr', 'grbg', 'gbrg')
H_G = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], dtype=np.float64) / 4
H_RB = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.float64) / 4


def masks(shape, pattern):
    m = {c: np.zeros(shape, dtype=np.float64) for c in 'rgb'}
    for c, (y, x) in zip(pattern.lower(), [(0, 0), (0, 1), (1, 0), (1, 1)]):
        m[c][y::2, x::2] = 1
    return m['r'], m['g'], m['b']


def demosaic(cfa, pattern):
    """cfa (H,W) -> (H,W,3) float64"""
    cfa = np.asarray(cfa, dtype=np.float64)
    r_m, g_m, b_m = masks(cfa.shape, pattern)
    return np.stack([convolve(cfa * r_m, H_RB), convolve(cfa * g_m, H_G), convolve(cfa * b_m, H_RB)], axis=-1)


def undistort_f64(image, lut):
    """image (H,W,C) of any dtype, lut (2,H,W) (row, col) -> (H,W,C) float64: one map_coordinates(order=1) per channel"""
    return np.stack([map_coordinates(image[:, :, c], lut, order=1, output=np.float64) for c in range(image.shape[2])], axis=-1)


def to_u8(x):
    """truncation toward zero, then the low byte (astype(np.uint8) of a value above 255 is platform-defined)"""
    return (np.trunc(x).astype(np.int64) & 255).astype(np.uint8)


def undistort(image, lut):
    """CameraModel.undistort: the image's dtype back"""
    out = undistort_f64(image, lut)
    return to_u8(out) if image.dtype == np.uint8 else out.astype(image.dtype)


def load_image(cfa, lut, pattern):
    """_load_image(path, model) on a decoded mosaic: (H,W) uint8 -> (H,W,3) uint8"""
    return to_u8(undistort_f64(demosaic(cfa, pattern), lut))


def make_lut(H, W, seed=0, k1=0.08, shift=0.37):
    """A mild radial model, (2,H,W) float64 (row, col): fractional coordinates everywhere, the corners pushed OUTSIDE the image
    (k1 > 0 magnifies with the radius), the centre inside.  Returns (lut, share of samples outside)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    cy, cx = (H - 1) / 2, (W - 1) / 2
    ny, nx = (yy - cy) / max(cy, 1.0), (xx - cx) / max(cx, 1.0)
    f = 1 + k1 * (ny * ny + nx * nx)
    lut = np.stack([cy + (yy - cy) * f + shift, cx + (xx - cx) * f - shift]) + rng.uniform(-0.25, 0.25, (2, H, W))
    outside = (lut[0] < 0) | (lut[0] > H - 1) | (lut[1] < 0) | (lut[1] > W - 1)
    return lut, float(outside.mean())


def edge_lut(H, W, seed=0):
    """make_lut with the special coordinates written over its first entries: integers, 0 and H-1 / W-1 exactly, a hair outside on
    either side, -0.5, and x.5 midpoints (as many as fit; every one needs a pixel)"""
    lut, _ = make_lut(H, W, seed)
    r, c = lut[0].reshape(-1), lut[1].reshape(-1)
    special = [(0.0, 0.0), (H - 1.0, W - 1.0), (-1e-12, 0.0), (0.5, 0.5),          # the four a 2x2 image has room for
               (0.0, W - 1.0), (H - 1.0, 0.0), (0.0, -1e-12), (H - 1 + 1e-12, 0.0),
               (0.0, W - 1 + 1e-12), (-0.5, 0.0), (0.0, -0.5), (H - 1.0, 0.5), (0.5, W - 1.0),
               (float(H // 2), float(W // 2)), (float(H // 2), W // 2 - 0.5), (H // 2 - 0.5, float(W // 2)), (1.0, 0.25), (0.75, 1.0)]
    n = min(len(special), r.size)
    at = np.linspace(0, r.size - 1, n).astype(int) if r.size > n else np.arange(n)
    for i, (a, b) in zip(at, special[:n]):
        r[i], c[i] = a, b
    return lut
