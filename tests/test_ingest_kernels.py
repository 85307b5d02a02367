"""The ten kernels of cl-slam_amd/csrc/ingest.hip one at a time, at the sizes where their launches change: past every grid cap
(a second iteration of each grid-stride loop), across the 64-block cap of the gray / luminance sums, on every alignment path of
the frame store, and on the branches the pipeline tests do not reach (clip of the resize, 1 and 4 channels, one resize axis
alone, the u8 contrast mean at an exact half, alpha exactly 0 and 1, invalid slots next to valid ones, a mixed `aug` table).

References (tests/ingest_reference.py, oracle/resize.py, oracle/jitter.py, oracle/jitter_tensor.py):
  * integer kernels (resize, ToTensor, u8 jitter, store_pack): bit-exact.
  * float jitter and frame-store gather, in two steps.  The test owns the `partial` scratch, pre-filled with NaN.  (1) Every
    partial is held to the float64 sum over the documented partition (block b of nblk takes the pixels
    b * 256 + t + k * nblk * 256) within (adds per thread + 8) * 2^-24 * sum |term| -- derived, see
    ingest_reference.partial_bound.  (2) The contrast mean is formed from the OBSERVED partials exactly as the apply kernel
    forms it (sequential fp32 sum, / f32(hw)) and injected into oracle.jitter_tensor's chain: the output must then be BITWISE
    that chain, ops behind contrast included.  Nothing is compared with another kernel of the library.
  * a record that names contrast twice is held to the kernels' documented contract: one mean per image, of the gray value in
    front of the FIRST contrast op, used by both.

Cost.  The emulator runs every case of this file in well under 10 s on the build host (slowest: the 2 x 1030 x 1100 -> 1024
resize with its numpy oracle, 1.4 s; the 1030 x 1020 u8 jitter, 0.7 s), so no grid-cap case is hip-only: all cases run on both
backends.  On gfx950 the slowest case takes 0.25 s.

Clip shares (test_resize_clip_is_reached, from the oracle's accumulator without the clip, 33 x 40 step edges + period-3
checkerboard): 40 -> 67 horizontally 15.9 % below 0 and 13.2 % above 255; 33 -> 55 vertically 11.8 % below 0, 9.1 % above 255.

Measured (emu | hip): the largest partial error as a fraction of the derived bound is 0.17 | 0.17 (f32 jitter, hw = 65536 /
65537) and 0.12 | 0.11 (gather, 192 x 640).  Every chain is bitwise the injected-mean reference on both backends, ops behind
contrast included: the 2e-6 of tests/test_replay_ingest.py is the summation order of torch.mean and nothing else.

Failures met while writing these tests: none against the kernels.  ingest.hip is unchanged.

One-line mutations of a scratch copy of ingest.hip (CPU emulator, never committed) and the new tests that fail:
  (a) store_pack_kernel's vector loop runs one pass only (`i += gridDim.x * 256` -> `i = nvec`)
          test_store_pack_counts[368640], [524295], test_store_pack_planes
  (b) store_gather_sum_kernel: stride `g.nblk * 256` -> `gridDim.x * 256`
          test_gather_slots_rows_and_records, test_gather_real_size, test_gather_mixed_aug_table_and_no_jitter,
          test_gather_unaligned_rows (partials of the levels with fewer blocks than level 0)
  (c) `partial` index `(li * n_images + img) * 64` -> `(img * n_images + li) * 64`, in the sum kernel alone or in both kernels
          the same four (a partial outside [level][image][64] or a wrong one; the scratch is max(levels, images)^2 x 64 so
          that the swapped index stays inside the test's allocation)
  (d) `m / (float)hw` -> `m / (nblk * 256 * k)`
          in jitter_f32_apply_kernel: test_jitter_f32_sizes[1, 63, 255, 257, 1025, 65537, 122880, 131372],
          test_jitter_f32_records[1025], [122880], test_jitter_f32_hue_at_the_wrap
          in store_gather_apply_kernel: all test_gather_* that jitter, test_gather_apply_grid_stride among them
  (e) jitter_contrast_pos returns the last contrast position instead of the first
          test_jitter_f32_records[1025], [122880] (the record [1, 0, 1, 2]: it differs from the original for no other record)
  (f) `acc >> 22` without the clip
          test_resize_clip_is_reached, test_resize_one_pass_alone (6 cases), test_resize_channels[1, 3, 4],
          test_resize_grid_stride
  (g) `c < C` -> `c < 3` in the accumulation of the resize
          test_resize_channels[4]
  (h) `+ 0.5` dropped from the u8 contrast mean
          test_jitter_u8_contrast_mean_at_an_exact_half[2, 6, 254, 258], test_jitter_u8_luminance_sum (7 sizes),
          test_jitter_u8_grid_stride, test_jitter_u8_ping_pong
  (i) `alpha <= 1.f` -> `alpha < 1.f`
          NO test fails, and none can: the mutation is equivalent.  It moves alpha == 1 alone from the truncating to the
          clipping branch; there t = other + 1 * (v - other) with integers below 2^8 in float32, which is v exactly, and
          both branches return v for 0 <= v <= 255.  (The same holds at alpha == 0, where t = other.)  Truncation and clip
          differ only for t < 0 or t >= 256, which no alpha in [0, 1] produces.  test_jitter_u8_blend_lattice runs alpha = 0,
          1 and the next double above 1 over the whole lattice all the same.
  (j) `d.aug[g.table]` -> `d.aug[0]` (both uses, or the flag alone)
          test_gather_mixed_aug_table_and_no_jitter; with both uses also test_gather_slots_rows_and_records,
          test_gather_real_size, test_gather_unaligned_rows
  (k) the `slot >= d.capacity` test removed
          test_gather_slots_rows_and_records (the row of the sample with slot == capacity loses its -7 prefill; the store is
          allocated one slot longer than it declares, nothing is read out of bounds)
  (l) `if (hh != 0.f && hh < 0.f)` -> `if (hh <= 0.f)`
          NO test fails, and none can: the mutation is equivalent.  It turns hh == 0 into hh == 1; then h6 = 6, floor 6, f = 0,
          i = 6 % 6 = 0 -- the f and i of hh == 0 -- so p, q, t and the selected triple are the same floats.
          test_jitter_f32_hue_at_the_wrap runs hh == 0 (gray pixels, factor 0), hh < 0 and the wrap past 1.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ingest_reference as R
from clslam_hip import _lib, ingest
from clslam_hip.ops import _stream
from emu_util import BACKENDS, use_backend
from oracle import jitter as oj
from oracle import resize as rz

GUARD = 64          # bytes behind a destination, pre-filled with 0xA5


def _lib_call(name, *args):
    _lib.get_lib().call(name, *args)


# ======================================================================================================================
# 1. resize_pass_u8_kernel, u8_to_planar_kernel
def _plan(in_size, out_size, dev):
    """the library's host-side tap plan, held to oracle.resize.lanczos_plan -> (bounds, coeffs, ksize) on dev"""
    lib = _lib.get_lib()
    ksize = lib.cdll.clslam_lanczos_ksize(in_size, out_size)
    bounds = torch.empty(out_size, 2, dtype=torch.int32)
    coeffs = torch.empty(out_size, ksize, dtype=torch.int32)
    lib.call('clslam_lanczos_plan', in_size, out_size, bounds.data_ptr(), coeffs.data_ptr())
    rb, rk = rz.lanczos_plan(in_size, out_size)
    assert rk.shape[1] == ksize and np.array_equal(bounds.numpy(), rb) and np.array_equal(coeffs.numpy(), rk)
    return bounds.to(dev), coeffs.to(dev), ksize


def _resize_pass(dev, img, out_size, axis, planar):
    """img (N,h,w,C) uint8 numpy -> (out uint8 numpy, planar float tensor or None, guard bytes) through ONE pass of the C entry"""
    N, h, w, ch = img.shape
    oh, ow = (out_size, w) if axis == 0 else (h, out_size)
    b, k, ks = _plan(h if axis == 0 else w, out_size, dev)
    src = torch.from_numpy(img).to(dev)
    n = N * oh * ow * ch
    dst = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    pl = torch.full((N * ch * oh * ow + 16,), -7.0, device=dev) if planar else None
    _lib_call('clslam_resize_pass_u8', src.data_ptr(), dst.data_ptr(), None if pl is None else pl.data_ptr(), b.data_ptr(),
              k.data_ptr(), ks, N, h, w, ch, out_size, axis, _stream(src))
    dst = dst.cpu()
    assert bool((dst[n:] == 0xA5).all()), 'bytes behind the last pixel were written'
    if pl is not None:
        pl = pl.cpu()
        assert bool((pl[-16:] == -7.0).all())
        pl = pl[:-16].view(N, ch, oh, ow)
    return dst[:n].view(N, oh, ow, ch).numpy(), pl


def _check_pass(dev, img, out_size, axis, planar):
    want = rz._resample_axis(img, out_size, 1 if axis == 0 else 2)
    got, pl = _resize_pass(dev, img, out_size, axis, planar)
    assert np.array_equal(got, want), (img.shape, out_size, axis, int((got != want).sum()))
    if planar:
        assert torch.equal(pl, R.to_planar(want)), (img.shape, out_size, axis)


PAIRS = [(64, 32), (53, 20), (20, 33), (37, 37), (9, 1), (1, 5)]


@pytest.mark.parametrize('axis', [1, 0])
@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: f'{p[0]}to{p[1]}')
@pytest.mark.parametrize('backend', BACKENDS)
def test_resize_one_pass_alone(backend, pair, axis):
    """one pass along one axis (the wrappers always run the horizontal one first), the other axis at 7 and 33, with and
    without the fused ToTensor; 37 -> 37 runs the identity plan the wrappers never launch"""
    dev = use_backend(backend)
    n_in, n_out = pair
    rng = np.random.default_rng(100 * n_in + n_out + axis)
    for other in (7, 33):
        shape = (2, other, n_in, 3) if axis == 1 else (2, n_in, other, 3)
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        for planar in (False, True):
            _check_pass(dev, img, n_out, axis, planar)


@pytest.mark.parametrize('ch', [1, 3, 4])
@pytest.mark.parametrize('backend', BACKENDS)
def test_resize_channels(backend, ch):
    """1, 3 and 4 channels, batch 3 of different images, both axes; the 64 bytes behind the destination stay 0xA5 (checked by
    _resize_pass for every call of this file) -- a loop over 4 channels instead of C writes them"""
    dev = use_backend(backend)
    rng = np.random.default_rng(ch)
    for axis, shape in ((1, (3, 7, 53, ch)), (0, (3, 53, 7, ch))):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert not np.array_equal(img[0], img[1]) and not np.array_equal(img[1], img[2])
        _check_pass(dev, img, 20, axis, True)
        _check_pass(dev, img, 77, axis, False)
    flat = rng.integers(0, 256, (3, 5, 9, ch), dtype=np.uint8)
    got = ingest.to_tensor(torch.from_numpy(flat).to(dev)).cpu()
    assert torch.equal(got, R.to_planar(flat))


def _clip_images():
    """0 / 255 step edges (runs of 5 and 7) and a 0 / 255 checkerboard of period 3 (two off, one on), 33 x 40"""
    x = np.arange(40)
    y = np.arange(33)[:, None]
    steps = np.where((x // 5 + y // 7) % 2 == 0, 0, 255) + 0 * y
    checker = np.where((x % 3 == 0) ^ (y % 3 == 0), 255, 0)
    return np.stack([np.repeat(im[..., None], 3, -1) for im in (steps, checker)]).astype(np.uint8)


@pytest.mark.parametrize('backend', BACKENDS)
def test_resize_clip_is_reached(backend):
    """LANCZOS overshoot on both sides: before the kernel is asked, the oracle's accumulator is recomputed WITHOUT the clip and
    at least 1 % of the outputs lie below 0 and at least 1 % above 255.  Measured: 40 -> 67 horizontally 15.9 % / 13.2 %,
    33 -> 55 vertically 11.8 % / 9.1 %."""
    dev = use_backend(backend)
    img = _clip_images()
    for axis, out_size in ((1, 67), (0, 55)):
        raw = R.resample_axis_raw(img, out_size, 1 if axis == 0 else 2)
        low, high = float((raw < 0).mean()), float((raw > 255).mean())
        print(f'clip axis {axis} -> {out_size}: {100 * low:.1f} % below 0, {100 * high:.1f} % above 255')
        assert low >= 0.01 and high >= 0.01, (axis, low, high)
        _check_pass(dev, img, out_size, axis, True)


@pytest.mark.parametrize('backend', BACKENDS)
def test_resize_grid_stride(backend):
    """more output pixels than 8192 blocks x 256 threads: batch 2 of 1030 x 1100 -> 1030 x 1024 (2109440 pixels), and ToTensor
    of 1030 x 2050 x 3 (2111500)."""
    dev = use_backend(backend)
    rng = np.random.default_rng(8192)
    img = rng.integers(0, 256, (2, 1030, 1100, 3), dtype=np.uint8)
    assert 2 * 1030 * 1024 > 8192 * 256
    _check_pass(dev, img, 1024, 1, False)
    flat = rng.integers(0, 256, (1, 1030, 2050, 3), dtype=np.uint8)
    assert 1030 * 2050 > 8192 * 256
    assert torch.equal(ingest.to_tensor(torch.from_numpy(flat).to(dev)).cpu(), R.to_planar(flat))


@pytest.mark.parametrize('backend', BACKENDS)
def test_resize_argument_checks(backend):
    dev = use_backend(backend)
    b, k, ks = _plan(9, 4, dev)
    src = torch.zeros(3 * 9 * 5, dtype=torch.uint8, device=dev)
    dst = torch.full((256,), 0xA5, dtype=torch.uint8, device=dev)

    def call(batch=1, in_h=3, in_w=9, ch=3, out=4, axis=1, ksize=ks):
        _lib_call('clslam_resize_pass_u8', src.data_ptr(), dst.data_ptr(), None, b.data_ptr(), k.data_ptr(), ksize, batch, in_h, in_w,
                  ch, out, axis, _stream(src))
    for bad in (dict(ch=5), dict(ch=0), dict(axis=2), dict(ksize=0), dict(batch=1 << 20, in_h=1 << 11, in_w=9, out=1)):
        with pytest.raises(_lib.ClslamError):
            call(**bad)
    with pytest.raises(_lib.ClslamError):          # ToTensor: 2^31 pixels, checked before the launch
        _lib_call('clslam_u8_to_planar_f32', src.data_ptr(), torch.zeros(4, device=dev).data_ptr(), 1 << 11, 1 << 10, 1 << 10, 3, _stream(src))
    call(batch=0)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    call()
    assert not bool((dst.cpu()[:3 * 4 * 3] == 0xA5).all()) and bool((dst.cpu()[3 * 4 * 3:] == 0xA5).all())


# ======================================================================================================================
# 2. u8 colour jitter

# every (r, g, b) over these 41 values: both ends of the byte range, the middle, and a stride of 7 in between
LATTICE = [0, 1, 2, 3, 5, 12, 19, 26, 33, 40, 47, 54, 61, 68, 75, 82, 89, 96, 103, 110, 117, 124, 126, 127, 128, 129, 131, 138,
           145, 152, 159, 166, 173, 180, 187, 194, 201, 252, 253, 254, 255]
U8_FACTORS = [0.0, 0.5, 0.8, 1.0, float(np.nextafter(1.0, 2.0)), 1.2, 2.0]
HUE_FACTORS = [-0.5, -0.1, -1 / 255, 0.0, 1 / 255, 0.037, 0.1, 0.5]


def _lattice_image():
    """the 41^3 = 68921 pixels as one ragged image of 7 rows x 9846 (the last pixel repeated once)"""
    assert len(LATTICE) == 41 and sorted(set(LATTICE)) == LATTICE
    v = np.array(LATTICE, np.uint8)
    px = np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(-1, 3)
    px = np.concatenate([px, px[-1:]])
    assert px.shape[0] == 7 * 9846
    return px.reshape(1, 7, 9846, 3)


def _jitter_u8(dev, img, order, factors, lsum=None):
    """img (N,h,w,3) uint8 numpy through clslam_color_jitter_u8 -> (dst numpy, src after the call, lsum tensor)"""
    N, h, w, _ = img.shape
    src = torch.from_numpy(img).to(dev)
    n = N * h * w * 3
    dst = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    scratch = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    if lsum is None:
        lsum = torch.zeros(N, dtype=torch.int64, device=dev)
    order_c = (C.c_int * max(len(order), 1))(*[int(o) for o in order])
    factors_c = (C.c_double * 4)(*[float(f) for f in factors])
    _lib_call('clslam_color_jitter_u8', src.data_ptr(), dst.data_ptr(), scratch.data_ptr(), lsum.data_ptr(), N, h, w, order_c,
              len(order), factors_c, _stream(src))
    dst, scratch = dst.cpu(), scratch.cpu()
    assert bool((dst[n:] == 0xA5).all()) and bool((scratch[n:] == 0x5A).all())
    return dst[:n].view(N, h, w, 3).numpy(), src.cpu().numpy(), lsum


def _oracle_u8(img, order, factors):
    return np.stack([oj.color_jitter(im, order, factors) for im in img])


@pytest.mark.parametrize('op', [oj.BRIGHTNESS, oj.CONTRAST, oj.SATURATION])
@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_u8_blend_lattice(backend, op):
    """every lattice pixel x factors in and outside [0, 1]: 0 and 1 exactly (the boundary between truncating and clipping), the
    next double above 1 (a C float 1.0), both clip sides (the C API does not restrict the factors)"""
    dev = use_backend(backend)
    img = _lattice_image()
    for f in U8_FACTORS:
        factors = [1.0, 1.0, 1.0, 0.0]
        factors[op] = f
        got, _, _ = _jitter_u8(dev, img, [op], factors)
        want = _oracle_u8(img, [op], factors)
        assert np.array_equal(got, want), (op, f, int((got != want).any(-1).sum()))
    if op == oj.BRIGHTNESS:           # both clip sides are reached by the out-of-range factors
        assert _oracle_u8(img, [op], [2.0, 1, 1, 0]).max() == 255 and (_oracle_u8(img, [1], [1, 2.0, 1, 0]) == 0).any()


@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_u8_hue_lattice(backend):
    dev = use_backend(backend)
    img = _lattice_image()
    shifts = set()
    for f in HUE_FACTORS:
        shifts.add(oj.hue_shift(f))
        got, _, _ = _jitter_u8(dev, img, [oj.HUE], [1.0, 1.0, 1.0, f])
        want = _oracle_u8(img, [oj.HUE], [1.0, 1.0, 1.0, f])
        assert np.array_equal(got, want), (f, int((got != want).any(-1).sum()))
    assert shifts == {129, 231, 255, 0, 1, 9, 25, 127}, shifts       # both wraps of the uint8 hue, 0 and +-1


def _half_mean_image(hw, k, rng):
    """hw pixels whose luminance sum is (2 k + 1) * hw / 2: gray pixels (L of (v, v, v) is v) in pairs around k + 1/2"""
    d = rng.integers(0, 4, hw // 2)
    v = np.concatenate([k - d, k + 1 + d])
    rng.shuffle(v)
    return np.repeat(v[:, None], 3, 1).astype(np.uint8).reshape(1, hw, 3)


@pytest.mark.parametrize('hw', [2, 6, 254, 258])
@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_u8_contrast_mean_at_an_exact_half(backend, hw):
    """int(mean + 0.5) with the mean at k + 1/2, two images with different k in one launch; factor 0 returns the mean itself"""
    dev = use_backend(backend)
    rng = np.random.default_rng(hw)
    img = np.stack([_half_mean_image(hw, 100, rng), _half_mean_image(hw, 37, rng)])
    for im, k in zip(img, (100, 37)):
        assert 2 * int(oj.to_l(im).astype(np.int64).sum()) == (2 * k + 1) * hw        # the precondition
    for f in (0.0, 0.5, 1.2):
        got, _, lsum = _jitter_u8(dev, img, [oj.CONTRAST], [1.0, f, 1.0, 0.0])
        assert np.array_equal(got, _oracle_u8(img, [oj.CONTRAST], [1.0, f, 1.0, 0.0])), f
        assert lsum.cpu().tolist() == [(2 * 100 + 1) * hw // 2, (2 * 37 + 1) * hw // 2]
    assert bool((got[0] != got[1]).any())
    got0, _, _ = _jitter_u8(dev, img, [oj.CONTRAST], [1.0, 0.0, 1.0, 0.0])
    assert bool((got0[0] == 101).all()) and bool((got0[1] == 38).all())


@pytest.mark.parametrize('hw', [1, 63, 64, 65, 255, 256, 257, 16384, 16385, 16384 + 257])
@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_u8_luminance_sum(backend, hw):
    """the exact integer sum per image in the caller's `lsum`, up to and across the 64-block cap (hw > 16384), batch 3, with
    garbage in `lsum` on entry: the entry point zeroes it"""
    dev = use_backend(backend)
    rng = np.random.default_rng(hw)
    img = rng.integers(0, 256, (3, 1, hw, 3), dtype=np.uint8)
    img[1] //= 3
    want = [int(oj.to_l(im).astype(np.int64).sum()) for im in img]
    assert len(set(want)) == 3 or hw == 1
    for garbage in (0, 0x0123456789ABCDEF):
        lsum = torch.full((3,), garbage, dtype=torch.int64, device=dev)
        got, _, lsum = _jitter_u8(dev, img, [oj.CONTRAST], [1.0, 0.9, 1.0, 0.0], lsum=lsum)
        assert lsum.cpu().tolist() == want, (hw, garbage)
        assert np.array_equal(got, _oracle_u8(img, [oj.CONTRAST], [1.0, 0.9, 1.0, 0.0]))


@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_u8_grid_stride(backend):
    """one image of 1030 x 1020 = 1050600 pixels, more than 4096 blocks x 256 threads, order (hue, brightness, saturation,
    contrast)."""
    dev = use_backend(backend)
    assert 1030 * 1020 > 4096 * 256
    img = np.random.default_rng(4096).integers(0, 256, (1, 1030, 1020, 3), dtype=np.uint8)
    factors = [1.13, 0.87, 1.09, 0.06]
    got, src, _ = _jitter_u8(dev, img, [3, 0, 2, 1], factors)
    assert np.array_equal(src, img)
    want = _oracle_u8(img, [3, 0, 2, 1], factors)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())


@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_u8_ping_pong(backend):
    """1 .. 8 ops (repeats allowed by the C API): the result is in `dst` for even and odd counts, `src` is unchanged; an empty
    chain copies"""
    dev = use_backend(backend)
    img = np.random.default_rng(7).integers(0, 256, (2, 5, 13, 3), dtype=np.uint8)
    chain = [0, 3, 1, 2, 0, 3, 2, 1]
    factors = [0.9, 1.15, 1.1, -0.07]
    for n in range(0, 9):
        got, src, _ = _jitter_u8(dev, img, chain[:n], factors)
        assert np.array_equal(src, img), n
        assert np.array_equal(got, _oracle_u8(img, chain[:n], factors)), n
    for bad in ([4], [-1]):
        with pytest.raises(_lib.ClslamError):
            _jitter_u8(dev, img, bad, factors)
    with pytest.raises(_lib.ClslamError):
        _jitter_u8(dev, img, [0], [1.0, 1.0, 1.0, 0.6])


# ======================================================================================================================
# 3. jitter_f32_sum_kernel, jitter_f32_apply_kernel
ORDERS = [list(p) for p in itertools.permutations(range(4))]
F32_FACTORS = [0.93, 1.07, 1.13, 0.037]
# (order as the record holds it, factors).  After the 24 orders: single ops, the empty chain, chains ended early by -1 (with ops
# BEHIND the terminator that must not run), contrast named twice (one mean, in front of the first)
RECORDS = [(o, F32_FACTORS) for o in ORDERS]
RECORDS += [([op], [1.15, 0.85, 1.2, -0.1]) for op in range(4)]
RECORDS += [([], [1, 1, 1, 0]), ([3, 0, 1, -1], [0.88, 1.17, 1.09, -0.08]), ([2, -1, 1, 3], [0.95, 1.06, 0.83, 0.031]),
            ([1, -1, -1, -1], [1.0, 1.2, 1.0, 0.0]), ([0, 2, 3, -1], [1.19, 1.0, 1.12, -0.1]),
            ([1, 0, 1, 2], [1.1, 0.9, 1.05, 0.02]), ([3], [1, 1, 1, -0.5]), ([3], [1, 1, 1, 0.5]), ([3, 1], [1, 0.8, 1, 0.0])]


def _record_params(records, dev):
    """ingest.jitter_params, but the order is written as given: -1 may stand in front of further ops"""
    rec = np.zeros(len(records), dtype=[('order', np.int32, 4), ('f', np.float32, 4), ('omf', np.float32, 4)])
    for i, (order, factors) in enumerate(records):
        o = [int(v) for v in order]
        rec['order'][i] = o + [-1] * (4 - len(o))
        rec['f'][i] = [np.float32(float(v)) for v in factors]
        rec['omf'][i] = [np.float32(1.0 - float(v)) for v in factors]
    plain = [r for r in records if -1 not in r[0]]
    if plain:          # the wrapper writes the same bytes for records it can express
        mine = torch.from_numpy(rec.view(np.uint8).reshape(-1, 48).copy())[[i for i, r in enumerate(records) if -1 not in r[0]]]
        assert torch.equal(ingest.jitter_params(plain, 'cpu').view(-1, 48), mine)
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)


def _f32_images(n, h, w, seed):
    """n images (3,h,w) in [0,1], cycling through: noise, gray stretches, a saturated channel, byte fractions, all zero, all
    one, hue at the wrap (r the maximum, g one float below b: h lands one step under 1)"""
    g = torch.Generator().manual_seed(seed)
    imgs = torch.rand(n, 3, h, w, generator=g)
    flat = imgs.view(n, 3, -1)
    for i in range(n):
        kind = i % 7
        if kind == 1:
            flat[i, :, ::3] = flat[i, :1, ::3]
        elif kind == 2:
            flat[i, 0] = 1.0
        elif kind == 3:
            flat[i] = (flat[i] * 255).round() / 255
        elif kind == 4:
            flat[i] = 0.0
        elif kind == 5:
            flat[i] = 1.0
        elif kind == 6:
            flat[i, 0] = 0.5 + 0.5 * flat[i, 0]
            flat[i, 2] = 0.5 * flat[i, 2]
            flat[i, 1] = torch.nextafter(flat[i, 2], torch.tensor(-1.0))
            flat[i, :, ::5] = flat[i, :1, ::5]          # and gray pixels: h = 0 exactly
    return imgs


def _check_f32(dev, imgs, records):
    """one clslam_color_jitter_f32 launch over imgs (n,3,h,w) with one record per image, held to the two-step reference"""
    n, _, h, w = imgs.shape
    hw, nblk = h * w, R.sum_blocks(h * w)
    assert _lib.get_lib().cdll.clslam_color_jitter_f32_blocks(h, w) == nblk
    params = _record_params(records, dev)
    src = imgs.to(dev)
    dst = torch.full((n * 3 * hw + 16,), -7.0, device=dev)
    partial = torch.full((n * nblk + 64,), float('nan'), device=dev)
    _lib_call('clslam_color_jitter_f32', src.data_ptr(), dst.data_ptr(), params.data_ptr(), partial.data_ptr(), n, h, w, _stream(src))
    assert torch.equal(src.cpu(), imgs)
    dst, partial = dst.cpu(), partial.cpu()
    assert bool((dst[-16:] == -7.0).all()) and bool(partial[n * nblk:].isnan().all())
    out, partial = dst[:-16].view(n, 3, h, w), partial[:n * nblk].view(n, nblk)
    worst = 0.0
    for i, (order, factors) in enumerate(records):
        gray = R.gray_before_contrast(imgs[i], order, factors)
        if gray is None:
            assert bool(partial[i].isnan().all()), (i, order, 'a partial of an image without contrast was written')
            mean = torch.tensor(float('nan'))
        else:
            sums, abs_sums = R.partition_sums(gray)
            err, bound = (partial[i].double() - sums).abs(), R.partial_bound(hw, abs_sums)
            assert bool((err <= bound).all()), (i, order, hw, err.tolist(), bound.tolist())
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            mean = R.kernel_mean(partial[i], hw)
        want = R.color_jitter_injected(imgs[i], order, factors, mean)
        assert torch.equal(out[i], want), (i, order, hw, float((out[i] - want).abs().max()))
    return worst


@pytest.mark.parametrize('hw', [1, 63, 255, 256, 257, 1024, 1025, 65536, 65537, 122880, 131072 + 300])
@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_f32_sizes(backend, hw):
    """one to three images per size, contrast first / in the middle / last: one sum block, the step to two (1025), the 64-block
    cap (hw > 65536, 192 x 640 = 122880 among them), and past the apply kernel's 256 blocks x 512 pixels"""
    dev = use_backend(backend)
    h, w = (192, 640) if hw == 122880 else (1, hw)
    n = 3 if hw <= 65537 else 2
    records = [([1, 0, 2, 3], [1.13, 0.84, 0.91, 0.06]), ([3, 2, 0, 1], [0.88, 1.17, 1.09, -0.08]),
               ([2, 1, 3, 0], [0.95, 1.06, 0.83, 0.031])][:n]
    worst = _check_f32(dev, _f32_images(n, h, w, hw), records)
    print(f'hw {hw}: worst partial error / derived bound {worst:.3f}')


@pytest.mark.parametrize('hw', [1025, 122880])
@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_f32_records(backend, hw):
    """all 24 orders, the single ops, the empty chain, early-terminated chains, contrast at every position and absent -- each
    image of ONE launch with its own record, over the special images"""
    dev = use_backend(backend)
    h, w = (192, 640) if hw == 122880 else (1, hw)
    assert {o.index(1) for o, _ in RECORDS[:24]} == {0, 1, 2, 3} and any(1 not in R.chain_of(o) for o, _ in RECORDS)
    # the image kind cycles with 7, the records do not: every special image meets chains with and without contrast
    imgs = _f32_images(len(RECORDS), h, w, 11 + hw)
    step = len(RECORDS) if hw == 1025 else 8          # 192 x 640: eight images (12 MB) per launch
    worst = max(_check_f32(dev, imgs[i:i + step], RECORDS[i:i + step]) for i in range(0, len(RECORDS), step))
    print(f'hw {hw}: worst partial error / derived bound {worst:.3f}')


@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_f32_hue_at_the_wrap(backend):
    """r the maximum and g one float below b (h one step under 1), and gray pixels (h = 0): hue factors -0.1, +0.1 and 0 alone
    and in front of / behind contrast"""
    dev = use_backend(backend)
    imgs = _f32_images(7, 1, 1300, 5)[6:].repeat(7, 1, 1, 1)
    records = [([3], [1, 1, 1, -0.1]), ([3], [1, 1, 1, 0.1]), ([3], [1, 1, 1, 0.0]), ([3, 1], [1, 1.1, 1, 0.1]),
               ([1, 3], [1, 1.1, 1, -0.1]), ([1, 3], [1, 0.9, 1, 0.1]), ([3, 1, 2, 0], [0.9, 1.1, 1.2, 0.0])]
    _check_f32(dev, imgs, records)


@pytest.mark.parametrize('backend', BACKENDS)
def test_jitter_f32_argument_checks(backend):
    dev = use_backend(backend)
    x = torch.zeros(3 * 4, device=dev)
    p = _record_params([([0], F32_FACTORS)], dev)
    for args in ((None, x, p, x), (x, None, p, x), (x, x, None, x), (x, x, p, None)):
        with pytest.raises(_lib.ClslamError):
            _lib_call('clslam_color_jitter_f32', *[None if a is None else a.data_ptr() for a in args], 1, 2, 2, _stream(x))
    with pytest.raises(_lib.ClslamError):
        _lib_call('clslam_color_jitter_f32', x.data_ptr(), x.data_ptr(), p.data_ptr(), x.data_ptr(), 65536, 2, 2, _stream(x))
    _lib_call('clslam_color_jitter_f32', None, None, None, None, 0, 2, 2, _stream(x))


# ======================================================================================================================
# 4. store_pack_kernel
def _pack(dev, planes, offsets, slot, inexact, n_planes=None, counts=None):
    desc = _lib.StorePackDesc()
    desc.n_planes = len(planes) if n_planes is None else n_planes
    for k, (t, off) in enumerate(zip(planes, offsets)):
        desc.plane[k], desc.offset[k], desc.count[k] = t.data_ptr(), int(off), t.numel() if counts is None else counts[k]
    _lib_call('clslam_store_pack', C.byref(desc), slot.data_ptr(), inexact.data_ptr(), _stream(slot))


def _pack_values(n, seed):
    """byte fractions, every eleventh value moved off its byte (counted), every 97th outside [0, 1]"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n).astype(np.float32) / np.float32(255)
    x[3::11] = np.nextafter(x[3::11], np.float32(2))
    x[5::97] = rng.uniform(-0.5, 1.5, x[5::97].shape).astype(np.float32)
    return x


def _check_pack(dev, xs, offsets, src_shift=0, slot_bytes=None, inexact0=0):
    """xs: numpy float32 planes; offsets: bytes from the slot's start.  Every byte of the slot that belongs to no plane stays
    0xA5.  src_shift: floats the source views are shifted against a 16-byte aligned allocation."""
    slot_bytes = slot_bytes or max(o + x.size for o, x in zip(offsets, xs)) + GUARD
    slot = torch.full((slot_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    inexact = torch.full((1,), inexact0, dtype=torch.int64, device=dev)
    planes = []
    for x in xs:
        buf = torch.zeros(x.size + 8, device=dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[src_shift:src_shift + x.size]
        view.copy_(torch.from_numpy(x))
        planes.append(view)
    _pack(dev, planes, offsets, slot, inexact)
    want = np.full(slot_bytes, 0xA5, np.uint8)
    bad = inexact0
    for x, o in zip(xs, offsets):
        b, n_bad = R.pack_bytes(x)
        want[o:o + x.size] = b
        bad += n_bad
    got = slot.cpu().numpy()
    assert np.array_equal(got, want), [int(v) for v in np.nonzero(got != want)[0][:8]]
    assert int(inexact.item()) == bad
    return bad


@pytest.mark.parametrize('count', [1, 3, 4, 5, 1023, 1025, 368640, 2 * 262144 + 7])
@pytest.mark.parametrize('backend', BACKENDS)
def test_store_pack_counts(backend, count):
    """bytes and the inexact count, exactly; 368640 is the real level 0 and 2 * 262144 + 7 three passes of the 256-block grid:
    the vector loop strides.  Counts that are no multiple of 4 run the scalar tail next to the vector part."""
    dev = use_backend(backend)
    assert 368640 > 256 * 256 * 4
    bad = _check_pack(dev, [_pack_values(count, count)], [16])
    assert count < 11 or bad > 0


@pytest.mark.parametrize('backend', BACKENDS)
def test_store_pack_alignment(backend):
    """a source one float off a 16-byte boundary (all scalar), a destination that is 4- but not 16-byte aligned (vector), one
    that is not 4-byte aligned (all scalar)"""
    dev = use_backend(backend)
    x = _pack_values(2053, 1)
    _check_pack(dev, [x], [16], src_shift=1)
    _check_pack(dev, [x], [4])
    _check_pack(dev, [x], [18])
    _check_pack(dev, [x, x[:1025]], [18, 18 + 2053 + 7], src_shift=3)


@pytest.mark.parametrize('backend', BACKENDS)
def test_store_pack_planes(backend):
    """12 planes of different counts in one launch (3 frames x 4 levels of 192 x 640), 16 bytes of 0xA5 between them; no plane at
    all; more planes than the descriptor holds"""
    dev = use_backend(backend)
    counts = [3 * (192 >> s) * (640 >> s) for s in range(4)] * 3
    offsets, off = [], 0
    for c in counts:
        offsets.append(off)
        off += (c + 15) // 16 * 16 + 16
    xs = [_pack_values(c, 50 + k) for k, c in enumerate(counts)]
    _check_pack(dev, xs, offsets)
    slot = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    inexact = torch.zeros(1, dtype=torch.int64, device=dev)
    x = torch.full((8,), 0.3, device=dev)
    _pack(dev, [], [], slot, inexact)
    with pytest.raises(_lib.ClslamError):
        _pack(dev, [x], [0], slot, inexact, n_planes=_lib.STORE_MAX_PLANES + 1)
    with pytest.raises(_lib.ClslamError):
        _pack(dev, [x], [0], slot, inexact, counts=[0])
    with pytest.raises(_lib.ClslamError):
        _pack(dev, [x], [-16], slot, inexact)
    assert bool((slot.cpu() == 0xA5).all()) and int(inexact.item()) == 0


@pytest.mark.parametrize('backend', BACKENDS)
def test_store_pack_odd_values(backend):
    """NaN, infinities, -0.0, values just outside [0, 1], the neighbours of k / 255, denormals: the bytes and the count of the
    float32 reference.  -0.0 packs to 0 and compares equal to 0 / 255: not counted."""
    dev = use_backend(backend)
    f = np.float32
    ks = np.array([0, 1, 7, 127, 128, 254, 255], f) / f(255)
    odd = np.concatenate([
        np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1e-3, 1 + 1e-3, 1.0, 0.5 / 255, 1.5 / 255, 254.5 / 255, 3e38, -3e38,
                  1e-45, -1e-45, 1.1754942e-38, 1e-39], f),
        ks, np.nextafter(ks, f(2)), np.nextafter(ks, f(-2))])
    want_b, want_bad = R.pack_bytes(odd)
    assert want_b[0] == 0 and want_b[1] == 255 and want_b[2] == 0 and want_b[3] == 0 and want_b[6] == 255
    assert want_bad == odd.size - 2 - 1 - len(ks)        # all but -0.0, 0.0, 1.0 and the seven k / 255
    for shift in (0, 1):                                 # vector path and scalar path
        assert _check_pack(dev, [odd], [16], src_shift=shift) == want_bad
    assert _check_pack(dev, [np.array([-0.0], f)], [16]) == 0
    assert _check_pack(dev, [np.array([-0.0, -0.0, -0.0, -0.0, np.nan], f)], [16]) == 1


@pytest.mark.parametrize('backend', BACKENDS)
def test_store_pack_inexact_accumulates(backend):
    """`inexact` is added to, never reset: two launches, the second on top of the first one's count"""
    dev = use_backend(backend)
    first = _check_pack(dev, [_pack_values(777, 2)], [16])
    assert first > 0
    total = _check_pack(dev, [_pack_values(1300, 3)], [16], inexact0=first)
    assert total > first


# ======================================================================================================================
# 5. store_gather_sum_kernel, store_gather_apply_kernel
class _Store:
    """a frame store laid out by hand: random bytes at the documented offsets (frame-major, then level; planar (3, h, w) blocks
    rounded up to 16 bytes), `slots` slots allocated of which `capacity` are declared"""

    def __init__(self, dev, sizes, n_frames, slots, capacity, seed):
        self.dev, self.sizes, self.n_frames, self.capacity = dev, sizes, n_frames, capacity
        self.offsets, off = [], 0
        for _ in range(n_frames):
            for h, w in sizes:
                self.offsets.append(off)
                off += (3 * h * w + 15) // 16 * 16
        self.slot_bytes = off
        self.host = torch.randint(0, 256, (slots * off,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        self.data = self.host.to(dev)

    def block(self, slot, frame, li):
        h, w = self.sizes[li]
        o = slot * self.slot_bytes + self.offsets[frame * len(self.sizes) + li]
        return self.host[o:o + 3 * h * w].view(3, h, w)


def _gather(store, slot_idx, records, rows, row0=0, aug_levels=None, rgb_shift=0, aug_shift=0, with_params=True):
    """one clslam_store_gather_jitter launch.  aug_levels: levels whose table entries get an `aug` pointer (None: all, (): none).
    -> (rgb, aug, partial) on the host: rgb / aug [table] (rows,3,h,w) prefilled with -7, partial [level][image][64] prefilled
    with NaN (and the NaN slack behind it checked)."""
    dev, sizes, nf = store.dev, store.sizes, store.n_frames
    L, n_img = len(sizes), len(slot_idx)
    aug_levels = tuple(range(L)) if aug_levels is None else tuple(aug_levels)
    desc = _lib.StoreGatherDesc()
    desc.n_frames, desc.n_levels, desc.slot_bytes, desc.capacity = nf, L, store.slot_bytes, store.capacity
    for li, (h, w) in enumerate(sizes):
        desc.h[li], desc.w[li] = h, w
    rgb, aug = [], []
    for t in range(nf * L):
        h, w = sizes[t % L]
        n = rows * 3 * h * w
        r = torch.full((n + 8,), -7.0, device=dev)
        a = torch.full((n + 8,), -7.0, device=dev)
        assert r.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0
        rgb.append(r)
        aug.append(a)
        desc.rgb[t] = r.data_ptr() + 4 * rgb_shift
        desc.aug[t] = a.data_ptr() + 4 * aug_shift if t % L in aug_levels else None
        desc.stride[t], desc.offset[t] = 3 * h * w, store.offsets[t]
    params = _record_params(records, dev) if with_params else None
    side = max(L, n_img)
    partial = torch.full((side * side * 64,), float('nan'), device=dev) if with_params else None
    idx = torch.tensor(slot_idx, dtype=torch.int32).to(dev)
    _lib_call('clslam_store_gather_jitter', C.byref(desc), store.data.data_ptr(), idx.data_ptr(),
              None if params is None else params.data_ptr(), None if partial is None else partial.data_ptr(), n_img, row0,
              _stream(store.data))
    assert torch.equal(store.data.cpu(), store.host)
    out = []
    for shift, bufs in ((rgb_shift, rgb), (aug_shift, aug)):
        views = []
        for t, buf in enumerate(bufs):
            h, w = sizes[t % L]
            buf = buf.cpu()
            n = rows * 3 * h * w
            assert bool((buf[:shift] == -7.0).all()) and bool((buf[shift + n:] == -7.0).all())
            views.append(buf[shift:shift + n].view(rows, 3, h, w))
        out.append(views)
    if partial is not None:
        partial = partial.cpu()
        assert bool(partial[L * n_img * 64:].isnan().all()), 'a partial was written outside [level][image][64]'
        partial = partial[:L * n_img * 64].view(L, n_img, 64)
    return out[0], out[1], partial


def _check_gather(store, slot_idx, records, rows, row0=0, aug_levels=None, **kw):
    """the launch of _gather against the reference: `rgb` rows = byte / 255, `aug` rows = the injected-mean chain, partials
    within the derived bound of the float64 partition sums; rows of invalid slots, rows above row0, `aug` of entries without a
    pointer and partials nobody owes keep their prefill"""
    sizes, nf = store.sizes, store.n_frames
    L, n_img = len(sizes), len(slot_idx)
    rgb, aug, partial = _gather(store, slot_idx, records, rows, row0, aug_levels, **kw)
    aug_levels = tuple(range(L)) if aug_levels is None else tuple(aug_levels)
    written = set()
    worst = 0.0
    for img, slot in enumerate(slot_idx):
        frame, row = img % nf, row0 + img // nf
        order, factors = records[img]
        for li, (h, w) in enumerate(sizes):
            t, hw = frame * L + li, h * w
            nblk = R.sum_blocks(hw)
            valid = 0 <= slot < store.capacity
            owes = valid and li in aug_levels
            want = store.block(slot, frame, li).to(torch.float32) / 255 if valid else None
            gray = R.gray_before_contrast(want, order, factors) if valid and aug_levels else None
            if gray is None:
                assert bool(partial is None or partial[li, img].isnan().all()), (img, li, 'partial written')
            else:
                assert bool(partial[li, img, nblk:].isnan().all())
                sums, abs_sums = R.partition_sums(gray)
                err, bound = (partial[li, img, :nblk].double() - sums).abs(), R.partial_bound(hw, abs_sums)
                assert bool((err <= bound).all()), (img, li, err.tolist(), bound.tolist())
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            if not valid:
                continue
            written.add((t, row))
            assert torch.equal(rgb[t][row], want), (img, li, 'rgb')
            if owes:
                mean = R.kernel_mean(partial[li, img, :nblk], hw) if gray is not None else torch.tensor(float('nan'))
                ref = R.color_jitter_injected(want, order, factors, mean)
                assert torch.equal(aug[t][row], ref), (img, li, order, float((aug[t][row] - ref).abs().max()))
    for t in range(nf * L):
        for row in range(rows):
            if (t, row) not in written:
                assert bool((rgb[t][row] == -7.0).all()) and bool((aug[t][row] == -7.0).all()), (t, row, 'untouched row written')
            elif t % L not in aug_levels:
                assert bool((aug[t][row] == -7.0).all()), (t, row, 'aug written without a pointer')
    return rgb, aug, worst


def _pyramid(h, w, levels=4):
    return [(h >> s, w >> s) for s in range(levels)]


GATHER_RECORDS = [([1, 0, 2, 3], [1.13, 0.84, 0.91, 0.06]), ([3, 2, 0, 1], [0.88, 1.17, 1.09, -0.08]),
                  ([2, 1, 3, 0], [0.95, 1.06, 0.83, 0.031]), ([0, 3, 2], [1.19, 1.0, 1.12, -0.1]),
                  ([0, 1, 3, 2], [1.05, 0.9, 1.1, 0.09]), ([2, 3, 1, -1], [1.0, 1.2, 0.8, -0.03]), ([1], [1.0, 0.8, 1.0, 0.0])]


@pytest.mark.parametrize('backend', BACKENDS)
def test_gather_slots_rows_and_records(backend):
    """3 frames x 4 levels at 48 x 42 (2016 / 504 / 120 / 30 pixels: two sum blocks down to no vector part).  Samples from the
    slots [1, -1, 0, capacity, 1] in one launch behind an untouched row 0, a different record for each of the 15 images (contrast
    at every position and absent).  The store is allocated one slot longer than `capacity`, so the slot index `capacity` points
    at valid bytes of the test's own allocation: a kernel that served it would fill a row that must keep its prefill."""
    dev = use_backend(backend)
    store = _Store(dev, _pyramid(48, 42), 3, slots=3, capacity=2, seed=1)
    slots = [1, -1, 0, store.capacity, 1]
    slot_idx = [s for s in slots for _ in range(3)]
    records = [GATHER_RECORDS[i % 7] for i in range(15)]
    _check_gather(store, slot_idx, records, rows=6, row0=1)
    # the same record for every image: repeated slots give identical rows
    rgb, aug, _ = _check_gather(store, slot_idx, [GATHER_RECORDS[2]] * 15, rows=6, row0=1)
    for t in range(12):
        assert torch.equal(rgb[t][1], rgb[t][5]) and torch.equal(aug[t][1], aug[t][5])
        assert not torch.equal(rgb[t][1], rgb[t][3])


@pytest.mark.parametrize('backend', BACKENDS)
def test_gather_real_size(backend):
    """192 x 640, 3 frames x 4 levels, one record per frame: level 0 has 122880 pixels, past the 64 blocks of the sum pass"""
    dev = use_backend(backend)
    store = _Store(dev, _pyramid(192, 640), 3, slots=1, capacity=1, seed=2)
    assert R.sum_blocks(192 * 640) == 64 and R.adds_per_thread(192 * 640) > 1
    _, _, worst = _check_gather(store, [0, 0, 0], GATHER_RECORDS[:3], rows=1)
    print(f'192 x 640: worst partial error / derived bound {worst:.3f}')


@pytest.mark.parametrize('backend', BACKENDS)
def test_gather_apply_grid_stride(backend):
    """1 frame x 1 level at 512 x 520 = 266240 pixels: more than the apply kernel's 256 blocks x 1024 pixels"""
    dev = use_backend(backend)
    assert 512 * 520 > 256 * 1024
    store = _Store(dev, [(512, 520)], 1, slots=1, capacity=1, seed=3)
    _check_gather(store, [0], [GATHER_RECORDS[1]], rows=1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_gather_mixed_aug_table_and_no_jitter(backend):
    """`aug` pointers for level 0 only: `rgb` is written at every level, `aug` at level 0 alone.  Without any `aug` pointer,
    `params` and `partial` may be null."""
    dev = use_backend(backend)
    store = _Store(dev, _pyramid(48, 42), 3, slots=2, capacity=2, seed=4)
    slot_idx = [1, 1, 1, 0, 0, 0]
    records = [GATHER_RECORDS[i % 7] for i in range(6)]
    _check_gather(store, slot_idx, records, rows=2, aug_levels=(0,))
    _check_gather(store, slot_idx, records, rows=2, aug_levels=(2, 3))
    _check_gather(store, slot_idx, records, rows=2, aug_levels=(), with_params=False)
    _check_gather(store, slot_idx, records, rows=2, aug_levels=())


@pytest.mark.parametrize('backend', BACKENDS)
def test_gather_unaligned_rows(backend):
    """row pointers one float off a 16-byte boundary force the scalar loop (48 x 40: every level could run the vector path)"""
    dev = use_backend(backend)
    store = _Store(dev, _pyramid(48, 40), 3, slots=2, capacity=2, seed=5)
    slot_idx = [0, 0, 0, 1, 1, 1]
    records = [GATHER_RECORDS[(i + 1) % 7] for i in range(6)]
    _check_gather(store, slot_idx, records, rows=2)                              # vector path
    _check_gather(store, slot_idx, records, rows=2, rgb_shift=1)
    _check_gather(store, slot_idx, records, rows=2, aug_shift=3)
    _check_gather(store, slot_idx, records, rows=2, rgb_shift=2, aug_shift=2)


@pytest.mark.parametrize('backend', BACKENDS)
def test_gather_argument_checks(backend):
    dev = use_backend(backend)
    store = _Store(dev, _pyramid(16, 16, 2), 3, slots=1, capacity=1, seed=6)
    recs = [GATHER_RECORDS[0]] * 6
    _gather(store, [], [], rows=1)                                               # no image: returns
    with pytest.raises(_lib.ClslamError):                                        # no whole samples
        _gather(store, [0, 0], recs[:2], rows=1)
    with pytest.raises(_lib.ClslamError):                                        # aug without params
        _gather(store, [0, 0, 0], recs[:3], rows=1, with_params=False)
    with pytest.raises(_lib.ClslamError):
        _gather(store, [0, 0, 0], recs[:3], rows=1, row0=-1)
    store.sizes = [(16, 16), (0, 8)]                                             # a level with h = 0
    with pytest.raises(_lib.ClslamError):
        _gather(store, [0, 0, 0], recs[:3], rows=1)
    desc = _lib.StoreGatherDesc()                                                # 5 frames x 4 levels > 16 planes
    desc.n_frames, desc.n_levels, desc.slot_bytes, desc.capacity = 5, 4, 64, 1
    idx = torch.zeros(5, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.ClslamError):
        _lib_call('clslam_store_gather_jitter', C.byref(desc), store.data.data_ptr(), idx.data_ptr(), None, None, 5, 0,
                  _stream(store.data))
