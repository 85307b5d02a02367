"""csrc/png_encode.hip against tests/png_reference.py, Pillow and zlib: the filtered stream byte for byte, the file by decoding it
(Pillow), by inflating it (zlib), by its checksums (zlib.crc32 / zlib.adler32) and by walking its deflate blocks bit by bit.

Sizes.  Filter: W in {1, 2, 5, 64, 67} (no left neighbour; one; odd; a quarter of the 256-thread row and just past it), H in
{1, 2, 3, 33} (no row above; one; the Up / Average / Paeth rows), 1 and 3 channels.  Deflate: S = 16384 filtered bytes per block, so
streams of S - 1, S, S + 1 and 2 S + 3 bytes (one block short of full, full, a one-byte second block, a three-byte third) put codes
across 32-bit words and block edges; 960x1280x3 (a RobotCar frame, 226 blocks) runs on the device only."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_reference as ref
from emu_util import BACKENDS, use_backend

S = ref.S
WIDTHS, HEIGHTS = [1, 2, 5, 64, 67], [1, 2, 3, 33]
KINDS = ['random', 'smooth', 'constant']
_CACHE = {}


def _image(kind, H, W, C):
    shape = (H, W) if C == 1 else (H, W, 3)
    if kind == 'random':
        return np.random.default_rng(H * 1000 + W * 10 + C).integers(0, 256, shape, dtype=np.uint8)
    if kind == 'constant':
        return np.full(shape, 77, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    g = (3 * x + 5 * y) % 256
    return (g if C == 1 else np.stack([g, (g + 40) % 256, (2 * x + y) % 256], -1)).astype(np.uint8)


def _filtered(kind, H, W, C, fixed=None):
    key = (kind, H, W, C, fixed)
    if key not in _CACHE:
        stream, types = ref.filter_rows(_image(kind, H, W, C), fixed)
        stream.setflags(write=False)
        _CACHE[key] = (stream, types)
    return _CACHE[key]


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _files(out, lengths):
    out, lengths = out.cpu().numpy(), lengths.cpu().numpy()
    assert (out[np.arange(out.shape[1])[None] >= lengths[:, None]] == 0).all()       # nothing behind the file
    return [out[i, :n].tobytes() for i, n in enumerate(lengths)]


def _check(data, image, filtered):
    """the round trip and every checksum of one file -> its deflate blocks"""
    image = np.asarray(image)
    H, W = image.shape[:2]
    C = 1 if image.ndim == 2 else 3
    assert len(data) <= ref.bound(H, W, C)
    z = ref.check_file(data, bytes(filtered), H, W, C)
    assert np.array_equal(np.array(Image.open(io.BytesIO(data))), image)
    return ref.check_blocks(z, bytes(filtered))


# ---- 1. filter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_filter_matches_the_reference_byte_for_byte(backend, kind, C):
    from clslam_hip import ops
    device = use_backend(backend)
    seen = set()
    for H in HEIGHTS:
        for W in WIDTHS:
            image = _image(kind, H, W, C)
            want, types = _filtered(kind, H, W, C)
            got = ops.png_filter(_dev(image[None], device)).cpu().numpy()
            assert got.shape == (1, H * (1 + W * C)) and got.dtype == np.uint8
            assert np.array_equal(got[0], want), (H, W)
            seen |= set(types)
    if kind != 'constant':
        assert len(seen) >= 3                                            # the rule picks: not one type everywhere


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('fixed', [0, 1, 2, 3, 4])
def test_every_fixed_filter_type(backend, fixed):
    from clslam_hip import ops
    device = use_backend(backend)
    for C in (1, 3):
        for H, W in [(1, 1), (2, 5), (3, 67), (33, 64)]:
            image = _image('random', H, W, C)
            want, _ = _filtered('random', H, W, C, fixed)
            got = ops.png_filter(_dev(image[None], device), fixed).cpu().numpy()[0]
            assert np.array_equal(got, want), (C, H, W)
    name = {0: 'none', 1: 'sub', 2: 'up', 3: 'average', 4: 'paeth'}[fixed]
    assert np.array_equal(ops.png_filter(_dev(image[None], device), name).cpu().numpy()[0], want)


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_score_tie_goes_to_the_lower_type(backend):
    """row 0 = [2, 254]: None gives 2, 254 -> 2 + 2, Sub gives 2, 252 -> 2 + 4, Up = None on row 0 (the row above is 0): None (0)
    and Up (2) tie at 4 and None wins.  Row 1 = [4, 0]: None 4, 0 -> 4; Sub 4, 252 -> 8; Up 2, 2 -> 4; Average 3, 127 (a = 4,
    b = 254: (4 + 254) // 2 = 129, 0 - 129 = 127) -> 3 + 127: None and Up tie at 4 again, None wins."""
    from clslam_hip import ops
    device = use_backend(backend)
    image = np.array([[2, 254], [4, 0]], dtype=np.uint8)
    got = ops.png_filter(_dev(image[None], device)).cpu().numpy()[0]
    assert got.tolist() == [0, 2, 254, 0, 4, 0]
    want, types = ref.filter_rows(image)
    assert types == [0, 0] and np.array_equal(got, want)
    # and one where the tie is between Sub (1) and Paeth (4) on row 0 (Paeth = Sub there), both below None
    image = np.array([[100, 101, 102]], dtype=np.uint8)
    got = ops.png_filter(_dev(image[None], device)).cpu().numpy()[0]
    assert got.tolist() == [1, 100, 1, 1]


# ---- 2. round trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_round_trip_and_checksums(backend, kind, C):
    from clslam_hip import ops
    device = use_backend(backend)
    for H in HEIGHTS:
        for W in WIDTHS:
            image = _image(kind, H, W, C)
            want, _ = _filtered(kind, H, W, C)
            data, = _files(*ops.png_encode(_dev(image[None], device)))
            _check(data, image, want)
    image = _image(kind, 33, 67, C)
    for fixed in range(5):
        data, = _files(*ops.png_encode(_dev(image[None], device), fixed))
        _check(data, image, _filtered(kind, 33, 67, C, fixed)[0])


# ---- 3. block edges --------------------------------------------------------------------------------------------------------
def _peaked(H, W, seed):
    """bytes a Huffman code shortens: a geometric distribution, so the blocks are dynamic and their codes of many lengths"""
    return np.minimum(np.random.default_rng(seed).geometric(0.15, (H, W)) - 1, 255).astype(np.uint8)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('F,H,W', [(S - 1, 127, 128), (S, 128, 127), (S + 1, 113, 144), (2 * S + 3, 1, 2 * S + 2)])
def test_block_edges(backend, F, H, W):
    from clslam_hip import ops
    device = use_backend(backend)
    assert H * (1 + W) == F
    image = _peaked(H, W, F)
    want, _ = ref.filter_rows(image, 0)
    data, = _files(*ops.png_encode(_dev(image[None], device), 'none'))
    bl = _check(data, image, want)
    assert len(bl) == -(-F // S)
    assert [len(b['data']) for b in bl] == [S] * (F // S) + ([F % S] if F % S else [])
    assert bl[0]['type'] == 'dynamic' and len(set(bl[0]['lengths'])) > 4
    if F % S and F % S < 16:
        assert bl[-1]['type'] == 'stored'                                # a few bytes: the 1106-bit header does not pay
    adaptive, = _files(*ops.png_encode(_dev(image[None], device)))
    _check(adaptive, image, ref.filter_rows(image)[0])


# ---- 4. codes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_a_constant_image_gives_the_two_symbol_code(backend):
    """all zeros: every filter gives zeros, None wins every tie, so the stream is one literal and end-of-block: lengths 1 and 1"""
    from clslam_hip import ops
    device = use_backend(backend)
    image = np.zeros((40, 50), dtype=np.uint8)
    data, = _files(*ops.png_encode(_dev(image[None], device)))
    bl = _check(data, image, np.zeros(40 * 51, np.uint8))
    assert len(bl) == 1 and bl[0]['type'] == 'dynamic'
    assert bl[0]['lengths'][0] == 1 and bl[0]['lengths'][256] == 1 and sum(bl[0]['lengths']) == 2
    assert bl[0]['payload_bits'] == 40 * 51 + 1


@pytest.mark.parametrize('backend', BACKENDS)
def test_all_256_byte_values(backend):
    """every literal used, unevenly (value v occurs about 2 + 40 * 2^-(v % 9) times): 257 codes, none unused"""
    from clslam_hip import ops
    device = use_backend(backend)
    counts = [2 + (40 >> (v % 9)) for v in range(256)]
    vals = np.repeat(np.arange(256, dtype=np.uint8), counts)
    np.random.default_rng(0).shuffle(vals)
    H = 2
    W = len(vals) // H
    image = vals[:H * W].reshape(H, W)
    assert len(np.unique(image)) == 256
    want, _ = ref.filter_rows(image, 0)
    data, = _files(*ops.png_encode(_dev(image[None], device), 0))
    bl = _check(data, image, want)
    assert bl[0]['type'] == 'dynamic' and all(bl[0]['lengths'][:257])


def _fibonacci_stream():
    """one row behind filter type 0 whose histogram, end-of-block (1) first, is 1, 1, 2, 3, 5, ... over 18 literals: every partial
    sum is one below the next-but-one count, so there are no ties and the only Huffman tree is a chain, 18 deep -- no optimal code
    fits in 15 bits"""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    fib = fib[1:]                                                        # fib[0] is end-of-block's
    fib[-1] -= 1                                                         # the type byte, 0, is one of the most frequent literal's
    body = np.repeat(np.arange(17, -1, -1).astype(np.uint8), fib)        # literal 0 is the most frequent
    np.random.default_rng(1).shuffle(body)
    return np.concatenate([np.zeros(1, np.uint8), body])


@pytest.mark.parametrize('backend', BACKENDS)
def test_fibonacci_histogram_is_length_limited(backend):
    from clslam_hip import ops
    device = use_backend(backend)
    stream = _fibonacci_stream()
    F = len(stream)
    assert F <= S
    hist = {s: c for s, c in enumerate(np.bincount(stream).tolist()) if c}
    hist[256] = 1
    cost, depth = ref.huffman(hist)
    assert depth > 15
    padded = np.zeros((1, (F + 15) & ~15), np.uint8)
    padded[0, :F] = stream
    data, = _files(*ops.png_deflate(_dev(padded, device), 1, F - 1, 1))
    bl = _check(data, stream[1:].reshape(1, F - 1), stream)
    assert len(bl) == 1 and bl[0]['type'] == 'dynamic'
    used = [l for l in bl[0]['lengths'] if l]
    assert max(used) == 15 and sum(2 ** (15 - l) for l in used) == 2 ** 15
    assert cost < bl[0]['payload_bits'] <= cost + cost // 100           # the limit costs something, and little


# ---- 5. no expansion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_random_bytes_are_stored_and_the_bound_is_enforced(backend):
    from clslam_hip import ops
    from clslam_hip._lib import ClslamError
    device = use_backend(backend)
    H, W = 40, 300                                                       # 36040 filtered bytes: three blocks
    image = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want, _ = ref.filter_rows(image)
    d_image = _dev(image[None], device)
    data, = _files(*ops.png_encode(d_image))
    bl = _check(data, image, want)
    assert [b['type'] for b in bl] == ['stored'] * 3
    bound = ops.png_bound(H, W, 3)
    assert bound == ref.bound(H, W, 3) and len(data) == bound            # all stored: the bound is attained
    out = torch.full((1, (bound + 3) & ~3), 255, dtype=torch.uint8, device=device)
    files, lengths = ops.png_encode(d_image, out=out)
    assert files.data_ptr() == out.data_ptr() and _files(files, lengths)[0] == data
    small = torch.full((1, bound - 1), 255, dtype=torch.uint8, device=device)
    with pytest.raises(ClslamError, match='clslam_png_bound'):
        ops.png_encode(d_image, out=small)
    assert bool((small == 255).all())                                    # refused before any launch
    assert ops.png_bound(1, 1, 1) == 2 + 5 + 63 and ops.png_bound(1, 1, 2) == 0 and ops.png_bound(0, 4, 1) == 0


# ---- 6. batch and determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_a_batch_equals_its_images_one_by_one_and_runs_repeat(backend):
    from clslam_hip import ops
    device = use_backend(backend)
    H, W = 33, 200                                                       # 19833 filtered bytes: two blocks
    images = np.stack([_image('smooth', H, W, 3), _image('random', H, W, 3),
                       np.stack([_peaked(H, W, s) for s in (1, 2, 3)], -1)])
    batch = _files(*ops.png_encode(_dev(images, device)))
    again = _files(*ops.png_encode(_dev(images, device)))
    assert batch == again
    assert len(set(batch)) == 3
    for i in range(3):
        one, = _files(*ops.png_encode(_dev(images[i:i + 1], device)))
        assert one == batch[i]
        _check(one, images[i], ref.filter_rows(images[i])[0])


# ---- 7. a full frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_frame():
    from clslam_hip import ops, synth
    device = use_backend('hip')
    rgb = synth._texture(960, 1280, 4, 0.0)                              # (3,H,W) float32 in 0..1: sinusoids + a little noise
    image = np.ascontiguousarray((rgb.transpose(1, 2, 0) * 255).astype(np.uint8))
    assert image.shape == (960, 1280, 3) and np.unique(image).size > 16
    want, types = ref.filter_rows(image)
    data, = _files(*ops.png_encode(_dev(image[None], device)))
    assert len(data) <= ops.png_bound(960, 1280, 3)
    z = ref.check_file(data, bytes(want), 960, 1280, 3)
    assert np.array_equal(np.array(Image.open(io.BytesIO(data))), image)
    assert len(z) < len(want)                                            # it compresses


# ---- 8. bad arguments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_bad_arguments_raise_before_a_launch(backend):
    from clslam_hip import ops
    from clslam_hip._lib import ClslamError
    device = use_backend(backend)
    other = torch.device('meta')
    good = torch.zeros(1, 6, 10, 3, dtype=torch.uint8, device=device)
    for fn in (ops.png_filter, ops.png_encode):
        with pytest.raises(ClslamError, match='uint8'):
            fn(good.float())
        with pytest.raises(ClslamError, match=r'\(N,H,W\)'):
            fn(torch.zeros(1, 6, 10, 2, dtype=torch.uint8, device=device))
        with pytest.raises(ClslamError, match=r'\(N,H,W\)'):
            fn(torch.zeros(1, 6, 10, 4, dtype=torch.uint8, device=device))
        with pytest.raises(ClslamError, match='contiguous'):
            fn(torch.zeros(1, 6, 20, 3, dtype=torch.uint8, device=device)[:, :, ::2])
        with pytest.raises(ClslamError, match='filter'):
            fn(good, 5)
        with pytest.raises(ClslamError, match='filter'):
            fn(good, 'best')
    with pytest.raises(ClslamError, match='out must be'):
        ops.png_filter(good, out=torch.zeros(1, 6 * 31, dtype=torch.uint8, device=other))
    with pytest.raises(ClslamError, match='out must be'):
        ops.png_encode(good, out=torch.zeros(1, 512, dtype=torch.uint8, device=other))
    # the library's own checks, behind the wrapper's: filter type 5 and a short buffer are refused by the entry point itself
    lib = __import__('clslam_hip')._lib.get_lib()
    out = torch.zeros(1, 512, dtype=torch.uint8, device=device)
    with pytest.raises(ClslamError, match='filter type'):
        lib.call('clslam_png_filter', good.data_ptr(), out.data_ptr(), 512, 1, 6, 10, 3, 5, 0)
    with pytest.raises(ClslamError, match='channels'):
        lib.call('clslam_png_filter', good.data_ptr(), out.data_ptr(), 512, 1, 6, 10, 2, 0, 0)
    assert not out.any()


def test_the_abi_number_stays_and_the_symbols_are_listed():
    from clslam_hip import _lib
    assert _lib.ABI_VERSION == 114
    assert {'clslam_png_filter', 'clslam_png_deflate', 'clslam_png_encode', 'clslam_png_bound',
            'clslam_png_scratch'} <= set(_lib.exported_symbols())
    assert _lib.PNG_BLOCK == S
