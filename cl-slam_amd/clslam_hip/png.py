"""PNG files written on the device (csrc/png_encode.hip, include/clslam_hip.h "PNG encoding").

``encode(image, filter='adaptive') -> bytes``               one (H,W) or (H,W,3) uint8 image, numpy or tensor
``encode_batch(images, filter='adaptive') -> list[bytes]``  (N,H,W[,3]): one set of launches, one read of the N lengths, then
                                                            only the bytes of each file
``save(path, image, filter='adaptive')``                    encode, then write the file

Scanline filter, a deflate stream of literal-only Huffman (or stored) blocks, Adler-32 and the chunk CRCs are formed on the
device; the pixels of a tensor that is already there never reach the host.  There is no LZ77 matching, so the files are larger
than zlib's (profiles/png_encode.txt says by how much); every PNG reader decodes them to the same pixels.
`filter`: 'adaptive' (per row the type with the smallest sum of min(b, 256 - b)) or 'none', 'sub', 'up', 'average', 'paeth' / 0..4.
"""
import numpy as np
import torch

from . import _lib, ops


def _images(fn: str, images, rank_gray: int) -> torch.Tensor:
    if not isinstance(images, torch.Tensor):
        images = np.asarray(images)
        if images.dtype != np.uint8:
            raise _lib.ClslamError(f'{fn}: uint8 images, got {images.dtype}')
        images = np.ascontiguousarray(images)
        images = torch.from_numpy(images if images.flags.writeable else images.copy())
    if images.dtype is not torch.uint8:
        raise _lib.ClslamError(f'{fn}: uint8 images, got {images.dtype}')
    if images.dim() not in (rank_gray, rank_gray + 1) or (images.dim() == rank_gray + 1 and images.shape[-1] != 3) \
            or min(images.shape, default=0) == 0:
        want = '(H,W) or (H,W,3)' if rank_gray == 2 else '(N,H,W) or (N,H,W,3)'
        raise _lib.ClslamError(f'{fn}: a non-empty {want} image is expected, got {tuple(images.shape)}')
    lib = _lib.get_lib()
    if images.device.type != lib.device_type:
        images = images.to(torch.device('cuda', torch.cuda.current_device()) if lib.is_device else torch.device('cpu'))
    return images.contiguous()


def encode_batch(images, filter='adaptive'):
    """(N,H,W) or (N,H,W,3) uint8 -> the N files"""
    t = _images('png.encode_batch', images, 3)
    files, lengths = ops.png_encode(t, filter)
    lengths = lengths.cpu().tolist()                                      # the one synchronising read
    return [files[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lengths)]


def encode(image, filter='adaptive') -> bytes:
    """(H,W) or (H,W,3) uint8 -> the file"""
    return encode_batch(_images('png.encode', image, 2)[None], filter)[0]


def save(path, image, filter='adaptive') -> None:
    data = encode(image, filter)
    with open(path, 'wb') as f:
        f.write(data)
