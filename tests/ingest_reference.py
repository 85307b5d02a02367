"""TEST INFRASTRUCTURE: plain restatements of what the kernels of cl-slam_amd/csrc/ingest.hip compute, for
tests/test_ingest_kernels.py.  The integer paths (LANCZOS resize, uint8 colour jitter) and the float chain are restated in
oracle/resize.py, oracle/jitter.py and oracle/jitter_tensor.py; this file adds what those leave open:

    resample_axis_raw   one pass of oracle.resize._resample_axis WITHOUT the clip to [0, 255] (to show that an input overshoots)
    to_planar           ToTensor: uint8 (N,H,W,C) -> float32 (N,C,H,W) = f32(byte) / f32(255)
    sum_blocks          blocks of the gray-sum pass: clamp(ceil(hw / 1024), 1, 64)
    partition_sums      the sum pass's partition in float64: block b of nblk takes the pixels b * 256 + t + k * nblk * 256
    kernel_mean         the contrast mean as the apply kernels form it: sequential fp32 sum of the partials, then / f32(hw)
    gray_before_contrast, color_jitter_injected
                        oracle.jitter_tensor's chain cut in front of `contrast`, and the whole chain with a GIVEN contrast mean
                        (everything but torch.mean's summation order is bitwise in oracle.jitter_tensor)
    pack_bytes          the frame store's float -> byte: clamp(rint(x * 255), 0, 255) in float32, and its inexact count

Sums are float64; everything that is compared bitwise is evaluated in float32 operation by operation.  Nothing here runs on
the device."""
import numpy as np
import torch

from oracle import jitter_tensor as jt
from oracle import resize as rz

CONTRAST = jt.CONTRAST


# ----------------------------------------------------------------------------------------------------------------------
# resize
def resample_axis_raw(img: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    """(acc >> 22) of one resize pass along `axis` as int64, NOT clipped: values < 0 or > 255 are LANCZOS overshoot"""
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    bounds, kk = rz.lanczos_plan(a.shape[0], out_size)
    out = np.empty((out_size,) + a.shape[1:], np.int64)
    for xx in range(out_size):
        xmin, xmax = (int(v) for v in bounds[xx])
        acc = np.full(a.shape[1:], 1 << (rz.PRECISION_BITS - 1), np.int64)
        for x in range(xmax):
            acc += a[xmin + x] * int(kk[xx, x])
        out[xx] = acc >> rz.PRECISION_BITS
    return np.moveaxis(out, 0, axis)


def to_planar(u8: np.ndarray) -> torch.Tensor:
    """(N,H,W,C) uint8 -> (N,C,H,W) float32"""
    return torch.from_numpy(np.ascontiguousarray((u8.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)))


# ----------------------------------------------------------------------------------------------------------------------
# float colour jitter
def sum_blocks(hw: int) -> int:
    return min(max((hw + 1023) // 1024, 1), 64)


def adds_per_thread(hw: int) -> int:
    """the most pixels one thread of the sum pass adds up"""
    return -(-hw // (sum_blocks(hw) * 256))


def partition_sums(gray: torch.Tensor):
    """gray: the hw fp32 terms of one image -> (sums, sums of |term|), float64, one per block of the sum pass"""
    g = gray.reshape(-1).double()
    hw, nblk = g.numel(), sum_blocks(g.numel())
    block = (torch.arange(hw) // 256) % nblk            # i = b * 256 + t + k * nblk * 256
    s = torch.zeros(nblk, dtype=torch.float64).index_add_(0, block, g)
    a = torch.zeros(nblk, dtype=torch.float64).index_add_(0, block, g.abs())
    return s, a


def partial_bound(hw: int, abs_sums: torch.Tensor) -> torch.Tensor:
    """|fp32 block sum - exact| <= depth * 2^-24 * sum |term| (Higham, Accuracy and Stability, section 4.2): a term passes
    through at most adds_per_thread additions in its thread, 6 butterfly steps of the wave sum and 2 of the four-wave tree"""
    return (adds_per_thread(hw) + 8) * 2.0 ** -24 * abs_sums


def kernel_mean(partials: torch.Tensor, hw: int) -> torch.Tensor:
    """partials: the fp32 block sums of one image, in index order -> fp32 scalar tensor"""
    m = np.float32(0)
    for p in partials.detach().cpu().numpy().astype(np.float32):
        m = np.float32(m + p)
    return torch.tensor(np.float32(m / np.float32(hw)))


def chain_of(order):
    """the ops a record applies: up to four, ended by the first negative id"""
    out = []
    for op in list(order)[:4]:
        if op < 0:
            break
        out.append(int(op))
    return out


def gray_before_contrast(img: torch.Tensor, order, factors):
    """img (3,h,w) fp32 -> fp32 gray plane behind the ops in front of the FIRST contrast op, None without one"""
    ops = chain_of(order)
    if CONTRAST not in ops:
        return None
    x = img.unsqueeze(0)
    for op in ops[:ops.index(CONTRAST)]:
        x = jt.OPS[op](x, factors[op])
    return jt.rgb_to_grayscale(x)[0, 0]


def color_jitter_injected(img: torch.Tensor, order, factors, mean) -> torch.Tensor:
    """oracle.jitter_tensor.color_jitter on ONE image (3,h,w) whose contrast op blends with `mean` (an fp32 scalar tensor)
    instead of torch.mean of the gray plane.  A record that names contrast twice blends with the same mean twice: the kernels
    form one mean per image, in front of the first contrast op."""
    x = img.unsqueeze(0)
    for op in chain_of(order):
        if op == CONTRAST:
            x = jt._blend(x, mean.to(torch.float32).reshape(1, 1, 1, 1), factors[op])
        else:
            x = jt.OPS[op](x, factors[op])
    return x[0]


# ----------------------------------------------------------------------------------------------------------------------
# frame store
def pack_bytes(x: np.ndarray):
    """x float32 -> (bytes, inexact count).  fmax / fmin like the kernel's fmaxf / fminf: a NaN becomes 0"""
    x = np.asarray(x, np.float32)
    with np.errstate(all='ignore'):
        q = np.fmin(np.fmax(np.rint(x * np.float32(255)), np.float32(0)), np.float32(255))
        b = q.astype(np.uint8)
        back = b.astype(np.float32) / np.float32(255)
    return b, int(np.count_nonzero(back != x))
