"""Image-pyramid ingest on the GPU: uint8 frames uploaded once -> the ``('rgb', f, s)``
float pyramids of the sample dict, bit-identical to what the reference's datasets build with PIL
(``datasets/utils.py:62-66,154-163,213-215``: LANCZOS resize of every level from the previous one, ToTensor).

    pyr = ImagePyramid(192, 640)                    # model resolution, scales 0..3
    levels = pyr(frames_u8)                         # (N,Hraw,Wraw,3) uint8 on the GPU -> {s: (N,3,H>>s,W>>s) float32}

The tap plans (Pillow's double-precision Lanczos-3 weights in 22-bit fixed point) are computed once per size pair
by the library's host function and kept on the device; the kernels are integer multiply-accumulates.
``color_jitter`` applies the datasets' colour augmentation (``datasets/utils.py:236-259``: torchvision's brightness /
contrast / saturation / hue adjustments of PIL images in a drawn order) with Pillow's arithmetic, also bit-exact.
"""
import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from .ops import _p, _pa, _stream


class ImagePyramid:
    def __init__(self, height: int, width: int, scales: Sequence[int] = (0, 1, 2, 3)) -> None:
        self.height, self.width, self.scales = int(height), int(width), tuple(scales)
        self._plans: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor, int]] = {}

    def _plan(self, in_size: int, out_size: int, device: torch.device):
        key = (in_size, out_size, str(device))
        plan = self._plans.get(key)
        if plan is None:
            lib = _lib.get_lib()
            ksize = lib.cdll.clslam_lanczos_ksize(in_size, out_size)
            bounds = torch.empty(out_size, 2, dtype=torch.int32)
            coeffs = torch.empty(out_size, ksize, dtype=torch.int32)
            lib.call('clslam_lanczos_plan', in_size, out_size, bounds.data_ptr(), coeffs.data_ptr())   # host function
            plan = (bounds.to(device), coeffs.to(device), ksize)
            self._plans[key] = plan
        return plan

    def _resize(self, src: torch.Tensor, out_h: int, out_w: int, planar: torch.Tensor) -> torch.Tensor:
        """src (N,h,w,C) uint8 -> (N,out_h,out_w,C) uint8; planar receives ToTensor(result)."""
        N, h, w, Cc = src.shape
        lib = _lib.get_lib()
        cur = src
        if w != out_w:                                        # Pillow: horizontal pass first
            b, k, ks = self._plan(w, out_w, src.device)
            dst = torch.empty(N, h, out_w, Cc, dtype=torch.uint8, device=src.device)
            last = h == out_h
            lib.call('clslam_resize_pass_u8', _pa(cur, torch.uint8), _pa(dst, torch.uint8), _p(planar) if last else None,
                     _pa(b, torch.int32), _pa(k, torch.int32), ks, N, h, w, Cc, out_w, 1, _stream(src))
            cur = dst
        if h != out_h:
            b, k, ks = self._plan(h, out_h, src.device)
            dst = torch.empty(N, out_h, out_w, Cc, dtype=torch.uint8, device=src.device)
            lib.call('clslam_resize_pass_u8', _pa(cur, torch.uint8), _pa(dst, torch.uint8), _p(planar), _pa(b, torch.int32),
                     _pa(k, torch.int32), ks, N, h, out_w, Cc, out_h, 0, _stream(src))
            cur = dst
        if cur is src:                                        # already at the target size: ToTensor only
            lib.call('clslam_u8_to_planar_f32', _pa(src, torch.uint8), _p(planar), N, h, w, Cc, _stream(src))
        return cur

    def __call__(self, frames: torch.Tensor, return_u8: bool = False):
        """-> {scale: (N,C,h,w) float32}; with return_u8 also {scale: (N,h,w,C) uint8} (the reference jitters every
        level's uint8 image separately, kitti.py:345-347)."""
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] not in (1, 3, 4):
            raise _lib.ClslamError(f'ImagePyramid expects (N,H,W,C) uint8 frames, got {tuple(frames.shape)} {frames.dtype}')
        frames = frames.contiguous()
        N, Cc = frames.shape[0], frames.shape[-1]
        out: Dict[int, torch.Tensor] = {}
        out_u8: Dict[int, torch.Tensor] = {}
        cur = frames
        for s in range(max(self.scales) + 1):
            h, w = self.height >> s, self.width >> s
            planar = torch.empty(N, Cc, h, w, device=frames.device)
            cur = self._resize(cur, h, w, planar)
            if s in self.scales:
                out[s] = planar
                out_u8[s] = cur
        return (out, out_u8) if return_u8 else out


def to_tensor(frames: torch.Tensor) -> torch.Tensor:
    """ToTensor (datasets/utils.py:213-215) of (N,H,W,C) uint8 frames -> (N,C,H,W) float32 = byte / 255."""
    frames = frames.contiguous()
    N, H, W, Cc = frames.shape
    planar = torch.empty(N, Cc, H, W, device=frames.device)
    _lib.get_lib().call('clslam_u8_to_planar_f32', _pa(frames, torch.uint8), _p(planar), N, H, W, Cc, _stream(frames))
    return planar


BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def color_jitter(frames: torch.Tensor, order: Sequence[int], factors: Sequence[float]) -> torch.Tensor:
    """frames (N,H,W,3) uint8 on the library's device -> jittered copy.  ``order``: op ids in application order (as
    ``random.shuffle`` left them in get_random_color_jitter), ``factors`` = (brightness, contrast, saturation, hue)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise _lib.ClslamError(f'color_jitter expects (N,H,W,3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}')
    frames = frames.contiguous()
    N, H, W, _ = frames.shape
    out, scratch = torch.empty_like(frames), torch.empty_like(frames)
    lsum = torch.zeros(N, dtype=torch.int64, device=frames.device)
    order_c = (C.c_int * max(len(order), 1))(*[int(o) for o in order])
    factors_c = (C.c_double * 4)(*[float(f) for f in factors])
    _lib.get_lib().call('clslam_color_jitter_u8', _pa(frames, torch.uint8), _pa(out, torch.uint8), _pa(scratch, torch.uint8),
                        _pa(lsum, torch.int64), N, H, W, order_c, len(order), factors_c, _stream(frames))
    return out


# ======================================================================================================================
# The replay buffer's samples on the GPU (the path that runs on EVERY adapted frame: slam/slam.py:98 builds
# the buffer with do_augmentation=True, slam/replay_buffer.py:186-235 `get` -> :263-291 `_get`)
def jitter_params(draws, device) -> torch.Tensor:
    """draws: one (order, factors) per image -- op ids in application order and the four factors by op id, as
    get_random_color_jitter (datasets/utils.py:236-259) draws them -> the device records clslam_color_jitter_f32 reads."""
    import numpy as np
    rec = np.zeros(len(draws), dtype=[('order', np.int32, 4), ('f', np.float32, 4), ('omf', np.float32, 4)])
    for i, (order, factors) in enumerate(draws):
        o = [int(v) for v in order][:4]
        rec['order'][i] = o + [-1] * (4 - len(o))
        rec['f'][i] = [np.float32(float(v)) for v in factors]
        rec['omf'][i] = [np.float32(1.0 - float(v)) for v in factors]        # 1.0 - ratio in double, then a C float (torch)
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(device)


def color_jitter_tensor(images: torch.Tensor, params: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """images (N,3,h,w) float32 in [0,1] on the library's device, params = jitter_params(...) with N records: torchvision's
    tensor-path adjust_brightness / _contrast / _saturation / _hue chain per image (each with its own contrast mean)."""
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 3:
        raise _lib.ClslamError(f'color_jitter_tensor expects (N,3,h,w) float32 images, got {tuple(images.shape)} {images.dtype}')
    images = images.contiguous()
    N, _, h, w = images.shape
    if params.numel() != N * 48:
        raise _lib.ClslamError(f'color_jitter_tensor: {params.numel()} parameter bytes for {N} images (48 each)')
    lib = _lib.get_lib()
    out = torch.empty_like(images) if out is None else out
    partial = torch.empty(max(N, 1) * lib.cdll.clslam_color_jitter_f32_blocks(h, w), device=images.device)
    lib.call('clslam_color_jitter_f32', _p(images), _p(out), _pa(params, torch.uint8), _p(partial), N, h, w, _stream(images))
    return out


def draw_color_jitter(brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-.1, .1), rng=None):
    """The draws of datasets/utils.py:236-259 from Python's `random` IN THE REFERENCE'S ORDER (four uniforms, then the shuffle of
    the four-element transform list), so that a run seeded like the reference consumes the same random stream."""
    import random
    rng = random if rng is None else rng
    factors = [rng.uniform(*brightness), rng.uniform(*contrast), rng.uniform(*saturation), rng.uniform(*hue)]
    order = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
    rng.shuffle(order)
    return order, factors


class FrameStore:
    """Device-resident uint8 store of whole replay samples (include/clslam_hip.h, clslam_store_*).  When ``ReplayBuffer.add``
    (slam/replay_buffer.py:82-184) sees a sample, that sample already holds the un-augmented pyramid ``_get`` later rebuilds from
    the PNGs (replay_buffer.py:270-279 runs the dataset's own chain, datasets/kitti.py:249-259, datasets/utils.py:154-171): every
    value is fl32(b / 255) of a byte b, so the bytes are all a replayed sample needs.

    One slot = one sample: per frame (in ``frames`` order) and level (in ``scales`` order) a planar (3, H>>s, W>>s) uint8 block at
    a fixed offset (rounded up to 16 bytes).  ``store_bytes // slot_bytes`` slots, one tensor allocated on first use; keyed by the
    sample's .pkl file name; when full the OLDEST slot is reused (its sample falls back to the PNG path).  The pickled non-image
    entries of every sample stay on the host: a hit opens no file at all.  Every kernel runs on the caller's current stream: a
    slot is packed, reused and gathered on that one stream, so reuse needs no further ordering."""

    def __init__(self, height: int, width: int, scales: Sequence[int] = (0, 1, 2, 3), frames: Sequence[int] = (0, -1, 1),
                 store_bytes: int = 0, device=None) -> None:
        self.height, self.width, self.scales, self.frames = int(height), int(width), tuple(scales), tuple(frames)
        if len(self.scales) * len(self.frames) > _lib.STORE_MAX_PLANES:
            raise _lib.ClslamError(f'FrameStore: {len(self.frames)} frames x {len(self.scales)} levels, at most {_lib.STORE_MAX_PLANES}')
        self.device = torch.device('cuda' if device is None else device)
        self.sizes = [(self.height >> s, self.width >> s) for s in self.scales]
        self.offsets, off = [], 0                       # [frame index * levels + level index] -> bytes from the slot's start
        for _ in self.frames:
            for h, w in self.sizes:
                self.offsets.append(off)
                off += (3 * h * w + 15) // 16 * 16
        self.slot_bytes = off
        self.capacity = int(store_bytes) // self.slot_bytes
        self._data: Optional[torch.Tensor] = None
        self._stage: Optional[torch.Tensor] = None
        self._inexact: Optional[torch.Tensor] = None
        self._slots: Dict[str, int] = {}                # key -> slot, oldest first (dicts keep insertion order)
        self._free = list(range(self.capacity - 1, -1, -1))
        self._entries: Dict[str, Dict] = {}

    @staticmethod
    def key_of(filename) -> str:
        return os.fspath(filename)

    def __contains__(self, key) -> bool:
        return self.key_of(key) in self._slots

    def __len__(self) -> int:
        return len(self._slots)

    def _allocate(self) -> None:
        if self._data is None:
            self._data = torch.zeros(self.capacity * self.slot_bytes, dtype=torch.uint8, device=self.device)
            self._stage = torch.empty(self.slot_bytes, device=self.device)          # float staging of one sample's host planes
            self._inexact = torch.zeros(1, dtype=torch.int64, device=self.device)

    def add_sample(self, key, sample: Dict, entries: Optional[Dict] = None) -> bool:
        """Keep the ``('rgb', frame, scale)`` planes of `sample` (host tensors, pinned or not, or device tensors; (1,3,h,w) or
        (3,h,w) float32) under `key`, the sample's .pkl file.  `entries`: its non-image entries; None = read them from that file,
        once, now.  -> False when the store has no slot at all (then nothing is kept)."""
        key = self.key_of(key)
        if self.capacity <= 0:
            return False
        self._allocate()
        planes = []
        for fi, frame in enumerate(self.frames):
            for li, s in enumerate(self.scales):
                t, (h, w) = sample['rgb', frame, s], self.sizes[li]
                if t.dtype != torch.float32 or t.numel() != 3 * h * w or tuple(t.shape[-3:]) != (3, h, w):
                    raise _lib.ClslamError(f"FrameStore.add_sample: ('rgb', {frame}, {s}) is {tuple(t.shape)} {t.dtype}, expected "
                                           f'(1, 3, {h}, {w}) float32')
                if t.device != self._data.device or not t.is_contiguous():
                    o = self.offsets[fi * len(self.scales) + li]                 # floats here, bytes in the slot: 16-byte aligned
                    staged = self._stage[o:o + 3 * h * w]
                    staged.view(t.shape).copy_(t, non_blocking=True)             # one asynchronous copy per plane
                    t = staged
                planes.append(t)
        if entries is None:
            import pickle
            with open(key, 'rb') as f:
                entries = pickle.load(f)
        entries = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in entries.items()
                   if not (isinstance(k, tuple) and k[0] in ('rgb', 'rgb_aug'))}                      # ('rgb', frame): the PNG's path
        slot = self._slots.pop(key, None)
        if slot is None:
            if not self._free:
                oldest = next(iter(self._slots))
                self._free.append(self._slots.pop(oldest))
                del self._entries[oldest]
            slot = self._free.pop()
        ops.store_pack(planes, self.offsets, self._data[slot * self.slot_bytes:(slot + 1) * self.slot_bytes], self._inexact)
        self._slots[key], self._entries[key] = slot, entries
        return True

    def drop(self, key) -> None:
        key = self.key_of(key)
        slot = self._slots.pop(key, None)
        if slot is not None:
            self._free.append(slot)
            del self._entries[key]

    def entries(self, key) -> Dict:
        """a fresh copy of the sample's non-image entries (`_get` changes its dict, replay_buffer.py:286-290)"""
        return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in self._entries[self.key_of(key)].items()}

    def slot_of(self, key) -> int:
        return self._slots.get(self.key_of(key), -1)

    def inexact_pixels(self) -> int:
        """values packed so far that were no byte / 255 (0 for samples a dataset built).  Debug / test read: it synchronises."""
        return 0 if self._inexact is None else int(self._inexact.item())

    def gather(self, keys, params: Optional[torch.Tensor], rgb, aug, row0: int = 0) -> None:
        """rows row0 + i of the (rows, 3, h, w) tensors rgb[frame index * levels + level index] (and aug, with the jitter of
        params = jitter_params(...), one record per IMAGE; aug None: no jitter) <- the sample stored under keys[i]; a key that is
        None or not in the store leaves its rows untouched."""
        slots = [-1 if k is None else self.slot_of(k) for k in keys]
        if self._data is None or all(v < 0 for v in slots):
            return
        idx = torch.tensor([v for v in slots for _ in self.frames], dtype=torch.int32).to(self._data.device, non_blocking=True)
        ops.store_gather_jitter(self._data, self.slot_bytes, self.offsets, self.sizes, len(self.frames), idx, params, rgb, aug, row0)


class ReplaySampleBuilder:
    """What ``ReplayBuffer._get`` (slam/replay_buffer.py:263-291) builds per replayed sample -- PNG -> RGB, the LANCZOS pyramid level
    from level, ToTensor, one drawn colour jitter on every level -- with the pixels on the GPU: the host decodes the PNGs
    (Pillow, on a small thread pool: its decoder releases the GIL), the raw uint8 frames cross PCIe ONCE, pyramid and jitter are
    three kernels per level for all samples and frames of a minibatch.

        build = ReplaySampleBuilder(height, width, scales, frames, device)
        build.install(slam.replay_buffer, slam)       # the reference's Slam / ReplayBuffer objects, everything else unchanged
        samples = build.get_many(filenames)           # or by hand: the K samples of a frame in one go

    Non-image entries of the pickled sample (camera matrices, relative distances, index ...) are passed through unchanged.
    """

    def __init__(self, height: int, width: int, scales: Sequence[int] = (0, 1, 2, 3), frames: Sequence[int] = (0, -1, 1),
                 device=None, do_augmentation: bool = True, cache_frames: int = 0, cache_bytes: int = 256 << 20,
                 decode_threads: int = 16, store_bytes: int = 0) -> None:
        self.height, self.width, self.scales, self.frames = int(height), int(width), tuple(scales), tuple(frames)
        self.device = torch.device('cuda' if device is None else device)
        self.do_augmentation = bool(do_augmentation)
        # opt-in: keep the samples themselves as bytes in device memory (FrameStore): a sample seen by `add`, or decoded once,
        # is served without its PNGs.  0: no store, everything below behaves as without this argument.
        self.store = FrameStore(height, width, self.scales, self.frames, store_bytes, self.device) if store_bytes > 0 else None
        if self.store is not None and self.store.capacity < 1:
            raise _lib.ClslamError(f'store_bytes = {store_bytes} holds no sample ({self.store.slot_bytes} bytes each)')
        self.pyramid = ImagePyramid(height, width, tuple(range(max(self.scales) + 1)))
        # opt-in: keep the DECODED uint8 frames of the last `cache_frames` image files on the host (a replay buffer re-serves
        # the same few hundred samples: a 1241x376 PNG costs ~7 ms to decode, its 1.4 MB cost nothing to keep).  Bounded by
        # count AND by bytes (`cache_bytes`, page-locked memory on a GPU build): the oldest entries go first.
        self.cache_frames = int(cache_frames)
        self.cache_bytes = int(cache_bytes)
        self._cached_bytes = 0
        self._decoded: Dict = {}
        # The K x 3 PNGs of a minibatch are decoded concurrently: Image.open(...).convert('RGB') (replay_buffer.py:271) spends its
        # time in Pillow's C decoder with the GIL released.  0 / 1: in the calling thread, like the reference.
        self.decode_threads = int(decode_threads)
        self._pool = None

    # ------------------------------------------------------------------------------------------------------------------
    def install(self, replay_buffer, slam=None) -> 'ReplaySampleBuilder':
        """Switch the REFERENCE's objects to this builder -- instance attributes only, their classes stay untouched:

        * ``replay_buffer.get`` still runs the reference's own sampling code (slam/replay_buffer.py:186-227: the choice of the
          files is its business), but with ``_get`` recording the file names instead of decoding them one by one; the K samples
          are then built by ONE get_many() -- one upload, one pyramid / jitter pass -- and concatenated per key exactly like
          replay_buffer.py:229-233.  The colour-jitter draws come from Python's ``random`` in the reference's order (one draw
          per file, the sampler draws from its own numpy generator before any of them), so a seeded run consumes the same
          random streams.
        * ``replay_buffer._get`` (direct callers) becomes get_one.
        * with ``store_bytes > 0`` and a buffer that has an ``add``: ``replay_buffer.add`` still runs the reference's own add, then
          the file names that appeared in / vanished from ``online_filenames`` are added to / dropped from the frame store (the
          online sample holds the very planes `_get` would rebuild from the PNGs -- as long as the online dataset neither flips
          nor jitters its 'rgb' entries, which the reference's driver does not).
        Calling install() again is harmless: the buffer's own methods are kept on the buffer and wrapped afresh.
        * ``slam._cat_dict`` (slam/slam.py:300-309 joins the online sample, host tensors, with the replay minibatch) becomes
          cat_dict below: torch.cat refuses mixed devices, the online entries are uploaded first.
        """
        builder = self
        # the buffer's own bound methods are kept ON the buffer: a second install() (of this or another builder) wraps them, not
        # the wrappers of the first
        if not hasattr(replay_buffer, '_clslam_reference_get'):
            replay_buffer._clslam_reference_get = replay_buffer.get
        reference_get = replay_buffer._clslam_reference_get
        replay_buffer._get = self.get_one

        def get(*args, **kwargs):
            names = []

            def record(filename, include_batch=True):
                names.append((filename, include_batch))
                return {}                                 # nothing to concatenate: replay_buffer.py:229-233 loops over its keys
            replay_buffer._get = record
            try:
                stub = reference_get(*args, **kwargs)
            finally:
                replay_buffer._get = builder.get_one
            if not names:
                return stub
            if builder.store is not None and names[0][1]:
                return builder.get_batch([n for n, _ in names])
            datas = builder.get_many([n for n, _ in names], include_batch=names[0][1])
            out = datas[0]
            for data in datas[1:]:
                for key in out:
                    out[key] = torch.cat([out[key], data[key]])
            return out
        replay_buffer.get = get
        if self.store is not None and (hasattr(replay_buffer, 'add') or hasattr(replay_buffer, '_clslam_reference_add')):
            if not hasattr(replay_buffer, '_clslam_reference_add'):
                replay_buffer._clslam_reference_add = replay_buffer.add
            reference_add = replay_buffer._clslam_reference_add

            def add(sample, *args, **kwargs):
                # the reference's own add, unchanged (replay_buffer.py:82-184); what it did shows in online_filenames
                before = list(replay_buffer.online_filenames)
                out = reference_add(sample, *args, **kwargs)
                after = list(replay_buffer.online_filenames)
                for fn in before:
                    if fn not in after:
                        builder.store.drop(fn)
                for fn in after:
                    if fn not in before and builder._has_planes(sample):
                        builder.store.add_sample(fn, sample)
                return out
            replay_buffer.add = add
        elif hasattr(replay_buffer, '_clslam_reference_add'):          # a builder without a store after one with a store
            replay_buffer.add = replay_buffer._clslam_reference_add
        if slam is not None:
            slam._cat_dict = cat_dict
        return self

    def close(self) -> None:
        """shut the PNG decode pool down (idle threads otherwise live as long as the builder)"""
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def _has_planes(self, sample) -> bool:
        return all(('rgb', f, s) in sample for f in self.frames for s in self.scales)

    def _decode_file(self, path):
        import numpy as np
        from PIL import Image
        return torch.from_numpy(np.asarray(Image.open(path).convert('RGB')).copy())       # replay_buffer.py:271

    def _keep(self, key, img):
        if self.cache_frames <= 0:
            return img
        if self.device.type == 'cuda':
            img = img.pin_memory()                                  # page-locked ONCE (~40 ms): later uploads are asynchronous DMAs
        nbytes = img.numel()
        while self._decoded and (len(self._decoded) >= self.cache_frames or self._cached_bytes + nbytes > self.cache_bytes):
            old = self._decoded.pop(next(iter(self._decoded)))
            self._cached_bytes -= old.numel()
        if nbytes <= self.cache_bytes:
            self._decoded[key] = img
            self._cached_bytes += nbytes
        return img

    def _decode_all(self, paths):
        """decoded uint8 frames of `paths` (cache hits first, the misses concurrently)"""
        keys = [str(p) for p in paths]
        out = {k: self._decoded[k] for k in keys if k in self._decoded}
        misses = [k for k in dict.fromkeys(keys) if k not in out]
        if len(misses) > 1 and self.decode_threads > 1:
            if self._pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(max_workers=self.decode_threads, thread_name_prefix='clslam-png')
            imgs = list(self._pool.map(self._decode_file, misses))
        else:
            imgs = [self._decode_file(k) for k in misses]
        for k, img in zip(misses, imgs):
            out[k] = self._keep(k, img)
        return [out[k] for k in keys]

    def get_many(self, filenames, include_batch: bool = True, rng=None):
        """-> one dict per file, exactly the entries `_get(filename, include_batch)` returns."""
        import pickle

        if self.store is not None:
            keys, whole, singles = self._build_batch(filenames, rng)
            datas = []
            for i, single in enumerate(singles):
                data = dict(single)
                for k in keys:
                    data[k] = whole[k][1 + i:2 + i] if include_batch else whole[k][1 + i]
                if not include_batch:                                # replay_buffer.py:286-289
                    for key in single:
                        data[key] = data[key].squeeze(0)
                datas.append(data)
            return datas
        datas, paths, draws = [], [], []
        for fn in filenames:
            # the jitter is drawn BEFORE the file is read (replay_buffer.py:264-268): same random stream as the reference
            draw = draw_color_jitter(rng=rng) if self.do_augmentation else None
            with open(fn, 'rb') as f:
                data = pickle.load(f)
            datas.append(data)
            for frame in self.frames:
                paths.append(data['rgb', frame])
                draws.append(draw)
        if not paths:
            return []
        raws = self._decode_all(paths)
        if len({tuple(r.shape) for r in raws}) != 1:
            raise _lib.ClslamError('replay samples with different raw image sizes in one batch')
        # one device staging block, one asynchronous copy per (page-locked) frame
        stage = torch.empty((len(raws),) + tuple(raws[0].shape), dtype=torch.uint8, device=self.device)
        for i, r in enumerate(raws):
            stage[i].copy_(r, non_blocking=True)
        levels = self.pyramid(stage)                                 # {s: (n_img,3,h,w) float}, bit-exact vs Pillow
        aug = levels
        if self.do_augmentation:
            params = jitter_params(draws, self.device)
            aug = {s: color_jitter_tensor(levels[s], params) for s in self.scales}
        nf = len(self.frames)
        for i, data in enumerate(datas):
            for j, frame in enumerate(self.frames):
                k = i * nf + j
                for s in self.scales:
                    rgb, rga = levels[s][k], aug[s][k]
                    data['rgb', frame, s] = rgb.unsqueeze(0) if include_batch else rgb
                    data['rgb_aug', frame, s] = rga.unsqueeze(0) if include_batch else rga
                del data['rgb', frame]
            if not include_batch:                                # replay_buffer.py:286-289
                for key in data:
                    if not ('rgb' in key or 'rgb_aug' in key):
                        data[key] = data[key].squeeze(0)
        return datas

    def _build_batch(self, filenames, rng=None):
        """The K samples of `filenames` through the frame store -> (image keys in `_get`'s order, {key: (1 + K, 3, h, w) tensor
        whose rows 1.. are the samples}, the K dicts of non-image entries).  Hits are gathered from the store by two launches;
        misses take the PNG path, are copied into their rows and packed into the store (decoded at most once)."""
        import pickle
        store, K, nf = self.store, len(filenames), len(self.frames)
        singles, miss, draws = [], [], []
        for i, fn in enumerate(filenames):
            # the jitter is drawn first, hit or miss (replay_buffer.py:264-268): Python's random stream is the reference's
            draw = draw_color_jitter(rng=rng) if self.do_augmentation else None
            draws.extend([draw] * nf)
            if fn in store:
                singles.append(store.entries(fn))
            else:
                with open(fn, 'rb') as f:
                    data = pickle.load(f)
                miss.append((i, fn, [data.pop(('rgb', frame)) for frame in self.frames]))
                singles.append(data)
        # ONE allocation for the batch; every key is a contiguous (1 + K, 3, h, w) piece of it
        sizes = store.sizes
        per_row = sum(3 * h * w for h, w in sizes) * nf
        n_kinds = 2 if self.do_augmentation else 1
        block = torch.empty(n_kinds * (1 + K) * per_row, device=self.device)
        pieces, at = [], 0
        for _ in range(n_kinds * nf):
            for h, w in sizes:
                n = (1 + K) * 3 * h * w
                pieces.append(block[at:at + n].view(1 + K, 3, h, w))
                at += n
        rgb, aug = pieces[:nf * len(sizes)], (pieces[nf * len(sizes):] if self.do_augmentation else None)
        params = jitter_params(draws, self.device) if self.do_augmentation else None
        missed = {i for i, _, _ in miss}
        store.gather([None if i in missed else fn for i, fn in enumerate(filenames)], params, rgb, aug, row0=1)
        if miss:
            raws = self._decode_all([p for _, _, paths in miss for p in paths])
            if len({tuple(r.shape) for r in raws}) != 1:
                raise _lib.ClslamError('replay samples with different raw image sizes in one batch')
            stage = torch.empty((len(raws),) + tuple(raws[0].shape), dtype=torch.uint8, device=self.device)
            for i, r in enumerate(raws):
                stage[i].copy_(r, non_blocking=True)
            levels = self.pyramid(stage)
            if self.do_augmentation:
                pick = torch.tensor([i * nf + j for i, _, _ in miss for j in range(nf)], device=self.device)
                miss_params = params.view(-1, 48)[pick].reshape(-1)
                jit = {s: color_jitter_tensor(levels[s], miss_params) for s in self.scales}
            rows = torch.tensor([1 + i for i, _, _ in miss], device=self.device)
            for j in range(nf):
                for li, s in enumerate(self.scales):
                    rgb[j * len(sizes) + li].index_copy_(0, rows, levels[s][j::nf])
                    if self.do_augmentation:
                        aug[j * len(sizes) + li].index_copy_(0, rows, jit[s][j::nf])
            for m, (i, fn, _) in enumerate(miss):                      # after the gather (same stream): a reused slot was read
                store.add_sample(fn, {('rgb', frame, s): levels[s][m * nf + j] for j, frame in enumerate(self.frames)
                                      for s in self.scales}, entries=singles[i])
        keys, whole = [], {}
        for j, frame in enumerate(self.frames):
            for li, s in enumerate(self.scales):
                t = j * len(sizes) + li
                keys += [('rgb', frame, s), ('rgb_aug', frame, s)]
                whole['rgb', frame, s] = rgb[t]
                whole['rgb_aug', frame, s] = aug[t] if self.do_augmentation else rgb[t]
        return keys, whole, singles

    def get_batch(self, filenames, rng=None) -> Dict:
        """What ``ReplayBuffer.get`` returns for `filenames` (replay_buffer.py:229-233: the K dicts of `_get` concatenated key by
        key), with a frame store: every entry is rows 1.. of a freshly allocated (1 + K, ...) tensor, so that cat_dict() only has
        to fill row 0 with the online sample.  New tensors on every call."""
        if self.store is None:
            datas = self.get_many(filenames, rng=rng)
            return {k: torch.cat([d[k] for d in datas]) for k in datas[0]} if datas else {}
        if not len(filenames):
            return {}
        keys, whole, singles = self._build_batch(filenames, rng)
        out = {}
        for k in singles[0]:
            vals = [d[k] for d in singles]
            v0 = vals[0]
            if all(isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == 1 and v.shape == v0.shape and v.dtype == v0.dtype
                   and v.device == v0.device for v in vals):
                w = torch.empty((1 + len(vals),) + tuple(v0.shape[1:]), dtype=v0.dtype, device=v0.device)
                torch.cat(vals, out=w[1:])
                out[k] = _rows_of(w)
            else:
                out[k] = torch.cat(vals)
        for k in keys:
            out[k] = _rows_of(whole[k])
        return out

    def get_one(self, filename, include_batch: bool = True):
        """``ReplayBuffer._get(filename, include_batch=True)``"""
        return self.get_many([filename], include_batch)[0]


def _rows_of(whole: torch.Tensor) -> torch.Tensor:
    """whole[1:], remembering the tensor it is cut from: cat_dict() fills row 0 instead of concatenating"""
    rows = whole[1:]
    rows._clslam_whole = whole
    return rows


def cat_dict(online: Dict, replay: Dict, device=None) -> Dict:
    """slam/slam.py:300-309 (`_cat_dict`) for a replay dict whose image tensors already live on the GPU: entries present in both
    dicts are concatenated there (the online sample's entries are uploaded; torch.cat refuses mixed devices).  An entry that
    get_batch() cut from a (1 + K, ...) tensor is not concatenated: the online entry is copied into row 0 and that tensor is
    returned (it shares its rows 1.. with `replay`; a second cat_dict on the same `replay` overwrites row 0)."""
    out = {}
    for k in online:
        if k in replay:
            a, b = online[k], replay[k]
            whole = getattr(b, '_clslam_whole', None)
            if (whole is not None and a.shape[0] == 1 and a.shape[1:] == whole.shape[1:] and a.dtype == whole.dtype
                    and whole.shape[0] == b.shape[0] + 1 and whole.data_ptr() + whole.stride(0) * whole.element_size() == b.data_ptr()):
                whole[:1].copy_(a, non_blocking=True)
                out[k] = whole if device is None or whole.device == torch.device(device) else whole.to(device, non_blocking=True)
                continue
            dev = device if device is not None else (b.device if b.device.type != 'cpu' else a.device)
            out[k] = torch.cat([a.to(dev, non_blocking=True), b.to(dev, non_blocking=True)])
    return out


# ======================================================================================================================
# The driver's ONLINE sample on the GPU: `online_data = next(self.online_dataloader_iter)` (slam/slam.py:141) runs the dataset's
# __getitem__ (datasets/kitti.py:231-317) on the driver's thread in front of every frame -- three PNGs, three four-level LANCZOS
# chains, 24 ToTensor planes -- although sample t + 1 shares two of its three frames with sample t.
class FrameRing:
    """One uint8 allocation of `capacity` slots, one FRAME per slot: per level s of `scales` an interleaved (H>>s, W>>s, 3) image
    at a fixed offset, ``slot_bytes`` = sum of 3 * (H>>s) * (W>>s).  ``put`` builds a frame's pyramid once -- one
    clslam_resize_level_u8 launch per level, level 0 from the uploaded raw frame, level s from level s - 1 inside the slot
    (datasets/kitti.py:258, datasets/utils.py:160-163) -- and ``gather`` writes the float planes of a sample from the slots of its
    frames in one launch.  The oldest slot is reused first.  Every kernel runs on the caller's current stream."""

    def __init__(self, height: int, width: int, scales: Sequence[int] = (0, 1, 2, 3), capacity: int = 8, device=None) -> None:
        self.height, self.width, self.scales = int(height), int(width), tuple(int(s) for s in scales)
        if self.scales != tuple(range(len(self.scales))) or not self.scales:
            raise ValueError(f'FrameRing: scales = {tuple(scales)}; every level is built from the one above it, so they must be 0, 1, 2, ...')
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError(f'FrameRing: capacity = {capacity}')
        self.device = torch.device('cuda' if device is None else device)
        self.sizes = [(self.height >> s, self.width >> s) for s in self.scales]
        self.offsets, off = [], 0
        for h, w in self.sizes:
            self.offsets.append(off)
            off += 3 * h * w
        self.slot_bytes = off
        self._data = torch.zeros(self.capacity * self.slot_bytes, dtype=torch.uint8, device=self.device)
        self._slots: Dict = {}                          # key -> slot, oldest first
        self._free = list(range(self.capacity - 1, -1, -1))
        self._pyramid = ImagePyramid(height, width, self.scales)       # its cache of tap plans

    def __contains__(self, key) -> bool:
        return key in self._slots

    def __len__(self) -> int:
        return len(self._slots)

    def slot_of(self, key) -> int:
        return self._slots.get(key, -1)

    def level(self, key, scale: int) -> torch.Tensor:
        """the (h, w, 3) uint8 image of `key` at `scale`: a view into the ring (debug / test read)"""
        li = self.scales.index(scale)
        h, w = self.sizes[li]
        at = self._slots[key] * self.slot_bytes + self.offsets[li]
        return self._data[at:at + 3 * h * w].view(h, w, 3)

    def put(self, key, raw_u8: torch.Tensor, keep=()) -> int:
        """raw_u8: the decoded frame, (Hraw, Wraw, 3) uint8 on the ring's device -> its slot.  The oldest slot whose key is not in
        `keep` (the other frames of the sample being assembled) is reused when none is free."""
        if raw_u8.dtype != torch.uint8 or raw_u8.dim() != 3 or raw_u8.shape[-1] != 3:
            raise _lib.ClslamError(f'FrameRing.put expects an (H,W,3) uint8 frame, got {tuple(raw_u8.shape)} {raw_u8.dtype}')
        slot = self._slots.pop(key, None)
        if slot is None:
            if not self._free:
                oldest = next((k for k in self._slots if k not in keep), None)
                if oldest is None:
                    raise _lib.ClslamError(f'FrameRing: all {self.capacity} slots are held by the sample being assembled')
                self._free.append(self._slots.pop(oldest))
            slot = self._free.pop()
        base = slot * self.slot_bytes
        src = raw_u8.contiguous().unsqueeze(0)
        for li, (h, w) in enumerate(self.sizes):
            dst = self._data[base + self.offsets[li]:base + self.offsets[li] + 3 * h * w]
            _, sh, sw, _ = src.shape
            ops.resize_level_u8(src, dst, h, w, self._pyramid._plan(sw, w, self.device) if sw != w else None,
                                self._pyramid._plan(sh, h, self.device) if sh != h else None)
            src = dst.view(1, h, w, 3)
        self._slots[key] = slot
        return slot

    def gather(self, keys, rgb, aug) -> None:
        """rgb / aug [frame index * levels + level index] (contiguous float tensors of 3 * h * w values) <- byte / 255 of the frames
        stored under `keys`, one launch"""
        ops.ring_gather(self._data, self.slot_bytes, self.offsets, self.sizes, [self._slots[k] for k in keys], rgb, aug)


class _OnlineIterator:
    """what iter(DataLoader(dataset, batch_size=1)) is to slam/slam.py:141: sample(0), sample(1), ..., then StopIteration"""

    def __init__(self, builder: 'OnlineSampleBuilder') -> None:
        self._builder, self._next, self._len = builder, 0, len(builder.dataset)

    def __iter__(self):
        return self

    def __len__(self) -> int:
        return self._len

    def __next__(self):
        if self._next >= self._len:
            raise StopIteration
        self._next += 1
        return self._builder.sample(self._next - 1)


class OnlineSampleBuilder:
    """The reference driver's online sample with its pixels on the GPU.

        online = OnlineSampleBuilder(slam.online_dataset)        # the reference's Kitti / Robotcar object
        online.install(slam)                                     # slam.step() runs unchanged

    ``sample(i)`` is ``default_collate([dataset[i]])`` (what the driver's DataLoader(batch_size=1) yields) with the 24 image entries
    as fresh (1,3,h,w) float32 tensors on `device`, bitwise the dataset's; the other entries are formed from the dataset's own
    attributes like datasets/kitti.py:263-274,302-314 and `_preprocess` (:348-353) form them and stay on the host.  Each PNG is
    decoded once (ahead of time on a small thread pool: Pillow's decoder releases the GIL), uploaded once from page-locked memory,
    its pyramid is built once into a FrameRing slot by four launches, and a sample is one launch.

    Covers the driver's configuration (slam/slam.py:44-72): no augmentation, one view, neither masks nor ground-truth depth;
    anything else raises ValueError here, not at the first frame.  Kitti and Robotcar expose the same attributes
    (datasets/robotcar.py:220-270 is kitti.py:231-317 without the depth branch) and go through the same code.

    ``camera_model`` (a clslam_hip.robotcar.CameraModel): the dataset's PNGs are RobotCar's RAW frames, as downloaded.  Each is
    read as one channel, uploaded, and demosaiced and undistorted by one fused launch in front of ``FrameRing.put``, so the
    reference's offline pass (datasets/robotcar.py:493-548) is not needed.  The frame keeps its size; the dataset's camera matrix
    (normalised by that size, robotcar.py _load_camera_calibration) is used as it is."""

    _NEEDS = ('frame_ids', 'scales', 'height', 'width', 'camera_matrix', 'relative_distances', '_pre_getitem', '_scale_camera_matrix')

    def __init__(self, dataset, device='cuda', ring_frames: int = 8, prefetch: int = 2, decode_threads: int = 2,
                 camera_model=None) -> None:
        for name in self._NEEDS:
            if not hasattr(dataset, name):
                raise ValueError(f'OnlineSampleBuilder: the dataset has no `{name}` (a datasets.Kitti / Robotcar object is expected)')
        if getattr(dataset, 'do_augmentation', False):
            raise ValueError('OnlineSampleBuilder: do_augmentation=True (flip and colour jitter) is not covered; the driver builds its '
                             'online dataset with do_augmentation=False')
        if getattr(dataset, 'with_mask', False):
            raise ValueError('OnlineSampleBuilder: with_mask=True is not covered')
        if getattr(dataset, 'with_depth', False):
            raise ValueError('OnlineSampleBuilder: with_depth=True is not covered')
        if len(getattr(dataset, 'views', ('left',))) != 1:
            raise ValueError(f'OnlineSampleBuilder: views={tuple(dataset.views)}: one view is covered')
        scales = tuple(dataset.scales)
        if not scales or scales != tuple(range(len(scales))):
            raise ValueError(f'OnlineSampleBuilder: scales={scales}: the pyramid levels 0, 1, 2, ... are covered')
        self.dataset = dataset
        self.frame_ids = tuple(dataset.frame_ids)
        self.scales = scales
        if len(self.frame_ids) * len(scales) > _lib.STORE_MAX_PLANES:
            raise ValueError(f'OnlineSampleBuilder: frame_ids={self.frame_ids} x scales={scales}: at most {_lib.STORE_MAX_PLANES} planes')
        if int(ring_frames) < len(self.frame_ids):
            raise ValueError(f'OnlineSampleBuilder: ring_frames={ring_frames} cannot hold the {len(self.frame_ids)} frames of one sample')
        self.device = torch.device(device)
        self.ring = FrameRing(dataset.height, dataset.width, scales, ring_frames, self.device)
        self.prefetch = max(int(prefetch), 0)
        self.decode_threads = max(int(decode_threads), 1)
        self._pool = None
        self._decoded: Dict = {}                        # path -> Future of the decoded (page-locked) frame, oldest first
        self._matrices = None
        self._per_sample = sum(3 * h * w for h, w in self.ring.sizes) * len(self.frame_ids)
        # a robotcar.CameraModel: the dataset's files are RAW frames (one-channel Bayer mosaics, distorted), rectified on the device
        self.camera_model = camera_model

    # ------------------------------------------------------------------------------------------------------------------
    def _decode_file(self, path) -> torch.Tensor:
        import numpy as np
        from PIL import Image
        if self.camera_model is None:
            img = torch.from_numpy(np.asarray(Image.open(path).convert('RGB')).copy())        # datasets/kitti.py:249
        else:
            img = torch.from_numpy(np.array(Image.open(path)))                                # the mosaic: a third of the bytes
            if img.dim() != 2 or img.dtype is not torch.uint8:
                raise ValueError(f'OnlineSampleBuilder: camera_model is set, but {path} is no one-channel 8-bit raw frame '
                                 f'({tuple(img.shape)} {img.dtype})')
        return img.pin_memory() if self.device.type == 'cuda' else img

    def _submit(self, path) -> None:
        if path in self._decoded or path in self.ring:
            return
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.decode_threads, thread_name_prefix='clslam-online-png')
        while len(self._decoded) >= self.prefetch + 3:                    # the bound on decoded frames held
            self._decoded.pop(next(iter(self._decoded))).cancel()
        self._decoded[path] = self._pool.submit(self._decode_file, path)

    def _paths(self, index: int):
        img_filenames, _, shifted, _, _ = self.dataset._pre_getitem(index)
        return [str(img_filenames[shifted + f]) for f in self.frame_ids], shifted

    def _ensure(self, paths) -> None:
        """every frame of `paths` into the ring: decode (the misses of one sample concurrently), one pinned upload, four launches"""
        misses = [p for p in dict.fromkeys(paths) if p not in self.ring]
        if len(misses) > 1 and self.decode_threads > 1:
            for p in misses:
                self._submit(p)
        for p in misses:
            fut = self._decoded.pop(p, None)
            raw = self._decode_file(p) if fut is None or fut.cancelled() else fut.result()
            raw = raw.to(self.device, non_blocking=True)
            if self.camera_model is not None:                             # datasets/robotcar.py:522-548 in one launch
                raw = self.camera_model.rectify(raw)
            self.ring.put(p, raw, keep=paths)

    def _host_item(self, shifted: int) -> Dict:
        """the non-image entries of dataset[index], un-collated, in the dataset's key order"""
        ds = self.dataset
        if self._matrices is None:                                        # kitti.py:263-267: the same matrices for every index
            self._matrices = [ds._scale_camera_matrix(ds.camera_matrix, s) for s in range(len(self.scales))]
        item = {('index'): shifted}
        for s, (camera_matrix, inv_camera_matrix) in enumerate(self._matrices):
            item['camera_matrix', s] = torch.from_numpy(camera_matrix.copy())                # _preprocess :348-349
            item['inv_camera_matrix', s] = torch.from_numpy(inv_camera_matrix.copy())
        for f in self.frame_ids[1:]:
            item['relative_distance', f] = ds.relative_distances[shifted + f]                # kitti.py:303-304
        if getattr(ds, 'include_poses', False):
            for f in self.frame_ids[1:]:                                                     # kitti.py:306-314, ToTensor of a (4,4) array
                item['relative_pose', f] = _array_to_tensor(ds.relative_poses[shifted + f])
                item['absolute_pose', f] = _array_to_tensor(ds.global_poses[shifted + f])
        return item

    def _build(self, index: int, collated: bool) -> Dict:
        from torch.utils.data import default_collate
        paths, shifted = self._paths(index)
        self._ensure(paths)
        block = torch.empty(2 * self._per_sample, device=self.device)
        shape = (lambda h, w: (1, 3, h, w)) if collated else (lambda h, w: (3, h, w))
        rgb, aug, at = [], [], 0
        for group in (rgb, aug):
            for _ in self.frame_ids:
                for h, w in self.ring.sizes:
                    group.append(block[at:at + 3 * h * w].view(shape(h, w)))
                    at += 3 * h * w
        self.ring.gather(paths, rgb, aug)
        host = self._host_item(shifted)
        if collated:
            host = default_collate([host])
        # the dataset's key order: index, level 0 of every frame, the host entries, the lower levels, then every rgb_aug
        nl = len(self.scales)
        item = {('index'): host.pop('index')}
        for j, f in enumerate(self.frame_ids):
            item['rgb', f, 0] = rgb[j * nl]
        item.update(host)
        for j, f in enumerate(self.frame_ids):
            for li in range(1, nl):
                item['rgb', f, self.scales[li]] = rgb[j * nl + li]
        for key in [k for k in item if isinstance(k, tuple) and k[0] == 'rgb']:
            _, f, s = key
            item['rgb_aug', f, s] = aug[self.frame_ids.index(f) * nl + self.scales.index(s)]
        return item

    def sample(self, index: int) -> Dict:
        """the collated dict the driver gets from its DataLoader(batch_size=1) for `index`"""
        out = self._build(index, collated=True)
        n = len(self.dataset)
        for nxt in range(index + 1, min(index + 1 + self.prefetch, n)):      # decode ahead: the frames of the next samples
            for p in self._paths(nxt)[0]:
                self._submit(p)
        return out

    def item(self, index: int) -> Dict:
        """``dataset[index]`` (un-collated): what slam/slam.py:228 reads for a loop-closure candidate"""
        return self._build(index, collated=False)

    # ------------------------------------------------------------------------------------------------------------------
    def install(self, slam) -> 'OnlineSampleBuilder':
        """Switch the REFERENCE's driver object over: ``slam.online_dataloader_iter`` becomes an iterator over sample(0), sample(1),
        ... (slam/slam.py:141), and ``slam.online_dataset`` gets a subclass of its own class, created here, whose __getitem__ is
        item() (slam/slam.py:228: a dunder is looked up on the type, not on the instance).  The dataset's class itself and every
        other instance keep their code.  Calling install() again rewinds the iterator and does not nest the subclass."""
        if slam.online_dataset is not self.dataset:
            raise ValueError('OnlineSampleBuilder.install: slam.online_dataset is not the dataset this builder was made for')
        builder = self
        base = getattr(type(self.dataset), '_clslam_online_base', type(self.dataset))

        def getitem(_self, index):
            return builder.item(index)
        self.dataset.__class__ = type(base.__name__, (base,), {'__getitem__': getitem, '_clslam_online_base': base,
                                                               '__module__': base.__module__})
        slam.online_dataloader_iter = _OnlineIterator(self)
        return self

    def close(self) -> None:
        """shut the PNG decode pool down and forget the frames decoded ahead"""
        for fut in self._decoded.values():
            fut.cancel()
        self._decoded.clear()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None


def _array_to_tensor(value) -> torch.Tensor:
    """torchvision's ToTensor of a 2-D numpy array that is no uint8 image (datasets/utils.py:213-215 on a (4,4) pose): (1,4,4),
    dtype kept, nothing scaled"""
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(np.asarray(value)[None]))
