"""The frame store of the replay ingest (clslam_hip.ingest.FrameStore, clslam_store_pack / clslam_store_gather_jitter): samples kept
as bytes in device memory and served without their PNGs.  The claims: a byte survives pack -> gather bitwise, `rgb_aug` from the
store is BITWISE what to_tensor + clslam_color_jitter_f32 give on the same bytes, and a builder with a store returns bitwise what
the PNG path returns (which tests/test_replay_ingest.py holds against the reference's own `_get`)."""
import os
import pickle
import random
from pathlib import Path

import numpy as np
import pytest
import torch

from clslam_hip import ingest
from emu_util import BACKENDS, use_backend

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'replay_get.npz'
FRAMES, SCALES = (0, -1, 1), (0, 1, 2, 3)

# the contrast op (id 1) first, last, in the middle, absent
DRAWS = [([1, 0, 2, 3], [1.13, 0.84, 0.91, 0.06]), ([3, 2, 0, 1], [0.88, 1.17, 1.09, -0.08]),
         ([2, 1, 3, 0], [0.95, 1.06, 0.83, 0.031]), ([0, 3, 2], [1.19, 1.0, 1.12, -0.1])]


def _byte_sample(gen, H, W, dev):
    """random bytes per frame and level -> ({('rgb', f, s): (1,3,h,w) float on dev}, {(f, s): (1,h,w,3) uint8 on dev})"""
    sample, raw = {}, {}
    for f in FRAMES:
        for s in SCALES:
            u8 = torch.randint(0, 256, (1, H >> s, W >> s, 3), generator=gen, dtype=torch.uint8).to(dev)
            raw[f, s] = u8
            sample['rgb', f, s] = ingest.to_tensor(u8)
    return sample, raw


@pytest.mark.parametrize('W', [80, 42])
@pytest.mark.parametrize('backend', BACKENDS)
def test_pack_and_gather_are_bitwise_on_ragged_shapes(backend, W):
    """48 x 80: level 0 has 3840 pixels = 4 blocks of the sum pass, level 3 has 60 = less than one wave.  48 x 42: level sizes
    2016 / 504 / 120 / 30 pixels -- widths that are no multiple of 4, a block that is no multiple of 16 bytes, a level without
    any vector part.  Three rows gathered from two slots (permuted, one repeated) behind an untouched row 0."""
    dev = use_backend(backend)
    H = 48
    gen = torch.Generator().manual_seed(W)
    store = ingest.FrameStore(H, W, SCALES, FRAMES, store_bytes=1 << 20, device=dev)
    assert store.slot_bytes % 16 == 0 and store.slot_bytes >= 3 * sum(3 * (H >> s) * (W >> s) for s in SCALES)
    samples = [_byte_sample(gen, H, W, dev) for _ in range(2)]
    for i, (sample, _) in enumerate(samples):
        # host planes (staged by one copy each) for one sample, device planes for the other
        planes = {k: v.cpu() for k, v in sample.items()} if i == 0 else sample
        assert store.add_sample(f's{i}', planes, entries={})
    assert len(store) == 2 and 's0' in store and 's1' in store and 's2' not in store
    order = [1, 0, 1]
    n_img = len(order) * len(FRAMES)
    draws = [DRAWS[i % 4] for i in range(n_img)]
    params = ingest.jitter_params(draws, dev)
    rows = 1 + len(order)
    rgb = [torch.full((rows, 3, H >> s, W >> s), -7.0, device=dev) for _ in FRAMES for s in SCALES]
    aug = [torch.full((rows, 3, H >> s, W >> s), -7.0, device=dev) for _ in FRAMES for s in SCALES]
    store.gather([f's{i}' for i in order], params, rgb, aug, row0=1)
    for li, s in enumerate(SCALES):
        # the same bytes through the existing entry points: ToTensor, then ONE clslam_color_jitter_f32 launch over the images
        images = torch.cat([ingest.to_tensor(samples[i][1][f, s]) for i in order for f in FRAMES])
        jittered = ingest.color_jitter_tensor(images, params)
        for j in range(len(FRAMES)):
            got_rgb, got_aug = rgb[j * len(SCALES) + li], aug[j * len(SCALES) + li]
            assert torch.equal(got_rgb[1:], images[j::len(FRAMES)]), (s, j)
            assert torch.equal(got_aug[1:], jittered[j::len(FRAMES)]), (s, j)
            assert bool((got_rgb[0] == -7.0).all()) and bool((got_aug[0] == -7.0).all()), (s, j)
    assert store.inexact_pixels() == 0
    # a key that is not stored leaves its rows alone
    store.gather(['s0', 'nowhere'], ingest.jitter_params(draws[:6], dev), rgb, aug, row0=1)
    assert torch.equal(aug[0][2], ingest.color_jitter_tensor(ingest.to_tensor(samples[0][1][0, 0]), params[3 * 48:4 * 48])[0])
    # one value moved to the next float above fl32(7 / 255): counted, exactly once
    off = dict(samples[0][0])
    plane = off['rgb', -1, 2].clone()
    seven = torch.tensor(7.0) / 255
    plane.view(-1)[11] = torch.nextafter(seven, torch.tensor(1.0)).to(dev)
    off['rgb', -1, 2] = plane
    store.add_sample('s0', off, entries={})
    assert store.inexact_pixels() == 1 and len(store) == 2


@pytest.mark.parametrize('backend', BACKENDS)
def test_every_byte_value_survives_the_round_trip(backend):
    """x = fl32(b / 255) -> b = rint(x * 255) -> fl32(b / 255), bitwise, for all 256 bytes (the claim the store rests on)"""
    dev = use_backend(backend)
    store = ingest.FrameStore(16, 16, (0,), (0,), store_bytes=4096, device=dev)
    assert store.capacity == 4096 // 768
    u8 = (torch.arange(768) % 256).to(torch.uint8).reshape(1, 16, 16, 3).to(dev)
    x = ingest.to_tensor(u8)
    want = (u8.cpu().permute(0, 3, 1, 2).to(torch.float32) / 255)
    assert torch.equal(x.cpu(), want)
    store.add_sample('all', {('rgb', 0, 0): x}, entries={})
    out = [torch.zeros(1, 3, 16, 16, device=dev)]
    store.gather(['all'], None, out, None, row0=0)
    assert torch.equal(out[0].cpu(), want) and store.inexact_pixels() == 0
    assert sorted(set((out[0].cpu() * 255).round().to(torch.int64).view(-1).tolist())) == list(range(256))


def _write_samples(tmp_path, z, extra=0):
    """the fixture's samples as .pkl + PNG files, like tests/test_replay_ingest.py; `extra` more made of flipped raw frames"""
    from PIL import Image
    frames = [int(f) for f in z['frames']]
    files, pngs = [], []
    n = int(z['n_samples'])
    for i in range(n + extra):
        sample = {('camera_matrix', 0): torch.from_numpy(z['camera_matrix']).clone(), ('index',): torch.tensor([i])}
        mine = []
        for f in frames:
            raw = z[f'raw_{i}_{f}'] if i < n else np.ascontiguousarray(z[f'raw_{i % n}_{f}'][::-1, ::-1])
            png = tmp_path / f's{i}_f{f}.png'
            Image.fromarray(raw).save(png)
            sample['rgb', f] = png
            mine.append(png)
        fn = tmp_path / f'kitti_{i:05}.pkl'
        with open(fn, 'wb') as fh:
            pickle.dump(sample, fh)
        files.append(fn)
        pngs.append(mine)
    return files, pngs


def _geometry(z):
    return int(z['height']), int(z['width']), [int(s) for s in z['scales']], [int(f) for f in z['frames']]


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].device == b[k].device, k
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_builder_with_a_store_matches_the_reference_fixture_without_the_pngs(backend, tmp_path):
    """every sample built once by the PNG path, its 'rgb' planes added as HOST tensors, the PNGs deleted: get_many under the same
    seed returns the fixture ('rgb' bit-exact, 'rgb_aug' <= 2e-6 as tests/test_replay_ingest.py holds the PNG path) and BITWISE
    what the PNG path returned, leaves Python's random stream where the PNG path leaves it, and opens no image file."""
    dev = use_backend(backend)
    z = np.load(GOLDEN, allow_pickle=False)
    H, W, scales, frames = _geometry(z)
    files, pngs = _write_samples(tmp_path, z)
    plain = ingest.ReplaySampleBuilder(H, W, scales, frames, device=dev)
    random.seed(int(z['seed']))
    by_png = plain.get_many(files)
    after_png = random.random()
    build = ingest.ReplaySampleBuilder(H, W, scales, frames, device=dev, store_bytes=8 << 20)
    for fn, data in zip(files, by_png):
        assert build.store.add_sample(fn, {k: v.cpu() for k, v in data.items() if k[0] == 'rgb'})
    assert build.store.inexact_pixels() == 0 and len(build.store) == len(files)
    for png in sum(pngs, []):
        os.remove(png)
    random.seed(int(z['seed']))
    by_store = build.get_many(files)
    assert random.random() == after_png
    for i, (a, b) in enumerate(zip(by_png, by_store)):
        _same(a, b)
        want_keys = {tuple(k.split('|')[1:]) for k in z.files if k.startswith(f'out{i}|')}
        assert {tuple(str(p) for p in k) for k in b} == want_keys
        for k in b:
            ref = torch.from_numpy(z['|'.join([f'out{i}'] + [str(p) for p in k])])
            assert tuple(b[k].shape) == tuple(ref.shape), k
            if k[0] == 'rgb_aug':
                assert float((b[k].cpu() - ref).abs().max()) <= 2e-6, k
            else:
                assert torch.equal(b[k].cpu(), ref), k
        assert b['rgb_aug', 0, 0].device.type == dev.type
    # one by one and without the batch dimension, like `_get(filename, include_batch=False)`
    random.seed(int(z['seed']))
    one = build.get_one(files[0], include_batch=False)
    assert one['rgb', 0, 0].shape == (3, H, W) and torch.equal(one['rgb_aug', 0, 0], by_png[0]['rgb_aug', 0, 0][0])
    assert one['index',].shape == () and one['camera_matrix', 0].shape == (4, 4)


class _BufferShapedLikeTheReference:
    """slam/replay_buffer.py's ReplayBuffer as far as install() touches it: `add` (:82-184) writes the sample's .pkl, appends it to
    `online_filenames` and, over `buffer_size`, removes one file name (here: the oldest); `get` (:186-235) chooses files, calls
    `self._get(filename)` per file and concatenates key by key."""

    def __init__(self, storage_dir, buffer_size):
        self.storage_dir, self.buffer_size, self.online_filenames, self.pick, self.calls = storage_dir, buffer_size, [], [], 0

    def add(self, sample, sample_filenames, image_features=None, verbose=False):
        index = sample['index',].item()
        filename = self.storage_dir / f'kitti_{index:>05}.pkl'
        data = {key: value for key, value in sample.items() if 'index' in key or 'camera_matrix' in key}
        data['rgb', -1], data['rgb', 0], data['rgb', 1] = sample_filenames['images']
        with open(filename, 'wb') as f:
            pickle.dump(data, f, pickle.HIGHEST_PROTOCOL)
        self.online_filenames.append(filename)
        if len(self.online_filenames) > self.buffer_size:
            os.remove(self.online_filenames[0])
            self.online_filenames.remove(self.online_filenames[0])

    def _get(self, filename, include_batch=True):
        self.calls += 1
        raise AssertionError('the reference _get must not run once a builder is installed')

    def get(self, sample, image_features=None):
        filenames = [self.online_filenames[i] for i in self.pick]
        return_data = self._get(filenames[0])
        for filename in filenames[1:]:
            data = self._get(filename)
            for key in return_data:
                return_data[key] = torch.cat([return_data[key], data[key]])
        return return_data


class _SlamShapedLikeTheReference:
    @staticmethod
    def _cat_dict(a, b):                 # slam/slam.py:300-309
        return {k: torch.cat([a[k], b[k]]) for k in a if k in b}


def _online_samples(tmp_path, z, dev, extra):
    """three online samples as the driver holds them at `add` time: host tensors, the pyramid `_get` would build, and the names
    of their PNGs in the order replay_buffer.py:172-174 reads them (-1, 0, 1)"""
    H, W, scales, frames = _geometry(z)
    files, pngs = _write_samples(tmp_path / 'src', z, extra)
    plain = ingest.ReplaySampleBuilder(H, W, scales, frames, device=dev)
    samples = []
    for fn, mine in zip(files, pngs):
        data = plain.get_many([fn])[0]
        sample = {k: v.cpu() for k, v in data.items() if k[0] != 'rgb_aug'}
        names = dict(zip(frames, mine))
        samples.append((sample, {'index': int(sample['index',]), 'images': [names[-1], names[0], names[1]]}))
    return plain, samples, pngs


def _by_png(plain, filenames, seed):
    random.seed(seed)
    datas = plain.get_many(filenames)
    return {k: torch.cat([d[k] for d in datas]) for k in datas[0]}


@pytest.mark.parametrize('backend', BACKENDS)
def test_install_with_a_store_serves_added_samples_from_the_store(backend, tmp_path):
    dev = use_backend(backend)
    z = np.load(GOLDEN, allow_pickle=False)
    H, W, scales, frames = _geometry(z)
    (tmp_path / 'src').mkdir()
    (tmp_path / 'buf').mkdir()
    plain, samples, pngs = _online_samples(tmp_path, z, dev, extra=1)
    buf, slam = _BufferShapedLikeTheReference(tmp_path / 'buf', buffer_size=3), _SlamShapedLikeTheReference()
    slot_bytes = ingest.FrameStore(H, W, scales, frames, device=dev).slot_bytes
    build = ingest.ReplaySampleBuilder(H, W, scales, frames, device=dev, decode_threads=2, store_bytes=2 * slot_bytes + 100)
    store = build.store
    assert store.capacity == 2 and slot_bytes == 3 * 3 * sum((H >> s) * (W >> s) for s in scales)
    packs = []
    real_add_sample = store.add_sample
    store.add_sample = lambda key, *a, **kw: (packs.append(os.fspath(key)), real_add_sample(key, *a, **kw))[1]
    # installed twice: every sample is still stored once
    assert build.install(buf, slam) is build and build.install(buf, slam) is build
    for sample, names in samples:
        buf.add(sample, names)
    files = list(buf.online_filenames)
    assert packs == [os.fspath(f) for f in files] and buf.calls == 0
    # capacity 2, three adds: the oldest sample left the store and takes the PNG path, the batch is mixed -- and bitwise the PNG path's
    assert len(store) == 2 and files[0] not in store and files[1] in store and files[2] in store
    buf.pick = [2, 0, 1]
    want = _by_png(plain, [files[i] for i in buf.pick], 21)
    random.seed(21)
    got = buf.get(samples[0][0])
    after = random.random()
    _same(want, got)
    random.seed(21)
    plain.get_many([files[i] for i in buf.pick])
    assert random.random() == after
    # ... the miss was packed (in place of the then oldest, sample 1): served again with its PNGs gone
    assert files[0] in store and files[1] not in store and len(store) == 2 and packs[-1] == os.fspath(files[0])
    buf.pick = [0, 2]
    want = _by_png(plain, [files[0], files[2]], 22)
    for png in pngs[0] + pngs[2]:
        os.remove(png)
    random.seed(22)
    got = buf.get(samples[0][0])
    _same(want, got)
    assert store.inexact_pixels() == 0
    # slam._cat_dict: (1 + K) rows, row 0 the online sample, rows 1.. bitwise `got`; a later frame gets storage of its own
    online = samples[1][0]
    joined = slam._cat_dict(online, got)
    assert set(joined) == set(online) & set(got)
    kept = {k: v.clone() for k, v in joined.items()}
    for k in joined:
        assert joined[k].shape[0] == 3 and torch.equal(joined[k][:1].cpu(), online[k]) and torch.equal(joined[k][1:], got[k]), k
    assert joined['rgb', 0, 0].device.type == dev.type
    random.seed(23)
    joined2 = slam._cat_dict(samples[0][0], buf.get(samples[0][0]))
    for k in joined:
        assert joined2[k].data_ptr() != joined[k].data_ptr() and torch.equal(joined[k], kept[k]), k
        assert torch.equal(joined2[k][:1].cpu(), samples[0][0][k]), k
    # a sample `add` removes from online_filenames leaves the store, too
    buf.buffer_size = 2
    fourth = {k: v.clone() for k, v in samples[1][0].items()}
    fourth['index',] = torch.tensor([7])
    buf.add(fourth, dict(samples[1][1], index=7))
    assert files[0] not in store and files[0] not in buf.online_filenames and buf.online_filenames[-1] in store
    build.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_without_store_bytes_nothing_changes(backend, tmp_path):
    """store_bytes = 0 (the default): no store, `add` stays the buffer's own, `get` is bitwise the concatenated get_many"""
    dev = use_backend(backend)
    z = np.load(GOLDEN, allow_pickle=False)
    H, W, scales, frames = _geometry(z)
    (tmp_path / 'src').mkdir()
    (tmp_path / 'buf').mkdir()
    plain, samples, _ = _online_samples(tmp_path, z, dev, extra=0)
    buf = _BufferShapedLikeTheReference(tmp_path / 'buf', buffer_size=3)
    build = ingest.ReplaySampleBuilder(H, W, scales, frames, device=dev)
    assert build.store is None
    build.install(buf).install(buf)
    assert 'add' not in vars(buf) and buf.add.__func__ is _BufferShapedLikeTheReference.add
    for sample, names in samples:
        buf.add(sample, names)
    buf.pick = [1, 0]
    want = _by_png(plain, [buf.online_filenames[i] for i in buf.pick], 5)
    random.seed(5)
    got = buf.get(samples[0][0])
    _same(want, got)
    assert all(not hasattr(v, '_clslam_whole') for v in got.values()) and buf.calls == 0
    build.close()
