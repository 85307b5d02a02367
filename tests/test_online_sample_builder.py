"""clslam_hip.ingest.OnlineSampleBuilder / FrameRing against a stand-in of the reference's dataset.

The referee is `_KittiShapedLikeTheReference` below: its __getitem__ restates datasets/kitti.py:231-317 (with _pre_getitem,
_post_getitem and _scale_camera_matrix of datasets/utils.py:104-171 and _preprocess, kitti.py:333-355) with Pillow on a temporary
directory of small random PNGs, and `default_collate` stands for the driver's DataLoader(batch_size=1).  torchvision's
Resize(LANCZOS) of a PIL image IS Image.resize(size, LANCZOS) and its ToTensor of an RGB image IS uint8 -> float32 / 255, which
is what the stand-in calls.  Model size 16 x 48 on 37 x 123 PNGs, 9 files (7 samples); the adapt() parity at the golden 64 x 128."""
import pickle
import threading

import numpy as np
import pytest
import torch
from PIL import Image
from torch.utils.data import default_collate

from clslam_hip import ingest, ops
from emu_util import BACKENDS, use_backend

H, W, RAW_H, RAW_W, N_FILES = 16, 48, 37, 123, 9


def _to_tensor(pic):
    """torchvision.transforms.ToTensor (datasets/utils.py:213-215): a PIL RGB image -> float32 (3,h,w) / 255; a 2-D array that is
    no uint8 image -> (1,h,w), dtype kept"""
    if isinstance(pic, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(pic[:, :, None].transpose(2, 0, 1)))
    return torch.from_numpy(np.ascontiguousarray(np.asarray(pic).transpose(2, 0, 1))).to(torch.float32).div(255)


class _KittiShapedLikeTheReference:
    def __init__(self, root, height=H, width=W, scales=(0, 1, 2, 3), frame_ids=(0, -1, 1), n_files=N_FILES, raw=(RAW_H, RAW_W),
                 do_augmentation=False, views=('left',), with_depth=False, with_mask=False, poses=True, seed=0):
        self.frame_ids, self.scales, self.height, self.width = sorted(frame_ids), scales, height, width
        self.do_augmentation, self.views, self.with_depth, self.with_mask = do_augmentation, tuple(set(views)), with_depth, with_mask
        self.include_poses = poses
        rng = np.random.default_rng(seed)
        root.mkdir(parents=True, exist_ok=True)
        self.left_img_filenames = []
        for i in range(n_files):
            fn = root / f'{i:06}.png'
            if not fn.exists():
                Image.fromarray(rng.integers(0, 256, raw + (3,), dtype=np.uint8)).save(fn)
            self.left_img_filenames.append(fn)
        self.sequence_indices = {9: (0, n_files - 1)}
        self.camera_matrix = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        rng = np.random.default_rng(seed + 1000)               # not the pixels' generator: a second object on the same tree skips them
        self.relative_distances = [0.] + [float(v) for v in rng.uniform(0.2, 1.5, n_files - 1)]
        self.global_poses = [np.eye(4, dtype=np.float32) + rng.normal(0, 0.1, (4, 4)).astype(np.float32) for _ in range(n_files)]
        self.relative_poses = np.stack([np.eye(4, dtype=np.float32)] + [np.linalg.inv(a) @ b for a, b in
                                                                        zip(self.global_poses, self.global_poses[1:])])

    def __len__(self):
        return len(self.views) * (len(self.left_img_filenames) - 2 * len(self.sequence_indices))

    def _scale_camera_matrix(self, camera_matrix, scale):                      # datasets/utils.py:104-110
        scaled = camera_matrix.copy()
        scaled[0, :] *= self.width // (2**scale)
        scaled[1, :] *= self.height // (2**scale)
        return scaled, np.linalg.pinv(scaled)

    def _pre_getitem(self, index):                                             # datasets/utils.py:112-152, one view
        if index < 0 or index >= len(self):
            raise IndexError()
        for i, seq in enumerate(self.sequence_indices.values()):
            if seq[0] < index + 2 * i + 1 < seq[1]:
                index += 2 * i + 1
                break
        return self.left_img_filenames, [], index, False, False

    def _resize(self, img, scale):                                             # Resize((h, w), LANCZOS) of a PIL image
        return img.resize((self.width // 2**scale, self.height // 2**scale), Image.LANCZOS)

    def __getitem__(self, index):                                              # datasets/kitti.py:231-317
        img_filenames, _, index, _, _ = self._pre_getitem(index)
        item = {('index'): index}
        for frame_id in self.frame_ids:
            rgb = Image.open(img_filenames[index + frame_id]).convert('RGB')
            item['rgb', frame_id, 0] = self._resize(rgb, 0)
        for scale in range(len(self.scales)):
            item['camera_matrix', scale], item['inv_camera_matrix', scale] = self._scale_camera_matrix(self.camera_matrix, scale)
        for frame_id in self.frame_ids[1:]:
            item['relative_distance', frame_id] = self.relative_distances[index + frame_id]
        if self.include_poses:
            for frame_id in self.frame_ids[1:]:
                item['relative_pose', frame_id] = self.relative_poses[index + frame_id]
                item['absolute_pose', frame_id] = self.global_poses[index + frame_id]
        for key in list(item.keys()):                                          # _post_getitem, datasets/utils.py:154-171
            if 'rgb' in key:
                k, frame_id, _ = key
                for scale in self.scales:
                    if scale != 0:
                        item[k, frame_id, scale] = self._resize(item[k, frame_id, scale - 1], scale)
        for key in list(item.keys()):                                          # _preprocess, datasets/kitti.py:341-353
            value = item[key]
            if 'rgb' in key:
                k, frame_id, scale = key
                item[key] = _to_tensor(value)
                item[f'{k}_aug', frame_id, scale] = _to_tensor(value)
            elif 'camera_matrix' in key or 'inv_camera_matrix' in key:
                item[key] = torch.from_numpy(value)
            elif 'relative_pose' in key or 'absolute_pose' in key:
                item[key] = _to_tensor(value)
        return item

    def get_item_filenames(self, index):                                       # datasets/utils.py:217-230
        names, _, index, _, _ = self._pre_getitem(index)
        return {'index': index, 'images': [names[index + f] for f in self.frame_ids], 'masks': []}


def _is_image(key):
    return isinstance(key, tuple) and key[0] in ('rgb', 'rgb_aug')


def _assert_same_sample(got, want, dev):
    assert list(got) == list(want)                      # the key set, in the dataset's order
    for k in want:
        g, w = got[k], want[k]
        if not isinstance(w, torch.Tensor):
            assert type(g) is type(w) and g == w, k
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.device.type == (dev.type if _is_image(k) else 'cpu'), (k, g.device)
        assert torch.equal(g.cpu(), w), k
    planes = [got[k] for k in got if _is_image(k)]
    assert len(planes) == 24 and len({t.data_ptr() for t in planes}) == 24


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """the PNG tree and the referee's collated samples, computed once"""
    root = tmp_path_factory.mktemp('online') / 'image_2'
    ds = _KittiShapedLikeTheReference(root)
    assert len(ds) == N_FILES - 2
    return root, [default_collate([ds[i]]) for i in range(len(ds))]


class _Counters:
    """Image.open and ops.resize_level_u8 wrapped to count their calls (the decode pool calls the first from its threads)"""

    def __init__(self, monkeypatch):
        self.opened, self.levels, self._lock = [], 0, threading.Lock()
        image_open, level = Image.open, ops.resize_level_u8

        def counted_open(fp, *a, **k):
            with self._lock:
                self.opened.append(str(fp))
            return image_open(fp, *a, **k)

        def counted_level(*a, **k):
            self.levels += 1
            return level(*a, **k)
        monkeypatch.setattr(Image, 'open', counted_open)
        monkeypatch.setattr(ops, 'resize_level_u8', counted_level)


@pytest.mark.parametrize('backend', BACKENDS)
def test_sample_is_the_collated_dataset_item(backend, tree):
    dev = use_backend(backend)
    root, want = tree
    ds = _KittiShapedLikeTheReference(root)
    build = ingest.OnlineSampleBuilder(ds, device=dev)
    try:
        for i in range(len(ds)):
            _assert_same_sample(build.sample(i), want[i], dev)
        with pytest.raises(IndexError):
            build.sample(len(ds))
    finally:
        build.close()
    no_poses = _KittiShapedLikeTheReference(root, poses=False)
    build = ingest.OnlineSampleBuilder(no_poses, device=dev, prefetch=0)
    _assert_same_sample(build.sample(2), default_collate([no_poses[2]]), dev)


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_ring_saves_work_and_survives_eviction(backend, tree, monkeypatch):
    """a walk over all indices with a ring of 4 frames: every file is decoded exactly once and every new frame costs exactly four
    level launches; the jump back to index 0 afterwards (its frames were evicted) returns the same sample again"""
    dev = use_backend(backend)
    root, want = tree
    ds = _KittiShapedLikeTheReference(root)
    count = _Counters(monkeypatch)
    build = ingest.OnlineSampleBuilder(ds, device=dev, ring_frames=4)
    try:
        assert build.ring.slot_bytes == 3 * (16 * 48 + 8 * 24 + 4 * 12 + 2 * 6) and build.ring.capacity == 4
        for i in range(len(ds)):
            _assert_same_sample(build.sample(i), want[i], dev)
            assert len(build._decoded) <= build.prefetch + 3
        assert sorted(count.opened) == sorted(str(f) for f in ds.left_img_filenames)
        assert count.levels == 4 * N_FILES
        assert str(ds.left_img_filenames[0]) not in build.ring and len(build.ring) == 4
        _assert_same_sample(build.sample(0), want[0], dev)
        assert count.levels == 4 * (N_FILES + 3)
    finally:
        build.close()
    assert build._pool is None


@pytest.mark.parametrize('backend', BACKENDS)
def test_prefetch_0_gives_the_same_samples(backend, tree, monkeypatch):
    dev = use_backend(backend)
    root, want = tree
    ds = _KittiShapedLikeTheReference(root)
    count = _Counters(monkeypatch)
    build = ingest.OnlineSampleBuilder(ds, device=dev, ring_frames=4, prefetch=0)
    for i in range(len(ds)):
        _assert_same_sample(build.sample(i), want[i], dev)
    assert sorted(count.opened) == sorted(str(f) for f in ds.left_img_filenames) and not build._decoded
    build.close()


class _SlamShapedLikeTheReference:
    """slam/slam.py:44-82 as far as install() touches it"""

    def __init__(self, dataset):
        self.online_dataset = dataset
        self.online_dataloader_iter = iter(torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=0))

    @staticmethod
    def _cat_dict(a, b):                 # slam/slam.py:300-309
        return {k: torch.cat([a[k], b[k]]) for k in a if k in b}


@pytest.mark.parametrize('backend', BACKENDS)
def test_install_switches_a_slam_object_over(backend, tree):
    dev = use_backend(backend)
    root, want = tree
    ds = _KittiShapedLikeTheReference(root)
    slam = _SlamShapedLikeTheReference(ds)
    type_before = type(slam.online_dataset)
    own = {i: ds[i]['rgb', 1, 0] for i in (0, 3, 6)}               # the stand-in's own, before the switch
    build = ingest.OnlineSampleBuilder(ds, device=dev)
    try:
        assert build.install(slam) is build
        assert len(slam.online_dataloader_iter) == len(ds)
        for i in range(len(ds)):
            _assert_same_sample(next(slam.online_dataloader_iter), want[i], dev)
        with pytest.raises(StopIteration):
            next(slam.online_dataloader_iter)
        for i, plane in own.items():                                # slam/slam.py:228
            got = slam.online_dataset[i]['rgb', 1, 0]
            assert got.device.type == dev.type and got.shape == plane.shape and torch.equal(got.cpu(), plane)
        item = slam.online_dataset[3]
        assert item['index'] == 4 and isinstance(item['relative_distance', 1], float) and item['camera_matrix', 0].shape == (4, 4)
        assert isinstance(slam.online_dataset, type_before) and type(slam.online_dataset) is not type_before
        first = type(slam.online_dataset)
        build.install(slam)                                         # again: rewinds, does not nest
        assert type(slam.online_dataset).__mro__[1] is type_before and type(slam.online_dataset) is not first
        _assert_same_sample(next(slam.online_dataloader_iter), want[0], dev)
        # the class keeps its own code: another instance still decodes on the host
        assert _KittiShapedLikeTheReference(root)[0]['rgb', 0, 0].device.type == 'cpu'
        with pytest.raises(ValueError, match='online_dataset'):
            build.install(_SlamShapedLikeTheReference(_KittiShapedLikeTheReference(root)))
    finally:
        build.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_refusals_name_the_option(backend, tree):
    dev = use_backend(backend)
    root, _ = tree
    for kwargs, name in ((dict(do_augmentation=True), 'do_augmentation'), (dict(with_depth=True), 'with_depth'),
                         (dict(with_mask=True), 'with_mask'), (dict(views=('left', 'right')), 'views'),
                         (dict(scales=(0, 2)), 'scales'), (dict(scales=()), 'scales')):
        with pytest.raises(ValueError, match=name):
            ingest.OnlineSampleBuilder(_KittiShapedLikeTheReference(root, **kwargs), device=dev)
    with pytest.raises(ValueError, match='ring_frames'):
        ingest.OnlineSampleBuilder(_KittiShapedLikeTheReference(root), device=dev, ring_frames=2)
    other = _KittiShapedLikeTheReference(root)
    del other.relative_distances                        # a dataset class without the reference's attributes
    with pytest.raises(ValueError, match='relative_distances'):
        ingest.OnlineSampleBuilder(other, device=dev)


class _BufferShapedLikeTheReference:
    """slam/replay_buffer.py's ReplayBuffer as far as ReplaySampleBuilder.install() touches it: `add` (:82-184) pickles the host
    entries and the three PNG names, `get` (:186-235) calls `self._get(filename)` per file and concatenates key by key"""

    def __init__(self, storage_dir):
        self.storage_dir, self.online_filenames = storage_dir, []
        storage_dir.mkdir(parents=True, exist_ok=True)

    def add(self, sample, sample_filenames, image_features=None, verbose=False):
        index = sample['index'].item()
        filename = self.storage_dir / f'kitti_{index:>05}.pkl'
        data = {key: value for key, value in sample.items()
                if 'index' in key or 'camera_matrix' in key or 'inv_camera_matrix' in key or 'relative_distance' in key}
        data['rgb', -1], data['rgb', 0], data['rgb', 1] = sample_filenames['images']
        with open(filename, 'wb') as f:
            pickle.dump(data, f, pickle.HIGHEST_PROTOCOL)
        self.online_filenames.append(filename)

    def _get(self, filename, include_batch=True):
        raise AssertionError('the reference _get must not run once a builder is installed')

    def get(self, sample, image_features=None):
        data = self._get(self.online_filenames[0])
        for fn in self.online_filenames[1:]:
            nxt = self._get(fn)
            for key in data:
                data[key] = torch.cat([data[key], nxt[key]])
        return data


@pytest.mark.parametrize('backend', BACKENDS)
def test_composes_with_the_replay_builder_and_its_frame_store(backend, tree, tmp_path):
    """one add + get round with the replay drop-in and its frame store installed: the device-resident online sample fills the
    store and the joined minibatch exactly like the host-built one, and nothing it packs is inexact"""
    dev = use_backend(backend)
    root, want = tree
    ds = _KittiShapedLikeTheReference(root)
    online = ingest.OnlineSampleBuilder(ds, device=dev)
    batches = {}
    try:
        for kind in ('host', 'device'):
            buf, slam = _BufferShapedLikeTheReference(tmp_path / kind), _SlamShapedLikeTheReference(ds)
            replay = ingest.ReplaySampleBuilder(H, W, (0, 1, 2, 3), (0, -1, 1), device=dev, do_augmentation=False, store_bytes=1 << 20)
            replay.install(buf, slam)
            for i in (1, 4):
                sample = {k: v.clone() for k, v in want[i].items()} if kind == 'host' else online.sample(i)
                buf.add(sample, ds.get_item_filenames(i))
            assert len(replay.store) == 2 and all(fn in replay.store for fn in buf.online_filenames)
            sample = {k: v.clone() for k, v in want[5].items()} if kind == 'host' else online.sample(5)
            got = slam._cat_dict(sample, buf.get(sample))
            assert replay.store.inexact_pixels() == 0
            batches[kind] = got
            replay.close()
    finally:
        online.close()
    assert list(batches['host']) == list(batches['device'])
    for k, w in batches['host'].items():
        g = batches['device'][k]
        assert g.shape == w.shape and g.dtype == w.dtype and g.shape[0] == 3, k
        assert torch.equal(g.cpu(), w.cpu()), k
        if _is_image(k):
            assert g.device.type == dev.type
            for row, i in enumerate((5, 1, 4)):                     # the online sample, then the two stored ones: the dataset's own
                assert torch.equal(g[row].cpu(), want[i][k][0]), (k, row)


@pytest.mark.gpu
def test_adapt_sees_the_same_frame():
    """64 x 128 (the golden size): predictor.adapt(sample, None) on the builder's sample and on the stand-in's host sample give
    bitwise the same depth and pose"""
    import tempfile
    from pathlib import Path
    from clslam_hip import synth
    from predictor_util import make_predictor
    dev = use_backend('hip')
    with tempfile.TemporaryDirectory() as tmp:
        ds = _KittiShapedLikeTheReference(Path(tmp) / 'image_2', height=64, width=128, n_files=4, raw=(94, 310), seed=3)
        host = default_collate([ds[1]])
        build = ingest.OnlineSampleBuilder(ds, device=dev)
        try:
            mine = build.sample(1)
        finally:
            build.close()
    _assert_same_sample(mine, host, dev)
    p = make_predictor(64, 128, 1)
    p.set_tie_break_noise(synth.make_noise(1, 64, 128, seed=5))
    out_host, _ = p.adapt(host, None)
    out_host = {k: out_host[k].clone() for k in (('depth', 0), ('cam_T_cam', 0, 1))}
    out_mine, _ = p.adapt(mine, None)
    for k, w in out_host.items():
        assert torch.isfinite(w).all() and torch.equal(out_mine[k].cpu(), w.cpu()), k
