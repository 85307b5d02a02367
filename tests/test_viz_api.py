"""clslam_hip.viz (depth_range, colorize, trajectory_image, frame_panel, generate_figure, PanelWriter) and
DepthPosePrediction.save_prediction against tests/viz_reference.py, on tiny generated frames."""
import itertools
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import viz_reference as ref
from emu_util import BACKENDS, use_backend

H, W = 12, 20


def _frame(seed=0):
    rng = np.random.default_rng(seed)
    image = rng.random((3, H, W)).astype(np.float32)
    depth = (rng.random((H, W)) ** 2 * 60 + 0.5).astype(np.float32)
    pcl = rng.random((H, W, 3)).astype(np.float32)
    gt = np.cumsum(rng.normal(size=(30, 2)) * 9, 0) + [-200.0, 50.0]
    pred = gt + rng.normal(size=gt.shape) * 4
    return image, depth, pcl, gt, pred


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_panel_every_subset_of_rows(backend):
    from clslam_hip import viz
    device = use_backend(backend)
    image, depth, pcl, gt, pred = _frame()
    for use_pcl, use_gt, use_pred in itertools.product((False, True), repeat=3):
        args = (image, depth, pcl if use_pcl else None, gt if use_gt else None, pred if use_pred else None)
        want, want_vmax = ref.frame_panel(*args)
        assert want.shape == ((2 + use_pcl + (use_gt or use_pred)) * H, W, 3)
        got, vmax = viz.frame_panel(*args)                                    # numpy in, numpy out
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        assert isinstance(vmax, np.ndarray) and vmax.dtype == np.float32 and vmax == want_vmax
        tensors = [None if a is None else torch.from_numpy(a).to(device) for a in args]
        got, vmax = viz.frame_panel(*tensors)                                 # tensors in, tensors on the same device out
        assert isinstance(got, torch.Tensor) and got.device == device and np.array_equal(got.cpu().numpy(), want)
        assert isinstance(vmax, torch.Tensor) and vmax.device == device and float(vmax) == float(want_vmax)
    # the other layouts of the image rows, the network's (1,1,H,W) depth, the other map and another percentile
    u8 = ref.image_row(image, chw=True)
    got, vmax = viz.frame_panel(u8, depth[None, None], pcl.astype(np.float64), None, pred, cmap='magma', q=50.0, xlim=(-300, 0), ylim=(0, 100))
    want, want_vmax = ref.frame_panel(u8, depth, pcl.astype(np.float64), None, pred, cmap='magma', q=50.0, xlim=(-300, 0), ylim=(0, 100))
    assert np.array_equal(got, want) and vmax == want_vmax


@pytest.mark.parametrize('backend', BACKENDS)
def test_frame_panel_refuses_other_sizes(backend):
    from clslam_hip import viz
    from clslam_hip._lib import ClslamError
    use_backend(backend)
    image, depth, pcl, gt, pred = _frame()
    with pytest.raises(ClslamError, match='image must be'):
        viz.frame_panel(image[:, :-1], depth)
    with pytest.raises(ClslamError, match='image_pcl must be'):
        viz.frame_panel(image, depth, pcl[:, :-1])
    with pytest.raises(ClslamError, match='image must be'):
        viz.frame_panel(image.astype(np.float64), depth)                      # (3,H,W) is the float32 network layout only
    with pytest.raises(ClslamError, match='one depth plane'):
        viz.frame_panel(image, np.stack([depth, depth]))
    with pytest.raises(ClslamError, match=r'\(N,2\)'):
        viz.frame_panel(image, depth, None, gt[:, :1], None)


@pytest.mark.parametrize('backend', BACKENDS)
def test_depth_range_colorize_and_trajectory_image(backend):
    from clslam_hip import viz
    device = use_backend(backend)
    _, depth, _, gt, pred = _frame(3)
    batch = np.stack([depth, depth[::-1] * 0.5, np.round(depth)])
    want = [ref.depth_range(p) for p in batch]
    vmin, vmax = viz.depth_range(batch)
    assert vmin.shape == (3,) and vmin.tolist() == [w[0] for w in want] and vmax.tolist() == [w[1] for w in want]
    vmin, vmax = viz.depth_range(torch.from_numpy(batch[:, None]).to(device), q=50.0)
    assert vmax.device == device and vmax.tolist() == [ref.depth_range(p, 50.0)[1] for p in batch]
    vmin, vmax = viz.depth_range(depth)
    assert vmin.shape == () and (vmin, vmax) == want[0][:2]
    got = viz.colorize(batch)
    assert got.shape == (3, H, W, 3) and all(np.array_equal(got[i], ref.colorize(batch[i], *want[i][:2])) for i in range(3))
    assert np.array_equal(viz.colorize(depth, cmap='magma', vmin=2.0, vmax=30.0), ref.colorize(depth, 2.0, 30.0, 'magma'))
    assert np.array_equal(viz.colorize(depth, vmax=30.0), ref.colorize(depth, want[0][0], 30.0))
    got = viz.colorize(torch.from_numpy(batch[:, None]).to(device), vmin=torch.tensor([1.0, 2.0, 3.0]), vmax=40.0)
    assert got.shape == (3, 1, H, W, 3) and got.device == device
    assert all(np.array_equal(got[i, 0].cpu().numpy(), ref.colorize(batch[i], i + 1.0, 40.0)) for i in range(3))
    got = viz.trajectory_image(gt, torch.from_numpy(pred).to(device), (H, W))
    assert got.device == device and np.array_equal(got.cpu().numpy(), ref.trajectory_row(gt, pred, (H, W)))
    assert np.array_equal(viz.trajectory_image(None, pred, (5, 7), xlim=(-250, -100), ylim=(0, 90)),
                          ref.trajectory_row(None, pred, (5, 7), xlim=(-250, -100), ylim=(0, 90)))


@pytest.mark.parametrize('backend', BACKENDS)
def test_generate_figure_writes_the_panel(backend, tmp_path):
    from clslam_hip import viz
    device = use_backend(backend)
    image, depth, pcl, gt, pred = _frame(1)
    want, _ = ref.frame_panel(image, depth, pcl, gt, pred)
    out_dir = tmp_path / 'figures' / 'sequence_08'
    assert viz.generate_figure(7, image, depth, pcl, gt, pred, out_dir=out_dir) is None
    assert [p.name for p in out_dir.iterdir()] == ['00007.png']
    assert np.array_equal(np.array(Image.open(out_dir / '00007.png')), want)
    tensors = [torch.from_numpy(a).to(device) for a in (image, depth, pcl, gt, pred)]
    viz.generate_figure(12345, *tensors, save_figure=True, out_dir=out_dir)
    assert np.array_equal(np.array(Image.open(out_dir / '12345.png')), want)
    got = viz.generate_figure(8, *tensors, save_figure=False, out_dir=tmp_path / 'nothing')
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(viz.generate_figure(8, image, depth, pcl, gt, pred, False, out_dir=tmp_path / 'nothing'), want)
    assert not (tmp_path / 'nothing').exists() and sorted(p.name for p in out_dir.iterdir()) == ['00007.png', '12345.png']


@pytest.mark.parametrize('backend', BACKENDS)
def test_panel_writer_keeps_the_inputs_it_was_given(backend, tmp_path):
    from clslam_hip import viz
    device = use_backend(backend)
    frames = [_frame(10 + i) for i in range(3)]
    image, depth, pcl, gt, pred = (torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=device) for a in frames[0])
    writer = viz.PanelWriter(tmp_path / 'panels', workers=2)
    handles = []
    for i, frame in enumerate(frames):
        for dst, src in zip((image, depth, pcl, gt, pred), frame):
            dst.copy_(torch.from_numpy(src))
        handles.append(writer.submit(40 + i, image, depth, pcl, gt, pred))
        for dst in (image, depth, pcl, gt, pred):                            # overwritten right after submit()
            dst.fill_(0.25)
    assert handles[0].result() == tmp_path / 'panels' / '00040.png'
    writer.close()
    assert sorted(p.name for p in (tmp_path / 'panels').iterdir()) == ['00040.png', '00041.png', '00042.png']
    for i, frame in enumerate(frames):
        assert np.array_equal(np.array(Image.open(tmp_path / 'panels' / f'{40 + i:05}.png')), ref.frame_panel(*frame)[0]), i
    with viz.PanelWriter(tmp_path / 'panels2') as w2:
        w2.submit(1, *frames[0][:2])
    assert np.array_equal(np.array(Image.open(tmp_path / 'panels2' / '00001.png')), ref.frame_panel(*frames[0][:2])[0])


@pytest.mark.parametrize('backend', BACKENDS)
def test_panel_writer_bounds_the_frames_in_flight(backend, tmp_path):
    """more frames than slots: never more than `in_flight` pending, the staging buffers are reused, every file is right; a
    writer's error is raised by close()"""
    from clslam_hip import viz
    device = use_backend(backend)
    frames = [_frame(20 + i)[:2] for i in range(7)]
    writer = viz.PanelWriter(tmp_path / 'ring', workers=2, in_flight=2)
    for i, (image, depth) in enumerate(frames):
        writer.submit(i, torch.from_numpy(image).to(device), torch.from_numpy(depth).to(device))
        assert writer.pending() <= 2
    buffers = {id(s['host']) for s in writer._slots}
    writer.close()
    assert writer.pending() == 0 and len(writer._slots) == 2 and len(buffers) <= 2
    for i, frame in enumerate(frames):
        assert np.array_equal(np.array(Image.open(tmp_path / 'ring' / f'{i:05}.png')), ref.frame_panel(*frame)[0]), i
    broken = viz.PanelWriter(tmp_path / 'gone', in_flight=1)
    (tmp_path / 'gone').rmdir()
    broken.submit(0, *frames[0])
    broken.submit(1, *frames[1])                                             # retires the failed frame 0 without raising
    with pytest.raises(OSError):
        broken.close()


@pytest.mark.gpu
def test_a_cpu_tensor_comes_back_on_the_cpu():
    """on the device library a CPU tensor is computed on the GPU and the result returned where the input was"""
    from clslam_hip import viz
    use_backend('hip')
    image, depth, pcl, gt, pred = _frame(2)
    panel, vmax = viz.frame_panel(*(torch.from_numpy(a) for a in (image, depth, pcl, gt, pred)))
    want, want_vmax = ref.frame_panel(image, depth, pcl, gt, pred)
    assert panel.device.type == 'cpu' and vmax.device.type == 'cpu' and np.array_equal(panel.numpy(), want) and float(vmax) == float(want_vmax)
    assert viz.colorize(torch.from_numpy(depth)).device.type == 'cpu' and viz.depth_range(torch.from_numpy(depth))[1].device.type == 'cpu'
    assert viz.trajectory_image(torch.from_numpy(gt), None, (H, W)).device.type == 'cpu'
    mixed, _ = viz.frame_panel(torch.from_numpy(image).cuda(), torch.from_numpy(depth))          # the first tensor decides
    assert mixed.device.type == 'cuda' and np.array_equal(mixed.cpu().numpy(), ref.frame_panel(image, depth)[0])


def test_a_wait_has_a_deadline():
    from clslam_hip import viz
    from clslam_hip._lib import ClslamError

    class Never:
        def query(self):
            return False
    with pytest.raises(ClslamError, match='did not finish'):
        viz._wait(Never(), 0.0, 'test')
    viz._wait(None, 0.0, 'test')


@pytest.mark.gpu
def test_save_prediction_and_validate_still_warns(tmp_path):
    from clslam_hip import synth, viz
    from predictor_util import make_predictor
    use_backend('hip')
    Hp, Wp, B = 64, 128, 2
    p = make_predictor(Hp, Wp, B, log_path=str(tmp_path / 'log'), save_val_depth=True, save_val_depth_batches=1)
    p.epoch = 3
    batch = synth.make_batch(B, Hp, Wp, seed=3)
    inputs = {k: v.clone() for k, v in batch.items()}
    inputs['index'] = torch.tensor([17, 4])
    outputs = p.predict({k: v.clone() for k, v in batch.items()})
    assert outputs['depth', 0].shape == (B, 1, Hp, Wp)
    p.save_prediction(inputs, outputs)
    folder = tmp_path / 'log' / 'prediction' / 'val_depth_003'
    assert sorted(f.name for f in folder.iterdir()) == ['00004.png', '00017.png']
    colours = viz.colorize(outputs['depth', 0])
    for i, index in enumerate((17, 4)):
        depth = outputs['depth', 0][i, 0].cpu().numpy()
        want = np.concatenate([ref.image_row(batch['rgb', 0, 0][i].numpy(), chw=True), colours[i, 0].cpu().numpy()])
        assert np.array_equal(np.array(Image.open(folder / f'{index:05}.png')), want)
        assert np.array_equal(want[Hp:], ref.colorize(depth, *ref.depth_range(depth)[:2]))
    # validate() is not wired to save_prediction: it still says so, once, and writes nothing
    p.set_tie_break_noise(synth.make_noise(B, Hp, Wp, seed=5))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        p.validate(data_loader=[{k: v.clone() for k, v in batch.items()}])
    assert len([r for r in rec if 'save_val_depth' in str(r.message)]) == 1
    assert sorted(f.name for f in folder.iterdir()) == ['00004.png', '00017.png']
