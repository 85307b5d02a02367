"""Frame panels on the device at 192x640 (the network's frame): the range of a depth plane, colorize, a four-row frame_panel,
generate_figure to a file, PanelWriter's throughput -- and, in the same session, a matplotlib figure of the same content as
the reference's generate_figure (slam/utils.py:85-121; host_figure below, written for this benchmark) on the host if
matplotlib imports; otherwise the report says that it was not measured.

Device rows: device events around `--reps` back-to-back calls on prepared device tensors (allocations from torch's cache are
inside), `--blocks` such blocks after a warm-up; the median block per call with the smallest and largest.  File rows: a host
clock around calls that end with the file written.  Writes the report to `--out` and prints one JSON line.

    python tools/bench_viz.py [--out profiles/viz.txt]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / 'cl-slam_amd', ROOT / 'tests'):
    sys.path.insert(0, str(p))

import viz_reference as ref                            # noqa: E402
from clslam_hip import ops, viz                        # noqa: E402

H, W = 192, 640


def scene(seed=0, poses=1100):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (3.0 + 70.0 * (1.0 - yy / H) ** 2 + 2.0 * np.sin(xx / 37.0) + rng.random((H, W))).astype(np.float32)
    image = np.clip(0.5 + 0.4 * np.sin(xx / 23.0)[None] * np.cos(yy / 17.0)[None] + 0.1 * rng.random((3, H, W)), 0, 1).astype(np.float32)
    pcl = np.moveaxis(image, 0, -1)[:, ::-1].copy()
    gt = np.cumsum(rng.normal(size=(poses, 2)) * 0.6 + [-0.25, 0.05], 0)
    pred = gt + np.cumsum(rng.normal(size=gt.shape) * 0.05, 0)
    return image, depth, pcl, gt, pred


def device_time(fn, blocks, reps, warmup):
    """us per call: (median, min, max) over the blocks"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out)), min(out), max(out)


def host_time(fn, blocks, reps, warmup):
    """ms per call of a function that returns with its work done"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3 / reps)
    return float(np.median(out)), min(out), max(out)


FIGURE_PX, FIGURE_DPI = (800, 1000), 100        # the host figure's canvas: the size of the reference's page


def host_figure(path, image, depth, image_pcl, gt_xz, pred_xz):
    """A matplotlib figure of the same content as utils.py:85-121, written for this benchmark through the object API: four
    stacked axes -- frame, depth as magma_r up to its 95th percentile, projected map, the two trajectories in viz's window with
    a legend -- each with a caption, saved as a PNG of FIGURE_PX."""
    from matplotlib.figure import Figure
    fig = Figure(figsize=(FIGURE_PX[0] / FIGURE_DPI, FIGURE_PX[1] / FIGURE_DPI), dpi=FIGURE_DPI, layout='tight')
    top, second, third, bottom = fig.subplots(4, 1)
    upper = float(np.percentile(depth, 95))
    for ax, picture, caption, style in ((top, image, 'frame', {}),
                                        (second, depth, f'depth, colours end at {upper:.3f}', {'cmap': 'magma_r', 'vmax': upper}),
                                        (third, image_pcl, 'map seen from the frame', {})):
        ax.imshow(picture, **style)
        ax.set_axis_off()
        ax.set_title(caption)
    for xz, name in ((gt_xz, 'ground truth'), (pred_xz, 'estimate')):
        bottom.plot(xz[:, 0], xz[:, 1], label=name)
    bottom.set(xlim=viz.XLIM, ylim=viz.YLIM)
    bottom.legend()
    fig.savefig(path)


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'viz.txt'))
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--frames', type=int, default=200)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    image, depth, pcl, gt, pred = scene()
    t_image, t_depth, t_pcl, t_gt, t_pred = (torch.from_numpy(a).to(dev) for a in (image, depth, pcl, gt, pred))
    planes = t_depth[None]
    lines = [f'Frame panels on the device, MI355X, {H}x{W} (tools/bench_viz.py); {gt.shape[0]} poses per trajectory', '']

    # ---- results first ----
    panel, vmax = viz.frame_panel(t_image, t_depth, t_pcl, t_gt, t_pred)
    want, want_vmax = ref.frame_panel(image, depth, pcl, gt, pred)
    assert np.array_equal(panel.cpu().numpy(), want) and float(vmax) == float(want_vmax), 'the panel is not the numpy restatement'
    lines += ['0. Checked before timing: the four-row panel and its vmax equal tests/viz_reference.py bit for bit.', '']
    result = {}

    # ---- 1. device time ----
    rng, _ = ops.viz_range(planes)
    rows = {
        'range': lambda: ops.viz_range(planes),
        'colour row alone': lambda: ops.viz_compose([ops.viz_cmap_row(planes, rng)], 1, H, W),
        'colorize': lambda: viz.colorize(t_depth),
        'frame_panel x4': lambda: viz.frame_panel(t_image, t_depth, t_pcl, t_gt, t_pred),
        'frame_panel x2': lambda: viz.frame_panel(t_image, t_depth),
    }
    lines += [f'1. Device events around back-to-back Python calls, us per call: median of {args.blocks} blocks of {args.reps} calls (min .. max), '
              f'{args.warmup} warm-up calls.',
              '   This is the cost of ISSUING the launches from Python, which the device hides behind nothing here: NOT kernel time.',
              '   range = memset + 5 launches; colorize = range + 1 composing launch; frame_panel = range + 1 composing launch.']
    for name, fn in rows.items():
        med, lo, hi = device_time(fn, args.blocks, args.reps, args.warmup)
        result[name.replace(' ', '_') + '_us'] = round(med, 2)
        lines.append(f'   {name:18s} {med:9.1f}  ({lo:.1f} .. {hi:.1f})')
    lines.append('')

    # ---- 2. files ----
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        med, lo, hi = host_time(lambda: viz.generate_figure(1, t_image, t_depth, t_pcl, t_gt, t_pred, out_dir=tmp / 'g'), args.blocks, 10, 5)
        assert np.array_equal(np.array(Image.open(tmp / 'g' / '00001.png')), want)
        result['generate_figure_ms'] = round(med, 3)
        lines += ['2. Files, host clock, ms per frame.',
                  f'   generate_figure -> PNG file (4 rows)     {med:8.3f}  ({lo:.3f} .. {hi:.3f})   panel + device PNG + one length read + write']
        times = []
        for rep in range(3):
            writer = viz.PanelWriter(tmp / f'w{rep}', workers=2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.frames):
                writer.submit(i, t_image, t_depth, t_pcl, t_gt, t_pred)
            t_submit = time.perf_counter() - t0
            writer.close()
            times.append(((time.perf_counter() - t0) * 1e3 / args.frames, t_submit * 1e3 / args.frames))
        assert np.array_equal(np.array(Image.open(tmp / 'w2' / f'{args.frames - 1:05}.png')), want)
        per, sub = sorted(times)[1]
        result['panel_writer_ms'], result['panel_writer_submit_ms'] = round(per, 3), round(sub, 3)
        lines.append(f'   PanelWriter, {args.frames} frames, 2 threads, 4 slots {per:8.3f}   per frame until close() returns; submit() itself {sub:.3f} '
                     '(median of 3 runs)')
        try:
            import matplotlib
            hwc = np.moveaxis(image, 0, -1)
            med, lo, hi = host_time(lambda: host_figure(tmp / 'host.png', hwc, t_depth.cpu().numpy(), pcl, gt, pred), 5, 3, 2)
            result['matplotlib_ms'] = round(med, 1)
            lines.append(f'   matplotlib {matplotlib.__version__} figure (host)              {med:8.1f}  ({lo:.1f} .. {hi:.1f})   a figure of the same content as '
                         f'utils.py:85-121 ({FIGURE_PX[0]}x{FIGURE_PX[1]} px, four axes), incl. the depth plane\'s copy to the host, same session')
        except ImportError:
            result['matplotlib_ms'] = None
            lines.append('   matplotlib figure (host)                  not measured: matplotlib does not import on this machine')
    lines.append('')
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('\n'.join(lines))
    print('\n'.join(lines))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
