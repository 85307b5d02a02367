#!/usr/bin/env python
"""Record tests/golden/viz_colormap.npz from the installed matplotlib: the byte tables of magma and magma_r, and what
`cmap(Normalize(vmin, vmax)(x), bytes=True)[..., :3]` gives for the inputs of tests/test_viz_kernels.py's colour-map test.

    python tests/golden/make_viz_golden.py

The tests read the file; matplotlib is only needed to make it."""
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

WIDTHS, HEIGHTS = (1, 5, 64, 67), (1, 3, 33)
# the first two differences are not float32 numbers: dividing by the rounded difference moves exact-integer xa by one table entry
RANGES = ((np.float32(0.4), np.float32(55.5)), (np.float32(-3.0), np.float32(0.7)), (np.float32(2.0), np.float32(2.0)))


def colour_plane(h: int, w: int, vmin, vmax, seed: int) -> np.ndarray:
    """(h,w) float32: the ends of the range, their float32 neighbours on both sides, values whose xa = t * 256 is an exact integer
    (vmin + j (vmax - vmin) / 256), NaN and both infinities first, then uniform values a little wider than the range."""
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    d = vmax - vmin
    special = [vmin, vmax, np.nextafter(vmin, np.float32(-np.inf)), np.nextafter(vmin, np.float32(np.inf)),
               np.nextafter(vmax, np.float32(-np.inf)), np.nextafter(vmax, np.float32(np.inf)), np.float32(np.nan),
               np.float32(np.inf), np.float32(-np.inf)]
    special += [np.float32(vmin + np.float32(j) * d / np.float32(256)) for j in (1, 2, 3, 64, 127, 128, 129, 200, 254, 255)]
    rng = np.random.default_rng(seed)
    span = float(d) if d > 0 else 1.0
    x = (float(vmin) - 0.1 * span + rng.random(h * w) * 1.2 * span).astype(np.float32)
    # the specials go in at random places when there is room for all of them, else as many as fit
    k = min(len(special), x.size)
    x[rng.permutation(x.size)[:k]] = np.array(special, np.float32)[rng.permutation(len(special))[:k]]
    return x.reshape(h, w)


def cases():
    """(name, plane, vmin, vmax, cmap) of every recorded case: every size with every range, the two maps in turn (three ranges
    against two maps: every pair of them occurs)"""
    seed = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            for r, (vmin, vmax) in enumerate(RANGES):
                cmap = ('magma_r', 'magma')[seed % 2]
                seed += 1
                yield f'{cmap}_{h}x{w}_r{r}', colour_plane(h, w, vmin, vmax, seed), vmin, vmax, cmap


def main() -> None:
    import matplotlib
    matplotlib.use('Agg')
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    out = {}
    for name in ('magma', 'magma_r'):
        out[name] = np.ascontiguousarray(colormaps[name](np.arange(256), bytes=True)[:, :3])
    assert (out['magma_r'] == out['magma'][::-1]).all()
    for name, x, vmin, vmax, cmap in cases():
        out['rgb_' + name] = np.ascontiguousarray(colormaps[cmap](Normalize(vmin, vmax)(x), bytes=True)[..., :3])
    out['matplotlib_version'] = np.array(matplotlib.__version__)
    np.savez_compressed(HERE / 'viz_colormap.npz', **out)
    print('wrote', HERE / 'viz_colormap.npz', (HERE / 'viz_colormap.npz').stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
