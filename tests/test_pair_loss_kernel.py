"""The fused pair-loss kernel (ops.pair_loss / pair_loss_rng) and its finalize (ops.pair_loss_finalize) against the float64
restatement of tests/pair_loss_reference.py + tests/loss_reference.py, by the method of tests/test_loss_kernels.py (its
input generators, its comparison helpers and its rules for bounds are imported, not restated).

Inputs.  Disparities, intrinsics and poses are test_loss_kernels' (per-sample different K, oblique rotation, MOTIONS).  The
images are built so that both candidates win somewhere: src is strongly textured (a flat window divides the fp32 rounding of
the SSIM variances by sigma + C2 and moves a map by more than the 1e-5 the selection is held to); the target is the float64
warp of src plus grain in the upper 60 % of the rows (the reprojection wins) and src itself plus grain below (the identity
wins).  The fraction of identity pixels is asserted on the float64 reference (20-80 %) before the kernel is looked at.

Measured figures (kernel | torch fp32, against float64), the worst case over the five cases; emu = the kernel sources on the
CPU emulator, hip = gfx950 (every row is printed per case with -s):
  quantity                                   emu kernel | fp32   (ratio)     hip kernel | fp32   (ratio)
  pair_loss depth max                          2.38e-07 | 2.38e-07 (1.00x)     2.38e-07 | 2.38e-07 (1.00x)
  pair_loss identity map max                   5.41e-06 | 5.44e-06 (0.99x)     8.49e-06 | 5.44e-06 (1.56x)
  pair_loss identity map rel L2                1.34e-06 | 1.33e-06 (1.01x)     1.25e-06 | 1.33e-06 (0.94x)
  pair_loss reprojection map max               2.52e-05 | 2.52e-05 (1.00x)     1.62e-05 | 1.51e-05 (1.07x)
  pair_loss reprojection map rel L2            4.80e-06 | 4.69e-06 (1.02x)     4.51e-06 | 4.83e-06 (0.93x)
  (largest ratio of any row of any case: 1.61x emu, 1.87x hip, both the maximum of a map at one pixel)
  cells / sel differing from float64           0 of <= 16384 px, every case, both backends
  block sums max |d| / bound                   0.085                           0.100
  fused minimum vs the unfused chain, max      5.96e-08 (0.001 x the bound)    2.27e-05 (0.225 x the bound 4 x 2.52e-05)
      (hip: photo_map divides where the fused kernel multiplies by a hardware reciprocal; the emulator's reciprocal IS a division)
  depth vs warp_fwd, block sums vs photo_automask_pyramid on the same pair: the same bits, both backends
  pair_loss_finalize losses max rel            4.22e-06 (the smooth term of the flattened mode, whose two rounded quotients
                                               cancel: bound 70 u + canc); every other scalar <= 5.8e-07, bounds >= 3.9e-06
"""
import pytest
import torch

import loss_reference as R
import pair_loss_reference as PR
import test_loss_kernels as T
from clslam_hip import ops
from emu_util import BACKENDS, use_backend

U, F32, F64, NAN = T.U, torch.float32, torch.float64, float('nan')

# B, H, W, depth mode, motion.  24x80: the smallest level the library sees; 20x36: no multiple of the 8 x 64 tile, the only
# tile is partial in both directions; 64x128: 8 x 2 tiles; 24x80 'right': a band of samples past the right border (clip and
# last-cell read); B = 1 and 2.
CASES = [pytest.param(1, 24, 80, 1, 'small', id='24x80-B1-small'), pytest.param(2, 24, 80, 0, 'right', id='24x80-B2-right'),
         pytest.param(2, 20, 36, 2, 'small', id='20x36-B2-ragged'), pytest.param(1, 64, 128, 1, 'left', id='64x128-B1-left'),
         pytest.param(2, 64, 128, 2, 'small', id='64x128-B2-small')]


def _scene(seed, B, H, W, mode, motion):
    g = T._gen(seed)
    K, Kinv = T._camera(B, H, W)
    disp = T._smooth_field(g, B, H, W, 0.2, 0.8)
    pose = T._poses(B, H, W, K, mode, motion)
    P = R.pose_to_proj(pose, K)[1][0].float().contiguous()          # frame index 0 = the inverted transform of frame -1
    src = (T._smooth_field(g, B * 3, H, W, 0.3, 0.7, 0.0).reshape(B, 3, H, W) + 0.6 * (torch.rand(B, 3, H, W, generator=g) - 0.5)).contiguous()
    depths = T.DEPTH_MODES[mode]
    w64 = PR.view_and_maps(disp, src, src, Kinv, P, *depths)['warped'].float()
    rows = (torch.arange(H) < int(0.6 * H))[None, None, :, None]
    target = (torch.where(rows, w64, src) + 0.03 * (torch.rand(B, 3, H, W, generator=g) - 0.5)).contiguous()
    noise = (1e-5 * torch.randn(B, 1, H, W, generator=g)).contiguous()
    return dict(B=B, H=H, W=W, K=K, Kinv=Kinv, disp=disp, pose=pose, P=P, src=src, target=target, noise=noise, depths=depths)


def _kernel_cells(sc, dev):
    """the bilinear cells of the kernel's positions: warp_cells_pyramid evaluates the same functions of geometry_dev.h on the
    same disparity (scale 0 of a pyramid whose other levels are never looked at)"""
    B, H, W = sc['B'], sc['H'], sc['W']
    disps = [sc['disp']] + [sc['disp'][:, ::1 << s, ::1 << s].contiguous() for s in (1, 2, 3)]
    cells = torch.full((4, 2, B, H, W), -1, dtype=torch.int32, device=dev)
    ops.warp_cells_pyramid(T._dev_list(disps, dev), sc['Kinv'].to(dev), torch.stack([sc['P'], sc['P']]).to(dev), cells, *sc['depths'])
    x0, y0, mx, my = R.unpack_cells(cells[0].cpu())
    return x0, y0, mx, my


def _run(sc, dev, outputs=True, rng=None):
    B, H, W = sc['B'], sc['H'], sc['W']
    t = lambda v: v.contiguous().to(dev)
    nblk = ops.automask_blocks(H, W)
    partial = torch.full((B, nblk), NAN, device=dev)
    kw = {}
    if outputs:
        kw = dict(depth=torch.full((B, H, W), NAN, device=dev), sel=torch.full((B, H, W), 9, dtype=torch.uint8, device=dev),
                  maps=torch.full((2, B, H, W), NAN, device=dev))
    if rng is None:
        ops.pair_loss(t(sc['disp']), t(sc['src']), t(sc['target']), t(sc['Kinv']), t(sc['P']), t(sc['noise']), partial, *sc['depths'], **kw)
    else:
        ops.pair_loss_rng(t(sc['disp']), t(sc['src']), t(sc['target']), t(sc['Kinv']), t(sc['P']), rng[0], rng[1], partial, *sc['depths'], **kw)
    return partial, kw


def _tiles(v, H, W):
    ty, tx = -(-H // 8), -(-W // 64)
    return torch.nn.functional.pad(v, (0, tx * 64 - W, 0, ty * 8 - H)).reshape(v.shape[0], ty, 8, tx, 64).sum((2, 4)).reshape(v.shape[0], -1)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,mode,motion', CASES)
def test_pair_loss(backend, B, H, W, mode, motion, capsys):
    """Optional outputs, selection and block sums of ops.pair_loss.
    depth, identity map, reprojection map: <= 4 x the error of the fp32 restatement (largest absolute error and relative L2),
    both evaluated on the kernel's bilinear cells (checked against the float64 cells: near-ties only, <= 0.1 %) and on the
    float64 SSIM clamp flags; the fp32 figure is formed first.  sel: equals the float64 selection except where the float64
    gap is below GAP_LIMIT, <= 0.1 % of the pixels -- the same cap is asserted for the fp32 restatement first.  Block sums:
    against the float64 sum of the candidates the kernel selected, bound = 4 x the summed fp32 map error of the tile + 11 u
    sum (2 terms per thread, 6 shuffle levels, 3 adds, the rounding of identity + noise): the photo_automask tile-sum rule.
    Without the optional outputs the same partials, bit for bit, and nothing else is written."""
    dev = use_backend(backend)
    name = f'pair_loss {H}x{W} B{B} {motion}'
    sc = _scene(61, B, H, W, mode, motion)
    own64 = PR.view_and_maps(sc['disp'], sc['src'], sc['target'], sc['Kinv'], sc['P'], *sc['depths'])
    _, sel_own, _ = PR.select(own64['maps'], sc['noise'])
    frac_id = float((sel_own == 0).double().mean())
    assert 0.2 <= frac_id <= 0.8, frac_id
    if motion in ('left', 'right'):          # a band of samples is clipped at that border; right: its cell is the last column
        ix = own64['ix'][0]
        assert float(((ix <= 0) if motion == 'left' else (ix >= W - 1)).double().mean()) >= 0.05
        if motion == 'right':
            assert float((own64['cell'][0][0] == W - 1).double().mean()) >= 0.05
    # the fp32 restatement on its own decisions stays within the caps
    own32 = PR.view_and_maps(sc['disp'], sc['src'], sc['target'], sc['Kinv'], sc['P'], *sc['depths'], dtype=F32)
    diff, _ = R.cell_mismatch(tuple(c[:1] for c in own32['cell']), tuple(c[:1] for c in own64['cell']), tuple(m[:1] for m in own64['margins']))
    assert int(diff.sum()) <= 1e-3 * B * H * W
    kc = _kernel_cells(sc, dev)
    ref = dict(cell=own64['cell'], margins=own64['margins'])
    T._cells_ok(backend, name, kc, ref)
    r64 = PR.view_and_maps(sc['disp'], sc['src'], sc['target'], sc['Kinv'], sc['P'], *sc['depths'], cell=kc)
    r32 = PR.view_and_maps(sc['disp'], sc['src'], sc['target'], sc['Kinv'], sc['P'], *sc['depths'], dtype=F32, cell=kc, flag=r64['flag'])
    e32 = (r32['maps'].double() - r64['maps']).abs()
    cand, sel64, gap = PR.select(r64['maps'], sc['noise'])
    _, sel32, _ = PR.select(r32['maps'], sc['noise'], F32)
    d32 = sel32 != sel64
    assert int(d32.sum()) <= 1e-3 * d32.numel() and bool((gap[d32] < R.GAP_LIMIT).all())
    # ---- the kernel
    partial, out = _run(sc, dev)
    T._measured(backend, name, 'depth', out['depth'], r64['depth'], r32['depth'], l2=False)
    T._measured(backend, name, 'identity map', out['maps'][0], r64['maps'][0], r32['maps'][0])
    T._measured(backend, name, 'reprojection map', out['maps'][1], r64['maps'][1], r32['maps'][1])
    ksel = out['sel'].cpu()
    assert bool((ksel <= 1).all())
    differ = ksel.long() != sel64
    T._row(backend, name, 'sel differing / px', int(differ.sum()), differ.numel())
    assert bool((gap[differ] < R.GAP_LIMIT).all()) and int(differ.sum()) <= 1e-3 * differ.numel()
    kval = torch.gather(cand, 0, ksel.long()[None])[0]
    tot, tol = _tiles(kval, H, W), 4 * _tiles(e32.max(0).values, H, W) + 11 * U * _tiles(kval, H, W)
    got = partial.cpu().double()
    T._row(backend, name, 'block sums max |d| / tol', float(((got - tot).abs() / tol).max()), 1.0)
    assert bool(((got - tot).abs() <= tol).all())
    # ---- nothing but the partials: optional outputs null, the partials inside a guarded buffer
    nblk = partial.shape[1]
    arena = torch.full((B * nblk + 64,), 7.0, device=dev)
    bystanders = [torch.full((B, H, W), 7.0, device=dev), torch.full((B, H, W), 7, dtype=torch.uint8, device=dev),
                  torch.full((2, B, H, W), 7.0, device=dev)]
    p2 = arena[32:32 + B * nblk].view(B, nblk)
    t = lambda v: v.contiguous().to(dev)
    ops.pair_loss(t(sc['disp']), t(sc['src']), t(sc['target']), t(sc['Kinv']), t(sc['P']), t(sc['noise']), p2, *sc['depths'])
    assert torch.equal(p2, partial)
    assert bool((arena[:32] == 7.0).all()) and bool((arena[32 + B * nblk:] == 7.0).all())
    assert all(bool((b == 7).all()) for b in bystanders)
    T._flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,mode,motion', [CASES[1], CASES[2]])
def test_pair_loss_equals_the_unfused_chain(backend, B, H, W, mode, motion, capsys):
    """warp_fwd with the source frame in both slots, photo_map of the warped image and of the source frame, the two-way minimum
    on the host: per pixel the fused kernel's minimum stays within 4 x the fp32 figure of test_pair_loss (the largest error
    of the fp32 restatement's maps against float64) of the chain's.  The depth is the same bits.
    And against the fused kernel the step uses: photo_automask_pyramid on the pair (warped, source) with the identity
    candidates at +inf takes min(map(warped), map(source)) per pixel through the arithmetic photo_pair_px restates -- its
    block sums and this kernel's (no noise) are the same bits."""
    dev = use_backend(backend)
    sc = _scene(61, B, H, W, mode, motion)
    t = lambda v: v.contiguous().to(dev)
    kc = _kernel_cells(sc, dev)
    r64 = PR.view_and_maps(sc['disp'], sc['src'], sc['target'], sc['Kinv'], sc['P'], *sc['depths'], cell=kc)
    r32 = PR.view_and_maps(sc['disp'], sc['src'], sc['target'], sc['Kinv'], sc['P'], *sc['depths'], dtype=F32, cell=kc, flag=r64['flag'])
    fig = float((r32['maps'].double() - r64['maps']).abs().max())
    partial, out = _run(sc, dev)
    depth = torch.full((B, H, W), NAN, device=dev)
    warped = torch.full((2, B, 3, H, W), NAN, device=dev)
    P2 = torch.stack([sc['P'], sc['P']])
    ops.warp_fwd(t(sc['disp']), t(sc['src']), t(sc['src']), t(sc['Kinv']), t(P2), depth, warped, *sc['depths'])
    assert torch.equal(depth, out['depth'])
    rp, idm = torch.full((B, H, W), NAN, device=dev), torch.full((B, H, W), NAN, device=dev)
    ops.photo_map(warped[0].contiguous(), t(sc['target']), rp, None, B, B, H, W)
    ops.photo_map(t(sc['src']), t(sc['target']), idm, None, B, B, H, W)
    chain = torch.minimum(idm + t(sc['noise'])[:, 0], rp).cpu().double()
    fused = torch.where(out['sel'].bool(), out['maps'][1], out['maps'][0] + t(sc['noise'])[:, 0]).cpu().double()
    d = float((fused - chain).abs().max())
    T._row(backend, f'pair vs chain {H}x{W}', 'minimum max |d| / (4 x fp32)', d, 4 * fig, f'(ratio {d / (4 * fig):.3f})')
    assert d <= 4 * fig, (d, fig)
    # the same pair through photo_automask_pyramid
    nblk = partial.shape[1]
    wall = torch.stack([warped[0], t(sc['src'])])[None].repeat(4, 1, 1, 1, 1, 1).contiguous()
    sel4 = torch.full((4, B, H, W), 9, dtype=torch.uint8, device=dev)
    part4 = torch.full((4, B, nblk), NAN, device=dev)
    ops.photo_automask_pyramid(wall, t(sc['target']), torch.full((2, B, H, W), float('inf'), device=dev), None, sel4, None, part4, B, H, W)
    quiet = dict(sc, noise=torch.zeros_like(sc['noise']))
    p0, o0 = _run(quiet, dev)
    assert torch.equal(p0, part4[0])
    assert torch.equal(o0['sel'].cpu() == 1, sel4[0].cpu() == 2)
    T._flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
def test_pair_loss_rng_is_the_documented_stream(backend):
    """pair_loss_rng(seed, offset) == pair_loss(noise) bit for bit when noise[b, 0, y, x] is out[2 * (b H W + y W + x)] of
    tie_break_noise(seed, offset): the first value of the pair of element b * H * W + pixel (include/clslam_hip.h)."""
    dev = use_backend(backend)
    B, H, W = 2, 20, 36
    sc = _scene(62, B, H, W, 1, 'small')
    seed, offset = 0x1234567890ABCDEF, (3 << 40) | 17
    pairs = torch.full((B * H * W, 2), NAN, device=dev)
    ops.tie_break_noise(pairs, seed, offset)
    noise = pairs[:, 0].reshape(B, 1, H, W).cpu()
    assert 5e-6 < float(noise.std()) < 2e-5
    pr, outr = _run(sc, dev, rng=(seed, offset))
    pn, outn = _run(dict(sc, noise=noise), dev)
    assert torch.equal(pr, pn) and all(torch.equal(outr[k], outn[k]) for k in outr)
    p_other, _ = _run(sc, dev, rng=(seed, offset + 1))
    assert not torch.equal(p_other, pr)


FIN_CASES = [pytest.param((0.5, 0.3, 0.2), (0.1, 0.6, 0.3), False, 0.05, id='quirk-vel'),
             pytest.param((0.7, 0.0, 0.3), (0.0, 0.25, 0.75), False, 0.0, id='quirk-novel'),
             pytest.param((0.2, 0.2, 0.6), None, True, 0.05, id='intended-vel'),
             pytest.param((1.0,), (1.0,), False, 0.0, id='quirk-B1'), pytest.param((1.0,), None, True, 0.0, id='intended-B1')]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('sw,smw,intended,vel', FIN_CASES)
def test_pair_loss_finalize(backend, sw, smw, intended, vel, capsys):
    """The seven scalars at 24x80 against float64, both smoothness modes, with and without the velocity term.
    Bounds as test_disp_mean_and_finalize derives them: every scalar is a sum of non-negative terms, so n terms carrying k
    roundings each stay within (n + k) u of the value; n = nblk + B + n_smooth, k = 16 for the smoothness term.  This entry
    point also forms the disparity means (and the per-sample sums) itself: a chunk sum adds ceil(per / 256) terms per
    thread, 6 shuffle levels, 3 adds, then 32 chunks -- m = ceil(per / 256) + 41 more roundings on the mean (a common factor
    of every smoothness term), 2 ceil(per / 256) + 41 on a per-sample sum.  The flattened terms subtract two ROUNDED quotients
    d / mean: that adds u (|a| + |b|) absolute per difference, summed with the weights (`canc`).  depth_loss is
    depth_loss/scale_0 / 4 exactly (a division by a power of two); the total adds one more term (+ 2)."""
    dev = use_backend(backend)
    B, H, W = len(sw), 24, 80
    g = T._gen(71)
    disp = T._smooth_field(g, B, H, W, 0.05, 0.95)
    rgb0 = torch.rand(B, 3, H, W, generator=g)
    nblk = ops.automask_blocks(H, W)
    partial = (0.03 + 0.05 * torch.rand(B, nblk, generator=g)) * 512
    pose = torch.randn(B, 12, generator=g) * 0.1
    dist = torch.tensor([0.5, -0.8, 0.25][:B], dtype=F64)
    pose[0, 3:6] = torch.tensor([1.0, 0.0, 0.0]) * 0.5          # |t| == |dist| exactly for sample 0
    swt = torch.tensor(sw)
    smt = None if smw is None else torch.tensor(smw)
    losses = torch.full((7,), NAN, device=dev)
    scratch = torch.full((ops.pair_loss_scratch(B),), NAN, device=dev)
    t = lambda v: None if v is None else v.contiguous().to(dev)
    ops.pair_loss_finalize(t(partial), t(disp), t(rgb0), t(pose), t(dist) if vel else None, t(swt), t(smt), intended, scratch, losses,
                           1e-3, vel)
    L64 = PR.finalize(partial, disp, rgb0, pose, dist, swt, smt, intended, H, W, 1e-3, vel)
    L32 = PR.finalize(partial, disp, rgb0, pose, dist, swt, smt, intended, H, W, 1e-3, vel, dtype=F32)
    per = -(-H * W // 32)
    m = -(-per // 256) + 41
    n_smooth = 0 if (smt is None or intended) else len(smw)
    n = nblk + B + n_smooth + 16 + (2 * m if intended else m)
    canc = 0.0
    if n_smooth:
        n0 = disp[0].double() / (disp[0].double().mean() + 1e-7)
        canc = float((U * smt.double() * ((n0[0, :n_smooth].abs() + n0[0, 1:n_smooth + 1].abs()) + (n0[0, :n_smooth].abs() + n0[1, :n_smooth].abs()))).sum())
    tol = n * U * L64
    tol[1] += canc
    tol[2:5] += 1e-3 * canc
    tol[6] = (n + 2) * U * L64[6] + 1e-3 * canc
    got = losses.cpu().double()
    T._row(backend, 'pair_loss_finalize', 'losses max rel', float(((got - L64).abs() / L64.clamp_min(1e-30)).max()),
           float(((L32.double() - L64).abs() / L64.clamp_min(1e-30)).max()), f'(bound {n} u = {n * U:.1e})')
    T._flush(capsys)
    assert float(L64[0]) > 0 and float(L64[1]) > 0
    assert bool(((got - L64).abs() <= tol).all()), ((got - L64).abs() / tol.clamp_min(1e-300)).tolist()
    assert float(losses[4]) == float(losses[3]) / 4
    if vel:
        assert float(got[5]) > 0 and float(got[6]) > float(got[4])
    else:
        assert float(got[5]) == 0 and float(got[6]) == float(got[4])
