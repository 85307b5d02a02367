"""mask_dynamic=True (dpp.py:1063-1090, 1148-1176): "potentially dynamic" pixels (inputs['mask', 0, s] == 1) leave the
reprojection mean and the smoothness, and the reprojection term becomes one mean over the static pixels of the minibatch.

64 x 128 (not square; scale 3 is 8 x 16, so cropped planes and tiles have edges), B = 2 and B = 1.  The float64 reference is
tests/masked_loss_reference.py, which calls torch.masked_select where the reference does; as in tests/loss_reference.py the
kernel's own selection `sel` is imposed on it.

One property of the issue's list is stated more narrowly than there, because the wider form does not hold for the reference
itself: "ddisp_up is exactly 0 at every dynamic pixel" / "flipping image values under the mask changes no loss bit".  SSIM is
a 3 x 3 window statistic (layers.py:107-137), so a dynamic pixel next to a static one is read by that static pixel's term:
its warped value has a non-zero gradient in the reference's autograd and its image value changes the reference's loss.  Both
properties are asserted for every dynamic pixel whose whole 3 x 3 neighbourhood is dynamic -- all pixels they can hold for."""
import functools

import numpy as np
import pytest
import torch

import loss_reference as R
import masked_loss_reference as M
from clslam_hip import ops, synth
from emu_util import BACKENDS, use_backend
from predictor_util import make_predictor

H, W = 64, 128
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
NAN = float('nan')
RECT = (0, 0, 3, 0, 70)         # rows 0-2 of sample 0, columns 0-69: across the x = 64 edge of the 8 x 64 tiles of both kernels

MASKS = {
    'random': dict(dynamic=0.3),
    'rect': dict(dynamic=0.1, rect=RECT),
    'values': dict(dynamic=0.3, static_values=(0.0, 0.5, 2.0)),
    'static': dict(dynamic=0.0),
}


def _batch(B, mask_kw=None, seed=7):
    batch = synth.make_batch(B, H, W, seed=seed)
    if mask_kw is not None:
        batch.update(synth.make_masks(B, H, W, seed=23, **mask_kw))
    return batch


def _step(backend, B, mask_kw, **over):
    """one adapt step -> (predictor, outputs, losses, the dict handed to adapt, its host copy)"""
    use_backend(backend)
    host = _batch(B, mask_kw)
    p = make_predictor(H, W, B, **over)
    p.set_tie_break_noise(synth.make_noise(B, H, W, seed=17))
    given = {k: v.clone() for k, v in host.items()}
    out, losses = p.adapt(None, given, steps=1)
    p.engine.wait_training()
    return p, out, losses, given, host


@functools.lru_cache(maxsize=None)
def _masked_run(backend, B, case, quirks=True, smooth=0.1, vel=0.05):
    return _step(backend, B, MASKS[case], mask_dynamic=True, reference_quirks=quirks, disparity_smoothness=smooth,
                 velocity_loss_scaling=vel)


def _cpu(t):
    return t.detach().cpu()


# ---- 1. constructs and runs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B', [2, 1])
def test_masked_step_runs(backend, B):
    p, out, losses, _, _ = _masked_run(backend, B, 'random')
    assert p.mask_dynamic and p.engine.mask_dynamic
    assert np.isfinite(float(losses['loss'])) and float(losses['loss']) > 0
    assert tuple(out['disp', 0].shape) == (B, 1, H, W)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('missing', [0, 3])
def test_missing_mask_is_a_key_error(backend, missing):
    use_backend(backend)
    batch = _batch(2, MASKS['random'])
    del batch['mask', 0, missing]
    p = make_predictor(H, W, 2, mask_dynamic=True)
    with pytest.raises(KeyError) as e:
        p.adapt(None, batch, steps=1)
    assert e.value.args[0] == ('mask', 0, missing)


# ---- 2. all-static mask = the unmasked path ---------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_all_static_mask_equals_unmasked(backend):
    """Uniform sample weights: sum_b (sum_b / HW) / B = sum / (B HW), so only the order of the arithmetic differs.  Loss
    scalars at the parity bound 1e-4; disparity-logit and pose gradients at the bound tests/test_backward_parity.py holds the
    backward arithmetic to once the selection is the same (relative L2 3e-4) -- the selections ARE the same here."""
    B = 2
    pm, _, lm, _, _ = _masked_run(backend, B, 'static')
    pu, _, lu, _, _ = _step(backend, B, None, disparity_smoothness=0.1)
    for k, v in lu.items():
        assert abs(float(lm[k]) - float(v)) <= 1e-4 * max(abs(float(v)), 1e-4), (k, float(lm[k]), float(v))
    tm, tu = pm.engine._ws[B].train, pu.engine._ws[B].train
    assert torch.equal(pm.engine._ws[B].sel, pu.engine._ws[B].sel)
    pairs = [(f'dz_disp{s}', tm.dz_disp[s], tu.dz_disp[s]) for s in range(4)] + [('dpose', tm.dpose, tu.dpose)]
    for name, a, b in pairs:
        a, b = _cpu(a).double(), _cpu(b).double()
        err = float((a - b).norm() / b.norm())
        assert float(b.norm()) > 0 and err < 3e-4, (name, err)


# ---- 3. kernel-level parity against float64 ---------------------------------------------------------------------------------
def _maps64(ws, c, B, dtype=F64):
    """candidates (4,B,H,W) per scale from the engine's own warped images, in `dtype`"""
    tgt = _cpu(c.rgb[0])
    idm = torch.stack([R.photo_map(_cpu(c.rgb[f]), tgt, dtype)['map'] for f in (-1, 1)])
    noise = _cpu(ws.noise)
    out = []
    for s in range(4):
        rp = R.photo_map(_cpu(ws.warped[s]).reshape(2 * B, 3, H, W), tgt, dtype)['map'].reshape(2, B, H, W)
        cand, _, _ = R.automask(idm, noise[s], rp, dtype)
        out.append(cand)
    return out


def _tiles(v, B):
    ty, tx = -(-H // 8), -(-W // 64)
    return torch.nn.functional.pad(v, (0, tx * 64 - W, 0, ty * 8 - H)).reshape(B, ty, 8, tx, 64).sum((2, 4)).reshape(B, -1)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,case', [(B, case) for B in (2, 1) for case in ('random', 'rect', 'values')])
def test_masked_kernels_against_float64(backend, B, case, capsys):
    """Tile sums and counts, the 18 losses, dz_disp and dp_partial of one masked step, on the tensors the step itself produced.
    Tolerances are those of the unmasked kernel tests (tests/test_loss_kernels.py): tile sums 4 x the fp32 restatement of the
    map + 11 u of the sum; losses (nblk + B + n_smooth + 16) u on top of the map's share; gradients 4 x the fp32 restatement
    (+ the final rounding to fp32 for dz).  Counts and positions are integers: exact."""
    p, _, losses, _, host = _masked_run(backend, B, case)
    eng = p.engine
    ws = eng._ws[B]
    c, t = ws.ctx, ws.train
    masks = [host['mask', 0, s] for s in range(4)]
    st0 = M.static(masks[0])[:, 0]
    if case == 'values':
        assert bool(((masks[0] == 0.5) | (masks[0] == 2.0)).any()) and bool(st0[(masks[0][:, 0] == 0.5) | (masks[0][:, 0] == 2.0)].all())
    sel = _cpu(ws.sel).long()
    c64, c32 = _maps64(ws, c, B), _maps64(ws, c, B, F32)
    kval = [c64[s].gather(0, sel[s][None])[0] for s in range(4)]
    e32 = [(c32[s].double() - c64[s]).abs().max(0).values for s in range(4)]
    # tile sums and counts
    cnt = _cpu(ws.cnt_partial).long()
    assert torch.equal(cnt, _tiles(st0.double(), B).long()) and int(cnt.sum()) == int(st0.sum())
    stf = st0.double()
    for s in range(4):
        tot, tol = _tiles(kval[s] * stf, B), 4 * _tiles(e32[s] * stf, B) + 11 * U * _tiles(kval[s] * stf, B)
        got = _cpu(ws.partial[s]).double()
        assert bool(((got - tot).abs() <= tol).all()), (s, float(((got - tot).abs() - tol).max()))
    mstat = _cpu(ws.mstat).double()
    n_static = int(st0.sum())
    assert float(mstat[1]) == n_static and abs(float(mstat[0]) * n_static - 1) <= 2 * U
    # located positions = masked_select's
    loc = _cpu(ws.loc)
    for s in range(4):
        for d, (b_ref, p_ref) in enumerate(M.quirk_positions(masks[s], B)):
            assert bool((b_ref == 0).all()) and p_ref.numel() == B          # the supported layout
            assert loc[s, d, :B].tolist() == p_ref.tolist(), (s, d)
            assert loc[s, d, B:].tolist() == [1] * B
    if case == 'rect':
        assert int(loc[0, 0, 0]) == RECT[4] and int(loc[0, 1, 0]) == RECT[4]            # off the old layout: not pixel 0
    # the 18 losses
    sw = _cpu(c.sample_w)
    disps, rgb0 = [_cpu(d) for d in ws.disp], [_cpu(x) for x in c.rgb0]
    d0, d1 = _cpu(c.d0), _cpu(c.d1)
    L64 = M.losses(kval, masks, disps, rgb0, _cpu(ws.pose), d0, d1, sw, eng.smooth_scale, eng.vel_scale)
    n = ws.nblk * B + B + B + 16
    tol = n * U * L64.abs()
    for s in range(4):
        share = 4 * float((e32[s] * stf).sum()) / n_static
        tol[4 * s] += share
        tol[4 * s + 3] += share
    tol[17] = (n + 6) * U * L64[17] + sum(4 * float((e32[s] * stf).sum()) / n_static for s in range(4)) / 4
    got = _cpu(ws.losses).double()
    with capsys.disabled():
        print(f'\n  [{backend}] masked losses B={B} {case}: max |d| / tol = {float(((got - L64).abs() / tol).max()):.3f}')
    assert bool(((got - L64).abs() <= tol).all()), ((got - L64).abs() / tol).tolist()
    assert {k: float(v) for k, v in losses.items()} == {k: float(v) for k, v in eng.losses_dict(_cpu(ws.losses)).items()}
    # backward: loss_bwd2 on the step's own tensors, then dz
    dev = ws.sel.device
    dd = torch.full((4, B, H, W), NAN, device=dev)
    dpp = torch.full((4, B, t.nb2, 24), NAN, dtype=F64, device=dev)
    ops.loss_bwd2_pyramid_masked(ws.disp, ws.sel, ws.coef, ws.warped, c.rgb[0], c.rgb[-1], c.rgb[1], c.Kinv, ws.P, c.masks[0],
                                 ws.mstat, dd, dpp, eng.min_depth, eng.max_depth)
    assert torch.equal(dd, t.ddisp_up) and torch.equal(dpp, t.dp_partial)
    cells = torch.zeros(4, 2, B, H, W, dtype=torch.int32, device=dev)
    ops.warp_cells_pyramid(ws.disp, c.Kinv, ws.P, cells, eng.min_depth, eng.max_depth)
    cells = _cpu(cells)
    src_m1, src_p1, tgt, Kinv, P = (_cpu(x) for x in (c.rgb[-1], c.rgb[1], c.rgb[0], c.Kinv, ws.P))
    coef = torch.nan_to_num(_cpu(ws.coef))
    for s in range(4):
        refs = []
        for dt in (F64, F32):
            g = M.photo_backward(_cpu(ws.sel[s]), coef[s], _cpu(ws.warped[s]), tgt, masks[0], dt)
            ddr, dP = R.warp_backward(g, disps[s], src_m1, src_p1, Kinv, P, H, W, eng.min_depth, eng.max_depth,
                                      R.unpack_cells(cells[s]), dt)
            refs.append((ddr, dP.transpose(0, 1).reshape(B, 24)))
        (dd64, dP64), (dd32, dP32) = refs
        assert float(dd64.abs().max()) > 0 and float(dP64.abs().max()) > 0
        for name, gotv, r64, r32 in (('ddisp_up', _cpu(dd[s]), dd64, dd32), ('dP sums', _cpu(dpp[s]).sum(1), dP64, dP32)):
            ek, e3 = float((gotv.double() - r64).abs().max()), float((r32.double() - r64).abs().max())
            nk, n3 = float((gotv.double() - r64).norm()), float((r32.double() - r64).norm())
            assert ek <= 4 * e3 and nk <= 4 * n3, (s, name, ek, e3, nk, n3)
        assert bool((_cpu(dd[s])[~st0 & _eroded(~st0)] == 0).all())
        z64 = M.disp_backward(_cpu(dd[s]), disps[s], rgb0[s], masks[s], H, W, sw, eng.smooth_scale, s)
        z32 = M.disp_backward(_cpu(dd[s]), disps[s], rgb0[s], masks[s], H, W, sw, eng.smooth_scale, s, dtype=F32)
        gz = _cpu(t.dz_disp[s]).double()
        ek, e3 = float((gz - z64).abs().max()), float((z32.double() - z64).abs().max())
        assert ek <= 4 * e3 + 2 * U * float(z64.abs().max()), (s, 'dz_disp', ek, e3)


def _eroded(dyn):
    """(B,H,W) bool -> True where the whole 3 x 3 neighbourhood (inside the image) is True"""
    x = torch.nn.functional.pad(dyn[:, None].float(), (1, 1, 1, 1), value=1.0)
    return (torch.nn.functional.avg_pool2d(x, 3, 1) > 1 - 1e-6)[:, 0]


@pytest.mark.parametrize('backend', BACKENDS)
def test_masked_per_sample_smoothness(backend):
    """reference_quirks=False under the mask: the smoothness scalars against the masked_select restatement (16 + 32 chunk
    sums of non-negative terms: (chunks + pixels / 256 + 16) u) and dz_disp like above."""
    B = 2
    p, _, _, _, host = _masked_run(backend, B, 'random', quirks=False)
    eng = p.engine
    ws = eng._ws[B]
    c, t = ws.ctx, ws.train
    masks = [host['mask', 0, s] for s in range(4)]
    sw = _cpu(c.sample_w)
    got = _cpu(ws.losses).double()
    for s in range(4):
        d = _cpu(ws.disp[s]).double()[:, None]
        norm = d / (d.mean(2, True).mean(3, True) + 1e-7)
        sm = float((M.smooth_intended(norm, _cpu(c.rgb0[s]).double(), masks[s]) * sw.double()).sum())
        assert abs(float(got[4 * s + 1]) - sm) <= (32 + (H * W >> 2 * s) / 256 + 48) * U * sm, (s, float(got[4 * s + 1]), sm)
        z64 = M.disp_backward(_cpu(t.ddisp_up[s]), _cpu(ws.disp[s]), _cpu(c.rgb0[s]), masks[s], H, W, sw, eng.smooth_scale, s, quirks=False)
        z32 = M.disp_backward(_cpu(t.ddisp_up[s]), _cpu(ws.disp[s]), _cpu(c.rgb0[s]), masks[s], H, W, sw, eng.smooth_scale, s, quirks=False,
                              dtype=F32)
        ek, e3 = float((_cpu(t.dz_disp[s]).double() - z64).abs().max()), float((z32.double() - z64).abs().max())
        assert ek <= 4 * e3 + 2 * U * float(z64.abs().max()), (s, ek, e3)


# ---- 4. dynamic pixels get nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_dynamic_pixels_get_nothing(backend):
    B = 2
    p, _, _, _, host = _masked_run(backend, B, 'rect', smooth=0.0, vel=None)
    eng = p.engine
    ws = eng._ws[B]
    c, t = ws.ctx, ws.train
    dyn = ~M.static(host['mask', 0, 0])[:, 0]
    inner = dyn & _eroded(dyn)
    assert int(inner[0, :2, :69].sum()) == 2 * 69 and int((dyn & ~inner).sum()) > 0
    dd = _cpu(t.ddisp_up)
    assert float(dd.abs().max()) > 0
    for s in range(4):
        assert bool((dd[s][inner] == 0).all()), s
    # other image values where only dynamic pixels can see them: no bit of the sums, counts or losses moves
    dev = ws.sel.device
    m = inner.to(dev)

    def rerun(target, warped, idmap):
        partial = torch.full_like(ws.partial, NAN)
        cnt = torch.full_like(ws.cnt_partial, -1)
        sel = torch.empty_like(ws.sel)
        ops.photo_automask_pyramid_masked(warped, target, idmap, ws.noise, 0, 0, c.masks[0], sel, None, partial, cnt, B, H, W)
        out = torch.full((18,), NAN, device=dev)
        mstat = torch.full((2,), NAN, device=dev)
        ops.loss_finalize_masked([partial[s] for s in range(4)], ws.disp, c.rgb0, [ws.means[s] for s in range(4)], ws.pose, None, None,
                                 c.sample_w, None, out, None, cnt, None, mstat, B, ws.nblk, H, W, 0, 0.0, 0.0)
        return _cpu(partial), _cpu(cnt), _cpu(out), _cpu(mstat)
    base = rerun(c.rgb[0], ws.warped, ws.idmap)
    # (the re-run leaves the smoothness out: the reprojection slots and the counts are the step's own bits)
    assert torch.equal(base[0], _cpu(ws.partial)) and torch.equal(base[2][0:16:4], _cpu(ws.losses)[0:16:4]) and torch.equal(base[3], _cpu(ws.mstat))
    flipped = rerun(torch.where(m[:, None], 1 - c.rgb[0], c.rgb[0]), torch.where(m[None, None, :, None], 1 - ws.warped, ws.warped),
                    torch.where(m[None], ws.idmap + 0.25, ws.idmap))
    for a, b in zip(base, flipped):
        assert torch.equal(a, b)


# ---- 5. degenerate masks ---------------------------------------------------------------------------------------------------
def _degenerate_masks(kind, B):
    masks = synth.make_masks(B, H, W, seed=23, dynamic=0.3)
    for s in range(4):
        m = masks['mask', 0, s]
        if kind == 'sample1':
            m[1] = 1.0
        elif kind == 'all':
            m[:] = 1.0
        elif kind == 'few':                 # sample 0: one static element in each cropped plane (< B = 2), sample 1 as drawn
            m[0] = 1.0
            m[0, 0, 2, 3] = 0.0
    return masks


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('kind,quirks', [('sample1', True), ('sample1', False), ('all', True), ('few', True)])
def test_degenerate_masks_raise_nan_loss_and_undo_the_step(backend, kind, quirks):
    use_backend(backend)
    B = 2
    batch = _batch(B)
    masks = _degenerate_masks(kind, B)
    assert all(bool(torch.isfinite(v).all()) for v in list(batch.values()) + list(masks.values()))
    batch.update({k: v.clone() for k, v in masks.items()})
    p = make_predictor(H, W, B, mask_dynamic=True, reference_quirks=quirks, disparity_smoothness=0.1)
    p.set_tie_break_noise(synth.make_noise(B, H, W, seed=17))
    good = _batch(B, MASKS['random'])
    p.adapt(None, good, steps=1)                                        # one good masked step: moments non-zero
    p.engine.wait_training()
    before = (p.engine.w.clone(), p.engine.m.clone(), p.engine.v.clone(), p.engine.adam_step_count)
    with pytest.raises(RuntimeError, match='NaN loss'):
        with _quiet():
            p.adapt(None, batch, steps=1)
    p.engine.wait_training()
    assert torch.equal(p.engine.w, before[0]) and torch.equal(p.engine.m, before[1]) and torch.equal(p.engine.v, before[2])
    assert p.engine.adam_step_count == before[3]
    ws = p.engine._ws[B]
    got = _cpu(ws.losses).double()
    assert bool(torch.isnan(got[17]))
    if kind == 'sample1':
        # the reprojection terms are finite: N_static counts sample 0 only
        st0 = M.static(masks['mask', 0, 0])[:, 0]
        assert int(_cpu(ws.cnt_partial)[1].sum()) == 0 and float(_cpu(ws.mstat)[1]) == int(st0[0].sum())
        c64 = _maps64(ws, ws.ctx, B)
        sel = _cpu(ws.sel).long()
        for s in range(4):
            ref = float(M.reprojection(c64[s].gather(0, sel[s][None])[0], masks['mask', 0, 0]))
            assert abs(float(got[4 * s]) - ref) <= 1e-5 * ref, (s, float(got[4 * s]), ref)
            assert bool(torch.isnan(got[4 * s + 1]))
        if quirks:
            # term 0 is a number, term 1 is NaN, as the second masked_select of the restatement gives them
            d = _cpu(ws.disp[0]).double()[:, None]
            terms = M.smooth_quirk(d / (d.mean(2, True).mean(3, True) + 1e-7), _cpu(ws.ctx.rgb0[0]).double(), masks['mask', 0, 0])
            assert bool(torch.isfinite(terms[0])) and bool(torch.isnan(terms[1]))
            assert _cpu(ws.loc)[0, :, B:].tolist() == [[1, 0], [1, 0]]
    if kind == 'few':
        assert _cpu(ws.loc)[0, :, :B].tolist() == [[2 * W + 3, -1], [2 * W + 3, -1]]


class _quiet:
    """the NaN path prints the loss dict (dpp.py:1116-1117)"""
    def __enter__(self):
        import contextlib
        import io
        self.cm = contextlib.redirect_stdout(io.StringIO())
        return self.cm.__enter__()

    def __exit__(self, *exc):
        return self.cm.__exit__(*exc)


# ---- 6. reproducible ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_masked_step_is_bitwise_reproducible(backend):
    B = 2
    runs = []
    for _ in range(2):
        p, _, _, _, _ = _step(backend, B, MASKS['random'], mask_dynamic=True, disparity_smoothness=0.1)
        ws = p.engine._ws[B]
        runs.append([_cpu(ws.losses), _cpu(ws.partial), _cpu(ws.cnt_partial), _cpu(ws.train.ddisp_up), _cpu(ws.train.dp_partial),
                     _cpu(ws.train.dpose), _cpu(p.engine.g)] + [_cpu(d) for d in ws.train.dz_disp])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_refusals(backend):
    use_backend(backend)
    p = make_predictor(H, W, 2, mask_dynamic=True)
    with pytest.raises(ValueError, match='mask_dynamic'):
        p.enable_data_parallel(4, 0)
    img = torch.rand(3, H, W)
    K = torch.eye(4)[None]
    with pytest.raises(ValueError, match='mask_dynamic'):
        p.predict_from_images(img, img, return_loss=True, camera_matrix=K, inv_camera_matrix=K)
    d0, d1, T = p.predict_from_images(img, img)         # without the loss the call is served as before
    assert d0.shape == (H, W) and T.shape == (4, 4)
