"""The view-synthesis and loss kernels of csrc/geometry.hip and csrc/loss.hip one entry point of `ops` at a time, each on
inputs this file constructs (never the previous kernel's output), against the float64 restatement of tests/loss_reference.py.

Every bound is one of
  * an identity (bitwise): a pyramid launch == the single-scale launches, two launches == each other, an all-identity
    selection gives gradients of exactly 0;
  * a derived figure (the docstring of the test says how): sums of n non-negative fp32 terms are held to n * 2^-24 relative
    (the textbook bound of recursive summation), the sampling positions to the maxima tests/test_warp_positions.py derives;
  * a measured figure: the SAME restatement evaluated in torch float32 on the same input with the same imposed decisions
    gives an error against float64; the kernel is allowed 4 x that, in the same metric (largest absolute error, and relative
    L2 where it says so).  The fp32 figure is computed before the kernel's output is looked at.  Where the kernel is
    deliberately better than fp32 autograd (double accumulators of the pose-gradient sums, the analytic d depth / d (u, v),
    the all-double pose chain) the 4 x bound is kept; it is not tightened to the kernel.

Decisions.  A kernel that decides something itself (bilinear cell and clip flags, 4-way selection, SSIM clamp flag) is
compared on ITS decision: the reference evaluates the smooth part of the formula on the imposed decision, so no pixel is
left out of any comparison or sum.  The decision itself must equal the float64 one except where the float64 margin is
below the fp32 resolution of the quantity (2.5e-4 px in x, 8e-5 px in y, 1e-5 for the gap of the two smallest
candidates, the propagated rounding of the SSIM variances for the clamp flag); a differing decision with a larger margin
fails, and differing cells / selections are capped at 0.1 % of the pixels of a case (asserted for the fp32 restatement
before the kernel is compared).

Measured figures (kernel | torch fp32, against float64), emu = kernel sources on the CPU emulator, hip = gfx950:
the worst case over all cases and scales of each quantity (every row is printed per case when the tests run with -s):
  quantity                                   emu kernel | fp32   (ratio)     hip kernel | fp32   (ratio)
  pose_to_proj T max                           4.75e-08 | 4.75e-08 (1.00x)     4.75e-08 | 4.75e-08 (1.00x)
  pose_to_proj P max                           6.92e-06 | 6.92e-06 (1.00x)     6.92e-06 | 6.92e-06 (1.00x)
  warp_fwd depth max                           9.91e-07 | 6.67e-07 (1.49x)     9.91e-07 | 6.67e-07 (1.49x)
  warp_fwd warped max                          5.33e-06 | 3.13e-06 (1.70x)     5.33e-06 | 3.88e-06 (1.37x)
  warp_fwd warped rel L2                       4.21e-07 | 3.44e-07 (1.22x)     4.21e-07 | 4.14e-07 (1.02x)
  warp_coords ix max px                        9.81e-05 | 7.04e-05 (1.39x)     9.81e-05 | 7.69e-05 (1.28x)
  warp_coords iy max px                        1.46e-05 | 1.04e-05 (1.40x)     2.52e-05 | 1.81e-05 (1.39x)
  cells differing from float64                 <= 1 of 6144 px per scale (a near-tie), both backends
  photo_map map max                            4.39e-05 | 4.29e-05 (1.02x)     3.95e-05 | 4.29e-05 (0.92x)
  photo_map d map / d window max               2.32e-04 | 2.45e-04 (0.95x)     2.08e-04 | 2.45e-04 (0.85x)
  automask block sums, relative                4.58e-08 (bound 7.15e-07)       3.79e-08 (bound 7.15e-07)
  photo_automask sel differing                 <= 1 of 7680 px per scale (a near-tie), both backends
  photo_automask tile sums |d| / bound         0.034                           0.022
  loss_finalize losses max rel                 1.36e-07 | 1.25e-07 (bound 1.8e-06)   the same
  loss_finalize aux max rel                    3.40e-07 | 2.14e-06               the same
  loss_bwd2 ddisp_up max                       7.85e-09 | 3.81e-09 (2.06x)     7.82e-09 | 5.26e-09 (1.49x)
  loss_bwd2 dP sums max                        1.90e-08 | 6.14e-09 (3.09x)     1.46e-07 | 4.38e-08 (3.33x)
  loss_bwd2 dP sums rel L2                     5.79e-07 | 1.88e-07 (3.08x)     1.08e-06 | 3.85e-07 (2.81x)
  photo_grad dpred max                         4.22e-10 | 4.22e-10 (1.00x)     6.12e-10 | 6.12e-10 (1.00x)
  warp_bwd ddisp_up max                        8.09e-09 | 3.81e-09 (2.12x)     7.88e-09 | 5.26e-09 (1.50x)
  warp_bwd dP sums max                         1.90e-08 | 6.14e-09 (3.09x)     1.44e-07 | 7.59e-08 (1.90x)
  disp_grad dz max                             1.97e-09 | 1.74e-09 (1.13x)     5.50e-10 | 4.34e-10 (1.27x)
  disp_grad_pyramid dz max                     2.91e-10 | 3.82e-10 (0.76x)     2.91e-10 | 3.82e-10 (0.76x)
  pose_bwd dpose max (|ref| 2.5e+04)           4.88e-04 | 1.38e-01 (0.004x)    4.88e-04 | 1.38e-01 (0.004x)
  smooth_intended_fwd chunk sums, relative     1.69e-07 | 1.17e-07 (bound 1.3e-06)   1.91e-07 | 1.17e-07 (bound 1.3e-06)
  smooth_intended_fwd T, relative              5.52e-08 | 2.15e-08 (bound 1.3e-06)   4.90e-08 | 2.15e-08 (bound 1.3e-06)
  smooth_intended_finalize aux max rel         2.90e-07 | 1.45e-07 (bound 2.1e-06)   the same
  smooth_intended_finalize losses max rel      2.88e-07 | 1.66e-07 (bound 4.4e-06)   3.58e-07 | 2.48e-07 (bound 4.4e-06)
  smooth_intended_bwd dz max (|ref| 4.8e-04)   1.14e-10 | 8.47e-11 (1.35x)     6.34e-11 | 8.47e-11 (0.75x)
  smooth_intended_bwd dz rel L2                1.88e-07 | 1.64e-07 (1.15x)     1.45e-07 | 1.11e-07 (1.31x)
  (the largest ratio of any smooth_intended_bwd row, any case, scale and smooth_scale: 1.35x emu, 1.31x hip)
photo_grad: before photo_grad_px summed alpha + beta x + gamma y per neighbour (csrc/loss.hip) the emulator gave
photo_grad dpred 3.45e-09 | 3.87e-10 (8.9x): the check that failed.

One-line mutations of the kernels (CPU emulator, scratch copies) and the test of this file that fails; "before" = whether
test_loss_stage.py (as it was), test_backward_parity.py and test_warp_positions.py caught it on the emulator:
  sample_w[0] for sample_w[b] in loss_bwd2_kernel          test_loss_backward[32x96-mode1-small]         before: no
  sample_w[0] for sample_w[b] in pose_bwd_kernel           test_pose_bwd[0.05-random-4-8]                before: no
  `if (x == W - 2) wx[2] = 2.f` dropped (loss_bwd2)        test_loss_backward[32x96-mode1-small]         before: yes
  x1ok = s.x0 + 1 <= W in warp_fwd_kernel                  test_warp_fwd_last_cell_reads_inside_the_image before: no
      (value-neutral inside the image: the extra tap has weight 0; only the read past the last pixel shows)
  s.mx = 1 at the right border in sample_coords            test_loss_backward[32x96-mode0-right]         before: yes
  mode-0/1 branch of `dd = ...` used for mode 2 (bwd2)     test_loss_backward[24x160-mode2-left]         before: yes
  `angle > 0.0` guard removed in pose_bwd_kernel           test_pose_bwd[0.05-random-4-8]                before: no
  dist0 / dist1 swapped in pose_bwd_kernel                 test_pose_bwd[0.05-random-4-8]                before: no
  dPs[fi * 12 + k] -> dPs[k]                               test_pose_bwd[0.05-random-4-8]                before: yes
  `raw.x <= 1.f` dropped from kf (photo_automask)          SURVIVES, equivalent: |S| <= 1 (see _photo_pair), raw > 1 cannot occur;
      dropping `raw.x >= 0.f` survives too: raw < 0 arises only by rounding at S = 1, where the coefficients vanish anyway

The three smooth_intended_* kernels, same procedure; "before" = whether test_smooth_intended.py as it was (one case: 64 x 64,
B = 2, uniform weights, gradients at 3e-2) caught it on the emulator.  Each test named fails at every case but those in ():
  nx / ny swapped in smooth_intended_fwd_kernel            test_smooth_intended_fwd[32x96-B3]  (16x16: nx == ny)  before: no
  nx / ny swapped in smooth_intended_bwd_kernel            test_smooth_intended_bwd[32x96-B3]  (16x16)            before: no
  sample_w[0] for sample_w[b] in the backward              test_smooth_intended_bwd[32x96-B3]  (16x16: B = 1)     before: no
  sample_w[0] for sample_w[b] in the finalize              test_smooth_intended_finalize[arbitrary-32x96-B3] (16x16)  before: no
  `- T * inv * inv / hw` dropped                           test_smooth_intended_bwd[32x96-B3]                     before: yes
  `/ (float)(1 << sc)` dropped in the backward             test_smooth_intended_bwd[32x96-B3]                     before: yes
  si_edge_weight(img, hw, p - 1, p) -> (p, p + 1)          test_smooth_intended_bwd[32x96-B3]                     before: no
  `+=` -> `=` on the dz store                              test_smooth_intended_bwd[32x96-B3]                     before: yes
  `/ 4.f` dropped from the losses[17] update               test_smooth_intended_finalize[arbitrary-32x96-B3]      before: yes
  `y + 1 <= h` in the forward (an edge past the sample)    test_smooth_intended_fwd[32x96-B3]                     before: yes
      (the next sample's first row changes the value; behind the last sample the NaN around the inputs shows it)
  y = p / h for p / w in the backward / in the forward     test_smooth_intended_bwd / _fwd[32x96-B3]  (16x16)     before: no / no
Of the engine-level tests test_smooth_intended.py has now, the 64 x 128 oracle case fails for the forward nx / ny swap and
the two p / h ones but not for the backward nx / ny swap or the edge-weight one (they stay inside its 3e-2);
test_intended_smoothness_gradient_alone fails for all five.  Neither sees sample_w[0] (the engine's weights are uniform).
None survives.
The backward's store: hipcc fused the last product of the gradient into `dz +=` (v_fmac_f32), so on gfx950 the kernel wrote
fl(dz + a * dl) with a * dl unrounded, and dz was not fl32(what was there + what a run on zeros writes); the emulator (no
contraction) could not show it, the gfx950 assembly did.  si_accumulate() in csrc/loss.hip keeps the addition unfused.
"""
import math

import numpy as np
import pytest
import torch

import loss_reference as R
from clslam_hip import ops, synth
from clslam_hip._lib import ClslamError
from emu_util import BACKENDS, use_backend

U = 2.0 ** -24          # unit round-off of fp32
F32, F64 = torch.float32, torch.float64
NAN = float('nan')


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _smooth_field(g, n, h, w, lo, hi, grain=0.02):
    low = torch.rand(n, 1, 4, 6, generator=g)
    f = torch.nn.functional.interpolate(low, [h, w], mode='bicubic', align_corners=False).clamp(0, 1)[:, 0]
    return (lo + (hi - lo) * f + grain * (torch.rand(n, h, w, generator=g) - 0.5)).clamp(lo, hi).contiguous()


def _images(g, B, H, W):
    """three frames (B,3,H,W) in [0, 1]: smooth texture + grain, the source frames shifted copies with their own grain"""
    base = _smooth_field(g, B * 3, H, W + 8, 0.05, 0.95, 0.08).reshape(B, 3, H, W + 8)
    fr = [(base[..., o:o + W] + 0.02 * (torch.rand(B, 3, H, W, generator=g) - 0.5)).clamp(0, 1).contiguous() for o in (1, 4, 7)]
    return fr[0], fr[1], fr[2]          # src_m1, target, src_p1


def _camera(B, H, W):
    """per-sample different intrinsics (focal lengths 4 % apart), inverse taken in float64"""
    K0, _ = synth.camera_matrices(H, W)
    K = torch.as_tensor(np.asarray(K0), dtype=F64).repeat(B, 1, 1)
    for b in range(B):
        K[b, 0, 0] *= 1 + 0.04 * b
        K[b, 1, 1] *= 1 - 0.03 * b
    return K.float().contiguous(), torch.linalg.inv(K).float().contiguous()


def _pyramid_shapes(H, W):
    return [(H >> s, W >> s) for s in range(4)]


def _disps(g, B, H, W, lo=0.2, hi=0.8):
    return [_smooth_field(g, B, h, w, lo, hi) for h, w in _pyramid_shapes(H, W)]


def _ref_depth(mode_depths, disp=0.5):
    return float(R.OF.disp_to_depth(torch.tensor(disp, dtype=F64), *mode_depths))


DEPTH_MODES = {0: (None, None), 1: (0.1, None), 2: (0.1, 100.0)}
# translation of frame +1 in pixels of image shift at the depth of disparity 0.5 (as a fraction of W, H) and along z in
# units of that depth.  A positive x-shift moves the samples to the right, i.e. a band leaves on the right.
MOTIONS = {'small': (0.03, -0.04, 0.05), 'left': (-0.2, 0.02, 0.03), 'right': (0.2, -0.02, 0.03), 'top': (0.02, -0.25, 0.03),
           'bottom': (-0.02, 0.25, 0.03), 'behind': (0.03, 0.04, -1.0)}


def _poses(B, H, W, K, mode, motion):
    """(2B,12) pose rows: a small rotation about an oblique axis (no coordinate sits on an integer) and the translation of
    MOTIONS for frame +1; frame -1 (inverted by pose_to_proj) gets the opposite one so that both leave on the same side"""
    sx, sy, sz = MOTIONS[motion]
    d = _ref_depth(DEPTH_MODES[mode])
    pose = torch.zeros(2 * B, 12)
    for b in range(B):
        t = torch.tensor([sx * W * d / float(K[b, 0, 0]), sy * H * d / float(K[b, 1, 1]), sz * d]) * (1 + 0.1 * b)
        pose[B + b, 0:3] = torch.tensor([0.011, -0.017, 0.013]) * (1 + 0.2 * b)
        pose[B + b, 3:6] = t
        pose[b, 0:3] = torch.tensor([0.009, 0.015, -0.012]) * (1 + 0.2 * b)
        pose[b, 3:6] = -t
    return pose


def _scene(seed, B, H, W, mode, motion):
    g = _gen(seed)
    K, Kinv = _camera(B, H, W)
    src_m1, target, src_p1 = _images(g, B, H, W)
    if motion == 'behind':   # two depth layers, the near one behind the source camera (den < 0), nothing close to den = 0
        disps = [torch.where(torch.arange(w)[None, None, :] < w // 2, 0.75, 0.25) + _smooth_field(g, B, h, w, -0.05, 0.05)
                 for h, w in _pyramid_shapes(H, W)]
    else:
        disps = _disps(g, B, H, W)
    pose = _poses(B, H, W, K, mode, motion)
    P = R.pose_to_proj(pose, K)[1].float().contiguous()          # the test's own projection matrices, rounded to fp32
    return dict(B=B, H=H, W=W, K=K, Kinv=Kinv, src_m1=src_m1, target=target, src_p1=src_p1, disps=disps, pose=pose, P=P,
                depths=DEPTH_MODES[mode], g=g)


# ---- comparison helpers ---------------------------------------------------------------------------------------------------
ROWS = []


def _row(backend, name, what, ek, e32, extra=''):
    ROWS.append(f'  [{backend}] {name:<34} {what:<26} {ek:9.2e} | {e32:9.2e} {extra}')


def _measured(backend, name, what, got, ref64, ref32, l2=True, check=True):
    """largest absolute error (and relative L2) of the kernel <= 4 x that of the fp32 restatement; e32 is formed first"""
    ref64 = ref64.detach().double()
    e32 = float((ref32.detach().double() - ref64).abs().max())
    n32 = float((ref32.detach().double() - ref64).norm())
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), (name, what, 'non-finite output')
    ek, nk = float((got - ref64).abs().max()), float((got - ref64).norm())
    nr = max(float(ref64.norm()), 1e-300)
    _row(backend, name, what + ' max', ek, e32, f'(|ref| max {float(ref64.abs().max()):.2e})')
    assert not check or ek <= 4 * e32, (name, what, 'max', ek, e32)
    if l2:
        _row(backend, name, what + ' rel L2', nk / nr, n32 / nr)
        assert not check or nk <= 4 * n32, (name, what, 'L2', nk / nr, n32 / nr)


def _flush(capsys):
    with capsys.disabled():
        print()
        while ROWS:
            print(ROWS.pop(0))


def _cells_ok(backend, name, kcell, ref, cap_cell=None):
    """the kernel's cells against the float64 decisions: every difference a near-tie, at most 0.1 % of the pixels"""
    diff, wrong = R.cell_mismatch(kcell, ref['cell'], ref['margins'])
    npx = diff[0].numel()
    ndiff = int(diff.any(0).sum())
    _row(backend, name, 'cells differing / px', ndiff, npx)
    assert int(wrong.sum()) == 0, (name, 'a cell or clip flag differs from float64 at a margin above the fp32 resolution',
                                   [(float(ref['margins'][0][i]), float(ref['margins'][1][i])) for i in zip(*torch.nonzero(wrong, as_tuple=True))][:5])
    assert ndiff <= 1e-3 * npx, (name, ndiff, npx)


def _dev_list(ts, dev):
    return [t.contiguous().to(dev) for t in ts]


# ---- pose_to_proj ---------------------------------------------------------------------------------------------------------
def _pose_cases():
    """rows of (axis-angle, translation): angle 0, 1e-8, 1e-3, 0.5 about x, y, z and an oblique axis"""
    axes = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.48, -0.6, 0.64)]
    rows = [((0.0, 0.0, 0.0), (0.3, -0.2, 0.9))]
    for ang in (1e-8, 1e-3, 0.5):
        for k, ax in enumerate(axes):
            rows.append((tuple(ang * a for a in ax), (0.6 - 0.3 * k, 0.5 * (-1) ** k, 0.62 + 0.1 * k)))
    return rows


@pytest.mark.parametrize('backend', BACKENDS)
def test_pose_to_proj(backend, capsys):
    """T and P of every case of _pose_cases() as frame -1 (inverted; |t| ~ 1) and as frame +1, per-sample different K.
    Derived bounds: an entry of R is a sum of two products of factors <= 1 (each factor carries <= 3 roundings: the
    division by angle + 1e-7, sinf / cosf at <= 2 ulp, 1 - cos), so |dR| <= 8 u; the inverted translation is a 3-term dot
    product of those with t: |dT[:, 3]| <= (8 + 3) u sum |R| |t| <= 11 u * sqrt(3) |t|.  P = K T adds a 4-term dot
    product: |dP| <= 4 u (|K| |T|) + |K| |dT|.  The error of torch's fp32 evaluation is printed beside the kernel's."""
    dev = use_backend(backend)
    rows = _pose_cases()
    B = len(rows)
    pose = torch.zeros(2 * B, 12)
    for b, (aa, t) in enumerate(rows):
        pose[b, :3] = pose[B + b, :3] = torch.tensor(aa)
        pose[b, 3:6] = pose[B + b, 3:6] = torch.tensor(t)
    pose[:, 6:] = 7.0                                     # the second predicted frame of the decoder's rows: never read
    K, _ = _camera(B, 32, 96)
    T = torch.full((2, B, 4, 4), NAN, device=dev)
    P = torch.full((2, B, 3, 4), NAN, device=dev)
    ops.pose_to_proj(pose.to(dev), K.to(dev), T, P)
    T64, P64 = R.pose_to_proj(pose, K)
    T32, P32 = R.pose_to_proj(pose, K, F32)
    tn = pose[:, 3:6].double().norm(dim=1).reshape(2, B, 1)
    tolT = torch.full((2, B, 4, 4), 8 * U, dtype=F64)
    tolT[:, :, :3, 3] = 11 * U * math.sqrt(3) * tn
    tolP = 4 * U * torch.matmul(K.double().abs()[None], T64.abs())[:, :, :3] + torch.matmul(K.double().abs()[None], tolT)[:, :, :3]
    dT, dP = (T.cpu().double() - T64).abs(), (P.cpu().double() - P64).abs()
    _row(backend, 'pose_to_proj', 'T max', float(dT.max()), float((T32.double() - T64).abs().max()))
    _row(backend, 'pose_to_proj', 'P max', float(dP.max()), float((P32.double() - P64).abs().max()))
    _flush(capsys)
    assert bool((dT <= tolT).all()), float((dT - tolT).max())
    assert bool((dP <= tolP).all()), float((dP / tolP).max())
    assert torch.equal(T.cpu()[:, :, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(2, B, 4))


# ---- warp_fwd, warp_fwd_pyramid, warp_coords / warp_cells -----------------------------------------------------------------
WARP_CASES = [  # B, H, W, depth mode, motion
    pytest.param(3, 32, 96, 1, 'small', id='32x96-mode1-small'), pytest.param(2, 24, 160, 2, 'left', id='24x160-mode2-left'),
    pytest.param(2, 32, 96, 0, 'right', id='32x96-mode0-right'), pytest.param(2, 32, 96, 1, 'top', id='32x96-mode1-top'),
    pytest.param(2, 32, 96, 2, 'bottom', id='32x96-mode2-bottom'), pytest.param(2, 20, 70, 0, 'small', id='20x70-mode0-ragged'),
    pytest.param(2, 32, 96, 1, 'behind', id='32x96-mode1-behind')]


def _side_fractions(ref, H, W):
    ix, iy = ref['ix'][1], ref['iy'][1]          # frame +1
    return dict(left=float((ix <= 0).double().mean()), right=float((ix >= W - 1).double().mean()),
                top=float((iy <= 0).double().mean()), bottom=float((iy >= H - 1).double().mean()))


def _kernel_cells(sc, dev):
    B, H, W = sc['B'], sc['H'], sc['W']
    cells = torch.full((4, 2, B, H, W), -1, dtype=torch.int32, device=dev)
    ops.warp_cells_pyramid(_dev_list(sc['disps'], dev), sc['Kinv'].to(dev), sc['P'].to(dev), cells, *sc['depths'])
    return [R.unpack_cells(cells[s].cpu()) for s in range(4)]


def _refs(sc, s, dtype, cell=None):
    return R.warp_fwd(sc['disps'][s], sc['src_m1'], sc['src_p1'], sc['Kinv'], sc['P'], sc['H'], sc['W'], *sc['depths'], dtype=dtype, cell=cell)


def _check_motion(sc, motion, ref):
    """the case does what its name says: >= 5 % of the samples of frame +1 clipped on that side (for right / bottom these
    are the samples whose cell is the last column / row), part of the image behind the source camera"""
    H, W = sc['H'], sc['W']
    fr = _side_fractions(ref, H, W)
    if motion in fr:
        assert fr[motion] >= 0.05, (motion, fr)
        if motion == 'right':
            assert float((ref['cell'][0][1] == W - 1).double().mean()) >= 0.05
        if motion == 'bottom':
            assert float((ref['cell'][1][1] == H - 1).double().mean()) >= 0.05
    if motion == 'behind':
        neg = float((ref['den'] < 0).double().mean())
        assert 0.1 < neg < 0.9 and float(ref['den'].abs().min()) > 0.02, (neg, float(ref['den'].abs().min()))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,mode,motion', WARP_CASES)
def test_warp_fwd(backend, B, H, W, mode, motion, capsys):
    """depth and warped of warp_fwd_pyramid against float64, warped on the kernel's own cells (warp_cells_pyramid); the four
    single-scale launches of warp_fwd write the same bits (the ragged case upsamples 10x35 to 20x70 at scale 1); the
    positions of warp_coords_pyramid within the derived maxima 2.5e-4 / 8e-5 px of the float64 ones and within 4 x the fp32
    restatement's error (the den < 0 case: the latter only -- a perspective division by a small negative den amplifies the
    rounding of P X beyond the figure derived for ordinary motion)."""
    dev = use_backend(backend)
    name = f'warp_fwd {H}x{W} m{mode} {motion}'
    sc = _scene(11, B, H, W, mode, motion)
    disps_d = _dev_list(sc['disps'], dev)
    t = lambda v: v.contiguous().to(dev)
    ref64 = [_refs(sc, s, F64) for s in range(4)]
    _check_motion(sc, motion, ref64[0])
    # the fp32 restatement's own decisions stay within the cap
    for s in range(4):
        own32 = _refs(sc, s, F32)['cell']
        diff, _ = R.cell_mismatch(own32, ref64[s]['cell'], ref64[s]['margins'])
        assert int(diff.any(0).sum()) <= 1e-3 * B * H * W, (s, int(diff.any(0).sum()))
    kcells = _kernel_cells(sc, dev)
    depth = torch.full((4, B, H, W), NAN, device=dev)
    warped = torch.full((4, 2, B, 3, H, W), NAN, device=dev)
    ops.warp_fwd_pyramid(disps_d, t(sc['src_m1']), t(sc['src_p1']), t(sc['Kinv']), t(sc['P']), depth, warped, *sc['depths'])
    coords = torch.full((4, 2, B, H, W, 2), NAN, device=dev)
    ops.warp_coords_pyramid(disps_d, t(sc['Kinv']), t(sc['P']), coords, *sc['depths'])
    for s in range(4):
        d1 = torch.full((B, H, W), NAN, device=dev)
        w1 = torch.full((2, B, 3, H, W), NAN, device=dev)
        ops.warp_fwd(disps_d[s], t(sc['src_m1']), t(sc['src_p1']), t(sc['Kinv']), t(sc['P']), d1, w1, *sc['depths'])
        assert torch.equal(d1, depth[s]) and torch.equal(w1, warped[s]), s
        _cells_ok(backend, name + f' s{s}', kcells[s], ref64[s])
        r64, r32 = _refs(sc, s, F64, kcells[s]), _refs(sc, s, F32, kcells[s])
        _measured(backend, name + f' s{s}', 'depth', depth[s], r64['depth'], r32['depth'], l2=False)
        _measured(backend, name + f' s{s}', 'warped', warped[s], r64['warped'], r32['warped'])
        for c, (key, lim, n) in enumerate((('ix', R.X_LIMIT, W), ('iy', R.Y_LIMIT, H))):
            got = coords[s, ..., c].cpu().double()
            e = (got - r64[key].clamp(0, n - 1)).abs()
            e32 = (r32[key].double().clamp(0, n - 1) - r64[key].clamp(0, n - 1)).abs()
            _row(backend, name + f' s{s}', key + ' max px', float(e.max()), float(e32.max()))
            assert float(e.max()) <= 4 * float(e32.max()), (s, key)
            if motion != 'behind':
                assert float(e.max()) <= lim, (s, key, float(e.max()))
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
def test_warp_fwd_last_cell_reads_inside_the_image(backend):
    """Every sample pushed beyond the bottom-right corner: the cell is (W-1, H-1), its right and lower neighbours do not exist,
    and warped must be the corner pixel of the source bit for bit (weight 1 on one tap).  The source frames are views of a
    buffer whose next element is NaN: a tap taken at x0 + 1 or y0 + 1 there has weight 0 but would still turn the last
    sample's last channel into NaN (x1ok / y1ok of warp_fwd_kernel; the addresses are clamped, so nothing is read outside)."""
    dev = use_backend(backend)
    B, H, W = 2, 20, 70
    g = _gen(13)
    K, Kinv = _camera(B, H, W)
    n = B * 3 * H * W
    bufs = [torch.cat([torch.rand(n, generator=g), torch.tensor([NAN])]).to(dev) for _ in range(2)]
    src = [b[:n].view(B, 3, H, W) for b in bufs]
    pose = torch.zeros(2 * B, 12)
    pose[B:, 3], pose[B:, 4] = 40.0, 15.0             # frame +1: far to the right and down at every depth
    pose[:B, 3], pose[:B, 4] = -40.0, -15.0           # frame -1 is inverted
    P = R.pose_to_proj(pose, K)[1].float().contiguous()
    disps = _disps(g, B, H, W)
    ref = R.warp_fwd(disps[1], src[0].cpu(), src[1].cpu(), Kinv, P, H, W, 0.1, None)
    assert bool((ref['cell'][0] == W - 1).all()) and bool((ref['cell'][1] == H - 1).all())
    depth = torch.full((B, H, W), NAN, device=dev)
    warped = torch.full((2, B, 3, H, W), NAN, device=dev)
    ops.warp_fwd(disps[1].to(dev), src[0], src[1], Kinv.to(dev), P.to(dev), depth, warped, 0.1, None)
    for fi in range(2):
        assert torch.equal(warped[fi], src[fi][:, :, H - 1:, W - 1:].expand(B, 3, H, W)), fi


# ---- photo_map ------------------------------------------------------------------------------------------------------------
def _photo_pair(g, B, H, W):
    """pred (2B,3,H,W), target (B,3,H,W) with the kinks of the photometric term built in (regions of sample 0 / pred 0):
    a constant patch, patches saturated at 0 and at 1, pred == target exactly, and an anti-correlated texture.
    raw > 1 itself cannot be built: |2 mu_x mu_y + C1| <= mu_x^2 + mu_y^2 + C1 and |2 sigma_xy + C2| <= sigma_x + sigma_y + C2
    (Cauchy-Schwarz) give |S| <= 1, so raw = (1 - S) / 2 lies in [0, 1] for every real image and leaves it only by rounding,
    which happens at S = 1 (raw = -1e-8 where pred == target) but not at S = -1: that needs mu_x = -mu_y, and even then C1
    keeps S above -1 + 2 C1 / (2 mu^2 + C1), 4e-4 for |mu| <= 0.5, against a rounding of 1e-5.  The upper clamp and the
    `raw <= 1` half of the flag are unreachable; the anti-correlated patch takes raw as far up as it goes (> 0.9)."""
    _, target, _ = _images(g, B, H, W)
    pred = (target.repeat(2, 1, 1, 1) + 0.05 * (torch.rand(2 * B, 3, H, W, generator=g) - 0.5)).clamp(0, 1)
    target[0, :, 2:8, 3:12] = 0.4375;  pred[0, :, 2:8, 3:12] = 0.4375           # constant, equal (zero variance, raw = 0)
    target[0, :, 2:8, 14:22] = 0.0;    pred[0, :, 2:8, 16:24] = 0.0             # saturated at 0, partly overlapping
    target[0, :, 2:8, 26:34] = 1.0;    pred[0, :, 2:8, 28:36] = 1.0             # saturated at 1
    pred[0, :, 10:16, 3:20] = target[0, :, 10:16, 3:20]                         # pred == target on a textured region
    chk = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2).float()
    target[0, :, 10:18, 40:60] = 0.5 + 0.3 * (chk[10:18, 40:60] - 0.5)          # anti-correlated checkerboards
    pred[0, :, 10:18, 40:60] = 0.5 - 0.3 * (chk[10:18, 40:60] - 0.5)
    pred[B:, :, :, :2] = target[:, :, :, :2]                                    # ... and equality on the reflected border
    return pred.contiguous(), target.contiguous()


def _flag_resolution(ref):
    """fp32 resolution of raw = (1 - S) / 2, S = n1 n2 / (d1 d2): the three variances E[ab] - mu_a mu_b are differences of
    numbers <= 1 carrying 2 roundings each, |d sigma| <= 4 u; n2 = 2 sigma_xy + C2 and d2 = sigma_x + sigma_y + C2 move by
    <= 8 u, so |dS| <= (n1 / d1) (8 u / d2) (1 + |S|) <= 8 u (1 + |S|) / d2 and |d raw| is half of that."""
    S = 1 - 2 * ref['raw']
    return 4 * U * (1 + S.abs()) / ref['d2']


def _check_flags(name, kflag, ref):
    differ = kflag != ref['flag']
    wrong = differ & (ref['flag_margin'] >= _flag_resolution(ref))
    assert int(wrong.sum()) == 0, (name, 'SSIM clamp flag differs from float64 away from the kink', int(wrong.sum()))


@pytest.mark.parametrize('backend', BACKENDS)
def test_photo_map(backend, capsys):
    """map of photo_map against the float64 SSIM + L1, and the nine coefficients as d map / d (window element) = alpha +
    beta x_r + gamma y_r against float64 autograd through the reflection-padded windows, at 20x70 (ragged), B = 2,
    npred = 4, on the images of _photo_pair.  The clamp flag of the kernel is read off its gamma coefficient (2 n1 / d > 0
    unless the flag cleared it); the comparison imposes it.  With and without `coef` the map has the same bits."""
    dev = use_backend(backend)
    B, H, W = 2, 20, 70
    pred, target = _photo_pair(_gen(21), B, H, W)
    own = R.photo_map(pred, target)
    assert float(own['raw'].max()) > 0.9 and float((own['raw'] < 1e-9).double().mean()) > 0.01     # the kinks are there
    assert float((own['l1_margin'] == 0).double().mean()) > 0.02
    out = torch.full((2 * B, H, W), NAN, device=dev)
    out2 = torch.full((2 * B, H, W), NAN, device=dev)
    coef = torch.full((2 * B, 9, H, W), NAN, device=dev)
    ops.photo_map(pred.to(dev), target.to(dev), out, coef, 2 * B, B, H, W)
    ops.photo_map(pred.to(dev), target.to(dev), out2, None, 2 * B, B, H, W)
    assert torch.equal(out, out2)
    kflag = coef.cpu()[:, 2::3] != 0
    own['d2'] = _d2(pred, target)
    _check_flags('photo_map', kflag, own)
    r64, r32 = R.photo_map(pred, target, F64, kflag), R.photo_map(pred, target, F32, kflag)
    _measured(backend, 'photo_map 20x70', 'map', out, r64['map'], r32['map'])
    _measured(backend, 'photo_map 20x70', 'd map / d window', R.coef_window_gradient(coef.cpu(), pred, target), r64['gw'], r32['gw'])
    # the reference's own coefficients (used as inputs of the backward tests) state the same derivative
    cref = R.ssim_coefficients(pred, target, F64, kflag)
    assert float((R.coef_window_gradient(cref, pred, target) - r64['gw']).abs().max()) <= 1e-9 * float(r64['gw'].abs().max())
    _flush(capsys)


def _d2(pred, target):
    xw, yw = R.windows(pred.double()), R.windows(target.double().repeat(pred.shape[0] // target.shape[0], 1, 1, 1))
    return (xw * xw).mean(2) - xw.mean(2) ** 2 + (yw * yw).mean(2) - yw.mean(2) ** 2 + 0.03 ** 2


# ---- automask, automask_pyramid, photo_automask_pyramid -------------------------------------------------------------------
def _sel_ok(backend, name, ksel, cand, sel64, gap):
    differ = ksel.long() != sel64
    _row(backend, name, 'sel differing / px', int(differ.sum()), differ.numel())
    # a differing selection is legitimate only between candidates closer than the fp32 resolution of the gap
    kval = torch.gather(cand, 0, ksel.long()[None])[0]
    assert bool(((kval - cand.min(0).values)[differ] < R.GAP_LIMIT).all()) and bool((gap[differ] < R.GAP_LIMIT).all()), name
    assert int(differ.sum()) <= 1e-3 * differ.numel(), (name, int(differ.sum()))
    return kval


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W', [(3, 32, 96), (2, 24, 160), (2, 20, 70)])
@pytest.mark.parametrize('with_noise', [True, False])
def test_automask(backend, B, H, W, with_noise, capsys):
    """sel and the block sums of automask / automask_pyramid on maps the test draws.  Sample 0 is a standing vehicle: both
    identity maps are equal, and without noise the lowest index wins (sel never 1 there).  Without noise every candidate is
    an input, so sel must equal the float64 selection exactly.  Block sums, derived: a block adds cdiv(ppb, 256) terms per
    thread, 6 shuffle levels and 3 adds of non-negative terms: |d sum| <= (cdiv(ppb, 256) + 10) u sum (the +1 covers the
    rounding of idmap + noise)."""
    dev = use_backend(backend)
    g = _gen(31)
    idmap = 0.02 + 0.05 * torch.rand(2, B, H, W, generator=g)
    idmap[1, 0] = idmap[0, 0]
    rpmap = 0.02 + 0.05 * torch.rand(4, 2, B, H, W, generator=g)
    rpmap[:, 1, :, :4] = rpmap[:, 0, :, :4]                              # exact ties between the reprojections too
    noise = 1e-5 * torch.randn(4, B, 2, H, W, generator=g) if with_noise else None
    nblk = ops.automask_blocks(H, W)
    sel = torch.full((4, B, H, W), 9, dtype=torch.uint8, device=dev)
    partial = torch.full((4, B, nblk), NAN, device=dev)
    ops.automask_pyramid(idmap.to(dev), None if noise is None else noise.to(dev), rpmap.to(dev), sel, partial, B, H, W)
    n = -(-(-(-H * W // nblk)) // 256) + 10
    for s in range(4):
        sel1 = torch.full((B, H, W), 9, dtype=torch.uint8, device=dev)
        part1 = torch.full((B, nblk), NAN, device=dev)
        ops.automask(idmap.to(dev), None if noise is None else noise[s].to(dev), rpmap[s].to(dev), sel1, part1, B, H, W)
        assert torch.equal(sel1, sel[s]) and torch.equal(part1, partial[s])
        cand, sel64, gap = R.automask(idmap, None if noise is None else noise[s], rpmap[s])
        if with_noise:
            kval = _sel_ok(backend, f'automask {H}x{W} s{s}', sel[s].cpu(), cand, sel64, gap)
        else:
            assert torch.equal(sel[s].cpu().long(), sel64) and not bool((sel[s].cpu()[0] == 1).any())
            assert bool((sel[s].cpu()[:, :4] != 3).all())
            kval = cand.min(0).values
        tot, got = kval.sum((1, 2)), partial[s].cpu().double().sum(1)
        _row(backend, f'automask {H}x{W} s{s}', 'sum of minima rel', float(((got - tot).abs() / tot).max()), n * U)
        assert bool(((got - tot).abs() <= n * U * tot).all())
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W', [(3, 32, 96), (2, 24, 160)])
@pytest.mark.parametrize('with_noise', [True, False])
def test_photo_automask_pyramid(backend, B, H, W, with_noise, capsys):
    """The fused map + automask kernel on warped images the test draws (sample 0 a standing vehicle: src_m1 == src_p1, so the
    identity candidates tie exactly).  sel against float64 (near-ties only, <= 0.1 %); the per-tile sums against the float64
    sum of the candidates the kernel selected, bound = 4 x the summed elementwise error of the fp32 restatement's maps
    + the summation bound (2 terms per thread, 6 shuffle levels, 3 adds: 11 u sum); coef_sel against float64 autograd of the
    selected frame's map.  coef_sel is NOT bitwise photo_map's coefficient: this kernel divides by 9 with a reciprocal +
    correction step and forms 1 / (d1 d2) with the hardware reciprocal, photo_map divides; both are held to the 4 x bound.
    Pixels that selected an identity candidate keep their pre-filled NaN in coef_sel (nothing reads them).
    The fp32 restatement's own maps must stay within the 1e-5 of the selection rule on this input (asserted first)."""
    dev = use_backend(backend)
    g = _gen(41)
    # strongly textured, unsaturated images: the fp32 rounding of the SSIM variances is divided by sigma_x + sigma_y + C2,
    # and on flat or saturated windows that alone moves a map by more than the 1e-5 the selection is held to
    target = _smooth_field(g, B * 3, H, W, 0.3, 0.7, 0.0).reshape(B, 3, H, W) + 0.6 * (torch.rand(B, 3, H, W, generator=g) - 0.5)
    src_m1, src_p1 = (target + 0.1 * (torch.rand(B, 3, H, W, generator=g) - 0.5) for _ in range(2))
    src_m1[0] = src_p1[0]
    warped = (target[None, None] + 0.03 * (torch.rand(4, 2, B, 3, H, W, generator=g) - 0.5)).contiguous()
    warped[..., W // 2:] = torch.rand(4, 2, B, 3, H, W - W // 2, generator=g)                 # right half: the identity wins
    ids = torch.stack([src_m1, src_p1]).reshape(2 * B, 3, H, W)
    idmap = R.photo_map(ids, target)['map'].float().reshape(2, B, H, W).contiguous()
    assert torch.equal(idmap[0, 0], idmap[1, 0])
    noise = 1e-5 * torch.randn(4, B, 2, H, W, generator=g) if with_noise else None
    nblk = ops.automask_blocks(H, W)
    outs = []
    for _ in range(2):
        sel = torch.full((4, B, H, W), 9, dtype=torch.uint8, device=dev)
        coef = torch.full((4, B, 9, H, W), NAN, device=dev)
        partial = torch.full((4, B, nblk), NAN, device=dev)
        ops.photo_automask_pyramid(warped.to(dev), target.to(dev), idmap.to(dev), None if noise is None else noise.to(dev), sel, coef,
                                   partial, B, H, W)
        sel_i = torch.full((4, B, H, W), 9, dtype=torch.uint8, device=dev)
        part_i = torch.full((4, B, nblk), NAN, device=dev)
        ops.photo_automask_pyramid(warped.to(dev), target.to(dev), idmap.to(dev), None if noise is None else noise.to(dev), sel_i, None,
                                   part_i, B, H, W)
        assert torch.equal(sel_i, sel) and torch.equal(part_i, partial)          # inference form: same selection, same sums
        outs.append((sel.cpu(), coef.cpu(), partial.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    assert torch.equal(torch.nan_to_num(outs[0][1], nan=7.0), torch.nan_to_num(outs[1][1], nan=7.0))
    sel, coef, partial = outs[0]
    ty, tx = -(-H // 8), -(-W // 64)
    for s in range(4):
        name = f'photo_automask {H}x{W} s{s}' + ('' if with_noise else ' no noise')
        pm64, pm32 = (R.photo_map(warped[s].reshape(2 * B, 3, H, W), target, dt) for dt in (F64, F32))
        assert float((pm32['map'].double() - pm64['map']).abs().max()) < R.GAP_LIMIT
        cand, sel64, gap = R.automask(idmap, None if noise is None else noise[s], pm64['map'].reshape(2, B, H, W))
        frac = float((sel64 >= 2).double().mean())
        assert 0.2 < frac < 0.8, frac
        kval = _sel_ok(backend, name, sel[s], cand, sel64, gap)
        if not with_noise:
            assert not bool((sel[s][0] == 1).any())
        e32 = (pm32['map'].double() - pm64['map']).abs().reshape(2, B, H, W).max(0).values
        tiles = lambda v: torch.nn.functional.pad(v, (0, tx * 64 - W, 0, ty * 8 - H)).reshape(B, ty, 8, tx, 64).sum((2, 4)).reshape(B, -1)
        tot, tol = tiles(kval), 4 * tiles(e32) + 11 * U * tiles(kval)
        got = partial[s].double()
        _row(backend, name, 'tile sums max |d| / tol', float(((got - tot).abs() / tol).max()), 1.0)
        assert bool(((got - tot).abs() <= tol).all())
        # coefficients of the selected frame
        chosen = sel[s] >= 2
        assert bool(torch.isnan(coef[s]).all(1)[~chosen].all()) and bool(torch.isfinite(coef[s]).all(1)[chosen].all())
        both = warped[s].reshape(2 * B, 3, H, W)
        own = R.photo_map(both, target)
        own['d2'] = _d2(both, target)
        mine = torch.stack([sel[s] == 2, sel[s] == 3]).reshape(2 * B, 1, H, W)             # frame f is the selected one
        kflag = torch.where(mine, (torch.nan_to_num(coef[s])[:, 2::3] != 0).repeat(2, 1, 1, 1), own['flag'])
        _check_flags(name, kflag, own)
        r64, r32 = R.photo_map(both, target, F64, kflag), R.photo_map(both, target, F32, kflag)
        m = mine[:, :, None].double()
        got = R.coef_window_gradient(torch.nan_to_num(coef[s]).repeat(2, 1, 1, 1), both, target) * m
        _measured(backend, name, 'coef_sel as d map / d win', got, r64['gw'] * m, r32['gw'] * m)
    _flush(capsys)


# ---- disp_mean, loss_finalize ---------------------------------------------------------------------------------------------
FINALIZE_CASES = [  # sample_w, smooth_w, |t| relative to the ground-truth distance per sample
    pytest.param((0.5, 0.3, 0.2), (0.1, 0.6, 0.3), (1.5, 0.5, 1.2), id='nonuniform'),
    pytest.param((0.7, 0.0, 0.3), (0.0, 0.25, 0.75), (0.6, 1.7, 1.0), id='zero-weight'),
    pytest.param((0.2, 0.2, 0.6), None, (0.5, 1.5, 0.9), id='n_smooth0')]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('sw,smw,trel', FINALIZE_CASES)
def test_disp_mean_and_finalize(backend, sw, smw, trel, capsys):
    """disp_mean / disp_mean_pyramid (the same bits; chunk sums against float64) and the 18 losses and the smoothness
    bookkeeping of loss_finalize at 32x96, B = 3, with sample weights and smoothness weights that differ from each other and
    between samples, a zero weight, translations on both sides of |t| = relative_distance and one exactly on it.
    Derived bounds: every loss is a sum of NON-NEGATIVE terms (minima of maps, absolute values, non-negative weights), so
    recursive summation of n terms that carry k roundings each is within (n + k) u of the value: n = nblk + B + n_smooth
    terms, k = 16 (the smoothness term: two divisions by the mean, a 3-term sum, expf at 2 ulp, three products); the total
    adds the four scales and the velocity: + 6.  aux: 1 / (mean + 1e-7) from 32 chunk sums: 40 u; gxs, gys products of five
    factors, one of them expf: 10 u; fb a sum of 2 n_smooth non-negative products of those: (2 n_smooth + 24) u."""
    dev = use_backend(backend)
    B, H, W = 3, 32, 96
    g = _gen(51)
    disps = _disps(g, B, H, W, 0.05, 0.95)
    rgb0 = [torch.rand(B, 3, h, w, generator=g) for h, w in _pyramid_shapes(H, W)]
    chunks = ops.disp_mean_chunks()
    means = torch.full((4, B, chunks), NAN, device=dev)
    ops.disp_mean_pyramid(_dev_list(disps, dev), means, H, W)
    for s in range(4):
        m1 = torch.full((B, chunks), NAN, device=dev)
        ops.disp_mean(disps[s].to(dev), m1)
        assert torch.equal(m1, means[s])
        hw = disps[s][0].numel()
        per = -(-hw // chunks)
        ref = torch.nn.functional.pad(disps[s].double().reshape(B, hw), (0, per * chunks - hw)).reshape(B, chunks, per).sum(2)
        assert bool(((means[s].cpu().double() - ref).abs() <= (-(-per // 256) + 10) * U * ref).all()), s
    # finalize on inputs of its own: block sums and chunk sums drawn / rounded by the test
    nblk = ops.automask_blocks(H, W)
    partials = [(0.03 + 0.05 * torch.rand(B, nblk, generator=g)) * 512 for _ in range(4)]
    mean_in = [torch.nn.functional.pad(disps[s].double().reshape(B, -1), (0, -(-disps[s][0].numel() // chunks) * chunks - disps[s][0].numel()))
               .reshape(B, chunks, -1).sum(2).float() for s in range(4)]
    dist0, dist1 = torch.tensor([0.5, 0.8, 0.25], dtype=F64), torch.tensor([-0.4, 0.6, 0.25], dtype=F64)   # (|.| is taken)
    pose = torch.randn(2 * B, 12, generator=g) * 0.1
    for b in range(B):
        for fi, d in enumerate((dist0, dist1)):
            t = torch.tensor([1.0, 0.0, 0.0]) if trel[b] == 1.0 else torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
            pose[fi * B + b, 3:6] = t * abs(float(d[b])) * trel[b]
    swt = torch.tensor(sw)
    n_smooth = 0 if smw is None else len(smw)
    smt = None if smw is None else torch.tensor(smw)
    losses = torch.full((18,), NAN, device=dev)
    aux = torch.full((4, 2 + 2 * n_smooth), NAN, device=dev) if n_smooth else None
    ops.loss_finalize(_dev_list(partials, dev), _dev_list(disps, dev), _dev_list(rgb0, dev), _dev_list(mean_in, dev), pose.to(dev),
                      dist0.to(dev), dist1.to(dev), swt.to(dev), None if smt is None else smt.to(dev), losses, aux, B, nblk, H, W,
                      n_smooth, 1e-3, 0.05)
    L64, A64 = R.finalize(partials, disps, rgb0, mean_in, pose, dist0, dist1, swt, smt, H, W, n_smooth, 1e-3, 0.05)
    L32, A32 = R.finalize(partials, disps, rgb0, mean_in, pose, dist0, dist1, swt, smt, H, W, n_smooth, 1e-3, 0.05, dtype=F32)
    assert float(L64[16]) > 0 and all(float(L64[4 * s]) > 0 for s in range(4))
    n = nblk + B + n_smooth + 16
    tol = torch.full((18,), n * U, dtype=F64) * L64
    tol[17] = (n + 6) * U * L64[17]
    got = losses.cpu().double()
    _row(backend, 'loss_finalize', 'losses max rel', float(((got - L64).abs() / L64.clamp_min(1e-30)).max()),
         float(((L32.double() - L64).abs() / L64.clamp_min(1e-30)).max()), f'(bound {n} u = {n * U:.1e})')
    assert bool(((got - L64).abs() <= tol).all()), ((got - L64).abs() / tol.clamp_min(1e-300)).tolist()
    if n_smooth:
        ga = aux.cpu().double()
        tol_a = torch.full_like(A64, 10 * U) * A64.abs()
        tol_a[:, 0] = 40 * U * A64[:, 0]
        tol_a[:, 1] = (2 * n_smooth + 24) * U * A64[:, 1].abs()
        assert bool((A64[:, 1] > 0).all()) and bool((A64[:, 2:] != 0).any())
        _row(backend, 'loss_finalize', 'aux max rel', float(((ga - A64).abs() / A64.abs().clamp_min(1e-30)).max()),
             float(((A32.double() - A64).abs() / A64.abs().clamp_min(1e-30)).max()))
        assert bool(((ga - A64).abs() <= tol_a).all()), ((ga - A64).abs() / tol_a.clamp_min(1e-300)).max(1).values.tolist()
    _flush(capsys)


# ---- the loss backward ----------------------------------------------------------------------------------------------------
def _selection(g, s, B, H, W, identity=False):
    """constructed selections per scale: 0 one-pixel stripes on and next to each border (the reflection fold), 1 a 2 / 3
    checkerboard, 2 all 2 / all 3 by sample, 3 a random mix of all four"""
    ys, xs = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    sel = torch.zeros(B, H, W, dtype=torch.uint8)
    if identity:
        return (torch.rand(B, H, W, generator=g) < 0.5).to(torch.uint8)
    for b in range(B):
        if s == 0:
            cols, rows = ((xs == 0) | (xs == W - 2), (ys == 1) | (ys == H - 1)) if b % 2 == 0 else ((xs == 1) | (xs == W - 1), (ys == 0) | (ys == H - 2))
            a, c = (2, 3) if b % 2 == 0 else (3, 2)
            sel[b] = torch.where(cols, a, torch.where(rows, c, b % 2)).to(torch.uint8)
        elif s == 1:
            sel[b] = (2 + (ys + xs + b) % 2).to(torch.uint8)
        elif s == 2:
            sel[b] = 2 + b % 2
        else:
            sel[b] = torch.randint(0, 4, (H, W), generator=g).to(torch.uint8)
    return sel


def _backward_inputs(sc, identity=False):
    """per scale: warped (the float64 warp rounded to fp32), sel (constructed), coef_sel (float64 coefficients of the selected
    frame rounded to fp32, NaN where an identity candidate is selected)"""
    B, H, W = sc['B'], sc['H'], sc['W']
    warped, sels, coefs = [], [], []
    for s in range(4):
        wv = _refs(sc, s, F64)['warped'].float()
        sel = _selection(sc['g'], s, B, H, W, identity)
        c2 = R.ssim_coefficients(wv.reshape(2 * B, 3, H, W), sc['target']).float().reshape(2, B, 9, H, W)
        coef = torch.where((sel == 2)[:, None], c2[0], torch.where((sel == 3)[:, None], c2[1], torch.full_like(c2[0], NAN)))
        warped.append(wv); sels.append(sel); coefs.append(coef)
    return torch.stack(warped).contiguous(), torch.stack(sels).contiguous(), torch.stack(coefs).contiguous()


def _reference_backward(sc, s, sel, coef, warped, sw, cell, dtype):
    g = R.photo_backward(sel, torch.nan_to_num(coef), warped, sc['target'], sw, dtype)
    dd, dP = R.warp_backward(g, sc['disps'][s], sc['src_m1'], sc['src_p1'], sc['Kinv'], sc['P'], sc['H'], sc['W'], *sc['depths'], cell, dtype)
    return g, dd, dP.transpose(0, 1).reshape(sc['B'], 24)


SAMPLE_W = {2: (0.65, 0.35), 3: (0.5, 0.3, 0.2)}


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,mode,motion', WARP_CASES)
def test_loss_backward(backend, B, H, W, mode, motion, capsys):
    """loss_bwd2_pyramid and the single-scale pair photo_grad + warp_bwd on the same
    constructed inputs: sel by _selection, coef_sel from the float64 reference rounded to fp32 (NaN where nothing may be
    read), warped = the float64 warp rounded to fp32, non-uniform sample weights, the cases of test_warp_fwd (W = 96 / 160,
    20x70 with H % 8 = 4, depth modes 0 / 1 / 2, a band of samples leaving on each side, den < 0).
    Compared: dL / d warped of photo_grad, ddisp_up elementwise and the 24 pose-gradient sums (block partials added in
    float64), each against float64 autograd on the kernels' own cells, 4 x the fp32 restatement.  The kernels do better than
    fp32 autograd here on purpose (double accumulators; d depth / d (u, v) in the analytically cancelled form); the bound
    stays 4 x fp32.  Two launches of loss_bwd2_pyramid write the same bits."""
    dev = use_backend(backend)
    name = f'bwd {H}x{W} m{mode} {motion}'
    sc = _scene(11, B, H, W, mode, motion)
    sw = torch.tensor(SAMPLE_W[B])
    warped, sel, coef_sel = _backward_inputs(sc)
    t = lambda v: v.contiguous().to(dev)
    disps_d = _dev_list(sc['disps'], dev)
    ref_own = [_refs(sc, s, F64) for s in range(4)]
    kcells = _kernel_cells(sc, dev)
    for s in range(4):
        _cells_ok(backend, name + f' s{s}', kcells[s], ref_own[s])
    refs = [(_reference_backward(sc, s, sel[s], coef_sel[s], warped[s], sw, kcells[s], F64),
             _reference_backward(sc, s, sel[s], coef_sel[s], warped[s], sw, kcells[s], F32)) for s in range(4)]
    args = (t(warped), t(sc['target']), t(sc['src_m1']), t(sc['src_p1']), t(sc['Kinv']), t(sc['P']), t(sw))
    # --- loss_bwd2_pyramid (twice)
    nb2 = ops.loss_bwd2_blocks(H, W)
    runs = []
    for _ in range(2):
        dd = torch.full((4, B, H, W), NAN, device=dev)
        dpp = torch.full((4, B, nb2, 24), NAN, dtype=F64, device=dev)
        ops.loss_bwd2_pyramid(disps_d, t(sel), t(coef_sel), *args, dd, dpp, *sc['depths'])
        runs.append((dd.cpu(), dpp.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    coef2 = torch.stack([torch.where((sel == 2 + fi)[:, :, None], coef_sel, torch.full_like(coef_sel, NAN)) for fi in range(2)], 1)
    # --- single scale: photo_grad + warp_bwd
    nbw = ops.warp_bwd_blocks(H, W)
    for s in range(4):
        (g64, dd64, dP64), (g32, dd32, dP32) = refs[s]
        assert float(dd64.abs().max()) > 0 and float(dP64.abs().max()) > 0
        _measured(backend, name + f' s{s}', 'loss_bwd2 ddisp_up', runs[0][0][s], dd64, dd32)
        _measured(backend, name + f' s{s}', 'loss_bwd2 dP sums', runs[0][1][s].sum(1), dP64, dP32)
        dpred = torch.full((2, B, 3, H, W), NAN, device=dev)
        ops.photo_grad(t(sel[s]), t(coef2[s]), t(warped[s]), *args[1:2], t(sw), dpred, B, H, W)
        _measured(backend, name + f' s{s}', 'photo_grad dpred', dpred, g64, g32)
        ddu = torch.full((B, H, W), NAN, device=dev)
        dpw = torch.full((B, nbw, 24), NAN, dtype=F64, device=dev)
        ops.warp_bwd(dpred, disps_d[s], *args[2:6], ddu, dpw, *sc['depths'])
        _measured(backend, name + f' s{s}', 'warp_bwd ddisp_up', ddu, dd64, dd32)
        _measured(backend, name + f' s{s}', 'warp_bwd dP sums', dpw.cpu().sum(1), dP64, dP32)
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W', [(3, 32, 96), (2, 20, 70)])
def test_identity_selection_gives_exact_zero(backend, B, H, W):
    """sel all 0 / 1 (the automask won everywhere): every element of ddisp_up and of the pose-gradient partials is written,
    and is exactly 0, by loss_bwd2_pyramid and by the single-scale pair photo_grad + warp_bwd; coef_sel is NaN throughout (nothing may be read from it)."""
    dev = use_backend(backend)
    sc = _scene(12, B, H, W, 1, 'small')
    sw = torch.tensor(SAMPLE_W[B])
    warped, sel, coef_sel = _backward_inputs(sc, identity=True)
    assert bool(torch.isnan(coef_sel).all()) and int(sel.max()) == 1 and int(sel.min()) == 0
    t = lambda v: v.contiguous().to(dev)
    disps_d = _dev_list(sc['disps'], dev)
    args = (t(warped), t(sc['target']), t(sc['src_m1']), t(sc['src_p1']), t(sc['Kinv']), t(sc['P']), t(sw))
    dd = torch.full((4, B, H, W), NAN, device=dev)
    dpp = torch.full((4, B, ops.loss_bwd2_blocks(H, W), 24), NAN, dtype=F64, device=dev)
    ops.loss_bwd2_pyramid(disps_d, t(sel), t(coef_sel), *args, dd, dpp, *sc['depths'])
    assert float(dd.abs().max()) == 0.0 and float(dpp.abs().max()) == 0.0
    coef2 = torch.full((4, 2, B, 9, H, W), NAN)
    dpred = torch.full((2, B, 3, H, W), NAN, device=dev)
    ops.photo_grad(t(sel[1]), t(coef2[1]), t(warped[1]), t(sc['target']), t(sw), dpred, B, H, W)
    assert float(dpred.abs().max()) == 0.0
    ddu = torch.full((B, H, W), NAN, device=dev)
    dpw = torch.full((B, ops.warp_bwd_blocks(H, W), 24), NAN, dtype=F64, device=dev)
    ops.warp_bwd(dpred, disps_d[1], *args[2:6], ddu, dpw, *sc['depths'])
    assert float(ddu.abs().max()) == 0.0 and float(dpw.abs().max()) == 0.0


# ---- disp_grad ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,smw', [(3, 32, 96, (0.1, 0.6, 0.3)), (2, 24, 160, None), (2, 20, 70, (0.8, 0.2))])
def test_disp_grad(backend, B, H, W, smw, capsys):
    """dz of disp_grad (every scale as a single launch; 20x70 from 10x35, 5x17 and 2x8 is ragged) and of disp_grad_pyramid
    (H, W multiples of 8) against float64 autograd of <ddisp_up, upsample(sigmoid(z))> + the smoothness term; the smoothness
    bookkeeping the kernel consumes is the float64 reference's (loss_reference.finalize, by autograd) rounded to fp32.
    n_smooth = 0 and > 0."""
    dev = use_backend(backend)
    g = _gen(61)
    disps = _disps(g, B, H, W, 0.05, 0.95)
    rgb0 = [torch.rand(B, 3, h, w, generator=g) for h, w in _pyramid_shapes(H, W)]
    ddisp_up = torch.randn(4, B, H, W, generator=g) * 1e-3
    n_smooth = 0 if smw is None else len(smw)
    smt = None if smw is None else torch.tensor(smw)
    aux = None
    if n_smooth:
        chunks = ops.disp_mean_chunks()
        mean_in = [torch.nn.functional.pad(d.double().reshape(B, -1), (0, -(-d[0].numel() // chunks) * chunks - d[0].numel()))
                   .reshape(B, chunks, -1).sum(2) for d in disps]
        zero = torch.zeros(2 * B, 12)
        aux = R.finalize([torch.zeros(B, 1)] * 4, disps, rgb0, mean_in, zero, None, None, torch.ones(B), smt, H, W, n_smooth, 1e-3, 0.0)[1]
        aux = aux.float().contiguous()
    ref = [[R.disp_backward(ddisp_up[s], disps[s], H, W, rgb0[s], smt, 1e-3, s, dt) for dt in (F64, F32)] for s in range(4)]
    disps_d = _dev_list(disps, dev)
    if n_smooth == 0 or n_smooth < (W >> 3) - 1:
        for s in range(4):
            if (H >> s) * (2 ** s) != H or (W >> s) * (2 ** s) != W:
                continue          # disp_grad requires an integer factor (the pyramid's odd scales of 20x70 are warp-only)
            dz = torch.full(disps[s].shape, NAN, device=dev)
            ops.disp_grad(ddisp_up[s].contiguous().to(dev), disps_d[s], None if aux is None else aux[s].contiguous().to(dev), n_smooth, dz, H, W)
            _measured(backend, f'disp_grad {H}x{W} s{s} n{n_smooth}', 'dz', dz, ref[s][0], ref[s][1])
    if H % 8 == 0 and W % 8 == 0:
        dzs = [torch.full(d.shape, NAN, device=dev) for d in disps]
        ops.disp_grad_pyramid(ddisp_up.to(dev), disps_d, None if aux is None else aux.to(dev), n_smooth, dzs, H, W)
        for s in range(4):
            _measured(backend, f'disp_grad_pyramid {H}x{W} s{s} n{n_smooth}', 'dz', dzs[s], ref[s][0], ref[s][1])
    _flush(capsys)


# ---- pose_bwd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('nscale,nblk', [(4, 8), (1, 3), (2, 57), (4, 40)])
@pytest.mark.parametrize('partials', ['random', 'cancelling'])
@pytest.mark.parametrize('vel_scale', [0.05, 0.0])
def test_pose_bwd(backend, nscale, nblk, partials, vel_scale, capsys):
    """dpose[:, :6] against float64 autograd of <sum of the partials, P(pose)> + the weighted velocity term, dpose[:, 6:] == 0.
    The partials are drawn by the test: random doubles, or of the form dP[2] = -(u dP[0] + v dP[1]) with u ~ 600 (what a
    view-synthesis backward produces: K^T dP then cancels to a small fraction of its terms).  nblk below, equal to and not a
    multiple of the kernel's 40 row lanes.  Poses: the angles of _pose_cases() (0, 1e-8, 1e-3, 0.5; four axes), plus t = 0 and
    |t| == relative_distance exactly (both guarded kinks: the gradient of the velocity term is 0 there), |t| on both sides
    of the distance, non-uniform sample weights.  The kernel's chain is all double, the yardstick is fp32 autograd: the
    kernel is far inside the 4 x bound, which is kept as it is."""
    dev = use_backend(backend)
    rows = _pose_cases() + [((0.02, -0.01, 0.03), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.25, 0.0, 0.0))]
    B = len(rows)
    g = _gen(71 + nblk)
    pose = torch.zeros(2 * B, 12)
    for b, (aa, t) in enumerate(rows):
        pose[b, :3] = pose[B + b, :3] = torch.tensor(aa)
        pose[b, 3:6] = torch.tensor(t)
        pose[B + b, 3:6] = -0.5 * torch.tensor(t)
    pose[:, 6:] = 3.0
    K, _ = _camera(B, 192, 640)
    tn = pose[:, 3:6].double().norm(dim=1)
    dist0 = (tn[:B] * torch.where(torch.arange(B) % 2 == 0, 1.3, 0.7)).clone()
    dist1 = -(tn[B:] * torch.where(torch.arange(B) % 2 == 0, 0.6, 1.4)).clone()
    dist0[B - 1] = 0.25                                          # |t| == distance exactly (0.25 and its square are exact)
    dist0[B - 2] = 0.4                                           # t = 0 against a positive distance
    sw = torch.rand(B, generator=g) + 0.1
    sw = (sw / sw.sum()).float()
    dp = torch.randn(nscale, B, nblk, 24, dtype=F64, generator=g)
    if partials == 'cancelling':
        u, v = 600 + 20 * torch.rand(nscale, B, nblk, 1, dtype=F64, generator=g), 90 + 10 * torch.rand(nscale, B, nblk, 1, dtype=F64, generator=g)
        d = dp.reshape(nscale, B, nblk, 2, 3, 4).clone()
        d[..., 2, :] = -(u[..., None] * d[..., 0, :] + v[..., None] * d[..., 1, :])
        dp = d.reshape(nscale, B, nblk, 24).contiguous()
    r64 = R.pose_backward(dp, pose, K, dist0, dist1, sw, vel_scale)
    r32 = R.pose_backward(dp, pose, K, dist0, dist1, sw, vel_scale, F32)
    assert bool((r64[:, 6:] == 0).all())
    dpose = torch.full((2 * B, 12), NAN, device=dev)
    ops.pose_bwd(dp.to(dev), nscale, nblk, pose.to(dev), K.to(dev), dist0.to(dev), dist1.to(dev), sw.to(dev), vel_scale, dpose)
    assert float(dpose[:, 6:].abs().max()) == 0.0
    _measured(backend, f'pose_bwd {nscale}x{nblk} {partials} v{vel_scale}', 'dpose', dpose[:, :6], r64[:, :6], r32[:, :6])
    # per row too, relative to the row's own fp32 error: a mistake confined to one sample or frame shows
    for n in range(2 * B):
        e32 = float((r32[n, :6].double() - r64[n, :6]).abs().max())
        ek = float((dpose[n, :6].cpu().double() - r64[n, :6]).abs().max())
        assert ek <= 4 * e32 + 2 * U * float(r64[n, :6].abs().max()), (n, ek, e32)     # + the final rounding of the output to fp32
    _flush(capsys)


# ---- the opt-in per-sample ("intended") smoothness: smooth_intended_fwd / _finalize / _bwd --------------------------------
# B, H, W, sample_w: non-square with three samples; scale 3 = 3x20; scale 3 = 2x2, the smallest the entry points accept (4 pixels
# in 32 chunks); 320 pixels per chunk at scale 0 (the 256-thread stride loop wraps)
SI_CASES = [
    pytest.param(3, 32, 96, (0.1, 0.6, 0.3), id='32x96-B3'), pytest.param(2, 24, 160, (0.8, 0.2), id='24x160-B2'),
    pytest.param(1, 16, 16, (0.7,), id='16x16-B1'), pytest.param(2, 64, 160, (0.8, 0.2), id='64x160-B2')]
SI_SCALES = (1e-3, 0.1)          # smooth_scale: the shipped weight and the one test_smooth_intended.py uses
GUARD = 7.0


def _guarded(t, dev, guard, fill=NAN):
    """t on `dev` as a view into a buffer that holds `guard` elements of `fill` before and behind it -> (buffer, view)"""
    n = t.numel()
    buf = torch.full((n + 2 * guard,), fill, dtype=t.dtype)
    buf[guard:guard + n] = t.reshape(-1)
    buf = buf.to(dev)
    return buf, buf[guard:guard + n].view(t.shape)


def _guards_intact(buf, guard, fill=GUARD):
    return bool((buf[:guard] == fill).all()) and bool((buf[-guard:] == fill).all())


def _si_inputs(seed, B, H, W):
    """disparities and target images of the four scales.  Every sample holds a block of EXACTLY equal disparities (2 x 3; at
    2 x 2 three of the four pixels), i.e. differences of 0 along x and along y: sgn(0) = 0 of the backward has to meet the
    abs'(0) = 0 of autograd, and the forward adds nothing there."""
    g = _gen(seed)
    disps = _disps(g, B, H, W, 0.05, 0.95)
    rgb0 = [_images(g, B, h, w)[1] for h, w in _pyramid_shapes(H, W)]
    for d in disps:
        h, w = d.shape[-2:]
        for b in range(B):
            if w >= 4:
                d[b, h // 2 - 1:h // 2 + 1, 1:4] = 0.3 + 0.125 * b
            else:
                d[b, 0, :] = d[b, 1, 0] = 0.3 + 0.125 * b
        assert bool((d[:, :, :-1] == d[:, :, 1:]).any(2).any(1).all()) and bool((d[:, :-1] == d[:, 1:]).any(2).any(1).all())
        assert float((d[:, :, :-1] != d[:, :, 1:]).double().mean()) >= 0.5
    return disps, rgb0


def _si_device_inputs(disps, rgb0, dev, W):
    """views whose surroundings are NaN: an edge taken past the first or last pixel of the batch turns the result into NaN
    (an edge taken into the NEXT sample changes the value instead)"""
    return [_guarded(d, dev, W)[1] for d in disps], [_guarded(i, dev, W)[1] for i in rgb0]


def _chunk_sums(t, chunks):
    """(B, ...) -> (B, chunks) float64 sums over ranges of ceil(n / chunks) consecutive elements"""
    B, n = t.shape[0], t[0].numel()
    per = -(-n // chunks)
    return torch.nn.functional.pad(t.double().reshape(B, n), (0, per * chunks - n)).reshape(B, chunks, per).sum(2)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,sw', SI_CASES)
def test_smooth_intended_fwd(backend, B, H, W, sw, capsys):
    """The 4 x B x 32 chunk sums against float64, chunk by chunk, and their float64 sum against T (stated twice in the
    reference: by oracle.functional.smooth_loss_intended and as the sum of the chunks).  Derived bound: a chunk is a sum of
    non-negative terms |d_p - d_q| e nx; a term carries k = 12 roundings (the difference 1; the argument of expf is a sum of
    three |differences| / 3 <= 1: 3 + 2 + 1 roundings of a number <= 1 move e by <= 4 u relative after the exponential,
    expf itself at 2 ulp = 4 u; two products; nx), a thread adds 2 cdiv(per, 256) of them, the block 6 shuffle levels and 2
    adds: (2 cdiv(per, 256) + 8 + 12) u relative.  Chunks past the last pixel (16x16: 28 of 32 at level 3, 16 at level 2)
    are exactly 0, as are chunks of tied pixels only.  `partial` lies between guard elements; it is pre-filled with NaN, so
    every chunk is written.  The fp32 restatement's figure is printed beside the kernel's."""
    dev = use_backend(backend)
    name = f'smooth_intended_fwd {H}x{W}'
    disps, rgb0 = _si_inputs(81, B, H, W)
    chunks = ops.smooth_intended_chunks()
    assert chunks == 32
    refs = [(R.smooth_intended_T(disps[s], rgb0[s], F64, chunks), R.smooth_intended_T(disps[s], rgb0[s], F32, chunks)) for s in range(4)]
    disps_d, rgb0_d = _si_device_inputs(disps, rgb0, dev, W)
    buf, partial = _guarded(torch.full((4, B, chunks), NAN), dev, 64, GUARD)
    ops.smooth_intended_fwd(disps_d, rgb0_d, partial, H, W)
    assert _guards_intact(buf, 64)
    got = partial.cpu().double()
    assert torch.isfinite(got).all()
    for s, (h, w) in enumerate(_pyramid_shapes(H, W)):
        (T64, c64), (T32, c32) = refs[s]
        per = -(-h * w // chunks)
        n = 2 * -(-per // 256) + 8 + 12
        assert float(((c64.sum(1) - T64).abs() / T64).max()) < 1e-13 and bool((T64 > 0).all())
        empty = torch.arange(chunks) * per >= h * w
        assert bool((got[s][:, empty] == 0).all()) and bool((got[s][c64 == 0] == 0).all())
        rel = lambda v, r: float(((v - r).abs() / r.clamp_min(1e-300)).max())
        _row(backend, name + f' s{s}', 'chunks max rel', rel(got[s], c64), rel(c32.double(), c64), f'(bound {n} u = {n * U:.1e}, {int(empty.sum())} empty)')
        _row(backend, name + f' s{s}', 'T max rel', rel(got[s].sum(1), T64), rel(T32.double(), T64))
        assert bool(((got[s] - c64).abs() <= n * U * c64).all()), (s, rel(got[s], c64))
        assert bool(((got[s].sum(1) - T64).abs() <= n * U * T64).all()), s
    if (H, W) == (64, 160):
        assert -(-H * W // chunks) > 256                    # the block's stride loop wraps at level 0
    _flush(capsys)


def _si_finalize_inputs(B, H, W):
    """partial and the disparity chunk sums as INPUTS: the float64 sums rounded to fp32"""
    disps, rgb0 = _si_inputs(82, B, H, W)
    partial = torch.stack([R.smooth_intended_T(disps[s], rgb0[s], F64, ops.smooth_intended_chunks())[1] for s in range(4)]).float()
    means = torch.stack([_chunk_sums(disps[s], ops.disp_mean_chunks()) for s in range(4)]).float()
    return disps, rgb0, partial.contiguous(), means.contiguous()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,sw', SI_CASES)
@pytest.mark.parametrize('prefill', ['arbitrary', 'loss_finalize'])
def test_smooth_intended_finalize(backend, B, H, W, sw, prefill, capsys):
    """aux and the 18 losses at both smooth_scale values, on chunk sums the test rounds from float64.  `losses` holds 18
    positive numbers before ('arbitrary': drawn; 'loss_finalize': what ops.loss_finalize(..., n_smooth=0) wrote on inputs of
    its own -- the engine's sequence).  Entries 4s and 16 keep their bits; 4s + 1 and 4s + 2 are overwritten by sm_s, reg_s;
    4s + 3 grows by reg_s and 17 by sum_s reg_s / 4; losses and aux lie between guard elements.
    Derived bounds (sums of non-negative terms, u per rounding): inv_b = 1 / (sum of dm chunk sums / hw + 1e-7): (dm + 3) u;
    T_b: 32 u; sm_s sums B products inv T w: (dm + 3 + 32 + 2 + B) u = n u; reg_s: + 2 (smooth_scale as fp32, the product;
    2^-s is exact); 4s + 3: the rounding of the sum, u |result|, + the error of reg_s; 17: the four reg_s added (+ 4, / 4
    exact), then as for 4s + 3.  The fp32 restatement's figure is printed beside the kernel's."""
    dev = use_backend(backend)
    disps, rgb0, partial, means = _si_finalize_inputs(B, H, W)
    swt = torch.tensor(sw)
    dm = ops.disp_mean_chunks()
    g = _gen(83)
    for smooth_scale in SI_SCALES:
        if prefill == 'arbitrary':
            before = 0.2 + torch.rand(18, generator=g)
        else:
            nblk = ops.automask_blocks(H, W)
            parts = [(0.03 + 0.05 * torch.rand(B, nblk, generator=g)) * 512 for _ in range(4)]
            pose = torch.randn(2 * B, 12, generator=g) * 0.1
            dist0, dist1 = (0.3 + torch.rand(B, dtype=F64, generator=g) for _ in range(2))
            lf = torch.full((18,), NAN, device=dev)
            ops.loss_finalize(_dev_list(parts, dev), _dev_list(disps, dev), _dev_list(rgb0, dev), _dev_list(list(means), dev), pose.to(dev),
                              dist0.to(dev), dist1.to(dev), swt.to(dev), None, lf, None, B, nblk, H, W, 0, smooth_scale, 0.05)
            before = lf.cpu()
            assert bool((before[[0, 3, 4, 7, 8, 11, 12, 15, 16, 17]] > 0).all()) and bool((before[[1, 2, 5, 6, 9, 10, 13, 14]] == 0).all())
        A64, L64, reg64 = R.smooth_intended_finalize(partial, means, swt, before, H, W, smooth_scale)
        A32, L32, _ = R.smooth_intended_finalize(partial, means, swt, before, H, W, smooth_scale, F32)
        lbuf, losses = _guarded(before, dev, 8, GUARD)
        abuf, aux = _guarded(torch.full((4, B, 2), NAN), dev, 8, GUARD)
        ops.smooth_intended_finalize(partial.to(dev), means.to(dev), swt.to(dev), losses, aux, B, H, W, smooth_scale)
        assert _guards_intact(lbuf, 8) and _guards_intact(abuf, 8)
        got, ga = losses.cpu(), aux.cpu().double()
        keep = [0, 4, 8, 12, 16]
        assert torch.equal(got[keep], before[keep])
        got = got.double()
        n = dm + 37 + B
        tol_a = torch.stack([(dm + 3) * U * A64[..., 0], 32 * U * A64[..., 1]], -1)
        tol = torch.zeros(18, dtype=F64)
        for s in range(4):
            tol[4 * s + 1], tol[4 * s + 2] = n * U * L64[4 * s + 1], (n + 2) * U * L64[4 * s + 2]
            tol[4 * s + 3] = U * L64[4 * s + 3] + (n + 2) * U * reg64[s]
        tol[17] = U * L64[17] + (n + 6) * U * reg64.sum() / 4
        assert bool((reg64 > 0).all()) and bool((L64[[3, 7, 11, 15, 17]] > before.double()[[3, 7, 11, 15, 17]]).all())
        rel = lambda v, r: float(((v - r).abs() / r.abs().clamp_min(1e-300)).max())
        name = f'smooth_intended_finalize {H}x{W} {prefill} {smooth_scale:g}'
        _row(backend, name, 'aux max rel', rel(ga, A64), rel(A32.double(), A64), f'(bound {dm + 3} u = {(dm + 3) * U:.1e})')
        _row(backend, name, 'losses max rel', rel(got, L64), rel(L32.double(), L64), f'(bound {n + 2} u = {(n + 2) * U:.1e})')
        assert bool(((ga - A64).abs() <= tol_a).all()), ((ga - A64).abs() / tol_a).max()
        assert bool(((got - L64).abs() <= tol).all()), ((got - L64).abs() / tol.clamp_min(1e-300)).tolist()
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('B,H,W,sw', SI_CASES)
def test_smooth_intended_bwd(backend, B, H, W, sw, capsys):
    """dz of smooth_intended_bwd at both smooth_scale values against float64 autograd of the weighted, mean-normalised
    smoothness of the four scales through disp = sigmoid(z): measured class, 4 x the fp32 restatement per scale (largest
    absolute error and relative L2), every pixel included -- the sign of an fp32 difference is the sign of the exact one, and
    on the tied block both sides give 0.  aux = (1 / (mean + 1e-7), T) is the float64 reference's, rounded to fp32.
    The kernel ADDS: on a dz that holds numbers of the gradient's own size it writes fl32(what was there + what it writes
    on zeros), bit for bit.  The four dz are views between guard elements (the launch has cdiv(H W, 256) blocks for every
    scale: at scale 3 all but one are past the last pixel)."""
    dev = use_backend(backend)
    disps, rgb0 = _si_inputs(84, B, H, W)
    swt = torch.tensor(sw)
    disps_d, rgb0_d = _si_device_inputs(disps, rgb0, dev, W)
    aux = torch.stack([torch.stack([1 / (disps[s].double().mean((1, 2)) + 1e-7), R.smooth_intended_T(disps[s], rgb0[s])[0]], 1)
                       for s in range(4)]).float().contiguous()
    g = _gen(85)
    for smooth_scale in SI_SCALES:
        r64 = R.smooth_intended_backward(disps, rgb0, swt, smooth_scale)
        r32 = R.smooth_intended_backward(disps, rgb0, swt, smooth_scale, F32)
        runs = []
        for fill in (False, True):
            pre = [torch.randn(d.shape, generator=g) * float(r64[s].abs().max()) if fill else torch.zeros(d.shape) for s, d in enumerate(disps)]
            bufs, dzs = zip(*[_guarded(p, dev, 256, GUARD) for p in pre])
            ops.smooth_intended_bwd(disps_d, rgb0_d, aux.to(dev), swt.to(dev), list(dzs), H, W, smooth_scale)
            assert all(_guards_intact(b, 256) for b in bufs)
            runs.append((pre, [d.cpu() for d in dzs]))
        for s in range(4):
            name = f'smooth_intended_bwd {H}x{W} s{s} {smooth_scale:g}'
            tied = (disps[s][:, :, :-1] == disps[s][:, :, 1:])
            assert float(r64[s].abs().max()) > 0 and bool(tied.any())
            _measured(backend, name, 'dz', runs[0][1][s], r64[s], r32[s])
            assert torch.equal(runs[1][1][s], runs[1][0][s] + runs[0][1][s]), (s, 'dz is not what was there + the gradient')
            assert not torch.equal(runs[1][1][s], runs[0][1][s])
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
def test_smooth_intended_geometry(backend):
    """H = 8 or W = 8 (a scale-3 map of one row or one column: no edge along y / x, ny or nx = 1 / 0) is rejected by the
    forward AND by the backward, before anything is written; B = 0 returns without touching anything."""
    dev = use_backend(backend)
    chunks = ops.smooth_intended_chunks()
    one = torch.ones(1, device=dev)
    for B, H, W in ((2, 8, 32), (2, 32, 8), (0, 32, 96)):
        disps = [torch.rand(max(B, 1), h, w)[:B].contiguous().to(dev) for h, w in _pyramid_shapes(H, W)]
        rgb0 = [torch.rand(max(B, 1), 3, h, w)[:B].contiguous().to(dev) for h, w in _pyramid_shapes(H, W)]
        partial = torch.full((4, max(B, 1), chunks), GUARD, device=dev)
        aux = torch.full((4, max(B, 1), 2), 0.5, device=dev)
        dzs = [torch.full((max(B, 1), h, w), GUARD, device=dev) for h, w in _pyramid_shapes(H, W)]
        losses = torch.full((18,), GUARD, device=dev)
        if B:
            with pytest.raises(ClslamError):
                ops.smooth_intended_fwd(disps, rgb0, partial, H, W)
            with pytest.raises(ClslamError):
                ops.smooth_intended_bwd(disps, rgb0, aux, one, dzs, H, W, 0.1)
        else:
            ops.smooth_intended_fwd(disps, rgb0, partial, H, W)
            ops.smooth_intended_finalize(partial, partial, one, losses, aux, B, H, W, 0.1)
            ops.smooth_intended_bwd(disps, rgb0, aux, one, dzs, H, W, 0.1)
        assert bool((partial == GUARD).all()) and bool((losses == GUARD).all()) and bool((aux == 0.5).all())
        assert all(bool((d == GUARD).all()) for d in dzs)
