"""Thin tensor-level wrappers over the C ABI (pointer / shape plumbing only; no math here)."""
import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import ACT_ELU, ACT_HSIGMOID, ACT_HSWISH, ACT_NONE, ACT_RELU, PAD_REFLECT, PAD_ZERO  # noqa: F401


# profile_begin() sets this to a list collecting (kind, tile config, algorithmic flops, description) per conv launch
PROFILE = None


def profile_begin(max_launches: int = 8192) -> None:
    """Measurement (bench.py's roofline leg): every conv2d() launch from now on is timestamped by the library itself
    (clslam_conv_profile_begin: kernel start/stop, the duration rocprofv3 reports).  Run the launches in serial order
    (engine.use_side_stream = False): concurrent kernels share the GPU and a launch's duration says little then."""
    global PROFILE
    _lib.get_lib().call('clslam_conv_profile_begin', max_launches)
    PROFILE = []


def profile_end():
    """-> [(kind, config, flops, seconds, description, algorithmic_bytes)] in launch order; disarms."""
    global PROFILE
    meta, PROFILE = PROFILE, None
    cap = max(1, len(meta))
    ms = (C.c_float * cap)()
    count = C.c_int(0)
    _lib.get_lib().call('clslam_conv_profile_end', C.cast(ms, C.c_void_p), cap, C.cast(C.pointer(count), C.c_void_p))
    if not _lib.get_lib().is_device:      # the emulator build has no timestamps
        return [(k, cfg, fl, 0.0, desc, nb) for k, cfg, fl, desc, nb in meta]
    if count.value != len(meta):
        raise _lib.ClslamError(f'profile_end: {count.value} timed launches for {len(meta)} conv2d calls')
    return [(k, cfg, fl, ms[i] * 1e-3, desc, nb) for i, (k, cfg, fl, desc, nb) in enumerate(meta)]


# These two helpers run ~1000 times per step; at B <= 2 the step is host-bound, so they avoid every avoidable
# Python-level call (torch.cuda.current_stream() builds a Stream object: ~2 us each, 200 times per step).
_raw_stream = torch._C._cuda_getCurrentRawStream if hasattr(torch._C, '_cuda_getCurrentRawStream') else None


_FORCED_STREAM: Optional[int] = None


class launch_on:
    """`with launch_on(stream):` -- every launch of this module inside the block goes to `stream` (a torch.cuda.Stream).
    Unlike `torch.cuda.stream()` (6 us per block, ~25 blocks per step: the B = 1 step is bound by the host) it does not touch
    torch's current stream: only for blocks that contain nothing but launches of this module."""
    __slots__ = ('handle', 'prev')

    def __init__(self, stream):
        self.handle = None if stream is None else stream.cuda_stream

    def __enter__(self):
        global _FORCED_STREAM
        self.prev = _FORCED_STREAM
        if self.handle is not None:
            _FORCED_STREAM = self.handle
        return self

    def __exit__(self, *exc):
        global _FORCED_STREAM
        _FORCED_STREAM = self.prev
        return False


def _stream(t: torch.Tensor) -> int:
    """raw hipStream_t the launch goes to: the launch_on() stream if one is set, else torch's current stream on t's device
    (0 = the emulator's only stream)"""
    if _FORCED_STREAM is not None:
        return _FORCED_STREAM
    if t.is_cuda:
        if _raw_stream is not None:
            return _raw_stream(t.device.index)
        return torch.cuda.current_stream(t.device).cuda_stream
    return 0


_QUERY_CACHE: dict = {}


def _query(name: str, *args) -> int:
    """Launch-geometry queries of the library (pure functions of integer arguments): asked once, then remembered -- a bare
    ctypes call costs ~10 us and fold_blocks() alone was asked ten times per step."""
    lib = _lib._LIB or _lib.get_lib()
    key = (id(lib), name, args)
    v = _QUERY_CACHE.get(key)
    if v is None:
        v = _QUERY_CACHE[key] = getattr(lib.cdll, name)(*args)
    return v


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    lib = _lib._LIB or _lib.get_lib()
    if t.is_cuda != lib.is_device or t.dtype is not torch.float32 or not t.is_contiguous():
        if t.device.type != lib.device_type:
            raise _lib.ClslamError(f'tensor on {t.device}, library {lib.path.name} runs on {lib.device_type}')
        raise _lib.ClslamError(f'expected contiguous fp32, got {t.dtype} contiguous={t.is_contiguous()}')
    return t.data_ptr()


def _pa(t: Optional[torch.Tensor], dtype):
    """pointer of a contiguous tensor of another dtype (uint8 selection maps, float64 distances)"""
    if t is None:
        return None
    lib = _lib.get_lib()
    if t.device.type != lib.device_type or t.dtype != dtype or not t.is_contiguous():
        raise _lib.ClslamError(f'expected contiguous {dtype} on {lib.device_type}, got {t.dtype} on {t.device}')
    return t.data_ptr()


class Handoff:
    """Releases a consumer stream behind ONE launch of a producer stream without a marker packet on the producer
    (clslam_handoff_*, include/clslam_hip.h): `arm()` right before the producing conv2d() / fold_act_grad() call, `release(producer,
    consumer)` after it.  A pool of events, re-used round-robin (an event may be re-armed once it has been waited on; the pool is
    much larger than the hand-offs in flight).  On the emulator (one stream) both calls are no-ops."""
    POOL = 64

    def __init__(self) -> None:
        self.lib = _lib.get_lib()
        self.events = []
        self.next = 0
        self.armed = None

    def arm(self) -> None:
        if not self.lib.is_device:
            return
        if len(self.events) < self.POOL:
            ev = self.lib.cdll.clslam_handoff_event_create()
            if not ev:
                raise _lib.ClslamError('clslam_handoff_event_create failed: ' + self.lib.cdll.clslam_last_error().decode())
            self.events.append(ev)
            self.armed = ev
        else:
            self.armed = self.events[self.next % self.POOL]
        self.next += 1
        self.lib.call('clslam_handoff_arm', self.armed)

    def release(self, producer, consumer) -> None:
        """`consumer` (torch.cuda.Stream) waits for the armed launch -- or, had none taken the event, for everything enqueued on
        `producer` so far"""
        ev, self.armed = self.armed, None
        if ev is None:
            return
        self.lib.call('clslam_handoff_wait', ev, producer.cuda_stream, consumer.cuda_stream)

    def __del__(self):
        try:
            for ev in self.events:
                self.lib.cdll.clslam_handoff_event_destroy(ev)
        except Exception:
            pass


# split-K scratch per stream (stream handle -> zero-initialised uint8 tensor), see clslam_conv_desc.workspace
_CONV_WORKSPACES = {}


def set_conv_workspace(stream_handle: int, workspace: Optional[torch.Tensor]) -> None:
    """Register the split-K scratch conv2d() uses for launches on `stream_handle` (None: drop it).  The
    tensor must be zero-filled once and used by that stream only."""
    if workspace is None:
        _CONV_WORKSPACES.pop(stream_handle, None)
    else:
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous()
        _CONV_WORKSPACES[stream_handle] = workspace


# clslam_conv_desc.cu_limit of the conv launches that follow (0 = the whole chip): set by the engine per step, see there
PERSISTENT_CU_LIMIT = 0


# Descriptors of the engine's fixed call sites (conv2d(..., key=...)): the same layer on the same workspace buffers every step.
# Building the 28-field ctypes structure costs 2.2 of the 5.8 us a conv2d() call takes on the MI355X box's host; a single-triplet
# step (75 convolutions, host-bound) pays that 75 times.  An entry is re-used only while the three tensors that can change under
# a call site (source, weight, output) still sit where they sat; everything else of a site is fixed by construction.
_CONV_DESC_CACHE: dict = {}


def _conv_input_geometry(src_a, src_b, ksize, pad, upsample_a):
    """(Hi, Wi, Ca, Cb, pad) of a conv descriptor: the input size after the optional nearest-2x upsampling of source a, the
    channels of the two sources, and the padding (default: "same", ksize // 2)"""
    Ha, Wa, Ca = src_a.shape[1:]
    Hi, Wi = (Ha * 2, Wa * 2) if upsample_a else (Ha, Wa)
    Cb = 0 if src_b is None else src_b.shape[3]
    return Hi, Wi, Ca, Cb, ksize // 2 if pad is None else pad


def conv2d(src_a, weight, out, *, src_b=None, scale=None, shift=None, residual=None, ksize=3, stride=1,
           pad=None, pad_mode=PAD_ZERO, upsample_a=False, act=ACT_NONE, config=-1, actgrad_src=None,
           actgrad_kind=ACT_NONE, workspace=None, weight_wino=None, cu_limit=None, key=None, cache=None):
    """src_a (B,Ha,Wa,Ca) NHWC; weight (Cout, k*k, Ca+Cb); out (B,Ho,Wo,Cout); weight_wino: wino_weight_transform(weight).
    key (hashable, optional): identifies a FIXED call site -- same layer, same buffers, same keyword arguments every time;
    its descriptor is kept and only stream-dependent fields (split-K scratch, cu_limit) are refreshed.
    cache: the dict the descriptor lives in.  The engine passes its OWN (Engine._desc_cache): the entries then die with the
    buffers they point into -- a module-global cache keyed by id() could hand a later engine, whose workspace happens to be
    allocated at the same addresses, a descriptor with another geometry; the global one serves tests and tools."""
    if cache is None:
        cache = _CONV_DESC_CACHE
    if key is not None and PROFILE is None:
        ent = cache.get(key)
        if ent is not None:
            d, ref, lib = ent
            if d.src_a == src_a.data_ptr() and d.out == out.data_ptr() and d.weight == weight.data_ptr():
                stream = _stream(out)
                ws = workspace if workspace is not None else (_CONV_WORKSPACES.get(stream) if _CONV_WORKSPACES else None)
                if ws is None:
                    d.workspace, d.workspace_bytes = None, 0
                else:
                    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
                d.cu_limit = PERSISTENT_CU_LIMIT if cu_limit is None else cu_limit
                rc = lib.cdll.clslam_conv2d(ref, stream)
                if rc != _lib.OK:
                    raise _lib.ClslamError(f'clslam_conv2d failed ({rc}): {lib.cdll.clslam_last_error().decode()}')
                return out
    B, Ho, Wo, Cout = out.shape
    Hi, Wi, Ca, Cb, pad = _conv_input_geometry(src_a, src_b, ksize, pad, upsample_a)
    assert weight.shape[0] == Cout and weight.numel() == Cout * ksize * ksize * (Ca + Cb), weight.shape
    stream = _stream(out)
    if workspace is None and _CONV_WORKSPACES:
        workspace = _CONV_WORKSPACES.get(stream)
    d = _lib.ConvDesc(_p(src_a), _p(src_b), _p(weight), _p(scale), _p(shift), _p(residual), _p(out),
                      B, Hi, Wi, Ca, Cb, Ho, Wo, Cout, ksize, stride, pad, pad_mode, int(upsample_a), act, config,
                      _p(actgrad_src), actgrad_kind, None if workspace is None else workspace.data_ptr(),
                      0 if workspace is None else workspace.numel(), _p(weight_wino),
                      PERSISTENT_CU_LIMIT if cu_limit is None else cu_limit)
    if PROFILE is not None:     # armed by profile_begin(): the library timestamps the launch itself
        cfg = config if config >= 0 else _lib.get_lib().cdll.clslam_conv2d_pick_config(C.byref(d))
        # algorithmic bytes: every operand once (source a as stored, i.e. before the nearest-2x upsampling)
        nbytes = 4.0 * (src_a.numel() + (0 if src_b is None else src_b.numel()) + weight.numel() + out.numel() +
                        (0 if residual is None else residual.numel()) + (0 if actgrad_src is None else actgrad_src.numel()))
        PROFILE.append(('conv', cfg, 2.0 * B * Ho * Wo * Cout * ksize * ksize * (Ca + Cb),
                        f'B{B} {Hi}x{Wi} {Ca}+{Cb}->{Cout} k{ksize} s{stride} pad{pad}', nbytes))
    lib = _lib.get_lib()
    lib.call('clslam_conv2d', C.byref(d), stream)
    if key is not None and PROFILE is None:
        cache[key] = (d, C.byref(d), lib)
    return out


def conv_desc(src_a, out_shape, *, src_b=None, ksize=3, stride=1, pad=None, pad_mode=PAD_ZERO, upsample_a=False):
    """Geometry-only descriptor of a forward conv (used by wgrad)."""
    B, Ho, Wo, Cout = out_shape
    Hi, Wi, Ca, Cb, pad = _conv_input_geometry(src_a, src_b, ksize, pad, upsample_a)
    return _lib.ConvDesc(_p(src_a), _p(src_b), None, None, None, None, None, B, Hi, Wi, Ca, Cb, Ho, Wo, Cout,
                         ksize, stride, pad, pad_mode, int(upsample_a), ACT_NONE, -1, None, ACT_NONE, None, 0, None, 0)


def wino_weight_transform(w, out=None):
    """w (Cout, 9, Cin) -> the Winograd F(2x2,3x3) filter image clslam_conv2d takes as `weight_wino` (conv_wino.hip)."""
    Cout, taps, Cin = w.shape
    assert taps == 9
    n = _lib.get_lib().cdll.clslam_wino_weight_size(Cout, Cin)
    if out is None:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    assert out.numel() >= n
    _lib.get_lib().call('clslam_wino_weight_transform', _p(w), _p(out), Cout, Cin, _stream(w))
    return out


def weight_transpose(w, wt, ch_in_sel=None):
    """w (Cout,taps,Cin) -> wt (Cin_sel,taps,Cout), taps flipped."""
    Cout, taps, Cin = w.shape
    sel = Cin if ch_in_sel is None else ch_in_sel
    assert wt.numel() >= sel * taps * Cout
    _lib.get_lib().call('clslam_weight_transpose', _p(w), _p(wt), Cout, taps, Cin, sel, _stream(w))
    return wt


def transpose_table(items):
    """items: [(w (Cout,taps,Cin), wt, ch_in_sel | None)] -> a host table for weight_transpose_multi (build once: the
    arena views and the wt buffers of an engine never move)"""
    tab = (_lib.TransposeItem * len(items))()
    for rec, (w, wt, sel) in zip(tab, items):
        Cout, taps, Cin = w.shape
        sel = Cin if sel is None else sel
        assert wt.numel() >= sel * taps * Cout
        rec.w, rec.wt, rec.ch_out, rec.taps, rec.ch_in, rec.ch_in_sel = _p(w), _p(wt), Cout, taps, Cin, sel
    return tab


def weight_transpose_multi(table, stream_ref):
    """every weight tensor of `table` flipped / transposed for its dgrad convolution, in one launch"""
    _lib.get_lib().call('clslam_weight_transpose_multi', table, len(table), _stream(stream_ref))


def fold_blocks(batch, h, w, ch, pool) -> int:
    return _query('clslam_fold_blocks', batch, h, w, ch, int(pool))


def fold_act_grad(dxp, yout, dz, *, h, w, ch, border, pool, act, bias_partial=None, disp_dz=None, disp_w=None):
    """disp_dz (B,h,w) + disp_w (9,ch): also add the dispconv head's data gradient (dxp may be None then)."""
    B = dz.shape[0]
    _lib.get_lib().call('clslam_fold_act_grad', _p(dxp), _p(yout), _p(dz), _p(bias_partial), B, h, w, ch,
                        ch if dxp is None else dxp.shape[3], border, int(pool), act, _p(disp_dz), _p(disp_w), _stream(dz))
    return dz


def wgrad_splits(desc, target_blocks=1024) -> int:
    return _lib.get_lib().cdll.clslam_wgrad_splits(C.byref(desc), target_blocks)


def conv_wgrad(desc, dz, partial, splits):
    _lib.get_lib().call('clslam_conv_wgrad', C.byref(desc), _p(dz), _p(partial), splits, _stream(dz))
    return partial


def wgrad_patch_supported(desc) -> bool:
    return bool(_lib.get_lib().cdll.clslam_wgrad_patch_supported(C.byref(desc)))


def wgrad_patch_splits(desc, target_blocks=1024) -> int:
    return _lib.get_lib().cdll.clslam_wgrad_patch_splits(C.byref(desc), target_blocks)


def conv_wgrad_patch(desc, dz, partial, splits):
    _lib.get_lib().call('clslam_conv_wgrad_patch', C.byref(desc), _p(dz), _p(partial), splits, _stream(dz))
    return partial


def reduce_partials(partial, out, n, splits, scale=1.0):
    _lib.get_lib().call('clslam_reduce_partials', _p(partial), _p(out), n, splits, scale, _stream(out))
    return out


def make_reduce_table(items, device):
    """items: list of (partial tensor, out tensor, n, splits) -> device byte tensor for reduce_multi"""
    import numpy as np
    rec = np.zeros(len(items), dtype=np.dtype([('partial', '<u8'), ('out', '<u8'), ('n', '<u8'), ('splits', '<i4'), ('scale', '<f4')]))
    for i, (part, out, n, splits) in enumerate(items):
        rec[i] = (_p(part), _p(out), n, splits, 1.0)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device)


def reduce_multi(table, nitems, stream_ref, blocks_per_item=384):
    _lib.get_lib().call('clslam_reduce_multi', table.data_ptr(), nitems, blocks_per_item, _stream(stream_ref))


def colsum_blocks(rows: int) -> int:
    return _query('clslam_colsum_blocks', rows)


def colsum(x, partial, rows, ch):
    _lib.get_lib().call('clslam_colsum', _p(x), _p(partial), rows, ch, _stream(x))
    return partial


def stem_pack_weight(weight):
    """OIHW (64,3|6,7,7) conv1 weight -> packed LDS-image slabs for stem_conv"""
    n_img = weight.shape[1] // 3
    packed = torch.empty(_lib.get_lib().cdll.clslam_stem_packed_size(n_img), device=weight.device)
    _lib.get_lib().call('clslam_stem_pack_weight', _p(weight), _p(packed), n_img, _stream(weight))
    return packed


def stem_conv(img_a, img_b, weight, scale, shift, out):
    """img_* planar (B,3,H,W); weight = stem_pack_weight(conv1.weight); out NHWC (B,H/2,W/2,64)."""
    B, _, H, W = img_a.shape
    n_img = 1 if img_b is None else 2
    _lib.get_lib().call('clslam_stem_conv', _p(img_a), _p(img_b), _p(weight), _p(scale), _p(shift), _p(out),
                        B, H, W, n_img, _stream(out))
    return out


def maxpool3x3s2(x, out):
    B, H, W, Cc = x.shape
    _lib.get_lib().call('clslam_maxpool3x3s2', _p(x), _p(out), B, H, W, Cc, _stream(out))
    return out


def dispconv_fwd(x, w, bias, disp):
    B, H, W, Cc = x.shape
    _lib.get_lib().call('clslam_dispconv_fwd', _p(x), _p(w), _p(bias), _p(disp), B, H, W, Cc, _stream(disp))
    return disp


def dispconv_bwd_data(dz, w, dxp, ch, accumulate):
    B, H, W = dz.shape[0], dz.shape[-2], dz.shape[-1]
    _lib.get_lib().call('clslam_dispconv_bwd_data', _p(dz), _p(w), _p(dxp), B, H, W, ch, int(accumulate), _stream(dxp))
    return dxp


def dispconv_wgrad_blocks(pixels: int) -> int:
    return _query('clslam_dispconv_wgrad_blocks', pixels)


def dispconv_wgrad(dz, x, partial):
    B, H, W, Cc = x.shape
    _lib.get_lib().call('clslam_dispconv_wgrad', _p(dz), _p(x), _p(partial), B, H, W, Cc, _stream(x))
    return partial


def pose_head_fwd(x, w2, b2, mean, pose):
    N, H, W, _ = x.shape
    _lib.get_lib().call('clslam_pose_head_fwd', _p(x), _p(w2), _p(b2), _p(mean), _p(pose), N, H * W, _stream(x))
    return pose


def pose_head_bwd(dpose, x, w2, mean, dz1, dw2, db2, grad_scale=1.0):
    N, H, W, _ = x.shape
    _lib.get_lib().call('clslam_pose_head_bwd', _p(dpose), _p(x), _p(w2), _p(mean), _p(dz1), _p(dw2), _p(db2),
                        N, H * W, grad_scale, _stream(x))


def _nd(v):
    return -1.0 if v is None else float(v)


def pose_to_proj(pose, kmat, cam_t_cam, proj):
    B = kmat.shape[0]
    _lib.get_lib().call('clslam_pose_to_proj', _p(pose), _p(kmat), _p(cam_t_cam), _p(proj), B, _stream(pose))


def warp_fwd(disp_s, src_m1, src_p1, inv_k, proj, depth, warped, min_depth, max_depth):
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    h, w = disp_s.shape[-2:]
    _lib.get_lib().call('clslam_warp_fwd', _p(disp_s), h, w, _p(src_m1), _p(src_p1), _p(inv_k), _p(proj), _p(depth),
                        _p(warped), B, H, W, _nd(min_depth), _nd(max_depth), _stream(depth))


def warp_bwd_blocks(H, W) -> int:
    return _query('clslam_warp_bwd_blocks', H, W)


def warp_bwd(dpred, disp_s, src_m1, src_p1, inv_k, proj, ddisp_up, dp_partial, min_depth, max_depth):
    B, H, W = ddisp_up.shape[0], ddisp_up.shape[-2], ddisp_up.shape[-1]
    h, w = disp_s.shape[-2:]
    _lib.get_lib().call('clslam_warp_bwd', _p(dpred), _p(disp_s), h, w, _p(src_m1), _p(src_p1), _p(inv_k), _p(proj),
                        _p(ddisp_up), _pa(dp_partial, torch.float64), B, H, W, _nd(min_depth), _nd(max_depth), _stream(dpred))


def pose_bwd(dp_partial, nscale, nblk, pose, kmat, dist0, dist1, sample_w, vel_scale, dpose):
    B = kmat.shape[0]
    _lib.get_lib().call('clslam_pose_bwd', _pa(dp_partial, torch.float64), nscale, nblk, _p(pose), _p(kmat), _pa(dist0, torch.float64),
                        _pa(dist1, torch.float64), _p(sample_w), float(vel_scale or 0.0), _p(dpose), B, _stream(pose))


def photo_map(pred, target, out_map, coef, npred, batch, H, W):
    _lib.get_lib().call('clslam_photo_map', _p(pred), _p(target), _p(out_map), _p(coef), npred, batch, H, W,
                        _stream(out_map))


def automask_blocks(H, W) -> int:
    return _query('clslam_automask_blocks', H, W)


def automask(idmap, noise, rpmap, sel, partial, batch, H, W):
    _lib.get_lib().call('clslam_automask', _p(idmap), _p(noise), _p(rpmap), _pa(sel, torch.uint8), _p(partial), batch,
                        H, W, _stream(idmap))


def disp_mean_chunks() -> int:
    return _query('clslam_disp_mean_chunks')


def disp_mean(disp, means):
    B = disp.shape[0]
    _lib.get_lib().call('clslam_disp_mean', _p(disp), _p(means), B, disp.numel() // B, _stream(disp))


def loss_finalize(partials, disps, rgb0s, means, pose, dist0, dist1, sample_w, smooth_w, losses, smooth_aux, batch,
                  nblk, H, W, n_smooth, smooth_scale, vel_scale):
    d = _lib.LossDesc()
    for s in range(4):
        d.partial[s] = _p(partials[s]); d.disp[s] = _p(disps[s]); d.rgb0[s] = _p(rgb0s[s]); d.means[s] = _p(means[s])
    d.pose = _p(pose)
    d.dist0 = _pa(dist0, torch.float64); d.dist1 = _pa(dist1, torch.float64)
    d.sample_w = _p(sample_w); d.smooth_w = _p(smooth_w); d.losses = _p(losses); d.smooth_aux = _p(smooth_aux)
    d.batch, d.nblk, d.H, d.W, d.n_smooth = batch, nblk, H, W, n_smooth
    d.smooth_scale, d.vel_scale = float(smooth_scale), float(vel_scale or 0.0)
    _lib.get_lib().call('clslam_loss_finalize', C.byref(d), _stream(losses))


def photo_grad(sel, coef, pred, target, sample_w, dpred, batch, H, W):
    _lib.get_lib().call('clslam_photo_grad', _pa(sel, torch.uint8), _p(coef), _p(pred), _p(target), _p(sample_w),
                        _p(dpred), batch, H, W, _stream(dpred))


def disp_grad(ddisp_up, disp, smooth_aux, n_smooth, dz, H, W):
    B, h, w = disp.shape[0], disp.shape[-2], disp.shape[-1]
    _lib.get_lib().call('clslam_disp_grad', _p(ddisp_up), _p(disp), _p(smooth_aux), n_smooth, _p(dz), B, h, w, H, W,
                        _stream(dz))


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, guard=None):
    """guard: optional 1-element fp32 tensor (the step's loss); NaN there turns the launch into a no-op."""
    _lib.get_lib().call('clslam_adam_step', _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, beta1,
                        beta2, eps, step, grad_scale, _p(guard), _stream(param))


# ---- loop-closure encoder (MobileNetV3-small) ops ------------------------------------------------
def mbv3_stem(img, weight, scale, shift, out):
    B, _, H, W = img.shape
    _lib.get_lib().call('clslam_mbv3_stem', _p(img), _p(weight), _p(scale), _p(shift), _p(out), B, H, W, _stream(out))
    return out


def dwconv(x, weight, scale, shift, out, ksize, stride, act):
    B, H, W, Cc = x.shape
    _lib.get_lib().call('clslam_dwconv', _p(x), _p(weight), _p(scale), _p(shift), _p(out), B, H, W, Cc, ksize, stride, act,
                        _stream(out))
    return out


def avgpool_chunks(hw: int) -> int:
    return _query('clslam_avgpool_chunks', hw)


def global_avgpool(x, out, partial=None):
    """partial: optional (B * avgpool_chunks(HW) * C) scratch -> two-stage reduction over pixel chunks."""
    B, Cc = x.shape[0], x.shape[-1]
    hw = 1
    for n in x.shape[1:-1]:
        hw *= n
    _lib.get_lib().call('clslam_global_avgpool', _p(x), _p(out), _p(partial), B, hw, Cc, _stream(out))
    return out


def se_gate(pool, w1, b1, w2, b2, gate):
    B, Cc = pool.shape
    _lib.get_lib().call('clslam_se_gate', _p(pool), _p(w1), _p(b1), _p(w2), _p(b2), _p(gate), B, Cc, w1.shape[0],
                        _stream(gate))
    return gate


def channel_scale(x, gate):
    B, Cc = x.shape[0], x.shape[-1]
    _lib.get_lib().call('clslam_channel_scale', _p(x), _p(gate), B, x.numel() // (B * Cc), Cc, _stream(x))
    return x


# ---- pyramid forms: one launch for the four scales -----------------------------------------------------
def _ptr4(tensors):
    return (C.c_void_p * 4)(*[_p(t) for t in tensors])


def warp_fwd_pyramid(disps, src_m1, src_p1, inv_k, proj, depth, warped, min_depth, max_depth):
    B, H, W = depth.shape[1], depth.shape[-2], depth.shape[-1]
    _lib.get_lib().call('clslam_warp_fwd_pyramid', _ptr4(disps), _p(src_m1), _p(src_p1), _p(inv_k), _p(proj), _p(depth),
                        _p(warped), B, H, W, _nd(min_depth), _nd(max_depth), _stream(depth))


def warp_cells_pyramid(disps, inv_k, proj, cells, min_depth, max_depth):
    """diagnostic: cells (4,2,B,H,W) int32 = x0 | y0 << 12 | (x not clipped) << 24 | (y not clipped) << 25"""
    B, H, W = cells.shape[2], cells.shape[-2], cells.shape[-1]
    _lib.get_lib().call('clslam_warp_cells_pyramid', _ptr4(disps), _p(inv_k), _p(proj), _pa(cells, torch.int32), B, H, W,
                        _nd(min_depth), _nd(max_depth), _stream(cells))
    return cells


def warp_coords_pyramid(disps, inv_k, proj, coords, min_depth, max_depth):
    """diagnostic: coords (4,2,B,H,W,2) float32 = the clipped sampling position (ix, iy) in pixels"""
    B, H, W = coords.shape[2], coords.shape[3], coords.shape[4]
    _lib.get_lib().call('clslam_warp_coords_pyramid', _ptr4(disps), _p(inv_k), _p(proj), _p(coords), B, H, W,
                        _nd(min_depth), _nd(max_depth), _stream(coords))
    return coords


def automask_pyramid(idmap, noise, rpmap, sel, partial, batch, H, W):
    _lib.get_lib().call('clslam_automask_pyramid', _p(idmap), _p(noise), _p(rpmap), _pa(sel, torch.uint8), _p(partial), 4,
                        batch, H, W, _stream(idmap))


def disp_mean_pyramid(disps, means, H, W):
    _lib.get_lib().call('clslam_disp_mean_pyramid', _ptr4(disps), _p(means), disps[0].shape[0], H, W, _stream(means))


def disp_grad_pyramid(ddisp_up, disps, smooth_aux, n_smooth, dzs, H, W):
    _lib.get_lib().call('clslam_disp_grad_pyramid', _p(ddisp_up), _ptr4(disps), _p(smooth_aux), n_smooth, _ptr4(dzs),
                        disps[0].shape[0], H, W, _stream(ddisp_up))


def photo_automask_pyramid(warped, target, idmap, noise, sel, coef_sel, partial, batch, H, W):
    _lib.get_lib().call('clslam_photo_automask_pyramid', _p(warped), _p(target), _p(idmap), _p(noise), _pa(sel, torch.uint8),
                        _p(coef_sel), _p(partial), batch, H, W, _stream(warped))


def photo_automask_pyramid_rng(warped, target, idmap, seed, offset, sel, coef_sel, partial, batch, H, W):
    """tie-break noise drawn in the kernel (Philox): seed != 0, offset = draw counter of the step"""
    if not seed:
        raise _lib.ClslamError('photo_automask_pyramid_rng: seed must be non-zero')
    _lib.get_lib().call('clslam_photo_automask_pyramid_rng', _p(warped), _p(target), _p(idmap), int(seed), int(offset),
                        _pa(sel, torch.uint8), _p(coef_sel), _p(partial), batch, H, W, _stream(warped))


def tie_break_noise(out, seed, offset):
    """out (..., 2) fp32: the in-kernel tie-break stream, element e -> out.view(-1, 2)[e]"""
    _lib.get_lib().call('clslam_tie_break_noise', _p(out), out.numel() // 2, int(seed), int(offset), _stream(out))
    return out


def pair_loss(disp, src, target, inv_k, proj, noise, partial, min_depth, max_depth, depth=None, sel=None, maps=None):
    """Fused single-source view synthesis + photometric automask at scale 0: disp (B,H,W), src / target (B,3,H,W),
    proj (B,3,4), noise (B,1,H,W) already x 1e-5 or None -> partial (B, automask_blocks(H, W)); depth (B,H,W), sel (B,H,W) u8
    and maps (2,B,H,W) are written only when given."""
    B, H, W = disp.shape
    _lib.get_lib().call('clslam_pair_loss', _p(disp), _p(src), _p(target), _p(inv_k), _p(proj), _p(noise), _p(partial), _p(depth),
                        _pa(sel, torch.uint8), _p(maps), B, H, W, _nd(min_depth), _nd(max_depth), _stream(partial))


def pair_loss_rng(disp, src, target, inv_k, proj, seed, offset, partial, min_depth, max_depth, depth=None, sel=None, maps=None):
    """pair_loss with the noise drawn in the kernel: the first value of element b * H * W + pixel of tie_break_noise(seed, offset)"""
    if not seed:
        raise _lib.ClslamError('pair_loss_rng: seed must be non-zero')
    B, H, W = disp.shape
    _lib.get_lib().call('clslam_pair_loss_rng', _p(disp), _p(src), _p(target), _p(inv_k), _p(proj), int(seed), int(offset), _p(partial),
                        _p(depth), _pa(sel, torch.uint8), _p(maps), B, H, W, _nd(min_depth), _nd(max_depth), _stream(partial))


def pair_loss_scratch(batch: int) -> int:
    return _query('clslam_pair_loss_scratch', batch)


def pair_loss_finalize(partial, disp, rgb0, pose, dist, sample_w, smooth_w, intended, scratch, losses, smooth_scale, vel_scale):
    """losses (7) = reprojection, smooth, reg, depth_loss/scale_0, depth_loss (= that / 4), velocity, loss"""
    B, H, W = disp.shape
    n_smooth = 0 if (smooth_w is None or intended) else int(smooth_w.numel())
    _lib.get_lib().call('clslam_pair_loss_finalize', _p(partial), partial.shape[1], _p(disp), _p(rgb0), _p(pose),
                        _pa(dist, torch.float64), _p(sample_w), _p(smooth_w) if n_smooth else None, n_smooth, 1 if intended else 0,
                        _p(scratch), _p(losses), B, H, W, float(smooth_scale), float(vel_scale or 0.0), _stream(losses))


def smooth_intended_chunks() -> int:
    return _query('clslam_smooth_intended_chunks')


def smooth_intended_fwd(disps, rgb0, partial, H, W):
    _lib.get_lib().call('clslam_smooth_intended_fwd', _ptr4(disps), _ptr4(rgb0), _p(partial), disps[0].shape[0], H, W,
                        _stream(partial))


def smooth_intended_finalize(partial, means, sample_w, losses, aux, batch, H, W, smooth_scale):
    _lib.get_lib().call('clslam_smooth_intended_finalize', _p(partial), _p(means), _p(sample_w), _p(losses), _p(aux), batch, H, W,
                        float(smooth_scale), _stream(losses))


def smooth_intended_bwd(disps, rgb0, aux, sample_w, dz, H, W, smooth_scale):
    _lib.get_lib().call('clslam_smooth_intended_bwd', _ptr4(disps), _ptr4(rgb0), _p(aux), _p(sample_w), _ptr4(dz),
                        disps[0].shape[0], H, W, float(smooth_scale), _stream(aux))


def loss_bwd2_blocks(H, W) -> int:
    return _query('clslam_loss_bwd2_blocks', H, W)


def loss_bwd2_pyramid(disps, sel, coef_sel, warped, target, src_m1, src_p1, inv_k, proj, sample_w, ddisp_up, dp_partial,
                      min_depth, max_depth):
    B, H, W = ddisp_up.shape[1], ddisp_up.shape[-2], ddisp_up.shape[-1]
    _lib.get_lib().call('clslam_loss_bwd2_pyramid', _ptr4(disps), _pa(sel, torch.uint8), _p(coef_sel), _p(warped), _p(target),
                        _p(src_m1), _p(src_p1), _p(inv_k), _p(proj), _p(sample_w), _p(ddisp_up), _pa(dp_partial, torch.float64), B, H, W,
                        _nd(min_depth), _nd(max_depth), _stream(ddisp_up))


# ---- mask_dynamic=True: the masked loss (include/clslam_hip.h "mask_dynamic = True") --------------------------------------------
def photo_automask_pyramid_masked(warped, target, idmap, noise, seed, offset, mask0, sel, coef_sel, partial, cnt_partial,
                                  batch, H, W):
    """noise (4,B,2,H,W) or None with seed != 0 (drawn in the kernel); mask0 (B,H,W) fp32; cnt_partial (B,nblk) int32"""
    if noise is None and not seed:
        raise _lib.ClslamError('photo_automask_pyramid_masked: a noise tensor or a non-zero seed')
    _lib.get_lib().call('clslam_photo_automask_pyramid_masked', _p(warped), _p(target), _p(idmap), _p(noise), int(seed), int(offset),
                        _p(mask0), _pa(sel, torch.uint8), _p(coef_sel), _p(partial), _pa(cnt_partial, torch.int32), batch, H, W,
                        _stream(warped))


def smooth_locate(masks, loc, H, W):
    """masks: four (B,h_s,w_s) fp32 planes; loc (4,2,2B) int32"""
    _lib.get_lib().call('clslam_smooth_locate', _ptr4(masks), _pa(loc, torch.int32), masks[0].shape[0], H, W, _stream(loc))


def loss_finalize_masked(partials, disps, rgb0s, means, pose, dist0, dist1, sample_w, smooth_w, losses, smooth_aux, cnt_partial,
                         loc, mstat, batch, nblk, H, W, n_smooth, smooth_scale, vel_scale):
    d = _lib.LossDesc()
    for s in range(4):
        d.partial[s] = _p(partials[s]); d.disp[s] = _p(disps[s]); d.rgb0[s] = _p(rgb0s[s]); d.means[s] = _p(means[s])
    d.pose = _p(pose)
    d.dist0 = _pa(dist0, torch.float64); d.dist1 = _pa(dist1, torch.float64)
    d.sample_w = _p(sample_w); d.smooth_w = _p(smooth_w); d.losses = _p(losses); d.smooth_aux = _p(smooth_aux)
    d.batch, d.nblk, d.H, d.W, d.n_smooth = batch, nblk, H, W, n_smooth
    d.smooth_scale, d.vel_scale = float(smooth_scale), float(vel_scale or 0.0)
    _lib.get_lib().call('clslam_loss_finalize_masked', C.byref(d), _pa(cnt_partial, torch.int32), _pa(loc, torch.int32), _p(mstat),
                        _stream(losses))


def loss_bwd2_pyramid_masked(disps, sel, coef_sel, warped, target, src_m1, src_p1, inv_k, proj, mask0, inv_n, ddisp_up, dp_partial,
                             min_depth, max_depth):
    B, H, W = ddisp_up.shape[1], ddisp_up.shape[-2], ddisp_up.shape[-1]
    _lib.get_lib().call('clslam_loss_bwd2_pyramid_masked', _ptr4(disps), _pa(sel, torch.uint8), _p(coef_sel), _p(warped), _p(target),
                        _p(src_m1), _p(src_p1), _p(inv_k), _p(proj), _p(mask0), _p(inv_n), _p(ddisp_up),
                        _pa(dp_partial, torch.float64), B, H, W, _nd(min_depth), _nd(max_depth), _stream(ddisp_up))


def smooth_pos_bwd(disps, smooth_aux, loc, n_smooth, dzs, H, W):
    _lib.get_lib().call('clslam_smooth_pos_bwd', _ptr4(disps), _p(smooth_aux), _pa(loc, torch.int32), n_smooth, _ptr4(dzs),
                        disps[0].shape[0], H, W, _stream(smooth_aux))


def smooth_intended_masked_fwd(disps, rgb0, masks, partial, cnt, H, W):
    _lib.get_lib().call('clslam_smooth_intended_masked_fwd', _ptr4(disps), _ptr4(rgb0), _ptr4(masks), _p(partial),
                        _pa(cnt, torch.int32), disps[0].shape[0], H, W, _stream(partial))


def smooth_intended_masked_finalize(partial, cnt, means, sample_w, losses, aux, batch, H, W, smooth_scale):
    _lib.get_lib().call('clslam_smooth_intended_masked_finalize', _p(partial), _pa(cnt, torch.int32), _p(means), _p(sample_w),
                        _p(losses), _p(aux), batch, H, W, float(smooth_scale), _stream(losses))


def smooth_intended_masked_bwd(disps, rgb0, masks, aux, sample_w, dz, H, W, smooth_scale):
    _lib.get_lib().call('clslam_smooth_intended_masked_bwd', _ptr4(disps), _ptr4(rgb0), _ptr4(masks), _p(aux), _p(sample_w),
                        _ptr4(dz), disps[0].shape[0], H, W, float(smooth_scale), _stream(aux))


# ---- SE(3) pose-graph optimisation (csrc/pose_graph.hip; the Levenberg control is clslam_hip/pose_graph.py) ----------------
def _pd(t):
    return _pa(t, torch.float64)


def _pi(t):
    return _pa(t, torch.int32)


def pgo_lin_stride() -> int:
    return _query('clslam_pgo_lin_stride')


def pgo_solve_workspace(na: int) -> int:
    return _query('clslam_pgo_solve_workspace', na)


def pgo_edge_eval(est, edge_v, meas, err, jac_i, jac_j, stream):
    _lib.get_lib().call('clslam_pgo_edge_eval', _pd(est), _pi(edge_v), _pd(meas), edge_v.shape[0], _pd(err), _pd(jac_i), _pd(jac_j),
                        stream)


def pgo_build_system(est, edge_v, meas, info, huber, ne, cptr, contrib, diag, nnzb, na, lin, H, b, scal, stream):
    _lib.get_lib().call('clslam_pgo_build_system', _pd(est), _pi(edge_v), _pd(meas), _pd(info), _pd(huber), ne, _pi(cptr),
                        _pi(contrib), _pi(diag), nnzb, na, _pd(lin), _pd(H), _pd(b), _pd(scal), stream)


def pgo_solve(H, rptr, col, tri, b, lam, na, tol, max_iter, delta, work, scal, stream):
    _lib.get_lib().call('clslam_pgo_solve', _pd(H), _pi(rptr), _pi(col), _pi(tri), _pd(b), float(lam), na, float(tol), int(max_iter),
                        _pd(delta), _pd(work), _pd(scal), stream)


def pgo_update_score(est, trial, act, nv, delta, edge_v, meas, info, huber, ne, robust, scal, out_index, stream):
    _lib.get_lib().call('clslam_pgo_update_score', _pd(est), _pd(trial), _pi(act), nv, _pd(delta), _pi(edge_v), _pd(meas), _pd(info),
                        _pd(huber), ne, int(robust), _pd(scal), int(out_index), stream)


# ---- depth-error metrics (csrc/depth_eval.hip; the evaluator's API is clslam_hip/depth_eval.py) ----------------------------
def depth_metrics_scratch(n: int, hg: int, wg: int) -> int:
    return _query('clslam_depth_metrics_scratch', n, hg, wg)


def depth_metrics(pred, gt, min_depth, max_depth, median_scaling=True, from_disp=False, out=None, resampled=None, medians=None):
    """pred (N,h,w) depth (from_disp: sigmoid disparity), gt (N,Hg,Wg) -> (N,10) device tensor
    [abs_diff, abs_rel, sq_rel, a1, a2, a3, rmse, rmse_log, ratio, n] (slam/utils.py:389-442); max_depth None = no upper bound.
    resampled (N,Hg,Wg) / medians (N,2): optional extra outputs (the resampled prediction, [median gt, median pred])."""
    for name, t in (('pred', pred), ('gt', gt)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise _lib.ClslamError(f'depth_metrics: {name} must be a (N, rows, cols) tensor, got '
                                   f'{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
    N, (h, w), (hg, wg) = pred.shape[0], pred.shape[1:], gt.shape[1:]
    if gt.shape[0] != N or gt.device != pred.device:
        raise _lib.ClslamError(f'depth_metrics: pred {tuple(pred.shape)} on {pred.device} and gt {tuple(gt.shape)} on {gt.device} '
                               'must hold the same number of images on one device')
    if min_depth is None:
        raise _lib.ClslamError('depth_metrics: min_depth is required (the mask is gt > min_depth)')
    if out is None:
        out = torch.empty(N, 10, device=pred.device)
    for name, t, shape in (('out', out, (N, 10)), ('resampled', resampled, (N, hg, wg)), ('medians', medians, (N, 2))):
        if t is not None and tuple(t.shape) != shape:
            raise _lib.ClslamError(f'depth_metrics: {name} must be {shape}, got {tuple(t.shape)}')
    if N == 0:
        return out
    if min(h, w, hg, wg) == 0:
        raise _lib.ClslamError(f'depth_metrics: empty plane (pred {h}x{w}, gt {hg}x{wg})')
    words = depth_metrics_scratch(N, hg, wg)
    if words <= 0:
        raise _lib.ClslamError(f'depth_metrics: {N} planes of {hg}x{wg} are beyond the kernel\'s range (2^24 pixels per plane)')
    scratch = torch.empty((words + 1) // 2, dtype=torch.float64, device=pred.device)
    flags = ((_lib.DEPTH_EVAL_MEDIAN_SCALING if median_scaling else 0) | (_lib.DEPTH_EVAL_FROM_DISP if from_disp else 0)
             | (_lib.DEPTH_EVAL_NO_MAX if max_depth is None else 0))
    _lib.get_lib().call('clslam_depth_metrics', _p(pred), _p(gt), _p(out), _pa(scratch, torch.float64), _p(resampled), _p(medians),
                        N, h, w, hg, wg, float(min_depth), 0.0 if max_depth is None else float(max_depth), flags, _stream(pred))
    return out


# ---- trajectory and pose-error metrics (csrc/traj_eval.hip; the evaluator's API is clslam_hip/traj_eval.py) ------------------
def _poses(fn: str, name: str, t) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (4, 4) or t.dtype is not torch.float64:
        raise _lib.ClslamError(f'{fn}: {name} must be a (n, 4, 4) float64 tensor, got '
                               f'{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}')


def pose_pair_error(a, b, a_inverted=False, out=None):
    """a, b (n,4,4) fp64 -> (n,2) fp64 device tensor [translation_error, rotation_error (rad)] of inv(b_i) @ a_i, or of
    inv(b_i) @ inv(a_i) with a_inverted (slam.py:257-259 / dpp.py:505-511)"""
    fn = 'pose_pair_error'
    _poses(fn, 'a', a)
    _poses(fn, 'b', b)
    n = a.shape[0]
    if b.shape[0] != n or b.device != a.device:
        raise _lib.ClslamError(f'{fn}: a {tuple(a.shape)} on {a.device} and b {tuple(b.shape)} on {b.device} must hold the same '
                               'number of poses on one device')
    if out is None:
        out = torch.empty(n, 2, dtype=torch.float64, device=a.device)
    elif tuple(out.shape) != (n, 2):
        raise _lib.ClslamError(f'{fn}: out must be {(n, 2)}, got {tuple(out.shape)}')
    _lib.get_lib().call('clslam_pose_pair_error', _pd(a), _pd(b), n, int(bool(a_inverted)), _pd(out), _stream(a))
    return out


def traj_metrics_scratch(n: int) -> int:
    return _query('clslam_traj_metrics_scratch', n)


def traj_segments(n: int) -> int:
    """rows of the `segments` output: eight lengths for every tenth first frame (utils.py:225-230)"""
    return (n + 9) // 10 * 8


def traj_metrics(pred, gt, optimize_scale=False, out=None, segments=None, dist=None, pairs=None):
    """pred, gt (n,4,4) fp64 -> (8,) fp64 device tensor [ave_t_err, ave_r_err, n_segments, ate, rpe_trans, rpe_rot, scaling,
    path_length] (slam/utils.py:129-383).  Optional outputs: segments (ceil(n/10)*8, 6), dist (n), pairs (max(n-1, 0), 2) = the
    RPE pair errors (copied out of the scratch)."""
    fn = 'traj_metrics'
    _poses(fn, 'pred', pred)
    _poses(fn, 'gt', gt)
    n = pred.shape[0]
    if gt.shape[0] != n or gt.device != pred.device:
        raise _lib.ClslamError(f'{fn}: pred {tuple(pred.shape)} on {pred.device} and gt {tuple(gt.shape)} on {gt.device} must hold '
                               'the same number of poses on one device')
    words = traj_metrics_scratch(n)
    if words <= 0:
        raise _lib.ClslamError(f'{fn}: {n} poses are beyond the kernel\'s range ({_lib.TRAJ_MAX_POSES})')
    if out is None:
        out = torch.empty(8, dtype=torch.float64, device=pred.device)
    for name, t, shape in (('out', out, (8,)), ('segments', segments, (traj_segments(n), 6)), ('dist', dist, (n,)),
                           ('pairs', pairs, (max(n - 1, 0), 2))):
        if t is not None and tuple(t.shape) != shape:
            raise _lib.ClslamError(f'{fn}: {name} must be {shape}, got {tuple(t.shape)}')
    scratch = torch.empty(words, dtype=torch.float64, device=pred.device)
    _lib.get_lib().call('clslam_traj_metrics', _pd(pred), _pd(gt), n, int(bool(optimize_scale)), _pd(out), _pd(segments), _pd(dist),
                        _pd(scratch), _stream(pred))
    if pairs is not None and n > 1:
        pairs.copy_(scratch[8:8 + 2 * (n - 1)].view(n - 1, 2))
    return out


# ---- dense mapping (csrc/mapping.hip; the map's API is clslam_hip/mapping.py) -----------------------------------------------
def _pl(t):
    return _pa(t, torch.int64)


def _cloud(name: str, fn: str, t) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 6:
        raise _lib.ClslamError(f'{fn}: {name} must be a (M, 6) tensor, got '
                               f'{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')


def _segments(fn: str, points, offsets, poses):
    """offsets (F+1) int64 and poses (F,4,4) fp64 of a cloud, on its device; offsets given on the host (a list, an array, a host
    tensor) are checked against the cloud and uploaded, a device tensor is taken as it is (the kernels never walk past it)"""
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise _lib.ClslamError(f'{fn}: poses must be a (F, 4, 4) tensor, got '
                               f'{tuple(poses.shape) if isinstance(poses, torch.Tensor) else type(poses).__name__}')
    F = poses.shape[0]
    if not (isinstance(offsets, torch.Tensor) and offsets.device == points.device and offsets.device.type != 'cpu'):
        host = torch.as_tensor(offsets)
        if host.dim() != 1 or host.is_floating_point():
            raise _lib.ClslamError(f'{fn}: offsets must be a one-dimensional integer sequence')
        host = host.to(torch.int64).cpu()
        if host.numel() == F + 1 and (int(host[0]) != 0 or int(host[-1]) != points.shape[0] or bool((host[1:] < host[:-1]).any())):
            raise _lib.ClslamError(f'{fn}: offsets must rise from 0 to the {points.shape[0]} points of the cloud')
        offsets = host.to(points.device)
    if offsets.dim() != 1 or offsets.numel() != F + 1:
        raise _lib.ClslamError(f'{fn}: {F} poses need {F + 1} offsets, got {tuple(offsets.shape)}')
    if poses.device != points.device:
        raise _lib.ClslamError(f'{fn}: poses on {poses.device}, the cloud on {points.device}')
    if F == 0 and points.shape[0]:
        raise _lib.ClslamError(f'{fn}: {points.shape[0]} points and no segment')
    return offsets, poses


def pcl_backproject_scratch(n: int, h: int, w: int) -> int:
    return _query('clslam_pcl_backproject_scratch', n, h, w)


def pcl_backproject(depth, inv_K, image, dist_threshold=float('inf'), out=None, narrow=True):
    """depth (N,1,H,W), inv_K (N,4,4), image (N,3,H,W) fp32 -> (points (sum M,6) fp32, offsets (N+1) int64), both on the device:
    [cam_x, cam_y, cam_z, r, g, b] of the pixels with |cam| < dist_threshold, in image and pixel order (slam/utils.py:25-38).
    out: a (>= N*H*W, 6) buffer to write into.  With a finite threshold the number of rows is known on the device only:
    narrow=True reads it back (8 bytes) and returns out[:sum M]; narrow=False returns the whole buffer and reads nothing."""
    fn = 'pcl_backproject'
    for name, t, rank in (('depth', depth, 4), ('inv_K', inv_K, 3), ('image', image, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != rank:
            raise _lib.ClslamError(f'{fn}: {name} must be a tensor of rank {rank}, got '
                                   f'{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
    N, H, W = depth.shape[0], depth.shape[2], depth.shape[3]
    if depth.shape[1] != 1 or tuple(image.shape) != (N, 3, H, W) or tuple(inv_K.shape) != (N, 4, 4):
        raise _lib.ClslamError(f'{fn}: depth (N,1,H,W), inv_K (N,4,4) and image (N,3,H,W) expected, got {tuple(depth.shape)}, '
                               f'{tuple(inv_K.shape)}, {tuple(image.shape)}')
    if inv_K.device != depth.device or image.device != depth.device:
        raise _lib.ClslamError(f'{fn}: depth on {depth.device}, inv_K on {inv_K.device}, image on {image.device}')
    thr = float(dist_threshold)
    if thr != thr:
        raise _lib.ClslamError(f'{fn}: dist_threshold is NaN')
    if N and H * W == 0:
        raise _lib.ClslamError(f'{fn}: empty plane ({H}x{W})')
    rows = N * H * W
    if out is None:
        out = torch.empty(rows, 6, device=depth.device)
    _cloud('out', fn, out)
    if out.shape[0] < rows:
        raise _lib.ClslamError(f'{fn}: out has room for {out.shape[0]} rows, {N} planes of {H}x{W} may give {rows}')
    offsets = torch.empty(N + 1, dtype=torch.int64, device=depth.device)
    if N == 0:
        offsets.zero_()
        return out[:0], offsets
    words = pcl_backproject_scratch(N, H, W)
    if words <= 0:
        raise _lib.ClslamError(f'{fn}: {N} planes of {H}x{W} are beyond the kernel\'s range (65535 planes of 2^30 pixels)')
    scratch = torch.empty(words, dtype=torch.int64, device=depth.device)
    _lib.get_lib().call('clslam_pcl_backproject', _p(depth), _p(inv_K), _p(image), _p(out), _pl(offsets), _pl(scratch), N, H, W,
                        thr, _stream(depth))
    if not narrow:
        return out, offsets
    return out[:rows if thr in (float('inf'), float('-inf')) else int(offsets[-1])], offsets


def pcl_transform(points, offsets, poses, out=None):
    """points (M,6) fp32, offsets (F+1) int64, poses (F,4,4) fp64 -> (M,6): segment f posed by poses[f] in fp64, rounded once
    to fp32, colours copied (slam/utils.py:76-82)"""
    fn = 'pcl_transform'
    _cloud('points', fn, points)
    offsets, poses = _segments(fn, points, offsets, poses)
    if out is None:
        out = torch.empty_like(points)
    _cloud('out', fn, out)
    if out.shape != points.shape or out.device != points.device:
        raise _lib.ClslamError(f'{fn}: out must be {tuple(points.shape)} on {points.device}')
    M = points.shape[0]
    if M == 0:
        return out
    _lib.get_lib().call('clslam_pcl_transform', _p(points), _pl(offsets), _pd(poses), _p(out), M, poses.shape[0], _stream(points))
    return out


def pcl_splat_scratch(rows: int, cols: int) -> int:
    return _query('clslam_pcl_splat_scratch', rows, cols)


def pcl_to_image(points, K, image_shape, offsets=None, poses=None, min_z=None, return_dist=False, return_index=False,
                 max_launch_points=1 << 32):
    """points (M,6) fp32 [, offsets (F+1) int64 + poses (F,4,4) fp64 applied on the fly], K (3,3) fp64 -> (rows,cols,3) fp32:
    the colour of the closest point (Euclidean distance, lowest index among equals) that projects into each pixel, 0 elsewhere
    (slam/utils.py:41-58).  Points behind the camera project mirrored, as in the reference; min_z culls z <= min_z instead.
    return_dist / return_index add the (rows,cols) fp32 distance plane (+inf where empty) and the int64 index plane (-1).
    A launch takes max_launch_points (at most 2^32) points; a larger cloud goes in several, merged on the device."""
    fn = 'pcl_to_image'
    _cloud('points', fn, points)
    if not isinstance(K, torch.Tensor) or tuple(K.shape) != (3, 3) or K.device != points.device:
        raise _lib.ClslamError(f'{fn}: K must be a (3, 3) tensor on {points.device}')
    rows, cols = (int(v) for v in image_shape[:2])
    words = pcl_splat_scratch(rows, cols) if rows > 0 and cols > 0 else 0
    if words <= 0:
        raise _lib.ClslamError(f'{fn}: an image of {rows}x{cols} is empty or beyond 2^28 pixels')
    if (offsets is None) != (poses is None):
        raise _lib.ClslamError(f'{fn}: offsets and poses go together')
    F = 0
    if poses is not None:
        offsets, poses = _segments(fn, points, offsets, poses)
        F = poses.shape[0]
    if min_z is not None and float(min_z) != float(min_z):
        raise _lib.ClslamError(f'{fn}: min_z is NaN')
    if not 0 < max_launch_points <= 1 << 32:
        raise _lib.ClslamError(f'{fn}: max_launch_points must be in 1 .. 2^32')
    dev, M = points.device, points.shape[0]
    image = torch.empty(rows, cols, 3, device=dev)
    dist = torch.empty(rows, cols, device=dev) if return_dist or M > max_launch_points else None
    index = torch.empty(rows, cols, dtype=torch.int64, device=dev) if return_index else None
    zbuf = torch.empty(words, dtype=torch.int64, device=dev)
    lib, stream = _lib.get_lib(), _stream(points)
    base = 0
    while True:
        count = min(M - base, max_launch_points)
        lib.call('clslam_pcl_splat', _p(points) if M else None, _pl(offsets), _pd(poses), F, _pd(K), _pl(zbuf), rows, cols, base,
                 count, int(min_z is not None), 0.0 if min_z is None else float(min_z), 1, stream)
        lib.call('clslam_pcl_resolve', _p(points) if M else None, _pl(zbuf), base, _p(image), _p(dist), _pl(index), rows, cols,
                 int(base > 0), stream)
        base += count
        if base >= M:
            break
    extra = ([dist] if return_dist else []) + ([index] if return_index else [])
    return (image, *extra) if extra else image


def pcl_voxel_scratch(m: int) -> int:
    return _query('clslam_pcl_voxel_scratch', m)


def pcl_voxel_downsample(points, voxel_size, offsets=None, poses=None, min_points=1, return_info=False):
    """points (M,6) fp32 [, offsets (F+1) int64 + poses (F,4,4) fp64 applied on the fly, as pcl_transform would] ->
    (rows (V,6) fp32, counts (V,) int32) on the device: one row per cell of a grid of voxel_size with at least min_points
    members, in ascending order of key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20), i = floor(double(c) / voxel_size);
    each value is the fp64 mean of the members' fp32 values, rounded once.  Rows with a non-finite value are dropped; a cell
    index outside [-2^20, 2^20) raises.  The counts of the sort (cells, rows out of range, radix passes run, rows dropped) come
    back through pinned memory behind an event, 32 bytes; return_info=True appends them as a dict."""
    fn = 'pcl_voxel_downsample'
    _cloud('points', fn, points)
    vs = float(voxel_size)
    if not (vs > 0.0 and vs != float('inf')):
        raise _lib.ClslamError(f'{fn}: voxel_size must be finite and above 0, got {voxel_size}')
    if int(min_points) != min_points or min_points < 1 or min_points >= 1 << 31:
        raise _lib.ClslamError(f'{fn}: min_points must be an integer of at least 1, got {min_points}')
    if (offsets is None) != (poses is None):
        raise _lib.ClslamError(f'{fn}: offsets and poses go together')
    F = 0
    if poses is not None:
        offsets, poses = _segments(fn, points, offsets, poses)
        F = poses.shape[0]
    dev, M = points.device, points.shape[0]
    if M == 0:
        empty = torch.empty(0, 6, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        return (*empty, {'cells': 0, 'out_of_range': 0, 'passes': 0, 'dropped': 0}) if return_info else empty
    words = pcl_voxel_scratch(M)
    if words <= 0:
        raise _lib.ClslamError(f'{fn}: one call takes fewer than 2^31 points, got {M}')
    scratch = torch.empty(words, dtype=torch.int64, device=dev)
    lib, stream = _lib.get_lib(), _stream(points)
    lib.call('clslam_pcl_voxel_sort', _p(points), _pl(offsets), _pd(poses), F, M, vs, int(min_points), _pl(scratch), stream)
    if scratch.is_cuda:
        host = torch.empty(4, dtype=torch.int64, pin_memory=True)
        if _FORCED_STREAM is None:
            host.copy_(scratch[2:6], non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(dev))
            event.synchronize()
        else:                                   # a launch_on() stream torch does not know: wait for it as a whole
            torch.cuda.synchronize(dev)
            host.copy_(scratch[2:6])
    else:
        host = scratch[2:6]
    cells, out_of_range, passes, dropped = (int(v) for v in host)
    if out_of_range:
        raise _lib.ClslamError(f'{fn}: {out_of_range} of {M} points fall into cells beyond index -2^20 .. 2^20 - 1 at voxel_size {vs}')
    rows = torch.empty(cells, 6, device=dev)
    counts = torch.empty(cells, dtype=torch.int32, device=dev)
    lib.call('clslam_pcl_voxel_reduce', _p(points), _pl(offsets), _pd(poses), F, M, _pl(scratch), _p(rows) if cells else None,
             _pi(counts) if cells else None, cells, stream)
    info = {'cells': cells, 'out_of_range': out_of_range, 'passes': passes, 'dropped': dropped}
    return (rows, counts, info) if return_info else (rows, counts)


# ----------------------------------------------------------------------------------------------------------------------
# Frame store of the replay ingest (clslam_store_*, include/clslam_hip.h)
def store_pack(planes, offsets, slot: torch.Tensor, inexact: torch.Tensor) -> None:
    """planes: contiguous float tensors on the library's device (3 * h * w values each), written as bytes to slot[offsets[k]:];
    `inexact` (int64, 1 element) counts the values that are no byte / 255."""
    if len(planes) != len(offsets) or len(planes) > _lib.STORE_MAX_PLANES:
        raise _lib.ClslamError(f'store_pack: {len(planes)} planes, {len(offsets)} offsets (at most {_lib.STORE_MAX_PLANES})')
    desc = _lib.StorePackDesc()
    desc.n_planes = len(planes)
    for k, (t, off) in enumerate(zip(planes, offsets)):
        if off < 0 or off + t.numel() > slot.numel():
            raise _lib.ClslamError(f'store_pack: plane {k} ({t.numel()} bytes at {off}) leaves the slot ({slot.numel()} bytes)')
        desc.plane[k], desc.offset[k], desc.count[k] = _p(t), int(off), t.numel()
    _lib.get_lib().call('clslam_store_pack', C.byref(desc), _pa(slot, torch.uint8), _pa(inexact, torch.int64), _stream(slot))


def store_gather_jitter(store: torch.Tensor, slot_bytes: int, offsets, sizes, n_frames: int, slot_idx: torch.Tensor,
                        params: Optional[torch.Tensor], rgb, aug, row0: int) -> None:
    """store (capacity * slot_bytes,) uint8; offsets[frame * n_levels + level] bytes inside a slot; sizes[level] = (h, w);
    slot_idx (n_images,) int32, < 0 = skip; rgb / aug: per table entry a contiguous (rows, 3, h, w) float tensor (aug None: no
    jitter), image i goes to row row0 + i // n_frames."""
    n_levels, n_img = len(sizes), slot_idx.numel()
    n_tab = n_frames * n_levels
    if n_tab > _lib.STORE_MAX_PLANES or len(offsets) != n_tab or len(rgb) != n_tab or n_img % n_frames:
        raise _lib.ClslamError(f'store_gather_jitter: {n_frames} frames x {n_levels} levels, {len(offsets)} offsets, {len(rgb)} outputs, '
                               f'{n_img} images')
    if aug is not None and (len(aug) != n_tab or params is None or params.numel() != n_img * 48):
        raise _lib.ClslamError(f'store_gather_jitter: rgb_aug rows need {n_tab} outputs and 48 parameter bytes per image')
    desc = _lib.StoreGatherDesc()
    desc.n_frames, desc.n_levels, desc.slot_bytes = n_frames, n_levels, int(slot_bytes)
    desc.capacity = store.numel() // int(slot_bytes)
    rows_needed = row0 + n_img // n_frames
    for li, (h, w) in enumerate(sizes):
        desc.h[li], desc.w[li] = int(h), int(w)
    for t in range(n_tab):
        h, w = sizes[t % n_levels]
        if offsets[t] < 0 or offsets[t] + 3 * h * w > slot_bytes:
            raise _lib.ClslamError(f'store_gather_jitter: entry {t} leaves the slot')
        for out in (rgb[t],) + (() if aug is None else (aug[t],)):
            if out.dim() != 4 or tuple(out.shape[1:]) != (3, h, w) or out.shape[0] < rows_needed:
                raise _lib.ClslamError(f'store_gather_jitter: entry {t} needs ({rows_needed}+, 3, {h}, {w}), got {tuple(out.shape)}')
        desc.rgb[t], desc.aug[t] = _p(rgb[t]), None if aug is None else _p(aug[t])
        desc.stride[t], desc.offset[t] = 3 * h * w, int(offsets[t])
    partial = torch.empty(n_levels * max(n_img, 1) * 64, device=store.device) if aug is not None else None
    _lib.get_lib().call('clslam_store_gather_jitter', C.byref(desc), _pa(store, torch.uint8), _pa(slot_idx, torch.int32),
                        None if aug is None else _pa(params, torch.uint8), _p(partial), n_img, int(row0), _stream(store))


# ----------------------------------------------------------------------------------------------------------------------
# Online ingest: ring of per-frame uint8 pyramids (clslam_resize_level_u8, clslam_ring_gather, include/clslam_hip.h)
def resize_level_u8(src: torch.Tensor, dst: torch.Tensor, out_h: int, out_w: int, plan_h, plan_v, pitch: Optional[int] = None) -> None:
    """src (N,h,w,3) uint8 -> the bytes of `dst` (flat uint8, starting at the first output pixel) as (N,out_h,out_w,3) with `pitch`
    bytes per row (default out_w * 3): Pillow's LANCZOS resize, both passes in one launch.  plan_h / plan_v = (bounds, coeffs,
    ksize) on the device for w -> out_w / h -> out_h, None for an axis that keeps its size."""
    if src.dim() != 4 or src.shape[-1] != 3:
        raise _lib.ClslamError(f'resize_level_u8 expects (N,h,w,3) uint8 frames, got {tuple(src.shape)}')
    N, h, w, _ = src.shape
    pitch = out_w * 3 if pitch is None else int(pitch)
    if pitch < out_w * 3 or dst.numel() < (N * out_h - 1) * pitch + out_w * 3:
        raise _lib.ClslamError(f'resize_level_u8: {N} x {out_h} rows of {out_w} pixels at pitch {pitch} leave the {dst.numel()} bytes of dst')
    if (w != out_w and plan_h is None) or (h != out_h and plan_v is None):
        raise _lib.ClslamError(f'resize_level_u8: {h} x {w} -> {out_h} x {out_w} needs a tap plan per resized axis')
    bh, kh, ksh = plan_h if w != out_w else (None, None, 0)
    bv, kv, ksv = plan_v if h != out_h else (None, None, 0)
    _lib.get_lib().call('clslam_resize_level_u8', _pa(src, torch.uint8), _pa(dst, torch.uint8), pitch, _pa(bh, torch.int32),
                        _pa(kh, torch.int32), ksh, _pa(bv, torch.int32), _pa(kv, torch.int32), ksv, N, h, w, 3, int(out_h), int(out_w),
                        _stream(src))


def ring_gather(ring: torch.Tensor, slot_bytes: int, offsets, sizes, slots, rgb, aug) -> None:
    """ring (capacity * slot_bytes,) uint8; offsets[level] bytes inside a slot, sizes[level] = (h, w); slots[frame] = the slot of that
    frame; rgb / aug [frame * levels + level]: distinct contiguous float tensors of 3 * h * w values, both <- byte / 255."""
    n_levels, n_frames = len(sizes), len(slots)
    n_tab = n_frames * n_levels
    if n_tab > _lib.STORE_MAX_PLANES or len(offsets) != n_levels or len(rgb) != n_tab or len(aug) != n_tab:
        raise _lib.ClslamError(f'ring_gather: {n_frames} frames x {n_levels} levels, {len(offsets)} offsets, {len(rgb)} + {len(aug)} outputs')
    desc = _lib.RingGatherDesc()
    desc.n_frames, desc.n_levels, desc.slot_bytes = n_frames, n_levels, int(slot_bytes)
    desc.capacity = ring.numel() // int(slot_bytes)
    for li, (h, w) in enumerate(sizes):
        desc.h[li], desc.w[li], desc.offset[li] = int(h), int(w), int(offsets[li])
    for fi, slot in enumerate(slots):
        desc.slot[fi] = int(slot)
    for t in range(n_tab):
        h, w = sizes[t % n_levels]
        for out in (rgb[t], aug[t]):
            if out.numel() != 3 * h * w:
                raise _lib.ClslamError(f'ring_gather: entry {t} needs 3 x {h} x {w} values, got {tuple(out.shape)}')
        desc.rgb[t], desc.aug[t] = _p(rgb[t]), _p(aug[t])
    _lib.get_lib().call('clslam_ring_gather', C.byref(desc), _pa(ring, torch.uint8), _stream(ring))


# ----------------------------------------------------------------------------------------------------------------------
# RobotCar raw frames (csrc/robotcar.hip; the reference's names are in clslam_hip/robotcar.py)
def _bayer(fn: str, pattern) -> int:
    code = _lib.BAYER_PATTERNS.get(pattern.lower() if isinstance(pattern, str) else pattern)
    if code is None:
        raise ValueError(f'{fn}: pattern must be one of {sorted(_lib.BAYER_PATTERNS)}, got {pattern!r}')
    return code


def _frames(fn: str, name: str, t, rank: int, dtypes) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != rank or t.dtype not in dtypes:
        raise _lib.ClslamError(f'{fn}: {name} must be a tensor of rank {rank} and dtype {" or ".join(str(d) for d in dtypes)}, got '
                               f'{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}')
    if t.numel() and min(t.shape[1:]) == 0:
        raise _lib.ClslamError(f'{fn}: {name} has an empty plane, {tuple(t.shape)}')


def _lut(fn: str, lut, like: torch.Tensor) -> None:
    """the (2,H,W) float64 table of (row, col) source coordinates for frames shaped like `like` (N,H,W,...), on their device"""
    H, W = like.shape[1], like.shape[2]
    if not isinstance(lut, torch.Tensor) or lut.dtype is not torch.float64 or tuple(lut.shape) != (2, H, W):
        raise _lib.ClslamError(f'{fn}: lut must be a {(2, H, W)} float64 tensor for frames of {H}x{W}, got '
                               f'{(tuple(lut.shape), lut.dtype) if isinstance(lut, torch.Tensor) else type(lut).__name__}')
    if lut.device != like.device:
        raise _lib.ClslamError(f'{fn}: lut on {lut.device}, the frames on {like.device}')


def _out_like(fn: str, out, shape, dtype, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype is not dtype or out.device != like.device:
        raise _lib.ClslamError(f'{fn}: out must be {tuple(shape)} {dtype} on {like.device}, got {tuple(out.shape)} {out.dtype} on {out.device}')
    return out


def demosaic_bilinear(cfa, pattern, out=None):
    """cfa (N,H,W) uint8 Bayer mosaic -> (N,H,W,3) float64: colour_demosaicing.demosaicing_CFA_Bayer_bilinear (datasets/robotcar.py:544),
    borders by scipy.ndimage's 'reflect'"""
    fn = 'demosaic_bilinear'
    code = _bayer(fn, pattern)
    _frames(fn, 'cfa', cfa, 3, (torch.uint8,))
    N, H, W = cfa.shape
    out = _out_like(fn, out, (N, H, W, 3), torch.float64, cfa)
    for n0 in range(0, N, 65535):
        n = min(65535, N - n0)
        _lib.get_lib().call('clslam_demosaic_bilinear', _pa(cfa[n0:n0 + n], torch.uint8), _pd(out[n0:n0 + n]), n, H, W, code, _stream(cfa))
    return out


def undistort_lut(image, lut, out=None):
    """image (N,H,W,C) uint8 or float64, lut (2,H,W) float64 (row, col) -> the same shape and dtype: per channel
    scipy.ndimage.map_coordinates(order=1, mode='constant', cval=0) (datasets/robotcar.py:631-642); uint8 = trunc(t) & 255"""
    fn = 'undistort_lut'
    _frames(fn, 'image', image, 4, (torch.uint8, torch.float64))
    _lut(fn, lut, image)
    N, H, W, Cn = image.shape
    out = _out_like(fn, out, image.shape, image.dtype, image)
    _lib.get_lib().call('clslam_undistort_lut', _pa(image, image.dtype), _pd(lut), _pa(out, image.dtype), N, H, W, Cn,
                        int(image.dtype is torch.float64), _stream(image))
    return out


def robotcar_rectify(cfa, lut, pattern, out=None):
    """cfa (N,H,W) uint8 raw frames, lut (2,H,W) float64 -> (N,H,W,3) uint8 = undistort_lut(demosaic_bilinear(cfa)) as uint8, one
    launch, no float64 image in memory (datasets/robotcar.py:522-548 _load_image with a model)"""
    fn = 'robotcar_rectify'
    code = _bayer(fn, pattern)
    _frames(fn, 'cfa', cfa, 3, (torch.uint8,))
    _lut(fn, lut, cfa)
    N, H, W = cfa.shape
    out = _out_like(fn, out, (N, H, W, 3), torch.uint8, cfa)
    _lib.get_lib().call('clslam_robotcar_rectify', _pa(cfa, torch.uint8), _pd(lut), _pa(out, torch.uint8), N, H, W, code, _stream(cfa))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# PNG encoding (csrc/png_encode.hip; the user-facing names are in clslam_hip/png.py)
def _png_filter_code(fn: str, filter) -> int:
    code = _lib.PNG_FILTERS.get(filter.lower()) if isinstance(filter, str) else filter
    if isinstance(code, bool) or not isinstance(code, int) or not (_lib.PNG_FILTER_ADAPTIVE <= code <= 4):
        raise _lib.ClslamError(f'{fn}: filter must be one of {sorted(_lib.PNG_FILTERS)} or a type 0..4, got {filter!r}')
    return code


def _png_images(fn: str, images):
    """(N,H,W) or (N,H,W,3) contiguous uint8 on the kernels' device -> (N, H, W, channels, filtered bytes per image)"""
    if not isinstance(images, torch.Tensor) or images.dtype is not torch.uint8 or images.dim() not in (3, 4) \
            or (images.dim() == 4 and images.shape[3] != 3):
        raise _lib.ClslamError(f'{fn}: images must be an (N,H,W) or (N,H,W,3) uint8 tensor, got '
                               f'{(tuple(images.shape), images.dtype) if isinstance(images, torch.Tensor) else type(images).__name__}')
    if not images.is_contiguous():
        raise _lib.ClslamError(f'{fn}: images must be contiguous')
    N, H, W = images.shape[:3]
    Cn = 3 if images.dim() == 4 else 1
    if png_bound(H, W, Cn) == 0:
        raise _lib.ClslamError(f'{fn}: images of {H}x{W}x{Cn} are not taken (H, W >= 1, at most 2^27 filtered bytes each)')
    return N, H, W, Cn, H * (1 + W * Cn)


def png_bound(h: int, w: int, channels: int) -> int:
    """worst-case size of the PNG file of an (h, w[, 3]) uint8 image (clslam_png_bound; 0: a geometry the library does not take)"""
    return int(_query('clslam_png_bound', int(h), int(w), int(channels)))


def png_filter(images, filter=_lib.PNG_FILTER_ADAPTIVE, out=None):
    """images (N,H,W) or (N,H,W,3) uint8 -> (N, H * (1 + W * channels)) uint8: every scanline behind its filter type byte
    (RFC 2083 section 6).  filter 'adaptive' (per row the smallest sum of min(b, 256 - b), ties to the lowest type) or a type 0..4."""
    fn = 'png_filter'
    code = _png_filter_code(fn, filter)
    N, H, W, Cn, F = _png_images(fn, images)
    out = _out_like(fn, out, (N, F), torch.uint8, images)
    _lib.get_lib().call('clslam_png_filter', _pa(images, torch.uint8), _pa(out, torch.uint8), F, N, H, W, Cn, code, _stream(images))
    return out


def _png_files(fn: str, out, N: int, H: int, W: int, Cn: int, like: torch.Tensor):
    """-> (files (N, stride) uint8, lengths (N,) int32): stride >= clslam_png_bound, a multiple of 4"""
    bound = png_bound(H, W, Cn)
    if out is None:
        out = torch.empty((N, (bound + 3) & ~3), dtype=torch.uint8, device=like.device)
    elif not isinstance(out, torch.Tensor) or out.dtype is not torch.uint8 or out.dim() != 2 or out.shape[0] != N \
            or out.device != like.device or not out.is_contiguous():
        raise _lib.ClslamError(f'{fn}: out must be a contiguous ({N}, >= {bound}) uint8 tensor on {like.device}')
    return out, torch.empty((N,), dtype=torch.int32, device=like.device)


def png_deflate(filtered, h: int, w: int, channels: int, out=None):
    """filtered (N, F >= h * (1 + w * channels)) uint8, rows 16-byte aligned -> (files (N, stride) uint8, lengths (N,) int32): the
    complete PNG file of every filtered stream, literal-only dynamic / stored deflate blocks of 16 KiB (include/clslam_hip.h)"""
    fn = 'png_deflate'
    if not isinstance(filtered, torch.Tensor) or filtered.dtype is not torch.uint8 or filtered.dim() != 2:
        raise _lib.ClslamError(f'{fn}: filtered must be an (N, F) uint8 tensor')
    N = filtered.shape[0]
    if png_bound(h, w, channels) == 0:
        raise _lib.ClslamError(f'{fn}: images of {h}x{w}x{channels} are not taken')
    out, lengths = _png_files(fn, out, N, h, w, channels, filtered)
    nbytes = int(_query('clslam_png_scratch', N, int(h), int(w), int(channels)))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=filtered.device)
    _lib.get_lib().call('clslam_png_deflate', _pa(filtered, torch.uint8), filtered.shape[1], _pa(out, torch.uint8), out.shape[1],
                        _pa(lengths, torch.int32), _pa(scratch, torch.uint8), nbytes, N, int(h), int(w), int(channels),
                        _stream(filtered))
    return out, lengths


def png_encode(images, filter=_lib.PNG_FILTER_ADAPTIVE, out=None):
    """images (N,H,W) or (N,H,W,3) uint8 -> (files (N, stride) uint8, lengths (N,) int32): file i is files[i, :lengths[i]].  One set
    of launches for the batch, nothing synchronises; `out` (N, >= png_bound(H, W, channels), a multiple of 4) is overwritten."""
    fn = 'png_encode'
    code = _png_filter_code(fn, filter)
    N, H, W, Cn, _ = _png_images(fn, images)
    out, lengths = _png_files(fn, out, N, H, W, Cn, images)
    nbytes = int(_query('clslam_png_scratch', N, H, W, Cn))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=images.device)
    _lib.get_lib().call('clslam_png_encode', _pa(images, torch.uint8), _pa(out, torch.uint8), out.shape[1], _pa(lengths, torch.int32),
                        _pa(scratch, torch.uint8), nbytes, N, H, W, Cn, code, _stream(images))
    return out, lengths


# ----------------------------------------------------------------------------------------------------------------------
# Frame panels (csrc/viz.hip; the user-facing names are in clslam_hip/viz.py)
_VIZ_IMAGE_KINDS = {torch.float32: _lib.VIZ_ROW_HWC_F32, torch.float64: _lib.VIZ_ROW_HWC_F64, torch.uint8: _lib.VIZ_ROW_HWC_U8}


def viz_range(planes, q: float = 95.0):
    """planes (N,H,W) fp32 -> (range (N,2) fp32 = {vmin, vmax}, count (N,) int32) on the device: the smallest finite value, the
    q-th percentile of the finite values by the float64 rule of include/clslam_hip.h, their number.  Nothing synchronises."""
    fn = 'viz_range'
    if not isinstance(planes, torch.Tensor) or planes.dtype is not torch.float32 or planes.dim() != 3 or planes.shape[0] == 0 \
            or planes.shape[1] * planes.shape[2] == 0:
        raise _lib.ClslamError(f'{fn}: planes must be a non-empty (N,H,W) float32 tensor, got '
                               f'{(tuple(planes.shape), planes.dtype) if isinstance(planes, torch.Tensor) else type(planes).__name__}')
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise _lib.ClslamError(f'{fn}: q must lie in [0, 100], got {q}')
    N, npx = planes.shape[0], planes.shape[1] * planes.shape[2]
    rng = torch.empty((N, 2), dtype=torch.float32, device=planes.device)
    count = torch.empty((N,), dtype=torch.int32, device=planes.device)
    for n0 in range(0, N, 65535):
        n = min(65535, N - n0)
        nbytes = int(_query('clslam_viz_range_scratch', n))
        scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device=planes.device)
        _lib.get_lib().call('clslam_viz_range', _pa(planes[n0:n0 + n], torch.float32), _pa(rng[n0:n0 + n], torch.float32),
                            _pa(count[n0:n0 + n], torch.int32), _pa(scratch, torch.int64), nbytes, n, npx, q, _stream(planes))
    return rng, count


def viz_image_row(image, chw: bool = False):
    """a row of a panel from an image: (N,3,H,W) fp32 in [0,1] with chw, else (N,H,W,3) fp32 / fp64 / uint8"""
    return ('image', image, bool(chw))


def viz_cmap_row(planes, rng, cmap='magma_r'):
    """a row of a panel from planes (N,H,W) fp32 through the colour map, rng (N,2) fp32 {vmin, vmax} on the device"""
    return ('cmap', planes, rng, cmap)


def viz_traj_row(gt_xz, pred_xz, xlim=(-400.0, 15.0), ylim=(-60.0, 160.0)):
    """a white row with the polylines gt_xz (Ng,2) and pred_xz (Np,2), fp64 on the device (either may be None or empty)"""
    return ('traj', gt_xz, pred_xz, tuple(xlim), tuple(ylim))


def viz_compose(rows, n: int, h: int, w: int, dst=None, row0: int = 0):
    """rows: up to four of viz_image_row / viz_cmap_row / viz_traj_row -> dst (n, >= row0 + len(rows) * h, >= w, 3) uint8: row r
    fills the pixel rows [row0 + r*h, row0 + (r+1)*h) x [0, w) of every image, ONE launch, nothing else of dst is written.  dst
    may be a view with wider rows (stride(1) >= 3 * w, pixels and channels dense); None: a new (n, len(rows) * h, w, 3)."""
    fn = 'viz_compose'
    lib = _lib.get_lib()
    n, h, w, row0 = int(n), int(h), int(w), int(row0)
    if not 1 <= len(rows) <= _lib.VIZ_MAX_ROWS:
        raise _lib.ClslamError(f'{fn}: 1..{_lib.VIZ_MAX_ROWS} rows, got {len(rows)}')
    if n < 1 or h < 1 or not 1 <= w <= _lib.VIZ_MAX_W:
        raise _lib.ClslamError(f'{fn}: n >= 1 images of h >= 1, 1 <= w <= {_lib.VIZ_MAX_W}, got n={n} h={h} w={w}')
    descs = (_lib.VizRow * len(rows))()
    keep = []                                                  # the tensors behind the descriptors' pointers
    for d, row in zip(descs, rows):
        if row[0] == 'image':
            _, t, chw = row
            shape = (n, 3, h, w) if chw else (n, h, w, 3)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or (t.dtype is not torch.float32 if chw else t.dtype not in _VIZ_IMAGE_KINDS):
                raise _lib.ClslamError(f'{fn}: an image row must be {shape} {"float32" if chw else "float32 / float64 / uint8"}, got '
                                       f'{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}')
            d.kind = _lib.VIZ_ROW_CHW_F32 if chw else _VIZ_IMAGE_KINDS[t.dtype]
            d.src, d.src_stride = _pa(t, t.dtype), 3 * h * w
            keep.append(t)
        elif row[0] == 'cmap':
            _, t, rng, cmap = row
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n, h, w) or t.dtype is not torch.float32:
                raise _lib.ClslamError(f'{fn}: a colour row must be ({n},{h},{w}) float32, got '
                                       f'{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}')
            if not isinstance(rng, torch.Tensor) or tuple(rng.shape) != (n, 2) or rng.dtype is not torch.float32:
                raise _lib.ClslamError(f'{fn}: the range of a colour row must be ({n},2) float32')
            if cmap not in _lib.VIZ_CMAPS:
                raise _lib.ClslamError(f'{fn}: cmap must be one of {sorted(_lib.VIZ_CMAPS)}, got {cmap!r}')
            d.kind, d.cmap = _lib.VIZ_ROW_CMAP, _lib.VIZ_CMAPS[cmap]
            d.src, d.src_stride, d.range = _pa(t, torch.float32), h * w, _pa(rng, torch.float32)
            keep += [t, rng]
        elif row[0] == 'traj':
            _, gt, pred, xlim, ylim = row
            d.kind = _lib.VIZ_ROW_TRAJ
            d.xlim[0], d.xlim[1], d.ylim[0], d.ylim[1] = float(xlim[0]), float(xlim[1]), float(ylim[0]), float(ylim[1])
            for name, line in (('gt_xz', gt), ('pred_xz', pred)):
                if line is None or (isinstance(line, torch.Tensor) and line.numel() == 0):
                    continue
                if not isinstance(line, torch.Tensor) or line.dim() != 2 or line.shape[1] != 2 or line.dtype is not torch.float64:
                    raise _lib.ClslamError(f'{fn}: {name} must be an (N,2) float64 tensor')
                setattr(d, name, _pd(line))
                setattr(d, 'n_gt' if name == 'gt_xz' else 'n_pred', line.shape[0])
                keep.append(line)
        else:
            raise _lib.ClslamError(f'{fn}: unknown row {row[0]!r}')
    device = keep[0].device if keep else torch.device('cuda', torch.cuda.current_device()) if lib.is_device else torch.device('cpu')
    if dst is None:
        dst = torch.empty((n, row0 + len(rows) * h, w, 3), dtype=torch.uint8, device=device)
    if not isinstance(dst, torch.Tensor) or dst.dtype is not torch.uint8 or dst.dim() != 4 or dst.shape[0] != n or dst.shape[3] != 3 \
            or dst.shape[1] < row0 + len(rows) * h or dst.shape[2] < w or row0 < 0 or dst.stride(3) != 1 or dst.stride(2) != 3 \
            or dst.stride(1) < 3 * w or dst.device.type != lib.device_type:
        raise _lib.ClslamError(f'{fn}: dst must be ({n}, >= {row0 + len(rows) * h}, >= {w}, 3) uint8 on {lib.device_type} with dense '
                               f'pixels, got {(tuple(dst.shape), dst.dtype, dst.stride()) if isinstance(dst, torch.Tensor) else type(dst).__name__}')
    lib.call('clslam_viz_compose', descs, len(rows), dst.data_ptr(), dst.stride(0) if n > 1 else 0, dst.stride(1), row0, n, h, w,
             _stream(dst))
    return dst
