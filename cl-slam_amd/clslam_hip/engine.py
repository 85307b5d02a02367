"""The per-frame schedule of the MI355X-native depth/pose path.

One ``Engine`` owns, in HBM:
  * the frozen encoder weights, re-laid out once per ``load`` (OHWI conv weights, eval-mode
    BatchNorm folded into per-channel scale/shift -- legal because adaptation never changes encoder
    or BN parameters, dpp.py:308,813-819),
  * ONE flat fp32 arena for the 36 trainable tensors (depth decoder + pose decoder, 4.47 M floats)
    and three more of the same layout for gradients and Adam's two moments -- so the data-parallel
    gradient exchange is a single all-reduce and Adam a single kernel,
  * a workspace of NHWC activations and loss-stage planes, planned once per batch size (every shape
    is static given B, H, W).
and sequences the C-ABI kernels (clslam_hip.ops) for: encoder/decoder/pose forward -> view synthesis
+ loss -> hand-written backward of everything that has gradients -> fused Adam.  No torch autograd,
no torch.nn compute: torch supplies device memory, streams and torch.distributed only.

Reference call graph being replaced: dpp.py:906-923 (_process_batch), :925-974, :976-1017,
:1019-1120, and dpp.py:309-313 (zero_grad / backward / optimizer.step).
"""
import contextlib
import itertools
import math
import os
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import ops
from ._lib import ACT_ELU, ACT_NONE, ACT_RELU, PAD_REFLECT, PAD_ZERO, ClslamError, get_lib

NUM_CH_ENC = (64, 64, 128, 256, 512)
NUM_CH_DEC = (16, 32, 64, 128, 256)
BN_EPS = 1e-5

LOSS_NAMES = ('reprojection_loss', 'smooth_loss', 'reg_loss', 'depth_loss')

# blocks a weight-gradient launch is split into, two per CU: 256 / 128 would halve / quarter the 220 MB of split partials but
# measured 3.38 / 3.44 ms per step against 3.34 (the wgrad launches become the tail of the backward)
WGRAD_TARGET_BLOCKS = 512


def _align4(n: int) -> int:
    return (n + 3) // 4 * 4


class TrainableLayout:
    """Flat arena layout of the trainable tensors in compute order; names are
    '<model>/<state-dict key>' in the reference's parameter order."""

    def __init__(self) -> None:
        self.entries: List[Tuple[str, int, Tuple[int, ...]]] = []  # (name, offset, reference shape)
        self.offset: Dict[str, int] = {}
        off = 0

        def add(name: str, shape: Tuple[int, ...]) -> None:
            nonlocal off
            self.entries.append((name, off, shape))
            self.offset[name] = off
            off = _align4(off + math.prod(shape))

        for i in range(4, -1, -1):
            cin0 = NUM_CH_ENC[-1] if i == 4 else NUM_CH_DEC[i + 1]
            add(f'depth_decoder/upconv_{i}_0.conv.conv.weight', (NUM_CH_DEC[i], cin0, 3, 3))
            add(f'depth_decoder/upconv_{i}_0.conv.conv.bias', (NUM_CH_DEC[i],))
            cin1 = NUM_CH_DEC[i] + (NUM_CH_ENC[i - 1] if i > 0 else 0)
            add(f'depth_decoder/upconv_{i}_1.conv.conv.weight', (NUM_CH_DEC[i], cin1, 3, 3))
            add(f'depth_decoder/upconv_{i}_1.conv.conv.bias', (NUM_CH_DEC[i],))
        for s in range(4):
            # weight immediately followed by its bias (clslam_dispconv_wgrad reduces both at once)
            name = f'depth_decoder/dispconv_{s}.conv.weight'
            self.entries.append((name, off, (1, NUM_CH_DEC[s], 3, 3)))
            self.offset[name] = off
            off += 9 * NUM_CH_DEC[s]
            name = f'depth_decoder/dispconv_{s}.conv.bias'
            self.entries.append((name, off, (1,)))
            self.offset[name] = off
            off = _align4(off + 1)
        add('pose_decoder/squeeze.weight', (256, 512, 1, 1))
        add('pose_decoder/squeeze.bias', (256,))
        for k in (0, 1):
            add(f'pose_decoder/pose_{k}.weight', (256, 256, 3, 3))
            add(f'pose_decoder/pose_{k}.bias', (256,))
        add('pose_decoder/pose_2.weight', (12, 256, 1, 1))
        add('pose_decoder/pose_2.bias', (12,))
        self.size = off

    @staticmethod
    def to_compute(t: torch.Tensor) -> torch.Tensor:
        """reference OIHW -> OHWI ([Cout][taps][Cin]); 1-D tensors unchanged."""
        return t.permute(0, 2, 3, 1).reshape(-1) if t.dim() == 4 else t.reshape(-1)

    @staticmethod
    def to_reference(flat: torch.Tensor, shape: Tuple[int, ...]) -> torch.Tensor:
        if len(shape) == 4:
            o, i, kh, kw = shape
            return flat.view(o, kh, kw, i).permute(0, 3, 1, 2)
        return flat.view(shape)


_STREAM_POOL: Dict[Any, Dict[str, Any]] = {}


def _device_streams(device) -> Dict[str, Any]:
    """main / side / wgrad / tail streams of this process on `device` (created once)."""
    if device.type != 'cuda':
        return {}
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    pool = _STREAM_POOL.get(key)
    if pool is None:
        pool = {name: torch.cuda.Stream(device=device, priority=0) for name in ('main', 'side', 'wg', 'tail')}
        _STREAM_POOL[key] = pool
    return pool


class Engine:
    def __init__(self, height: int, width: int, device: torch.device, *, min_depth: Optional[float],
                 max_depth: Optional[float], disparity_smoothness: float, velocity_loss_scaling: Optional[float],
                 reference_quirks: bool = True, mask_dynamic: bool = False) -> None:
        lib = get_lib()  # raises if libclslam_hip.so is missing -- there is no fallback
        if device.type != lib.device_type:
            raise ClslamError(f'engine on {device} but {lib.path.name} executes on {lib.device_type}; the MI355X path '
                              'needs a GPU and has no CPU fallback')
        if height % 32 or width % 32:
            raise ValueError('height and width must be multiples of 32 (five stride-2 stages)')
        # reference_quirks=False: the per-sample edge-aware smoothness the reference evidently meant instead of
        # the flattened-batch behaviour of dpp.py:1148-1176; opt-in, parity runs use the default
        self.smooth_intended = not reference_quirks
        # mask_dynamic=True (dpp.py:1063-1090): "potentially dynamic" pixels (inputs['mask', 0, s] == 1) leave the reprojection
        # mean and the smoothness; the reprojection term becomes one mean over the static pixels of the whole minibatch
        # (no sample weights).  A second loss stage beside the unmasked one (_masked_loss / _masked_loss_backward).
        self.mask_dynamic = bool(mask_dynamic)
        if min_depth is None and max_depth is not None:
            raise ValueError('min_depth is None')        # disp_to_depth, utils.py:134-135
        self.H, self.W, self.device = height, width, device
        self.min_depth, self.max_depth = min_depth, max_depth
        self.smooth_scale = float(disparity_smoothness)
        self.vel_scale = float(velocity_loss_scaling) if velocity_loss_scaling else 0.0
        self.layout = TrainableLayout()
        n = self.layout.size
        # the four arenas; `engine.w / g / m / v` (properties below) are the same tensors for OUTSIDE readers: the access
        # orders the current stream behind the training step still in flight on the engine's own stream
        self._w = torch.zeros(n, device=device)
        self._wb_cache: Dict[str, Any] = {}
        self._desc_cache: Dict[Any, Any] = {}     # conv descriptors of this engine's fixed call sites (ops.conv2d(cache=...))
        self._main = None
        self._g = torch.zeros(n, device=device)
        self._m = torch.zeros(n, device=device)
        self._v = torch.zeros(n, device=device)
        self.adam_step_count = 0
        self.enc: Dict[str, Any] = {}
        self._ws: Dict[int, SimpleNamespace] = {}
        self.models = None
        self._packed_version = None
        self._tracked = None
        self._modules_stale = False
        # The streams are shared by every engine of the process on this device (HIP spreads a process's streams over four
        # hardware queues: 3.84 instead of 3.33 ms per step with three predictors' private streams).
        pool = _device_streams(device)
        # Detached training (CLSLAM_DETACHED_TRAINING=0: off, bitwise the same, tests/test_detached_training.py): a training
        # adapt() runs on the engine's own stream; the caller's stream is ordered behind the forward and the first three launches
        # of the backward only (`inputs_released`), so its read-backs return while the rest of the step keeps the GPU busy.
        # Whatever touches trainable state or the workspace afterwards goes through wait_training().  DESIGN.md "Round 4".
        self.main_stream = pool.get('main')
        self.detached_training = os.environ.get('CLSLAM_DETACHED_TRAINING', '1') != '0'
        self._train_done = None       # event: the last detached training step (incl. its optimizer step) has completed
        self._caller = None           # the caller's stream while a detached call is being enqueued
        self.inputs_released = None
        self._prealloc = None         # output planes allocated by the caller's stream for the call's last forward (prealloc_outputs)
        self._prealloc_armed = False
        # The pose net runs on `side_stream` beside the depth net (they are independent until the loss stage, and again in the
        # backward); `wg_stream` takes the leaves of both passes: identity maps, disparity heads, weight gradients.
        # CLSLAM_SIDE_STREAM=0: everything on one stream.  DESIGN.md "Schedule (host side)".
        self.use_side_stream = os.environ.get('CLSLAM_SIDE_STREAM', '1') != '0'
        self.side_stream = pool.get('side')
        self.wg_stream = pool.get('wg')
        # split-K scratch of the small-M 3x3 convs: one zero-filled buffer per stream convs are launched on
        self._conv_ws: Dict[int, torch.Tensor] = pool.setdefault('conv_ws', {}) if pool else {}
        for st in (self.main_stream, self.side_stream, self.wg_stream):
            if st is not None:
                self._conv_workspace(st.cuda_stream)
        # Asynchronous tail (data-parallel mode): gradient reduction + all-reduce + Adam of step N run on `tail_stream` and the
        # caller's stream does not wait for them, so the frozen encoders of step N+1 overlap the xGMI all-reduce.  Whatever
        # reads trainable state waits on the event (wait_training()).
        self.async_tail = False
        self.data_parallel = False    # set by DepthPosePrediction.enable_data_parallel: an all-reduce sits between reduction and Adam
        self.tail_stream = pool.get('tail')
        self._tail_event = None       # optimizer step in flight on tail_stream
        self._tail_open = False       # backward() left its reduction on tail_stream; adam() closes it
        # Descriptor memo: slam.py:143-147 runs models['depth_encoder'](online_image) on every frame right
        # before adapt(), whose depth-encoder pass over the (un-augmented) online sample repeats it.  run_encoder() keeps its input
        # and features; a single-triplet forward whose network input has the same CONTENT takes them instead of 22 launches.
        self.descriptor_memo = os.environ.get('CLSLAM_DESCRIPTOR_MEMO', '1') != '0'
        self._memo = None
        self.memo_hits = 0
        # Data-parallel gradient exchange in buckets (DESIGN.md section 6 "Round 4"): the arena is cut into
        # contiguous ranges in the order their gradients complete in the backward (bucket_ranges()); each is reduced and
        # all-reduced on the tail stream as soon as its last weight-gradient kernel is enqueued, Adam follows once.  The sequence
        # of collectives is the same on every rank whatever its workspace / overlap state.
        self.grad_buckets = int(os.environ.get('CLSLAM_GRAD_BUCKETS', '3'))
        self.grads_synced = False
        self.time_exchange = False    # bench.py --gpus N: time the bucket all-reduces (exchange_report())
        self.exchange_events: List[Any] = []
        self.exchange_main_done = None
        # tie-break noise drawn in the loss kernel (Philox): keyed by the seed of torch's generator of this device, re-read on
        # every forward -- torch.manual_seed() after construction re-keys the stream and restarts its draw counter, like the
        # global generator the reference draws from (dpp.py:1055-1056).  noise_stream = the data-parallel shard offset: ranks
        # seeded identically still draw different fields for their different samples.
        self._noise_torch_seed = None
        self.noise_seed = 1
        self.noise_draws = 0
        self.noise_stream = 0
        # A side stream is released behind ONE launch of the dependency chain by that launch's own completion signal (+1.3 us on
        # the producer) instead of an event recorded behind it (+5.0 us, ~17 hand-offs per step: tools/micro/event_gap.hip,
        # profiles/r05_micro_calibration.txt).  ops.PROFILE runs still record events.
        self._handoff = ops.Handoff() if device.type == 'cuda' else None
        self._cu_enc = self._cu_dec = self._cu_pose = self._cu_depth = 0     # cu_limit() per forward(); the stand-alone callables (run_encoder, ...) take the whole chip
        self.device_cus = (torch.cuda.get_device_properties(device).multi_processor_count if device.type == 'cuda' else 256)
        # steps 2..S of adapt(steps=S) keep the frozen encoders' features (see forward)
        self.reuse_frozen_features = os.environ.get('CLSLAM_REUSE_FROZEN', '1') != '0'
        # Winograd F(2x2,3x3) for the frozen encoders' 3x3 stride-1 convolutions (CLSLAM_NO_WINOGRAD=1: the direct kernels)
        self.winograd = not os.environ.get('CLSLAM_NO_WINOGRAD')

    # ------------------------------------------------------------------------------------------
    # parameters
    def bind(self, models: Dict[str, torch.nn.Module]) -> None:
        self.models = models
        for name, m in models.items():
            m._bind(self, name)

    def _module_version(self) -> int:
        """cheap fingerprint of the module parameters/buffers (in-place edits bump ``_version``;
        load_state_dict copies in place, so the tensor objects themselves are stable)"""
        if self._tracked is None:
            self._tracked = [t for m in self.models.values() for t in torch.nn.Module.state_dict(m, keep_vars=True).values()]
        return sum(t._version for t in self._tracked)

    def pack_if_needed(self) -> None:
        """Re-layout the module parameters into the engine's buffers when they were modified from
        outside (load_model, load_state_dict, manual edits)."""
        ver = self._module_version()
        if ver != self._packed_version:
            if self._modules_stale:
                raise ClslamError('module parameters were modified while newer adapted weights live in the engine; '
                                  'call sync_modules() first')
            self.pack()

    def _on(self, st):
        """context: the launches of the block go to stream `st`.  This is ops.launch_on (no change of torch's current stream,
        0.3 us instead of 6): the blocks it wraps contain launches of clslam_hip.ops only."""
        if st is None:
            return contextlib.nullcontext()
        return ops.launch_on(st)

    def _use_tail(self) -> bool:
        return self.async_tail and self.tail_stream is not None and self.device.type == 'cuda' and ops.PROFILE is None

    def _side_streams(self):
        """(side, wg): the pose branch's and the wgrad stream; None each when use_side_stream is off or there is none"""
        return (self.side_stream, self.wg_stream) if self.use_side_stream else (None, None)

    def cu_limit(self, B: int, phase: str = 'encoders') -> int:
        """clslam_conv_desc.cu_limit of the persistent (stream-K / Winograd) conv launches of a phase (0: the whole chip).  A
        persistent launch that takes every CU shuts the other stream out for its whole duration; on disjoint shares the two
        frozen encoders run side by side.  Measured at 192x640 (profiles/r05_cu_limit_sweep.txt): 3 / 5 / 9 triplets -2.7 / -2.9 /
        -1.8 % per step, 1 triplet +4 % (latency counts, not occupancy), 33 triplets +3.7 % (every launch fills the chip alone)
        -- hence the band 2 <= B <= 16.  DESIGN.md "`cu_limit` by section".
        phase: 'enc_pose' / 'enc_depth' (5/8 and 3/8 of the chip), 'decoders', 'backward' (the whole chip: in steps 2..S of
        adapt(steps=S) nothing runs beside the depth decoder's launches -- and the decoders' summation order must not depend
        on whether the encoders ran, tests/test_frozen_reuse.py holds the reuse bitwise invisible)"""
        if not phase.startswith('enc'):
            return 0
        if not (self.use_side_stream and 2 <= B <= 16):
            return 0
        # The pose encoder sees 2B images, the depth encoder B (and the depth decoder follows it on the same stream): 5/8 : 3/8 of
        # the chip instead of half each.  Measured at K = 4 (round 6, MI355X): pose / depth = 128/128 2.904, 144/112 2.871,
        # 160/96 2.863, 176/80 2.909, 192/64 3.002, 112/144 3.007 ms per step; whole chip each 3.027.
        if phase == 'enc_pose':
            return self.device_cus * 5 // 8
        if phase == 'enc_depth':
            return self.device_cus * 3 // 8
        return self.device_cus // 2

    def wait_training(self, stream=None) -> None:
        """Make `stream` (default: the current one) wait for the training step in flight: the optimizer step on the tail
        stream (data-parallel mode) and / or the detached backward + optimizer step on the engine's own stream."""
        if self._tail_event is not None:
            (stream or torch.cuda.current_stream(self.device)).wait_event(self._tail_event)
        if self._train_done is not None:
            (stream or torch.cuda.current_stream(self.device)).wait_event(self._train_done)

    # the arenas for outside readers (tests, tools, checkpointing, the asynchronous mode's snapshots): ordered behind the step
    @property
    def w(self) -> torch.Tensor:
        self.wait_training()
        return self._w

    @property
    def g(self) -> torch.Tensor:
        self.wait_training()
        return self._g

    @property
    def m(self) -> torch.Tensor:
        self.wait_training()
        return self._m

    @property
    def v(self) -> torch.Tensor:
        self.wait_training()
        return self._v

    def prealloc_outputs(self, B: int) -> None:
        """Called on the CALLER's stream right before a detached training call: the output planes of the call's last forward,
        allocated from the caller's pool.  The engine's stream writes them (it is ordered behind the caller at
        begin_detached()), the caller reads them behind `inputs_released` -- after which nothing on the engine's streams
        touches them any more (backward(): the loss backward's three launches are the last readers) -- and frees them."""
        H, W = self.H, self.W
        E = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        self._prealloc = (B, ([E(B, H >> s, W >> s) for s in range(4)], E(2 * B, 12), E(2, B, 4, 4), E(4, B, H, W),
                              E(4, 2, B, 3, H, W), E(18)))

    def detached_ok(self) -> bool:
        """A training adapt() may run on the engine's own stream (see __init__)."""
        return (self.detached_training and self.main_stream is not None and self.device.type == 'cuda'
                and ops.PROFILE is None)

    def begin_detached(self):
        """-> (caller's stream, engine stream): the engine stream is ordered behind everything the caller has enqueued (its
        inputs) and becomes torch's current stream for the enqueueing that follows (`with torch.cuda.stream(em)`)."""
        cur = torch.cuda.current_stream(self.device)
        em = self.main_stream
        if cur.cuda_stream == em.cuda_stream:      # nested / already there
            return cur, None
        em.wait_stream(cur)
        self._caller = cur
        return cur, em

    def end_detached(self, cur, released, failed: bool = False) -> None:
        """The caller's stream continues behind `released` (backward(): the last read of the caller's minibatch, ~0.1 ms into
        the backward); everything that touches trainable state or the workspace waits through wait_training()."""
        self._caller = None
        self._prealloc, self._prealloc_armed = None, False
        ev = torch.cuda.Event()
        ev.record(self.main_stream)
        self._train_done = ev
        cur.wait_event(ev if (failed or released is None) else released)

    def training_stream(self):
        """Context manager: the stream the gradient all-reduce of the step in flight belongs on."""
        return torch.cuda.stream(self.tail_stream) if self._tail_open else contextlib.nullcontext()

    @torch.no_grad()
    def pack(self) -> None:
        dev = self.device
        self.wait_training()
        for which in ('depth_encoder', 'pose_encoder'):
            sd = {k: v.detach().to(dev, torch.float32) for k, v in torch.nn.Module.state_dict(self.models[which]).items()}
            e = SimpleNamespace()

            def bn(prefix):
                scale = sd[prefix + '.weight'] / torch.sqrt(sd[prefix + '.running_var'] + BN_EPS)
                shift = sd[prefix + '.bias'] - sd[prefix + '.running_mean'] * scale
                return scale.contiguous(), shift.contiguous()

            def conv(key):
                wt = sd[key]
                return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], wt.shape[2] * wt.shape[3], wt.shape[1]).contiguous()

            e.stem_w = ops.stem_pack_weight(sd['resnet.conv1.weight'].contiguous())
            e.stem_scale, e.stem_shift = bn('resnet.bn1')
            e.blocks = []
            for li, (cin, cout, stride) in enumerate(((64, 64, 1), (64, 128, 2), (128, 256, 2), (256, 512, 2)), start=1):
                for bi in range(2):
                    p = f'resnet.layer{li}.{bi}'
                    blk = SimpleNamespace(stride=stride if bi == 0 else 1, cin=cin if bi == 0 else cout, cout=cout)
                    blk.w1 = conv(p + '.conv1.weight'); blk.s1, blk.b1 = bn(p + '.bn1')
                    blk.w2 = conv(p + '.conv2.weight'); blk.s2, blk.b2 = bn(p + '.bn2')
                    # frozen 3x3 stride-1 filters, transformed ONCE per load for the Winograd F(2x2,3x3) kernel (conv_wino.hip:
                    # U = G g G^T in double, rounded once); clslam_conv2d picks the kernel per layer shape
                    blk.u1 = ops.wino_weight_transform(blk.w1) if (blk.stride == 1 and self.winograd) else None
                    blk.u2 = ops.wino_weight_transform(blk.w2) if self.winograd else None
                    blk.wd = None
                    if (p + '.downsample.0.weight') in sd:
                        blk.wd = conv(p + '.downsample.0.weight'); blk.sd, blk.bd = bn(p + '.downsample.1')
                    e.blocks.append(blk)
            self.enc[which] = e
        for name, off, shape in self.layout.entries:
            model, key = name.split('/', 1)
            t = torch.nn.Module.state_dict(self.models[model])[key].detach().to(dev, torch.float32)
            flat = TrainableLayout.to_compute(t)
            self._w[off:off + flat.numel()].copy_(flat)
        self._packed_version = self._module_version()
        self._modules_stale = False
        self._desc_cache.clear()               # re-laid-out weights / BN vectors: the kept descriptors point at the old ones
        for ws in self._ws.values():           # features of the previous encoder weights are void
            if hasattr(ws, 'frozen_valid'):
                ws.frozen_valid = False
        self._memo = None

    @torch.no_grad()
    def sync_modules(self) -> None:
        """Write the engine's adapted weights back into the module parameters (reference layout)."""
        if not self._modules_stale or self.models is None:
            return
        self.wait_training()
        for name, off, shape in self.layout.entries:
            model, key = name.split('/', 1)
            p = torch.nn.Module.state_dict(self.models[model], keep_vars=True)[key]
            p.data.copy_(TrainableLayout.to_reference(self._w[off:off + math.prod(shape)], shape))
        self._modules_stale = False
        self._packed_version = self._module_version()

    @torch.no_grad()
    def install_weights(self, flat: torch.Tensor, adam_step_count: Optional[int] = None) -> None:
        """Replace the whole trainable arena (compute layout, `layout.size` floats) -- the receiving side of a weight
        broadcast (clslam_hip.async_mode).  Module parameters are re-materialised lazily like after an optimizer step."""
        self.pack_if_needed()
        self.wait_training()
        self._w.copy_(flat.reshape(-1)[:self.layout.size])
        if adam_step_count is not None:
            self.adam_step_count = int(adam_step_count)
        self._modules_stale = True

    def wview(self, name: str) -> torch.Tensor:
        self.wait_training()
        for n, off, shape in self.layout.entries:
            if n == name:
                return self._w[off:off + math.prod(shape)]
        raise KeyError(name)

    def _slot(self, buf: torch.Tensor, name: str, numel: int) -> torch.Tensor:
        off = self.layout.offset[name]
        return buf[off:off + numel]

    # ------------------------------------------------------------------------------------------
    # workspace
    def workspace(self, B: int) -> SimpleNamespace:
        ws = self._ws.get(B)
        if ws is not None:
            return ws
        dev, H, W = self.device, self.H, self.W
        E = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        ws = SimpleNamespace(B=B)
        ws.denc = self._enc_bufs(B)
        ws.penc = self._enc_bufs(2 * B)
        self._depth_dec_bufs(B, ws)
        self._pose_dec_bufs(2 * B, ws)
        # loss stage
        ws.T = E(2, B, 4, 4)
        ws.P = E(2, B, 3, 4)
        ws.depth = E(4, B, H, W)
        ws.warped = E(4, 2, B, 3, H, W)
        ws.idmap = E(2, B, H, W)
        ws.coef = None  # allocated on the first training step
        ws.sel = torch.empty(4, B, H, W, dtype=torch.uint8, device=dev)
        ws.nblk = ops.automask_blocks(H, W)
        ws.partial = E(4, B, ws.nblk)
        ws.means = E(4, B, ops.disp_mean_chunks())
        ws.losses = E(18)
        ws.noise = E(4, B, 2, H, W)
        ws.train = None
        self._ws[B] = ws
        return ws

    def _enc_bufs(self, n: int) -> SimpleNamespace:
        dev, H, W = self.device, self.H, self.W
        E = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        hs = [H >> k for k in range(6)]
        wsz = [W >> k for k in range(6)]
        e = SimpleNamespace()
        e.f0 = E(n, hs[1], wsz[1], 64)
        e.pool = E(n, hs[2], wsz[2], 64)
        e.t = [E(n, hs[2 + li], wsz[2 + li], c) for li, c in enumerate((64, 128, 256, 512))]
        e.ds = [None] + [E(n, hs[2 + li], wsz[2 + li], c) for li, c in ((1, 128), (2, 256), (3, 512))]
        e.y = [[E(n, hs[2 + li], wsz[2 + li], c) for _ in range(2)] for li, c in enumerate((64, 128, 256, 512))]
        return e

    def _depth_dec_bufs(self, n: int, st: Optional[SimpleNamespace] = None) -> SimpleNamespace:
        """depth-decoder activations of n images on `st`: x[i, j] = output of upconv_i_j (post-ELU, NHWC), disp[s]"""
        st = SimpleNamespace() if st is None else st
        H, W = self.H, self.W
        E = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        st.x = {}
        for i in range(4, -1, -1):
            st.x[i, 0] = E(n, H >> (i + 1), W >> (i + 1), NUM_CH_DEC[i])
            st.x[i, 1] = E(n, H >> i, W >> i, NUM_CH_DEC[i])
        st.disp = [E(n, H >> s, W >> s) for s in range(4)]
        return st

    def _pose_dec_bufs(self, n: int, st: Optional[SimpleNamespace] = None) -> SimpleNamespace:
        """pose-decoder activations of n images (2B inside a step) on `st`"""
        st = SimpleNamespace() if st is None else st
        h5, w5 = self.H >> 5, self.W >> 5
        E = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        st.sq, st.p0, st.p1 = E(n, h5, w5, 256), E(n, h5, w5, 256), E(n, h5, w5, 256)
        st.pmean, st.pose = E(n, 256), E(n, 12)
        return st

    def _train_bufs(self, ws: SimpleNamespace) -> SimpleNamespace:
        if ws.train is not None:
            return ws.train
        dev, H, W, B = self.device, self.H, self.W, ws.B
        E = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        t = SimpleNamespace()
        ws.coef = E(4, B, 9, H, W)       # SSIM coefficients of the selected frame per pixel
        t.ddisp_up = E(4, B, H, W)
        t.nb2 = ops.loss_bwd2_blocks(H, W)
        t.dp_partial = torch.empty(4, B, t.nb2, 24, dtype=torch.float64, device=dev)   # block sums of dL/dP, in double
        t.dz_disp = [torch.empty(B, H >> s, W >> s, device=dev) for s in range(4)]
        t.dpose = E(2 * B, 12)
        t.dz = {k: torch.empty_like(v) for k, v in ws.x.items()}   # d(pre-ELU) of every upconv output
        pad_elems = max(B * ((H >> i) + 2) * ((W >> i) + 2) * NUM_CH_DEC[i] for i in range(5))
        t.dxp = [E(pad_elems), E(pad_elems)]
        t.wt_ready = None
        t.wt_dec = {}   # (i, j) -> flipped/transposed upconv_i_j weight for the dgrad convs (refreshed every backward)
        t.wt_pose = {}  # 0 / 1 -> the same for pose_decoder pose_0 / pose_1
        t.wt_table = None
        t.dz_p1 = torch.empty_like(ws.p1)
        t.dz_p0 = torch.empty_like(ws.p0)
        t.dz_sq = torch.empty_like(ws.sq)
        t.plan, t.items, t.table, t.disp_part = {}, [], None, {}
        t.side = SimpleNamespace()
        # fused bias-grad partials per layer: one row per fold workgroup (pooled folds run at the resolution of x)
        t.bias_part = {k: E(ops.fold_blocks(v.shape[0], v.shape[1], v.shape[2], v.shape[3], False) * v.shape[-1])
                       for k, v in ws.x.items()}
        ws.train = t
        return t

    # ------------------------------------------------------------------------------------------
    # forward pieces
    CONV_WS_BYTES = 32 << 20

    def _conv_workspace(self, handle: Optional[int] = None) -> None:
        """Make sure the stream `handle` (default: the current stream) has its split-K scratch registered."""
        if self.device.type != 'cuda' and handle is None:
            handle = 0
        if handle is None:
            handle = torch.cuda.current_stream(self.device).cuda_stream
        if handle not in self._conv_ws:
            self._conv_ws[handle] = torch.zeros(self.CONV_WS_BYTES, dtype=torch.uint8, device=self.device)
            ops.set_conv_workspace(handle, self._conv_ws[handle])

    def _encoder(self, e, bufs, n: int, stem_inputs, waits=None, stream=None, aux=None, cu_limit=None) -> List[torch.Tensor]:
        """stem_inputs: list of (img_a, img_b|None, batch offset, count); returns the 5 NHWC features.
        waits: one event per stem launch (its input image still crossing PCIe) for the current stream to wait on.
        aux: a second stream for the three 1x1 stride-2 `downsample` convolutions of the stage entries.  They read the same
        input as the stage's first 3x3 convolution and nothing depends on them until its second one, but at 0.16-0.3 GF
        they are pure launch latency (~11 us each for ~1 us of MFMA work): on `aux` they run underneath conv1 instead of
        between conv1 and conv2 of the chain.  `stream`: the stream this encoder's launches go to (needed with aux)."""
        ops.PERSISTENT_CU_LIMIT = self._cu_enc if cu_limit is None else cu_limit
        ek = (id(self), 'enc', id(e), id(bufs), n)       # descriptor-cache key prefix of this encoder on these buffers
        for i, (img_a, img_b, off, cnt) in enumerate(stem_inputs):
            if waits is not None:
                (stream or torch.cuda.current_stream(self.device)).wait_event(waits[i])
            ops.stem_conv(img_a, img_b, e.stem_w, e.stem_scale, e.stem_shift, bufs.f0[off:off + cnt])
        ops.maxpool3x3s2(bufs.f0, bufs.pool)
        x = bufs.pool
        feats = [bufs.f0]
        for li in range(4):
            for bi in range(2):
                blk = e.blocks[li * 2 + bi]
                t, y = bufs.t[li], bufs.y[li][bi]
                res, joined = x, None
                if blk.wd is not None:
                    res = bufs.ds[li]
                    if aux is not None and stream is not None:
                        evs = bufs.__dict__.setdefault('ds_events', {})
                        fork, joined = evs.get(li) or evs.setdefault(li, (torch.cuda.Event(), torch.cuda.Event()))
                        fork.record(stream)                 # x is complete on the chain's stream
                        aux.wait_event(fork)
                        with self._on(aux):
                            ops.conv2d(x, blk.wd, res, scale=blk.sd, shift=blk.bd, ksize=1, stride=blk.stride, pad=0, act=ACT_NONE,
                                       cache=self._desc_cache, key=(ek, li, bi, 'd'))
                        joined.record(aux)
                ops.conv2d(x, blk.w1, t, scale=blk.s1, shift=blk.b1, ksize=3, stride=blk.stride, act=ACT_RELU, weight_wino=blk.u1,
                           cache=self._desc_cache, key=(ek, li, bi, 1))
                if blk.wd is not None and joined is None:
                    ops.conv2d(x, blk.wd, res, scale=blk.sd, shift=blk.bd, ksize=1, stride=blk.stride, pad=0, act=ACT_NONE,
                               cache=self._desc_cache, key=(ek, li, bi, 'd'))
                if joined is not None:
                    stream.wait_event(joined)
                ops.conv2d(t, blk.w2, y, scale=blk.s2, shift=blk.b2, residual=res, ksize=3, act=ACT_RELU, weight_wino=blk.u2,
                           cache=self._desc_cache, key=(ek, li, bi, 2))
                x = y
            feats.append(x)
        return feats

    def _wb(self, prefix: str, cout: int, cin: int, taps: int):
        # views of the flat weight arena (allocated once, packed in place): built once per layer, ~70 lookups per step
        hit = self._wb_cache.get(prefix)
        if hit is None:
            w = self._slot(self._w, prefix + '.weight', cout * taps * cin).view(cout, taps, cin)
            b = self._slot(self._w, prefix + '.bias', cout)
            hit = self._wb_cache[prefix] = (w, b)
        return hit

    def _depth_decoder(self, ws, feats: List[torch.Tensor]) -> None:
        x = feats[4]
        ops.PERSISTENT_CU_LIMIT = self._cu_dec
        # the disparity heads of scales 3..1 are leaves of the chain (only the view synthesis reads them): they go to
        # the wgrad stream, idle during the forward, instead of sitting between two convolutions of the chain
        main = self._main
        leaf = self._side_streams()[1] if main is not None else None
        forked = False
        for i in range(4, -1, -1):
            cin0 = NUM_CH_ENC[-1] if i == 4 else NUM_CH_DEC[i + 1]
            w, b = self._wb(f'depth_decoder/upconv_{i}_0.conv.conv', NUM_CH_DEC[i], cin0, 9)
            ops.conv2d(x, w, ws.x[i, 0], shift=b, ksize=3, pad_mode=PAD_REFLECT, act=ACT_ELU, cache=self._desc_cache, key=(id(self), 'dec', id(ws), i, 0))
            skip = feats[i - 1] if i > 0 else None
            cin1 = NUM_CH_DEC[i] + (NUM_CH_ENC[i - 1] if i > 0 else 0)
            w, b = self._wb(f'depth_decoder/upconv_{i}_1.conv.conv', NUM_CH_DEC[i], cin1, 9)
            fork = leaf is not None and 0 < i <= 3
            ho = self._handoff if (fork and ops.PROFILE is None) else None
            if ho is not None:
                ho.arm()          # the leaf stream is released by this convolution's own completion signal
            ops.conv2d(ws.x[i, 0], w, ws.x[i, 1], src_b=skip, shift=b, ksize=3, pad_mode=PAD_REFLECT, upsample_a=True,
                       act=ACT_ELU, cache=self._desc_cache, key=None if skip is None else (id(self), 'dec', id(ws), i, 1, skip.data_ptr()))
            x = ws.x[i, 1]
            if i <= 3:
                w, b = self._wb(f'depth_decoder/dispconv_{i}.conv', 1, NUM_CH_DEC[i], 9)
                if fork:
                    if ho is not None:
                        ho.release(main, leaf)
                    else:
                        ev = torch.cuda.Event()
                        ev.record(main)
                        leaf.wait_event(ev)
                    with self._on(leaf):
                        ops.dispconv_fwd(x, w.view(9, NUM_CH_DEC[i]), b, ws.disp[i])
                    forked = True
                else:
                    ops.dispconv_fwd(x, w.view(9, NUM_CH_DEC[i]), b, ws.disp[i])
        if forked:
            main.wait_stream(leaf)

    def _pose_decoder(self, ws, f4: torch.Tensor) -> None:
        ops.PERSISTENT_CU_LIMIT = self._cu_dec
        w, b = self._wb('pose_decoder/squeeze', 256, 512, 1)
        ops.conv2d(f4, w, ws.sq, shift=b, ksize=1, pad=0, act=ACT_RELU, cache=self._desc_cache, key=(id(self), 'pdec', id(ws), 0))
        w, b = self._wb('pose_decoder/pose_0', 256, 256, 9)
        ops.conv2d(ws.sq, w, ws.p0, shift=b, ksize=3, act=ACT_RELU, cache=self._desc_cache, key=(id(self), 'pdec', id(ws), 1))
        w, b = self._wb('pose_decoder/pose_1', 256, 256, 9)
        ops.conv2d(ws.p0, w, ws.p1, shift=b, ksize=3, act=ACT_RELU, cache=self._desc_cache, key=(id(self), 'pdec', id(ws), 2))
        w, b = self._wb('pose_decoder/pose_2', 12, 256, 1)
        ops.pose_head_fwd(ws.p1, w.view(12, 256), b, ws.pmean, ws.pose)

    # ------------------------------------------------------------------------------------------
    def forward(self, inputs: Dict[Any, torch.Tensor], *, train: bool, sample_w: torch.Tensor,
                smooth_w: Optional[torch.Tensor], noise: Optional[Dict[int, torch.Tensor]] = None,
                reuse_frozen: bool = False, inputs_ready=None) -> Tuple[Dict[Any, torch.Tensor], torch.Tensor]:
        """One _process_batch (dpp.py:906-923).  `inputs` tensors must already live on the device.

        reuse_frozen: the caller guarantees that `inputs` are the tensors of the previous forward of this
        batch size (steps 2..S of one adapt(steps=S) call, dpp.py:309-313).  Both encoders are frozen and in
        eval mode there (dpp.py:308), so their features and the identity-reprojection maps are bit-for-bit
        what the previous step computed: they are kept instead of recomputed (54 % of a step's forward
        flops).  Ignored when no valid features are held."""
        # the caller's stream, looked up ONCE per call (torch.cuda.current_stream() costs 3 us; it was asked 30x per step)
        self._main = torch.cuda.current_stream(self.device) if self.device.type == 'cuda' else None
        self._conv_workspace(None if self._main is None else self._main.cuda_stream)
        if self._train_done is not None and self._main.cuda_stream != self.main_stream.cuda_stream:
            # a forward on the caller's stream (predict(), adapt(online, None)) after a detached training step: the encoders
            # below overwrite workspace the backward in flight still reads
            self._main.wait_event(self._train_done)
        # what the stages share: the call's arguments, the converted frames, and what the schedule leaves for the loss stage
        c = SimpleNamespace(inputs=inputs, inputs_ready=inputs_ready, train=train, noise=noise, have_noise=False,
                            id_ready=None)
        self._convert_inputs(c)
        B = c.B
        self._cu_enc, self._cu_dec = self.cu_limit(B, 'encoders'), self.cu_limit(B, 'decoders')
        self._cu_pose, self._cu_depth = self.cu_limit(B, 'enc_pose'), self.cu_limit(B, 'enc_depth')
        ops.PERSISTENT_CU_LIMIT = self._cu_dec
        ws = self.workspace(B)
        c.reuse = bool(reuse_frozen and self.reuse_frozen_features and getattr(ws, 'frozen_valid', False))
        ws.frozen_valid = False
        c.memo_feats = self._memo_lookup(c.aug[0]) if (B == 1 and not c.reuse) else None
        if train:
            self._train_bufs(ws)
        self._fresh_output_planes(ws, B)
        self._networks(ws, c)
        self._loss_stage(ws, c, sample_w, smooth_w)
        ws.frozen_valid = True      # encoder features + identity maps of THESE inputs and encoder weights are held
        return self._outputs(ws, B), ws.losses

    def _convert_inputs(self, c) -> None:
        """c.aug / c.rgb: the three frames as contiguous fp32, c.B; the kernels index with the engine's resolution, so
        anything else is refused up front."""
        inputs, H, W = c.inputs, self.H, self.W
        if c.inputs_ready is not None:
            # inputs still crossing PCIe on the caller's copy stream: events (rgb_aug[0], rgb_aug[-1], rgb_aug[+1], everything
            # there).  The depth net only reads rgb_aug[0], the pose net the three rgb_aug frames; the un-augmented
            # frames are first needed by the identity maps / the loss stage.
            # _img() converts non-fp32 / non-contiguous images with a torch kernel on the MAIN stream: that kernel must not
            # read planes still in flight on the copy stream, so a batch that needs a conversion waits for all of it
            needs_conversion = any(inputs[k, f, 0].dtype != torch.float32 or not inputs[k, f, 0].is_contiguous()
                                   for k in ('rgb_aug', 'rgb') for f in (-1, 0, 1))
            self._main.wait_event(c.inputs_ready[3 if needs_conversion else 0])
        c.aug = {f: self._img(inputs['rgb_aug', f, 0]) for f in (-1, 0, 1)}
        c.rgb = {f: self._img(inputs['rgb', f, 0]) for f in (-1, 0, 1)}
        B = c.B = c.aug[0].shape[0]
        for name, group in (('rgb_aug', c.aug), ('rgb', c.rgb)):
            for f, t in group.items():
                if tuple(t.shape) != (B, 3, H, W):
                    raise ClslamError(f"('{name}', {f}, 0) must be ({B}, 3, {H}, {W}), got {tuple(t.shape)}")
        for s in range(1, 4):
            t = inputs['rgb', 0, s]
            if tuple(t.shape) != (B, 3, H >> s, W >> s):
                raise ClslamError(f"('rgb', 0, {s}) must be ({B}, 3, {H >> s}, {W >> s}), got {tuple(t.shape)}")
        for k in (('camera_matrix', 0), ('inv_camera_matrix', 0)):
            if tuple(inputs[k].shape) != (B, 4, 4):
                raise ClslamError(f'{k} must be ({B}, 4, 4), got {tuple(inputs[k].shape)}')
        if self.mask_dynamic:
            for s in range(4):
                t = inputs['mask', 0, s]          # a missing mask is a KeyError naming the key, like dpp.py:1066 / 1081
                if t.numel() != B * (H >> s) * (W >> s):
                    raise ClslamError(f"('mask', 0, {s}) must be ({B}, 1, {H >> s}, {W >> s}), got {tuple(t.shape)}")

    def _fresh_output_planes(self, ws, B: int) -> None:
        """The reference returns fresh tensors from every call: the output planes are (cheap, cached) new allocations that
        the kernels write directly -- no copies."""
        H, W = self.H, self.W
        pre = self._prealloc if self._prealloc_armed else None
        if pre is not None and pre[0] == B:
            self._prealloc = None
            # detached step: allocated by the caller's stream (prealloc_outputs) -- the blocks belong to the pool of the
            # stream that will read and free them, so no record_stream bookkeeping is needed (it cost ~0.1 ms per step at
            # B = 1: an event per block and free, polled by every later allocation)
            ws.disp, ws.pose, ws.T, ws.depth, ws.warped, ws.losses = pre[1]
        else:
            E = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
            ws.disp = [E(B, H >> s, W >> s) for s in range(4)]
            ws.pose, ws.T = E(2 * B, 12), E(2, B, 4, 4)
            ws.depth, ws.warped, ws.losses = E(4, B, H, W), E(4, 2, B, 3, H, W), E(18)

    def _identity_and_noise(self, ws, c) -> bool:
        """Identity reprojection maps (dpp.py:1047-1052) and the tie-break noise depend on the inputs only.
        -> whether ws.noise holds this forward's noise (injected); otherwise the loss kernel draws it."""
        if not c.reuse:
            # one launch per source frame straight from the caller's planes (stacking them first cost two 7 MB copies)
            ops.photo_map(c.rgb[-1], c.rgb[0], ws.idmap[0], None, c.B, c.B, self.H, self.W)
            ops.photo_map(c.rgb[1], c.rgb[0], ws.idmap[1], None, c.B, c.B, self.H, self.W)
        if c.noise is not None:
            for s in range(4):
                ws.noise[s].copy_(c.noise[s])
            return True
        return False

    def _enqueue_identity(self, ws, c, wg) -> None:
        """_identity_and_noise() on the wgrad stream, idle during the forward; c.id_ready is recorded behind it."""
        if c.inputs_ready is not None:
            wg.wait_event(c.inputs_ready[3])
        # (injected noise is written by torch ops: they need torch's current stream switched)
        with (torch.cuda.stream(wg) if c.noise is not None else ops.launch_on(wg)):
            c.have_noise = self._identity_and_noise(ws, c)
        c.id_ready = torch.cuda.Event()
        c.id_ready.record(wg)

    def _pose_encoder(self, ws, c, **kw) -> torch.Tensor:
        """last feature of the pose pairs in temporal order (dpp.py:949-955): (-1, 0) and (0, +1), batched as 2B"""
        aug, B = c.aug, c.B
        return self._encoder(self.enc['pose_encoder'], ws.penc, 2 * B, [(aug[-1], aug[0], 0, B), (aug[0], aug[1], B, B)],
                             waits=None if c.inputs_ready is None else c.inputs_ready[1:3], cu_limit=self._cu_pose, **kw)[4]

    def _pose_branch(self, ws, c, side, ds_aux) -> torch.Tensor:
        with self._on(side):
            pf4 = ws.pf4 if c.reuse else self._pose_encoder(ws, c, stream=side, aux=ds_aux)
            self.wait_training(side)      # the (frozen) encoder above does not need the optimizer step in flight
            self._pose_decoder(ws, pf4)
        return pf4

    def _networks(self, ws, c) -> None:
        """Depth net on the caller's stream, pose net on the side stream, input-only work on the wgrad stream."""
        B, reuse, main = c.B, c.reuse, self._main
        side, wg = self._side_streams()
        # the 1x1 downsample convolutions of both encoders go to the wgrad stream (idle during the forward once the identity
        # maps are out) -- for a single triplet only, where the step is a chain of dependent 5-15 us launches (K = 0, 192x640:
        # 1.454 -> 1.403 ms per frame incl. read-back).  At B = 5 the chip is throughput-bound and the six fork/join event
        # pairs cost more than the launches they hide (3.311 -> 3.377 ms).
        ds_aux = wg if B == 1 else None
        # A host minibatch still crossing PCIe: the identity maps read the un-augmented frames, i.e. they wait for the WHOLE
        # upload -- and so would everything queued behind them on the wgrad stream.  With the downsample convolutions on that
        # stream (single triplets) the first stage entry of the depth encoder must not inherit that wait: the
        # identity maps then go out AFTER the networks' launches.
        defer_identity = wg is not None and ds_aux is not None and c.inputs_ready is not None and not reuse
        if wg is not None:
            # the wgrad stream idles during the forward: the input-only work runs there, off the critical path
            wg.wait_stream(main)
            if not defer_identity:
                self._enqueue_identity(ws, c, wg)
        if side is not None:
            side.wait_stream(main)
            if reuse:                   # no encoders to hide the host's launches behind: the long chain goes out first
                dfeats = ws.dfeats
                self.wait_training(main)
                self._depth_decoder(ws, dfeats)
                pf4 = self._pose_branch(ws, c, side, ds_aux)
            else:
                # the host enqueues ~50 launches per branch (~0.7 ms): the depth branch is the longer dependency chain
                # (encoder + decoder), so its kernels go out first
                dfeats = c.memo_feats if c.memo_feats is not None else self._encoder(
                    self.enc['depth_encoder'], ws.denc, B, [(c.aug[0], None, 0, B)], stream=main, aux=ds_aux, cu_limit=self._cu_depth)
                pf4 = self._pose_branch(ws, c, side, ds_aux)
                self.wait_training(main)
                self._depth_decoder(ws, dfeats)
            main.wait_stream(side)
        else:
            self.wait_training()
            dfeats = (ws.dfeats if reuse else c.memo_feats if c.memo_feats is not None else
                      self._encoder(self.enc['depth_encoder'], ws.denc, B, [(c.aug[0], None, 0, B)], cu_limit=self._cu_depth))
            self._depth_decoder(ws, dfeats)
            pf4 = ws.pf4 if reuse else self._pose_encoder(ws, c)
            self._pose_decoder(ws, pf4)
        ws.dfeats, ws.pf4 = dfeats, pf4
        if defer_identity:
            self._enqueue_identity(ws, c, wg)

    def _loss_stage(self, ws, c, sample_w: torch.Tensor, smooth_w: Optional[torch.Tensor]) -> None:
        """View synthesis + photometric loss of the four scales -> ws.losses; ws.ctx keeps what backward() needs."""
        inputs, rgb, B, H, W = c.inputs, c.rgb, c.B, self.H, self.W
        if c.inputs_ready is not None:
            self._main.wait_event(c.inputs_ready[3])
        K = self._mat(inputs['camera_matrix', 0])
        Kinv = self._mat(inputs['inv_camera_matrix', 0])
        ops.pose_to_proj(ws.pose, K, ws.T, ws.P)
        ops.warp_fwd_pyramid(ws.disp, rgb[-1], rgb[1], Kinv, ws.P, ws.depth, ws.warped, self.min_depth, self.max_depth)
        if c.id_ready is not None:
            self._main.wait_event(c.id_ready)
        else:
            c.have_noise = self._identity_and_noise(ws, c)
        if self.mask_dynamic:
            self._masked_loss(ws, c, sample_w, smooth_w, K, Kinv)
            return
        # all four scales in one launch; reprojection maps stay in registers, only the selected frame's
        # SSIM coefficients are kept for the backward
        if c.have_noise:
            ops.photo_automask_pyramid(ws.warped, rgb[0], ws.idmap, ws.noise, ws.sel,
                                       ws.coef if c.train else None, ws.partial, B, H, W)
        else:
            # dpp.py:1055-1056 draws randn * 1e-5 on the compute device every scale, every step: here inside the kernel
            # (Philox keyed by torch's seed, one draw offset per forward: element index = (scale, sample, pixel)) -- no noise
            # tensor is written or read
            seed, offset = self._next_noise_draw()
            ops.photo_automask_pyramid_rng(ws.warped, rgb[0], ws.idmap, seed, offset, ws.sel,
                                           ws.coef if c.train else None, ws.partial, B, H, W)
        ops.disp_mean_pyramid(ws.disp, ws.means, H, W)
        n_smooth = 0 if (smooth_w is None or self.smooth_intended) else int(smooth_w.numel())
        if n_smooth and not (n_smooth < (W >> 3) - 1):
            raise ClslamError('reference smoothness layout needs batch < width/8 - 1')
        aux = getattr(ws, 'smooth_aux', None)
        if n_smooth and (aux is None or aux.shape[1] != 2 + 2 * n_smooth):
            aux = torch.zeros(4, 2 + 2 * n_smooth, device=self.device)
            ws.smooth_aux = aux
        d0 = inputs['relative_distance', 0].to(torch.float64).reshape(-1).contiguous() if self.vel_scale > 0 else None
        d1 = inputs['relative_distance', 1].to(torch.float64).reshape(-1).contiguous() if self.vel_scale > 0 else None
        rgb0 = [self._img(inputs['rgb', 0, s]) for s in range(4)]
        ops.loss_finalize([ws.partial[s] for s in range(4)], ws.disp, rgb0, [ws.means[s] for s in range(4)], ws.pose, d0, d1,
                          sample_w, smooth_w if n_smooth else None, ws.losses, aux if n_smooth else None, B, ws.nblk, H, W,
                          n_smooth, self.smooth_scale, self.vel_scale)
        if self.smooth_intended:
            if getattr(ws, 'si_partial', None) is None:
                ws.si_partial = torch.empty(4, B, ops.smooth_intended_chunks(), device=self.device)
                ws.si_aux = torch.empty(4, B, 2, device=self.device)
            ops.smooth_intended_fwd(ws.disp, rgb0, ws.si_partial, H, W)
            ops.smooth_intended_finalize(ws.si_partial, ws.means, sample_w, ws.losses, ws.si_aux, B, H, W, self.smooth_scale)
        ws.ctx = SimpleNamespace(rgb=rgb, K=K, Kinv=Kinv, d0=d0, d1=d1, sample_w=sample_w, n_smooth=n_smooth,
                                 aux=aux if n_smooth else None, B=B, rgb0=rgb0)

    def _masked_loss(self, ws, c, sample_w: torch.Tensor, smooth_w: Optional[torch.Tensor], K, Kinv) -> None:
        """The rest of _loss_stage under mask_dynamic (dpp.py:1063-1090): masked photometric sums and static counts, the
        positions of the quirk's smoothness terms on the masked planes (or the masked per-sample smoothness), the finalize.
        Nothing is read back: N_static stays on the device (ws.mstat) for the backward."""
        inputs, rgb, B, H, W = c.inputs, c.rgb, c.B, self.H, self.W
        masks = [self._img(inputs['mask', 0, s]).reshape(B, H >> s, W >> s) for s in range(4)]
        if getattr(ws, 'mstat', None) is None:
            ws.cnt_partial = torch.zeros(B, ws.nblk, dtype=torch.int32, device=self.device)
            ws.loc = torch.full((4, 2, 2 * B), -1, dtype=torch.int32, device=self.device)
            ws.mstat = torch.zeros(2, device=self.device)
            ws.smooth_aux_m = torch.zeros(4, 2 + 2 * B, device=self.device)
        if c.have_noise:
            seed = offset = 0
        else:
            seed, offset = self._next_noise_draw()
        ops.photo_automask_pyramid_masked(ws.warped, rgb[0], ws.idmap, ws.noise if c.have_noise else None, seed, offset, masks[0],
                                          ws.sel, ws.coef if c.train else None, ws.partial, ws.cnt_partial, B, H, W)
        ops.disp_mean_pyramid(ws.disp, ws.means, H, W)
        n_smooth = 0 if (smooth_w is None or self.smooth_intended) else int(smooth_w.numel())
        if n_smooth and n_smooth != B:
            raise ClslamError(f'mask_dynamic: the masked smoothness has one term per sample, got {n_smooth} weights for {B} samples')
        if n_smooth:
            ops.smooth_locate(masks, ws.loc, H, W)
        d0 = inputs['relative_distance', 0].to(torch.float64).reshape(-1).contiguous() if self.vel_scale > 0 else None
        d1 = inputs['relative_distance', 1].to(torch.float64).reshape(-1).contiguous() if self.vel_scale > 0 else None
        rgb0 = [self._img(inputs['rgb', 0, s]) for s in range(4)]
        aux = ws.smooth_aux_m if n_smooth else None
        ops.loss_finalize_masked([ws.partial[s] for s in range(4)], ws.disp, rgb0, [ws.means[s] for s in range(4)], ws.pose, d0, d1,
                                 sample_w, smooth_w if n_smooth else None, ws.losses, aux, ws.cnt_partial,
                                 ws.loc if n_smooth else None, ws.mstat, B, ws.nblk, H, W, n_smooth, self.smooth_scale,
                                 self.vel_scale)
        if self.smooth_intended:
            if getattr(ws, 'sim_partial', None) is None:
                chunks = ops.smooth_intended_chunks()
                ws.sim_partial = torch.empty(4, B, chunks, 2, device=self.device)
                ws.sim_cnt = torch.zeros(4, B, chunks, 2, dtype=torch.int32, device=self.device)
                ws.sim_aux = torch.empty(4, B, 4, device=self.device)
            ops.smooth_intended_masked_fwd(ws.disp, rgb0, masks, ws.sim_partial, ws.sim_cnt, H, W)
            ops.smooth_intended_masked_finalize(ws.sim_partial, ws.sim_cnt, ws.means, sample_w, ws.losses, ws.sim_aux, B, H, W,
                                                self.smooth_scale)
        ws.ctx = SimpleNamespace(rgb=rgb, K=K, Kinv=Kinv, d0=d0, d1=d1, sample_w=sample_w, n_smooth=n_smooth, aux=aux, B=B,
                                 rgb0=rgb0, masks=masks)

    def _memo_lookup(self, x: torch.Tensor) -> Optional[List[torch.Tensor]]:
        """Features of the last run_encoder('depth_encoder', ...) call if `x` (1,3,H,W on the device, already complete on the
        current stream) has the same content and the encoder weights have not been re-packed since.  The comparison is one
        small kernel + a 1-byte read-back (~30 us) against the ~0.3 ms of launch-bound encoder it replaces; identity cannot
        be used -- slam.py hands the descriptor pass a device copy and adapt() a host tensor (slam.py:145, 300-309)."""
        m = self._memo
        if (m is None or not self.descriptor_memo or m.version != self._packed_version
                or m.x.shape != x.shape or m.x.device != x.device):
            return None
        # ONE look-up per descriptor pass: slam.py runs the pass (and reads its 512 numbers back, i.e. the stream is drained)
        # right before the frame's adapt() -- that is the forward that can repeat it.  The comparison reads one byte back,
        # which is a stream synchronisation: any later forward (another frame without a descriptor pass, the asynchronous
        # modes) must not pay it against a stale memo while a training step is in flight.
        self._memo = None
        if not bool(torch.equal(m.x, x)):
            return None
        self.memo_hits += 1
        return m.feats

    def _next_noise_draw(self) -> Tuple[int, int]:
        """(Philox key, draw offset) of this forward's tie-break noise.  On the GPU the draw counter IS the device generator's
        Philox offset (advanced by 4 per forward like a torch kernel drawing up to four values per thread would): manual_seed,
        get_state / set_state of torch's generator reproduce the stream exactly as they do for the reference's torch.randn."""
        if self.device.type == 'cuda':
            gen = torch.cuda.default_generators[self.device.index if self.device.index is not None else torch.cuda.current_device()]
            ts = int(gen.initial_seed())
            off = int(gen.get_offset())
            gen.set_offset(off + 4)
            self.noise_draws = off // 4 + 1
        else:           # the test emulator's CPU generator has no offset: a counter that restarts when the seed changes
            ts = int(torch.default_generator.initial_seed())
            if ts != self._noise_torch_seed:
                self.noise_draws = 0
            self.noise_draws += 1
        if ts != self._noise_torch_seed:
            self._noise_torch_seed = ts
            self.noise_seed = (ts * 0x9E3779B97F4A7C15 + 0x7F4A7C15) & 0xFFFFFFFFFFFFFFFF or 1
        return self.noise_seed, (int(self.noise_stream) << 40) | self.noise_draws

    def _img(self, t: torch.Tensor) -> torch.Tensor:
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        return t

    def _mat(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(torch.float32).contiguous()

    def _outputs(self, ws, B: int) -> Dict[Any, torch.Tensor]:
        """Output dict with the reference's keys / shapes / insertion order."""
        out: Dict[Any, torch.Tensor] = {}
        for s in (3, 2, 1, 0):
            out['disp', s] = ws.disp[s].unsqueeze(1)
        for fi, f in enumerate((-1, 1)):
            out['axis_angle', 0, f] = ws.pose[fi * B:(fi + 1) * B, 0:3].unsqueeze(1)
            out['translation', 0, f] = ws.pose[fi * B:(fi + 1) * B, 3:6].unsqueeze(1)
            out['cam_T_cam', 0, f] = ws.T[fi]
        for s in range(4):
            out['depth', s] = ws.depth[s].unsqueeze(1)
            for fi, f in enumerate((-1, 1)):
                out['rgb', f, s] = ws.warped[s, fi]
        return out

    def losses_dict(self, losses: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Loss dict with the reference's keys (dpp.py:1074-1112); 'depth_loss' aliases the total
        (SURVEY.md 0.4)."""
        d: Dict[str, torch.Tensor] = {}
        for s in range(4):
            for j, name in enumerate(LOSS_NAMES):
                d[f'{name}/scale_{s}'] = losses[s * 4 + j]
        total = losses[17:18]
        d['depth_loss'] = total
        if self.vel_scale > 0:
            d['velocity_loss'] = losses[16]
        d['loss'] = total
        return d

    # ------------------------------------------------------------------------------------------
    # backward
    def _wgrad(self, t, desc_src, out_shape, dz, name_prefix: str, cout: int, cin: int, taps: int, bias_blocks: int = 0,
               bias_partial=None, **geom) -> None:
        """Weight (+ bias) gradient partials of one conv.  Every layer owns its partial buffers; the sums
        into the gradient arena happen in ONE batched reduction at the end of backward()
        (clslam_reduce_multi).  bias_blocks > 0: bias_partial already holds that many per-block column
        sums of dz (fused into fold_act_grad)."""
        desc = ops.conv_desc(desc_src[0], out_shape, src_b=desc_src[1], ksize=3 if taps == 9 else 1, **geom)
        n = cout * taps * cin
        plan = t.plan.get(name_prefix)
        if plan is None:
            use_patch = ops.wgrad_patch_supported(desc)
            splits = (ops.wgrad_patch_splits(desc, WGRAD_TARGET_BLOCKS) if use_patch else
                      ops.wgrad_splits(desc, WGRAD_TARGET_BLOCKS))
            plan = SimpleNamespace(use_patch=use_patch, splits=splits, partial=torch.empty(splits * n, device=self.device),
                                   colsum=None, nb=0)
            t.items.append((plan.partial, self._slot(self._g, name_prefix + '.weight', n), n, splits))
            if bias_blocks:
                t.items.append((bias_partial, self._slot(self._g, name_prefix + '.bias', cout), cout, bias_blocks))
            else:
                rows = out_shape[0] * out_shape[1] * out_shape[2]
                plan.nb = ops.colsum_blocks(rows)
                plan.colsum = torch.empty(plan.nb * cout, device=self.device)
                t.items.append((plan.colsum, self._slot(self._g, name_prefix + '.bias', cout), cout, plan.nb))
            t.plan[name_prefix] = plan
        if plan.use_patch:
            ops.conv_wgrad_patch(desc, dz, plan.partial, plan.splits)
        else:
            ops.conv_wgrad(desc, dz, plan.partial, plan.splits)
        if plan.colsum is not None:
            ops.colsum(dz, plan.colsum, out_shape[0] * out_shape[1] * out_shape[2], cout)

    def bucket_ranges(self):
        """[(name, first float, end float)] of the gradient buckets in backward-COMPLETION order (contiguous in the arena)."""
        off = self.layout.offset
        a_end, c_start = off['depth_decoder/upconv_3_0.conv.conv.weight'], off['pose_decoder/squeeze.weight']
        if self.grad_buckets >= 3:
            return [('pose', c_start, self.layout.size), ('mid', a_end, c_start), ('deep', 0, a_end)]
        if self.grad_buckets == 2:
            return [('early', a_end, self.layout.size), ('deep', 0, a_end)]
        return [('all', 0, self.layout.size)]

    def exchange_report(self) -> Optional[Dict[str, Any]]:
        """After a synchronised data-parallel step with `time_exchange` set: per bucket the all-reduce's time on the tail stream
        (events around the collective: its kernels AND whatever they waited for on that stream's queue), the part of the exchange
        that was still running when the backward's own last kernel had finished (`exposed_ms`: what the optimizer step waits
        for) and the fraction hidden under the backward."""
        if not self.exchange_events or self.exchange_main_done is None:
            return None
        buckets = [{'bucket': n, 'mbytes': round(nb / 1e6, 2), 'ms': round(e0.elapsed_time(e1), 4)} for n, e0, e1, nb in self.exchange_events]
        total = sum(b['ms'] for b in buckets)
        exposed = max(0.0, self.exchange_main_done.elapsed_time(self.exchange_events[-1][2]))
        rep = {'buckets': buckets, 'allreduce_ms': round(total, 4), 'exposed_ms': round(exposed, 4),
               'overlap_fraction': round(1.0 - min(exposed, total) / total, 4) if total > 0 else None}
        self.exchange_events, self.exchange_main_done = [], None
        return rep

    def _bucket_sync(self, t, name: str, events, allreduce) -> None:
        """tail stream: wait for the bucket's producers, reduce its partials into the arena, all-reduce its slice."""
        tail = self.tail_stream
        for ev in events:
            tail.wait_event(ev)
        table, n, lo, hi = t.bucket_tables[name]
        with torch.cuda.stream(tail):
            ops.reduce_multi(table, n, self._g)
            if self.time_exchange:
                # diagnosis of a multi-GPU run (bench.py --gpus N): how long each bucket's all-reduce took on the tail stream
                # and how much of it was still running when the backward's own last kernel had finished
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(tail)
                allreduce(self._g[lo:hi])
                e1.record(tail)
                self.exchange_events.append((name, e0, e1, (hi - lo) * 4))
            else:
                allreduce(self._g[lo:hi])

    def backward(self, B: int, allreduce=None) -> None:
        """dL/d(trainable arena) for the last training forward; fills self._g (dpp.py:312).
        allreduce: data-parallel mode -- callable(slice of the gradient arena) that sum-all-reduces it over the ranks on
        torch's current stream.  With it (and grad_buckets > 1) backward() exchanges the gradients itself, bucket by bucket
        (see __init__); self.grads_synced tells the caller so."""
        ops.PERSISTENT_CU_LIMIT = self.cu_limit(B, 'backward')
        ws = self._ws[B]
        t = ws.train
        self._main = torch.cuda.current_stream(self.device) if self.device.type == 'cuda' else None
        side, wg = self._side_streams()
        self._enqueue_weight_transposes(t, wg)
        self._loss_backward(ws, t, ws.ctx)
        bucketed = allreduce is not None and self.grad_buckets > 1
        # overlapped exchange: needs the tail stream, the side / wgrad streams and the per-bucket tables of a previous backward
        overlap = (bucketed and self._use_tail() and side is not None and wg is not None
                   and getattr(t, 'bucket_tables', None) is not None)
        self.grads_synced = False
        self._decoder_backwards(ws, t, B, side, allreduce if overlap else None)
        self._reduce_tables(t)
        self._finish_gradients(t, allreduce if bucketed else None, overlap)
        self.grads_synced = bucketed

    def _enqueue_weight_transposes(self, t, wg) -> None:
        """_transpose_decoder_weights() on the wgrad stream, BEFORE the loss backward goes out on the main stream (it
        overlaps it); t.wt_ready is recorded behind it.  Without a wgrad stream: in line, no event."""
        t.wt_ready = None
        if wg is None:
            self._transpose_decoder_weights(t)
            return
        wg.wait_stream(self._main)
        with self._on(wg):
            self._transpose_decoder_weights(t)
        t.wt_ready = torch.cuda.Event()
        t.wt_ready.record(wg)

    def _loss_backward(self, ws, t, c) -> None:
        """loss -> disparity logits (t.dz_disp) and pose-decoder output (t.dpose); records `inputs_released` behind them."""
        H, W = self.H, self.W
        if self.mask_dynamic:
            # a static pixel carries 1 / (4 N_static) (ws.mstat, device-resident), a dynamic one 0; the smoothness terms sit at
            # the located positions, so the row-0 layout of disp_grad_pyramid does not apply: their gradient is added behind it
            ops.loss_bwd2_pyramid_masked(ws.disp, ws.sel, ws.coef, ws.warped, c.rgb[0], c.rgb[-1], c.rgb[1], c.Kinv, ws.P,
                                         c.masks[0], ws.mstat, t.ddisp_up, t.dp_partial, self.min_depth, self.max_depth)
            ops.disp_grad_pyramid(t.ddisp_up, ws.disp, None, 0, t.dz_disp, H, W)
            if c.n_smooth:
                ops.smooth_pos_bwd(ws.disp, c.aux, ws.loc, c.n_smooth, t.dz_disp, H, W)
            if self.smooth_intended:
                ops.smooth_intended_masked_bwd(ws.disp, c.rgb0, c.masks, ws.sim_aux, c.sample_w, t.dz_disp, H, W, self.smooth_scale)
        else:
            ops.loss_bwd2_pyramid(ws.disp, ws.sel, ws.coef, ws.warped, c.rgb[0], c.rgb[-1], c.rgb[1], c.Kinv, ws.P, c.sample_w,
                                  t.ddisp_up, t.dp_partial, self.min_depth, self.max_depth)
            ops.disp_grad_pyramid(t.ddisp_up, ws.disp, c.aux if c.n_smooth else None, c.n_smooth, t.dz_disp, H, W)
            if self.smooth_intended:
                ops.smooth_intended_bwd(ws.disp, c.rgb0, ws.si_aux, c.sample_w, t.dz_disp, H, W, self.smooth_scale)
        ops.pose_bwd(t.dp_partial, 4, t.nb2, ws.pose, c.K, c.d0, c.d1, c.sample_w, self.vel_scale, t.dpose)
        self.inputs_released = None
        if self._caller is not None:
            # detached step: nothing below reads the caller's minibatch (frames, intrinsics, distances) or the output planes
            # handed to it any more -- the three launches above were the last.  The caller's stream continues behind THIS point:
            # it may overwrite its input buffers in place or drop them at once, like after the reference's synchronous step.
            self.inputs_released = torch.cuda.Event()
            self.inputs_released.record(self._main)

    def _decoder_backwards(self, ws, t, B: int, side, exchange) -> None:
        """Pose-decoder backward on the side stream beside the depth decoder's on the main stream (no side stream: one after
        the other).  exchange: the all-reduce of an overlapped data-parallel exchange (else None) -- every bucket but the
        last goes out on the tail stream as soon as its gradients are enqueued."""
        if side is None:
            self._backward_depth_decoder(ws, t, B)
            self._backward_pose_decoder(ws, t, B, t)
            return
        main = self._main
        side.wait_stream(main)
        if t.wt_ready is not None:
            side.wait_event(t.wt_ready)     # transposed pose_0 / pose_1 weights
        with self._on(side):
            self._backward_pose_decoder(ws, t, B, t.side)
        if exchange is not None and self.grad_buckets >= 3:
            ev = torch.cuda.Event()
            ev.record(side)                 # the pose decoder's three weight gradients + pose_2's are complete behind this
            self._bucket_sync(t, 'pose', [ev], exchange)
        self._backward_depth_decoder(ws, t, B, exchange)
        main.wait_stream(side)

    def _reduce_tables(self, t) -> None:
        """Built once per workspace, after its first backward has registered every partial buffer in t.items: t.table (all
        items: one batched, deterministic reduction of every weight / bias gradient partial into the arena) and
        t.bucket_tables (the same items by gradient bucket)."""
        if t.table is not None:
            return
        # pose_2's gradients are written straight into the arena by pose_head_bwd: identity items, so that every trainable
        # element is the output of exactly one item and the table covers the whole arena
        for key, n in (('pose_decoder/pose_2.weight', 12 * 256), ('pose_decoder/pose_2.bias', 12)):
            sl = self._slot(self._g, key, n)
            t.items.append((sl, sl, n, 1))
        t.table = ops.make_reduce_table(t.items, self.device)
        # the same items grouped by the bucket their destination lies in (every item reduces independently, in a fixed
        # order: three launches give bitwise the single launch's arena)
        base = self._g.data_ptr()
        t.bucket_tables = {}
        for name, lo, hi in self.bucket_ranges():
            its = [it for it in t.items if lo <= (it[1].data_ptr() - base) // 4 < hi]
            t.bucket_tables[name] = (ops.make_reduce_table(its, self.device), len(its), lo, hi)
        assert sum(v[1] for v in t.bucket_tables.values()) == len(t.items)

    def _finish_gradients(self, t, allreduce, overlap: bool) -> None:
        """Partials -> gradient arena, then the exchange backward() owns.  allreduce: the bucketed data-parallel exchange
        (None: single GPU, or the caller all-reduces the whole arena under training_stream())."""
        ranges = self.bucket_ranges() if allreduce is not None else []
        if overlap:
            # the earlier buckets went out during the backward; the last one (level 4) is complete on the main stream now
            if self.time_exchange:
                self.exchange_main_done = torch.cuda.Event(enable_timing=True)
                self.exchange_main_done.record(self._main)
            self.tail_stream.wait_stream(self._main)
            self._bucket_sync(t, ranges[-1][0], [], allreduce)
            self._tail_open = True
        elif self._use_tail():
            # the partial buffers are complete on the current stream; the reduction, the exchange (here in the engine's buckets,
            # or the caller's under training_stream()) and Adam follow on the tail stream and nobody waits for them here
            self.tail_stream.wait_stream(self._main)
            with torch.cuda.stream(self.tail_stream):
                self._reduce_and_exchange(t, ranges, allreduce)
            self._tail_open = True
        else:
            self._reduce_and_exchange(t, ranges, allreduce)

    def _reduce_and_exchange(self, t, ranges, allreduce) -> None:
        """One reduction of the whole table, then (no overlap possible: first backward of this workspace, no tail / side
        streams, instrumented run) the SAME sequence of collectives on the same slices as the overlapped exchange."""
        ops.reduce_multi(t.table, len(t.items), self._g)
        for _name, lo, hi in ranges:
            allreduce(self._g[lo:hi])

    def _transpose_decoder_weights(self, t) -> None:
        """Flipped/transposed weights for every dgrad conv of the step (nine depth-decoder upconvs, pose_0 / pose_1).
        They depend only on the weights, so all eleven are produced by ONE launch at the start of backward() on the
        wgrad stream, where it overlaps the loss backward instead of sitting between the dgrad convs of the critical
        paths (eleven launches before: 0.06 ms of the B = 1 step)."""
        if t.wt_table is None:
            items = []
            for i in range(5):
                ci = NUM_CH_DEC[i]
                cin1 = ci + (NUM_CH_ENC[i - 1] if i > 0 else 0)
                t.wt_dec[i, 1] = torch.empty(ci, 9, ci, device=self.device)
                w1, _ = self._wb(f'depth_decoder/upconv_{i}_1.conv.conv', ci, cin1, 9)
                items.append((w1, t.wt_dec[i, 1], ci))            # only the up(x[i,0]) half: the skip half is frozen
                if i < 4:
                    cin0 = NUM_CH_DEC[i + 1]
                    t.wt_dec[i, 0] = torch.empty(cin0, 9, ci, device=self.device)
                    w0, _ = self._wb(f'depth_decoder/upconv_{i}_0.conv.conv', ci, cin0, 9)
                    items.append((w0, t.wt_dec[i, 0], None))
            for k in (0, 1):
                t.wt_pose[k] = torch.empty(256, 9, 256, device=self.device)
                wp, _ = self._wb(f'pose_decoder/pose_{k}', 256, 256, 9)
                items.append((wp, t.wt_pose[k], None))
            t.wt_table = ops.transpose_table(items)
        ops.weight_transpose_multi(t.wt_table, self._w)

    def _backward_depth_decoder(self, ws, t, B: int, exchange=None) -> None:
        """dgrad chain (critical path) on the current stream; every weight/bias gradient is independent
        of the rest of the chain once its dz exists, so those run on a third stream (`wg_stream`).
        exchange: see _decoder_backwards -- the bucket of levels 0..3 goes out behind level 3."""
        H, W = self.H, self.W
        feats = ws.dfeats
        main = self._main
        side, wg = self._side_streams()
        if wg is not None:
            wg.wait_stream(main)

        # The weight-gradient kernels add up to about as much GPU time as the dgrad chain itself and the last
        # (largest-weight) layers only become ready at the very end, so they alternate between the wgrad stream
        # and the side stream (idle once the short pose-decoder backward is through): two wgrads in flight
        # instead of a serial tail after the dgrad chain.
        wg_streams = [wg] if (wg is None or side is None) else [wg, side]
        turn = itertools.cycle(wg_streams)      # whose turn the next weight-gradient launch is
        ho = self._handoff if (wg is not None and ops.PROFILE is None) else None
        behind_launch = 'armed' if ho is not None else 'record'

        def on_wg(fn, i, dep):
            """run fn(i) on the wgrad stream whose turn it is.  dep: 'record' -- after everything enqueued so far on the main
            stream (an event recorded there); 'armed' -- after the launch that took the hand-off event armed just before it (no
            marker packet on the chain); None -- its inputs were complete before this function started (both wgrad streams are
            ordered behind the loss backward by then)"""
            if wg is None:
                fn(i)
                return
            st = next(turn)
            if dep == 'armed':
                ho.release(main, st)
            elif dep == 'record':
                ev = torch.cuda.Event()
                ev.record(main)
                st.wait_event(ev)
            with self._on(st):
                fn(i)

        def disp_wgrad(i):      # dispconv_i weight + bias gradient partials
            hi, wi, ci = H >> i, W >> i, NUM_CH_DEC[i]
            if i not in t.disp_part:
                nb = ops.dispconv_wgrad_blocks(B * hi * wi)
                t.disp_part[i] = torch.empty(nb * (9 * ci + 1), device=self.device)
                t.items.append((t.disp_part[i], self._slot(self._g, f'depth_decoder/dispconv_{i}.conv.weight', 9 * ci + 1),
                                9 * ci + 1, nb))
            ops.dispconv_wgrad(t.dz_disp[i], ws.x[i, 1], t.disp_part[i])

        def upconv1_wgrad(i):   # upconv_i_1: input = cat(up(x[i,0]), feats[i-1])
            hi, wi, ci = H >> i, W >> i, NUM_CH_DEC[i]
            skip = feats[i - 1] if i > 0 else None
            cin1 = ci + (NUM_CH_ENC[i - 1] if i > 0 else 0)
            self._wgrad(t, (ws.x[i, 0], skip), (B, hi, wi, ci), t.dz[i, 1], f'depth_decoder/upconv_{i}_1.conv.conv', ci, cin1, 9,
                        bias_blocks=ops.fold_blocks(B, hi, wi, ci, False), bias_partial=t.bias_part[i, 1],
                        pad_mode=PAD_REFLECT, upsample_a=True)

        def upconv0_wgrad(i):   # upconv_i_0: input = x[i+1,1] (or the frozen encoder feature for i == 4)
            hi, wi, ci = H >> i, W >> i, NUM_CH_DEC[i]
            src = ws.x[i + 1, 1] if i < 4 else feats[4]
            cin0 = NUM_CH_ENC[-1] if i == 4 else NUM_CH_DEC[i + 1]
            self._wgrad(t, (src, None), (B, hi >> 1, wi >> 1, ci), t.dz[i, 0], f'depth_decoder/upconv_{i}_0.conv.conv', ci, cin0, 9,
                        bias_blocks=ops.fold_blocks(B, hi, wi, ci, True), bias_partial=t.bias_part[i, 0], pad_mode=PAD_REFLECT)

        if t.wt_ready is not None:
            main.wait_event(t.wt_ready)     # transposed dgrad weights (issued at the start of backward())

        dxp_in = None  # padded-domain gradient w.r.t. x[i,1] coming from upconv_{i-1}_0
        for i in range(5):
            hi, wi, ci = H >> i, W >> i, NUM_CH_DEC[i]
            wd = None
            if i <= 3:
                # the dispconv head's data gradient is folded in by fold_act_grad below (no separate pass over dxp)
                wd, _ = self._wb(f'depth_decoder/dispconv_{i}.conv', 1, ci, 9)
                # (reads dz_disp[i] -- the loss backward -- and the forward activation x[i,1] only)
                on_wg(disp_wgrad, i, None if ho is not None else 'record')
            if ho is not None:
                ho.arm()
            ops.fold_act_grad(dxp_in, ws.x[i, 1], t.dz[i, 1], h=hi, w=wi, ch=ci, border=1, pool=False, act=ACT_ELU,
                              bias_partial=t.bias_part[i, 1], disp_dz=t.dz_disp[i] if wd is not None else None,
                              disp_w=wd.view(9, ci) if wd is not None else None)
            on_wg(upconv1_wgrad, i, behind_launch)
            dxa = t.dxp[1][:B * (hi + 2) * (wi + 2) * ci].view(B, hi + 2, wi + 2, ci)
            ops.conv2d(t.dz[i, 1], t.wt_dec[i, 1], dxa, ksize=3, pad=2, cache=self._desc_cache, key=(id(self), 'dg', id(ws), i, 1))
            if ho is not None:
                ho.arm()
            ops.fold_act_grad(dxa, ws.x[i, 0], t.dz[i, 0], h=hi, w=wi, ch=ci, border=1, pool=True, act=ACT_ELU,
                              bias_partial=t.bias_part[i, 0])
            on_wg(upconv0_wgrad, i, behind_launch)
            if i < 4:
                h2, w2, cin0 = hi >> 1, wi >> 1, NUM_CH_DEC[i + 1]
                dxp_in = t.dxp[0][:B * (h2 + 2) * (w2 + 2) * cin0].view(B, h2 + 2, w2 + 2, cin0)
                ops.conv2d(t.dz[i, 0], t.wt_dec[i, 0], dxp_in, ksize=3, pad=2, cache=self._desc_cache, key=(id(self), 'dg', id(ws), i, 0))
            if i == 3 and exchange is not None:
                # every gradient of levels 0..3 and of the four disparity heads has been enqueued: weight gradients on the
                # wgrad streams, bias partials by the folds on the main stream.  Level 4 (53 % of the arena) is still to come.
                evs = []
                for st in [main] + [x for x in wg_streams if x is not None]:
                    ev = torch.cuda.Event()
                    ev.record(st)
                    evs.append(ev)
                self._bucket_sync(t, 'mid' if self.grad_buckets >= 3 else 'early', evs, exchange)
        if wg is not None:
            main.wait_stream(wg)

    def _backward_pose_decoder(self, ws, t, B: int, scratch) -> None:
        """`scratch` supplies the partial / colsum / wt buffers (a separate set when the pose branch runs
        concurrently with the depth branch)."""
        H, W = self.H, self.W
        n2 = 2 * B
        h5, w5 = H >> 5, W >> 5
        w2_, _ = self._wb('pose_decoder/pose_2', 12, 256, 1)
        ops.pose_head_bwd(t.dpose, ws.p1, w2_.view(12, 256), ws.pmean, t.dz_p1,
                          self._slot(self._g, 'pose_decoder/pose_2.weight', 12 * 256).view(12, 256),
                          self._slot(self._g, 'pose_decoder/pose_2.bias', 12))
        self._wgrad(t, (ws.p0, None), (n2, h5, w5, 256), t.dz_p1, 'pose_decoder/pose_1', 256, 256, 9)
        # (transposed weights: _transpose_decoder_weights, issued at the start of backward())
        ops.conv2d(t.dz_p1, t.wt_pose[1], t.dz_p0, ksize=3, pad=1, actgrad_src=ws.p0, actgrad_kind=ACT_RELU,
                   cache=self._desc_cache, key=(id(self), 'pdg', id(ws), 1))
        self._wgrad(t, (ws.sq, None), (n2, h5, w5, 256), t.dz_p0, 'pose_decoder/pose_0', 256, 256, 9)
        ops.conv2d(t.dz_p0, t.wt_pose[0], t.dz_sq, ksize=3, pad=1, actgrad_src=ws.sq, actgrad_kind=ACT_RELU,
                   cache=self._desc_cache, key=(id(self), 'pdg', id(ws), 0))
        self._wgrad(t, (ws.pf4, None), (n2, h5, w5, 256), t.dz_sq, 'pose_decoder/squeeze', 256, 512, 1, pad=0)

    # ------------------------------------------------------------------------------------------
    def adam(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, guard: Optional[torch.Tensor] = None) -> None:
        """guard: the step's loss (1 element); a NaN there makes the kernel skip the update."""
        self.adam_step_count += 1
        if self._tail_open:
            if guard is not None:
                guard.record_stream(self.tail_stream)      # a fresh per-call tensor allocated on the caller's stream
            with torch.cuda.stream(self.tail_stream):
                ops.adam_step(self._w, self._g, self._m, self._v, lr, self.adam_step_count, betas[0], betas[1], eps, guard=guard)
                self._tail_event = torch.cuda.Event()
                self._tail_event.record(self.tail_stream)
            self._tail_open = False
        else:
            self.wait_training()
            ops.adam_step(self._w, self._g, self._m, self._v, lr, self.adam_step_count, betas[0], betas[1], eps, guard=guard)
            self._tail_event = None
        self._modules_stale = True

    # ------------------------------------------------------------------------------------------
    # module-level entry points (slam/slam.py:146 calls models['depth_encoder'](img)[4])
    def run_encoder(self, which: str, x: torch.Tensor) -> List[torch.Tensor]:
        """NCHW feature list of one encoder, as the reference's ResnetEncoder.forward returns it."""
        self.pack_if_needed()
        self._conv_workspace()
        self.wait_training()
        x = self._img(x.to(self.device))
        n = x.shape[0]
        nimg = 1 if which == 'depth_encoder' else 2
        if x.shape[1] != 3 * nimg or x.shape[2] != self.H or x.shape[3] != self.W:
            raise ClslamError(f'{which} input must be (N,{3 * nimg},{self.H},{self.W}), got {tuple(x.shape)}')
        key = ('enc', which, n)
        bufs = self._ws.get(key)
        if bufs is None:
            bufs = self._enc_bufs(n)
            self._ws[key] = bufs
        if nimg == 1:
            stem = [(x, None, 0, n)]
        else:
            stem = [(x[:, :3].contiguous(), x[:, 3:].contiguous(), 0, n)]
        # the share of the chip the same encoder gets inside forward() for this many images: the persistent kernels' summation
        # order (and the Winograd / direct pick) depends on it, and models['depth_encoder'](x) is bitwise what predict() computes
        # (tests/test_slam_usage.py::test_the_four_models_are_callables)
        cu = self.cu_limit(n, 'enc_depth') if nimg == 1 else self.cu_limit(max(1, n // 2), 'enc_pose')
        feats = self._encoder(self.enc[which], bufs, n, stem, cu_limit=cu)
        self._memo = None
        if which == 'depth_encoder' and n == 1 and self.descriptor_memo:
            # (a private copy of the input: the caller owns x and may overwrite it; the feature buffers belong to this
            # workspace and are only rewritten by the next call of this function, which replaces the memo)
            self._memo = SimpleNamespace(x=x.clone(), feats=feats, version=self._packed_version)
        return [f.permute(0, 3, 1, 2) for f in feats]

    def run_pose(self, image_0: torch.Tensor, image_1: torch.Tensor) -> torch.Tensor:
        """predict_pose (dpp.py:628-664): pose_encoder(cat(img0,img1)) -> pose_decoder; returns (n,12)."""
        self.pack_if_needed()
        self._conv_workspace()
        self.wait_training()
        a, b = self._img(image_0.to(self.device)), self._img(image_1.to(self.device))
        n = a.shape[0] if a.dim() == 4 else -1
        # the stem kernel takes H, W from its input but writes buffers planned for the engine's resolution
        for name, t in (('image_0', a), ('image_1', b)):
            if tuple(t.shape) != (n, 3, self.H, self.W):
                raise ClslamError(f'predict_pose: {name} must be (N, 3, {self.H}, {self.W}) with equal N, got {tuple(t.shape)}')
        key = ('pose', n)
        st = self._ws.get(key)
        if st is None:
            st = self._ws[key] = self._pose_dec_bufs(n, SimpleNamespace(penc=self._enc_bufs(n)))
        self._cu_enc = self._cu_dec = 0
        feats = self._encoder(self.enc['pose_encoder'], st.penc, n, [(a, b, 0, n)])
        self._pose_decoder(st, feats[4])
        return st.pose

    def run_pair(self, image_0: torch.Tensor, image_1: torch.Tensor, *, want_loss: bool, K: Optional[torch.Tensor] = None,
                 inv_K: Optional[torch.Tensor] = None, relative_distance: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None, sample_w: Optional[torch.Tensor] = None,
                 smooth_w: Optional[torch.Tensor] = None) -> SimpleNamespace:
        """predict_from_images (dpp.py:556-626): ONE depth-network pass over the 2N stacked frames on the caller's stream, the
        pose network over cat(image_0, image_1) on the side stream (the chip shares forward() gives the two encoders of N
        samples), then -- want_loss -- the fused scale-0 pair loss with image_1 as target and image_0 as source.
        -> disp (2N,1,H,W) (image_0's first), pose (N,12), T (2,N,4,4) = [cam_T_cam(0,-1) (inverted), the plain transformation],
        losses (7,) or None (ops.pair_loss_finalize's order).  Every returned tensor is a fresh allocation.
        noise: (N,1,H,W), already x 1e-5 (parity runs); None draws it in the kernel from the engine's draw counter."""
        self.pack_if_needed()
        self._conv_workspace()
        self.wait_training()
        a, b = self._img(image_0.to(self.device)), self._img(image_1.to(self.device))
        n = a.shape[0] if a.dim() == 4 else -1
        H, W, dev = self.H, self.W, self.device
        for name, t in (('image_0', a), ('image_1', b)):
            if tuple(t.shape) != (n, 3, H, W):
                raise ClslamError(f'predict_from_images: {name} must be (N, 3, {H}, {W}) with equal N, got {tuple(t.shape)}')
        if want_loss:
            if K is None or inv_K is None or sample_w is None:
                raise ClslamError('predict_from_images: the loss needs camera_matrix, inv_camera_matrix and sample weights')
            K, inv_K = self._mat(K.to(dev)), self._mat(inv_K.to(dev))
            for name, t in (('camera_matrix', K), ('inv_camera_matrix', inv_K)):
                if tuple(t.shape) != (n, 4, 4):
                    raise ClslamError(f'predict_from_images: {name} must be ({n}, 4, 4), got {tuple(t.shape)}')
            if noise is not None and tuple(noise.shape) != (n, 1, H, W):
                raise ClslamError(f'predict_from_images: tie-break noise must be ({n}, 1, {H}, {W}), got {tuple(noise.shape)}')
            if self.vel_scale > 0 and (relative_distance is None or relative_distance.numel() != n):
                raise ClslamError(f'predict_from_images: relative_distance must hold {n} values')
        key = ('pair', n)
        st = self._ws.get(key)
        if st is None:
            E = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
            st = SimpleNamespace(denc=self._enc_bufs(2 * n), penc=self._enc_bufs(n), dec=self._depth_dec_bufs(2 * n),
                                 pad=E(2 * n, 12), eye=torch.eye(4, device=dev).repeat(n, 1, 1), P=E(2, n, 3, 4),
                                 nblk=ops.automask_blocks(H, W), scratch=E(ops.pair_loss_scratch(n)))
            st.partial = E(n, st.nblk)
            self._pose_dec_bufs(n, st)
            self._ws[key] = st
        main = torch.cuda.current_stream(dev) if dev.type == 'cuda' else None
        side = self._side_streams()[0] if main is not None else None
        self._cu_dec = self.cu_limit(n, 'decoders')
        cu_pose, cu_depth = self.cu_limit(n, 'enc_pose'), self.cu_limit(n, 'enc_depth')

        def pose_net():
            f4 = self._encoder(self.enc['pose_encoder'], st.penc, n, [(a, b, 0, n)], cu_limit=cu_pose)[4]
            self._pose_decoder(st, f4)

        if side is not None:
            side.wait_stream(main)
            with self._on(side):
                pose_net()
        feats = self._encoder(self.enc['depth_encoder'], st.denc, 2 * n, [(a, None, 0, n), (b, None, n, n)], cu_limit=cu_depth)
        keep, self._main = self._main, None          # a plain chain on the caller's stream (run_depth_decoder)
        try:
            self._depth_decoder(st.dec, feats)
        finally:
            self._main = keep
        if side is not None:
            main.wait_stream(side)
        else:
            pose_net()
        # frame idx 0 of pose_to_proj is the inverted transform cam_T_cam(0,-1) the view synthesis needs (dpp.py:609-611), idx 1
        # the plain one predict_from_images returns (dpp.py:593-595): the same six pose numbers in both halves
        st.pad[:n].copy_(st.pose)
        st.pad[n:].copy_(st.pose)
        T = torch.empty(2, n, 4, 4, device=dev)
        ops.pose_to_proj(st.pad, K if want_loss else st.eye, T, st.P)
        out = SimpleNamespace(disp=st.dec.disp[0].unsqueeze(1).clone(), pose=st.pose.clone(), T=T, losses=None)
        if want_loss:
            disp1 = st.dec.disp[0][n:]
            if noise is not None:
                ops.pair_loss(disp1, a, b, inv_K, st.P[0], self._img(noise.to(dev)), st.partial, self.min_depth, self.max_depth)
            else:
                seed, offset = self._next_noise_draw()
                ops.pair_loss_rng(disp1, a, b, inv_K, st.P[0], seed, offset, st.partial, self.min_depth, self.max_depth)
            dist = (relative_distance.to(dev, torch.float64).reshape(-1).contiguous() if self.vel_scale > 0 else None)
            out.losses = torch.empty(7, device=dev)
            ops.pair_loss_finalize(st.partial, disp1, b, st.pose, dist, sample_w, smooth_w, self.smooth_intended, st.scratch,
                                   out.losses, self.smooth_scale, self.vel_scale)
        return out

    def _nhwc(self, f: torch.Tensor) -> torch.Tensor:
        """(N,C,h,w) feature -> NHWC fp32 storage on the device (a view when it already is one: run_encoder's outputs are)"""
        f = f.to(self.device, torch.float32)
        return f.permute(0, 2, 3, 1).contiguous()

    def run_depth_decoder(self, input_features):
        """models['depth_decoder'](features) (dpp.py:931-936 calls it on the encoder's five features; networks/depth_decoder.py:
        51-71): {('disp', s): (N,1,H>>s,W>>s)} for s = 3..0 from the CURRENT decoder weights, by the same kernels as the step's
        forward.  Inference only: no graph is recorded and nothing of a training step in flight is touched."""
        self._cu_dec = self.cu_limit(0, 'decoders')
        self.pack_if_needed()
        self._conv_workspace()
        self.wait_training()
        feats = [self._nhwc(f) for f in input_features]
        n = feats[0].shape[0]
        for k, f in enumerate(feats):
            want = (n, self.H >> (k + 1), self.W >> (k + 1), NUM_CH_ENC[k])
            if tuple(f.shape) != want:
                raise ClslamError(f'depth_decoder: feature {k} must be (N, {want[3]}, {want[1]}, {want[2]}), got '
                                  f'{tuple(input_features[k].shape)} (the engine is planned for {self.H}x{self.W} inputs)')
        key = ('depth_decoder', n)
        st = self._ws.get(key)
        if st is None:
            st = self._ws[key] = self._depth_dec_bufs(n)
        main, self._main = self._main, None          # no side-stream fork: a plain chain on the caller's stream
        try:
            self._depth_decoder(st, feats)
        finally:
            self._main = main
        return {('disp', s): st.disp[s].unsqueeze(1).clone() for s in range(3, -1, -1)}

    def run_depth(self, x: torch.Tensor) -> torch.Tensor:
        """The depth network alone (dpp.py:548-549 predict_from_image; dpp.py:402 inside compute_depth_error): depth encoder ->
        depth decoder, no pose net, no warp, no loss.  -> ('disp', 0), (N,1,H,W)."""
        return self.run_depth_decoder(self.run_encoder('depth_encoder', x))['disp', 0]

    def run_pose_decoder(self, last_features):
        """models['pose_decoder']([features]) (dpp.py:957-965; networks/pose_decoder.py:37-54): (axis_angle, translation), each
        (N, 2, 1, 3), from the last feature map of ONE pose-encoder pass."""
        self._cu_dec = self.cu_limit(0, 'decoders')
        if len(last_features) != 1:
            raise ClslamError('pose_decoder: the MI355X-native path implements num_input_features = 1')
        self.pack_if_needed()
        self._conv_workspace()
        self.wait_training()
        f4 = self._nhwc(last_features[0])
        n = f4.shape[0]
        want = (n, self.H >> 5, self.W >> 5, NUM_CH_ENC[4])
        if tuple(f4.shape) != want:
            raise ClslamError(f'pose_decoder: the feature must be (N, 512, {want[1]}, {want[2]}), got {tuple(last_features[0].shape)}')
        key = ('pose_decoder', n)
        st = self._ws.get(key)
        if st is None:
            st = self._ws[key] = self._pose_dec_bufs(n)
        self._pose_decoder(st, f4)
        out = st.pose.clone().view(-1, 2, 1, 6)          # the 0.01 scale is applied by the head kernel (pose_decoder.py:50)
        return out[..., :3], out[..., 3:]
