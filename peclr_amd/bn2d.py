"""Fused BatchNorm2d (+ residual add) (+ ReLU) for the NHWC backbone (kernels: csrc/bn2d.hip).

`FusedBatchNormAct2d` IS an `nn.BatchNorm2d` (same parameters, buffers and state_dict keys -- the
reference builds its ResNet with `norm_layer=nn.BatchNorm2d`, resnet_model.py:15) whose forward also
takes the block's residual and a ReLU flag, so a ResNet block can hand the whole
"bn -> (+identity) -> relu" tail to one fused HIP pass.

Two execution modes, chosen EXPLICITLY (no silent dispatch):
  hip = False (default)  stock PyTorch ops: F.batch_norm, add, relu -- any device / layout / dtype;
                         this is the PyTorch-ROCm backbone BASELINE.json:north_star describes.
  hip = True             the hand-written HIP kernels; requires fp32, bf16 or fp16 (autocast) channels_last
                         HIP tensors and raises otherwise.  Turn it on with `enable_hip_batchnorm`.
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import os

from typing import Optional

import torch
from torch import Tensor, nn
from torch.nn import functional as F

from . import _capi


# ---- activation checkpointing: a residual block keeps only its INPUT for the
# backward pass and re-runs its forward there.  While a block is being re-run, BatchNorm layers must not
# move their running statistics a second time (`_RECOMPUTING`); batch statistics are recomputed and are
# identical (the kernels are deterministic).
_RECOMPUTING = False
_FIRST_RUN = False      # inside the no-grad first run of a checkpointed block (its BatchNorm layers note the statistics' shift)
# The statistics' shifts of the checkpointed block that is running: id(BatchNorm layer) -> the copy of its running mean the
# first run centred its sums on.  The dictionary belongs to ONE invocation (it lives on that invocation's autograd context):
# the first run fills it, the re-run of the same invocation reads it back -- whatever other forward passes (a second view
# pass, a no-grad evaluation, another accumulation micro-batch) went through the same layers in between.
_CKPT_SHIFTS = None


def _ckpt_shift_of(bn):
    """First run of a checkpointed block: take (once) and return the copy of `bn`'s running mean that this invocation centres
    its statistics on; re-run: the same copy; outside a checkpointed block: None."""
    if _CKPT_SHIFTS is None or not (_FIRST_RUN or _RECOMPUTING):
        return None
    key = id(bn)
    if _FIRST_RUN and key not in _CKPT_SHIFTS:
        _CKPT_SHIFTS[key] = bn.running_mean.detach().clone()
    return _CKPT_SHIFTS.get(key)


class _CheckpointedBlock(torch.autograd.Function):
    """y = run(x) without keeping run's intermediate activations; backward re-runs `run` on the saved input
    under the autocast state of the forward and back-propagates through that second graph (parameter
    gradients accumulate into `.grad` from inside, so gradient hooks -- the all-reduce buckets -- still fire)."""

    @staticmethod
    def forward(ctx, run, x):
        ctx.run = run
        ctx.autocast = (torch.is_autocast_enabled(x.device.type), torch.get_autocast_dtype(x.device.type))
        ctx.save_for_backward(x)
        ctx.shifts = {}
        global _FIRST_RUN, _CKPT_SHIFTS
        was = (_FIRST_RUN, _CKPT_SHIFTS)
        _FIRST_RUN, _CKPT_SHIFTS = True, ctx.shifts
        try:
            with torch.no_grad():
                return run(x)
        finally:
            _FIRST_RUN, _CKPT_SHIFTS = was

    @staticmethod
    def backward(ctx, dy):
        global _RECOMPUTING, _CKPT_SHIFTS
        (x,) = ctx.saved_tensors
        x = x.detach().requires_grad_(True)
        enabled, dtype = ctx.autocast
        was = (_RECOMPUTING, _CKPT_SHIFTS)
        _RECOMPUTING, _CKPT_SHIFTS = True, ctx.shifts
        try:
            with torch.enable_grad(), torch.autocast(x.device.type, dtype=dtype, enabled=enabled):
                y = ctx.run(x)
        finally:
            _RECOMPUTING, _CKPT_SHIFTS = was
        # (ctx.shifts stays with the context: a second backward over a retained graph re-runs the block centred where the first
        # run was and reproduces it bit for bit; the copies -- one running mean per BatchNorm layer of the block -- go with the graph)
        global _NESTED_BACKWARD
        _NESTED_BACKWARD += 1       # (its side-channel entries are drained with the enclosing pass: see _drain_after_backward)
        try:
            torch.autograd.backward((y,), (dy.to(y.dtype),))
        finally:
            _NESTED_BACKWARD -= 1
        _drain_after_backward()
        return None, x.grad


def checkpoint_block(run, x: Tensor) -> Tensor:
    """`run(x)` with activation checkpointing when a gradient will flow (otherwise plain)."""
    if torch.is_grad_enabled() and x.requires_grad and not _RECOMPUTING:
        return _CheckpointedBlock.apply(run, x)
    return run(x)


# gradient tensors whose producer (an input-gradient GEMM) already reduced them against the BatchNorm layer they arrive at:
# data_ptr -> (token of that layer's forward, partial sums, n_split); popped by the layer's backward
_BN_BWD_STATS: dict = {}

def _env_flag(name: str, default: str = "1") -> bool:
    return os.environ.get(name, default) != "0"


@dataclasses.dataclass
class Routing:
    """Every switch that decides which kernel a layer of the fused backbone runs on, in ONE object (`bn2d.ROUTING`).
    The defaults come from the `PECLR_*` environment variables (same-box A/B runs of one build); tests and tools change
    them through `with bn2d.routing(name=value, ...)`.  `force`: route every shape the in-tree kernels ACCEPT to them,
    ignoring the "does it beat MIOpen at this size" tests below -- so that a small problem exercises the same kernels, in
    the same composition, as the full-size configurations (the kernels' own shape constraints still apply)."""
    gemm_x6: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_GEMM_X6"))              # fp32 GEMM-shaped work as six bf16 MFMA products
    x6_min_k: int = dataclasses.field(default_factory=lambda: int(os.environ.get("PECLR_GEMM_X6_MIN_K", "128")))   # in-step A/B: 128 beats 256 by 0.1-0.4 ms
    gemm_x6p: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_GEMM_X6P"))            # weight planes packed once per step (peclr_gemm_x6p_f32)
    gemm_x6t: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_GEMM_X6T"))            # weight gradients on the 256 x 256-tile kernel
    bn_stats_in_gemm: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_BN_STATS_IN_GEMM"))   # BatchNorm statistics in the GEMM epilogue
    bn_bwd_in_gemm: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_BN_BWD_IN_GEMM"))       # BatchNorm backward reduction in the dgrad epilogue
    # the shortcut's BatchNorm (conv1x1 -> bn of a layer's first block) applied inside the block's last pass (bn3 + shortcut + ReLU)
    bn_shortcut_in_add: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_BN_SHORTCUT_IN_ADD"))
    # ... and its backward: the shortcut layer's reduction reads (dy, mask) and ONE apply pass writes the gradients of both layers'
    # inputs (peclr_bn2d_bwd_apply_res_bn) -- the masked gradient is not written out and read back (off: the three-pass form)
    bn_shortcut_bwd_fused: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_BN_SHORTCUT_BWD_FUSED"))
    x6_layer1: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_X6_LAYER1"))          # layer1's 64-channel 1x1 convolutions in-tree
    x6_layer1_fork: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_X6_LAYER1_FORK"))   # layer1's fused entry gradient (K = 64)
    x6_layer1_wgrad: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_X6_LAYER1_WGRAD"))  # layer1's 64-wide weight gradients
    conv3x3_x6: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_CONV3X3_X6"))        # 3x3 stride-1 convolutions as implicit GEMMs
    conv3x3_wgrad_x6: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_CONV3X3_WGRAD_X6"))   # their weight gradients (nine taps, one launch)
    conv3x3_tile_rows: int = dataclasses.field(default_factory=lambda: int(os.environ.get("PECLR_CONV3X3_TILE_ROWS", "256")))
    # (pair arithmetic: the rounds-of-slots policy, 0 -- same-box A/B at C2: 47.53 ms per step against 47.73 / 47.94 with 128 / 256 rows)
    conv3x3_pair_tile_rows: int = dataclasses.field(default_factory=lambda: int(os.environ.get("PECLR_CONV3X3_PAIR_TILE_ROWS", "0")))
    conv_s2_x6: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_CONV_S2_X6"))        # forward of the stride-2 convolutions
    conv_s2_wgrad_x6: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_CONV_S2_WGRAD_X6"))
    conv_s2_dgrad_x6: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_CONV_S2_DGRAD_X6"))   # 3x3 / stride-2 input gradient by parity classes
    s2_tile_rows: int = dataclasses.field(default_factory=lambda: int(os.environ.get("PECLR_CONV_S2_TILE_ROWS", "0")))   # 0 = the rounds-of-slots policy
    s2_dgrad_compact: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_S2_DGRAD_COMPACT"))   # the shortcut's compact input gradient
    lazy_residual_grad: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_LAZY_RESIDUAL_GRAD"))   # identity shortcut: (dy, mask) hand-over
    conv16: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_CONV16"))                # 16-bit (bf16 / fp16 autocast) convolutions in-tree
    # fp32 forward / input-gradient GEMMs in "pair" arithmetic (round 6): operands scaled by a per-tensor power of two and split into
    # two fp16 numbers, three MFMA products instead of six -- where the operand tensor carries its maximum (`_peclr_absmax`, written
    # by the BatchNorm pass that produced it); anything else runs the six-product kernels as before
    x6_pair: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_X6_PAIR"))
    wgrad16: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_WGRAD16"))              # ... and their weight gradients
    # ... the 3x3 ones of rows wider than 62 pixels too (inputs above 248 px: peclr_wgrad3w_h, column segments; off: MIOpen there.
    # On: 0.39 - 0.58 of MIOpen's time at layer1 of 448 and 256 px inputs, bf16 and fp16: profiles/wgrad3_wide_timing.txt)
    wgrad16_wide: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_WGRAD16_WIDE"))
    # ... the 3x3 / stride-2 ones that open layers 2 - 4 too (peclr_wgrad3s2_h, parity planes; off: MIOpen's atomic split-K there).
    # Opt-in: over C2's three shapes 352 against MIOpen's 397 us in bf16 but 360 against 345 in fp16, and the default's rule asks for both
    # formats (profiles/wgrad3_s2_timing.txt; the bf16 step is 0.07 ms faster with it: profiles/wgrad3_s2_step_ab.txt).  What it buys
    # besides: a 16-bit step without atomics (bit-reproducible), without an aten convolution and without a find-db entry
    wgrad16_s2: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_WGRAD16_S2", "0"))
    stem_wgrad: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_STEM_WGRAD"))        # ... and its weight gradient
    stem: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_STEM"))                    # the 7x7 / stride-2 stem forward in-tree (csrc/stem.hip)
    # 16-bit prediction: the eval-mode BatchNorm layers of the bottleneck blocks folded into the 16-bit convolutions' epilogues
    # (`fold_plan`, resnet.Bottleneck._run_folded).  Opt-in: FreiHANDPredictor(precision="bf16") turns it on for its own passes
    fold_eval_bn: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_FOLD_EVAL_BN", "0"))
    force: bool = dataclasses.field(default_factory=lambda: _env_flag("PECLR_ROUTE_FORCE", "0"))

    # ---- "does the in-tree kernel pay at this shape" (measured on ResNet-50's shapes; the kernels accept far more)
    def tiles(self, rows: int, n_out: int) -> int:
        """Workgroup tiles of a [rows, n_out] output on 128-row x 128-column (64 for narrow outputs) tiles."""
        return (rows // 128) * max(1, n_out // (128 if n_out >= 128 else 64))

    MALL_BYTES = 256 << 20        # Infinity Cache (MI355X_MICROARCH.md): tensors beyond it stream from HBM

    def streams_from_hbm(self, rows: int, k: int, n_out: int) -> bool:
        """The product's fp32 operand + output rows exceed the Infinity Cache: a separate BatchNorm statistics /
        backward-reduction pass over them would come from HBM again.  This is what makes the in-tree GEMM pay for the
        64-channel shapes (layer1), where the GEMM itself is a draw against MIOpen (both HBM-bound: tools/exp/layer1_probe.py)
        and the fused epilogue saves that pass."""
        return self.force or 4 * rows * (k + n_out) >= self.MALL_BYTES

    def fills_chip(self, rows: int, n_out: int, rounds: float = 0.765) -> bool:
        """At least `rounds` of the chip's 256 CUs get a tile: below that the launch is latency- and tail-bound and
        MIOpen's smaller tiles win (ResNet-50 @224 with 2 x 128 views: every routed shape has >= 196 tiles)."""
        return self.force or self.tiles(rows, n_out) >= 256 * rounds


ROUTING = Routing()


@contextlib.contextmanager
def routing(**overrides):
    """Temporarily change fields of `ROUTING` (tests, A/B tools): `with bn2d.routing(bn_bwd_in_gemm=False): ...`."""
    old = {k: getattr(ROUTING, k) for k in overrides}
    for k, v in overrides.items():
        if not hasattr(ROUTING, k):
            raise AttributeError(f"Routing has no field {k!r}")
        setattr(ROUTING, k, v)
    try:
        yield ROUTING
    finally:
        for k, v in old.items():
            setattr(ROUTING, k, v)


def _rows(x: Tensor) -> Tensor:
    """The NHWC storage of a channels_last [N, C, H, W] tensor seen as [N H W, C] (a view)."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _nchw(y2: Tensor, n: int, h: int, w: int) -> Tensor:
    """... and back: [N H W, C] rows as the channels_last [N, C, H, W] tensor they are (a view)."""
    return y2.view(n, h, w, y2.shape[1]).permute(0, 3, 1, 2)


class _PackedOnce:
    """Freshness of ONE set of packed weight planes (a plane set of an `X6PackGroup`, the stem filter of one precision): the
    planes object is (re-)packed when the weight asked about changed since the last pack (in-place update: `_version`; fused
    optimiser step, which writes through raw pointers: `_capi.WEIGHTS_EPOCH`; new storage: `data_ptr`) and by the FIRST request
    of every hipGraph capture, whatever the stamps say (the host-side stamps describe the moment of recording, a replay must
    re-split the weights it is about to use); it is built when there is none for the weights' present storage -- never while
    capturing: building uploads a pointer table (a host-to-device copy) and allocates the planes, and neither may be recorded
    into a hipGraph (`missing`: the error raised then)."""

    __slots__ = ("planes", "ptrs", "stamps", "capture")

    def __init__(self):
        self.planes, self.ptrs, self.stamps, self.capture = None, None, None, 0     # (capture: the one that already holds a pack launch)

    @staticmethod
    def stamp(w):
        return (w.data_ptr(), w._version, _capi.WEIGHTS_EPOCH)

    def pack(self, weights, build, missing: str):
        """Pack now; `build()` makes the planes object (one `.pack()` launch for all of `weights`)."""
        ptrs = [w.data_ptr() for w in weights]
        if self.planes is None or ptrs != self.ptrs:
            if _capi.capture_id() != 0:
                raise _capi.PeclrHipError(missing)
            self.planes, self.ptrs = build(), ptrs
        self.planes.pack()
        self.stamps = [self.stamp(w) for w in weights]

    def fresh(self, w, at: int, repack):
        """The planes object, after `repack()` (the owner's call of `pack`) if `w`, weight number `at` of the set, moved since the
        last pack or this capture has no pack launch yet."""
        stale = self.stamps is None or self.stamps[at] != self.stamp(w)
        cap = _capi.capture_id()
        if cap != self.capture:          # a new capture (or back to eager launches): this capture has no pack launch yet
            stale = stale or cap != 0
            self.capture = cap
        if stale:
            repack()
        return self.planes


class X6PackGroup:
    """The 1x1-convolution weights of one encoder that run as peclr_gemm_x6p_f32 GEMMs, split into fragment-ordered
    bf16 planes by ONE launch per optimiser step (peclr_x6_pack_f32): W[Cout][Cin] for the forward GEMM, W^T for the
    input-gradient GEMMs.  A member convolution asks `planes(conv)` right before it launches; the group re-packs
    everything when that convolution's weight changed since the last pack, and on the first `planes()` call of a hipGraph
    capture, whichever member makes it (`_PackedOnce`)."""

    MISSING = ("X6PackGroup: the weight planes of this precision do not exist yet and cannot be created "
               "while a hipGraph is being captured -- run one eager forward pass (same autocast dtype) first")

    def __init__(self, convs):
        self.convs = [c for c in convs if self.member(c)]
        # one plane set (`_PackedOnce`) per operand format: None = the three bf16 planes of the fp32 six-product kernels
        # (peclr_x6_pack_f32); "pair" = their fp16-pair format; torch.bfloat16 / torch.float16 = the single 16-bit plane of the
        # autocast kernels (peclr_h_pack), packed from the same fp32 master weights
        self._sets = {}
        for i, c in enumerate(self.convs):   # (position kept on the module: a deep copy of the model keeps group and members consistent)
            c.x6_group, c.x6_index = self, i

    @staticmethod
    def member(conv) -> bool:
        cout, cin = conv.out_channels, conv.in_channels
        if conv.stride not in ((1, 1), (2, 2)) or conv.groups != 1 or conv.bias is not None:
            return False            # (stride 2: the forward only, `_ConvS2Gemm`)
        if conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.dilation == (1, 1):
            return cout >= 64 and cin >= 64 and cout % 64 == 0 and cin % 64 == 0        # 64-column tiles for layer1
        return (conv.kernel_size == (1, 1) and conv.padding == (0, 0) and cout >= 64 and cin >= 64
                and cout % 64 == 0 and cin % 64 == 0)

    def _specs(self):
        specs = []
        for c in self.convs:
            if c.kernel_size == (3, 3):
                # [Cout][3][3][Cin] as it lies in (channels_last) memory: forward B_t = [Cout, 9 Cin]; input gradient
                # B_t[ci][tap * Cout + co] = W[co][tap][ci]
                w4 = c.weight.detach().permute(0, 2, 3, 1)
                if not w4.is_contiguous():
                    raise _capi.PeclrHipError("X6PackGroup: 3x3 weights must be channels_last (NHWC encoder)")
                specs += [(w4.reshape(c.out_channels, 9 * c.in_channels), False), (w4.reshape(c.out_channels * 9, c.in_channels), 9)]
            else:
                w2 = c.weight.detach().reshape(c.out_channels, c.in_channels)
                specs += [(w2, False), (w2, True)]
        return specs

    def _build(self, dtype):
        return (_capi.X6Planes(self._specs()) if dtype is None else _capi.X6Planes(self._specs(), pair=True) if dtype == "pair"
                else _capi.HPlanes(self._specs(), dtype))

    def pack(self, dtype=None):
        self._sets.setdefault(dtype, _PackedOnce()).pack([c.weight for c in self.convs], lambda: self._build(dtype), self.MISSING)

    def planes(self, conv, dtype=None):
        """(forward planes of W [Cout, Cin], input-gradient planes of W^T), fresh; dtype None: the fp32 kernels' three-plane
        format, "pair": their fp16-pair format (`pair_scales` gives the matrices' powers of two), torch.bfloat16 / torch.float16:
        the 16-bit kernels' format."""
        at = conv.x6_index
        if at >= len(self.convs) or self.convs[at] is not conv:
            raise _capi.PeclrHipError("X6PackGroup: convolution is not a member of its group (call enable_hip_batchnorm again)")
        st = self._sets.setdefault(dtype, _PackedOnce())
        planes = st.fresh(conv.weight, at, lambda: self.pack(dtype)).planes
        return planes[2 * at], planes[2 * at + 1]

    def pair_scales(self, conv):
        """The device floats holding the powers of two of `conv`'s two pair-format matrices (after `planes(conv, "pair")`)."""
        st = self._sets["pair"].planes
        return st.scale(2 * conv.x6_index), st.scale(2 * conv.x6_index + 1)


def _x6_planes(conv):
    """Packed planes of `conv`'s weight, or None when the convolution is not in a pack group (then the GEMMs split the
    weight per workgroup: peclr_gemm_x6_f32)."""
    group = getattr(conv, "x6_group", None) if conv is not None else None
    if group is None or not ROUTING.gemm_x6p or not conv.weight.is_cuda or conv.weight.dtype != torch.float32:
        return None
    return _LazyPlanes(group, conv)


class _LazyPlanes:
    """`planes[0]` / `planes[1]` of a convolution's six-product plane set, asked of the group (which re-packs a stale set: one launch
    for all members) only when a launch really takes them -- with `ROUTING.x6_pair` most launches take the pair set instead, and
    a step in which nothing falls back never packs the three-plane set at all."""

    __slots__ = ("group", "conv")

    def __init__(self, group, conv):
        self.group, self.conv = group, conv

    def __getitem__(self, which):
        return self.group.planes(self.conv)[which]


def _absmax_of(t):
    """The device float holding max |t| if the pass that wrote `t` left one (fp32 tensors, `ROUTING.x6_pair`) AND nothing has
    written to `t` since (its version counter stands where the pass left it: an in-place update would make the maximum -- and with
    it the fp16 range the pair kernels scale into -- stale), else None."""
    if not ROUTING.x6_pair or t is None:
        return None
    tag = getattr(t, "_peclr_absmax", None)
    return tag[0] if (tag is not None and tag[1] == t._version) else None


def _tag_absmax(t: Tensor, slot):
    """Attach the maximum `slot` (a one-element device tensor) to the tensor it describes."""
    t._peclr_absmax = (slot, t._version)


def _new_absmax(x: Tensor):
    """A zeroed slot for the maximum of a tensor a BatchNorm pass is about to write (None: not wanted)."""
    return _capi.absmax_slot(x.device) if (ROUTING.x6_pair and ROUTING.gemm_x6p and x.is_cuda and x.dtype == torch.float32) else None


def _publish_absmax(x: Tensor, amax):
    """The slot a forward pass over `x` writes its output's maximum to, published to the caller's list `amax` (None: the caller
    wants no maximum); None when there is none."""
    slot = _new_absmax(x) if amax is not None else None
    if slot is not None:
        amax[:] = [slot]
    return slot


def _tagged(t: Tensor, slot) -> Tensor:
    """`t`, carrying the maximum `slot` its pass wrote (None: the pass wrote none)."""
    if slot is not None:
        _tag_absmax(t, slot)
    return t


def _pair_planes(conv, amax, which: int, planes):
    """What a packed-weight GEMM of `conv` runs on: (planes, {"pair": (amax, w_scale)}) -- the fp16-pair planes of matrix `which`
    (0 forward, 1 input gradient) when the activation operand's maximum `amax` is known -- else (planes[which], {}): the
    six-product arithmetic."""
    group = getattr(conv, "x6_group", None) if conv is not None else None
    if amax is None or group is None or not ROUTING.x6_pair:
        return planes[which], {}
    pp = group.planes(conv, "pair")
    return pp[which], {"pair": (amax, group.pair_scales(conv)[which])}


def _launch_packed(kernel, a: Tensor, conv, amax, which: int, planes, *rest, rows_six_pair=None, **kw):
    """ONE launch of a packed-weight kernel of `conv`: `kernel(a, planes of matrix which, *rest, **kw)` on what `_pair_planes`
    picks -- the fp16-pair planes (and `pair=`) where the maximum `amax` of the activation operand `a` is known, else the
    six-product planes.  rows_six_pair: None, or the kernel's `tile_rows` as (in the six-product form, in pair arithmetic) -- the
    3x3 kernels' tile height depends on which arithmetic was taken."""
    pl, pkw = _pair_planes(conv, amax, which, planes)
    if rows_six_pair is not None:
        kw["tile_rows"] = rows_six_pair[bool(pkw)]
    return kernel(a, pl, *rest, **pkw, **kw)


_HALF = (torch.bfloat16, torch.float16)


def _h_ok(conv, x: Tensor) -> bool:
    """Does `conv` run on the in-tree 16-bit kernels for input `x`?  bf16 / fp16 NHWC activations under the matching autocast,
    fp32 master weights in a pack group (peclr_h_pack packs them once per step: autocast's per-forward cast is gone)."""
    return (ROUTING.conv16 and x.is_cuda and x.dtype in _HALF and x.dim() == 4 and torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == x.dtype and getattr(conv, "x6_group", None) is not None
            and conv.weight.is_cuda and conv.weight.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last))


class _BN2dAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn: "FusedBatchNormAct2d", relu: bool, pre=None, link=None, lazy_res=False, defer=None,
                res_deferred=None, amax=None):
        """link: None or an empty list that receives what a consumer's input-gradient GEMM needs to perform this layer's
        backward reduction in its epilogue: [x, save, scale_shift, relu mask or None, relu, token].
        defer: None, or an empty list -- the layer (a shortcut's BatchNorm, no ReLU) only finishes its statistics; the list comes
        back as [x, scale_shift, relu, hand-over record] and the result is a placeholder (`_deferred_view`) whose consumer -- the
        block's last BatchNorm pass -- computes the layer on the fly; any other reader materialises it (`_Materialize`).
        res_deferred: None, or (x_s, scale_shift_s, False, record) -- `residual` is the placeholder of the shortcut's BatchNorm layer (no
        ReLU), which left its apply pass to THIS pass: the residual is computed from that layer's input on the fly.
        amax: None, or an empty list that receives the device float holding max |y| (the "pair" GEMMs' operand scale)."""
        training, sync, stat_args, stat_kw = bn._fwd_args(pre)
        # the ReLU mask can be recomputed from x unless a residual was added before it; then the
        # forward writes a 1-bit mask (or, for C % 32 != 0, the backward re-reads y)
        need_mask = relu and residual is not None
        slot = _publish_absmax(x, amax if defer is None else None)
        y, save, ss, mask = _capi.bn2d_fwd(x, None if res_deferred is not None else residual, weight, bias, *stat_args, relu,
                                           want_mask=need_mask, apply=defer is None,
                                           residual_bn=res_deferred[:2] if res_deferred is not None else None, absmax=slot, **stat_kw)
        ctx.handover = None
        if defer is not None:
            # (the fourth entry: what the consumer's backward needs to perform this layer's backward too -- `_dual_backward_ok`)
            ctx.handover = dict(save=save, training=training, sync=sync, needs_dx=ctx.needs_input_grad[0],
                                checkpointed=_RECOMPUTING or _FIRST_RUN, materialized=False)
            defer[:] = [x, ss, relu, ctx.handover]
            y = _deferred_view(x)
        keep = mask if mask is not None else (y if need_mask else None)
        # the shortcut layer's backward in this layer's backward pass (ROUTING.bn_shortcut_bwd_fused): decided here as far as the
        # forward knows, and again in the backward (`_dual_backward_ok`)
        ctx.dual = None
        if (ROUTING.bn_shortcut_bwd_fused and res_deferred is not None and len(res_deferred) > 3 and relu and mask is not None
                and sync is None and res_deferred[3]["sync"] is None and res_deferred[3]["needs_dx"]
                and not (_RECOMPUTING or _FIRST_RUN or res_deferred[3]["checkpointed"])):
            ctx.dual = res_deferred[3]
        dual_saved = [res_deferred[0], res_deferred[3]["save"], res_deferred[1]] if ctx.dual is not None else []
        ctx.save_for_backward(x, save, ss, *([keep] if keep is not None else []), *dual_saved)
        ctx.cfg = (training, relu, residual is not None, keep is not None, mask is not None)
        ctx.sync_group = sync
        ctx.token = None
        # the residual's gradient is relu'(y) * dy: when its only consumer is the block's entry-gradient GEMM (which then
        # reads dy and the 1-bit mask itself), it is handed over as that pair instead of being written out
        ctx.lazy_res = bool(lazy_res and mask is not None and (x.dtype == torch.float32 or ROUTING.conv16))
        if link is not None and (x.dtype == torch.float32 or ROUTING.conv16) and (keep is None or mask is not None):
            ctx.token = object()
            link[:] = [x, save, ss, mask, relu, ctx.token]
        return y

    @staticmethod
    def backward(ctx, dy):
        training, relu, has_res, has_keep, is_mask = ctx.cfg
        x, save, ss = ctx.saved_tensors[:3]
        keep = ctx.saved_tensors[3] if has_keep else None
        y, mask = (None, keep) if is_mask else (keep, None)
        handed = _take_lazy(dy)
        if handed is not None and handed[0] == "bn":
            # the consumer's backward (the block's last BatchNorm pass) performed this layer's backward as well: nothing to launch
            _, dx, dgamma, dbeta, slot, owner = handed
            if owner is not ctx.handover:
                raise _capi.PeclrHipError("fused BatchNorm2d: a shortcut layer's gradients arrived at another layer")
            return _tagged(dx, slot), dgamma, dbeta, None, None, None, None, None, None, None, None, None
        if handed is not None:
            dy = _dense_of(handed, dy.shape)
        dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        pre = None
        ent = _BN_BWD_STATS.pop(dy.data_ptr(), None) if ctx.token is not None else None
        # the GEMM that produced dy reduced it against x already -- valid only for the tensor that GEMM wrote, untouched:
        # a second consumer of this layer's output makes autograd add its gradient INTO that buffer (in place: the
        # version counter moves), and the sums would miss that contribution
        if ent is not None and ent[0] is ctx.token and ent[3] == dy._version:
            pre = ent[1:3]
        lazy = ctx.lazy_res and has_res and ctx.needs_input_grad[3] and ROUTING.lazy_residual_grad and not torch.is_anomaly_enabled()
        slot = _new_absmax(x)
        if _dual_backward_ok(ctx):
            # first block of a stage: the shortcut layer's reduction on (dy, mask), then both layers' apply passes in one; that
            # layer's node receives its finished gradients (`_lazy_grad`) and launches nothing
            xs, save_s, ss_s = ctx.saved_tensors[-3:]
            slot_s = _new_absmax(xs)
            dx, dgamma, dbeta, dxs, dgamma_s, dbeta_s = _capi.bn2d_bwd_res_bn(dy, x, mask, save, ss, training, xs, save_s, ss_s,
                                                                              ctx.dual["training"], pre=pre, absmax=slot, absmax_s=slot_s)
            dres = _lazy_grad(("bn", dxs, dgamma_s, dbeta_s, slot_s, ctx.dual), xs.shape, xs.device, xs.dtype)
            return _tagged(dx, slot), dgamma, dbeta, dres, None, None, None, None, None, None, None, None
        dx, dgamma, dbeta, dres = _capi.bn2d_bwd(dy, x, y, mask, save, ss, training, relu,
                                                 has_res and ctx.needs_input_grad[3] and not lazy, sync_group=ctx.sync_group, pre=pre,
                                                 absmax=slot)
        _tagged(dx, slot)                       # (the convolution whose output x is reads it off its `gy`: same tensor object)
        if lazy:
            dres = _lazy_grad(("mask", dy, mask), x.shape, x.device, x.dtype)
        elif has_res and dres is None and ctx.needs_input_grad[3]:
            dres = dy
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None


def _dual_backward_ok(ctx) -> bool:
    """May the backward of the block's last BatchNorm pass (`ctx`) perform the shortcut layer's backward as well
    (peclr_bn2d_bwd_apply_res_bn)?  `ctx.dual` -- the shortcut layer's hand-over record -- is there when the forward found nothing
    against it (the switch, a 1-bit mask, per-rank statistics, no activation checkpointing, a shortcut input that wants its
    gradient); the backward adds what only it can know: the switch now, anomaly mode (the hand-over is a NaN view), a second
    reader for which the placeholder was written out after all (autograd would ADD its gradient to the view)."""
    return bool(ctx.dual is not None and ROUTING.bn_shortcut_bwd_fused and ctx.needs_input_grad[3] and not ctx.dual["materialized"]
                and not _NESTED_BACKWARD and not torch.is_anomaly_enabled())


_NAN_PLACEHOLDER = {}


def _deferred_view(x: Tensor) -> Tensor:
    """Stands for relu(bn(x)) where that tensor is never written: NaN under every index (one element, zero strides), so that a
    reader that does not know the protocol cannot go unnoticed."""
    nan = _NAN_PLACEHOLDER.get((x.device, x.dtype))      # (its own element: never the address of one of `_lazy_grad`'s sentinels)
    if nan is None:
        nan = _NAN_PLACEHOLDER[(x.device, x.dtype)] = torch.full((1,), float("nan"), device=x.device, dtype=x.dtype)
    return nan.view(1, 1, 1, 1).expand(x.shape)


class _Materialize(torch.autograd.Function):
    """The output of a BatchNorm layer whose apply pass was left to its consumer, written after all (the reader turned out
    not to be the pass that computes it on the fly): peclr_bn2d_apply on the finished table."""

    @staticmethod
    def forward(ctx, placeholder, deferred, amax=None):
        x, ss, relu = deferred[:3]
        return _capi.bn2d_apply(x, ss, relu=relu, absmax=_publish_absmax(x, amax))

    @staticmethod
    def backward(ctx, gy):
        return gy, None, None


def _materialized(x: Tensor, deferred) -> Tensor:
    if len(deferred) > 3:
        deferred[3]["materialized"] = True      # (this reader's gradient comes back dense: `_dual_backward_ok`)
    amax = []
    y = _tagged(_Materialize.apply(x, deferred, amax), amax[0] if amax else None)
    link = getattr(x, "_peclr_bn_link", None)
    if link:
        y._peclr_bn_link = link
    return y


class _BN2dReluPool(torch.autograd.Function):
    """Stem: BatchNorm2d -> ReLU -> MaxPool2d(3, 2, 1) without ever writing the un-pooled activation."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn: "FusedBatchNormAct2d", pre=None, amax=None):
        training, sync, stat_args, stat_kw = bn._fwd_args(pre)
        y, x_at_max, code, save, ss = _capi.bn2d_pool_fwd(x, weight, bias, *stat_args, absmax=_publish_absmax(x, amax), **stat_kw)
        ctx.save_for_backward(x, x_at_max, code, save, ss)
        ctx.cfg = (training, sync)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, x_at_max, code, save, ss = ctx.saved_tensors
        training, sync = ctx.cfg
        dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        dx, dgamma, dbeta = _capi.bn2d_pool_bwd(dy, x, x_at_max, code, save, ss, training, sync_group=sync)
        return dx, dgamma, dbeta, None, None, None


class _BN2dAddReluAvgPool(torch.autograd.Function):
    """Encoder tail (the last residual block's bn + identity + ReLU, then AdaptiveAvgPool2d((1, 1)) and
    flatten): returns the pooled fp32 [N, C] features; the [N, C, H, W] activation is never materialised,
    and the backward forms the pool's broadcast gradient on the fly."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn: "FusedBatchNormAct2d", pre=None):
        training, sync, stat_args, stat_kw = bn._fwd_args(pre)
        pooled, mask, save, ss = _capi.bn2d_avgpool_fwd(x, residual, weight, bias, *stat_args, **stat_kw)
        ctx.save_for_backward(x, mask, save, ss)
        ctx.cfg = (training, sync)
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        x, mask, save, ss = ctx.saved_tensors
        training, sync = ctx.cfg
        slot = _new_absmax(x)
        dx, dgamma, dbeta, dres = _capi.bn2d_avgpool_bwd(d_pooled.float().contiguous(), x, mask, save, ss, training,
                                                         sync_group=sync, absmax=slot)
        return _tagged(dx, slot), dgamma, dbeta, dres, None, None


# ---- weight gradients on a side stream.  In the backward pass a convolution's weight gradient (MFMA-bound) is
# needed only by the optimiser, while its input gradient feeds the next BatchNorm backward (HBM-bound) at once.
# With `enable_wgrad_overlap`, every convolution of the in-tree ResNet computes its weight gradient on a second
# HIP stream: it runs next to the glue kernels of the layers below it instead of in front of them, so the chip's
# MFMA pipes and its memory system are busy at the same time.  Such a gradient does NOT travel through autograd's
# AccumulateGrad (which would read it on the main stream): it is parked and handed to its parameter by
# `wgrad_join()`, which the caller runs after backward, once the main stream has waited for the side stream.
# Under hipGraph capture the side stream becomes a parallel branch of the graph.
class _WgradOverlap:
    stream = None        # torch.cuda.Stream or None (= mode off: everything on the current stream, through autograd)
    armed = False        # the mode only acts between `arm_wgrad_overlap()` (before a forward pass whose backward the
    #                      caller will follow with `wgrad_join()`) and that join: any other forward / backward in the
    #                      process -- a plain `loss.backward(); opt.step()` -- goes through autograd as usual
    parked: list = []    # (parameter, gradient computed on the side stream, tensors it read)


def enable_wgrad_overlap(enabled: bool = True):
    """Create (or drop) the side stream of the side-stream weight gradients; they act only while armed."""
    if enabled and _WgradOverlap.stream is None:
        _WgradOverlap.stream = torch.cuda.Stream()
    elif not enabled:
        wgrad_join()
        _WgradOverlap.stream = None


def arm_wgrad_overlap():
    """Before a forward pass whose backward will be followed by `wgrad_join()` (the Trainer does both)."""
    _WgradOverlap.armed = _WgradOverlap.stream is not None


def _overlap_stream():
    return _WgradOverlap.stream if _WgradOverlap.armed else None


def wgrad_join(on_joined=None):
    """After backward: wait for the side stream, then give every parked gradient to its parameter
    (`.grad = g`, or `.grad += g` when one is already there: accumulation windows, all-reduce bucket views), call
    `on_joined(parameter)` for each (the all-reduce buckets count their members off there: these gradients never pass
    AccumulateGrad, so no post-accumulate hook fires for them), and disarm."""
    _WgradOverlap.armed = False
    if not _WgradOverlap.parked:
        return
    torch.cuda.current_stream().wait_stream(_WgradOverlap.stream)
    with torch.no_grad():
        for param, g, _inputs in _WgradOverlap.parked:
            if param.grad is None:
                param.grad = g
            else:
                param.grad.add_(g)
            if on_joined is not None:
                on_joined(param)
    _WgradOverlap.parked.clear()


def _on_side_stream(param, inputs, run, parked_as=None):
    """A weight gradient `run()` computed from `inputs` = (gy, x).  Overlap off, no parameter to park it for, or inputs that are
    not on the device: computed here and returned.  Overlap on: issued on the side stream (`parked_as(g)`, there too, gives it the
    form `wgrad_join` hands over), parked for `param`, returns None."""
    st = _overlap_stream()
    if st is None or param is None or not inputs[0].is_cuda:
        return run()
    st.wait_stream(torch.cuda.current_stream())          # gy (and x) are ready where the side stream picks up
    with torch.cuda.stream(st):
        g = run()
        if parked_as is not None:
            g = parked_as(g)
    _WgradOverlap.parked.append((param, g, inputs))      # inputs stay referenced until the join
    return None


def _conv_wgrad(gy: Tensor, x: Tensor, weight: Tensor, stride, padding, param=None):
    """d(weight) of conv2d(x, weight) for output gradient gy, from MIOpen; parked for `param` (in the parameter's layout) on the
    side stream when that mode is on."""
    def run():
        g = torch.ops.aten.convolution_backward(gy, x, weight.to(x.dtype), None, list(stride), list(padding), [1, 1], False,
                                                [0, 0], 1, [False, True, False])[1]
        return g.to((param if param is not None else weight).dtype)

    def as_param(g):                                     # channels_last weights
        return g if g.stride() == param.stride() else torch.empty_like(param).copy_(g)
    return _on_side_stream(param, (gy, x), run, parked_as=as_param)


class _Conv2dSplitBackward(torch.autograd.Function):
    """conv2d (no bias, groups 1, dilation 1) whose backward computes the input gradient on the current stream and
    the weight gradient through `_conv_wgrad` (parked on the side stream when overlap is on)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, param):
        ctx.save_for_backward(x, weight)
        ctx.cfg = (tuple(stride), tuple(padding), param)
        return F.conv2d(x, weight, None, stride, padding)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, padding, param = ctx.cfg
        gy = gy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        dw = _conv_wgrad(gy, x, weight, stride, padding, param) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.ops.aten.convolution_backward(gy, x, weight.to(x.dtype), None, list(stride), list(padding), [1, 1], False,
                                                     [0, 0], 1, [True, False, False])[0]
        if dw is not None and dw.dtype != weight.dtype:
            dw = dw.to(weight.dtype)
        return dx, dw, None, None, None


def _x6_pays(rows: int, n_out: int, k: int) -> bool:
    """Does peclr_gemm_x6_f32 beat MIOpen's fp32 1x1 convolution for a [rows, k] x [k, n_out] product?  Measured on
    ResNet-50's shapes (tools/exp/conv1x1_probe.py, and in the step): from K = 128 on when the 128-wide column tile is
    full and the 128 x 128 tiles fill the chip; the K = 64 and N = 64 shapes of layer1 are HBM-bound either way."""
    # (64-wide outputs -- layer1 -- have a 128 x 64-tile variant in the library that wins in isolation, 256 vs 345 us,
    # and loses 0.4 ms per step inside it, where MIOpen's kernels find their operands in the caches: not routed)
    if not ROUTING.gemm_x6:
        return False
    if (k >= ROUTING.x6_min_k or (ROUTING.force and k >= 64)) and k % 4 == 0 and n_out >= 128 and n_out % 4 == 0 and ROUTING.fills_chip(rows, n_out):
        return True
    # layer1 (64 <-> 256 channels, 8e5 rows): HBM-bound, the GEMM itself is a draw against MIOpen (290 vs 296 us, 269 vs 331,
    # input gradient 253 vs 322: tools/exp/layer1_probe.py) -- what pays is that the in-tree GEMM also delivers the next
    # BatchNorm's statistics / performs the previous one's backward reduction, each a pass over up to 822 MB
    return (ROUTING.x6_layer1 and ROUTING.gemm_x6p and ROUTING.streams_from_hbm(rows, k, n_out) and k >= 64 and k % 16 == 0
            and n_out >= 64 and n_out % 64 == 0)


def _x6_wgrad_pays(rows: int, cout: int, cin: int) -> bool:
    """peclr_gemm_x6t_f32 against MIOpen's fp32 1x1 weight gradient (tools/exp/conv1x1_probe.py, wgrad_probe.py): 150-205 us
    against 208-267 from layer2 on; the 64-wide gradients of layer1 (HBM-bound: 8e5 rows of 64 + 256 channels) on 64 x 256 /
    256 x 64 / 64 x 128 tiles."""
    wide = 128 if not (ROUTING.gemm_x6t and ROUTING.x6_layer1_wgrad) else 64
    return ROUTING.gemm_x6 and cout >= wide and cin >= wide and cout % 4 == 0 and cin % 4 == 0 and (rows >= 8192 or ROUTING.force)


def _like_param(dw: Tensor, ref: Tensor, taps: int) -> Tensor:
    """The slab sum `dw` [Cout, taps * Cin] of a weight-gradient kernel as a tensor shaped and strided like the parameter `ref`
    (same memory): nine taps lie in the channels_last storage order [Cout][3][3][Cin]; one tap is [Cout][Cin] in memory under
    either of the parameter's layouts."""
    if taps == 9:
        return dw.view(ref.shape[0], 3, 3, ref.shape[1]).permute(0, 3, 1, 2)      # = a channels_last [Cout, Cin, 3, 3] tensor
    return dw.as_strided(ref.shape, ref.stride())


def _wgrad_1x1_x6(gy: Tensor, x: Tensor, weight: Tensor, param=None):
    """d(weight) of a 1x1 / stride-1 convolution as dY^T X on the bf16 matrix cores (fp32 accuracy, deterministic
    split-K), shaped and strided like the weight; parked for `param` on the side stream when that mode is on."""
    def run():
        gy2, x2 = _rows(gy), _rows(x)
        dw = (_capi.gemm_x6t(gy2, x2, tag="conv1x1_wgrad") if ROUTING.gemm_x6t
              else _capi.gemm_x6_tn(gy2, x2, tag="conv1x1_wgrad"))
        return _like_param(dw, param if param is not None else weight, 1)

    return _on_side_stream(param, (gy, x), run)


def _stat_shift_for(bn, cout: int):
    """The shift a GEMM epilogue subtracts before it sums the statistics `bn` will finalize (None: `bn` cannot take
    statistics from its producer -- not a fused training-mode BatchNorm of that width, or no running mean to centre on).
    The running mean is the natural centre (the sums are exact in the shift; it only has to be near the batch mean, and
    identical on every rank under synchronised statistics); the re-run of a checkpointed block under synchronised
    statistics re-uses the copy its first run took."""
    if (not isinstance(bn, FusedBatchNormAct2d) or not bn.hip or not bn.affine or bn.num_features != cout
            or bn.running_mean is None or not bn.training or not bn.running_mean.is_cuda):
        return None
    # activation checkpointing: the re-run centres its sums where the first run did (the running mean has moved in between),
    # so that it reproduces the first run's statistics bit for bit -- 16-bit activations amplify a last-bit difference in a
    # scale into whole-ulp differences a few layers on; under synchronised statistics the same copy is the common shift
    kept = _ckpt_shift_of(bn)
    return kept if kept is not None else bn.running_mean


def _with_stats(stats, cout: int, launch) -> Tensor:
    """Statistics in the GEMM epilogue: the output of a forward `launch(**kw)` of `cout` channels.  stats: None, or [bn] -- the
    BatchNorm2d that consumes the output; where that layer can take its statistics from its producer (`_stat_shift_for`) the
    launch gets `stat_shift` (and returns (y, partial, n_split)) and the list comes back as [partial, n_split, shift, bn] for
    `_attach_stats`; otherwise the launch is plain and the list is left untouched."""
    shift = _stat_shift_for(stats[0], cout) if (stats and ROUTING.bn_stats_in_gemm) else None
    if shift is None:
        return launch()
    y, partial, ns = launch(stat_shift=shift)
    stats[:] = [partial, ns, shift, stats[0]]
    return y


def _with_bn_bwd(link, x: Tensor, launch, same_dtype: bool = False) -> Tensor:
    """BatchNorm backward reduction in the input-gradient epilogue: dx of a convolution of input `x` from `launch(**kw)`.
    link: None, or `_bn_link_of(x)` -- x is the output of a fused BatchNorm layer and dx THE gradient arriving at it; where the
    epilogue takes that layer (same shape, whole 32-channel mask words; same_dtype: the 16-bit kernels also want the layer's
    input in the gradient's dtype) the launch gets `bn_bwd` (and returns (dx, partial, n_split)) and the sums are parked for
    the layer's backward (`_note_bn_bwd`); otherwise the launch is plain."""
    if (link is not None and link[0].shape == x.shape and x.shape[1] % 32 == 0
            and (not same_dtype or link[0].dtype == x.dtype)):
        dx, partial, ns = launch(bn_bwd=link[:5])
        _note_bn_bwd(dx, link, partial, ns)
        return dx
    return launch()


def _wgrad_3x3_x6(gy: Tensor, x: Tensor, weight: Tensor, param=None, stride: int = 1, taps: int = 9):
    """d(weight) of a 3x3 / padding-1 convolution (stride 1 or 2): nine dY^T X products with X read at the pixel each tap
    points at, all in one launch that splits dY once for the nine taps (peclr_gemm_x6t_f32, taps = 9; fp32 accuracy,
    fixed-order split-K: deterministic), written in the weight's own channels_last storage order [Cout][3][3][Cin].
    taps = 1 with stride 2: the 1x1 / stride-2 shortcut convolution (X read at every second pixel)."""
    ho, wo = gy.shape[2:]

    def run():
        dw = _capi.gemm_x6t(_rows(gy), _rows(x), taps=taps, hw=(ho, wo), stride=stride, tag="conv3x3_wgrad" if taps == 9 else "conv1x1_wgrad")
        return _like_param(dw, param if param is not None else weight, taps)

    return _on_side_stream(param, (gy, x), run)


def _conv1x1_fwd(x: Tensor, weight: Tensor, conv, planes, stats, amax) -> Tensor:
    """y = x . W^T of a 1x1 / stride-1 convolution of an NHWC fp32 tensor (`_Conv1x1Gemm`, `_ForkConv1x1`): on the weight planes
    packed once per step with the consuming BatchNorm's statistics in the epilogue (stats, amax: see `_Conv1x1Gemm.forward`), or
    -- planes None: the convolution is in no pack group -- on peclr_gemm_x6_f32, which has no such epilogue."""
    n, _, h, w = x.shape
    cout, cin = weight.shape[:2]
    x2 = _rows(x)
    if planes is None:
        return _nchw(_capi.gemm_x6(x2, weight.detach().reshape(cout, cin), tag="conv1x1_fwd"), n, h, w)
    launch = functools.partial(_launch_packed, _capi.gemm_x6p, x2, conv, amax, 0, planes, cout, tag="conv1x1_fwd")
    return _nchw(_with_stats(stats, cout, launch), n, h, w)          # channels_last NCHW view of the NHWC result


def _wgrad_narrow_x6(gy: Tensor, x: Tensor, weight: Tensor, param=None, stride: int = 1, taps: int = 9):
    """d(weight) of the convolutions `_wgrad_3x3_x6` takes, for feature maps narrower than the 6 columns its padded pixel space
    needs (layer3 / layer4 of small crops): the pixels every tap points at are gathered into one [rows, taps * Cin] matrix --
    plain copies -- and dY^T X runs as ONE taps = 1 product on peclr_gemm_x6t_f32, so the result is fixed-order and
    bit-identical run to run like the wide route's.  The gather costs taps x the input, which is why this is the route of
    `routing(force=True)` only: at these sizes MIOpen's kernels are faster, but do not give the same bits on every run."""
    n, cin = x.shape[:2]
    ho, wo = gy.shape[2:]

    def run():
        xn = x.permute(0, 2, 3, 1)                                      # the NHWC storage as it lies
        if taps == 9:
            xp = F.pad(xn, (0, 0, 1, 1, 1, 1))
            cols = torch.stack([xp[:, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride] for ky in range(3) for kx in range(3)], dim=3)
        else:
            cols = xn[:, ::stride, ::stride]
        # (.contiguous(): a no-op except where a one-pixel-wide slice kept the input's row stride)
        dw = _capi.gemm_x6t(_rows(gy).contiguous(), cols.reshape(n * ho * wo, taps * cin).contiguous(), tag="conv3x3_wgrad" if taps == 9 else "conv1x1_wgrad")
        return _like_param(dw, param if param is not None else weight, taps)

    return _on_side_stream(param, (gy, x), run)


def _wgrad(gy: Tensor, x: Tensor, weight: Tensor, param, *, taps: int, stride: int, padding):
    """d(weight) of an fp32 convolution of the fused backbone -- 1x1 / stride 1 (the bottleneck entry included), 3x3 / stride 1,
    3x3 and 1x1 / stride 2 -- from the kernel that pays for its shape: THE place that decides it.  Returns dW shaped and strided
    like the parameter, or None when the gradient was parked for `param` on the side stream.
    1x1 / stride 1: dY^T X on the matrix cores where `_x6_wgrad_pays`.  The others: peclr_gemm_x6t_f32 with taps / stride
    (`_wgrad_3x3_x6`) for channels_last weights of at least 64 channels (3x3 / stride 1: 64 output channels with
    `ROUTING.x6_layer1_wgrad` -- the 64 x 64 block with two tap halves -- else 128; stride 2: both sides, and an input exactly twice
    the output) whose output is at least 6 columns wide; narrower ones take the gathered, still fixed-order form
    (`_wgrad_narrow_x6`) under `ROUTING.force` only.  Everything else: MIOpen (`_conv_wgrad`)."""
    cin, cout = x.shape[1], gy.shape[1]
    if taps == 1 and stride == 1:
        if x.dtype == torch.float32 and _x6_wgrad_pays(x.shape[0] * x.shape[2] * x.shape[3], cout, cin):
            return _wgrad_1x1_x6(gy, x, weight, param)
        return _conv_wgrad(gy, x, weight, (1, 1), padding, param)
    in_tree = ROUTING.gemm_x6t and weight.is_contiguous(memory_format=torch.channels_last) and cin % 4 == 0 and cout % 4 == 0
    if stride == 1:
        in_tree = in_tree and ROUTING.conv3x3_wgrad_x6 and cout >= (64 if ROUTING.x6_layer1_wgrad else 128)
    else:
        in_tree = (in_tree and ROUTING.conv_s2_wgrad_x6 and x.shape[2] == 2 * gy.shape[2] and x.shape[3] == 2 * gy.shape[3]
                   and cout >= 64 and cin >= 64)
    if in_tree and (x if stride == 1 else gy).shape[3] >= 6:
        return _wgrad_3x3_x6(gy, x, weight, param, stride=stride, taps=taps)
    if in_tree and ROUTING.force:             # fewer than 6 columns: the gathered, still fixed-order form
        return _wgrad_narrow_x6(gy, x, weight, param, stride=stride, taps=taps)
    return _conv_wgrad(gy, x, weight, (stride, stride), padding, param)


class _Conv1x1Gemm(torch.autograd.Function):
    """1x1 / stride-1 convolution of an NHWC fp32 tensor as the GEMM it is, on the bf16 matrix cores at fp32 accuracy:
    forward y[R, Cout] = x[R, Cin] . W^T and / or the input gradient dx[R, Cin] = dy[R, Cout] . W, each where `_x6_pays`
    (weight planes packed once per step when the convolution belongs to an X6PackGroup: peclr_gemm_x6p_f32; otherwise
    both operands split per workgroup: peclr_gemm_x6_f32); the other direction stays on MIOpen.  Weight gradient: `_wgrad`."""

    @staticmethod
    def forward(ctx, x, weight, conv, use_fwd: bool, use_bwd: bool, stats=None, link=None, amax=None):
        """stats: None, or [bn] -- the BatchNorm2d that consumes the output; the GEMM epilogue then sums its statistics
        and the list comes back as [partial, n_split, shift, bn] (left untouched when that is not possible).
        amax: the device float holding max |x| (`_absmax_of`) -> the forward runs in pair arithmetic."""
        ctx.save_for_backward(x, weight)
        planes = _x6_planes(conv) if (use_fwd or use_bwd) else None
        ctx.cfg = (conv, use_bwd, planes)
        ctx.link = link
        return _conv1x1_fwd(x, weight, conv, planes, stats, amax) if use_fwd else F.conv2d(x, weight)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        conv, use_bwd, planes = ctx.cfg
        param = conv.weight if conv is not None else None
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        gy = gy.contiguous(memory_format=torch.channels_last)
        dw = _wgrad(gy, x, weight, param, taps=1, stride=1, padding=(0, 0)) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            if use_bwd and planes is not None:
                launch = functools.partial(_launch_packed, _capi.gemm_x6p, _rows(gy), conv, _absmax_of(gy), 1, planes, cin, tag="conv1x1_dgrad")
                dx = _nchw(_with_bn_bwd(ctx.link, x, launch), n, h, w)
            elif use_bwd:
                wt = weight.detach().reshape(cout, cin).t().contiguous()          # [Cin][Cout]: K-contiguous B operand
                dx = _nchw(_capi.gemm_x6(_rows(gy), wt, tag="conv1x1_dgrad"), n, h, w)
            else:
                dx = torch.ops.aten.convolution_backward(gy, x, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                         [True, False, False])[0]
        return dx, dw, None, None, None, None, None, None


class _Conv3x3Gemm(torch.autograd.Function):
    """3x3 / stride-1 / padding-1 convolution of an NHWC fp32 tensor as an implicit GEMM on the bf16 matrix cores at
    fp32 accuracy (peclr_conv3x3_x6p_f32: rows = output pixels, K = 9 Cin in (tap, channel) order, the activation rows
    of a k-step read from the pixel its tap points at, the filter from planes packed once per step): forward and input
    gradient (the same kernel on the flipped filter); the weight gradient where `_wgrad` routes it (nine dY^T X products in one
    launch: `_wgrad_3x3_x6`)."""

    @staticmethod
    def forward(ctx, x, weight, conv, stats=None, link=None, amax=None):
        ctx.save_for_backward(x, weight)
        planes = _x6_planes(conv)
        ctx.cfg = (conv, planes)
        ctx.link = link
        cout = weight.shape[0]
        return _with_stats(stats, cout, functools.partial(_launch_packed, _capi.conv3x3_x6p, x, conv, amax, 0, planes, cout, tag="conv3x3_fwd",
                                                          rows_six_pair=(ROUTING.conv3x3_tile_rows, ROUTING.conv3x3_pair_tile_rows)))

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        conv, planes = ctx.cfg
        gy = gy.contiguous(memory_format=torch.channels_last)
        dw = _wgrad(gy, x, weight, conv.weight, taps=9, stride=1, padding=(1, 1)) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _with_bn_bwd(ctx.link, x, functools.partial(
                _launch_packed, _capi.conv3x3_x6p, gy, conv, _absmax_of(gy), 1, planes, x.shape[1], flip=True, tag="conv3x3_dgrad",
                rows_six_pair=(ROUTING.conv3x3_tile_rows, ROUTING.conv3x3_pair_tile_rows)))
        return dx, dw, None, None, None, None


class _ConvS2Gemm(torch.autograd.Function):
    """Stride-2 3x3 (padding 1) / 1x1 convolution of an NHWC fp32 tensor: forward on the six-product kernel
    (peclr_conv_s2_x6p_f32: the k-step's tap and the stride select the source pixel; BatchNorm statistics of the output
    in the epilogue), weight gradient where `_wgrad` routes it (peclr_gemm_x6t_f32 with stride 2).  Input gradient: 3x3 -- one
    dense implicit GEMM per parity class of input pixels (peclr_conv3x3_s2_dgrad_x6p_f32); 1x1 shortcut -- kept compact for the
    block's entry-gradient GEMM where that is its consumer, else scattered into zeros (`_shortcut_grad`); MIOpen where the input
    is not exactly twice the output."""

    @staticmethod
    def forward(ctx, x, weight, conv, stats=None, compact=False, link=None, amax=None):
        ctx.save_for_backward(x, weight)
        ctx.conv = conv
        ctx.compact = compact
        ctx.link = link
        planes = _x6_planes(conv)
        cout, taps = weight.shape[0], weight.shape[2] * weight.shape[3]
        return _with_stats(stats, cout, functools.partial(_launch_packed, _capi.conv_s2_x6p, x, conv, amax, 0, planes, cout, taps,
                                                          tag="conv_s2_fwd", tile_rows=ROUTING.s2_tile_rows if taps == 9 else 0))

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        conv = ctx.conv
        gy = gy.contiguous(memory_format=torch.channels_last)
        pad = list(conv.padding)
        taps = weight.shape[2] * weight.shape[3]
        dw = _wgrad(gy, x, weight, conv.weight, taps=taps, stride=2, padding=pad) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            halved = x.shape[2] == 2 * gy.shape[2] and x.shape[3] == 2 * gy.shape[3]       # the input is exactly twice the output
            if weight.shape[2] == 1 and halved:
                # 1x1 shortcut: dY . W over the OUTPUT pixels only (three quarters of the input gradient are zeros).  Where it
                # goes straight into the block's fused entry gradient it stays compact (the consumer adds it at the even
                # pixels: no 4x larger tensor); elsewhere (BasicBlock networks: the block input is a plain tensor) it is
                # scattered into zeros here -- never MIOpen's input gradient, whose fp32 1x1 / stride-2 solver adds with float
                # atomics (a different last bit every run: tools/exp/two_outcome.py)
                dc = _launch_packed(_capi.gemm_x6p, _rows(gy), conv, _absmax_of(gy), 1, _x6_planes(conv), x.shape[1], tag="conv_s2_dgrad")
                dx = _shortcut_grad(dc, x.shape, ctx.compact)
            elif ROUTING.conv_s2_dgrad_x6 and weight.shape[2] == 3 and halved and x.shape[1] % 64 == 0 and gy.shape[1] % 16 == 0:
                # 3x3: one dense implicit GEMM per parity class of input pixels (1, 2, 2, 4 taps); dx is the gradient arriving
                # at the BatchNorm layer whose output x is: reduced in the epilogue
                dx = _with_bn_bwd(ctx.link, x, functools.partial(_launch_packed, _capi.conv3x3_s2_dgrad_x6p, gy, conv, _absmax_of(gy), 1,
                                                                 _x6_planes(conv), x.shape[1], tile_rows=ROUTING.s2_tile_rows))
            else:
                dx = torch.ops.aten.convolution_backward(gy, x, weight, None, [2, 2], pad, [1, 1], False, [0, 0], 1, [True, False, False])[0]
        return dx, dw, None, None, None, None, None


# ---- gradients handed to a block's entry-gradient GEMM in another form than a dense tensor.  An autograd function may only
# return a tensor of its input's shape.  Two producers would write such a tensor only for `_ForkConv1x1.backward` to read it
# back as its addend: the 1x1 / stride-2 shortcut of a layer's first block (three quarters of its input gradient are zeros:
# the compact [N, H/2, W/2, C] product is all there is to it) and the last BatchNorm of a block with an identity shortcut
# (the residual's gradient is relu'(out) * d(out): the GEMM can read d(out) and the 1-bit mask itself).  When their input is
# the identity output of `_ForkConv1x1` (whose backward is the only consumer of that gradient, and understands the
# protocol), they return a zero-stride NaN view of the right shape instead -- no memory, and loudly wrong should anything
# else ever consume or accumulate it -- and park the real payload here under the view's address.
_COMPACT = {}
_NAN_RING = {}


def _lazy_grad(payload, shape, device, dtype=torch.float32) -> Tensor:
    ring = _NAN_RING.get((device, dtype))        # (autograd casts a gradient of another dtype: that would materialise the view)
    if ring is None:
        ring = _NAN_RING[(device, dtype)] = [torch.full((64,), float("nan"), device=device, dtype=dtype), 0]
    buf, at = ring
    ring[1] = (at + 1) % 64
    sentinel = buf[at:at + 1].view(1, 1, 1, 1).expand(shape)
    _COMPACT[sentinel.data_ptr()] = (payload, tuple(shape))
    _drain_after_backward()
    return sentinel


def _compact_grad(dc: Tensor, shape) -> Tensor:
    return _lazy_grad(("s2", dc), shape, dc.device, dc.dtype)


def _shortcut_grad(dc: Tensor, shape, compact: bool) -> Tensor:
    """The input gradient (of `shape`) of a 1x1 / stride-2 shortcut convolution from its compact product `dc`: handed over compact
    where the consumer takes that form (`compact`: the block's entry-gradient GEMM) -- not under anomaly mode, whose checks would
    meet the NaN view -- else scattered into zeros."""
    return _compact_grad(dc, shape) if (compact and not torch.is_anomaly_enabled()) else _expand_compact(dc, shape)


def _take_lazy(g: Tensor):
    """The parked payload -- ("s2", compact gradient), ("mask", dy, bit mask) or ("bn", dx, dgamma, dbeta, absmax slot, hand-over
    record: a shortcut BatchNorm layer's finished gradients, `_BN2dAct.backward`) -- if `g` is one of `_lazy_grad`'s views."""
    # (a view expanded from one element: zero strides -- except along dimensions of size 1, which keep the element's own stride:
    # a [N, C, 1, 1] gradient arrives with strides (0, 0, 1, 1))
    if g is None or g.dim() != 4 or not _COMPACT or any(st for st, n in zip(g.stride(), g.shape) if n != 1):
        return None
    hit = _COMPACT.get(g.data_ptr())
    if hit is None or hit[1] != tuple(g.shape):
        return None
    del _COMPACT[g.data_ptr()]
    return hit[0]


def _take_compact(g: Tensor):
    hit = _take_lazy(g)
    return None if hit is None else _dense_of(hit, g.shape) if hit[0] != "s2" else hit[1]


def _dense_of(payload, shape) -> Tensor:
    """The dense gradient a payload stands for (fallback paths)."""
    if payload[0] == "s2":
        return _expand_compact(payload[1], shape)
    if payload[0] != "mask":
        # ("bn": a shortcut BatchNorm layer's finished gradients -- only that layer's own node may take them)
        raise _capi.PeclrHipError(f"a {payload[0]!r} gradient hand-over reached a consumer that cannot take it")
    _, dy, mask = payload
    n, c, h, w = shape
    bits = (mask.view(n * h * w, c // 32, 1) >> torch.arange(32, device=mask.device, dtype=torch.int32)) & 1
    return _nchw(_rows(dy) * bits.view(n * h * w, c).to(dy.dtype), n, h, w)


def _expand_compact(dc: Tensor, shape) -> Tensor:
    """The dense form (fallback paths): zeros with the compact gradient at the even pixels."""
    n, c, h, w = shape
    full = torch.zeros(shape, device=dc.device, dtype=dc.dtype).contiguous(memory_format=torch.channels_last)
    full[:, :, ::2, ::2] = _nchw(dc, n, h // 2, w // 2)
    return full


def _bn_link_of(x: Tensor):
    """(x_bn, save, scale_shift, mask, relu, token) if `x` is the output of a fused BatchNorm layer whose backward reduction
    a consumer's input-gradient GEMM may perform, else None."""
    link = getattr(x, "_peclr_bn_link", None)
    return tuple(link) if link and ROUTING.bn_bwd_in_gemm else None


_DRAIN_QUEUED = False
_NESTED_BACKWARD = 0       # > 0 inside the backward pass a checkpointed block runs over its re-run graph


def _drain_after_backward():
    """Called by the producers of side-channel entries (they run inside a backward pass): have the autograd engine call
    `end_backward()` when THIS backward pass is over, so that any training loop -- not only `Trainer`, which also calls it --
    leaves no stale entry pinning device tensors behind (should a pass end without running its callbacks, the token / version
    checks still keep a stale entry from ever being used, and the next pass drains it)."""
    global _DRAIN_QUEUED
    if _DRAIN_QUEUED or _NESTED_BACKWARD:
        return
    try:
        torch.autograd.Variable._execution_engine.queue_callback(_drained)
        _DRAIN_QUEUED = True          # (reset by the callback -- or by end_backward(), should a pass raise and skip its callbacks)
    except RuntimeError:        # not inside a backward pass (a kernel-level test calling a backward function by hand)
        pass


last_backward_leftovers = 0     # entries the engine-queued drain of the most recent backward pass had to drop (0 for the in-tree ResNets)


def _drained():
    global _DRAIN_QUEUED, last_backward_leftovers
    _DRAIN_QUEUED = False
    last_backward_leftovers = end_backward()


def _note_bn_bwd(dx: Tensor, link, partial, ns):
    _BN_BWD_STATS[dx.data_ptr()] = (link[5], partial, ns, dx._version)
    _drain_after_backward()


def end_backward(strict: bool = False) -> int:
    """After every backward pass (the Trainer calls it): drop what the side channels still hold -- a BatchNorm reduction
    whose gradient tensor was merged into another consumer's buffer and never arrived under its own address, a lazy
    payload whose NaN view nobody took -- so that nothing pins device memory or meets a recycled address later.  Returns
    the number of entries dropped; strict=True raises instead (tests: the in-tree ResNets leave none behind)."""
    global _DRAIN_QUEUED
    _DRAIN_QUEUED = False        # (a pass that raised skipped its engine callbacks: the next one queues its drain again)
    n = len(_BN_BWD_STATS) + len(_COMPACT)
    _BN_BWD_STATS.clear()
    _COMPACT.clear()
    if n and strict:
        raise _capi.PeclrHipError(f"{n} gradient hand-overs were never consumed")
    return n


def _attach_stats(y: Tensor, stats):
    """Hand the statistics a GEMM epilogue summed to the BatchNorm that consumes `y` (FusedBatchNormAct2d.forward looks for them)."""
    if stats is not None and len(stats) == 4:
        y._peclr_bn_stats = tuple(stats)
    return y


def _wgrad_h(gy: Tensor, x: Tensor, conv, stride: int):
    """d(weight) (fp32, the parameter's layout) of a 16-bit convolution.  In-tree (peclr_wgrad_h: fixed-order slabs, fp32
    out straight into the master weight's layout) where the kernel takes the shape, else MIOpen's 16-bit weight gradient
    (+ its cast to fp32)."""
    w = conv.weight
    taps = w.shape[2] * w.shape[3]
    wide = taps == 9 and gy.shape[3] > _capi.WGRAD3_MAX_W              # rows the one-ring kernel refuses: `wgrad16_wide`
    if (ROUTING.wgrad16 and (ROUTING.wgrad16_wide or not wide) and w.is_contiguous(memory_format=torch.channels_last)
            and _capi.wgrad_h_ok(gy, x, taps, stride)):
        return _on_side_stream(w, (gy, x), lambda: _like_param(_capi.wgrad_h(gy, x, taps, stride), w, taps))     # [Cout, taps * Cin] fp32
    # the 3x3 / stride-2 ones that open layers 2 - 4 (peclr_wgrad3s2_h; `force` does not widen the predicate)
    if (ROUTING.wgrad16 and ROUTING.wgrad16_s2 and taps == 9 and w.shape[2] == 3 and stride == 2 and tuple(conv.padding) == (1, 1)
            and w.is_contiguous(memory_format=torch.channels_last) and _capi.wgrad3_s2_h_ok(gy, x)):
        return _on_side_stream(w, (gy, x), lambda: _like_param(_capi.wgrad3_s2_h(gy, x), w, taps))
    return _conv_wgrad(gy, x, w, conv.stride, conv.padding, w)


class _ConvH(torch.autograd.Function):
    """A residual block's convolution on 16-bit (bf16 / fp16 autocast) NHWC activations, in-tree (csrc/conv_h.hip): 1x1 or
    3x3 / padding 1, stride 1 or 2 -- forward with the consuming BatchNorm's statistics in the epilogue, input gradient with
    the producing BatchNorm's backward reduction in the epilogue, both from weight planes packed once per step out of the
    fp32 master weights.  Same hand-over protocols as the fp32 classes above (`stats`, `link`, `_shortcut_grad`)."""

    @staticmethod
    def forward(ctx, x, weight, conv, stats=None, link=None, compact=False):
        ctx.save_for_backward(x)
        ctx.conv, ctx.link, ctx.compact = conv, link, compact
        planes = conv.x6_group.planes(conv, x.dtype)
        ctx.planes = planes
        cout, taps, stride = conv.out_channels, conv.kernel_size[0] * conv.kernel_size[1], conv.stride[0]
        n, _, h, w = x.shape
        if taps == 1 and stride == 1:
            return _nchw(_with_stats(stats, cout, lambda **kw: _capi.gemm_h(_rows(x), planes[0], cout, tag="conv1x1_fwd", **kw)), n, h, w)
        tag = "conv3x3_fwd" if stride == 1 else "conv_s2_fwd"
        return _with_stats(stats, cout, lambda **kw: _capi.conv_h(x, planes[0], cout, taps=taps, stride=stride, tag=tag, **kw))

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        conv, planes, link = ctx.conv, ctx.planes, ctx.link
        gy = gy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        n, cin, h, w = x.shape
        taps, stride = conv.kernel_size[0] * conv.kernel_size[1], conv.stride[0]
        dw = _wgrad_h(gy, x, conv, stride) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            if taps == 1 and stride == 1:
                dx = _nchw(_with_bn_bwd(link, x, lambda **kw: _capi.gemm_h(_rows(gy), planes[1], cin, tag="conv1x1_dgrad", **kw),
                                        same_dtype=True), n, h, w)
            elif taps == 9 and stride == 1:
                dx = _with_bn_bwd(link, x, lambda **kw: _capi.conv_h(gy, planes[1], cin, flip=True, tag="conv3x3_dgrad", **kw),
                                  same_dtype=True)
            elif taps == 9:
                dx = _with_bn_bwd(link, x, lambda **kw: _capi.conv3x3_s2_dgrad_h(gy, planes[1], cin, **kw), same_dtype=True)
            elif h == 2 * gy.shape[2] and w == 2 * gy.shape[3]:
                # 1x1 / stride-2 shortcut: dY . W over the OUTPUT pixels only; the block's entry-gradient GEMM adds it at the even
                # pixels, any other consumer gets it scattered into zeros (deterministic, unlike MIOpen's atomics)
                dc = _capi.gemm_h(_rows(gy), planes[1], cin, tag="conv_s2_dgrad")
                dx = _shortcut_grad(dc, x.shape, ctx.compact)
            else:
                dx = torch.ops.aten.convolution_backward(gy, x, conv.weight.detach().to(x.dtype), None, [2, 2], [0, 0], [1, 1], False,
                                                         [0, 0], 1, [True, False, False])[0]
        return dx, dw, None, None, None, None


def _stem_wgrad(gy: Tensor, x: Tensor, param):
    """d(weight) of the stem (peclr_stem_wgrad: fixed-order slabs, fp32 gradient of the fp32 master weight) in the parameter's
    memory format; parked for `param` on the side stream when that mode is on."""
    def run():
        dw = _capi.stem_wgrad(gy, x)
        return torch.empty_like(param).copy_(dw)                   # (9 408 elements: into the parameter's own strides)

    return _on_side_stream(param, (gy, x), run)


class _StemConv(torch.autograd.Function):
    """The encoder's 7x7 / stride-2 / padding-3 stem on fp32 NHWC images, in-tree (peclr_stem_conv7x7_s2): fp32 output at fp32
    accuracy, or -- under bf16 / fp16 autocast -- 16-bit output from the operands rounded inside the kernel (no cast pass over
    the images); the statistics of the BatchNorm behind it in the epilogue.  Weight gradient: peclr_stem_wgrad (the images need no
    gradient; one that is asked for comes from MIOpen)."""

    @staticmethod
    def forward(ctx, x, weight, conv, stats=None):
        half = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
        dtype = half if half in _HALF else torch.float32
        planes = conv._stem_planes(dtype)
        ctx.save_for_backward(x, weight)
        ctx.conv, ctx.dtype = conv, dtype
        return _with_stats(stats, 64, lambda **kw: _capi.stem_conv(x, planes, **kw))

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        conv = ctx.conv
        gy = gy.to(ctx.dtype).contiguous(memory_format=torch.channels_last)
        dw = None
        if ctx.needs_input_grad[1]:
            if ROUTING.stem_wgrad:
                dw = _stem_wgrad(gy, x, conv.weight)
            else:
                xin = x if ctx.dtype == torch.float32 else x.to(ctx.dtype)          # (what autocast's convolution saw)
                dw = _conv_wgrad(gy, xin, weight, (2, 2), (3, 3), conv.weight)
        dx = None
        if ctx.needs_input_grad[0]:
            xin = x if ctx.dtype == torch.float32 else x.to(ctx.dtype)
            dx = torch.ops.aten.convolution_backward(gy, xin, weight.to(ctx.dtype), None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0].to(x.dtype)
        if dw is not None and dw.dtype != weight.dtype:
            dw = dw.to(weight.dtype)
        return dx, dw, None, None


class Conv2d(nn.Conv2d):
    """nn.Conv2d (same parameters / state_dict) that routes through `_Conv2dSplitBackward` while the side-stream
    weight gradients are enabled and the input is a channels_last HIP tensor; the stock op otherwise."""

    hip_gemm = False   # enable_hip_batchnorm: fp32 1x1 / stride-1 convolutions as GEMMs on the bf16 matrix cores
    hip_stem = False   # enable_hip_batchnorm: this is the 7x7 / stride-2 stem of 3-channel images (csrc/stem.hip)
    STEM_MISSING = ("stem: the filter planes of this precision do not exist yet and cannot be created while a "
                    "hipGraph is being captured -- run one eager forward pass (same autocast dtype) first")

    def _stem_planes(self, dtype):
        """The stem filter packed for `dtype` (fp32: three bf16 planes; bf16 / fp16: one plane), fresh: re-packed when the weight
        changed since the last pack and once per hipGraph capture (`_PackedOnce`, one per dtype)."""
        st = self.__dict__.setdefault("_stem_sets", {}).setdefault(dtype, _PackedOnce())
        w = self.weight
        return st.fresh(w, 0, lambda: st.pack([w], lambda: _capi.StemPlanes(w.detach(), dtype), self.STEM_MISSING))

    def _in_tree(self, x: Tensor, stats, bn_link):
        """conv(x) on the in-tree arm that takes it -- the stem, the 16-bit kernels, fp32 1x1 / stride 1, stride 2, 3x3 / stride 1, in
        that order; each arm has its own eligibility test and its own rule for the BatchNorm hand-over `link` -- or None: no arm does.
        stats: None or [bn], for the arm's epilogue (`_with_stats`); bn_link: `_bn_link_of`, or a function returning None."""
        if (self.hip_stem and ROUTING.stem and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
                and x.shape[2] >= 8 and x.shape[3] >= 8 and x.is_contiguous(memory_format=torch.channels_last)
                and self.weight.is_cuda and self.weight.dtype == torch.float32):
            return _StemConv.apply(x, self.weight, self, stats)
        grad = torch.is_grad_enabled() and x.requires_grad
        # a 1x1 / stride-2 shortcut whose input gradient goes straight into the block's entry-gradient GEMM hands it over compact
        compact = (ROUTING.s2_dgrad_compact and self.kernel_size == (1, 1) and self.stride == (2, 2)
                   and getattr(x, "_peclr_compact_ok", False) and grad)
        if self.hip_gemm and _h_ok(self, x) and (x.shape[2] % self.stride[0] == 0 and x.shape[3] % self.stride[1] == 0):
            return _ConvH.apply(x, self.weight, self, stats, bn_link(x) if grad else None, compact)
        # what every fp32 in-tree arm below needs of its input: an NHWC fp32 device tensor outside autocast
        fp32 = (self.hip_gemm and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled("cuda") and x.dim() == 4
                and x.is_contiguous(memory_format=torch.channels_last))
        if (fp32 and self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding == (0, 0) and self.groups == 1
                and self.bias is None):
            rows = x.shape[0] * x.shape[2] * x.shape[3]
            use_fwd = _x6_pays(rows, self.out_channels, self.in_channels)
            use_bwd = _x6_pays(rows, self.in_channels, self.out_channels) and grad
            use_wgrad = (_x6_wgrad_pays(rows, self.out_channels, self.in_channels) and torch.is_grad_enabled()
                         and self.weight.requires_grad)
            if use_fwd or use_bwd or use_wgrad:
                return _Conv1x1Gemm.apply(x, self.weight, self, use_fwd, use_bwd, stats if use_fwd else None,
                                          bn_link(x) if use_bwd else None, _absmax_of(x))
        if (fp32 and ROUTING.conv_s2_x6 and ROUTING.gemm_x6p and getattr(self, "x6_group", None) is not None and self.stride == (2, 2)
                and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
                and (x.shape[0] * x.shape[2] * x.shape[3] >= 32768 or ROUTING.force)):
            link = bn_link(x) if (grad and self.kernel_size == (3, 3)) else None
            return _ConvS2Gemm.apply(x, self.weight, self, stats, compact, link, _absmax_of(x))
        if (fp32 and ROUTING.conv3x3_x6 and ROUTING.gemm_x6p and getattr(self, "x6_group", None) is not None and self.kernel_size == (3, 3)
                and self.stride == (1, 1)
                and (x.shape[0] * x.shape[2] * x.shape[3] >= 8192 or ROUTING.force)):
            return _Conv3x3Gemm.apply(x, self.weight, self, stats, bn_link(x), _absmax_of(x))
        return None

    def forward(self, x: Tensor, stats_for=None, sole_consumer: bool = False) -> Tensor:
        """stats_for: the BatchNorm2d that consumes the output -- when this convolution runs as an in-tree GEMM its
        epilogue sums that layer's training statistics (one pass over the activation less).
        sole_consumer: the caller guarantees that NOTHING else reads `x` (bn -> conv inside a residual block): only then
        is this convolution's input gradient THE gradient arriving at the BatchNorm layer that produced x, and only then
        may the input-gradient GEMM perform that layer's backward reduction in its epilogue.  A block input (x also feeds
        the shortcut) is not: BasicBlock.conv1 passes False."""
        deferred = getattr(x, "_peclr_deferred", None)
        if deferred is not None:
            x = _materialized(x, tuple(deferred))       # a BatchNorm layer's placeholder (its apply pass was left to another reader): written after all
        stats = [stats_for] if stats_for is not None else None
        y = self._in_tree(x, stats, _bn_link_of if sole_consumer else (lambda t: None))
        if y is not None:
            return _attach_stats(y, stats)              # (the ONE place the epilogue's statistics are handed on)
        if (_overlap_stream() is not None and x.is_cuda and torch.is_grad_enabled() and self.bias is None
                and self.groups == 1 and self.dilation == (1, 1) and isinstance(self.padding, tuple)
                and x.is_contiguous(memory_format=torch.channels_last) and self.weight.requires_grad):
            w = self.weight
            if torch.is_autocast_enabled("cuda"):
                half = torch.get_autocast_dtype("cuda")
                x, w = x.to(half), w.to(half)            # what autocast does for conv2d
            return _Conv2dSplitBackward.apply(x, w, self.stride, self.padding, self.weight)
        return super().forward(x)


def _entry_gemm(a: Tensor, planes: Tensor, n: int, addend=None, **kw):
    """The block's entry gradient a . W (+ the shortcut's gradient, + the BatchNorm backward reduction): peclr_gemm_x6p_f32.
    (Round 5 tried a barrier-free streaming kernel for the HBM-bound shapes here -- tools/exp/gemm_x6s.hip, bit-identical
    output -- and measured it slower: docs/history.md.)"""
    return _capi.gemm_x6p(a, planes, n, addend, tag="conv1x1_dgrad_add_x6", **kw)


def _entry_addend(gid: Tensor, lazy, x: Tensor) -> dict:
    """The addend keywords of a block's entry-gradient GEMM (peclr_gemm_x6p_f32 / peclr_gemm_h) for the identity branch's gradient
    `gid` of the block input `x`: dense rows, or -- lazy = `_take_lazy(gid)` -- the compact gradient of a stride-2 shortcut (added
    at the even pixels) / the (dy, mask) pair of an identity shortcut."""
    if lazy is None:
        return dict(addend=_rows(gid.to(x.dtype).contiguous(memory_format=torch.channels_last)))
    if lazy[0] == "s2":
        return dict(addend=lazy[1], addend_s2=tuple(x.shape[2:]))
    return dict(addend=_rows(lazy[1].contiguous(memory_format=torch.channels_last)), addend_mask=lazy[2])


class _ForkConv1x1(torch.autograd.Function):
    """Bottleneck entry: (x, W) -> (conv1x1(x, W), x).  The block input feeds both the first convolution and
    the identity branch, so its gradient is dY W + d_identity: autograd runs MIOpen's dgrad and then an
    elementwise add over the block input (3.6 % of the fp32 step); here both are ONE fp32 GEMM with the
    identity gradient added in the epilogue.  Small shapes' forward stays on MIOpen; the weight gradient goes where `_wgrad`
    routes it."""

    @staticmethod
    def forward(ctx, x, weight, conv, stats=None, link=None, flags=None, amax=None):
        ctx.save_for_backward(x, weight)
        ctx.param = weight if isinstance(weight, nn.Parameter) else None
        ctx.link = link
        ctx.conv = conv
        n, cin, h, w = x.shape
        cmid = weight.shape[0]
        r = n * h * w
        use_fwd = x.dtype == torch.float32 and _x6_pays(r, cmid, cin)
        # (two rounds of the chip's CUs: below that MIOpen's dgrad + the elementwise add are not slower)
        use_bwd = (x.dtype == torch.float32 and ROUTING.gemm_x6 and cin >= 128 and ROUTING.fills_chip(r, cin, rounds=2.0)
                   and (cmid >= ROUTING.x6_min_k or (ROUTING.x6_layer1_fork and ROUTING.gemm_x6p and ROUTING.streams_from_hbm(r, cmid, cin)
                                                     and cmid >= 64 and cmid % 16 == 0 and cin % 128 == 0)))
        ctx.planes = _x6_planes(conv) if (use_fwd or use_bwd) else None
        ctx.use_bwd = use_bwd
        if flags is not None:       # tells fork_conv1x1 whether the backward takes compact shortcut gradients (the x6p GEMM)
            flags.append(bool(use_bwd and ctx.planes is not None))
        return (_conv1x1_fwd(x, weight, conv, ctx.planes, stats, amax) if use_fwd else F.conv2d(x, weight)), x.view_as(x)

    @staticmethod
    def backward(ctx, gy, gid):
        x, weight = ctx.saved_tensors
        n, cin, h, w = x.shape
        cmid = weight.shape[0]
        dw = None
        gy = gy.to(x.dtype)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(gy.contiguous(memory_format=torch.channels_last), x, weight, ctx.param, taps=1, stride=1, padding=(0, 0))
        dx = None
        if ctx.needs_input_grad[0]:
            gy = gy.contiguous(memory_format=torch.channels_last)
            a = _rows(gy)                   # NHWC storage seen as [R, Cmid]: a view
            lazy = _take_lazy(gid)          # the shortcut's gradient in its compact / (dy, mask) form (see `_lazy_grad`)
            if ctx.use_bwd and ctx.planes is not None:
                # fp32 on the bf16 matrix cores (exact 3-way split, six products; `use_bwd`: fp32 only), weight planes packed once
                # per step; the result is the gradient arriving at the previous block's last BatchNorm: reduced in the epilogue
                out = _with_bn_bwd(ctx.link, x, functools.partial(_launch_packed, _entry_gemm, a, ctx.conv, _absmax_of(gy), 1, ctx.planes, cin,
                                                                  **_entry_addend(gid, lazy, x)))
            else:
                dense = gid if lazy is None else _dense_of(lazy, x.shape)        # (these kernels add a dense tensor only)
                d = _rows(dense.to(x.dtype).contiguous(memory_format=torch.channels_last))
                if x.dtype in _HALF:             # autocast backbone: 16-bit MFMA, fp32 accumulate
                    wt = torch.empty((cin, cmid), device=x.device, dtype=x.dtype)
                    wt.copy_(weight.detach().reshape(cmid, cin).t())      # transpose + cast in ONE launch
                    out = _capi.gemm_add_half(a, wt, d, tag="conv1x1_dgrad_add")
                elif ctx.use_bwd:
                    wt = weight.detach().reshape(cmid, cin).t().contiguous()
                    out = _capi.gemm_x6(a, wt, d, tag="conv1x1_dgrad_add_x6")
                else:
                    out = _capi.gemm_add(_capi.GEMM_NN, a, weight.reshape(cmid, cin), d, tag="conv1x1_dgrad_add")
            dx = _nchw(out, n, h, w)        # back to a channels_last NCHW tensor
        return dx, dw, None, None, None, None, None


class _ForkConvH(torch.autograd.Function):
    """Bottleneck entry on 16-bit activations, in-tree: (x, W) -> (conv1x1(x, W), x); forward with bn1's statistics, backward
    dY . W + the shortcut's gradient (dense, compact stride-2 or (dy, mask)) as ONE GEMM with the previous block's bn3
    backward reduction in its epilogue (peclr_gemm_h)."""

    @staticmethod
    def forward(ctx, x, weight, conv, stats=None, link=None):
        ctx.save_for_backward(x)
        ctx.conv, ctx.link = conv, link
        planes = ctx.planes = conv.x6_group.planes(conv, x.dtype)
        n, _, h, w = x.shape
        cmid = conv.out_channels
        y = _with_stats(stats, cmid, lambda **kw: _capi.gemm_h(_rows(x), planes[0], cmid, tag="conv1x1_fwd", **kw))
        return _nchw(y, n, h, w), x.view_as(x)

    @staticmethod
    def backward(ctx, gy, gid):
        (x,) = ctx.saved_tensors
        conv, planes, link = ctx.conv, ctx.planes, ctx.link
        n, cin, h, w = x.shape
        gy = gy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        dw = _wgrad_h(gy, x, conv, 1) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            addend = _entry_addend(gid, _take_lazy(gid), x)
            dx = _nchw(_with_bn_bwd(link, x, lambda **kw: _capi.gemm_h(_rows(gy), planes[1], cin, tag="conv1x1_dgrad_add", **addend, **kw),
                                    same_dtype=True), n, h, w)
        return dx, dw, None, None, None


def fork_conv1x1(conv: nn.Conv2d, x: Tensor, stats_for=None):
    """`(conv(x), x)` with the fused input gradient when `conv.hip_fork` is set (enable_hip_batchnorm does
    it for the bottlenecks' first 1x1 convolution) and the activations are channels_last on a HIP device,
    fp32 (no autocast) or bf16 (under bf16 autocast); the stock ops otherwise."""
    autocast = torch.is_autocast_enabled("cuda")
    dtype_ok = ((x.dtype == torch.float32 and not autocast)
                or (x.dtype in (torch.bfloat16, torch.float16) and autocast and torch.get_autocast_dtype("cuda") == x.dtype))
    ok = (getattr(conv, "hip_fork", False) and x.is_cuda and dtype_ok
          and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
          and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is None and x.requires_grad
          and x.is_contiguous(memory_format=torch.channels_last)
          and conv.weight.shape[0] % 8 == 0 and conv.weight.shape[1] % 8 == 0)
    if ok:
        stats = [stats_for] if stats_for is not None else None
        if _h_ok(conv, x):
            out, identity = _ForkConvH.apply(x, conv.weight, conv, stats, _bn_link_of(x))
            identity._peclr_compact_ok = True         # its backward takes the shortcut's gradient compact / as (dy, mask)
        else:
            flags, amax = [], _absmax_of(x)
            out, identity = _ForkConv1x1.apply(x, conv.weight, conv, stats, _bn_link_of(x), flags, amax)
            _tagged(identity, amax)                   # (the same values: the downsample convolution reads them too)
            if flags and flags[0]:
                identity._peclr_compact_ok = True     # a 1x1 / stride-2 shortcut may hand its input gradient over compact
        return _attach_stats(out, stats), identity
    return (conv(x, stats_for=stats_for) if isinstance(conv, Conv2d) else conv(x)), x     # (x has two consumers: no link)


class FusedBatchNormAct2d(nn.BatchNorm2d):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, **kw):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine,
                         track_running_stats=track_running_stats, **kw)
        self.hip = False
        self.default_relu = False  # stem BN inside an nn.Sequential: fuse the ReLU that follows it
        self.default_pool = False  # ... and the MaxPool2d(3, 2, 1) after that (the encoder's stem)
        # last BatchNorm of layer4 inside the encoder wrapper: in HIP mode its fused pass also performs the
        # AdaptiveAvgPool2d((1, 1)) + flatten that follow the block and returns fp32 [N, C]
        self.tail_avgpool = False
        # data parallel: a process group -> training statistics over the rows of ALL its ranks (what one
        # device holding the concatenated batch computes); None -> per-rank statistics (DDP's default)
        self.sync_group = None

    def _stat_buffers(self, training: bool):
        """(running_mean, running_var, num_batches_tracked, sync_shift) for the kernels.  The running statistics are
        NOT handed over while a checkpointed block is being re-run in the backward pass (the first run already moved
        them).  Synchronised statistics subtract a common shift -- the replicated running mean -- before summing: the
        first run keeps the copy it used, and the re-run gets that copy (the running mean has moved since) so that it
        reproduces the first run's statistics exactly and updates nothing."""
        sync = training and self.sync_group is not None
        if training and _RECOMPUTING:
            return None, None, None, (_ckpt_shift_of(self) if sync else None)
        shift = None
        if sync:
            shift = _ckpt_shift_of(self)         # (first run of a checkpointed block: the copy kept for its re-run)
            if shift is None:
                shift = self.running_mean.detach().clone()
        return self.running_mean, self.running_var, self.num_batches_tracked, shift

    def _fwd_args(self, pre):
        """What the three fused forwards hand their kernel about this layer: (training, sync group, the positional block
        (running_mean, running_var, num_batches_tracked, training, eps, momentum), the keywords sync_group / sync_shift / pre);
        `pre`: the statistics a producer's epilogue summed (training only)."""
        training = self.training or not self.track_running_stats
        sync = self.sync_group if training else None
        rm, rv, nbt, shift = self._stat_buffers(training)
        return (training, sync, (rm, rv, nbt, training, self.eps, self.momentum if self.momentum is not None else 0.1),
                dict(sync_group=sync, sync_shift=shift, pre=pre if training else None))

    def _takes_deferred_residual(self, x: Tensor) -> bool:
        """Can this layer's pass compute the shortcut's BatchNorm itself (peclr_bn2d_apply_res_bn)?  The plain fused pass only
        (not the stem's pooled form, not layer4's average-pooled tail)."""
        return bool(ROUTING.bn_shortcut_in_add and self.hip and self.affine and x.is_cuda and x.dim() == 4
                    and x.dtype in (torch.float32, torch.bfloat16, torch.float16)
                    and not (self.tail_avgpool and self.num_features % 32 == 0) and not self.default_pool)

    def forward(self, x: Tensor, residual: Optional[Tensor] = None, relu: Optional[bool] = None, consumer=None) -> Tensor:
        """consumer: the ONLY reader of the result.  For the BatchNorm of a shortcut (conv1x1 -> bn, no ReLU) it is the block's
        last FusedBatchNormAct2d, which adds the shortcut in its own pass (`_takes_deferred_residual`): the layer then only
        finishes its statistics and returns a placeholder carrying `_peclr_deferred = [x, scale_shift, relu, hand-over record]`: no
        apply pass, no output tensor.  A residual that is such a placeholder is computed on the fly (or materialised), and the
        consumer's backward then performs this layer's backward too (`_dual_backward_ok`).  (A Conv2d consumer that
        applied the layer in its own operand path was built in round 5 and taken out in round 6: docs/history.md E.)"""
        relu = self.default_relu if relu is None else relu
        pool = self.default_pool and relu and residual is None
        if self.hip:
            global _DRAIN_QUEUED
            if _DRAIN_QUEUED and not _RECOMPUTING and not _NESTED_BACKWARD:
                # a forward pass outside any backward: the drain queued by the last backward pass never ran (that pass raised, and
                # autograd skips its final callbacks then) -- loops that do not call end_backward() would never queue one again
                _DRAIN_QUEUED = False
                end_backward()
            if not self.affine or (self.training and self.momentum is None):
                raise _capi.PeclrHipError("fused BatchNorm2d needs affine=True and a fixed momentum")
            # statistics its producer already summed (a GEMM epilogue, `conv_stats_for`), valid for THIS layer in training
            pre = getattr(x, "_peclr_bn_stats", None)
            if pre is not None and (pre[3] is not self or not (self.training or not self.track_running_stats)):
                pre = None
            pre = pre[:3] if pre is not None else None
            # a residual that is the placeholder of the shortcut's BatchNorm: computed inside this layer's pass, or written after all
            res_deferred = getattr(residual, "_peclr_deferred", None) if residual is not None else None
            if res_deferred is not None:
                res_deferred = tuple(res_deferred)
                if (res_deferred[2] or not self._takes_deferred_residual(x) or res_deferred[0].shape != x.shape
                        or res_deferred[0].dtype != x.dtype):
                    residual, res_deferred = _materialized(residual, res_deferred), None
            amax = [] if (ROUTING.x6_pair and x.dtype == torch.float32) else None
            if pool:
                return _tagged(_BN2dReluPool.apply(x, self.weight, self.bias, self, pre, amax), amax[0] if amax else None)
            if self.tail_avgpool and relu and residual is not None and self.num_features % 32 == 0:
                return _BN2dAddReluAvgPool.apply(x, self.weight, self.bias, residual, self, pre)
            link = [] if (ROUTING.bn_bwd_in_gemm and torch.is_grad_enabled() and x.requires_grad) else None
            lazy_res = (ROUTING.lazy_residual_grad and relu and residual is not None and getattr(residual, "_peclr_compact_ok", False)
                        and torch.is_grad_enabled() and residual.requires_grad and self.num_features % 32 == 0)
            defer = None
            if consumer is not None and residual is None:
                if not relu and isinstance(consumer, FusedBatchNormAct2d) and consumer._takes_deferred_residual(x):
                    defer = []
            y = _BN2dAct.apply(x, self.weight, self.bias, residual, self, relu, pre, link, lazy_res, defer, res_deferred, amax)
            _tagged(y, amax[0] if amax else None)   # max |y|, on the device: the "pair" GEMMs that read y derive its power of two from it
            if link:
                y._peclr_bn_link = link
            if defer:
                y._peclr_deferred = defer
            return y
        if self.sync_group is not None and self.training:
            raise _capi.PeclrHipError("synchronised statistics are implemented by the HIP kernels only (hip=True)")
        if self.training and _RECOMPUTING:   # re-run of a checkpointed block: batch statistics, buffers untouched
            y = F.batch_norm(x, None, None, self.weight, self.bias, True, 0.0, self.eps)
        else:
            y = super().forward(x)
        if residual is not None:
            y = y + residual
        y = F.relu(y) if relu else y
        return F.max_pool2d(y, 3, stride=2, padding=1) if pool else y


# ------------------------------------------------------------------ 16-bit prediction: eval-mode BatchNorm in the convolution epilogues
def _fold_pair_ok(conv, bn, kernel, strides) -> bool:
    """May `bn` (eval mode) be folded into `conv`'s 16-bit epilogue?  The layer must have its own scale, shift and running
    statistics, the convolution must be one the pack groups take (`X6PackGroup.member`: channel counts conv_h accepts)."""
    return (isinstance(bn, FusedBatchNormAct2d) and bool(bn.affine) and bool(bn.track_running_stats) and isinstance(conv, Conv2d)
            and conv.kernel_size == kernel and conv.stride in strides and X6PackGroup.member(conv)
            and conv.out_channels == bn.num_features)


def fold_plan(backbone: nn.Module):
    """[(convolution name, BatchNorm name)] under `backbone` whose eval-mode BatchNorm2d the 16-bit prediction path applies in the
    convolution's epilogue (`ROUTING.fold_eval_bn`), in the order the blocks launch them.  Pure host logic.  Bottleneck blocks
    only, and a block only as a whole (one layer that does not qualify keeps the whole block on the unfolded path).  Two layers
    keep their pass because it does more than scale and shift: the stem's bn1 (its pass also max-pools; not in a block anyway)
    and the last block's bn3 when `tail_avgpool` is set (its pass average-pools and never writes the activation)."""
    from .resnet import Bottleneck

    plan = []
    for name, block in backbone.named_modules():
        if not isinstance(block, Bottleneck):
            continue
        one, any_s = ((1, 1),), ((1, 1), (2, 2))
        pairs = [("conv1", "bn1", block.conv1, block.bn1, (1, 1), one), ("conv2", "bn2", block.conv2, block.bn2, (3, 3), any_s)]
        ds = block.downsample
        if ds is not None:
            if not (isinstance(ds, nn.Sequential) and len(ds) == 2):
                continue
            pairs.append(("downsample.0", "downsample.1", ds[0], ds[1], (1, 1), any_s))
        pairs.append(("conv3", "bn3", block.conv3, block.bn3, (1, 1), one))
        if not all(_fold_pair_ok(conv, bn, k, s) for _, _, conv, bn, k, s in pairs):
            continue
        if getattr(block.bn3, "tail_avgpool", False):
            pairs.pop()
        plan += [(f"{name}.{c}", f"{name}.{b}") for c, b, *_ in pairs]
    return plan


class _FoldState:
    """What a backbone keeps between folded forwards: the plan (made once: `enable_hip_batchnorm` drops this object), its
    BatchNorm modules, and the `_capi.BnEvalTables` whose ONE launch per forward writes every layer's table -- inside a
    hipGraph capture too, so a replay sees the running statistics of its own moment.  The descriptor table is re-built only
    when a parameter or buffer has moved (`data_ptr`)."""

    MISSING = ("folded BatchNorm: the descriptor table of the scale / shift launch does not exist yet (or a parameter has moved) and "
               "cannot be uploaded while a hipGraph is being captured -- run one eager forward pass first")

    def __init__(self, backbone):
        mods = dict(backbone.named_modules())
        self.plan = fold_plan(backbone)
        self.bns = [mods[b] for _, b in self.plan]
        self.tables = None

    def begin(self):
        layers = [(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps) for bn in self.bns]
        if self.tables is None or self.tables.stale(layers):
            if _capi.capture_id() != 0:
                raise _capi.PeclrHipError(self.MISSING)
            self.tables = _capi.BnEvalTables(layers)
        self.tables.launch()
        for bn, ss in zip(self.bns, self.tables.views):
            bn.__dict__["_fold_ss"] = ss

    def end(self):
        for bn in self.bns:
            bn.__dict__.pop("_fold_ss", None)


def fold_applies(backbone: nn.Module, x: Tensor) -> bool:
    """Does a forward of `backbone` on `x` take the folded path?  The switch, eval mode, no autograd, HIP kernels on, a HIP input
    under bf16 / fp16 autocast -- and a plan that folds anything."""
    if not (ROUTING.fold_eval_bn and ROUTING.conv16 and not backbone.training and not torch.is_grad_enabled() and x.is_cuda
            and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in _HALF
            and getattr(getattr(backbone, "bn1", None), "hip", False)):
        return False
    st = backbone.__dict__.get("_fold_state")
    if st is None:
        st = backbone.__dict__["_fold_state"] = _FoldState(backbone)
    return bool(st.plan)


@contextlib.contextmanager
def folded_eval_bn(backbone: nn.Module):
    """One forward with the planned BatchNorm layers folded (after `fold_applies`): launches the tables, hands every planned
    layer its slice (`_fold_ss`) for the duration, and takes the slices back."""
    st = backbone.__dict__["_fold_state"]
    st.begin()
    try:
        yield st
    finally:
        st.end()


def fold_table_of(bn):
    """This forward's scale / shift table of `bn`, or None (not planned, or no folded forward is running)."""
    return bn.__dict__.get("_fold_ss")


def enable_hip_batchnorm(module: nn.Module, enabled: bool = True, sync_group=None) -> int:
    """Switch every FusedBatchNormAct2d under `module` to the HIP kernels (or back).  The caller is
    responsible for feeding fp32 channels_last HIP tensors; anything else raises.
    sync_group: process group whose ranks share their batch statistics (None = per-rank)."""
    n = 0
    for m in module.modules():
        m.__dict__.pop("_fold_state", None)             # (the folded-prediction plan and tables: re-made by the next folded forward)
        if isinstance(m, FusedBatchNormAct2d):
            m.hip = enabled
            m.sync_group = sync_group if enabled else None
            n += 1
        elif getattr(m, "fork_entry", False):   # bottleneck conv1 (resnet.Bottleneck marks it)
            m.hip_fork = enabled
        if (isinstance(m, Conv2d) and m.kernel_size == (7, 7) and m.stride == (2, 2) and m.padding == (3, 3) and m.in_channels == 3
                and m.out_channels == 64 and m.groups == 1 and m.bias is None and m.dilation == (1, 1)):
            m.hip_stem = enabled
            m.__dict__.pop("_stem_sets", None)
        if isinstance(m, Conv2d) and m.kernel_size in ((1, 1), (3, 3)) and m.stride in ((1, 1), (2, 2)):
            m.hip_gemm = enabled                # fp32 1x1 (where `_x6_pays`) and 3x3 stride-1 convolutions as in-tree GEMMs
            m.x6_group = None
    if enabled:                                 # their weights are split into bf16 planes once per step, all in one launch
        X6PackGroup([m for m in module.modules() if isinstance(m, Conv2d) and (m.hip_gemm or getattr(m, "hip_fork", False))])
    return n
