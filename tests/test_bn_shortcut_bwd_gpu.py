"""First block of a stage, backward of relu(bn3(x3) + bn_s(x_s)): the shortcut layer's reduction reads (dy, 1-bit mask) instead of
a written masked gradient, and ONE apply pass (peclr_bn2d_bwd_apply_res_bn) writes the input gradients of both BatchNorm layers.
The bar is bit equality with the three-pass form (`ROUTING.bn_shortcut_bwd_fused = False`): the arithmetic per element and the
order of every sum are the same."""
import copy
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (R, C): < 256 column groups with several rows per pass | tail loop only | unrolled loop + tail, odd R | column blocks > 1 | widest
SHAPES = [(98, 64), (1, 256), (1031, 256), (200, 1024), (37, 2048)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _nhwc(rows2d):
    """[R, C] rows as the channels_last [1, C, R, 1] tensor the binding takes."""
    r, c = rows2d.shape
    return rows2d.contiguous().view(1, r, 1, c).permute(0, 3, 1, 2)


def _kernel_inputs(r, c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(r, c, generator=g)
    dy[torch.rand(r, c, generator=g) < 0.1] = 0.0                         # exact zeros in G
    x3, xs = torch.randn(r, c, generator=g) * 1.3 + 0.2, torch.randn(r, c, generator=g) * 0.8 - 0.1
    mask = torch.randint(-2 ** 31, 2 ** 31, (r, c // 32), generator=g, dtype=torch.int64).to(torch.int32)     # about half the bits off
    mask[0, 0] = 0                                                        # ... and one word with none set
    tables = []
    for _ in range(2):
        mean, invstd = torch.randn(c, generator=g) * 0.3, torch.rand(c, generator=g) + 0.5
        scale, shift = torch.randn(c, generator=g) * 0.7 + 0.2, torch.randn(c, generator=g) * 0.5       # both signs
        tables.append((torch.stack([mean, invstd]).contiguous().to(DEV), torch.stack([scale, shift]).contiguous().to(DEV)))
    to = lambda t: _nhwc(t.to(DEV).to(dtype))
    return to(dy), to(x3), to(xs), mask.to(DEV), tables


def _kernel_case(r, c, dtype, training):
    """The dual apply and the MASK 3 reduction against today's launches; raises AssertionError where a bit differs."""
    from peclr_amd import _capi as capi

    dy, x3, xs, mask, ((save, ss), (save_s, ss_s)) = _kernel_inputs(r, c, dtype, 7 * r + c)
    fp32 = dtype == torch.float32
    slots = [capi.absmax_slot(torch.device(DEV)) if fp32 else None for _ in range(4)]
    # today: bn3's pass writes dres = mask . dy (the DRES instance), the shortcut layer reduces and applies it
    dx_w, dg_w, db_w, dres = capi.bn2d_bwd(dy, x3, None, mask, save, ss, training, True, True, absmax=slots[0])
    dxs_w, dgs_w, dbs_w, _ = capi.bn2d_bwd(dres, xs, None, None, save_s, ss_s, training, False, False, absmax=slots[1])
    got = capi.bn2d_bwd_res_bn(dy, x3, mask, save, ss, training, xs, save_s, ss_s, training, absmax=slots[2], absmax_s=slots[3])
    names = ("dx3", "dgamma3", "dbeta3", "dx_s", "dgamma_s", "dbeta_s")
    for name, a, b in zip(names, got, (dx_w, dg_w, db_w, dxs_w, dgs_w, dbs_w)):
        assert torch.equal(a, b), (name, r, c, dtype, training)
    assert not torch.isnan(got[0].float()).any() and not torch.isnan(got[3].float()).any()
    if fp32:
        assert torch.equal(slots[2], slots[0]) and torch.equal(slots[3], slots[1]), (r, c, training)
        assert float(slots[2]) == float(got[0].abs().max()) and float(slots[3]) == float(got[3].abs().max())
    # the reduction: MASK 3 on (G, mask, x_s) against MASK 0 on dres, the whole partial table, same n_split
    io = capi._IO[dtype][0]
    ns = capi.bn2d_n_split(r, c, io)
    tabs = []
    for d, m, relu in ((dres, None, 0), (dy, mask, 1)):
        partial = torch.full((2 * ns, c), float("nan"), device=DEV)
        capi._call("peclr_bn2d_bwd_reduce", d.data_ptr(), xs.data_ptr(), None, m.data_ptr() if m is not None else None, io, r, c, relu,
                   save_s[0].data_ptr(), save_s[1].data_ptr(), ss_s.data_ptr(), partial.data_ptr(), ns, capi._stream())
        tabs.append(partial)
    assert torch.equal(tabs[0], tabs[1]) and not torch.isnan(tabs[1]).any(), (r, c, dtype)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("r,c", SHAPES)
def test_dual_apply_and_mask_reduce_equal_the_two_launches(r, c, dtype, training):
    """dx3, dx_s, both maxima (fp32: 16-bit passes leave none) and the shortcut layer's partial table, bit for bit, in training and
    in eval mode (zero coefficients).  Row slices are walked back to front, the library's default."""
    _kernel_case(r, c, dtype, training)


def test_the_front_to_back_walk_gives_the_same_bits():
    """PECLR_BN_REVERSE=0 (read once per process): the same cases in a child process whose kernels walk the row slices front to
    back."""
    env = dict(os.environ, PECLR_BN_REVERSE="0")
    code = ("import torch, tests.test_bn_shortcut_bwd_gpu as t\n"
            "for r, c in t.SHAPES:\n"
            "    for dtype in t.DTYPES:\n"
            "        t._kernel_case(r, c, dtype, True)\n"
            "torch.cuda.synchronize(); print('forward walk ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "forward walk ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_the_entry_point_refuses_what_the_kernel_cannot_take():
    from peclr_amd import _capi as capi

    dy, x3, xs, mask, ((save, ss), (save_s, ss_s)) = _kernel_inputs(8, 64, torch.float32, 1)
    coef = torch.zeros(2, 64, device=DEV)
    dx, dxs = torch.empty_like(x3), torch.empty_like(x3)
    tabs = (save[0].data_ptr(), save[1].data_ptr(), ss.data_ptr(), coef.data_ptr(), save_s[0].data_ptr(), save_s[1].data_ptr(),
            ss_s.data_ptr(), coef.data_ptr())
    L = capi.lib()

    def rc(dyp=dy.data_ptr(), mp=mask.data_ptr(), c=64, out=dx.data_ptr(), outs=dxs.data_ptr()):
        return L.peclr_bn2d_bwd_apply_res_bn(dyp, mp, x3.data_ptr(), xs.data_ptr(), 0, 8, c, *tabs, out, outs, None, None, capi._stream())

    assert rc(mp=None) == -1 and rc(dyp=None) == -1            # no mask, no gradient
    assert rc(c=48) == -2                                      # no whole mask words
    assert rc(outs=dx.data_ptr()) == -2 and rc(out=x3.data_ptr()) == -2        # one output for both / in place
    assert rc(dyp=dy.data_ptr() + 4) == -3
    with pytest.raises(capi.PeclrHipError):
        capi.bn2d_bwd_res_bn(dy, x3, None, save, ss, True, xs, save_s, ss_s, True)


# ---------------------------------------------------------------- block level

@pytest.fixture(autouse=True)
def _deterministic_vendor_convolutions(request):
    """The small convolutions of the blocks below run in the vendor library; left alone, some of its kernels (forward and gradient)
    accumulate with atomics and two runs of the SAME form differ in their last bits.  As tests/test_stem_gpu.py does: torch's
    deterministic mode, so that a comparison bit for bit is a statement about the passes under test."""
    det = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(), torch.backends.cudnn.deterministic
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic = True
    request.addfinalizer(lambda: (torch.use_deterministic_algorithms(det[0], warn_only=det[1]), setattr(torch.backends.cudnn, "deterministic", det[2])))


def _first_block(planes, stride, seed):
    from peclr_amd import bn2d as B
    from peclr_amd import resnet

    torch.manual_seed(seed)
    out = planes * 4
    ds = torch.nn.Sequential(resnet.conv1x1(64, out, stride), B.FusedBatchNormAct2d(out))
    blk = resnet.Bottleneck(64, planes, stride, ds, norm_layer=B.FusedBatchNormAct2d).to(DEV).to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, B.FusedBatchNormAct2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.1, 0.1)
    B.enable_hip_batchnorm(blk)
    return blk.train()


def _run_block(blk, x0, fused, autocast=None, prepare=None, forward=None):
    """One forward + backward of a copy of `blk`: (output, dx, parameter gradients, buffers, launch log: tag -> [algorithmic bytes])."""
    from peclr_amd import _capi as capi
    from peclr_amd import bn2d as B

    blk = copy.deepcopy(blk)
    B.enable_hip_batchnorm(blk, **(prepare(blk) or {}) if prepare else {})
    x = (x0.clone() if autocast is None else x0.to(autocast)).requires_grad_(True)
    capi.EVENT_LOG = {}
    try:
        with B.routing(force=True, bn_shortcut_bwd_fused=fused), torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            y = (forward or (lambda b, t: b(t)))(blk, x)
            gy = torch.empty_like(y).copy_(torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
            y.backward(gy)
        torch.cuda.synchronize()
        log = {k: [e[2] for e in v] for k, v in capi.EVENT_LOG.items()}
    finally:
        capi.EVENT_LOG = None
    assert B.end_backward() == 0
    return (y.detach(), x.grad.clone(), {k: (p.grad.clone() if p.grad is not None else None) for k, p in blk.named_parameters()},
            {k: v.clone() for k, v in blk.named_buffers()}, log)


def _assert_same_bits(on, off, what):
    """`on` against `off`, bit for bit: the output, dx, every parameter gradient, every buffer (the running statistics).  The small
    convolutions of these blocks run in the vendor library; torch's deterministic mode (the fixture above) is what lets two runs
    of it agree to the bit, so that any difference here is the fused passes'."""
    pairs = [("y", on[0], off[0]), ("dx", on[1], off[1])] + [(k, on[2][k], off[2][k]) for k in on[2]] + [(k, on[3][k], off[3][k]) for k in on[3]]
    assert on[2].keys() == off[2].keys() and on[3].keys() == off[3].keys(), what
    for k, a, b in pairs:
        assert a is not None and b is not None, (what, k)
        assert torch.equal(a, b), (what, k)


@pytest.mark.parametrize("autocast", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", [16, 15])
@pytest.mark.parametrize("planes,stride", [(16, 1), (32, 1), (32, 2)])
def test_first_block_is_bit_identical_and_launches_one_apply_less(planes, stride, hw, autocast):
    blk = _first_block(planes, stride, seed=planes + stride)
    x0 = torch.randn(2, 64, hw, hw, generator=torch.Generator().manual_seed(hw)).to(DEV).contiguous(memory_format=torch.channels_last)
    on, off = (_run_block(blk, x0, f, autocast) for f in (True, False))
    _assert_same_bits(on, off, (planes, stride, hw, autocast))
    assert on[2]["downsample.1.weight"] is not None and on[2]["downsample.1.bias"] is not None
    assert not any(torch.isnan(g.float()).any() for g in on[2].values()) and not torch.isnan(on[1].float()).any()
    # the launch log: the block's output is [r, c] elements of e bytes
    ho = (hw + stride - 1) // stride
    r, c, e = 2 * ho * ho, 4 * planes, 4 if autocast is None else 2
    dres_bytes, dual_bytes = 4 * e * r * c + r * c // 8, 5 * e * r * c + r * c // 8
    assert off[4]["bn2d_bwd_apply"].count(dres_bytes) == 1 and dual_bytes not in off[4]["bn2d_bwd_apply"]
    assert dres_bytes not in on[4]["bn2d_bwd_apply"] and on[4]["bn2d_bwd_apply"].count(dual_bytes) == 1      # no DRES apply
    assert len(off[4]["bn2d_bwd_apply"]) - len(on[4]["bn2d_bwd_apply"]) == 1
    assert len(off[4].get("bn2d_bwd_reduce", [])) == len(on[4].get("bn2d_bwd_reduce", []))
    assert len(off[4]["bn2d_bwd_finalize"]) == len(on[4]["bn2d_bwd_finalize"])


# ---------------------------------------------------------------- fallbacks: the three-pass form, whatever the switch says

@pytest.fixture(scope="module")
def solo_group(tmp_path_factory):
    """A world-size-1 gloo group (as tests/test_hip_parity.py forms it): the synchronised-statistics route in one process."""
    import torch.distributed as td

    created = not td.is_initialized()
    if created:
        store = td.FileStore(str(tmp_path_factory.mktemp("store") / "rdzv"), 1)
        td.init_process_group("gloo", store=store, rank=0, world_size=1)
    yield td.group.WORLD
    if created:
        td.destroy_process_group()


def _assert_old_path(runs, what):
    on, off = runs
    _assert_same_bits(on, off, what)
    assert on[4]["bn2d_bwd_apply"] == off[4]["bn2d_bwd_apply"], what             # the same launches with the same bytes
    assert on[4].get("bn2d_bwd_reduce") == off[4].get("bn2d_bwd_reduce"), what


def _x0():
    return torch.randn(2, 64, 16, 16, generator=torch.Generator().manual_seed(4)).to(DEV).contiguous(memory_format=torch.channels_last)


def test_synchronised_statistics_take_the_three_pass_form(solo_group):
    blk = _first_block(32, 1, seed=5)
    runs = [_run_block(blk, _x0(), f, prepare=lambda b: dict(sync_group=solo_group)) for f in (True, False)]
    _assert_old_path(runs, "sync")
    assert "bn2d_combine" in runs[0][4]


def test_a_checkpointed_block_takes_the_three_pass_form():
    def ckpt(b):
        b.checkpoint = True

    blk = _first_block(32, 2, seed=6)
    _assert_old_path([_run_block(blk, _x0(), f, prepare=ckpt) for f in (True, False)], "checkpoint")


def test_a_second_reader_of_the_placeholder_takes_the_three_pass_form():
    """The shortcut layer's placeholder is read by bn3's pass AND written out for another reader (a convolution): that reader's
    gradient comes back dense and autograd adds the two -- the hand-over view must not be one of them."""
    from peclr_amd import bn2d as B
    from peclr_amd import resnet

    def forward(b, x):
        out, identity = B.fork_conv1x1(b.conv1, x, stats_for=b.bn1)
        ds = b.downsample
        identity = resnet._bn(ds[1], resnet._conv(ds[0], identity, ds[1]), consumer=b.bn3)
        assert getattr(identity, "_peclr_deferred", None) is not None
        out = resnet._bn(b.bn1, out, relu=True)
        out = resnet._bn(b.bn2, resnet._conv(b.conv2, out, b.bn2, sole_consumer=True), relu=True, consumer=b.conv3)
        y = resnet._bn(b.bn3, resnet._conv(b.conv3, out, b.bn3, sole_consumer=True), identity, relu=True)
        return y + b.extra(identity)

    blk = _first_block(32, 1, seed=7)
    torch.manual_seed(8)
    blk.extra = B.Conv2d(128, 128, 1, bias=False).to(DEV).to(memory_format=torch.channels_last)
    runs = [_run_block(blk, _x0(), f, forward=forward) for f in (True, False)]
    _assert_old_path(runs, "second reader")
    assert not torch.isnan(runs[0][1]).any()


# ---------------------------------------------------------------- step level

def test_resnet18_with_one_pixel_feature_maps_hands_the_gradients_over():
    """ResNet-18 on 32 x 32 images: BasicBlock shortcuts, and layer4 works on 1 x 1 feature maps -- the hand-over view of a
    [N, C, 1, 1] gradient keeps non-zero strides along its two dimensions of size 1 and must still be recognised (a view that is not
    arrives at the shortcut layer as NaNs)."""
    from peclr_amd import bn2d as B
    from peclr_amd.resnet import resnet18

    torch.manual_seed(4)
    net = resnet18().to(DEV).to(memory_format=torch.channels_last).train()
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV).contiguous(memory_format=torch.channels_last)

    def step(fused, frozen):
        m = copy.deepcopy(net)
        B.enable_hip_batchnorm(m)
        if frozen:
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.eval()
        with B.routing(force=True, bn_shortcut_bwd_fused=fused):
            y = m(x)
            (y.square().mean() + y.mean()).backward()
        torch.cuda.synchronize()
        assert B.end_backward() == 0
        return {k: p.grad.clone() for k, p in m.named_parameters()}

    for frozen in (False, True):
        on, off = step(True, frozen), step(False, frozen)
        for k in on:
            assert not torch.isnan(on[k]).any(), (frozen, k)
            assert torch.equal(on[k], off[k]), (frozen, k)


def test_resnet50_step_is_bit_identical_with_the_fused_shortcut_backward():
    """The fp32 ResNet-50 encoder at 2 x 4 views @64 with every in-tree kernel routed: loss and all gradients, switch on against
    off; four dual apply launches, four apply launches fewer."""
    from peclr_amd import _capi as capi
    from peclr_amd import bn2d as B
    from peclr_amd.resnet import resnet50

    torch.manual_seed(3)
    net = resnet50().to(DEV).to(memory_format=torch.channels_last).train()
    x = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV).contiguous(memory_format=torch.channels_last)

    def step(fused):
        m = copy.deepcopy(net)
        B.enable_hip_batchnorm(m)
        capi.EVENT_LOG = {}
        try:
            with B.routing(force=True, bn_shortcut_bwd_fused=fused):
                y = m(x)
                loss = y.square().mean() + y.mean()
                loss.backward()
            torch.cuda.synchronize()
            launches = {k: len(v) for k, v in capi.EVENT_LOG.items()}
        finally:
            capi.EVENT_LOG = None
        assert B.end_backward() == 0
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, launches

    on, off = step(True), step(False)
    assert torch.equal(on[0], off[0]) and torch.isfinite(on[0])
    assert on[1].keys() == off[1].keys() and len(on[1]) >= 150          # (53 convolutions, 53 x 2 BatchNorm parameters)
    for k in on[1]:
        assert torch.equal(on[1][k], off[1][k]), k
    assert off[2]["bn2d_bwd_apply"] - on[2]["bn2d_bwd_apply"] == 4, (on[2], off[2])
    assert off[2].get("bn2d_bwd_reduce", 0) == on[2].get("bn2d_bwd_reduce", 0)
