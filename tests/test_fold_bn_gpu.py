"""16-bit prediction with the eval-mode BatchNorm layers folded into the convolution epilogues (`-m gpu`): the table launch
(peclr_bn2d_eval_tables), the folded kernels (peclr_gemm_h_bnact / peclr_conv_h_bnact: EP bit 2 of conv_h_kernel) against
float64 on the same 16-bit operands and fp32 tables, the folded backbone against stock autocast, and the predictor.

The kernels' bar is the project's bar for its 16-bit convolutions (tests/test_conv_h_gpu.py::close, restated here): the stored
value is the exact value rounded ONCE to the 16-bit format plus fp32 accumulation noise relative to the tensor's scale,
    |out - ref| <= 1.01 (ULP[dtype] |ref| + 2e-6 max|ref|),   no element outside.
Weights are drawn x 0.05, scales in +-[0.5, 2] (three columns in ten negative), shifts in [-1, 1]: the terms of
fmaf(acc, scale, shift) + addend are then of the output's own magnitude, so that bar is the right one for the fused value too."""
import copy
import json
import os

import pytest
import torch

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]
RING = 1          # PECLR_CONV_H_RING


@pytest.fixture(scope="module")
def capi():
    from peclr_amd import _capi

    _capi.lib()
    return _capi


def close(out, ref, dtype, what=""):
    """|out - ref| <= one rounding of ref + accumulation noise relative to the tensor's scale (tests/test_conv_h_gpu.py::close)."""
    err = (out.double() - ref).abs()
    bound = ULP[dtype] * ref.abs() + 2e-6 * float(ref.abs().max()) + 1e-30
    bad = int((err > 1.01 * bound).sum())
    print(f"   {what}: worst |out - ref| / bound = {float((err / bound).max()):.3f}")
    assert bad == 0, (what, bad, float((err / bound).max()))


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def table(n, g):
    """fp32 [2, n]: scale in +-[0.5, 2], shift in [-1, 1]."""
    mag = 0.5 + 1.5 * torch.rand(n, device=DEV, generator=g)
    sign = torch.where(torch.rand(n, device=DEV, generator=g) < 0.3, -1.0, 1.0)
    return torch.stack([mag * sign, 2 * torch.rand(n, device=DEV, generator=g) - 1]).contiguous()


def fused_ref(acc, ss, relu, addend=None, channel_dim=1):
    """float64: relu(acc * scale + shift + addend); with ReLU the reference itself must have 20 - 80 % zeros."""
    shape = [1] * acc.dim()
    shape[channel_dim] = -1
    v = acc * ss[0].double().view(shape) + ss[1].double().view(shape)
    if addend is not None:
        v = v + addend.double()
    if relu:
        v = v.clamp_min(0.0)
        zeros = float((v == 0).double().mean())
        assert 0.2 <= zeros <= 0.8, f"the reference has {zeros:.0%} zeros: the ReLU is not exercised"
    return v


# ------------------------------------------------------------------ 1. the tables, all layers in one launch
def test_eval_tables_of_three_layers_in_one_launch_equal_the_per_layer_path_bit_for_bit(capi):
    g = torch.Generator(device=DEV).manual_seed(1)
    layers = []
    for c, eps in ((64, 1e-5), (256, 1e-3), (2048, 3e-2)):
        layers.append((torch.randn(c, device=DEV, generator=g), torch.randn(c, device=DEV, generator=g),
                       torch.randn(c, device=DEV, generator=g) * 0.3, torch.rand(c, device=DEV, generator=g) * 2 + 1e-3, eps))
    capi.EVENT_LOG = {}
    try:
        t = capi.bn2d_eval_tables(layers)
        torch.cuda.synchronize()
        assert [k for k in capi.EVENT_LOG] == ["bn2d_eval_tables"] and len(capi.EVENT_LOG["bn2d_eval_tables"]) == 1
    finally:
        capi.EVENT_LOG = None
    assert t.flat.numel() == 2 * (64 + 256 + 2048)
    for i, (gamma, beta, rm, rv, eps) in enumerate(layers):
        c = gamma.numel()
        x = nhwc(torch.zeros(1, c, 2, 2, device=DEV))
        _, _, ss, _ = capi.bn2d_fwd(x, None, gamma, beta, rm, rv, None, False, eps, 0.1, False)
        assert t.table(i).shape == (2, c) and torch.equal(t.table(i), ss), f"layer {i}"
    # the same object launched again after the statistics moved: the tables follow, nothing is re-uploaded
    assert not t.stale(layers)
    layers[1][3].mul_(1.7)
    t.launch()
    gamma, beta, rm, rv, eps = layers[1]
    _, _, ss, _ = capi.bn2d_fwd(nhwc(torch.zeros(1, 256, 2, 2, device=DEV)), None, gamma, beta, rm, rv, None, False, eps, 0.1, False)
    assert torch.equal(t.table(1), ss)
    assert t.stale([layers[0], layers[1], layers[2][:3] + (layers[2][3].clone(), layers[2][4])])


# ------------------------------------------------------------------ 2. 1x1: peclr_gemm_h_bnact
GEMM_SHAPES = [(256, 128, 64), (300, 64, 32), (1000, 192, 96)]


def gemm_case(capi, dtype, m, n, k):
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    a = torch.randn(m, k, device=DEV, generator=g).to(dtype)
    w = torch.randn(n, k, device=DEV, generator=g) * 0.05
    pk = capi.HPlanes([(w, False)], dtype).pack()
    ss = table(n, g)
    d = torch.randn(m, n, device=DEV, generator=g).to(dtype)
    acc = a.double() @ w.to(dtype).double().t()
    return a, pk, ss, d, acc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_h_bnact_matches_float64(capi, dtype, m, n, k):
    """(256, 128, 64): whole tiles; (300, 64, 32): a ragged last tile, the narrow 64-column kernels, one k-step; (1000, 192, 96):
    128 + 64 columns and three k-steps, which wrap the stages."""
    a, pk, ss, d, acc = gemm_case(capi, dtype, m, n, k)
    for relu in (False, True):
        for addend in (None, d):
            ref = fused_ref(acc, ss, relu, addend)
            for tile_rows in (0, 128, 256):
                out = capi.gemm_h_bnact(a, pk.planes[0], n, ss, relu=relu, addend=addend, tile_rows=tile_rows)
                assert out.dtype == dtype and out.shape == (m, n)
                close(out, ref, dtype, f"relu {relu} addend {addend is not None} tile_rows {tile_rows}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_h_bnact_treats_nan_as_the_unfolded_path_does(capi, dtype):
    m, n, k = 300, 64, 32
    a, pk, ss, d, _ = gemm_case(capi, dtype, m, n, k)
    a[17] = float("nan")
    gamma, beta = ss[0].clone(), ss[1].clone()                         # running mean 0, variance 1 - eps: scale = gamma, shift = beta
    rm, rv = torch.zeros(n, device=DEV), torch.full((n,), 1.0 - 1e-5, device=DEV)
    for relu in (False, True):
        y = capi.gemm_h(a, pk.planes[0], n)
        want, _, ss_u, _ = capi.bn2d_fwd(nhwc(y.view(m, n, 1, 1)), None, gamma, beta, rm, rv, None, False, 1e-5, 0.1, relu)
        got = capi.gemm_h_bnact(a, pk.planes[0], n, ss_u, relu=relu)
        assert torch.equal(got.isnan(), want.view(m, n).isnan())
        assert bool(got.isnan()[17].all()) == (not relu) and not bool(got.isnan()[:17].any()) and not bool(got.isnan()[18:].any())


# ------------------------------------------------------------------ 3. 3x3 and stride 2: peclr_conv_h_bnact
def conv_case(dtype, nb, cin, cout, h, w, taps):
    g = torch.Generator(device=DEV).manual_seed(nb + cin + cout + h + w + taps)
    x = nhwc(torch.randn(nb, cin, h, w, device=DEV, generator=g).to(dtype))
    kk = 3 if taps == 9 else 1
    wt = nhwc(torch.randn(cout, cin, kk, kk, device=DEV, generator=g) * 0.05)
    return x, wt, table(cout, g)


def pack(capi, wt, dtype):
    cout, cin = wt.shape[:2]
    return capi.HPlanes([(wt.permute(0, 2, 3, 1).reshape(cout, -1), False)], dtype).pack()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb,cin,cout,h,w,forms", [
    (2, 64, 64, 9, 7, (0, RING)),                   # ring, 320-row stages (0 picks it)
    (1, 32, 128, 5, 40, (0, RING)),                 # ring, 384-row stages, one 32-channel chunk
    (1, 64, 64, 3, 70, (128, 256, RING)),           # rows of 70 pixels: the per-tap 3x3 on both tiles, and the ring on 128-row tiles
])
def test_conv_h_bnact_3x3(capi, dtype, nb, cin, cout, h, w, forms):
    x, wt, ss = conv_case(dtype, nb, cin, cout, h, w, 9)
    pk = pack(capi, wt, dtype)
    acc = torch.nn.functional.conv2d(x.double(), wt.to(dtype).double(), padding=1)
    for relu in (False, True):
        ref = fused_ref(acc, ss, relu)
        for tile_rows in forms:
            y = capi.conv_h_bnact(x, pk.planes[0], cout, ss, relu=relu, tile_rows=tile_rows)
            assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
            close(y, ref, dtype, f"3x3 relu {relu} tile_rows {tile_rows}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb,cin,cout,h,w", [(2, 64, 64, 8, 8), (1, 192, 64, 2, 6)])
def test_conv_h_bnact_stride_2(capi, dtype, nb, cin, cout, h, w):
    for taps in (9, 1):
        x, wt, ss = conv_case(dtype, nb, cin, cout, h, w, taps)
        pk = pack(capi, wt, dtype)
        acc = torch.nn.functional.conv2d(x.double(), wt.to(dtype).double(), stride=2, padding=1 if taps == 9 else 0)
        for relu in (False, True):
            ref = fused_ref(acc, ss, relu)
            for tile_rows in (0, 128, 256):
                y = capi.conv_h_bnact(x, pk.planes[0], cout, ss, relu=relu, taps=taps, stride=2, tile_rows=tile_rows)
                close(y, ref, dtype, f"taps {taps} / 2 relu {relu} tile_rows {tile_rows}")


def test_the_folded_launches_log_under_their_own_tags(capi):
    x, wt, ss = conv_case(torch.bfloat16, 2, 64, 64, 8, 8, 9)
    pk = pack(capi, wt, torch.bfloat16)
    x1, w1, ss1 = conv_case(torch.bfloat16, 2, 64, 64, 8, 8, 1)
    p1 = pack(capi, w1, torch.bfloat16)
    capi.EVENT_LOG, capi.LAUNCH_ORDER = {}, []
    try:
        capi.conv_h_bnact(x, pk.planes[0], 64, ss)
        capi.conv_h_bnact(x, pk.planes[0], 64, ss, stride=2)
        capi.conv_h_bnact(x1, p1.planes[0], 64, ss1, taps=1, stride=2)
        capi.gemm_h_bnact(x1.permute(0, 2, 3, 1).reshape(-1, 64), p1.planes[0], 64, ss1)
        torch.cuda.synchronize()
        assert capi.LAUNCH_ORDER == ["conv3x3_bnact", "conv_s2_bnact", "conv_s2_bnact", "conv1x1_bnact"]
    finally:
        capi.EVENT_LOG, capi.LAUNCH_ORDER = None, None


# ------------------------------------------------------------------ 4. the same bits from launch to launch
@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_kernels_repeat_themselves_bit_for_bit(capi, dtype):
    a, pk, ss, d, _ = gemm_case(capi, dtype, 1000, 192, 96)
    one = capi.gemm_h_bnact(a, pk.planes[0], 192, ss, relu=True, addend=d)
    assert torch.equal(one, capi.gemm_h_bnact(a, pk.planes[0], 192, ss, relu=True, addend=d))
    x, wt, ss = conv_case(dtype, 2, 64, 64, 9, 7, 9)
    pk = pack(capi, wt, dtype)
    one = capi.conv_h_bnact(x, pk.planes[0], 64, ss, relu=True)
    assert torch.equal(one, capi.conv_h_bnact(x, pk.planes[0], 64, ss, relu=True))


# ------------------------------------------------------------------ 5. the backbone
def _rel(a, d):
    return float((a.double() - d.double()).norm() / (d.double().norm() + 1e-30))


@pytest.fixture(scope="module")
def backbones():
    """A random rn50 eval model with perturbed running statistics (as test_rn50_backbone_eval_on_the_hip_path_matches_stock_fp32
    builds it): the stock module and its copy on the HIP kernels; 2 images at 224 x 224; the stock fp32 features."""
    from peclr_amd import pose

    torch.manual_seed(4)
    ref = pose.RN25DwMLPref("rn50").eval()
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.2, 0.2)
            mod.running_var.uniform_(0.5, 2.0)
    hip = copy.deepcopy(ref).to(DEV).enable_hip()
    ref = ref.to(DEV)
    x = torch.randn(2, 3, 224, 224, device=DEV)
    with torch.no_grad():
        d = ref.features(x).float()
    return ref, hip, x, d


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_backbone_is_as_close_to_fp32_as_stock_autocast(backbones, dtype):
    """Four arms of `features`: (a) folded, (b) the same in-tree path unfolded, (c) the stock torch module under autocast, (d)
    stock fp32.  rel(x) = |x - d| / |d|.  Stock autocast is the yardstick: rel(a) <= 2 rel(c) -- one seed is a noisy sample of
    ~50 layers of rounding (hence the factor), while a lost scale, shift or ReLU moves the result by O(1).
    Measured on the MI355X (profiles/fold_bn_parity.txt): see the README."""
    from peclr_amd import bn2d

    ref, hip, x, d = backbones
    xc = nhwc(x)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        with bn2d.routing(fold_eval_bn=True):
            a = hip.features(xc).float()
        with bn2d.routing(fold_eval_bn=False):
            b = hip.features(xc).float()
        c = ref.features(x).float()
    ra, rb, rc = _rel(a, d), _rel(b, d), _rel(c, d)
    print(f"   {dtype}: rel(folded) = {ra:.3e}  rel(unfolded) = {rb:.3e}  rel(stock autocast) = {rc:.3e}")
    assert a.shape == (2, 2048) and bool(torch.isfinite(a).all())
    assert ra <= 2 * rc, (ra, rb, rc)
    assert not torch.equal(a, b)                    # (the folded arm really ran other arithmetic: one rounding per layer)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_folded_forward_launches_no_batchnorm_pass_but_the_stem_and_the_tail(backbones, capi, dtype):
    from peclr_amd import bn2d

    _, hip, x, _ = backbones
    xc = nhwc(x)

    def forward(fold):
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype), bn2d.routing(fold_eval_bn=fold):
            hip.features(xc)                                        # (weight planes and tables exist after this one)
            capi.EVENT_LOG, capi.LAUNCH_ORDER = {}, []
            try:
                hip.features(xc)
                torch.cuda.synchronize()
                return list(capi.LAUNCH_ORDER)
            finally:
                capi.EVENT_LOG, capi.LAUNCH_ORDER = None, None

    tags = forward(True)
    count = lambda t: sum(1 for k in tags if k == t)
    assert count("bn2d_apply") == 0
    assert count("bn2d_pool_apply") == 1 and count("bn2d_apply_avgpool") == 1 and count("bn2d_eval_tables") == 1
    assert sum(1 for k in tags if k.endswith("_bnact")) == 51
    assert count("conv1x1_bnact") == 16 + 15 + 1 and count("conv3x3_bnact") == 13 and count("conv_s2_bnact") == 3 + 3
    assert tags.index("bn2d_eval_tables") < min(i for i, k in enumerate(tags) if k.endswith("_bnact"))
    plain = forward(False)
    assert not any(k.endswith("_bnact") or k == "bn2d_eval_tables" for k in plain) and plain.count("bn2d_apply") >= 47
    assert hip.backend_model.layer1[0].bn1.__dict__.get("_fold_ss") is None          # the slices are taken back after the forward


# ------------------------------------------------------------------ 6. the predictor
@pytest.fixture(scope="module")
def models():
    from tests.test_pose_gpu import _images, _k_and_scale, _prediction_model

    cpu = _prediction_model()
    stock = copy.deepcopy(cpu).to(DEV)
    hip = copy.deepcopy(cpu).to(DEV).enable_hip()
    b = 8
    imgs = torch.from_numpy(_images(b, seed=1)).to(DEV)
    K, scale = (torch.from_numpy(a).to(DEV) for a in _k_and_scale(b, seed=1))
    return stock, hip, imgs, K, scale


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16_bit_predict_and_its_graph_replay(models, precision):
    from peclr_amd.pose import FreiHANDPredictor

    _, hip, imgs, K, scale = models
    pred = FreiHANDPredictor(hip, precision=precision)
    assert pred.fold_bn is FreiHANDPredictor.FOLD_BN_DEFAULT
    fh = pred.predict(imgs, K, scale)
    assert fh.dtype == torch.float64 and fh.shape == (8, 21, 3) and bool(torch.isfinite(fh).all())
    assert pred.last["pass2"]["kp25d"].dtype == torch.float32
    pred.capture(8)
    replay = pred.replay(imgs, K, scale)
    print(f"   {precision}: graph replay bit-equal to predict: {torch.equal(replay, fh)}, "
          f"max |replay - predict| / max |predict| = {float((replay - fh).abs().max() / fh.abs().max()):.2e}")
    torch.testing.assert_close(replay, fh, rtol=1e-5, atol=1e-5 * float(fh.abs().max()))     # (the fp32 replay test's bound)
    # a replay reads the running statistics of ITS moment: the tables are written by a launch inside the graph
    bn = hip.backend_model.layer3[2].bn2
    keep = bn.running_var.clone()
    try:
        bn.running_var.mul_(4.0)
        moved = pred.replay(imgs, K, scale)
        again = pred.predict(imgs, K, scale)
    finally:
        bn.running_var.copy_(keep)
    assert not torch.equal(moved, replay)
    torch.testing.assert_close(moved, again, rtol=1e-5, atol=1e-5 * float(again.abs().max()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_model_output_is_as_close_to_fp32_as_stock_autocast(models, capi, dtype):
    from peclr_amd import bn2d, pose

    stock, hip, imgs, K, _ = models
    b = imgs.shape[0]
    T1 = torch.from_numpy(pose.initial_transform()).reshape(1, 3, 3).to(DEV).expand(b, 3, 3).contiguous()
    table_ = torch.from_numpy(pose.normalisation_table()).to(DEV)
    x, k1 = capi.pose_crop(imgs, T1, K, table_, 224)                  # fixed crops: the same input for every arm
    with torch.no_grad():
        d = stock(x, k1)["kp25d"].float()
        with torch.autocast("cuda", dtype=dtype):
            c = stock(x, k1)["kp25d"].float()
            with bn2d.routing(fold_eval_bn=True):
                a = hip(x, k1)["kp25d"].float()
            with bn2d.routing(fold_eval_bn=False):
                u = hip(x, k1)["kp25d"].float()
    ra, ru, rc = _rel(a, d), _rel(u, d), _rel(c, d)
    print(f"   kp25d {dtype}: rel(folded) = {ra:.3e}  rel(unfolded) = {ru:.3e}  rel(stock autocast) = {rc:.3e}")
    assert bool(torch.isfinite(a).all()) and ra <= 2 * rc, (ra, ru, rc)


def test_default_predictor_launches_what_it_launched_before(models, capi):
    """`FreiHANDPredictor(hip)` with default arguments: the launch tags of one predict, in order, are the list recorded from the
    commit before the 16-bit path existed (tests/golden/g17_predict_launch_tags.json) -- and hold no folded launch."""
    from peclr_amd.pose import FreiHANDPredictor

    _, hip, imgs, K, scale = models
    pred = FreiHANDPredictor(hip)
    assert pred.autocast_dtype is None and pred.fold_bn is False
    pred.predict(imgs, K, scale)
    capi.EVENT_LOG, capi.LAUNCH_ORDER = {}, []
    try:
        pred.predict(imgs, K, scale)
        torch.cuda.synchronize()
        tags = list(capi.LAUNCH_ORDER)
    finally:
        capi.EVENT_LOG, capi.LAUNCH_ORDER = None, None
    assert not any(k.endswith("_bnact") or k == "bn2d_eval_tables" for k in tags)
    with open(os.path.join(GOLDEN, "g17_predict_launch_tags.json")) as f:
        before = json.load(f)["tags"]
    assert tags == before
