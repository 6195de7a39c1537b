"""The projection-head kernels on the paths the parity suite never reached: every `bn_relu` register variant at and past
its boundary, slab batches past the first eight, eval-mode backward on both routes of `ops.head_align`, the nullable
arguments, the backward's ReLU decision against the forward's, a large column mean, and NT-Xent where exp(s / tau) is large.

All references are float64 on the CPU (oracle/peclr_oracle.py, or a few lines of numpy here where the oracle has no
function: eval-mode BatchNorm1d).  Tolerances are those of tests/test_hip_parity.py::test_bn_relu_fwd_bwd and
::test_ntxent_vs_oracle (fp32 round-off at the same magnitudes) unless an assertion says otherwise.

Coverage of `rows_per_thread(M)` in csrc/bn_relu.hip (RPT rows of each of the 64 row slices held in registers, M <= 64 * RPT;
"strided" = the looping instance).  Each (M, instance) below is launched forward and backward, in training mode, by
test_bn_relu_every_variant_at_and_past_its_boundary:

    M =    1 -> RPT 1          M =  129 -> RPT 4          M =  513 -> RPT 16
    M =    2 -> RPT 1          M =  256 -> RPT 4  (max)   M = 1023 -> RPT 16
    M =   63 -> RPT 1          M =  257 -> RPT 8          M = 1024 -> RPT 16 (max)
    M =   64 -> RPT 1  (max)   M =  512 -> RPT 8  (max)   M = 1025 -> strided (its smallest M)
    M =   65 -> RPT 2                                     M = 1100 -> strided (the largest M used here; eval, ties and
    M =  128 -> RPT 2  (max)                                          large-mean tests)

so every register instance runs at its largest M = 64 * RPT and the next instance at 64 * RPT + 1.  n_slabs = 1 / 9 / 17
(one batch of `slab_sum`, a second batch with a one-slab tail, a third batch) each meet all six instances.
"""
import numpy as np
import pytest
import torch

from oracle import peclr_oracle as O
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def capi():
    from peclr_amd import _capi

    _capi.lib()
    return _capi


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def f64(*arrays):
    return tuple(np.asarray(a, np.float64) for a in arrays)


def head_inputs(m, h, slabs, seed):
    """Split-K slabs whose SUM is N(0, 1) per element (the magnitudes of test_bn_relu_fwd_bwd, whatever n_slabs is), bias,
    gamma in [0.5, ..), beta, running statistics.  Two rows: the variance of two samples is (x1 - x2)^2 / 4, arbitrarily
    close to 0 for random rows, where invstd has condition number |x| / |x1 - x2| with respect to the fp32 rounding of
    a_pre itself; the rows are placed 2 apart so that the bound derived for a well-conditioned column applies."""
    parts = rnd((slabs, m, h), seed, 1.0 / np.sqrt(slabs))
    if m == 2:
        parts *= 0.2
        parts[0, 0] += 1.0
        parts[0, 1] -= 1.0
    bias, gamma, beta = rnd((h,), seed + 1), 0.5 + np.abs(rnd((h,), seed + 2)), rnd((h,), seed + 3, 0.2)
    rm, rv = rnd((h,), seed + 4, 0.1), 1.0 + np.abs(rnd((h,), seed + 5, 0.1))
    return parts, bias, gamma, beta, rm, rv


def relu_decisions(y_ref, a_out):
    """The reference's own y > 0, except within O.RELU_TIE of zero, where fp32 round-off decides and the forward kernel's
    decision is adopted (oracle.projection_head_fwd's `relu_ties`).  That the BACKWARD kernel decides as the forward did
    is held exactly by test_bn_relu_backward_rectifies_exactly_where_the_forward_did."""
    return np.where(np.abs(y_ref) < O.RELU_TIE, host(a_out) > 0, y_ref > 0)


# ------------------------------------------------------------------ 1. every variant, at and past its boundary
_VARIANT_CASES = [
    # every M with H = 36 (three of the last workgroup's four column groups are out of range and still reduce)
    (1, 36, 9), (2, 36, 17), (63, 36, 1), (64, 36, 9), (65, 36, 17), (128, 36, 9), (129, 36, 1), (256, 36, 17),
    (257, 36, 9), (512, 36, 1), (513, 36, 17), (1023, 36, 1), (1024, 36, 9), (1025, 36, 17),
    # the n_slabs values an instance has not met above, at H = 4 (one column group) and H = 16 (a full workgroup)
    (128, 4, 1), (256, 16, 9), (512, 4, 17), (1025, 16, 1), (1025, 4, 9),
    # and the remaining boundaries at the other two H
    (1, 4, 1), (64, 4, 17), (65, 16, 1), (129, 4, 9), (257, 4, 1), (513, 16, 9), (1024, 16, 17),
]


def test_variant_cases_cover_what_the_docstring_says():
    ms = {1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024, 1025}
    assert {m for m, h, _ in _VARIANT_CASES if h == 36} == ms and {h for _, h, _ in _VARIANT_CASES} == {4, 16, 36}

    def rpt(m):
        return next((r for r in (1, 2, 4, 8, 16) if m <= 64 * r), 0)

    assert {(rpt(m), s) for m, _, s in _VARIANT_CASES} == {(r, s) for r in (0, 1, 2, 4, 8, 16) for s in (1, 9, 17)}


@pytest.mark.parametrize("m,h,slabs", _VARIANT_CASES)
def test_bn_relu_every_variant_at_and_past_its_boundary(capi, m, h, slabs):
    parts, bias, gamma, beta, rm, rv = head_inputs(m, h, slabs, 1000 + m)
    p64, b64, g64, be64, rm64, rv64 = f64(parts, bias, gamma, beta, rm, rv)
    a_ref = p64.sum(0) + b64
    y, (mean, var, invstd, xhat) = O.bn1d_train_fwd(a_ref, g64, be64, EPS)
    rm1, rv1 = O.bn1d_running_update(rm64, rv64, mean, var, m, MOM)
    drm, drv, nbt = dev(rm), dev(rv), torch.zeros((), dtype=torch.int64, device=DEV)
    a_pre, a_out, save = capi.bn_relu_fwd(dev(parts), dev(bias), dev(gamma), dev(beta), EPS, MOM, True, drm, drv, nbt)
    da = rnd((m, h), 1900 + m)
    d_a_pre, dg, db, dbias = capi.bn_relu_bwd(dev(da), a_pre, save, dev(gamma), dev(beta))
    got = [host(t) for t in (a_pre, a_out, save[0], save[1], drm, drv, d_a_pre, dg, db, dbias)]
    assert all(np.isfinite(g).all() for g in got) and int(nbt) == 1
    np.testing.assert_allclose(host(a_pre), a_ref, atol=2e-6)
    if m == 1:
        # torch refuses one row; the formulas give: mean = x, var = 0, xhat = 0, y = beta, and no gradient reaches x
        assert np.array_equal(host(a_out), np.maximum(beta, 0)[None])
        assert np.array_equal(host(save[0]), host(a_pre)[0])
        np.testing.assert_allclose(host(save[1]), np.full(h, 1.0 / np.sqrt(np.float64(np.float32(EPS)))), rtol=1e-6)
        np.testing.assert_allclose(host(drm), (1 - MOM) * rm64 + MOM * a_ref[0], atol=1e-6)
        np.testing.assert_allclose(host(drv), (1 - MOM) * rv64, atol=1e-6)      # towards 0: the batch variance is 0
        assert (host(drv) < rv).all()
        assert not host(d_a_pre).any() and not host(dg).any() and not host(dbias).any()
        np.testing.assert_array_equal(host(db), (da * (beta > 0))[0])
        return
    np.testing.assert_allclose(host(a_out), np.maximum(y, 0), atol=1e-5)
    np.testing.assert_allclose(host(save[0]), mean, atol=1e-5)
    np.testing.assert_allclose(host(save[1]), invstd, rtol=1e-5)
    np.testing.assert_allclose(host(drm), rm1, atol=1e-6)
    np.testing.assert_allclose(host(drv), rv1, atol=1e-6)
    dy = da * relu_decisions(y, a_out)
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    dx = (g64 * invstd / m) * (m * dy - dbeta - xhat * dgamma)
    scale = max(1.0, np.abs(dx).max())
    np.testing.assert_allclose(host(d_a_pre), dx, atol=2e-5 * scale)
    np.testing.assert_allclose(host(dg), dgamma, atol=2e-5 * max(1, np.abs(dgamma).max()))
    np.testing.assert_allclose(host(db), dbeta, atol=2e-5 * max(1, np.abs(dbeta).max()))
    assert np.abs(host(dbias)).max() < 1e-3 * scale  # analytically zero


# ------------------------------------------------------------------ 2. eval mode, both directions, both routes
def bn1d_eval_fwd(a, gamma, beta, rm, rv, eps=EPS):
    invstd = 1.0 / np.sqrt(rv + eps)
    xhat = (a - rm) * invstd
    return xhat * gamma + beta, invstd, xhat


@pytest.mark.parametrize("m", [12, 100, 700, 1100])
def test_bn_relu_eval_forward_and_backward(capi, m):
    h, slabs = 36, 2
    parts, bias, gamma, beta, rm, rv = head_inputs(m, h, slabs, 2000 + m)
    p64, b64, g64, be64, rm64, rv64 = f64(parts, bias, gamma, beta, rm, rv)
    a_ref = p64.sum(0) + b64
    y, invstd, xhat = bn1d_eval_fwd(a_ref, g64, be64, rm64, rv64)
    drm, drv, nbt = dev(rm), dev(rv), torch.full((), 5, dtype=torch.int64, device=DEV)
    a_pre, a_out, save = capi.bn_relu_fwd(dev(parts), dev(bias), dev(gamma), dev(beta), EPS, MOM, False, drm, drv, nbt)
    np.testing.assert_allclose(host(a_pre), a_ref, atol=2e-6)
    np.testing.assert_allclose(host(a_out), np.maximum(y, 0), atol=1e-5)
    assert np.array_equal(host(save[0]), rm)
    np.testing.assert_allclose(host(save[1]), invstd, rtol=1e-5)
    da = rnd((m, h), 2900 + m)
    d_a_pre, dg, db, dbias = capi.bn_relu_bwd(dev(da), a_pre, save, dev(gamma), dev(beta), False)
    assert np.array_equal(host(drm), rm) and np.array_equal(host(drv), rv) and int(nbt) == 5     # bit for bit
    dy = da * relu_decisions(y, a_out)
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    dx = g64 * invstd * dy
    dbias_ref = dx.sum(0)
    assert np.median(np.abs(dbias_ref)) > 1e-2 and np.abs(dbias_ref).max() > 1e-2     # not the training mode's zero
    scale = max(1.0, np.abs(dx).max())
    np.testing.assert_allclose(host(d_a_pre), dx, atol=2e-5 * scale)
    np.testing.assert_allclose(host(dg), dgamma, atol=2e-5 * max(1, np.abs(dgamma).max()))
    np.testing.assert_allclose(host(db), dbeta, atol=2e-5 * max(1, np.abs(dbeta).max()))
    np.testing.assert_allclose(host(dbias), dbias_ref, atol=2e-5 * max(1, np.abs(dbias_ref).max()))


def head_align_reference(h, w1, b1, gamma, beta, w2, rm, rv, n, g, training):
    """float64: Linear -> BatchNorm1d (batch or running statistics) -> ReLU -> Linear -> double normalise, loss = sum(z * g)."""
    h, w1, b1, gamma, beta, w2, rm, rv, g = f64(h, w1, b1, gamma, beta, w2, rm, rv, g)
    m = h.shape[0]
    if training:
        p, cache = O.projection_head_fwd(h, w1, b1, gamma, beta, w2, EPS)
        y = cache["y"]
    else:
        a_pre = O.linear_fwd(h, w1, b1)
        y, invstd, xhat = bn1d_eval_fwd(a_pre, gamma, beta, rm, rv)
        p = O.linear_fwd(np.maximum(y, 0), w2)
    z, _, ac = O.align_fwd(p, n, crop=False, rotate=False)
    dp = O.align_bwd(g, ac)
    if training:
        grads = O.projection_head_bwd(dp, cache)
        dy = (dp @ w2) * cache["on"]
        d_a_pre = (gamma * cache["invstd"] / m) * (m * dy - grads["dbeta"] - cache["xhat"] * grads["dgamma"])
    else:
        dy = (dp @ w2) * (y > 0)
        d_a_pre = gamma * invstd * dy
        grads = dict(dh=d_a_pre @ w1, dw1=d_a_pre.T @ h, db1=d_a_pre.sum(0), dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0),
                     dw2=dp.T @ np.maximum(y, 0))
    return z, grads, np.abs(y).min(), np.abs(d_a_pre).max()


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("hid", [48, 64])
@pytest.mark.parametrize("m", [1024, 1026])
def test_head_align_on_both_sides_of_the_route_switch(capi, m, hid, training):
    """M = 1024 is the last batch of the register-resident bn_relu kernels (`ops._REGISTER_BN_MAX_ROWS`); at M = 1026 a
    hidden width the streaming bn2d kernels take (64: H / 4 divides 256) goes to them, and one they do not take (48) to the
    strided bn_relu instance.  The same float64 reference everywhere, in both modes, d(b1) included (non-zero through
    running statistics: the kernel's column sum on the bn_relu kernels, scale * dbeta on the streaming route)."""
    from peclr_amd import ops

    assert ops._REGISTER_BN_MAX_ROWS == 1024
    n, din, seed = m // 2, 32, {48: 3020, 64: 3110}[hid]
    hh, w1, b1 = rnd((m, din), seed), rnd((hid, din), seed + 1, 0.2), rnd((hid,), seed + 2, 0.1)
    gamma, beta, w2 = 0.5 + np.abs(rnd((hid,), seed + 3)), rnd((hid,), seed + 4, 0.2), rnd((128, hid), seed + 5, 0.2)
    rm, rv, g = rnd((hid,), seed + 6, 0.1), 1.0 + np.abs(rnd((hid,), seed + 7, 0.1)), rnd((m, 128), seed + 8)
    z_ref, ref, y_min, d_a_pre_max = head_align_reference(hh, w1, b1, gamma, beta, w2, rm, rv, n, g, training)
    assert y_min > 2e-6, "a pre-activation of this seed is a rounding error away from 0: its ReLU decision is not the reference's to make"
    t = {k: dev(v).requires_grad_() for k, v in dict(h=hh, w1=w1, b1=b1, gamma=gamma, beta=beta, w2=w2).items()}
    drm, drv, nbt = dev(rm), dev(rv), torch.zeros((), dtype=torch.int64, device=DEV)
    capi.EVENT_LOG = {}                                                # the names of the launches: which route ran
    try:
        z, _ = ops.head_align(t["h"], t["w1"], t["b1"], t["gamma"], t["beta"], t["w2"],
                              ops.BNState(training, EPS, MOM, drm, drv, nbt), ops.AlignSpec(n_pairs=n))
        (z * dev(g)).sum().backward()
    finally:
        launched, capi.EVENT_LOG = set(capi.EVENT_LOG), None
    streaming = m > ops._REGISTER_BN_MAX_ROWS and hid == 64
    assert ({"bn2d_apply", "bn2d_bwd_apply"} <= launched) == streaming and ({"bn_relu_fwd", "bn_relu_bwd"} <= launched) != streaming
    np.testing.assert_allclose(host(z), z_ref, atol=2e-6)
    for k, r in (("h", "dh"), ("w1", "dw1"), ("gamma", "dgamma"), ("beta", "dbeta"), ("w2", "dw2")):
        scale = max(1.0, float(np.abs(ref[r]).max()))
        np.testing.assert_allclose(host(t[k].grad), ref[r], atol=5e-5 * scale, err_msg=r)
    db1 = host(t["b1"].grad)
    if training:
        assert np.abs(ref["db1"]).max() < 1e-9 and int(nbt) == 1
        if streaming:
            assert not db1.any()                                       # closed form
        else:
            assert np.abs(db1).max() < 5e-5 * max(1.0, d_a_pre_max)    # the kernel's column sum of d_a_pre
    else:
        assert np.median(np.abs(ref["db1"])) > 1e-3
        np.testing.assert_allclose(db1, ref["db1"], atol=5e-5 * max(1.0, float(np.abs(ref["db1"]).max())), err_msg="db1")
        assert np.array_equal(host(drm), rm) and np.array_equal(host(drv), rv) and int(nbt) == 0


# ------------------------------------------------------------------ 3. nullable arguments
@pytest.mark.parametrize("m,slabs", [(65, 1), (65, 3), (1025, 9)])
def test_bn_relu_forward_without_a_bias(capi, m, slabs):
    parts, _, gamma, beta, rm, rv = head_inputs(m, 36, slabs, 4000 + m)
    a_pre, a_out, save = capi.bn_relu_fwd(dev(parts), None, dev(gamma), dev(beta), EPS, MOM, True, dev(rm), dev(rv), None)
    a_ref = f64(parts)[0].sum(0)
    if slabs == 1:
        assert np.array_equal(host(a_pre), parts[0])
    np.testing.assert_allclose(host(a_pre), a_ref, atol=2e-6)
    y, _ = O.bn1d_train_fwd(a_ref, *f64(gamma, beta), EPS)
    np.testing.assert_allclose(host(a_out), np.maximum(y, 0), atol=1e-5)


@pytest.mark.parametrize("m", [65, 1025])
def test_bn_relu_training_forward_without_tracked_statistics_writes_only_its_outputs(capi, m):
    """running_mean = running_var = num_batches_tracked = NULL through the C entry point itself, with the four outputs placed
    inside one poisoned arena: what lies between and around them must come back untouched."""
    h, slabs, pad, poison = 36, 2, 64, -12345.0
    parts, bias, gamma, beta, _, _ = head_inputs(m, h, slabs, 4100 + m)
    sizes = [m * h, m * h, h, h]                                    # a_pre, a_out, save_mean, save_invstd
    starts = np.cumsum([pad] + [s + pad for s in sizes])[:4]        # multiples of 4 floats: 16-byte aligned
    arena = torch.full((int(starts[3]) + h + pad,), poison, device=DEV)
    views = [arena[int(s):int(s) + n] for s, n in zip(starts, sizes)]
    inputs = [dev(parts), dev(bias), dev(gamma), dev(beta)]
    before = [t.clone() for t in inputs]
    rc = capi.lib().peclr_bn_relu_fwd_f32(inputs[0].data_ptr(), slabs, inputs[1].data_ptr(), m, h, inputs[2].data_ptr(),
                                          inputs[3].data_ptr(), EPS, MOM, 1, None, None, None,
                                          *(v.data_ptr() for v in views), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    a_ref = f64(parts)[0].sum(0) + bias
    y, (mean, var, invstd, _) = O.bn1d_train_fwd(a_ref, *f64(gamma, beta), EPS)
    np.testing.assert_allclose(host(views[0]).reshape(m, h), a_ref, atol=2e-6)
    np.testing.assert_allclose(host(views[1]).reshape(m, h), np.maximum(y, 0), atol=1e-5)
    np.testing.assert_allclose(host(views[2]), mean, atol=1e-5)
    np.testing.assert_allclose(host(views[3]), invstd, rtol=1e-5)
    outside = torch.ones_like(arena, dtype=torch.bool)
    for s, n in zip(starts, sizes):
        outside[int(s):int(s) + n] = False
    assert int(outside.sum()) == 5 * pad and bool((arena[outside] == poison).all())
    assert all(torch.equal(a, b) for a, b in zip(inputs, before))


def test_bn_relu_eval_forward_without_running_statistics_is_an_error(capi):
    parts, bias, gamma, beta, rm, rv = head_inputs(12, 36, 1, 4200)
    for stats in ((None, None), (dev(rm), None), (None, dev(rv))):
        with pytest.raises(capi.PeclrHipError, match="peclr_bn_relu_fwd_f32"):
            capi.bn_relu_fwd(dev(parts), dev(bias), dev(gamma), dev(beta), EPS, MOM, False, *stats, None)


class FixedEncoder(torch.nn.Module):
    """Returns the stored encoder output of the golden run (leaf, so .grad = dL/dh)."""

    def __init__(self, h):
        super().__init__()
        self.h = torch.nn.Parameter(dev(h))

    def forward(self, x):
        return self.h


def test_head_with_an_untracked_batchnorm_trains_one_step():
    """BatchNorm1d(track_running_stats=False): `SimCLR._head_align` hands its three None buffers to the kernel.  Batch
    statistics are all such a layer ever uses, so the golden training step's loss and gradients are reproduced, in train()
    and in eval() alike; then one fused optimiser step moves the head."""
    from peclr_amd import Config, Hybrid2Model
    from peclr_amd.optim import LARSAdam

    g = load_golden("g4_hybrid2_none.npz")
    din, hid = g["in_w1"].shape[1], g["in_w1"].shape[0]
    cfg = Config(projection_head_input_dim=din, projection_head_hidden_dim=hid, output_dim=128, augmentation=[],
                 batch_size=8, num_samples=64, num_of_mini_batch=1, lr=1e-4, opt_weight_decay=1e-6, warmup_epochs=10,
                 optimizer="LARS")
    model = Hybrid2Model(cfg)
    model.encoder = FixedEncoder(g["h"])
    ph = model.projection_head
    ph[1] = torch.nn.BatchNorm1d(hid, track_running_stats=False)
    assert ph[1].running_mean is None and ph[1].running_var is None and ph[1].num_batches_tracked is None
    with torch.no_grad():
        for t, k in ((ph[0].weight, "in_w1"), (ph[0].bias, "in_b1"), (ph[1].weight, "in_gamma"), (ph[1].bias, "in_beta"),
                     (ph[3].weight, "in_w2")):
            t.copy_(torch.from_numpy(g[k]))
    model = model.to(DEV)
    n = int(g["n_pairs"])
    batch = {"transformed_image1": torch.zeros(n, 1, 4, 4, device=DEV), "transformed_image2": torch.zeros(n, 1, 4, 4, device=DEV)}
    for k in g:
        if k.startswith("batch_"):
            batch[k[6:]] = dev(g[k])
    assert abs(float(model.eval().validation_step(batch, 0)["loss"]) - float(g["loss"])) < 1e-5
    out = model.train().training_step(batch, 0)
    assert abs(float(out["loss"]) - float(g["loss"])) < 1e-5
    out["loss"].backward()
    grads = dict(dh=model.encoder.h.grad, dw1=ph[0].weight.grad, dgamma=ph[1].weight.grad, dbeta=ph[1].bias.grad,
                 dw2=ph[3].weight.grad)
    for k, v in grads.items():
        np.testing.assert_allclose(host(v), g[k], rtol=0, atol=3e-5 * max(1.0, float(np.abs(g[k]).max())), err_msg=k)
    assert float(ph[0].bias.grad.abs().max()) < 1e-5
    w_before = ph[0].weight.detach().clone()
    LARSAdam([{"params": list(ph.parameters()), "weight_decay": 1e-6}], lr=1e-3, lars=True).step()
    assert bool(torch.isfinite(ph[0].weight).all()) and not torch.equal(ph[0].weight, w_before)


# ------------------------------------------------------------------ 4. one ReLU decision per element
def tie_problem(m, h, invstd, seed):
    """Per column c: x_c, gamma_c random, xhat = fl32(x_c * invstd_c), beta_c = -fl32(xhat * gamma_c).  With
    running_mean = 0 the kernels' x - mean is exact and their xhat is this xhat, so the pre-activation of a tie element is
    exactly 0 when the multiply and the add round separately, and the rounding residual of the product (either sign) when
    they are fused.  Half of each column's rows are ties, the rest ordinary data."""
    rng = np.random.default_rng(seed)
    xc = rng.standard_normal(h).astype(np.float32)
    xc = np.where(np.abs(xc) < 0.05, np.float32(0.5), xc)
    gamma = (0.5 + rng.random(h)).astype(np.float32)
    xhat = (xc * invstd).astype(np.float32)
    assert np.array_equal(xhat, (xc.astype(np.float64) * invstd.astype(np.float64)).astype(np.float32))
    beta = -(xhat * gamma).astype(np.float32)
    residual = xhat.astype(np.float64) * gamma.astype(np.float64) + beta.astype(np.float64)
    x = rng.standard_normal((m, h)).astype(np.float32)
    tie = rng.permuted(np.arange(m)[:, None].repeat(h, 1) % 2 == 0, axis=0)
    x = np.where(tie, xc[None], x)
    da = ((0.5 + rng.random((m, h))) * rng.choice([-1.0, 1.0], (m, h))).astype(np.float32)
    return x, gamma, beta, da, tie, residual


def test_tie_seed_has_residuals_of_both_signs():
    """The condition of the test below, on the host with invstd = fl32(1 / sqrt(fl32(rv + eps))) (it is checked again there
    on the kernel's own save_invstd before anything is compared)."""
    rv = (0.5 + np.random.default_rng(4999).random(48)).astype(np.float32)
    invstd = (np.float32(1.0) / np.sqrt(rv + np.float32(EPS))).astype(np.float32)
    for m in (64, 512, 1100):
        residual = tie_problem(m, 48, invstd, 5000 + m)[5]
        assert (residual > 0).sum() >= 12 and (residual < 0).sum() >= 12


@pytest.mark.parametrize("m", [64, 512, 1100])
def test_bn_relu_backward_rectifies_exactly_where_the_forward_did(capi, m):
    """The backward does not read a_out: it recomputes the pre-activation's sign from a_pre in another kernel.  Wherever
    the two kernels round that expression differently, an element is rectified in one direction only.  Eval mode,
    running_mean = 0, one slab, no bias, d_a_out and gamma non-zero everywhere: d_a_pre != 0 IS the backward's decision."""
    h = 48
    rv = (0.5 + np.random.default_rng(4999).random(h)).astype(np.float32)
    drm, drv = torch.zeros(h, device=DEV), dev(rv)
    probe = capi.bn_relu_fwd(dev(rnd((1, m, h), 1)), None, dev(np.ones(h, np.float32)), dev(np.zeros(h, np.float32)), EPS, MOM,
                             False, drm, drv, None)[2]
    invstd = host(probe[1])
    np.testing.assert_allclose(invstd, 1.0 / np.sqrt(rv.astype(np.float64) + EPS), rtol=1e-6)
    x, gamma, beta, da, tie, residual = tie_problem(m, h, invstd, 5000 + m)
    assert (residual > 0).sum() >= h // 4 and (residual < 0).sum() >= h // 4, "the tie columns do not split both ways"
    a_pre, a_out, save = capi.bn_relu_fwd(dev(x[None]), None, dev(gamma), dev(beta), EPS, MOM, False, drm, drv, None)
    assert np.array_equal(host(a_pre), x) and np.array_equal(host(save[1]), invstd) and not host(save[0]).any()
    d_a_pre = capi.bn_relu_bwd(dev(da), a_pre, save, dev(gamma), dev(beta), False)[0]
    fwd_on, bwd_on = host(a_out) > 0, host(d_a_pre) != 0
    on_ties = fwd_on[tie].mean()
    print(f"M={m}: {int((fwd_on != bwd_on).sum())} of {fwd_on.size} decisions differ ({int((fwd_on != bwd_on)[tie].sum())} on ties); "
          f"forward rectifies {on_ties:.3f} of the ties on, residual > 0 on {np.mean(residual > 0):.3f} of the columns")
    assert np.array_equal(fwd_on, bwd_on), f"{int((fwd_on != bwd_on).sum())} elements are rectified in one direction only"
    # ordinary elements: the decision is the reference's
    y = bn1d_eval_fwd(*f64(x, gamma, beta, np.zeros(h), rv))[0]
    clear = ~tie & (np.abs(y) > O.RELU_TIE)
    assert np.array_equal(fwd_on[clear], (y > 0)[clear])


# ------------------------------------------------------------------ 5. a large mean does not cost the variance
@pytest.mark.parametrize("m", [256, 1024, 1100])
def test_bn_relu_with_a_large_column_mean(capi, m):
    """Columns 4096 + N(0, 1): a one-pass variance E[x^2] - E[x]^2 would lose all of it (4096^2 * 2^-24 = 1); the two-pass form
    pays the SQUARE of the mean's error.  The reference is float64 on the kernel's own fp32 a_pre (one slab, no bias: the
    input itself).

    Backward bounds: with delta = 8 * 2^-24 * 4096 * invstd the forward's bound on xhat's error (the same for every row of a
    column) and rho = 1e-4 its bound on invstd's relative error, first-order propagation through
    dgamma = sum(dy * xhat) and dx = gamma * invstd / M * (M dy - dbeta - xhat * dgamma) gives
    |d dgamma| <= (delta + rho |xhat|max) * sum|dy| and |d dx| <= gamma * invstd / M * (delta' |dgamma| + |xhat|max * |d dgamma|)
    + rho |dx|max, on top of test_bn_relu_fwd_bwd's round-off terms.  dbeta does not see xhat.  dbias, the column sum of dx,
    is -gamma * invstd / M * dgamma * sum(xhat), and sum(xhat) is no longer 0 but up to M * delta': even the correctly
    rounded fp32 mean of such a column is 2.4e-4 off (half a spacing at 4096), so |dbias| <= gamma * invstd * |dgamma| * delta'.  ReLU decisions within
    gamma * delta of zero are the forward's (relu_decisions' rule at this input's own uncertainty)."""
    h = 48
    x = (4096.0 + rnd((m, h), 6000 + m)).astype(np.float32)
    gamma, beta = 0.5 + np.abs(rnd((h,), 6001)), rnd((h,), 6002, 0.2)
    rm, rv, nbt = torch.zeros(h, device=DEV), torch.ones(h, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    a_pre, a_out, save = capi.bn_relu_fwd(dev(x[None]), None, dev(gamma), dev(beta), EPS, MOM, True, rm, rv, nbt)
    assert np.array_equal(host(a_pre), x)
    x64, g64, b64 = f64(x, gamma, beta)
    y, (mean, var, invstd, xhat) = O.bn1d_train_fwd(x64, g64, b64, EPS)
    xhat_bound = 8 * 2.0 ** -24 * 4096 * invstd
    inv_err = np.abs(host(save[1]) / invstd - 1).max()
    out_err = (np.abs(host(a_out) - np.maximum(y, 0)) - (1e-5 + g64 * xhat_bound)).max()
    print(f"M={m}: invstd rel. error {inv_err:.3e} (bound 1e-4); a_out error minus its bound {out_err:.3e} (<= 0 passes); "
          f"mean error {np.abs(host(save[0]) - mean).max():.3e}")
    np.testing.assert_allclose(host(save[1]), invstd, rtol=1e-4)
    assert (np.abs(host(a_out) - np.maximum(y, 0)) <= 1e-5 + g64 * xhat_bound).all(), f"a_out exceeds its bound by {out_err:.3e}"
    da = rnd((m, h), 6003)
    d_a_pre, dg, db, dbias = capi.bn_relu_bwd(dev(da), a_pre, save, dev(gamma), dev(beta))
    on = np.where(np.abs(y) < O.RELU_TIE + g64 * xhat_bound, host(a_out) > 0, y > 0)
    dy = da * on
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    k = g64 * invstd / m
    dx = k * (m * dy - dbeta - xhat * dgamma)
    xmax = np.abs(xhat).max(0)
    d_xhat = xhat_bound + 1e-4 * xmax
    d_dgamma = d_xhat * np.abs(dy).sum(0)
    d_dx = k * (d_xhat * np.abs(dgamma) + xmax * d_dgamma) + 1e-4 * np.abs(dx).max(0)
    scale = max(1.0, np.abs(dx).max())
    assert (np.abs(host(d_a_pre) - dx) <= 2e-5 * scale + d_dx).all()
    assert (np.abs(host(dg) - dgamma) <= 2e-5 * max(1, np.abs(dgamma).max()) + d_dgamma).all()
    np.testing.assert_allclose(host(db), dbeta, atol=2e-5 * max(1, np.abs(dbeta).max()))
    assert (np.abs(host(dbias)) <= 1e-3 * scale + g64 * invstd * np.abs(dgamma) * d_xhat).all()


# ------------------------------------------------------------------ 6. NT-Xent where the exponential is large
def close_pairs(n, ranks, seed):
    """Unit rows [ranks x (view 1 x n, view 2 x n), 128] (O.pair_index's layout).  Half of the pairs: view 2 = view 1 + 1e-3
    noise, renormalised, so the positive has s ~ 1; the others independent.  One row is copied exactly onto another SAMPLE's
    row: an off-diagonal s = 1 (exp(1 / tau) = 4.9e8 at tau = 0.05, the largest argument the kernel can meet)."""
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    blocks = []
    for _ in range(ranks):
        z1 = unit(rng.standard_normal((n, 128)))
        z2 = unit(rng.standard_normal((n, 128)))
        near = np.arange(n) % 2 == 0
        z2[near] = unit(z1[near] + 1e-3 * rng.standard_normal((int(near.sum()), 128)))
        blocks += [z1, z2]
    z = np.concatenate(blocks).astype(np.float32)
    z[1] = z[0]                      # two view-1 rows of different samples (sample 1's own pair is an independent one)
    return z


@pytest.mark.parametrize("tau", [0.07, 0.05])
@pytest.mark.parametrize("n", [37, 128])
def test_ntxent_at_small_temperature_with_close_positives(capi, n, tau):
    z = close_pairs(n, 1, 7000 + n)
    z64 = z.astype(np.float64)
    loss, s, lse_ref, _ = O.ntxent_fwd(z64, n, tau)
    assert np.sort(s[np.arange(n), np.arange(n) + n])[n // 2] > 0.999 and abs(s[0, 1] - 1) < 1e-6
    zall = dev(z)
    out17, lse, sim = capi.ntxent_fwd(zall, 0, zall, n, 1.0 / tau, 1.0 / (2 * n), want_sim=True)
    tol = 2e-6 * 0.5 / tau           # the error of s / tau grows as 1 / tau; 2e-6 is test_ntxent_vs_oracle's bound at tau = 0.5
    print(f"n={n} tau={tau}: loss error {abs(float(out17[16]) - loss):.3e}, lse error {np.abs(host(lse) - lse_ref).max():.3e} "
          f"(bound {tol:.1e}), sim error {np.abs(host(sim) - s).max():.3e}")
    assert np.isfinite(host(out17)).all()
    assert abs(float(out17[16]) - loss) < tol
    np.testing.assert_allclose(host(sim), s, atol=1e-6)
    np.testing.assert_allclose(host(lse), lse_ref, atol=tol)
    dl = torch.full((1,), 0.37, device=DEV)
    dz = host(capi.ntxent_bwd(zall, 0, zall, n, 1.0 / tau, lse, dl, 1.0 / (2 * n)))
    dz_ref = O.ntxent_bwd(z64, lse_ref, n, tau, dloss=0.37)
    np.testing.assert_allclose(dz, dz_ref, atol=5e-7 + 1e-5 * np.abs(dz_ref).max())


def test_ntxent_row_blocks_equal_full_at_small_temperature(capi):
    """test_ntxent_row_blocks_equal_full's decomposition (world = 4, n_local = 5) at tau = 0.05 on close positives.  Its
    bounds at tau = 0.5 (lse 1e-6, loss 2e-6, dz 1e-7) are fp32 spacings of quantities that grow as 1 / tau -- lse ~ 1 / tau,
    dz ~ 1 / (M tau) -- so they are taken times 0.5 / tau, like the oracle comparison's."""
    world, n_local, tau = 4, 5, 0.05
    mr, k = 2 * n_local, 0.5 / tau
    z = close_pairs(n_local, world, 7100)
    zall, one = dev(z), torch.ones(1, device=DEV)
    out_full, lse_full, _ = capi.ntxent_fwd(zall, 0, zall, n_local, 1.0 / tau, 1.0 / (world * mr))
    dz_full = capi.ntxent_bwd(zall, 0, zall, n_local, 1.0 / tau, lse_full, one, 1.0 / (world * mr))
    loss, lses, dzs = 0.0, [], []
    blocks = [zall[r * mr:(r + 1) * mr].contiguous() for r in range(world)]
    for r in range(world):
        out17, lse, _ = capi.ntxent_fwd(blocks[r], r * mr, zall, n_local, 1.0 / tau, 1.0 / (world * mr))
        loss += float(out17[16])
        lses.append(lse)
    lse_all = torch.cat(lses)
    np.testing.assert_allclose(host(lse_all), host(lse_full), atol=1e-6 * k)
    assert abs(loss - float(out_full[16])) < 2e-6 * k
    for r in range(world):
        dzs.append(capi.ntxent_bwd(blocks[r], r * mr, zall, n_local, 1.0 / tau, lse_all, one, 1.0 / (world * mr)))
    np.testing.assert_allclose(host(torch.cat(dzs)), host(dz_full), atol=1e-7 * k)
    ref_loss, _, lse_ref, _ = O.ntxent_fwd(z.astype(np.float64), n_local, tau)
    assert abs(loss - ref_loss) < 2e-6 * k
    np.testing.assert_allclose(host(lse_all), lse_ref, atol=2e-6 * k)
    dz_ref = O.ntxent_bwd(z.astype(np.float64), lse_ref, n_local, tau)
    np.testing.assert_allclose(host(dz_full), dz_ref, atol=5e-7 + 1e-5 * np.abs(dz_ref).max())
