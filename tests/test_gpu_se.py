"""The squeeze-excite stage ops (ops.se_*), bn_silu_se and the SE MBConv
model on the GPU.  Every stage is checked against float64 evaluated from the
previous stage's STORED output, so every bound is a one-step bound.

Bounds, u = 2^-24, SIG = 3e-8 (fast_sigmoid's absolute error, design doc):
  * a term formed from z = scale*y + shift through silu or silu' (a = silu(z),
    d = silu'(z), |silu'| <= 1.1, |silu''| <= 0.5): at most 8 fp32 roundings of
    values no larger than |t| + |z|, and at most 4 uses of the sigmoid:
        E(t) = 8u(|t| + |z|) + 4 SIG.
    Multiplied on by a factor f (dout, y - mean, g): E(t)|f| + 2u|t f| per
    factor (forming the factor, the product); no factor, no such term.
  * a reduction: the sum of its terms' bounds + RED_K * sum|t| (68u: at most
    64 fp32 additions, then fp64); finalizing fp64 into fp32: u|ref|.
  * a dot product of k terms: (k + 1)u * absref, absref the sum of the
    products' magnitudes and the bias's; errors of a recomputed operand add
    as |w| * E.  dpool's scaling by 1/HW is a term of its own, 2u|ref| (the
    reciprocal rounded to fp32, then the product).
  * a rounded output: half an ulp of its dtype, 2^-8 (bf16) or 2^-11 (half)
    of the value, and no less than 2^-25, half the spacing of half's
    subnormals (below 2^-14 the relative figure does not hold).
Layer and model level: the suite's _tol(dtype).
"""

import pytest
import torch
import torch.nn.functional as F

import test_gpu_reduction_edges as edges
from msbn import ops
from msbn.models import mbconv_net
from msbn.nn import SqueezeExcite
from msbn.nn.fused import SyncBatchNormAct2d, bn_silu_se, bn_silu_se_eligible

pytestmark = pytest.mark.gpu

DEV, U, RED_K, BF16, F16 = edges.DEV, edges.U, edges.RED_K, edges.BF16, edges.F16
SIG, EPS = 3e-8, 1e-5
KINDS = ("se_squeeze", "se_scale", "se_bwd_reduce", "se_bwd_elemt", "se_gate",
         "se_gate_bwd")

# name: (N, C, H, W), Cr, what the plan must show
CASES = {
    "one_pixel": ((2, 8, 1, 1), 2, lambda p: p["trips"] == 1),
    # 35 pixels over 32 thread rows (lpr is never below 8): two chunks, the
    # second of 3 pixels; the odd plane below one chunk is the 5 x 5 one
    "odd_plane": ((3, 8, 5, 7), 2, lambda p: p["chunks_per_image"] == 2),
    "below_one_chunk": ((3, 8, 5, 5), 2, lambda p: p["chunks_per_image"] == 1
                        and p["chunk_rows"] > 25 and p["trips"] == 1),
    "idle_lanes": ((2, 24, 5, 7), 6, lambda p: p["lpr"] == 8
                   and p["ctiles"] == 1),
    "two_channel_tiles": ((1, 72, 4, 5), 4, lambda p: p["ctiles"] == 2),
    "cr_1": ((2, 16, 3, 3), 1, lambda p: p["Cr"] == 1),
    "cr_10_of_40": ((2, 40, 3, 5), 10, lambda p: p["Cr"] == 10),
    "partial_last_chunk": ((1, 8, 9, 11), 2, lambda p:
                           p["chunks_per_image"] >= 2
                           and 99 % p["chunk_rows"] != 0),
    "past_a_flush": ((1, 8, 2048 * 32 * 65, 1), 2,
                     lambda p: p["trips"] > p["flush_every"] == 64),
    "second_finalize_trip": ((65, 8, 2, 3), 2,
                             lambda p: p["finalize_trips"] == 2),
}
PARAMS = [pytest.param(n, dt, id=f"{n}-{str(dt)[6:]}")
          for n in CASES for dt in (BF16, F16)]


def _d(t):
    return t.double()


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _err(t, z):
    return 8 * U * (t.abs() + z.abs()) + 4 * SIG


def _img_sums(t):  # [N, C, H, W] -> [N, C]
    return t.sum((2, 3))


def _check_partials(tag, parts, y, dout, scale, shift, mean):
    """{S, Q1, Q2} ({R, P1, P2} with dout) of the stored partials."""
    v = lambda t: _d(t).view(1, -1, 1, 1)
    z = v(scale) * _d(y) + v(shift)
    f = _d(dout) if dout is not None else torch.ones_like(z)
    xmu = _d(y) - v(mean)
    a, d = F.silu(z), _silu_grad(z)
    got = parts.sum(1)
    nf = 0 if dout is None else 1  # factors multiplied on: dout, y - mean
    for i, (t, e, m, k) in enumerate(((a, _err(a, z), f, nf),
                                      (d, _err(d, z), f, nf),
                                      (d, _err(d, z), f * xmu, nf + 1))):
        term = t * m
        bound = _img_sums(e * m.abs() + 2 * k * U * term.abs()) \
            + RED_K * _img_sums(term.abs())
        edges._within(f"{tag}[{i}]", got[..., i], _img_sums(term), bound)


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_stages_against_float64(name, dtype):
    (N, C, H, W), Cr, reaches = CASES[name]
    HW = H * W
    g = edges._gen(len(name))
    y, dout, _ = edges._ordinary((N, C, H, W), dtype, True, len(name))
    scale = torch.rand(C, generator=g, device=DEV) + 0.5
    shift, mean = edges._randn((2, C), g) * 0.5
    coefs = torch.cat([scale, shift])
    invstd = torch.rand(C, generator=g, device=DEV) + 0.5
    gamma = scale / invstd
    w1 = (edges._randn((Cr, C, 1, 1), g) / C ** 0.5).to(dtype)
    w2 = (edges._randn((C, Cr, 1, 1), g) / Cr ** 0.5).to(dtype)
    b1, b2 = edges._randn((Cr,), g, dtype), edges._randn((C,), g, dtype)
    W1, W2 = _d(w1).view(Cr, C), _d(w2).view(C, Cr)
    rel, floor = (2.0 ** -8, 0.0) if dtype == BF16 else (2.0 ** -11, 2.0 ** -25)

    def half_ulp(ref):
        return (rel * ref.abs()).clamp_min(floor)

    plans = [ops.launch_plan(k, y, (w1, w2) if "gate" in k else (dout,))
             for k in KINDS]
    assert all(p["path"] == ("se_gate" if "Cr" in p else "se") and p["V"] == 8
               for p in plans), plans
    assert reaches(plans[-1]), plans[-1]
    cpi = plans[0]["chunks_per_image"]

    # 1: squeeze
    parts = ops.se_squeeze(y, coefs, mean)
    assert tuple(parts.shape) == (N, cpi, C, 3) and parts.dtype == torch.float64
    _check_partials("SQ", parts, y, None, scale, shift, mean)
    # 2: gate, from the stored partials
    s, hpre, gt, q = ops.se_gate(parts, HW, w1, b1, w2, b2)
    tot = parts.sum(1)
    edges._within("s", s, tot[..., 0] / HW, U * (tot[..., 0] / HW).abs())
    edges._within("Q", q, tot[..., 1:], U * tot[..., 1:].abs())
    edges._within("hpre", hpre, _d(s) @ W1.t() + _d(b1), (C + 1) * U * (
        _d(s).abs() @ W1.abs().t() + _d(b1).abs()))
    h = F.silu(_d(hpre))
    e_h = SIG + 2 * U * h.abs()
    zg = h @ W2.t() + _d(b2)
    e_zg = (Cr + 1) * U * (h.abs() @ W2.abs().t() + _d(b2).abs()) \
        + e_h @ W2.abs().t()
    edges._within("g", gt, torch.sigmoid(zg), 0.25 * e_zg + SIG + U)
    # 3: scale, from the stored g
    out = ops.se_scale(y, coefs, gt)
    assert out.dtype == dtype and out.shape == y.shape
    assert out.is_contiguous(memory_format=torch.channels_last)
    v = lambda t: _d(t).view(1, C, 1, 1)
    z = v(scale) * _d(y) + v(shift)
    a, gk = F.silu(z), _d(gt).view(N, C, 1, 1)
    edges._within("out", out, a * gk, half_ulp(a * gk)
                  + _err(a, z) * gk + 2 * U * (a * gk).abs())
    # 4: backward reduce
    bparts = ops.se_backward_reduce(dout, y, coefs, mean)
    assert tuple(bparts.shape) == (N, cpi, C, 3)
    _check_partials("RP", bparts, y, dout, scale, shift, mean)
    # 5: gate backward, from the stored partials, g and hpre
    dpool, dz2, dz1, pt = ops.se_gate_backward(bparts, HW, gt, hpre, w1, w2)
    btot = bparts.sum(1)
    R, g64 = btot[..., 0], _d(gt)
    edges._within("P", pt, btot[..., 1:], U * btot[..., 1:].abs())
    edges._within("dz2", dz2, R * g64 * (1 - g64),
                  4 * U * (R * g64 * (1 - g64)).abs() + U * (R * g64).abs())
    dh = _d(dz2) @ W2
    e_dh = (C + 1) * U * (_d(dz2).abs() @ W2.abs())
    dsl = _silu_grad(_d(hpre))
    edges._within("dz1", dz1, dh * dsl, e_dh * dsl.abs()
                  + dh.abs() * _err(dsl, _d(hpre)) + 2 * U * (dh * dsl).abs())
    dp_ref = _d(dz1) @ W1 / HW
    e_inv_hw = 2 * U * dp_ref.abs()  # 1/HW rounded to fp32, then the product
    edges._within("dpool", dpool, dp_ref, e_inv_hw
                  + (Cr + 1) * U * (_d(dz1).abs() @ W1.abs()) / HW)
    # 6: the factorised BN sums and the parameter gradients, from the tables
    sum_dy, sum_dy_xmu, gw, gb = ops.se_backward_finalize(
        gt, dpool, pt, q, invstd, True, True)
    assert sum_dy.data_ptr() + 4 * C == sum_dy_xmu.data_ptr()
    for i, (name_, got) in enumerate((("sum_dy", sum_dy),
                                      ("sum_dy_xmu", sum_dy_xmu))):
        terms = torch.stack([g64 * _d(pt[..., i]), _d(dpool) * _d(q[..., i])])
        edges._within(name_, got, terms.sum((0, 1)),
                      2 * U * terms.abs().sum((0, 1)))
    edges._within("grad_bias", gb, _d(sum_dy), U * _d(sum_dy).abs())
    edges._within("grad_weight", gw, _d(sum_dy_xmu) * _d(invstd),
                  3 * U * (_d(sum_dy_xmu) * _d(invstd)).abs())
    dw1, db1, dw2, db2 = ops.se_param_backward(dz2, dz1, hpre, s, w1, w2)
    assert dw1.shape == w1.shape and dw2.shape == w2.shape
    assert {t.dtype for t in (dw1, db1, dw2, db2)} == {dtype}
    for name_, got, ref, absref in (
            ("dw1", dw1.view(Cr, C), _d(dz1).t() @ _d(s),
             _d(dz1).abs().t() @ _d(s).abs()),
            ("db1", db1, _d(dz1).sum(0), _d(dz1).abs().sum(0)),
            ("dw2", dw2.view(C, Cr), _d(dz2).t() @ h,
             _d(dz2).abs().t() @ (h.abs() + e_h / U)),
            ("db2", db2, _d(dz2).sum(0), _d(dz2).abs().sum(0))):
        edges._within(name_, got, ref, half_ulp(ref) + 2 * U * absref)
    # 7: elementwise backward, from the stored tables and sums
    count = torch.full((1,), float(N * HW), device=DEV)
    dy = ops.se_backward_elemt(dout, y, coefs, gt, dpool, mean, invstd, gamma,
                               sum_dy, sum_dy_xmu, count)
    assert dy.dtype == dtype and dy.shape == y.shape
    assert dy.is_contiguous(memory_format=torch.channels_last)
    d = _silu_grad(z)
    gin = _d(dout) * gk + _d(dpool).view(N, C, 1, 1)
    f1 = v(invstd) * v(gamma)
    f2, f3 = v(sum_dy) / (N * HW), v(invstd) ** 2 * v(sum_dy_xmu) / (N * HW)
    ref = f1 * (gin * d - f2 - (_d(y) - v(mean)) * f3)
    mag = f1.abs() * ((gin * d).abs() + f2.abs()
                      + (_d(y).abs() + v(mean).abs()) * f3.abs())
    edges._within("dy", dy, ref, half_ulp(ref) + 16 * U * mag
                  + f1.abs() * _err(d, z) * gin.abs())


def _modules(C, Cr, dtype, g):
    bn = SyncBatchNormAct2d(C, act="silu").to(DEV)
    se = SqueezeExcite(C, Cr).to(DEV, dtype)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g, device=DEV).abs() + 0.1)
        bn.bias.copy_(torch.randn(C, generator=g, device=DEV))
    return bn, se


def _layer_reference(y, gout, bn, se):
    """float64 composition on the CPU from the same rounded inputs:
    (leaves, output, gradients in the leaves' order, batch mean, variance)."""
    lv = [t.detach().cpu().double().requires_grad_(True) for t in (
        y, bn.weight, bn.bias, se.fc1.weight, se.fc1.bias, se.fc2.weight,
        se.fc2.bias)]
    a = F.silu(F.batch_norm(lv[0], None, None, lv[1], lv[2], True, 0.0, EPS))
    s = a.mean((2, 3), keepdim=True)
    out = a * torch.sigmoid(F.conv2d(F.silu(F.conv2d(s, lv[3], lv[4])),
                                     lv[5], lv[6]))
    grads = torch.autograd.grad(out, lv, gout.detach().cpu().double())
    return out.detach(), grads


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_layer_against_float64(dtype):
    g = edges._gen(21)
    C, Cr = 24, 6
    y = edges._ordinary((3, C, 7, 9), dtype, True, 21)[0].requires_grad_(True)
    bn, se = _modules(C, Cr, dtype, g)
    plain = SyncBatchNormAct2d(C, act="silu").to(DEV)
    assert bn_silu_se_eligible(bn, se, y)
    out = bn_silu_se(bn, se, y)
    gout = edges._randn(out.shape, g, dtype)
    out.backward(gout)
    plain(y.detach())
    assert torch.equal(bn.running_mean, plain.running_mean)
    assert torch.equal(bn.running_var, plain.running_var)
    assert torch.equal(bn.num_batches_tracked, plain.num_batches_tracked)
    want_out, want = _layer_reference(y, gout, bn, se)
    got = [y.grad, bn.weight.grad, bn.bias.grad, se.fc1.weight.grad,
           se.fc1.bias.grad, se.fc2.weight.grad, se.fc2.bias.grad]
    torch.testing.assert_close(out.detach().cpu().double(), want_out,
                               **edges._tol(dtype))
    for i, (a, b) in enumerate(zip(got, want)):
        torch.testing.assert_close(a.cpu().double(), b, **edges._tol(dtype),
                                   msg=lambda m, i=i: f"gradient {i}: {m}")


@pytest.mark.parametrize("case", ["fp32", "nchw", "eval", "hooks", "c_12"])
def test_declined_on_the_gpu_is_exactly_the_composition(case, monkeypatch):
    """Each check of bn_silu_se_eligible on CUDA tensors the others pass."""
    monkeypatch.setattr(ops, "se_scale", lambda *a: pytest.fail("se_scale"))
    g = edges._gen(7)
    C = 12 if case == "c_12" else 16
    dtype = torch.float32 if case == "fp32" else BF16
    y = edges._randn((2, C, 5, 6), g, dtype)
    if case != "nchw":
        y = y.contiguous(memory_format=torch.channels_last)
    bn, se = _modules(C, 4, dtype, g)
    ref_bn = SyncBatchNormAct2d(C, act="silu").to(DEV)
    ref_bn.load_state_dict(bn.state_dict())
    if case == "eval":
        bn.eval(), ref_bn.eval()
    if case == "hooks":
        se.register_forward_hook(lambda m, i, o: None)
    assert not bn_silu_se_eligible(bn, se, y)
    assert torch.equal(bn_silu_se(bn, se, y), se(ref_bn(y)))
    assert torch.equal(bn.running_var, ref_bn.running_var)


def test_gate_ops_decline_without_a_launch():
    """fp64 parameters and a bias of the wrong length: four None each."""
    g = edges._gen(8)
    parts = edges._randn((2, 1, 8, 3), g).double()
    w1, w2 = edges._randn((2, 8), g), edges._randn((8, 2), g)
    b1, b2 = edges._randn((2,), g), edges._randn((8,), g)
    none4 = (None,) * 4
    assert ops.se_gate(parts, 4, w1.double(), b1, w2, b2) == none4
    assert ops.se_gate(parts, 4, w1, b2, w2, b2) == none4
    s, hpre, gt, q = ops.se_gate(parts, 4, w1, b1, w2, b2)
    assert ops.se_gate_backward(parts, 4, gt.double(), hpre, w1, w2) == none4
    assert ops.se_backward_finalize(gt, gt, q, q.double(), b2, True,
                                    True) == none4
    assert ops.se_param_backward(gt, hpre, hpre, s, w1.t(), w2) == none4


def test_mbconv_se_model_against_the_composition(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "se_scale", lambda *a, real=ops.se_scale:
                        calls.append("se_scale") or real(*a))

    def build(flag):
        return mbconv_net((8, 16), (1, 2), num_classes=5, kernel_sizes=(3, 5),
                          se_ratio=0.25, conv_stats=flag, dw_grad=flag) \
            .to(DEV).to(BF16).to(memory_format=torch.channels_last).train()

    model, stock = build(True), build(False)
    stock.load_state_dict(model.state_dict())
    x = torch.randn(4, 3, 32, 32, device=DEV, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    losses = []
    for m in (model, stock):
        losses.append(m(x).float().square().mean())
        losses[-1].backward()
    assert calls == ["se_scale"] * 3
    torch.testing.assert_close(losses[0], losses[1], **edges._tol(BF16))
    for a, b in zip(model.blocks, stock.blocks):
        torch.testing.assert_close(a.se.fc2.bias.grad.float(),
                                   b.se.fc2.bias.grad.float(),
                                   **edges._tol(BF16))


def world2_case(rank, world, device, case):
    """bn_silu_se on unequal batch parts against the float64 full-batch
    composition: the factorised sums under the all_reduce."""
    dtype = getattr(torch, case)
    g = torch.Generator(device=device).manual_seed(9)  # the same on all ranks
    C, Cr, cuts = 16, 4, (0, 3, 5)
    full = (torch.randn((5, C, 6, 5), generator=g, device=device) * 2 + 0.5) \
        .to(dtype).contiguous(memory_format=torch.channels_last)
    gout = torch.randn((5, C, 6, 5), generator=g, device=device).to(dtype)
    bn, se = _modules(C, Cr, dtype, g)
    with torch.no_grad():
        for p in se.parameters():
            p.copy_(torch.randn(p.shape, generator=g, device=device) / 2)
    lo, hi = cuts[rank], cuts[rank + 1]
    y = full[lo:hi].contiguous(memory_format=torch.channels_last) \
        .requires_grad_(True)
    failures = []
    if not bn_silu_se_eligible(bn, se, y):
        failures.append("not eligible")
    out = bn_silu_se(bn, se, y)
    out.backward(gout[lo:hi])
    want_out, want = _layer_reference(full, gout, bn, se)
    for name, a, b in (("out", out, want_out[lo:hi]),
                       ("dy", y.grad, want[0][lo:hi])):
        try:
            torch.testing.assert_close(a.detach().cpu().double(), b,
                                       **edges._tol(dtype))
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    return failures


def test_world2_against_the_full_batch(tmp_path):
    import multirank_harness
    multirank_harness.run_cases(tmp_path, 2, DEV, "test_gpu_se:world2_case",
                                ["bfloat16", "float16"])
