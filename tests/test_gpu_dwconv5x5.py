"""ops.dwconv5x5_stats / ops.dwconv5x5_backward (depthwise 5x5 convolution
that emits the following BatchNorm's statistics, and its gradients) against
float64 ``F.conv2d(..., padding=2, groups=C)`` and its autograd on the CPU.

Bounds, the 3x3 rule of taps + 1.  y and dx: half an ulp of the output dtype
for the one rounding plus 26 * 2^-24 * absref for 25 fp32 products and sums.
dw: half an ulp plus 70 * 2^-24 * absref: at most MSBN_ACC_FLUSH = 64 fp32
additions before fp64, which every case asserts from the wgrad plan.
Statistics: tests/test_gpu_conv_stats.py's, against the stored y.  Layer and
model level: the suite's _tol(dtype).
"""

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_stats as cs
import test_gpu_dwconv_stats as d3
import test_gpu_reduction_edges as edges
from msbn import ops
from msbn.models import mbconv_net
from msbn.nn import SyncBatchNorm
from msbn.nn.fused import (SyncBatchNormAct2d, dwconv3x3_bn_act,
                           dwconv5x5_bn_act, dwconv5x5_stats_eligible)

pytestmark = pytest.mark.gpu

DEV, U, BF16, F16, EPS = d3.DEV, d3.U, d3.BF16, d3.F16, d3.EPS
KINDS = {1: ("dwconv5x5_stats", "dwconv5x5_dgrad", "dwconv5x5_wgrad"),
         2: ("dwconv5x5s2_stats", "dwconv5x5s2_dgrad", "dwconv5x5s2_wgrad")}

# name: shape (N, C, H, W) from (stride, forward tile, wgrad tile), and what
# the (forward, dgrad, wgrad) plans must show.  The flush case runs the forward
# alone: its gradients meet nothing the other cases do not.
CASES = {
    "one_pixel": (lambda s, f, w: (2, 8, 1, 1),
                  lambda f, d, w: f["items"] == d["items"] == w["items"] == 2),
    "plane_below_the_kernel": (lambda s, f, w: (3, 8, 2, 3),
                               lambda f, d, w: f["items"] == 3),
    "odd_sides_below_a_tile": (lambda s, f, w: (3, 8, 5, 7),
                               lambda f, d, w: f["items"] == 3),
    "even_sides": (lambda s, f, w: (2, 8, 6, 8), lambda f, d, w: True),
    "one_past_a_tile": (lambda s, f, w: (1, 8, f[0] * s + 1, f[1] * s + 1),
                        lambda f, d, w: f["items"] == 4 and d["items"] >= 4),
    "idle_lanes": (lambda s, f, w: (2, 24, 5, 7), lambda f, d, w: all(
        p["lpr"] == 8 and p["ctiles"] == 1 for p in (f, d, w))),
    "two_channel_tiles": (lambda s, f, w: (1, 72, 4, 5), lambda f, d, w: all(
        p["ctiles"] == 2 for p in (f, d, w))),
    # the second tile geometry: one row and one column past its tiles
    "lpr16_one_past_a_tile": (lambda s, f, w: (1, 1032, 9, 17),
                              lambda f, d, w: all(
        p["lpr"] == 16 and p["ctiles"] == 9 for p in (f, d, w))
        and f["items"] == d["items"] == 4 and w["items"] >= 4),
    "partial_last_chunk": (lambda s, f, w: (1025, 8, 2, 3), lambda f, d, w: all(
        p["nchunks"] >= 2 and p["items"] % p["chunk_items"] != 0
        for p in (f, d, w))),
    "wgrad_finalize_two_trips": (lambda s, f, w: (1, 8, 64 * w[0] * s + 1, 1),
                                 lambda f, d, w: w["finalize_trips"] == 2),
    "forward_past_a_flush": (lambda s, f, w: (1, 8, 8192 * f[0] * s + 1, 16),
                             lambda f, d, w: f["trips"] * f["strip"] >
                             f["flush_every"]),
}
PARAMS = [pytest.param(name, dt, s, id=f"{name}-{str(dt)[6:]}-s{s}")
          for name in CASES for dt in (BF16, F16) for s in (1, 2)]


def _inputs(shape, dtype, stride, seed):
    n, c, h, w_ = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    oshape = (n, c, (h - 1) // stride + 1, (w_ - 1) // stride + 1)

    def away(s, scale, gap):  # d3._away_from_zero: no subnormal outputs
        return d3._away_from_zero(
            torch.randn(s, generator=g, device=DEV) * scale, gap).to(dtype)

    x = away(shape, 1, 0.5).contiguous(memory_format=torch.channels_last)
    gy = away(oshape, 1, 0.5).contiguous(memory_format=torch.channels_last)
    return x, away((c, 1, 5, 5), 1 / 5, 0.2), gy


def _ref64(x, w, gy, stride):
    """(y, dx, dw) by float64 conv2d and its autograd on the CPU."""
    xd = x.cpu().double().requires_grad_(gy is not None)
    wd = w.cpu().double().requires_grad_(gy is not None)
    y = F.conv2d(xd, wd, stride=stride, padding=2, groups=x.shape[1])
    if gy is None:
        return y, None, None
    y.backward(gy.cpu().double())
    return y.detach(), xd.grad, wd.grad


def _plans(x, w, gy, stride):
    return [ops.launch_plan(k, x, (w,) if k.endswith("stats") else (w, gy))
            for k in KINDS[stride]]


@pytest.mark.parametrize("name,dtype,stride", PARAMS)
def test_forward_and_gradients_against_float64(name, dtype, stride):
    shape_of, reaches = CASES[name]
    probe = _plans(*_inputs((1, 8, 1, 1), dtype, stride, 0), stride)
    shape = shape_of(stride, (probe[0]["tile_h"], probe[0]["tile_w"]),
                     (probe[2]["tile_h"], probe[2]["tile_w"]))
    x, w, gy = _inputs(shape, dtype, stride, len(name) + stride)
    fp, dp, wp = plans = _plans(x, w, gy, stride)
    assert all(p["path"] == "dwconv" and p["V"] == 8 for p in plans), plans
    assert reaches(fp, dp, wp), plans
    # wgrad: one flush period per fp32 accumulator, by construction
    assert wp["trips"] * wp["strip"] <= wp["flush_every"] == 64, wp
    half_ulp = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
    fwd_only = name == "forward_past_a_flush"

    y, partials, nchunks = ops.dwconv5x5_stats(x, w, stride)
    assert nchunks == fp["nchunks"]
    assert tuple(partials.shape) == (shape[1], nchunks, 2)
    assert y.dtype == dtype and y.shape == gy.shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    ref = _ref64(x, w, None if fwd_only else gy, stride)
    absref = _ref64(x.abs(), w.abs(), None if fwd_only else gy.abs(), stride)
    edges._within("y", y.cpu(), ref[0],
                  half_ulp * ref[0].abs() + 26 * U * absref[0])
    cs._check_stats(y, partials, nchunks)
    if fwd_only:
        return
    dx, dw = ops.dwconv5x5_backward(gy, x, w, stride, True, True)
    assert dx.dtype == dw.dtype == dtype
    assert dx.shape == x.shape and dw.shape == w.shape
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert dw.is_contiguous()
    edges._within("dx", dx.cpu(), ref[1],
                  half_ulp * ref[1].abs() + 26 * U * absref[1])
    edges._within("dw", dw.cpu(), ref[2],
                  half_ulp * ref[2].abs() + 70 * U * absref[2])


@pytest.mark.parametrize("dtype", d3.DTYPES)
def test_off_centre_statistics(dtype):
    """Offset 8, spread 0.05, positive weights at H = W = 1: mean^2/var of
    the stored y is far above what raw sums survive."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (8 + 0.05 * torch.randn((512, 16, 1, 1), generator=g, device=DEV)) \
        .to(dtype).contiguous(memory_format=torch.channels_last)
    w = (torch.rand((16, 1, 5, 5), generator=g, device=DEV) * 0.1 + 0.05) \
        .to(dtype)
    y, partials, nchunks = ops.dwconv5x5_stats(x, w, 1)
    cs._check_stats(y, partials, nchunks)
    v = y.cpu().double()
    cond = v.mean((0, 2, 3)) ** 2 / v.var((0, 2, 3), unbiased=False)
    assert (cond >= 1e4).any(), cond


def test_wgrad_skips_columns_past_the_output():
    """x column 8 of a 9-wide plane is infinite.  At stride 1 the taps kw = 0
    and 1 reach it only from output columns 10 and 9, which do not exist:
    their dw is that of the same x with the column zeroed."""
    x, w, gy = _inputs((2, 8, 3, 9), BF16, 1, 7)
    x[:, :, :, 8] = float("inf")
    _, dw = ops.dwconv5x5_backward(gy, x, w, 1, False, True)
    x[:, :, :, 8] = 0
    _, _, ref = _ref64(x, w, gy, 1)
    _, _, absref = _ref64(x.abs(), w.abs(), gy.abs(), 1)
    edges._within("dw", dw.cpu()[..., :2], ref[..., :2],
                  2.0 ** -8 * ref[..., :2].abs() + 70 * U * absref[..., :2])


def test_want_flags_and_declines():
    x, w, gy = _inputs((2, 16, 5, 5), BF16, 1, 3)
    dx, dw = ops.dwconv5x5_backward(gy, x, w, 1, True, True)
    only_dx = ops.dwconv5x5_backward(gy, x, w, 1, True, False)
    only_dw = ops.dwconv5x5_backward(gy, x, w, 1, False, True)
    assert only_dx[1] is None and torch.equal(only_dx[0], dx)
    assert only_dw[0] is None and torch.equal(only_dw[1], dw)

    def cl(t):
        return t.contiguous(memory_format=torch.channels_last)

    nchw = torch.randn(2, 16, 5, 5, device=DEV).to(BF16)
    w3 = w[:, :, :3, :3].contiguous()
    declined = {
        "fp32": (x.float(), w.float(), gy.float(), 1),
        "nchw_x": (nchw, w, gy, 1),
        "nchw_grad_y": (x, w, nchw, 1),
        "misaligned_grad_y": (x, w, cs._declined_inputs("misaligned"), 1),
        "c_12": (cl(x[:, :12]), w[:12].contiguous(), cl(gy[:, :12]), 1),
        "weight_3x3": (x, w3, gy, 1),
        "cpu": (x.cpu(), w.cpu(), gy.cpu(), 1),
        "stride_3": (x, w, cl(gy[:, :, :2, :2]), 3),
    }
    for name, (x_, w_, gy_, s) in declined.items():
        assert ops.dwconv5x5_backward(gy_, x_, w_, s, True, True) == \
            (None, None), name
        fwd_too = not name.endswith("grad_y")
        if fwd_too:
            assert ops.dwconv5x5_stats(x_, w_, s) == (None, None, 0), name
        if name not in ("cpu", "stride_3"):  # what a plan can show
            for k in KINDS[1] + KINDS[2]:
                if k.endswith("stats") and not fwd_too:
                    continue
                others = (w_,) if k.endswith("stats") else (w_, gy_)
                assert ops.launch_plan(k, x_, others)["path"] == \
                    "ineligible", (name, k)
    # a 5x5 weight is not the 3x3 op's either
    assert ops.dwconv3x3_stats(x, w, 1) == (None, None, 0)
    assert ops.dwconv3x3_backward(gy, x, w, 1, True, True) == (None, None)
    conv = torch.nn.Conv2d(16, 16, 5, 1, 2, groups=16, bias=False).to(DEV, BF16)
    bn = SyncBatchNormAct2d(16, act="silu").to(DEV)
    ref_bn = SyncBatchNormAct2d(16, act="silu").to(DEV)
    assert dwconv5x5_stats_eligible(conv, bn, x)
    assert torch.equal(dwconv3x3_bn_act(conv, bn, x), ref_bn(conv(x)))


def _layer_reference(x, w, gamma, beta, stride, act, gout):
    """d3._layer_reference at kernel 5x5, padding 2."""
    return d3._layer_reference(x, w, gamma, beta, stride, act, gout, k=5)


@pytest.mark.parametrize("dtype", d3.DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("act", [True, False], ids=["silu", "plain"])
def test_layer_against_float64(act, stride, dtype, monkeypatch):
    calls = []
    for op in ("dwconv5x5_stats", "dwconv5x5_backward"):
        monkeypatch.setattr(ops, op, lambda *a, op=op, real=getattr(ops, op):
                            calls.append(op) or real(*a))
    g = torch.Generator(device=DEV).manual_seed(11 + stride)
    c = 24
    x = torch.randn((3, c, 7, 9), generator=g, device=DEV).to(dtype) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    conv = torch.nn.Conv2d(c, c, 5, stride, 2, groups=c, bias=False) \
        .to(DEV, dtype)
    bn = (SyncBatchNormAct2d(c, act="silu") if act else SyncBatchNorm(c)) \
        .to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g, device=DEV).abs() + 0.1)
        bn.bias.copy_(torch.randn(c, generator=g, device=DEV))
    y = dwconv5x5_bn_act(conv, bn, x, grad_kernels=True)
    gout = torch.randn(y.shape, generator=g, device=DEV).to(dtype)
    y.backward(gout)
    assert calls == ["dwconv5x5_stats", "dwconv5x5_backward"]
    want = _layer_reference(x, conv.weight, bn.weight, bn.bias, stride, act,
                            gout)
    got = {"y": y, "dx": x.grad, "dw": conv.weight.grad,
           "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    for k, v in got.items():
        torch.testing.assert_close(v.detach().cpu().double(), want[k],
                                   **edges._tol(dtype), msg=lambda m: k + m)


def test_mbconv_step_runs_every_5x5_site(monkeypatch):
    calls = []
    for op in ("dwconv5x5_stats", "dwconv5x5_backward"):
        monkeypatch.setattr(ops, op, lambda *a, op=op, real=getattr(ops, op):
                            calls.append(op) or real(*a))

    def build(flag):
        return mbconv_net((8, 16), (1, 2), num_classes=5, kernel_sizes=(5, 5),
                          conv_stats=flag, dw_grad=flag) \
            .to(DEV).to(BF16).to(memory_format=torch.channels_last).train()

    model, stock = build(True), build(False)
    stock.load_state_dict(model.state_dict())
    x = torch.randn(2, 3, 32, 32, device=DEV, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    for m in (model, stock):
        loss = m(x).float().square().mean()
        loss.backward()
        assert torch.isfinite(loss).item()
    assert calls.count("dwconv5x5_stats") == 3
    assert calls.count("dwconv5x5_backward") == 3
    assert all(p.grad is not None for p in model.parameters())
    for a, b in zip(model.blocks, stock.blocks):
        torch.testing.assert_close(a.conv2.weight.grad.float(),
                                   b.conv2.weight.grad.float(),
                                   **edges._tol(BF16))
