"""ops.dwconv3x3_backward (data and weight gradient of the depthwise 3x3
convolution) against plain float64 references on the CPU.

Bounds.  dx: half an ulp of the output dtype for the one rounding plus
10 * 2^-24 * (|dy| conv |w|) for at most nine fp32 products and sums.  dw:
half an ulp plus 70 * 2^-24 * sum |dy| |x|: at most MSBN_ACC_FLUSH = 64 fp32
additions before fp64, plus the product and conversion roundings.  The wgrad
plan bounds a thread to one flush period by construction, which every case
asserts.  Layer and model level: the suite's _tol(dtype).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_dwconv_stats as fwd
import test_gpu_reduction_edges as edges
from msbn import ops
from msbn.models import mbconv_net
from msbn.nn.fused import dwconv3x3_bn_act

pytestmark = pytest.mark.gpu

DEV, U, BF16, F16 = fwd.DEV, fwd.U, fwd.BF16, fwd.F16
KINDS = {1: ("dwconv3x3_dgrad", "dwconv3x3_wgrad"),
         2: ("dwconv3x3s2_dgrad", "dwconv3x3s2_wgrad")}

# name: shape (N, C, H, W) per stride, what the (dgrad, wgrad) plans must show
CASES = {
    "one_pixel": ((2, 8, 1, 1), lambda d, w: d["items"] == w["items"] == 2),
    "odd_narrower_than_a_strip": ((3, 8, 5, 7), lambda d, w: d["items"] == 15),
    "even_sides": ((2, 8, 6, 8), lambda d, w: True),
    "one_past_a_strip": ((2, 8, 3, 17), lambda d, w: d["items"] == 2 * 3 * 3),
    "idle_lanes": ((2, 24, 5, 7), lambda d, w: all(
        p["lpr"] == 8 and p["ctiles"] == 1 for p in (d, w))),
    "two_channel_tiles": ((1, 72, 4, 5), lambda d, w: all(
        p["ctiles"] == 2 for p in (d, w))),
    "partial_last_chunk": ((3, 8, 13, 40), lambda d, w: all(
        p["nchunks"] >= 2 and p["items"] % p["chunk_items"] != 0
        for p in (d, w))),
    # wgrad chunks hold at most 128 output pixels here: 65 of them
    "finalize_two_trips": ({1: (1, 8, 64 * 128 + 1, 1),
                            2: (1, 8, 2 * 64 * 128 + 1, 1)},
                           lambda d, w: w["finalize_trips"] == 2),
}
PARAMS = [pytest.param(name, dt, s, id=f"{name}-{str(dt)[6:]}-s{s}")
          for name in CASES for dt in (BF16, F16) for s in (1, 2)]


def _inputs(shape, dtype, stride, seed):
    n, c, h, w_ = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    oshape = (n, c, (h - 1) // stride + 1, (w_ - 1) // stride + 1)

    def away(s, scale, gap):  # fwd._away_from_zero: no subnormal outputs
        return fwd._away_from_zero(
            torch.randn(s, generator=g, device=DEV) * scale, gap).to(dtype)

    x = away(shape, 1, 0.5).contiguous(memory_format=torch.channels_last)
    gy = away(oshape, 1, 0.5).contiguous(memory_format=torch.channels_last)
    return x, away((c, 1, 3, 3), 1 / 3, 0.2), gy


def _ref64(x, w, gy, stride):
    """(dx, dw) by float64 autograd on the CPU."""
    xd = x.cpu().double().requires_grad_(True)
    wd = w.cpu().double().requires_grad_(True)
    F.conv2d(xd, wd, stride=stride, padding=1, groups=x.shape[1]) \
        .backward(gy.cpu().double())
    return xd.grad, wd.grad


@pytest.mark.parametrize("name,dtype,stride", PARAMS)
def test_gradients_against_float64(name, dtype, stride):
    shapes, reaches = CASES[name]
    shape = shapes[stride] if isinstance(shapes, dict) else shapes
    x, w, gy = _inputs(shape, dtype, stride, len(name) + stride)
    for s, kinds in KINDS.items():  # all four plans take the case
        g = gy if s == stride else _inputs(shape, dtype, s, 0)[2]
        plans = [ops.launch_plan(k, x, (w, g)) for k in kinds]
        assert all(p["path"] == "dwconv" and p["V"] == 8 for p in plans)
        # one flush period per thread, by construction
        assert plans[1]["trips"] * plans[1]["strip"] <= \
            plans[1]["flush_every"] == 64, plans[1]
        if s == stride:
            assert reaches(*plans), plans
    dx, dw = ops.dwconv3x3_backward(gy, x, w, stride, True, True)
    assert dx.dtype == dw.dtype == dtype
    assert dx.shape == x.shape and dw.shape == w.shape
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert dw.is_contiguous()
    ref_dx, ref_dw = _ref64(x, w, gy, stride)
    abs_dx, abs_dw = _ref64(x.abs(), w.abs(), gy.abs(), stride)
    half_ulp = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
    edges._within("dx", dx.cpu(), ref_dx,
                  half_ulp * ref_dx.abs() + 10 * U * abs_dx)
    edges._within("dw", dw.cpu(), ref_dw,
                  half_ulp * ref_dw.abs() + 70 * U * abs_dw)


def test_want_flags_and_declines():
    x, w, gy = _inputs((2, 16, 5, 5), BF16, 1, 3)
    dx, dw = ops.dwconv3x3_backward(gy, x, w, 1, True, True)
    only_dx = ops.dwconv3x3_backward(gy, x, w, 1, True, False)
    only_dw = ops.dwconv3x3_backward(gy, x, w, 1, False, True)
    assert only_dx[1] is None and torch.equal(only_dx[0], dx)
    assert only_dw[0] is None and torch.equal(only_dw[1], dw)

    nchw = torch.randn(2, 16, 5, 5, device=DEV).to(BF16)
    declined = {
        "fp32": (x.float(), w.float(), gy.float(), 1),
        "nchw_x": (nchw, w, gy, 1),
        "nchw_grad_y": (x, w, nchw, 1),
        "misaligned_grad_y": (x, w, fwd.cs._declined_inputs("misaligned"), 1),
        "c_12": (x[:, :12].contiguous(memory_format=torch.channels_last),
                 w[:12].contiguous(),
                 gy[:, :12].contiguous(memory_format=torch.channels_last), 1),
        "cpu": (x.cpu(), w.cpu(), gy.cpu(), 1),
        "stride_3": (x, w, gy[:, :, :2, :2].contiguous(
            memory_format=torch.channels_last), 3),
    }
    for name, (x_, w_, gy_, s) in declined.items():
        assert ops.dwconv3x3_backward(gy_, x_, w_, s, True, True) == \
            (None, None), name
        if name not in ("cpu", "stride_3"):  # what a plan can show
            for k in KINDS[1] + KINDS[2]:
                assert ops.launch_plan(k, x_, (w_, gy_))["path"] == \
                    "ineligible", (name, k)


@pytest.mark.parametrize("dtype", fwd.DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("act", [True, False], ids=["silu", "plain"])
def test_layer_against_float64(act, stride, dtype, monkeypatch):
    """The forward test's layer and float64 reference, with the layer's
    backward through the gradient kernels; then the flag off."""
    calls = []
    real = ops.dwconv3x3_backward
    monkeypatch.setattr(ops, "dwconv3x3_backward",
                        lambda *a: calls.append(1) or real(*a))
    monkeypatch.setattr(fwd, "dwconv3x3_bn_act", functools.partial(
        dwconv3x3_bn_act, grad_kernels=True))
    fwd._run_layer(act, stride, dtype, monkeypatch)
    assert len(calls) == 1
    monkeypatch.setattr(ops, "dwconv3x3_backward", None)  # not to be reached
    monkeypatch.setattr(fwd, "dwconv3x3_bn_act", dwconv3x3_bn_act)
    fwd._run_layer(act, stride, dtype, monkeypatch)


def test_mbconv_step_uses_the_gradient_kernels(monkeypatch):
    calls = []
    real = ops.dwconv3x3_backward
    monkeypatch.setattr(ops, "dwconv3x3_backward",
                        lambda *a: calls.append(1) or real(*a))

    def build(flag):
        return mbconv_net((8, 16), (1, 2), num_classes=5, conv_stats=True,
                          dw_grad=flag) \
            .to(DEV).to(BF16).to(memory_format=torch.channels_last).train()

    model, stock = build(True), build(False)
    stock.load_state_dict(model.state_dict())
    x = torch.randn(2, 3, 32, 32, device=DEV, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    for m in (model, stock):
        loss = m(x).float().square().mean()
        loss.backward()
        assert torch.isfinite(loss).item()
    assert len(calls) == 3
    assert all(p.grad is not None for p in model.parameters())
    for a, b in zip(model.blocks, stock.blocks):
        torch.testing.assert_close(a.conv2.weight.grad.float(),
                                   b.conv2.weight.grad.float(),
                                   **edges._tol(BF16))
