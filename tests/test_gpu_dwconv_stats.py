"""dwconv3x3_stats (depthwise 3x3 convolution that emits the following
BatchNorm's statistics) against plain float64 references on the CPU.

Bounds.  y: half an ulp of the output dtype (2^-8 / 2^-11 of |ref|) for the one
rounding, plus 10 * 2^-24 * (|x| * |w|) for nine fp32 products and sums.
Statistics: those of tests/test_gpu_conv_stats.py, against the float64
statistics of the y the kernel stored.  Layer level: the suite's _tol(dtype).
"""

import socket

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

import oracle64 as o64
import test_gpu_conv_stats as cs
import test_gpu_reduction_edges as edges
from msbn import ops
from msbn.models import mbconv_net
from msbn.nn import SyncBatchNorm
from msbn.nn.fused import (SyncBatchNormAct2d, dwconv3x3_bn_act,
                           dwconv_stats_eligible)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
U = 2.0 ** -24
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF16, id="bfloat16"), pytest.param(F16, id="float16")]
KIND = {1: "dwconv3x3_stats", 2: "dwconv3x3s2_stats"}

# name: (N, C, H, W) per stride, dtypes, what the plan / shape must show.
# The flush case needs 2048 chunks x 32 thread rows x 9 items (stride 1: full
# strips, 34M outputs; stride 2: one-column strips, 65 items per thread).
CASES = {
    "one_pixel": ({1: (2, 8, 1, 1), 2: (2, 8, 1, 1)}, (BF16, F16),
                  lambda p, s: s["OW"] == 1 and p["items"] == 2),
    "three_odd_images": ({1: (3, 8, 5, 7), 2: (3, 8, 5, 7)}, (BF16, F16),
                         lambda p, s: s["OW"] < p["strip"]),
    "even_stride2": ({1: (2, 8, 6, 8), 2: (2, 8, 6, 8)}, (BF16, F16),
                     lambda p, s: True),
    "one_past_a_strip": ({1: (2, 8, 3, 17), 2: (2, 8, 3, 17)}, (BF16, F16),
                         lambda p, s: s["OW"] % p["strip"] == 1
                         and s["OW"] > p["strip"]),
    "c24_idle_lanes": ({1: (2, 24, 5, 7), 2: (2, 24, 5, 7)}, (BF16, F16),
                       lambda p, s: p["lpr"] == 8 and p["ctiles"] == 1),
    "two_channel_tiles": ({1: (1, 72, 4, 5), 2: (1, 72, 4, 5)}, (BF16, F16),
                          lambda p, s: p["ctiles"] == 2),
    "partial_last_chunk": ({1: (3, 8, 13, 40), 2: (3, 8, 13, 40)}, (BF16, F16),
                           lambda p, s: p["nchunks"] >= 2
                           and p["items"] % p["chunk_items"] != 0),
    "past_a_flush": ({1: (1, 8, 2048 * 256 + 1, 8),
                      2: (1, 8, 2 * 2048 * 2048 + 1, 1)}, (BF16, F16),
                     lambda p, s: p["trips"] >= 2
                     and p["trips"] * p["strip"] > p["flush_every"]),
    "finalize_two_trips": ({1: (1, 8, 4160, 16), 2: (1, 8, 4160, 16)},
                           (BF16, F16),
                           lambda p, s: p["finalize_trips"] >= 2),
}
PARAMS = [pytest.param(name, dt, s, id=f"{name}-{str(dt)[6:]}-s{s}")
          for name, c in CASES.items() for dt in c[1] for s in c[0]]


def _away_from_zero(t, gap):
    """|t| >= gap.  The output bound models one rounding in T's normal range;
    a half output below 2^-14 is spaced 2^-24 whatever its size.  With |x| >=
    0.5 and |w| >= 0.2 the centre tap alone makes |x| * |w| >= 0.1, so the
    bound's second term (6e-8) covers half that spacing (3e-8).  With inputs
    that come arbitrarily close to zero, 12 of 33.5M half outputs of the
    stride-2 flush case (all taps' products below 6e-5) missed the bound by
    up to 2.55x while being correctly rounded."""
    return t + gap * torch.sign(t)


def _ref64(x, w, stride):
    """(conv, |conv|) in float64 on the CPU."""
    xd, wd = x.cpu().double(), w.cpu().double()
    kw = dict(stride=stride, padding=1, groups=x.shape[1])
    return F.conv2d(xd, wd, **kw), F.conv2d(xd.abs(), wd.abs(), **kw)


@pytest.mark.parametrize("name,dtype,stride", PARAMS)
def test_output_and_statistics(name, dtype, stride):
    shapes, _, reaches = CASES[name]
    n, c, h, w_ = shapes[stride]
    g = torch.Generator(device=DEV).manual_seed(len(name) + c + stride)
    x = _away_from_zero(torch.randn((n, c, h, w_), generator=g, device=DEV),
                        0.5).to(dtype) \
        .contiguous(memory_format=torch.channels_last)
    w = _away_from_zero(torch.randn((c, 1, 3, 3), generator=g, device=DEV) / 3,
                        0.2).to(dtype)
    oh, ow = (h - 1) // stride + 1, (w_ - 1) // stride + 1
    plan = ops.launch_plan(KIND[stride], x, (w,))
    assert plan["path"] == "dwconv" and plan["V"] == 8, plan
    assert reaches(plan, dict(OH=oh, OW=ow)), plan
    y, partials, nchunks = ops.dwconv3x3_stats(x, w, stride)
    assert nchunks == plan["nchunks"]
    assert tuple(partials.shape) == (c, nchunks, 2)
    assert y.dtype == dtype and tuple(y.shape) == (n, c, oh, ow)
    assert y.is_contiguous(memory_format=torch.channels_last)
    ref, absref = _ref64(x, w, stride)
    half_ulp = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
    edges._within("y", y.cpu(), ref, half_ulp * ref.abs() + 10 * U * absref)
    cs._check_stats(y, partials, nchunks)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(512, 16, 1, 1), (3, 16, 10, 10)],
                         ids=["pixels", "planes"])
def test_off_centre_output(shape, dtype):
    """A large common offset and all-positive weights.  With padding the
    border outputs sum fewer taps, so a plane as a whole is spread out
    (mean^2/var ~ 30) however narrow its interior: mean^2/var >= 1e4 holds for
    the whole stored y at H = W = 1 and for the interior of the 10x10 planes,
    whose three clusters of values (corner, edge, interior) each sit far
    from zero.  The statistics bounds apply to the whole y in both."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (8 + 0.05 * torch.randn(shape, generator=g, device=DEV)) \
        .to(dtype).contiguous(memory_format=torch.channels_last)
    w = (torch.rand((16, 1, 3, 3), generator=g, device=DEV) * 0.1 + 0.05) \
        .to(dtype)
    y, partials, nchunks = ops.dwconv3x3_stats(x, w, 1)
    cs._check_stats(y, partials, nchunks)
    v = (y if shape[2] == 1 else y[:, :, 1:-1, 1:-1]).cpu().double()
    cond = v.mean((0, 2, 3)) ** 2 / v.var((0, 2, 3), unbiased=False)
    print("mean^2/var", cond.min().item(), cond.max().item())
    assert (cond >= 1e4).any()


DECLINED = ["fp32", "nchw", "misaligned", "c_12", "multiplier_2",
            "dilation_2", "padding_0", "stride_3", "bias"]


@pytest.mark.parametrize("kind", DECLINED)
def test_declined_inputs_run_the_composition(kind, monkeypatch):
    c = 12 if kind == "c_12" else 16
    cout = 2 * c if kind == "multiplier_2" else c
    dtype = torch.float32 if kind == "fp32" else BF16
    x = cs._declined_inputs({"c_12": "cin_12"}.get(kind, kind))
    assert x.shape[1] == c and x.dtype == dtype
    conv = torch.nn.Conv2d(
        c, cout, 3, stride=3 if kind == "stride_3" else 1,
        padding=0 if kind == "padding_0" else (2 if kind == "dilation_2"
                                               else 1),
        dilation=2 if kind == "dilation_2" else 1, groups=c,
        bias=kind == "bias").to(DEV, dtype)
    bn = SyncBatchNormAct2d(cout, act="silu").to(DEV)
    ref_bn = SyncBatchNormAct2d(cout, act="silu").to(DEV)
    if kind in ("fp32", "nchw", "misaligned", "c_12", "multiplier_2"):
        # what the tensors themselves show: the plan and the op decline
        for k in KIND.values():
            assert ops.launch_plan(k, x, (conv.weight,))["path"] == \
                "ineligible"
        assert ops.dwconv3x3_stats(x, conv.weight, 1) == (None, None, 0)
    if kind == "stride_3":
        assert ops.dwconv3x3_stats(x, conv.weight, 3) == (None, None, 0)
    assert not dwconv_stats_eligible(conv, bn, x)
    monkeypatch.setattr(ops, "dwconv3x3_stats", None)  # must not be reached
    assert torch.equal(dwconv3x3_bn_act(conv, bn, x), ref_bn(conv(x)))
    assert torch.equal(bn.running_mean, ref_bn.running_mean)
    assert torch.equal(bn.running_var, ref_bn.running_var)


def _layer_reference(x, w, gamma, beta, stride, act, gout, k=3):
    """float64: silu?(bn(dwconv(x))) from fresh running statistics, the conv
    (``k`` x ``k``, padding ``k // 2``) output rounded to x's dtype forward
    and backward.  Outputs / gradients by name; ``conv`` / ``dconv`` / ``dz``
    are the stored conv output, the gradient that reaches the convolution and
    the one that reaches the BatchNorm's output (what a rank-local gradient
    is made of)."""
    c = x.shape[1]
    lv = {k: v.detach().cpu().double().requires_grad_(True) for k, v in
          dict(x=x, w=w, gamma=gamma, beta=beta).items()}
    raw = F.conv2d(lv["x"], lv["w"], stride=stride, padding=k // 2, groups=c)
    raw.retain_grad()
    yc = cs._Stored.apply(raw, x.dtype)
    mean, var, _ = o64.stats(yc.detach(), EPS)
    count = yc.numel() // c
    z = F.batch_norm(yc, None, None, lv["gamma"], lv["beta"], True, 0.0, EPS)
    z.retain_grad()
    want_y = F.silu(z) if act else z
    want_y.backward(gout.cpu().double())
    return {"y": want_y.detach(), "dx": lv["x"].grad, "dw": lv["w"].grad,
            "dgamma": lv["gamma"].grad, "dbeta": lv["beta"].grad,
            "running_mean": 0.1 * mean,
            "running_var": 0.9 + 0.1 * var * count / (count - 1.0),
            "conv": yc.detach(), "dconv": raw.grad, "dz": z.grad}


def _run_layer(act, stride, dtype, monkeypatch):
    g = torch.Generator(device=DEV).manual_seed(11 + stride)
    c, shape = 24, (3, 24, 7, 9)

    def rn(*s):
        return torch.randn(s, generator=g, device=DEV)

    x = rn(*shape).to(dtype).contiguous(memory_format=torch.channels_last) \
        .requires_grad_(True)
    conv = torch.nn.Conv2d(c, c, 3, stride, 1, groups=c, bias=False) \
        .to(DEV, dtype)
    bn = (SyncBatchNormAct2d(c, act="silu") if act else SyncBatchNorm(c)) \
        .to(DEV)
    with torch.no_grad():
        bn.weight.copy_(rn(c).abs() + 0.1)
        bn.bias.copy_(rn(c))

    launched = []
    real = ops.dwconv3x3_stats
    monkeypatch.setattr(ops, "dwconv3x3_stats",
                        lambda *a: launched.append(1) or real(*a))
    y = dwconv3x3_bn_act(conv, bn, x)
    assert len(launched) == 1
    gout = rn(*y.shape).to(dtype)
    y.backward(gout)

    want = _layer_reference(x, conv.weight, bn.weight, bn.bias, stride, act,
                            gout)
    got = {"y": y, "dx": x.grad, "dw": conv.weight.grad,
           "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    for k, v in got.items():
        torch.testing.assert_close(v.detach().cpu().double(), want[k],
                                   **edges._tol(dtype), msg=lambda m: k + m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("act", [True, False], ids=["silu", "plain"])
def test_layer_against_float64(act, stride, dtype, monkeypatch):
    _run_layer(act, stride, dtype, monkeypatch)


def test_layer_forced_sync_world1(monkeypatch):
    """The packed branch on a world-1 group, as
    tests/test_gpu_conv_stats.py runs it."""
    monkeypatch.setenv("MSBN_FORCE_SYNC", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        monkeypatch.setenv("MASTER_PORT", str(s.getsockname()[1]))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        packed = []
        real = ops.batch_norm_stats_packed_from_partials
        monkeypatch.setattr(ops, "batch_norm_stats_packed_from_partials",
                            lambda *a: packed.append(1) or real(*a))
        _run_layer(True, 2, BF16, monkeypatch)
        assert packed
    finally:
        dist.destroy_process_group()


def test_mbconv_step_runs_every_depthwise_site(monkeypatch):
    launched = []
    real = ops.dwconv3x3_stats
    monkeypatch.setattr(ops, "dwconv3x3_stats",
                        lambda *a: launched.append(1) or real(*a))

    def build(flag):
        return mbconv_net((8, 16), (1, 2), num_classes=5, conv_stats=flag) \
            .to(DEV).to(BF16).to(memory_format=torch.channels_last).train()

    model, plain = build(True), build(False)
    x = torch.randn(2, 3, 32, 32, device=DEV, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    loss = model(x).float().square().mean()
    loss.backward()
    assert torch.isfinite(loss).item()
    assert len(launched) == 3
    assert all(p.grad is not None for p in model.parameters())
    plain.load_state_dict(model.state_dict())
    assert torch.isfinite(plain(x)).all() and len(launched) == 3
