"""conv1x1_stats (MFMA 1x1 convolution that emits the following BatchNorm's
statistics) against plain float64 references on the CPU.

Bounds.  y: half an ulp of the output dtype (2^-8 / 2^-11 of |ref|) for the one
rounding, plus the fp32 accumulation bound (Cin + 1) * 2^-24 * (|x| . |w|^T).
Statistics: those of tests/test_gpu_reduction_edges.py, against the float64
statistics of the y the kernel stored.  Layer level: the suite's _tol(dtype);
elements whose ReLU gate the conv output's rounding could flip (|z| < 0.1)
carry no upstream gradient.
"""

import socket

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

import oracle64 as o64
import test_gpu_reduction_edges as edges
from msbn import ops
from msbn.nn import SyncBatchNorm
from msbn.nn.fused import (SyncBatchNormAct2d, bn_add_bn_act, conv1x1_bn_act,
                           conv1x1_with_stats)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
U = 2.0 ** -24
BF16, F16 = torch.bfloat16, torch.float16

# (N, H, W, Cin, Cout, dtypes, plan numbers the shape must reach)
CASES = {
    "below_one_tile": (1, 3, 3, 8, 8, (BF16, F16), dict(
        nchunks=1, k_trips=1, nslabs=1, slab=32, tiles_per_block=1)),
    "one_past_a_tile": (1, 3, 43, 24, 72, (BF16, F16), dict(
        nchunks=2, k_trips=1, nslabs=1, slab=128)),
    "two_tiles_per_block": (1, 1, 2049 * 128 + 1, 8, 8, (BF16, F16), dict(
        tiles_per_block=2, nchunks=1025, finalize_trips=17)),
    "two_slabs_cin_72": (2, 10, 10, 72, 136, (BF16, F16), dict(
        nslabs=2, slab=128, k_trips=1, nchunks=2)),
    "two_k_trips": (3, 10, 10, 256, 72, (BF16, F16), dict(
        k_trips=2, nchunks=3, slab=128)),
    "two_k_trips_two_tiles": (1, 1, 2049 * 128 + 1, 136, 8, (BF16,), dict(
        k_trips=2, tiles_per_block=2)),
}
PARAMS = [pytest.param(name, dt, id=f"{name}-{str(dt)[6:]}")
          for name, c in CASES.items() for dt in c[5]]

_cache = {}


def _case(name, dtype):
    """Inputs, the kernel's outputs and the float64 reference, computed once
    per case and left unchanged."""
    if (name, dtype) not in _cache:
        n, h, w_, cin, cout, _, want = CASES[name]
        g = torch.Generator(device=DEV).manual_seed(len(name) + cin)
        x = (torch.randn((n, cin, h, w_), generator=g, device=DEV) + 0.25) \
            .to(dtype).contiguous(memory_format=torch.channels_last)
        w = (torch.randn((cout, cin, 1, 1), generator=g, device=DEV)
             / cin ** 0.5).to(dtype)
        plan = ops.launch_plan("conv1x1_stats", x, (w,))
        assert plan["path"] == "mfma" and plan["row_tile"] == 128, plan
        for k, v in want.items():
            assert plan[k] == v, (k, plan)
        y, partials, nchunks = ops.conv1x1_stats(x, w)
        assert nchunks == plan["nchunks"]
        assert tuple(partials.shape) == (cout, nchunks, 2)
        x2 = x.permute(0, 2, 3, 1).reshape(-1, cin).cpu().double()
        w2 = w.reshape(cout, cin).cpu().double()
        _cache[name, dtype] = (x, w, y, partials, nchunks, x2 @ w2.T,
                               x2.abs() @ w2.abs().T)
    return _cache[name, dtype]


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_output_against_float64(name, dtype):
    x, w, y, _, _, ref, absref = _case(name, dtype)
    assert y.dtype == dtype and y.shape[:1] + y.shape[2:] == \
        x.shape[:1] + x.shape[2:]
    assert y.is_contiguous(memory_format=torch.channels_last)
    cin, cout = x.shape[1], w.shape[0]
    half_ulp = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
    got = y.permute(0, 2, 3, 1).reshape(-1, cout).cpu()
    edges._within("y", got, ref, half_ulp * ref.abs() + (cin + 1) * U * absref)


def _stat_wants(y, w, b, rm0, rv0, momentum):
    """{name: (float64 want, bound)} of everything the finalize stage emits,
    with the bounds of tests/test_gpu_reduction_edges.py."""
    count = y.numel() // y.shape[1]
    mean, var, invstd = o64.stats(y.cpu(), EPS)
    rtol, matol = edges._stat_bounds(mean, var)
    scale, shift = o64.coefs(mean, invstd, w.cpu(), b.cpu())
    scale_b = (rtol + 2 * U) * scale.abs()
    shift_b = (mean.abs() * scale_b + matol * scale.abs()
               + 2 * U * ((mean * scale).abs() + b.cpu().double().abs()))
    want_m, want_v = o64.running_update(rm0.cpu(), rv0.cpu(), mean, var,
                                        count, momentum)
    unb = var * (count / (count - 1.0))
    blend_m = 4 * U * ((1 - momentum) * rm0.cpu().double().abs()
                       + momentum * mean.abs())
    blend_v = 4 * U * ((1 - momentum) * rv0.cpu().double().abs()
                       + momentum * unb)
    return {
        "mean": (mean, matol), "invstd": (invstd, rtol * invstd),
        "scale": (scale, scale_b), "shift": (shift, shift_b),
        "running_mean": (want_m, momentum * matol + blend_m),
        "running_var": (want_v, momentum * 2 * rtol * (unb + EPS) + blend_v),
    }, mean, var


def _check_stats(y, partials, nchunks):
    C = y.shape[1]
    count = y.numel() // C
    g = torch.Generator(device=DEV).manual_seed(C)
    w = torch.randn(C, generator=g, device=DEV).abs() + 0.1
    b = torch.randn(C, generator=g, device=DEV)
    rm0 = torch.randn(C, generator=g, device=DEV)
    rv0 = torch.rand(C, generator=g, device=DEV) + 0.5
    momentum = 0.1
    wants, mean, var = _stat_wants(y, w, b, rm0, rv0, momentum)

    def unpack(res, rm, rv, packed):
        m, i, cnt, coefs = res
        assert cnt.item() == count and packed[2 * C].item() == count
        return {"mean": m, "invstd": i, "scale": coefs[:C],
                "shift": coefs[C:], "running_mean": rm, "running_var": rv,
                "packed mean": packed[:C], "packed invstd": packed[C:2 * C]}

    rm, rv = rm0.clone(), rv0.clone()
    got = unpack(
        ops.batch_norm_stats_local_from_partials(
            partials, nchunks, count, EPS, rm, rv, momentum, w, b, True),
        rm, rv, ops.batch_norm_stats_packed_from_partials(
            partials, nchunks, count, EPS,
            torch.empty(2 * C + 1, device=DEV)))
    rm, rv = rm0.clone(), rv0.clone()
    sib = unpack(
        ops._require_hip().batch_norm_stats_local(
            y, EPS, rm, rv, momentum, w, b, True),
        rm, rv, ops.batch_norm_stats_packed(
            y, EPS, torch.empty(2 * C + 1, device=DEV)))
    for key, val in got.items():
        want, bound = wants[key.replace("packed ", "")]
        edges._within(key, val.cpu(), want, bound)
        edges._within(key + " vs input-reading op", val.cpu(),
                      sib[key].cpu(), bound)
    return mean, var


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_statistics_of_the_stored_output(name, dtype):
    _, _, y, partials, nchunks, _, _ = _case(name, dtype)
    _check_stats(y, partials, nchunks)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bfloat16", "float16"])
def test_off_centre_output(dtype):
    """A large common offset and all-positive weights: mean^2/var >= 1e4 in
    the stored y, which a plain fp32 sum of squares misses by orders of
    magnitude."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (8 + 0.05 * torch.randn((3, 64, 10, 10), generator=g, device=DEV)) \
        .to(dtype).contiguous(memory_format=torch.channels_last)
    w = (torch.rand((16, 64, 1, 1), generator=g, device=DEV) * 0.1 + 0.05) \
        .to(dtype)
    y, partials, nchunks = ops.conv1x1_stats(x, w)
    mean, var = _check_stats(y, partials, nchunks)
    cond = mean * mean / var
    print("mean^2/var", cond.min().item(), cond.max().item())
    assert (cond >= 1e4).any()


def _declined_inputs(kind):
    g = torch.Generator(device=DEV).manual_seed(9)
    cin = 12 if kind == "cin_12" else 16
    dtype = torch.float32 if kind == "fp32" else BF16
    x = torch.randn((2, cin, 5, 5), generator=g, device=DEV).to(dtype)
    if kind != "nchw":
        x = x.contiguous(memory_format=torch.channels_last)
    if kind == "misaligned":
        buf = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
        v = buf[1:].view(2, 5, 5, cin).permute(0, 3, 1, 2)
        v.copy_(x)
        x = v
        assert x.is_contiguous(memory_format=torch.channels_last)
        assert x.data_ptr() % 16 != 0
    return x


@pytest.mark.parametrize("kind", ["fp32", "nchw", "misaligned", "cin_12"])
def test_declined_inputs_run_the_composition(kind):
    x = _declined_inputs(kind)
    conv = torch.nn.Conv2d(x.shape[1], 16, 1, bias=False).to(DEV, x.dtype)
    bn = SyncBatchNormAct2d(16).to(DEV)
    ref_bn = SyncBatchNormAct2d(16).to(DEV)
    plan = ops.launch_plan("conv1x1_stats", x, (conv.weight,))
    assert plan["path"] == "ineligible", plan
    assert ops.conv1x1_stats(x, conv.weight) == (None, None, 0)
    assert torch.equal(conv1x1_bn_act(conv, bn, x), ref_bn(conv(x)))
    assert torch.equal(bn.running_var, ref_bn.running_var)


class _Stored(torch.autograd.Function):
    """A tensor the layer keeps in ``dt``: the value is rounded on the way
    forward and its gradient on the way back, float64 otherwise."""

    @staticmethod
    def forward(ctx, t, dt):
        ctx.dt = dt
        return t.to(dt).double()

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).double(), None


def _layer_reference(x, w, res, gamma, beta, x_d, w_d, gamma_d, beta_d, g):
    """float64: relu(bn(conv(x)) + (res | bn_d(conv_d(x_d)))), the tensors
    between the operations rounded to the layer's dtype as it stores them.
    Returns the outputs / gradients by name and the gradient mask;
    ``conv_x`` / ``dconv_x`` are the stored conv output and the gradient
    that reaches the convolution (what a rank-local gradient is made of)."""
    dt = x.dtype
    leaves = {k: v.detach().cpu().double().requires_grad_(True)
              for k, v in dict(x=x, w=w, res=res, gamma=gamma, beta=beta,
                               x_d=x_d, w_d=w_d, gamma_d=gamma_d,
                               beta_d=beta_d).items() if v is not None}
    convs = {}

    def bn(t, gm, bt, tag):
        convs[t] = F.conv2d(leaves[t], leaves[tag])
        convs[t].retain_grad()
        y = _Stored.apply(convs[t], dt)
        out[f"conv_{t}"] = y.detach()
        mean, var, _ = o64.stats(y.detach(), EPS)
        out[f"rm_{t}"] = 0.1 * mean
        out[f"rv_{t}"] = 0.9 + 0.1 * var * (y.numel() // y.shape[1]) / (
            y.numel() // y.shape[1] - 1.0)
        return F.batch_norm(y, None, None, leaves[gm], leaves[bt], True,
                            0.0, EPS)

    out = {}
    z = bn("x", "gamma", "beta", "w")
    if res is not None:
        z = z + leaves["res"]
    if x_d is not None:
        z = z + _Stored.apply(bn("x_d", "gamma_d", "beta_d", "w_d"), dt)
    y = torch.relu(z)
    keep = (z.detach().abs() >= 0.1).to(g.dtype).to(g.device)
    y.backward((g * keep).cpu().double())
    out["y"] = y.detach()
    out.update({"d" + k: v.grad for k, v in leaves.items()})
    out.update({"dconv_" + k: v.grad for k, v in convs.items()})
    return out, keep


def _run_layer(mode, dtype, monkeypatch):
    g = torch.Generator(device=DEV).manual_seed(11)
    cin, cout, shape = 24, 40, (3, 24, 7, 9)

    def rn(*s):
        return torch.randn(s, generator=g, device=DEV)

    def cl(t):
        return t.to(dtype).contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)

    x, x_d, res = cl(rn(*shape)), None, None
    conv = torch.nn.Conv2d(cin, cout, 1, bias=False).to(DEV, dtype)
    bn = SyncBatchNormAct2d(cout).to(DEV)
    conv_d = bn_d = None
    with torch.no_grad():
        bn.weight.copy_(rn(cout).abs() + 0.1)
        bn.bias.copy_(rn(cout))
    if mode == "residual":
        res = cl(rn(3, cout, 7, 9))
    if mode == "dual":
        x_d = cl(rn(*shape))
        conv_d = torch.nn.Conv2d(cin, cout, 1, bias=False).to(DEV, dtype)
        bn_d = SyncBatchNorm(cout).to(DEV)
        with torch.no_grad():
            bn_d.weight.copy_(rn(cout).abs() + 0.1)
            bn_d.bias.copy_(rn(cout))
    gout = rn(3, cout, 7, 9).to(dtype)
    want, keep = _layer_reference(
        x, conv.weight, res, bn.weight, bn.bias, x_d,
        None if conv_d is None else conv_d.weight,
        None if bn_d is None else bn_d.weight,
        None if bn_d is None else bn_d.bias, gout)

    launched = []
    real = ops.conv1x1_stats
    monkeypatch.setattr(ops, "conv1x1_stats",
                        lambda *a: launched.append(1) or real(*a))
    if mode == "dual":
        y3, p3 = conv1x1_with_stats(conv, bn, x)
        yd, pd = conv1x1_with_stats(conv_d, bn_d, x_d)
        assert p3 is not None and pd is not None
        y = bn_add_bn_act(bn, bn_d, y3, yd, partials=p3, partials_skip=pd)
    else:
        y = conv1x1_bn_act(conv, bn, x, residual=res)
    assert len(launched) == (2 if mode == "dual" else 1)
    y.backward(gout * keep)
    got = {"y": y, "dx": x.grad, "dw": conv.weight.grad,
           "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "rm_x": bn.running_mean, "rv_x": bn.running_var}
    if res is not None:
        got["dres"] = res.grad
    if mode == "dual":
        got.update({"dx_d": x_d.grad, "dw_d": conv_d.weight.grad,
                    "dgamma_d": bn_d.weight.grad, "dbeta_d": bn_d.bias.grad,
                    "rm_x_d": bn_d.running_mean, "rv_x_d": bn_d.running_var})
    for k, v in got.items():
        torch.testing.assert_close(v.detach().cpu().double(), want[k],
                                   **edges._tol(dtype), msg=lambda m: k + m)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("mode", ["plain", "residual", "dual"])
def test_layer_against_float64(mode, dtype, monkeypatch):
    _run_layer(mode, dtype, monkeypatch)


def test_resnet50_step_runs_the_33_sites(monkeypatch):
    from msbn.models import resnet50

    launched, read = [], []
    real = ops.conv1x1_stats
    monkeypatch.setattr(ops, "conv1x1_stats",
                        lambda *a: launched.append(1) or real(*a))
    hip = ops._require_hip()

    class Spy:  # the extension, counting the input-reading statistics op
        def __getattr__(self, name):
            if name == "batch_norm_stats_local":
                read.append(1)
            return getattr(hip, name)

    monkeypatch.setattr(ops, "_require_hip", lambda: Spy())
    model = resnet50(fused=True, conv_stats=True).to(DEV).to(BF16) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 3, 64, 64, device=DEV, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    loss = model(x).float().square().mean()
    loss.backward()
    assert torch.isfinite(loss).item()
    assert len(launched) == 33
    assert len(read) == 53 - 33  # the other BatchNorms still read their input
    assert all(p.grad is not None for p in model.parameters())


def test_layer_forced_sync_world1(monkeypatch):
    """The packed branch (all_gather of [mean | invstd | count]) on a world-1
    group, as tests/test_gpu_nccl.py runs it."""
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
        _run_layer("residual", BF16, monkeypatch)
        assert packed
    finally:
        dist.destroy_process_group()
