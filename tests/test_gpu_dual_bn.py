"""Dual BN on the GPU: ``relu(bn(x) + bn_d(x_d))``, the closing layer of a
residual block whose skip path has a BatchNorm of its own, as three kernels
instead of five (docs/KERNEL_DESIGN.md "Dual BN").

The oracle throughout is the composition on the same inputs, and every
comparison is bytewise: the dual kernels use the single kernels' expressions
in their order and the reduce runs on the single reduce's launch plan, so the
change claims to move no bit.  The two layers get different, off-centre
statistics and affine parameters, so a swapped pointer cannot pass.

Shapes are the smallest that reach each path; each case first asserts through
``ops.launch_plan`` that the path is the one it is there for."""

import os
import socket
import subprocess
import sys

import pytest
import torch

import msbn.nn.fused as fused_mod
from msbn import ops
from msbn.models import resnet18, resnet50
from msbn.models.resnet import Bottleneck, conv1x1
from msbn.nn import SyncBatchNorm
from msbn.nn.batchnorm import _momentum_factor
from msbn.nn.fused import (SyncBatchNormAct2d, SyncBatchNormDualActFunction,
                           bn_add_bn_act)

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = 1e-5
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _cl(t, channels_last=True):
    return t.contiguous(memory_format=torch.channels_last) \
        if channels_last else t.contiguous()


def _storage_order(t, channels_last=True):
    """The elements of a dense tensor in the order of their storage."""
    return (t.permute(0, 2, 3, 1) if channels_last else t).reshape(-1)


def _same(a, b):
    """torch.equal that also holds for NaNs in the same places."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(
        a.contiguous().reshape(-1).view(torch.uint8),
        b.contiguous().reshape(-1).view(torch.uint8))


def _offset_view(t, k):
    """A channels-last copy of t living k ELEMENTS past an aligned
    allocation."""
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=t.device)
    flat = buf[k:k + t.numel()]
    N, C, H, W = t.shape
    v = flat.view(N, H, W, C).permute(0, 3, 1, 2)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + k * t.element_size()
    assert v.stride() == t.stride()
    return v


def _layer(shape, dtype=BF16, cl=True, seed=3, nans=False):
    """Inputs of a pair of layers.  Main and skip differ in everything and
    sit off-centre: activations and means of order 1."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    C = shape[1]

    def rand(scale=1.0, shift=0.0):
        t = torch.randn(shape, generator=g, device=DEV) * scale + shift
        return _cl(t.to(dtype), cl)

    t = {"x": rand(1.0, 1.0), "x_d": rand(2.0, -1.5), "dy": rand(),
         "dy2": rand()}
    if nans:
        for k in ("x", "x_d"):
            flat = _storage_order(t[k], cl)
            idx = torch.randperm(flat.numel(), generator=g, device=DEV)[:5]
            flat[idx] = float("nan")  # a view of the dense tensor
            assert int(torch.isnan(t[k]).sum()) == 5
    for s, off in (("", 1.0), ("2", -1.5)):
        t["w" + s] = torch.randn(C, generator=g, device=DEV).abs() + 0.1
        t["b" + s] = torch.randn(C, generator=g, device=DEV)
        t["mean" + s] = torch.randn(C, generator=g, device=DEV) * 0.3 + off
        t["invstd" + s] = torch.rand(C, generator=g, device=DEV) + 0.5
        t["coefs" + s] = ops.bn_make_coefs(t["mean" + s], t["invstd" + s],
                                           t["w" + s], t["b" + s])
    rows = t["x"].numel() // C
    t["count"] = torch.full((1,), float(rows), device=DEV)
    return t


# ------------------------------------------------------ the two routes, ops
def _composed_fwd(t):
    r = ops.batch_norm_elemt(t["x_d"], t["w2"], t["b2"], t["mean2"],
                             t["invstd2"], EPS)
    r = r.contiguous(memory_format=torch.channels_last) \
        if t["x"].is_contiguous(memory_format=torch.channels_last) else r
    y, gate = ops.batch_norm_elemt_act(
        t["x"], r, t["w"], t["b"], t["mean"], t["invstd"], True, t["coefs"],
        0.0, ops.gate_bits_empty(t["x"]))
    return y, gate, r


def _dual_fwd(t):
    bits = ops.gate_bits_empty(t["x"])
    y, stored = ops.batch_norm_elemt_act_dual(
        t["x"], t["x_d"], t["coefs"], t["coefs2"], True, 0.0, bits)
    return y, (bits if stored else None), stored


def _composed_reduce(t, gate, two, dy2=None):
    dy2 = (t["dy2"] if dy2 is None else dy2) if two else None
    gm = torch.empty_like(t["x"])
    main = ops.batch_norm_backward_reduce_act(
        t["dy"], t["x"], None, t["mean"], t["invstd"], t["w"], t["b"], True,
        True, True, True, t["coefs"], gm, 0.0, dy2, gate=gate)
    skip = ops.batch_norm_backward_reduce(
        gm, t["x_d"], t["mean2"], t["invstd2"], t["w2"], True, True, True)
    return (gm,) + tuple(main) + tuple(skip)


def _dual_reduce(t, gate, two, dy2=None):
    dy2 = (t["dy2"] if dy2 is None else dy2) if two else None
    gm = torch.empty_like(t["x"])
    out = ops.batch_norm_backward_reduce_act(
        t["dy"], t["x"], None, t["mean"], t["invstd"], t["w"], t["b"], True,
        True, True, True, t["coefs"], gm, 0.0, dy2, gate=gate,
        dual=(t["x_d"], t["mean2"], t["invstd2"], t["w2"]))
    assert len(out) == 8
    return (gm,) + tuple(out)


REDUCE_NAMES = ("gm", "sum_dy", "sum_dy_xmu", "grad_weight", "grad_bias",
                "sum_dy_2", "sum_dy_xmu_2", "grad_weight_2", "grad_bias_2")


def _sums_buffer(red, C):
    """The four sums of a dual reduce are views into ONE [4C] buffer."""
    parts = (red[1], red[2], red[5], red[6])
    sums = fused_mod._combined4(parts, C)
    assert sums.data_ptr() == parts[0].data_ptr(), "the sums were copied"
    assert sums.shape == (4 * C,) and sums.dtype == F32
    assert _same(sums, torch.cat(parts))
    return sums


def _composed_elemt(t, red):
    gm = red[0]
    dx = ops.batch_norm_backward_elemt(
        gm, t["x"], t["mean"], t["invstd"], t["w"], red[1], red[2],
        t["count"])
    dx_d = ops.batch_norm_backward_elemt(
        gm, t["x_d"], t["mean2"], t["invstd2"], t["w2"], red[5], red[6],
        t["count"])
    return dx, dx_d


def _dual_elemt(t, gm, sums):
    return ops.batch_norm_backward_elemt_dual(
        gm, t["x"], t["x_d"], t["mean"], t["mean2"], t["invstd"],
        t["invstd2"], t["w"], t["w2"], sums, t["count"])


def _single_numbers(plan):
    return {k: v for k, v in plan.items() if k not in ("gate", "dual")}


def _check_forward(t):
    """Plans, then y and the bits of both routes; returns the bits."""
    x = t["x"]
    p = ops.launch_plan("elemt_dual", x, (t["x_d"], t["coefs2"]), t["coefs"])
    assert p["path"] == "nhwc" and p["dual"] is True and p["V"] == 8, p
    y_c, gate_c, r = _composed_fwd(t)
    assert gate_c is not None
    single = ops.launch_plan("elemt", x, (r, gate_c), t["coefs"])
    assert _single_numbers(p) == _single_numbers(single), (p, single)
    y, gate, stored = _dual_fwd(t)
    assert stored
    assert _same(y, y_c), "y"
    assert _same(gate, gate_c), "gate bits"
    return gate, p


def _check_backward(t, gate, shows=None, dy2=None, want_dual=True,
                    elemt=True):
    x, C = t["x"], t["x"].shape[1]
    gm = torch.empty_like(x)
    dy2_ = t["dy2"] if dy2 is None else dy2
    for two in (False, True):
        p = ops.launch_plan("bwd_reduce_dual", x,
                            (t["dy"], t["x_d"], gm, dy2_ if two else None,
                             gate))
        single = ops.launch_plan("bwd_reduce", x,
                                 (t["dy"], None, gm, dy2_ if two else None,
                                  gate))
        if want_dual or not two:
            assert p["path"] == "nhwc" and p["dual"] is True, p
            assert p["V"] == 8 and p["gate"] is True, p
            assert _single_numbers(p) == _single_numbers(single), (p, single)
            if shows is not None:
                assert shows(p), p
        else:
            assert p["path"] == "ineligible", p
        want = _composed_reduce(t, gate, two, dy2)
        got = _dual_reduce(t, gate, two, dy2)
        for name, a, e in zip(REDUCE_NAMES, got, want):
            assert _same(a, e), (name, two)
        sums = _sums_buffer(got, C)
        if elemt:
            pe = ops.launch_plan("bwd_elemt_dual", x, (got[0], t["x_d"]))
            assert pe["path"] == "nhwc" and pe["dual"] is True, pe
            dx, dx_d = _dual_elemt(t, got[0], sums)
            dx_c, dx_d_c = _composed_elemt(t, want)
            assert _same(dx, dx_c), ("dx", two)
            assert _same(dx_d, dx_d_c), ("dx_d", two)


# (id, shape, dtype, what the reduce plan must show)
CASES = [
    ("one_pack_per_row", (2, 8, 3, 3), BF16,
     lambda p: p["trips"] == 1),
    ("lanes_not_pow2", (2, 24, 5, 5), BF16,
     lambda p: p["lpr"] == 8),
    ("chunks_and_trips", (2, 8, 9, 9), BF16,
     lambda p: p["nchunks"] > 1 and p["trips"] > 1),
    ("nhwc_past_flush", (8, 8, 725, 725), BF16,
     lambda p: p["trips"] > p["flush_every"]),
    ("half_nhwc", (3, 16, 5, 7), F16,
     lambda p: True),
]


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_op_dual_equals_composition(case):
    _, shape, dtype, shows = case
    t = _layer(shape, dtype)
    gate, _ = _check_forward(t)
    _check_backward(t, gate, shows)


@gpu
def test_elementwise_kernels_multi_trip():
    """Forward and backward elemt past one trip of the grid-stride loop."""
    shape = (1, 8, 4, 262152)  # just past 4096*256 packs of 8
    t = _layer(shape, BF16)
    gate, p = _check_forward(t)
    assert p["multi_trip"], p
    gm = t["dy"]  # any tensor of T stands in for the gated gradient
    C = shape[1]
    g = torch.Generator(device=DEV).manual_seed(9)
    sums = torch.randn(4 * C, generator=g, device=DEV)
    pe = ops.launch_plan("bwd_elemt_dual", t["x"], (gm, t["x_d"]))
    assert pe["path"] == "nhwc" and pe["dual"] and pe["multi_trip"], pe
    dx, dx_d = _dual_elemt(t, gm, sums)
    dx_c = ops.batch_norm_backward_elemt(
        gm, t["x"], t["mean"], t["invstd"], t["w"], sums[:C], sums[C:2 * C],
        t["count"])
    dx_d_c = ops.batch_norm_backward_elemt(
        gm, t["x_d"], t["mean2"], t["invstd2"], t["w2"], sums[2 * C:3 * C],
        sums[3 * C:], t["count"])
    assert _same(dx, dx_c) and _same(dx_d, dx_d_c)


@gpu
def test_op_nans_in_both_operands():
    t = _layer((4, 8, 4, 16), BF16, nans=True)
    gate, _ = _check_forward(t)
    _check_backward(t, gate)


@gpu
def test_second_gradient_off_alignment():
    """dy2 one element past an aligned allocation: the single gated reduce
    runs it at a narrower pack; the dual kernel declines, the op runs the
    two single reduces, and the results are equal."""
    t = _layer((4, 8, 4, 16), BF16)
    gate, _ = _check_forward(t)
    _check_backward(t, gate, dy2=_offset_view(t["dy2"], 1), want_dual=False,
                    elemt=False)


# ------------------------------------------------------------------ declines
def _misaligned_x_d():
    t = _layer((4, 8, 4, 16), BF16)
    t["x_d"] = _offset_view(t["x_d"], 1)
    return t


DECLINES = {
    "fp32": lambda: _layer((4, 8, 4, 16), F32),
    "c12": lambda: _layer((4, 12, 4, 4), BF16),
    "misaligned_x_d": _misaligned_x_d,
    "nchw": lambda: _layer((4, 8, 4, 16), BF16, cl=False),
}


def _modules(t, dtype=F32):
    C = t["x"].shape[1]
    bn = SyncBatchNormAct2d(C, relu=True).to(DEV).train()
    bn_skip = SyncBatchNorm(C).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(17)
    with torch.no_grad():
        for m, s in ((bn, ""), (bn_skip, "2")):
            m.weight.copy_(t["w" + s])
            m.bias.copy_(t["b" + s])
            m.running_mean.copy_(torch.randn(C, generator=g, device=DEV))
            m.running_var.copy_(torch.rand(C, generator=g, device=DEV) + 0.5)
    return bn, bn_skip


def _force_function(bn, bn_skip, x, x_d, fork):
    """What bn_add_bn_act does once it has chosen the dual route."""
    for m in (bn_skip, bn):
        m.num_batches_tracked.add_(1)
    return SyncBatchNormDualActFunction.apply(
        x, x_d, bn.weight, bn.bias, bn_skip.weight, bn_skip.bias,
        bn.running_mean, bn.running_var, bn_skip.running_mean,
        bn_skip.running_var, bn.eps, bn_skip.eps, _momentum_factor(bn),
        _momentum_factor(bn_skip), None, 1, fork)


def _run(t, route, fork=False, used="main", x_d_grad=True, saved=None):
    bn, bn_skip = _modules(t)
    x = t["x"].detach().clone(memory_format=torch.preserve_format)
    x_d = t["x_d"].detach()  # keeps a deliberate misalignment
    x.requires_grad_(True)
    x_d = x_d.requires_grad_(x_d_grad) if x_d_grad else x_d
    hooks = torch.autograd.graph.saved_tensors_hooks(
        lambda s: (saved.append(s) if saved is not None else None) or s,
        lambda s: s)
    with hooks:
        if route == "function":
            out = _force_function(bn, bn_skip, x, x_d, fork)
        elif route == "entry":
            out = bn_add_bn_act(bn, bn_skip, x, x_d, fork)
        elif fork:
            out = bn(x, residual=bn_skip(x_d), fork=True)
        else:
            out = bn(x, residual=bn_skip(x_d))
    main, skip = out if fork else (out, None)
    loss = 0
    if used in ("main", "both"):
        loss = loss + (main.float() * t["dy"].float()).sum()
    if used in ("skip", "both"):
        loss = loss + (skip.float() * t["dy2"].float()).sum()
    loss.backward()
    res = [main.detach(), x.grad, x_d.grad]
    for m in (bn, bn_skip):
        res += [m.weight.grad, m.bias.grad, m.running_mean, m.running_var,
                m.num_batches_tracked]
    x_d.grad = None
    return res, (x, x_d)


def _assert_runs_equal(got, want):
    assert len(got) == len(want) == 13
    for i, (a, e) in enumerate(zip(got, want)):
        assert _same(a, e), i


@gpu
@pytest.mark.parametrize("name", list(DECLINES))
def test_declines_and_function_falls_back(name, monkeypatch):
    t = DECLINES[name]()
    p = ops.launch_plan("elemt_dual", t["x"], (t["x_d"], t["coefs2"]),
                        t["coefs"])
    assert p["path"] == "ineligible", p
    y, gate, stored = _dual_fwd(t)
    assert stored is False and y is None and gate is None
    stored_seen = []
    real = ops.batch_norm_elemt_act_dual

    def spy(*a, **kw):
        out = real(*a, **kw)
        stored_seen.append(out[1])
        return out

    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act_dual", spy)
    want, _ = _run(t, "composition")
    got, _ = _run(t, "function")
    assert stored_seen == [False]
    _assert_runs_equal(got, want)


# ------------------------------------------------------------ function level
FORKS = [(False, "main"), (True, "main"), (True, "skip"), (True, "both")]


@gpu
@pytest.mark.parametrize("fork,used", FORKS,
                         ids=[f"fork{int(f)}-{u}" for f, u in FORKS])
def test_function_equals_composition(fork, used, monkeypatch):
    stored_seen = []
    real = ops.batch_norm_elemt_act_dual

    def spy(*a, **kw):
        out = real(*a, **kw)
        stored_seen.append(out[1])
        return out

    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act_dual", spy)
    t = _layer((4, 8, 4, 16), BF16)
    want, _ = _run(t, "composition", fork, used)
    assert stored_seen == []
    got, _ = _run(t, "entry", fork, used)
    assert stored_seen == [True], "bn_add_bn_act did not take the dual route"
    _assert_runs_equal(got, want)


@gpu
def test_skip_input_without_grad():
    t = _layer((4, 8, 4, 16), BF16)
    want, _ = _run(t, "composition", x_d_grad=False)
    got, _ = _run(t, "entry", x_d_grad=False)
    assert got[2] is None
    _assert_runs_equal(got, want)


@gpu
def test_forward_saves_no_tensor_of_the_outputs_size_but_x_and_x_d():
    t = _layer((4, 8, 4, 16), BF16)
    saved = []
    res, (x, x_d) = _run(t, "entry", saved=saved)
    assert saved
    numel = res[0].numel()
    own = {x.data_ptr(), x_d.data_ptr()}
    big = [s for s in saved if s is not None and s.numel() >= numel]
    assert big and all(s.data_ptr() in own for s in big), \
        [(s.shape, s.dtype) for s in big]
    assert any(s is not None and s.dtype == torch.uint8
               and s.numel() == numel // 8 for s in saved)


# -------------------------------------------------------------------- memory
@gpu
def test_bottleneck_with_downsample_memory():
    """Held after the forward: the same bytes (the skip BN's output was
    already released with gate bits).  Peak during the forward: lower by at
    least that tensor, which no longer exists.  16384 output elements: a
    whole number of allocator blocks.

    Measured on an MI355X: held 140800 B on both routes; peak above the
    starting point 173568 B composed, 140800 B dual: numel*itemsize =
    32768 B lower, and nothing is alive during the dual forward that is not
    held after it (the function keeps one count for the pair and the skip
    layer's [scale | shift], which its kernel reads while y exists)."""
    held, peak = {}, {}
    for dual_bn in (False, True):
        torch.manual_seed(0)
        down = torch.nn.Sequential(conv1x1(64, 64), SyncBatchNorm(64))
        block = Bottleneck(64, 16, 1, down, fused=True, dual_bn=dual_bn)
        block = block.to(DEV, BF16).to(memory_format=torch.channels_last)
        block.train()
        x = _cl(torch.randn(4, 64, 8, 8, device=DEV).to(BF16))
        x.requires_grad_(True)
        block(x)  # warm-up: MIOpen's own allocations
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = block(x)
        torch.cuda.synchronize()
        held[dual_bn] = torch.cuda.memory_allocated() - before
        peak[dual_bn] = torch.cuda.max_memory_allocated() - before
        numel, itemsize = out.numel(), out.element_size()
        del out
    print("held", held, "peak", peak)
    assert numel == 16384
    assert held[True] == held[False], held
    assert peak[False] - peak[True] >= numel * itemsize, peak


# --------------------------------------------------------------- model level
def _model(factory, dtype, dual_bn):
    torch.manual_seed(0)
    m = factory(num_classes=10, fused=True, dual_bn=dual_bn)
    return m.to(DEV, dtype).to(memory_format=torch.channels_last).train()


def _step(m, x, y):
    xg = x.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(m(xg).float(), y)
    loss.backward()
    return loss.detach(), xg.grad


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bfloat16", "float32"])
@pytest.mark.parametrize("factory,stages", [(resnet18, 3), (resnet50, 4)],
                         ids=["resnet18", "resnet50"])
def test_model_dual_on_equals_off(factory, stages, dtype, monkeypatch):
    """Loss, every BN affine gradient and the input-image gradient are
    bit-equal.  MIOpen's default solvers vary from run to run at these
    shapes, so the deterministic ones are asked for and the yardstick is
    first checked to repeat itself."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    stored_seen = []
    real = ops.batch_norm_elemt_act_dual

    def spy(*a, **kw):
        out = real(*a, **kw)
        stored_seen.append(out[1])
        return out

    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act_dual", spy)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = _cl(torch.randn(4, 3, 64, 64, generator=g, device=DEV).to(dtype))
    y = torch.randint(0, 10, (4,), generator=g, device=DEV)

    on, off = _model(factory, dtype, True), _model(factory, dtype, False)
    loss_a, dx_a = _step(on, x, y)
    # the first block of every stage with a downsample, bf16 only
    assert stored_seen == [True] * (stages if dtype == BF16 else 0)
    del stored_seen[:]
    loss_b, dx_b = _step(off, x, y)
    loss_c, dx_c = _step(_model(factory, dtype, False), x, y)
    assert stored_seen == []
    assert torch.equal(loss_b, loss_c) and torch.equal(dx_b, dx_c), \
        "the model does not repeat itself: convolutions vary"

    assert torch.equal(loss_a, loss_b)
    assert torch.equal(dx_a, dx_b)
    n_bn = 0
    for (n, p), (_, q) in zip(on.named_parameters(), off.named_parameters()):
        if p.dim() == 1 and "bn" in n or "downsample.1" in n:
            assert torch.equal(p.grad, q.grad), n
            n_bn += 1
    assert n_bn == 2 * (20 if factory is resnet18 else 53)
    for (n, p), (_, q) in zip(on.named_buffers(), off.named_buffers()):
        assert torch.equal(p, q), n


@gpu
def test_hooked_skip_bn_keeps_the_composition(monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the dual function ran past a hook")

    monkeypatch.setattr(fused_mod.SyncBatchNormDualActFunction, "apply",
                        never)
    t = _layer((4, 8, 4, 16), BF16)
    bn, bn_skip = _modules(t)
    seen = []
    bn_skip.register_forward_hook(lambda m, i, o: seen.append(1))
    x = t["x"].detach().requires_grad_(True)
    bn_add_bn_act(bn, bn_skip, x, t["x_d"]).float().sum().backward()
    assert seen == [1] and x.grad is not None


# ------------------------------------------------------ world-1 forced sync
@gpu
def test_forced_sync_world1():
    """Under MSBN_FORCE_SYNC on an RCCL group the pair sends ONE [4C]
    backward all_reduce, and dual on and off give equal gradients."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               PYTHONPATH=REPO, MSBN_COMM_LOG="1")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", "nccl_world1_check.py"),
         "dual"],
        capture_output=True, text=True, timeout=300, cwd=REPO, env=env,
    )
    assert r.returncode == 0 and "CASE dual OK" in r.stdout, (
        f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    )
