"""Gate bits on the GPU: the forward of a bn+add+act layer stores the
activation's branch as one bit per element and the backward reduce reads the
bit instead of re-reading the residual (docs/KERNEL_DESIGN.md "Gate bits").

The oracle throughout is the existing residual route on the same inputs, and
every comparison is ``torch.equal``: the change claims to move no bit.  Both
routes run the same kernel code after the gate, at the same vector width
(the bits are bytes and make no alignment demand), so their sums are formed
in the same order.

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
from msbn.nn.fused import SyncBatchNormActFunction

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = 1e-5
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _cl(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) \
        if channels_last else t.contiguous()


def _storage_order(t, channels_last):
    """The elements of a dense tensor in the order of their storage."""
    return (t.permute(0, 2, 3, 1) if channels_last else t).reshape(-1)


def _unpack(bits, numel):
    shifts = torch.arange(8, device=bits.device, dtype=torch.uint8)
    return ((bits[:, None] >> shifts) & 1).reshape(-1)[:numel].bool()


def _offset_view(t, k, channels_last):
    """A copy of t living k ELEMENTS past an aligned allocation."""
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=t.device)
    flat = buf[k:k + t.numel()]
    if channels_last:
        N, C, H, W = t.shape
        v = flat.view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        v = flat.view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + k * t.element_size()
    assert v.stride() == t.stride()
    return v


def _layer(shape, dtype, cl, seed=3, nans=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    C = shape[1]

    def rand():
        return _cl(torch.randn(shape, generator=g, device=DEV).to(dtype), cl)

    t = {k: rand() for k in ("x", "res", "dy", "dy2")}
    if nans:
        flat = _storage_order(t["x"], cl)
        idx = torch.randperm(flat.numel(), generator=g, device=DEV)[:5]
        # _storage_order of a dense tensor is a view: writes reach x
        flat[idx] = float("nan")
        assert int(torch.isnan(t["x"]).sum()) == 5
    t["w"] = torch.randn(C, generator=g, device=DEV).abs() + 0.1
    t["b"] = torch.randn(C, generator=g, device=DEV)
    t["mean"] = torch.randn(C, generator=g, device=DEV) * 0.1
    t["invstd"] = torch.rand(C, generator=g, device=DEV) + 0.5
    t["coefs"] = ops.bn_make_coefs(t["mean"], t["invstd"], t["w"], t["b"])
    return t


def _forward(t, slope, want_bits=True):
    """y of the plain call, and (y, gate) of the call with gate_out."""
    args = (t["x"], t["res"], t["w"], t["b"], t["mean"], t["invstd"], True,
            t["coefs"], slope)
    y = ops.batch_norm_elemt_act(*args)
    y_g, gate = ops.batch_norm_elemt_act(*args, ops.gate_bits_empty(t["x"]))
    assert torch.equal(y.view(torch.int16), y_g.view(torch.int16))
    assert (gate is not None) == want_bits
    if gate is not None:
        assert t["x"].numel() % 8 == 0  # V = 8: no partial last byte
        assert gate.dtype == torch.uint8
        assert gate.numel() == t["x"].numel() // 8
    return y, gate


def _reduce(t, slope, two, gate, dy=None, dy2=None):
    dy = t["dy"] if dy is None else dy
    dy2 = (t["dy2"] if dy2 is None else dy2) if two else None
    gm = torch.empty_like(t["x"])
    out = ops.batch_norm_backward_reduce_act(
        dy, t["x"], None if gate is not None else t["res"], t["mean"],
        t["invstd"], t["w"], t["b"], True, True, True, True, t["coefs"], gm,
        slope, dy2, gate=gate)
    return (gm,) + tuple(out)


def _same(a, b):
    """torch.equal that also holds for NaNs in the same places."""
    return a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _both_routes(t, slope, gate, **dys):
    for two in (False, True):
        want = _reduce(t, slope, two, None, **dys)
        got = _reduce(t, slope, two, gate, **dys)
        for name, a, e in zip(("gm", "sum_dy", "sum_dy_xmu", "grad_weight",
                               "grad_bias"), got, want):
            assert _same(a, e), (name, two)


def _plans(t, gate, dy=None, dy2=None):
    x = t["x"]
    dy = t["dy"] if dy is None else dy
    dy2 = t["dy2"] if dy2 is None else dy2
    gm = torch.empty_like(x)
    p_gate = ops.launch_plan("bwd_reduce", x, (dy, None, gm, dy2, gate))
    p_res = ops.launch_plan("bwd_reduce", x, (dy, t["res"], gm, dy2))
    assert p_gate["gate"] is True
    assert "gate" not in p_res
    assert {k: v for k, v in p_gate.items() if k != "gate"} == p_res
    assert ops.launch_plan("bwd_reduce", x,
                           (dy, t["res"], gm, dy2, None))["gate"] is False
    return p_gate


# (id, shape, dtype, channels_last, what the reduce plan must show)
CASES = [
    ("one_pack_per_row", (2, 8, 3, 3), BF16, True,
     lambda p: p["path"] == "nhwc" and p["V"] == 8 and p["trips"] == 1),
    ("lanes_not_pow2", (2, 24, 5, 5), BF16, True,
     lambda p: p["path"] == "nhwc" and p["V"] == 8 and p["lpr"] == 8),
    ("chunks_and_trips", (2, 8, 9, 9), BF16, True,
     lambda p: p["path"] == "nhwc" and p["nchunks"] > 1 and p["trips"] > 1),
    ("nhwc_past_flush", (8, 8, 725, 725), BF16, True,
     lambda p: p["path"] == "nhwc" and p["V"] == 8
     and p["trips"] > p["flush_every"]),
    ("nchw_vec_past_flush", (1030, 256, 2, 4), BF16, False,
     lambda p: p["path"] == "nchw_vec" and p["V"] == 8
     and p["trips"] > p["flush_every"]),
    ("nchw_vec_s64", (4, 8, 4, 16), BF16, False,
     lambda p: p["path"] == "nchw_vec" and p["V"] == 8),
    ("half_nhwc", (3, 16, 5, 7), F16, True,
     lambda p: p["path"] == "nhwc" and p["V"] == 8),
    ("half_nchw", (6, 5, 12, 20), F16, False,
     lambda p: p["path"] == "nchw_vec" and p["V"] == 8),
]


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_op_gate_route_equals_residual_route(case):
    _, shape, dtype, cl, shows = case
    t = _layer(shape, dtype, cl)
    plan = ops.launch_plan("elemt", t["x"], (t["res"], ops.gate_bits_empty(
        t["x"])), t["coefs"])
    assert plan["gate"] is True and plan["V"] == 8, plan
    assert "gate" not in ops.launch_plan("elemt", t["x"], (t["res"],),
                                         t["coefs"])
    y, gate = _forward(t, 0.0)
    # relu on randn data: no positive fp32 z underflows the 16-bit y
    assert torch.equal(_unpack(gate, y.numel()), _storage_order(y, cl) > 0)
    p = _plans(t, gate)
    assert shows(p), p
    _both_routes(t, 0.0, gate)


@gpu
def test_forward_multi_trip_stores_every_byte():
    shape = (1, 8, 4, 262152)  # just past 4096*256 packs of 8
    t = _layer(shape, BF16, True)
    plan = ops.launch_plan("elemt", t["x"], (t["res"], ops.gate_bits_empty(
        t["x"])), t["coefs"])
    assert plan["multi_trip"] and plan["gate"], plan
    y, gate = _forward(t, 0.0)
    assert torch.equal(_unpack(gate, y.numel()), _storage_order(y, True) > 0)


@gpu
@pytest.mark.parametrize("slope", [0.1, -0.5], ids=["leaky0.1", "leaky-0.5"])
@pytest.mark.parametrize("cl", [True, False], ids=["nhwc", "nchw"])
def test_op_leaky(cl, slope):
    t = _layer((4, 8, 4, 16), BF16, cl)
    y, gate = _forward(t, slope)
    z = (t["x"].float() * t["coefs"][:8].view(1, 8, 1, 1)
         + t["coefs"][8:].view(1, 8, 1, 1) + t["res"].float())
    # away from z == 0 the bit is the sign of z
    far = _storage_order(z.abs() > 1e-3, cl)
    assert torch.equal(_unpack(gate, y.numel())[far],
                       _storage_order(z > 0, cl)[far])
    _plans(t, gate)
    _both_routes(t, slope, gate)


@gpu
@pytest.mark.parametrize("slope", [0.0, 0.1], ids=["relu", "leaky"])
@pytest.mark.parametrize("cl", [True, False], ids=["nhwc", "nchw"])
def test_op_nan_rule(cl, slope):
    """A NaN z passes the gradient under relu and takes the slope branch
    under leaky, exactly as the recomputing kernels do."""
    t = _layer((4, 8, 4, 16), BF16, cl, nans=True)
    _, gate = _forward(t, slope)
    nan_at = _storage_order(torch.isnan(t["x"]), cl)
    bits = _unpack(gate, nan_at.numel())
    assert bits[nan_at].all() if slope == 0.0 else not bits[nan_at].any()
    _both_routes(t, slope, gate)


@gpu
@pytest.mark.parametrize("which", ["dy", "dy2"])
@pytest.mark.parametrize("k,want_v", [(1, 1), (4, 4)], ids=["V1", "V4"])
@pytest.mark.parametrize("cl,path", [(True, "nhwc"), (False, "nchw")],
                         ids=["nhwc", "nchw"])
def test_mixed_pack_widths(cl, path, k, want_v, which):
    """The forward ran at V = 8; a misaligned gradient makes the reduce run
    at V = 1 (contiguous: the nchw_flat kernel) or V = 4."""
    t = _layer((4, 8, 4, 16), BF16, cl)  # S = 64
    _, gate = _forward(t, 0.1)
    dys = {which: _offset_view(t[which], k, cl)}
    p = _plans(t, gate, **dys)
    assert p["V"] == want_v, p
    if not cl:
        assert p["path"] == ("nchw_flat" if want_v == 1 else "nchw_vec"), p
    _both_routes(t, 0.1, gate, **dys)
    _both_routes(t, 0.0, _forward(t, 0.0)[1], **dys)


# ------------------------------------------------------------- autograd
def _apply(t, gate_bits, slope=0.0, fork=False, res_grad=True):
    """One SyncBatchNormActFunction layer; returns results and what it
    saved."""
    x = t["x"].detach().requires_grad_(True)
    res = t["res"].detach().requires_grad_(res_grad)
    w = t["w"].detach().requires_grad_(True)
    b = t["b"].detach().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(
            lambda s: saved.append(s) or s, lambda s: s):
        out = SyncBatchNormActFunction.apply(
            x, res, w, b, None, None, EPS, 0.1, None, 1, True, slope, fork,
            gate_bits)
    return x, res, w, b, out, saved


def _saved_kinds(saved, res):
    has_bits = any(s.dtype == torch.uint8 for s in saved)
    has_res = any(s.data_ptr() == res.data_ptr() and s.dtype == res.dtype
                  for s in saved)
    return has_bits, has_res


def _function_equal(t, slope=0.0, want_bits=True):
    outs = []
    for gate_bits in (True, False):
        x, res, w, b, y, saved = _apply(t, gate_bits, slope)
        has_bits, has_res = _saved_kinds(saved, res)
        assert has_bits == (gate_bits and want_bits)
        assert has_res == (not has_bits)
        y.backward(t["dy"])
        outs.append((y.detach(), x.grad, res.grad, w.grad, b.grad))
    for a, e in zip(*outs):
        assert _same(a, e)


@gpu
@pytest.mark.parametrize("slope", [0.0, 0.1], ids=["relu", "leaky"])
@pytest.mark.parametrize("cl", [True, False], ids=["nhwc", "nchw"])
def test_function_saves_bits_not_residual(cl, slope):
    _function_equal(_layer((4, 8, 4, 16), BF16, cl), slope)


DECLINES = {
    "fp32": lambda: _layer((4, 8, 4, 16), F32, True),
    "nhwc_c12": lambda: _layer((4, 12, 4, 4), BF16, True),
    "nchw_s49": lambda: _layer((2, 8, 7, 7), BF16, False),
}


def _misaligned(which):
    def make():
        t = _layer((4, 8, 4, 16), BF16, True)
        t[which] = _offset_view(t[which], 1, True)
        return t
    return make


DECLINES["misaligned_x"] = _misaligned("x")
DECLINES["misaligned_res"] = _misaligned("res")


@gpu
@pytest.mark.parametrize("name", list(DECLINES))
def test_forward_declines_and_keeps_the_residual(name):
    t = DECLINES[name]()
    plan = ops.launch_plan("elemt", t["x"], (t["res"], ops.gate_bits_empty(
        t["x"])), t["coefs"])
    assert plan["gate"] is False and plan["V"] != 8, plan
    if t["x"].dtype != F32:
        _forward(t, 0.0, want_bits=False)
    _function_equal(t, 0.0, want_bits=False)


@gpu
def test_no_bits_for_a_residual_without_grad(monkeypatch):
    asked = []
    real = ops.batch_norm_elemt_act

    def spy(*a, **kw):
        asked.append(len(a) > 9 or kw.get("gate_out") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act", spy)
    t = _layer((4, 8, 4, 16), BF16, True)
    x, res, w, b, y, saved = _apply(t, True, res_grad=False)
    assert asked == [False]
    assert _saved_kinds(saved, res) == (False, True)
    y.backward(t["dy"])
    assert res.grad is None
    del asked[:]
    _apply(t, True)
    assert asked == [True]


@gpu
@pytest.mark.parametrize("used", ["main", "skip", "both"])
def test_fork_with_one_or_two_gradients(used):
    t = _layer((4, 8, 4, 16), BF16, True)
    outs = []
    for gate_bits in (True, False):
        x, res, w, b, (y, skip), saved = _apply(t, gate_bits, fork=True)
        assert _saved_kinds(saved, res)[0] == gate_bits
        loss = 0
        if used in ("main", "both"):
            loss = loss + (y.float() * t["dy"].float()).sum()
        if used in ("skip", "both"):
            loss = loss + (skip.float() * t["dy2"].float()).sum()
        loss.backward()
        outs.append((x.grad, res.grad, w.grad, b.grad))
    for a, e in zip(*outs):
        assert _same(a, e)


@gpu
def test_small_plane_path_never_sees_bits(monkeypatch):
    def no_bits(*a, **kw):
        raise AssertionError("the two-stage forward ran")

    t = _layer((4, 64, 16, 16), BF16, False)
    assert ops.launch_plan("fused_local", t["x"],
                           (t["res"],))["path"] == "small_plane"
    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act", no_bits)
    x, res, w, b, y, saved = _apply(t, True)
    assert _saved_kinds(saved, res) == (False, True)
    y.backward(t["dy"])
    assert res.grad is not None


# ---------------------------------------------------------- saved memory
@gpu
def test_bottleneck_with_downsample_holds_less():
    """The downsample BN's output is only alive as the closing BN's saved
    residual: with gate bits it is released when the forward returns, and
    the block holds numel*itemsize - numel/8 bytes less.  16384 output
    elements: both sizes are whole allocator blocks."""
    held = {}
    for gate_bits in (False, True):
        torch.manual_seed(0)
        down = torch.nn.Sequential(conv1x1(64, 64), SyncBatchNorm(64))
        block = Bottleneck(64, 16, 1, down, fused=True, gate_bits=gate_bits)
        block = block.to(DEV, BF16).to(memory_format=torch.channels_last)
        block.train()
        x = _cl(torch.randn(4, 64, 8, 8, device=DEV).to(BF16), True)
        x.requires_grad_(True)
        block(x)  # warm-up: MIOpen's own allocations
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = block(x)
        torch.cuda.synchronize()
        held[gate_bits] = torch.cuda.memory_allocated() - before
        numel, itemsize = out.numel(), out.element_size()
        del out
    assert numel == 16384
    assert held[False] - held[True] == numel * itemsize - numel // 8, held


# ------------------------------------------------------------ model level
def _model(factory, dtype, gate_bits):
    torch.manual_seed(0)
    m = factory(num_classes=10, fused=True, gate_bits=gate_bits)
    return m.to(DEV, dtype).to(memory_format=torch.channels_last).train()


def _step(m, x, y):
    xg = x.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(m(xg).float(), y)
    loss.backward()
    return loss.detach(), xg.grad


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bfloat16", "float32"])
@pytest.mark.parametrize("factory,blocks", [(resnet18, 8), (resnet50, 16)],
                         ids=["resnet18", "resnet50"])
def test_model_gate_bits_on_equals_off(factory, blocks, dtype, monkeypatch):
    """Loss, every BN affine gradient and the input-image gradient are
    bit-equal.  MIOpen's default solvers vary from run to run at these
    shapes (tests/test_gpu_grad_fork.py), so the deterministic ones are
    asked for and the yardstick is first checked to repeat itself."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    gated = []
    real = ops.batch_norm_backward_reduce_act

    def counting(*a, **kw):
        gated.append(kw.get("gate") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(fused_mod.ops, "batch_norm_backward_reduce_act",
                        counting)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = _cl(torch.randn(4, 3, 64, 64, generator=g, device=DEV).to(dtype),
            True)
    y = torch.randint(0, 10, (4,), generator=g, device=DEV)

    on, off = _model(factory, dtype, True), _model(factory, dtype, False)
    loss_a, dx_a = _step(on, x, y)
    # every closing BN of a bf16 model, none of an fp32 one
    assert sum(gated) == (blocks if dtype == BF16 else 0), gated
    del gated[:]
    loss_b, dx_b = _step(off, x, y)
    assert sum(gated) == 0
    loss_c, dx_c = _step(_model(factory, dtype, False), x, y)
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


# ------------------------------------------------------ world-1 forced sync
@gpu
def test_forced_sync_world1():
    """Under MSBN_FORCE_SYNC the statistics go through the collectives; the
    bits are local, so both routes hand them the same bytes."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               PYTHONPATH=REPO)
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", "nccl_world1_check.py"),
         "gate"],
        capture_output=True, text=True, timeout=300, cwd=REPO, env=env,
    )
    assert r.returncode == 0 and "CASE gate OK" in r.stdout, (
        f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    )
