"""Grouped BN (one BatchNorm over S tensors, each with its own statistics)
against float64 references per segment.

Bounds are those of tests/test_gpu_reduction_edges.py: ``_stat_bounds`` for
mean / invstd and what follows from them for the coefficients; the running
statistics after S sequential updates carry the sum of the S single-update
bounds (a later update scales an earlier error by 1 - momentum <= 1);
outputs: half an ulp of the dtype, the coefficient bounds propagated through
``x*scale + shift`` and 4u of its fp32 evaluation; gradients: ``_tol``.
Segment s sits at a mean of about 3*s, so anything that leaked across a
segment boundary would be off by whole units.  For ReLU, elements whose gate
rounding could flip (|z| < 0.1) carry no upstream gradient.
"""

import socket

import pytest
import torch
import torch.distributed as dist

import oracle64 as o64
import test_gpu_reduction_edges as edges
from msbn import ops
from msbn.models.retinanet import RetinaNet
from msbn.nn import SyncBatchNorm
from msbn.nn.batchnorm import _NormBase
from msbn.nn.fused import SyncBatchNormAct2d, bn_act_grouped

pytestmark = pytest.mark.gpu

DEV, EPS, U, MOM = "cuda:0", 1e-5, 2.0 ** -24, 0.1
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
HALF_ULP = {F32: U, BF16: 2.0 ** -8, F16: 2.0 ** -11}
PYRAMID = [(2, 13, 21), (2, 7, 11), (2, 4, 6), (2, 2, 3), (2, 1, 2)]

# name -> (C, [(N, H, W)], off-centre segment or None, what the plans must say)
GROUPS = {
    "single": (16, [(2, 5, 7)], None, lambda r, e: r["nchunks"] == [1]),
    # 546 rows at 128 per chunk: four full chunks and a partial one
    "pyramid": (16, PYRAMID, None, lambda r, e: r["chunk_rows"] == 128
                and r["nchunks"] == [5, 2, 1, 1, 1]
                and r["first_block"] == [0, 5, 7, 8, 9]),
    # a 20-row segment (< one chunk) between two 300-row ones whose last
    # chunk is partial; 72 channels are two (fp32: three) channel tiles
    "eight": (72, [(2, 10, 15), (1, 4, 5), (3, 10, 10), (2, 4, 5), (2, 2, 2),
                   (1, 8, 8), (1, 1, 7), (2, 5, 13)], None,
              lambda r, e: r["ctiles"] >= 2 and r["nchunks"][1] == 1
              and r["nchunks"][0] >= 2 and r["nchunks"][2] >= 2
              and 20 < r["chunk_rows"] and 300 % r["chunk_rows"] != 0),
    "second_trip": (16, [(2, 512, 520), (2, 3, 5)], None,
                    lambda r, e: e["multi_trip"] and e["trips"] >= 2),
    "offcentre": (16, [(2, 6, 7), (3, 10, 10), (2, 5, 5)], 1,
                  lambda r, e: True),
}
DTYPES = [pytest.param(d, id=str(d)[6:]) for d in (F32, BF16, F16)]
_cache = {}


def _case(name, dtype):
    """Inputs, plans and the float64 statistics, once per (group, dtype)."""
    if (name, dtype) not in _cache:
        C, shapes, off, want = GROUPS[name]
        g = edges._gen(len(name) + C)
        xs = []
        for s, (n, h, w) in enumerate(shapes):
            x = edges._randn((n, C, h, w), g) + 3.0 * s
            if s == off:
                x = 8 + 0.05 * edges._randn((n, C, h, w), g)
            xs.append(edges._cl(x.to(dtype), True))
        red = ops.launch_plan("stats_grouped", xs[0], xs[1:])
        elt = ops.launch_plan("elemt_grouped", xs[0], xs[1:])
        assert red["path"] == elt["path"] == "nhwc", (red, elt)
        assert red["S"] == len(xs) and red["V"] == 16 // xs[0].element_size()
        assert want(red, elt), (red, elt)
        stats = [o64.stats(x, EPS) for x in xs]
        if off is not None:
            cond = stats[off][0] ** 2 / stats[off][1]
            assert (cond >= 1e4).all(), cond.min()
        w, b = edges._affine(C, C)
        _cache[name, dtype] = (xs, stats, w, b)
    return _cache[name, dtype]


def _coef_bounds(mean, var, w, b):
    rtol, matol = edges._stat_bounds(mean, var)
    scale, shift = o64.coefs(mean, torch.rsqrt(var + EPS), w, b)
    scale_b = (rtol + 2 * U) * scale.abs()
    shift_b = (mean.abs() * scale_b + matol * scale.abs()
               + 2 * U * ((mean * scale).abs() + b.double().abs()))
    return scale, shift, scale_b, shift_b


def _running_chain(rm0, rv0, stats, counts, momentum=MOM):
    """(want_mean, want_var, bound_mean, bound_var) of the running statistics
    after one update per segment, in order, from each segment's float64
    (mean, var, ...) and element count: the S single-update bounds summed."""
    want_m, want_v = rm0.double(), rv0.double()
    bound_m = bound_v = 0.0
    for (m64, v64, *_), n in zip(stats, counts):
        rtol, matol = edges._stat_bounds(m64, v64)
        unb = v64 * (n / (n - 1.0))
        bound_m = bound_m + momentum * matol + 4 * U * (
            (1 - momentum) * want_m.abs() + momentum * m64.abs())
        bound_v = bound_v + momentum * 2 * rtol * (unb + EPS) + 4 * U * (
            (1 - momentum) * want_v.abs() + momentum * unb)
        want_m, want_v = o64.running_update(want_m, want_v, m64, v64, n,
                                            momentum)
    return want_m, want_v, bound_m, bound_v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(GROUPS))
def test_statistics_and_outputs(name, dtype):
    xs, stats, w, b = _case(name, dtype)
    C, S = xs[0].shape[1], len(xs)
    g = edges._gen(7)
    rm0, rv0 = edges._randn((C,), g), torch.rand(C, generator=g,
                                                 device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, count, coefs = ops.batch_norm_stats_local_grouped(
        xs, EPS, rm, rv, MOM, w, b)
    ys = ops.batch_norm_elemt_act_grouped(xs, coefs, True)
    assert mean.shape == invstd.shape == (S, C) and coefs.shape == (S, 2 * C)
    want_m, want_v, bound_m, bound_v = _running_chain(
        rm0, rv0, stats, [x.numel() // C for x in xs])
    for s, (x, (m64, v64, _)) in enumerate(zip(xs, stats)):
        n = x.numel() // C
        assert count[s].item() == n >= 2
        edges._check_stats(f"seg{s}", mean[s], invstd[s], m64, v64)
        edges._check_coefs(f"seg{s}", coefs[s], m64, v64, w, b)
        scale, shift, scale_b, shift_b = _coef_bounds(m64, v64, w, b)
        xd, ch = x.double(), lambda t: o64.chan(t, 4)
        ref = torch.relu(xd * ch(scale) + ch(shift))
        edges._within(
            f"seg{s} y", ys[s], ref,
            HALF_ULP[dtype] * ref.abs() + xd.abs() * ch(scale_b) + ch(shift_b)
            + 4 * U * ((xd * ch(scale)).abs() + ch(shift).abs()))
        assert ys[s].is_contiguous(memory_format=torch.channels_last)
    edges._within("running_mean", rm, want_m, bound_m)
    edges._within("running_var", rv, want_v, bound_v)


def _layer(name, dtype, relu):
    """bn_act_grouped forward + backward against float64, per segment."""
    xs, stats, w, b = _case(name, dtype)
    C = xs[0].shape[1]
    bn = (SyncBatchNormAct2d(C) if relu else SyncBatchNorm(C)).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
    g = edges._gen(13)
    leaves = [x.clone().requires_grad_(True) for x in xs]
    launched = []
    real = ops.batch_norm_elemt_act_grouped
    ops.batch_norm_elemt_act_grouped = \
        lambda *a: launched.append(1) or real(*a)
    try:
        ys = bn_act_grouped(bn, leaves)
    finally:
        ops.batch_norm_elemt_act_grouped = real
    assert launched == [1] and int(bn.num_batches_tracked) == len(xs)
    dgamma = dbeta = 0.0
    gouts, wants = [], []
    for x, (m64, v64, i64) in zip(xs, stats):
        z = o64.pre_activation(x, m64, i64, w, b)
        keep = (z.abs() >= 0.1) if relu else torch.ones_like(z, dtype=bool)
        gout = edges._cl(edges._randn(x.shape, g, dtype) * keep, True)
        r = o64.backward_reduce(gout, x, m64, i64, w, b, None, relu)
        dx, _ = o64.backward_elemt(gout, x, m64, i64, w, b, r["sum_dy"],
                                   r["sum_dy_xmu"], x.numel() // C, None,
                                   relu)
        dgamma, dbeta = dgamma + r["grad_weight"], dbeta + r["grad_bias"]
        gouts.append(gout)
        wants.append((o64.activation(z, relu), dx))
    torch.autograd.backward(ys, gouts)
    tol = edges._tol(dtype)
    for s, (y, leaf, (wy, wdx)) in enumerate(zip(ys, leaves, wants)):
        torch.testing.assert_close(y.double(), wy, **tol,
                                   msg=lambda m: f"y[{s}] {m}")
        torch.testing.assert_close(leaf.grad.double(), wdx, **tol,
                                   msg=lambda m: f"dx[{s}] {m}")
    torch.testing.assert_close(bn.weight.grad.double(), dgamma, **tol)
    torch.testing.assert_close(bn.bias.grad.double(), dbeta, **tol)


# the off-centre group is a statistics case: at mean^2/var >= 1e4 the fp32
# dx = a*g + b*x + d cancels past _tol(fp32) in any evaluation order
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "none"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [n for n in GROUPS if n != "offcentre"])
def test_layer_against_float64(name, dtype, relu):
    _layer(name, dtype, relu)


@pytest.fixture
def world1(monkeypatch):
    monkeypatch.setenv("MSBN_FORCE_SYNC", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        monkeypatch.setenv("MASTER_PORT", str(s.getsockname()[1]))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    calls = []
    for fn in ("all_gather_into_tensor", "all_reduce"):
        real = getattr(dist, fn)
        monkeypatch.setattr(
            dist, fn, lambda *a, _r=real, _f=fn, **k: calls.append(_f)
            or _r(*a, **k))
    yield calls
    dist.destroy_process_group()


def test_forced_sync_world1(world1):
    _layer("pyramid", BF16, True)
    assert world1 == ["all_gather_into_tensor", "all_reduce"]
    # the join() shadow step: N = 0 on this rank
    del world1[:]
    bn, twin = SyncBatchNorm(16).to(DEV), SyncBatchNorm(16).to(DEV)
    xs = [torch.empty((0, 16, h, w), device=DEV, dtype=BF16)
          .contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for _, h, w in PYRAMID]
    ys = bn_act_grouped(bn, xs, relu=True)
    assert [y.shape for y in ys] == [x.shape for x in xs]
    torch.autograd.backward(ys, [torch.empty_like(y) for y in ys])
    assert world1 == ["all_gather_into_tensor", "all_reduce"]
    assert all(x.grad is not None and x.grad.shape == x.shape for x in xs)
    for x in xs:
        twin(x.detach())
    assert torch.equal(bn.running_mean, twin.running_mean)
    assert torch.equal(bn.running_var, twin.running_var)
    assert int(bn.num_batches_tracked) == int(twin.num_batches_tracked) == 5


@pytest.mark.parametrize("kind", ["nchw", "nine", "momentum_none",
                                  "misaligned"])
def test_ineligible_groups_run_the_loop(kind, monkeypatch):
    g = edges._gen(9)
    shapes = PYRAMID + PYRAMID[:4] if kind == "nine" else PYRAMID
    xs = [edges._cl(edges._randn((n, 16, h, w), g, BF16), kind != "nchw")
          for n, h, w in shapes]
    if kind == "misaligned":
        buf = torch.empty(xs[2].numel() + 1, dtype=BF16, device=DEV)
        v = buf[1:].view(2, 4, 6, 16).permute(0, 3, 1, 2)
        xs[2] = v.copy_(xs[2])
        assert v.is_contiguous(memory_format=torch.channels_last)
        assert v.data_ptr() % 16 != 0
    momentum = None if kind == "momentum_none" else 0.1
    bn = SyncBatchNormAct2d(16, momentum=momentum).to(DEV)
    twin = SyncBatchNormAct2d(16, momentum=momentum).to(DEV)
    if kind != "momentum_none":
        for k in ("stats_grouped", "elemt_grouped"):
            assert ops.launch_plan(k, xs[0], xs[1:])["path"] == "ineligible"
    monkeypatch.setattr(ops, "batch_norm_elemt_act_grouped", None)  # unused
    got = bn_act_grouped(bn, xs)
    assert all(torch.equal(a, twin(x)) for a, x in zip(got, xs))
    assert torch.equal(bn.running_mean, twin.running_mean)
    assert torch.equal(bn.running_var, twin.running_var)
    assert int(bn.num_batches_tracked) == len(xs)


def test_retinanet_grouped_heads_step(monkeypatch):
    def build(grouped):
        torch.manual_seed(5)
        model = RetinaNet(num_classes=8, grouped_heads=grouped).to(DEV)
        model = model.to(BF16).to(memory_format=torch.channels_last).train()
        for m in model.modules():  # BatchNorm stays fp32, as in training
            if isinstance(m, _NormBase):
                m.float()
        return model

    launched = []
    real = ops.batch_norm_elemt_act_grouped
    monkeypatch.setattr(ops, "batch_norm_elemt_act_grouped",
                        lambda *a: launched.append(1) or real(*a))
    model, twin = build(True), build(False)
    twin.load_state_dict(model.state_dict())
    x = torch.randn(2, 3, 64, 64, device=DEV, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    loss = model.training_loss(x)
    loss.backward()
    assert torch.isfinite(loss).item() and len(launched) == 8
    assert all(p.grad is not None for p in model.parameters())
    torch.testing.assert_close(loss, twin.training_loss(x),
                               **edges._tol(BF16))
    assert len(launched) == 8
