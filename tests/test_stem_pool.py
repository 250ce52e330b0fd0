"""Stem pool fusion: bn + act + MaxPool2d(3, 2, 1) as one layer.

CPU cases check the pure-torch references of the three ops (msbn/ops/
_reference.py: code convention, rounding points) against torch's own pool.
GPU cases check the fused kernels against the stock composition run on the
same GPU -- batch_norm_elemt_act, F.max_pool2d(return_indices=True), torch's
pool backward, batch_norm_backward_reduce_act, batch_norm_backward_elemt_act
-- and demand equal bits everywhere: the pooled output, the codes (decoded to
torch's indices), sum_dy, sum_dy_xmu, grad_weight, grad_bias and dx, with one
gradient and with the two gradients of a forked output (against the eager
add)."""

import pytest
import torch
import torch.nn.functional as F

import msbn.nn.fused as fused_mod
from msbn import ops
from msbn.models import resnet18
from msbn.ops import _reference as ref

gpu = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
F32, BF16 = torch.float32, torch.bfloat16

# (shape, V for bf16, V for fp32, what it exercises)
SHAPES = [
    ((2, 8, 7, 9), 8, 4),      # odd sizes, clipped windows on every border
    ((3, 16, 10, 12), 8, 4),   # even sizes, last row / column in one window
    ((2, 24, 9, 14), 8, 4),    # V = 8 with three packs
    ((2, 12, 6, 6), 4, 4),     # V = 4
    ((2, 5, 5, 5), 1, 1),      # scalar path
    ((1, 8, 1, 1), 8, 4),      # degenerate planes
    ((1, 8, 2, 3), 8, 4),
]
NAMES = ("sum_dy", "sum_dy_xmu", "grad_weight", "grad_bias")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _sid(shape):
    return "x".join(map(str, shape))


def _pooled_shape(shape):
    N, C, H, W = shape
    return (N, C, ref.pool_out_size(H), ref.pool_out_size(W))


def _make(shape, dtype, dev, grid=False):
    """x, w, b, mean, invstd, dy1, dy2 -- random, or (grid) x drawn from a
    five-value integer grid so that equal maxima are common."""
    g = torch.Generator(device="cpu").manual_seed(sum(shape) + 3)
    C = shape[1]
    if grid:
        x = torch.randint(-2, 3, shape, generator=g).float()
    else:
        x = torch.randn(shape, generator=g) * 2.0 + 0.5
    x = _cl(x.to(dtype)).to(dev)
    if grid:  # y = relu(x) exactly: scale 1, shift 0
        mean = torch.zeros(C, device=dev)
        invstd = torch.ones(C, device=dev)
        w = torch.ones(C, device=dev)
        b = torch.zeros(C, device=dev)
    else:
        mean, invstd = ref.batch_norm_stats(x.cpu(), EPS)
        mean, invstd = mean.to(dev), invstd.to(dev)
        w = (torch.randn(C, generator=g).abs() + 0.1).to(dev)
        b = torch.randn(C, generator=g).to(dev)
    ps = _pooled_shape(shape)
    dy1 = _cl(torch.randn(ps, generator=g).to(dtype)).to(dev)
    dy2 = _cl(torch.randn(ps, generator=g).to(dtype)).to(dev)
    return x, w, b, mean, invstd, dy1, dy2


def _stock(x, w, b, mean, invstd, act, slope, dy1, dy2):
    """The unfused composition through msbn.ops and torch's pool."""
    y = ops.batch_norm_elemt_act(x, None, w, b, mean, invstd, act, None,
                                 slope)
    pooled, idx = F.max_pool2d(y, 3, 2, 1, return_indices=True)
    dy = dy1 if dy2 is None else dy1 + dy2  # the eager add
    g_full = _cl(torch.ops.aten.max_pool2d_with_indices_backward(
        dy, y, [3, 3], [2, 2], [1, 1], [1, 1], False, idx))
    red = ops.batch_norm_backward_reduce_act(
        g_full, x, None, mean, invstd, w, b, act, True, True, True, None,
        None, slope)
    count = torch.tensor([x.numel() // x.shape[1]], dtype=torch.float32,
                         device=x.device)
    dx, _ = ops.batch_norm_backward_elemt_act(
        g_full, x, None, mean, invstd, w, b, red[0], red[1], count, act,
        False, None, slope)
    return pooled, idx, red, dx


def _fused(x, w, b, mean, invstd, act, slope, dy1, dy2):
    pooled, codes = ops.batch_norm_elemt_act_pool(x, w, b, mean, invstd, act,
                                                  None, slope)
    red = ops.batch_norm_backward_reduce_act_pool(
        dy1, dy2, codes, x, mean, invstd, w, b, act, True, True, True, None,
        slope)
    count = torch.tensor([x.numel() // x.shape[1]], dtype=torch.float32,
                         device=x.device)
    dx = ops.batch_norm_backward_elemt_act_pool(
        dy1, dy2, codes, x, mean, invstd, w, b, red[0], red[1], count, act,
        None, slope)
    return pooled, codes, red, dx


def _check_equal(x, w, b, mean, invstd, act, slope, dy1, dy2):
    H, W = x.shape[2:]
    for second in (None, dy2):
        p0, idx, red0, dx0 = _stock(x, w, b, mean, invstd, act, slope, dy1,
                                    second)
        p1, codes, red1, dx1 = _fused(x, w, b, mean, invstd, act, slope, dy1,
                                      second)
        tag = "two gradients" if second is not None else "one gradient"
        assert codes.dtype == torch.uint8 and codes.shape == p0.shape
        assert torch.equal(p1, p0), tag
        assert torch.equal(ref.pool_codes_to_indices(codes, H, W), idx), tag
        for name, a, e in zip(NAMES, red1, red0):
            assert torch.equal(a, e), (tag, name, (a - e).abs().max().item())
        assert torch.equal(dx1, dx0), (tag, "dx")


# ------------------------------------------------------------------ CPU cases
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("act,slope", [(True, 0.0), (True, 0.1), (False, 0.0)],
                         ids=["relu", "leaky", "none"])
@pytest.mark.parametrize("shape", [s for s, _, _ in SHAPES], ids=_sid)
def test_reference_matches_torch_pool(shape, act, slope, dtype):
    """The references' forward is torch's max_pool2d of the rounded y, their
    codes decode to its indices, and the gathered gradient is, in fp32 (one
    window per element contributes, or sums of up to four that fp32 holds
    exactly enough to round the same way), the pool backward's."""
    x, w, b, mean, invstd, dy1, dy2 = _make(shape, dtype, "cpu")
    H, W = shape[2:]
    y = ref.batch_norm_elemt_act(x, None, w, b, mean, invstd, act, slope)
    pooled, idx = F.max_pool2d(y.float(), 3, 2, 1, return_indices=True)
    got, codes = ops.batch_norm_elemt_act_pool(x, w, b, mean, invstd, act,
                                               None, slope)
    assert got.dtype == dtype and codes.dtype == torch.uint8
    assert torch.equal(got.float(), pooled)
    assert torch.equal(ref.pool_codes_to_indices(codes, H, W), idx)
    assert int(codes.max()) <= 8
    for second in (None, dy2):
        dy = dy1 if second is None else dy1 + second
        want = torch.ops.aten.max_pool2d_with_indices_backward(
            dy.float(), y.float(), [3, 3], [2, 2], [1, 1], [1, 1], False,
            idx).to(dtype)
        g = ref.pool_gather_grad(dy1, second, codes, x)
        assert g.dtype == dtype and g.shape == x.shape
        # torch's CPU backward adds in ascending (oh, ow) order too
        assert torch.equal(g, want)
        red = ops.batch_norm_backward_reduce_act_pool(
            dy1, second, codes, x, mean, invstd, w, b, act, True, True, True,
            None, slope)
        want_red = ref.batch_norm_backward_reduce_act(
            g, x, None, mean, invstd, w, b, act, True, True, True, None,
            slope)
        for a, e in zip(red, want_red):
            assert torch.equal(a, e)
        count = torch.tensor([x.numel() // shape[1]], dtype=torch.float32)
        dx = ops.batch_norm_backward_elemt_act_pool(
            dy1, second, codes, x, mean, invstd, w, b, red[0], red[1], count,
            act, None, slope)
        want_dx, _ = ref.batch_norm_backward_elemt_act(
            g, x, None, mean, invstd, w, b, red[0], red[1], count, act,
            False, slope)
        assert torch.equal(dx, want_dx)


def _tie_fraction(x):
    """Share of windows whose positive maximum is reached more than once."""
    y = torch.relu(x.float())
    N, C, H, W = y.shape
    yp = F.pad(y, (1, 1, 1, 1), value=float("-inf"))
    win = F.unfold(yp.reshape(N * C, 1, H + 2, W + 2), 3, stride=2)
    mx = win.max(dim=1, keepdim=True).values
    tied = ((win == mx).sum(dim=1) > 1) & (mx.squeeze(1) > 0)
    return tied.float().mean().item()


TIE_SHAPE = (2, 16, 11, 13)


def test_tie_input_has_ties_and_first_maximum_wins():
    x, w, b, mean, invstd, dy1, dy2 = _make(TIE_SHAPE, F32, "cpu", grid=True)
    assert _tie_fraction(x) >= 0.10
    y = ref.batch_norm_elemt_act(x, None, w, b, mean, invstd, True, 0.0)
    assert torch.equal(y, torch.relu(x))
    pooled, idx = F.max_pool2d(y, 3, 2, 1, return_indices=True)
    got, codes = ops.batch_norm_elemt_act_pool(x, w, b, mean, invstd, True)
    assert torch.equal(got, pooled)
    assert torch.equal(ref.pool_codes_to_indices(codes, 11, 13), idx)


def test_cpu_and_eval_models_take_the_composed_route(monkeypatch):
    calls = []
    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act_pool",
                        lambda *a, **kw: calls.append(1))
    torch.manual_seed(3)
    m = resnet18(num_classes=10, fused=True)
    x = torch.randn(2, 3, 32, 32)
    for train in (True, False):
        m.train(train)
        a = m._stem(x)
        m.stem_pool = False
        bb = m._stem(x)
        m.stem_pool = True
        # a forking model hands layer1 a (main, skip) pair: one tensor twice
        assert isinstance(a, tuple) and a[0] is a[1]
        # training mode updates the running stats between the two calls; the
        # batch statistics, and so the output, do not depend on them
        assert torch.equal(a[0], bb)
        loss = m(x).sum()
        if train:
            loss.backward()
    assert not calls


def test_state_dict_keys_unchanged():
    fused = resnet18(num_classes=10, fused=True)
    plain = resnet18(num_classes=10, fused=False)
    assert list(fused.state_dict()) == list(plain.state_dict())
    assert fused.stem_pool and not plain.stem_pool
    assert isinstance(fused.maxpool, torch.nn.MaxPool2d)


def test_eligibility_falls_back():
    bn = fused_mod.SyncBatchNormAct2d(8)
    x = _cl(torch.randn(2, 8, 6, 6))
    ok = torch.nn.MaxPool2d(3, 2, 1)
    assert not fused_mod.stem_pool_eligible(bn, ok, x)  # CPU tensor
    y = fused_mod.bn_act_maxpool(bn, ok, x, fork=True)
    assert isinstance(y, tuple) and y[0] is y[1]


# ------------------------------------------------------------------ GPU cases
@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("act,slope", [(True, 0.0), (True, 0.1), (False, 0.0)],
                         ids=["relu", "leaky", "none"])
@pytest.mark.parametrize("case", SHAPES, ids=[_sid(s) for s, _, _ in SHAPES])
def test_fused_equals_stock_composition(case, act, slope, dtype):
    shape, v16, v32 = case
    x, w, b, mean, invstd, dy1, dy2 = _make(shape, dtype, DEV)
    codes = torch.empty(_pooled_shape(shape), dtype=torch.uint8, device=DEV)
    codes = _cl(codes)
    coefs = ops.bn_make_coefs(mean, invstd, w, b)
    want_v = v16 if dtype == BF16 else v32
    for kind, others in (("elemt_pool", (dy1, codes)),
                         ("bwd_reduce_pool", (dy1, dy2, codes)),
                         ("bwd_elemt_pool", (dy1, dy2, codes))):
        plan = ops.launch_plan(kind, x, others, coefs)
        assert plan["path"] == "nhwc" and plan["V"] == want_v, (kind, plan)
    _check_equal(x, w, b, mean, invstd, act, slope, dy1, dy2)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_tied_maxima(dtype):
    x, w, b, mean, invstd, dy1, dy2 = _make(TIE_SHAPE, dtype, DEV, grid=True)
    assert _tie_fraction(x.cpu()) >= 0.10
    _check_equal(x, w, b, mean, invstd, True, 0.0, dy1, dy2)


@gpu
def test_reduce_runs_many_chunks_past_the_flush_period():
    shape = (4, 3, 1030, 1030)
    x, w, b, mean, invstd, dy1, dy2 = _make(shape, BF16, DEV)
    codes = _cl(torch.empty(_pooled_shape(shape), dtype=torch.uint8,
                            device=DEV))
    plan = ops.launch_plan("bwd_reduce_pool", x, (dy1, dy2, codes))
    stock = ops.launch_plan("bwd_reduce", x, (x,))
    assert plan == stock, (plan, stock)
    assert plan["path"] == "nhwc" and plan["nchunks"] > 1, plan
    assert plan["trips"] > plan["flush_every"], plan
    _check_equal(x, w, b, mean, invstd, True, 0.0, dy1, dy2)


@gpu
def test_elemt_grid_takes_a_second_trip():
    shape = (2, 16, 520, 520)
    x, w, b, mean, invstd, dy1, dy2 = _make(shape, BF16, DEV)
    codes = _cl(torch.empty(_pooled_shape(shape), dtype=torch.uint8,
                            device=DEV))
    coefs = ops.bn_make_coefs(mean, invstd, w, b)
    plan = ops.launch_plan("bwd_elemt_pool", x, (dy1, dy2, codes), coefs)
    stock = ops.launch_plan("bwd_elemt", x, (x,), coefs)
    assert plan == stock, (plan, stock)
    assert plan["V"] == 8 and plan["multi_trip"] and plan["trips"] == 2, plan
    _check_equal(x, w, b, mean, invstd, True, 0.0, dy1, dy2)


# ---------------------------------------------------------------- module level
def _model(dtype, stem_pool):
    torch.manual_seed(7)
    m = resnet18(num_classes=10, fused=True).to(DEV)
    if dtype == BF16:  # bf16 convs, fp32 BatchNorm parameters and statistics
        m.to(BF16)
        for mod in m.modules():
            if hasattr(mod, "running_mean"):
                mod.float()
    m.stem_pool = stem_pool
    return m.to(memory_format=torch.channels_last).train()


def _step(m, x, y):
    xg = x.clone().requires_grad_(True)
    loss = F.cross_entropy(m(xg).float(), y)
    loss.backward()
    return loss.detach(), xg.grad


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bfloat16", "float32"])
def test_resnet18_fused_stem_matches_composed(dtype, monkeypatch):
    """Loss, every BN affine gradient and the input-image gradient are
    bit-equal between the fused and the composed stem (deterministic MIOpen
    solvers, as in test_gpu_grad_fork.py)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    used = []
    real = ops.batch_norm_elemt_act_pool

    def counting(*a, **kw):
        used.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(fused_mod.ops, "batch_norm_elemt_act_pool", counting)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = _cl(torch.randn(4, 3, 64, 64, generator=g, device=DEV).to(dtype))
    y = torch.randint(0, 10, (4,), generator=g, device=DEV)
    fused, composed = _model(dtype, True), _model(dtype, False)
    assert list(fused.state_dict()) == list(composed.state_dict())
    loss_a, dx_a = _step(fused, x, y)
    assert len(used) == 1
    loss_b, dx_b = _step(composed, x, y)
    assert len(used) == 1
    assert torch.equal(loss_a, loss_b)
    assert torch.equal(dx_a, dx_b)
    n_bn = 0
    for (n, p), (_, q) in zip(fused.named_parameters(),
                              composed.named_parameters()):
        if p.dim() == 1 and "bn" in n or "downsample.1" in n:
            assert torch.equal(p.grad, q.grad), n
            n_bn += 1
    assert n_bn == 2 * 20
    for k, v in fused.state_dict().items():
        if "running" in k:
            assert torch.equal(v, composed.state_dict()[k]), k

    # eval mode takes the composed route and agrees with it
    fused.eval(), composed.eval()
    with torch.no_grad():
        assert torch.equal(fused(x), composed(x))
    assert len(used) == 1


@gpu
def test_fused_stem_holds_less_memory():
    """After a forward of the stem alone, with the graph alive, the fused
    stem holds one stem activation and its int64 indices less, and a one-byte
    code tensor more."""
    N, C, H = 16, 64, 32                  # conv1 output of a 16x3x64x64 batch
    A = N * C * H * H * 2                 # one stem activation, bf16
    pooled = N * C * (H // 2) ** 2
    x = _cl(torch.randn(N, 3, 64, 64, device=DEV).to(BF16))
    held = {}
    for stem_pool in (False, True):
        m = _model(BF16, stem_pool)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = m._stem(x)
        torch.cuda.synchronize()
        held[stem_pool] = torch.cuda.memory_allocated() - before
        del out, m
    print(f"held after the stem forward: composed {held[False]} B, fused "
          f"{held[True]} B, saved {held[False] - held[True]} B")
    # per-channel buffers round to 512 B each: 64 KiB of slack
    assert held[False] - held[True] >= A + pooled * 8 - pooled - 64 * 1024, \
        held
