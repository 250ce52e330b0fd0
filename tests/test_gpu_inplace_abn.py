"""GPU numerics of the in-place activated BatchNorm kernels: the alias-safe
forward, the backward reduce from y and the backward elementwise from y,
against ``inplace_oracle`` (float64, textbook form, from the same stored
dtype-rounded y), through every path of the family: NCHW vectorised, NCHW
flat, NHWC; finalize with more than 64 chunks, loops past the flush period,
grid-stride second trips, a reduced vector width on a misaligned view; then
the autograd function GPU against CPU and the memory the feature is for.

The gate is sign(y) in the kernels and in the oracle, and y is data: no gate
can flip between the two, whatever the size.

Bound of the reductions (u = 2^-24), derived, not tuned:

* sum_dy.  Each fp32 partial holds at most MSBN_ACC_FLUSH = 64 terms before
  it is flushed to fp64: 63u * sum|g|.  A term g = slope*dy carries the
  rounding of the slope to fp32 and of the product, the fp32 result one
  more: 66u, held to the family's 68u * sum|g| (RED_K).
* sum_dy_xmu, terms t = g * ((z - bias) * (1/scale)).  Summation as above:
  63u * sum|t|; g brings its two roundings, the product g*(...) one, the
  fp32 result one: 67u <= 68u * sum|t|.  What is new is the reconstruction
  of x - mean, whose error scales with |g|*(|z| + |bias|)/|scale|, not with
  |t| (z and bias may cancel):
      1/slope           2   (the slope to fp32, the division)
      y * (1/slope)     1
      z - bias          1   (u*|z - bias| <= u*(|z| + |bias|))
      1/scale           2   (the product invstd*weight, the reciprocal)
      (z - bias)*(1/scale)  1
  k = 7:  RECON_K = 7u * sum |g|*(|z| + |bias|)/|scale|.
  The identity activation has fewer roundings and keeps the same bound.
* grad_weight = sum_dy_xmu*invstd adds 2u*|grad_weight| (the product, the
  cast), as in test_gpu_reduction_edges.

The oracle is given the fp32 invstd the kernels are given, so the
statistics' own error does not enter.  The fp32 reference ops are held to
the same bound on the CPU (test_reference_inside_the_reduction_bound).
"""

import functools

import pytest
import torch
import torch.nn as nn

import inplace_oracle as ipo
from leaky_inputs import EPS, gated_inputs
from msbn import ops
from msbn.nn.fused import (InPlaceSyncBatchNormActFunction,
                           SyncBatchNormAct2d)

gpu = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
RED_K = 68 * U
RECON_K = 7 * U
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

OP_SHAPES = [(4, 32, 9, 9), (2, 24, 8, 8), (3, 20, 7, 7)]
# (act, slope)
ACTS = [(True, 0.2), (True, 0.01), (False, 0.0)]
ACT_IDS = ["leaky0.2", "leaky0.01", "identity"]
OP_CASES = [(s, d) for s in OP_SHAPES for d in (F32, BF16)] \
    + [((2, 24, 8, 8), F16)]
SUMS = {"atol": 1e-3, "rtol": 1e-3}


def _elt(dtype):
    t = 1e-4 if dtype == F32 else 2e-2
    return {"atol": t, "rtol": t}


def _cl(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) \
        if channels_last else t.contiguous()


def _slope(act, slope):
    return slope if act else None


def _within(name, got, want, bound):
    """|got - want| <= bound elementwise; prints the figures first."""
    err = (got.double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64,
                            device=err.device).expand_as(err)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300),
                        torch.zeros_like(err))
    print(f"{name}: max|err| {err.max().item():.3e}  "
          f"max err/bound {ratio.max().item():.3e}")
    bad = err > bound
    assert not bad.any().item(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; worst "
        f"err/bound {ratio.max().item():.3e}")


def _check_sums(tag, got, want, invstd):
    sum_dy, sum_dy_xmu, gw, gb = got
    xmu_bound = RED_K * want["abs_xmu"] + RECON_K * want["abs_recon"]
    _within(tag + " sum_dy", sum_dy, want["sum_dy"], RED_K * want["abs_dy"])
    _within(tag + " sum_dy_xmu", sum_dy_xmu, want["sum_dy_xmu"], xmu_bound)
    _within(tag + " grad_bias", gb, want["grad_bias"],
            RED_K * want["abs_dy"])
    _within(tag + " grad_weight", gw, want["grad_weight"],
            xmu_bound * invstd.double() + 2 * U * want["grad_weight"].abs())


def _forward(x, w, b, act, slope):
    """(y in place over a copy of x, out-of-place y, mean, invstd)"""
    mean, invstd = ops.batch_norm_stats(x, EPS)
    ref = ops.batch_norm_elemt_act(x, None, w, b, mean, invstd, act, None,
                                   slope)
    xy = x.clone(memory_format=torch.preserve_format)
    y = ops.batch_norm_elemt_act_(xy, w, b, mean, invstd, act, None, slope)
    assert y.data_ptr() == xy.data_ptr()
    return y, ref, mean, invstd


# =================================================================
# the three ops on the small shapes
# =================================================================
@gpu
@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("channels_last", [False, True],
                         ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape,dtype", OP_CASES,
                         ids=[f"{'x'.join(map(str, s))}-{str(d)[6:]}"
                              for s, d in OP_CASES])
def test_inplace_ops_vs_oracle(shape, dtype, channels_last, act, slope):
    d = gated_inputs(shape, dtype, running=False)
    cl = channels_last
    x, dy = _cl(d["x"].to(DEV), cl), _cl(d["dy"].to(DEV), cl)
    w, b = d["w"].to(DEV), d["b"].to(DEV)
    n = x.numel() // shape[1]
    y, ref, mean, invstd = _forward(x, w, b, act, slope)
    assert torch.equal(y, ref)
    # with the caller's coefs too
    coefs = ops.bn_make_coefs(mean, invstd, w, b)
    xy = x.clone(memory_format=torch.preserve_format)
    assert torch.equal(ops.batch_norm_elemt_act_(xy, w, b, mean, invstd, act,
                                                 coefs, slope), ref)

    want = ipo.backward(y, dy, w, b, invstd, n, _slope(act, slope))
    got = ops.batch_norm_backward_reduce_inplace(
        dy, y, invstd, w, b, act, True, True, True, coefs, slope)
    assert got[0].data_ptr() + 4 * shape[1] == got[1].data_ptr()
    for k, g_ in zip(("sum_dy", "sum_dy_xmu", "grad_weight", "grad_bias"),
                     got):
        torch.testing.assert_close(g_.double(), want[k], **SUMS,
                                   msg=lambda m, k=k: f"{k}: {m}")
    dx = ops.batch_norm_backward_elemt_inplace(
        dy, y, mean, invstd, w, b, want["sum_dy"].float(),
        want["sum_dy_xmu"].float(), torch.full((1,), float(n), device=DEV),
        act, coefs, slope)
    assert dx.dtype == dtype and dx.stride() == x.stride()
    torch.testing.assert_close(dx.double(), want["dx"], **_elt(dtype))


@gpu
def test_inplace_ops_reject_plain_relu_and_keep_zero_scale_finite():
    x = torch.randn(2, 8, 4, 4, device=DEV)
    one, zero = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="invertible"):
        ops.batch_norm_elemt_act_(x.clone(), one, zero, zero, one, True,
                                  None, 0.0)
    with pytest.raises(RuntimeError, match="invertible"):
        ops.batch_norm_backward_reduce_inplace(
            x, x, one, one, zero, True, True, True, True, None, 0.0)
    with pytest.raises(RuntimeError, match="invertible"):
        ops.batch_norm_backward_elemt_inplace(
            x, x, zero, one, one, zero, zero, zero,
            torch.full((1,), 32.0, device=DEV), True, None, 0.0)
    # weight 0 in a channel: 1/scale := 0, everything stays finite
    w = one.clone()
    w[3] = 0.0
    got = ops.batch_norm_backward_reduce_inplace(
        x, x, one, w, zero, True, True, True, True, None, 0.2)
    assert all(torch.isfinite(t).all().item() for t in got)
    assert got[1][3].item() == 0.0
    dx = ops.batch_norm_backward_elemt_inplace(
        x, x, zero, one, w, zero, got[0], got[1],
        torch.full((1,), 32.0, device=DEV), True, None, 0.2)
    assert torch.isfinite(dx).all().item()


# =================================================================
# reduction edges: the shape lists of test_gpu_reduction_edges.py
# =================================================================
# (kind, path, shape, dtype, channels_last)
REDUCTION_CASES = [
    ("finalize", "nchw_vec", (100, 4, 4, 4), F32, False),
    ("finalize", "nchw_flat", (70, 2, 31, 31), F32, False),
    ("finalize", "nhwc", (3, 8, 53, 53), F32, True),
    ("finalize", "nhwc", (2, 2048, 42, 50), BF16, True),
    ("loop", "nchw_vec", (1030, 256, 2, 2), F32, False),
    ("loop", "nchw_flat", (130, 2048, 1, 127), F32, False),
    ("loop", "nhwc", (4, 3, 1030, 1030), BF16, True),
]
# the ones a CPU test can afford
SMALL_REDUCTION_CASES = [c for c in REDUCTION_CASES
                         if c[2][0] * c[2][1] * c[2][2] * c[2][3] < 2 ** 21]


def _red_id(c):
    return f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}-{str(c[3])[6:]}"


def _assert_property(plan, kind, path):
    assert plan["path"] == path, plan
    if kind == "finalize":
        assert plan["nchunks"] > 64 and plan["nchunks"] % 64 != 0, plan
    else:
        assert plan["trips"] > plan["flush_every"], plan


def _edge_data(shape, dtype, cl, device):
    """The suite's usual data (randn*2 + 0.5), drawn on the CPU."""
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[1]
    x = _cl((torch.randn(shape, generator=g) * 2 + 0.5).to(dtype), cl)
    dy = _cl(torch.randn(shape, generator=g).to(dtype), cl)
    w = torch.randn(C, generator=g).abs() + 0.1
    b = torch.randn(C, generator=g)
    return tuple(t.to(device) for t in (x, dy, w, b))


@pytest.mark.parametrize("case", REDUCTION_CASES, ids=_red_id)
def test_reduction_plans_are_host_only(case):
    kind, path, shape, dtype, cl = case
    y = _cl(torch.empty(shape, dtype=dtype), cl)
    _assert_property(ops.launch_plan("bwd_reduce_inplace", y, (y,)), kind,
                     path)
    # same host code, same numbers as the out-of-place reduce
    assert ops.launch_plan("bwd_reduce_inplace", y, (y,)) == \
        ops.launch_plan("bwd_reduce", y, (y,))


@pytest.mark.parametrize("act,slope", [(True, 0.2), (False, 0.0)],
                         ids=["leaky0.2", "identity"])
@pytest.mark.parametrize("case", SMALL_REDUCTION_CASES, ids=_red_id)
def test_reference_inside_the_reduction_bound(case, act, slope):
    """The fp32 reference ops meet the derived bound on the CPU: its
    reconstruction term is reachable by plain fp32 arithmetic."""
    kind, path, shape, dtype, cl = case
    x, dy, w, b = _edge_data(shape, dtype, cl, "cpu")
    mean, invstd = ops.batch_norm_stats(x, EPS)
    y = ops.batch_norm_elemt_act_(x.clone(), w, b, mean, invstd, act, None,
                                  slope)
    want = ipo.backward(y, dy, w, b, invstd, slope=_slope(act, slope))
    got = ops.batch_norm_backward_reduce_inplace(
        dy, y, invstd, w, b, act, True, True, True, None, slope)
    _check_sums(f"ref {_red_id(case)}", got, want, invstd)


@gpu
@pytest.mark.parametrize("act,slope", [(True, 0.2), (False, 0.0)],
                         ids=["leaky0.2", "identity"])
@pytest.mark.parametrize("case", REDUCTION_CASES, ids=_red_id)
def test_inplace_reduction_edges(case, act, slope):
    kind, path, shape, dtype, cl = case
    x, dy, w, b = _edge_data(shape, dtype, cl, DEV)
    y, ref, mean, invstd = _forward(x, w, b, act, slope)
    del x
    assert torch.equal(y, ref)
    del ref
    _assert_property(ops.launch_plan("bwd_reduce_inplace", y, (dy,)), kind,
                     path)
    want = ipo.backward(y, dy, w, b, invstd, slope=_slope(act, slope))
    got = ops.batch_norm_backward_reduce_inplace(
        dy, y, invstd, w, b, act, True, True, True, None, slope)
    _check_sums(f"gpu {_red_id(case)}", got, want, invstd)


# =================================================================
# grid-stride loops of the two elementwise kernels
# =================================================================
GRID_CASES = [
    ((3, 37, 97, 99), F32, False),
    ((3, 37, 97, 99), F32, True),
    ((1, 8, 4, 262152), BF16, True),
]


@gpu
@pytest.mark.parametrize("act,slope", [(True, 0.2), (False, 0.0)],
                         ids=["leaky0.2", "identity"])
@pytest.mark.parametrize(
    "shape,dtype,cl", GRID_CASES,
    ids=[f"{'x'.join(map(str, s))}-{str(d)[6:]}-{'nhwc' if c else 'nchw'}"
         for s, d, c in GRID_CASES])
def test_inplace_grid_stride(shape, dtype, cl, act, slope):
    x, dy, w, b = _edge_data(shape, dtype, cl, DEV)
    n = x.numel() // shape[1]
    for kind, others in (("elemt_inplace", ()),
                         ("bwd_elemt_inplace", (dy,))):
        plan = ops.launch_plan(kind, x, others)
        assert plan["multi_trip"] and plan["trips"] >= 2, (kind, plan)
    y, ref, mean, invstd = _forward(x, w, b, act, slope)
    assert torch.equal(y, ref)
    want = ipo.backward(y, dy, w, b, invstd, n, _slope(act, slope))
    dx = ops.batch_norm_backward_elemt_inplace(
        dy, y, mean, invstd, w, b, want["sum_dy"].float(),
        want["sum_dy_xmu"].float(), torch.full((1,), float(n), device=DEV),
        act, None, slope)
    torch.testing.assert_close(dx.double(), want["dx"], **_elt(dtype))


# =================================================================
# a misaligned view: the vector width drops, the neighbours stay
# =================================================================
MIS_SHAPE = (4, 8, 4, 16)


def _odd_view(t, cl, fill):
    """A copy of t one ELEMENT past an aligned allocation filled with
    ``fill``; returns (view, whole buffer)."""
    buf = torch.full((t.numel() + 64,), fill, dtype=t.dtype, device=t.device)
    flat = buf[1:1 + t.numel()]
    if cl:
        N, C, H, W = t.shape
        v = flat.view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        v = flat.view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + t.element_size()
    return v, buf


@gpu
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_inplace_misaligned_view(dtype, cl):
    vmax = 16 // torch.empty((), dtype=dtype).element_size()
    d = gated_inputs(MIS_SHAPE, dtype, running=False)
    x, dy = _cl(d["x"].to(DEV), cl), _cl(d["dy"].to(DEV), cl)
    w, b = d["w"].to(DEV), d["b"].to(DEV)
    n = x.numel() // MIS_SHAPE[1]
    y_al, ref, mean, invstd = _forward(x, w, b, True, 0.2)
    assert ops.launch_plan("elemt_inplace", x)["V"] == vmax

    xv, buf = _odd_view(x, cl, 7.0)
    assert ops.launch_plan("elemt_inplace", xv)["V"] == 1
    yv = ops.batch_norm_elemt_act_(xv, w, b, mean, invstd, True, None, 0.2)
    assert yv.data_ptr() == xv.data_ptr() and torch.equal(yv, ref)
    assert (buf[0] == 7.0).item() and (buf[1 + x.numel():] == 7.0).all()

    for kind in ("bwd_reduce_inplace", "bwd_elemt_inplace"):
        assert ops.launch_plan(kind, y_al, (dy,))["V"] == vmax
        assert ops.launch_plan(kind, yv, (dy,))["V"] == 1
    want = ipo.backward(yv, dy, w, b, invstd, n, 0.2)
    got = ops.batch_norm_backward_reduce_inplace(
        dy, yv, invstd, w, b, True, True, True, True, None, 0.2)
    _check_sums("misaligned", got, want, invstd)
    dyv, dybuf = _odd_view(dy, cl, 7.0)
    dx = ops.batch_norm_backward_elemt_inplace(
        dyv, yv, mean, invstd, w, b, want["sum_dy"].float(),
        want["sum_dy_xmu"].float(), torch.full((1,), float(n), device=DEV),
        True, None, 0.2)
    torch.testing.assert_close(dx.double(), want["dx"], **_elt(dtype))
    # the reads left the buffers as they were
    assert torch.equal(yv, ref)
    assert (buf[0] == 7.0).item() and (buf[1 + x.numel():] == 7.0).all()
    assert (dybuf[0] == 7.0).item() and (dybuf[1 + x.numel():] == 7.0).all()


# =================================================================
# the autograd function, GPU against CPU
# =================================================================
FN_SHAPE = (4, 64, 8, 8)   # NCHW: eligible for the small-plane kernels


def _run_function(d, dev, dtype, channels_last):
    C = d["x"].shape[1]

    def leaf(t):
        return t.detach().clone().to(dev).requires_grad_(True)

    x = leaf(d["x"].to(dtype))
    xin = _cl(x * 1.0, channels_last)
    w, b = leaf(d["w"]), leaf(d["b"])
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = InPlaceSyncBatchNormActFunction.apply(
        xin, w, b, rm, rv, EPS, 0.1, None, 1, True, 0.2)
    assert y.data_ptr() == xin.data_ptr()
    yv = y.detach().clone()
    y.backward(_cl(d["dy"].to(dtype).to(dev), channels_last))
    return dict(y=yv, dx=x.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)


@functools.lru_cache(maxsize=None)
def _function_case(dtype):
    d = gated_inputs(FN_SHAPE, dtype, running=False)
    want = _run_function(d, "cpu", dtype, False)
    return d, {k: v.float() for k, v in want.items()}


@gpu
@pytest.mark.parametrize("channels_last", [False, True],
                         ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_inplace_function_gpu_vs_cpu(dtype, channels_last, monkeypatch):
    """fp32: y 1e-5, dx 1e-4, sums 1e-3 against the CPU function.  bf16: y
    and dx 2e-2, grad_bias 1e-3; grad_weight is a function of the stored
    bf16 y, which the two devices may round differently in the last bit, so
    it is held to the oracle of the GPU's own y (1e-3)."""
    d, want = _function_case(dtype)
    x = _cl(d["x"].to(dtype).to(DEV), channels_last)
    stat = torch.zeros(FN_SHAPE[1], device=DEV)
    assert ops.bn_fused_local_eligible(
        x, d["w"].to(DEV), d["b"].to(DEV), stat, stat) == (not channels_last)
    assert ops.launch_plan("elemt_inplace", x)["path"] != "small_plane"

    def no_small_plane(*a, **k):
        raise AssertionError("the in-place function took the small-plane "
                             "kernels")

    monkeypatch.setattr(ops, "batch_norm_fwd_fused_local", no_small_plane)
    monkeypatch.setattr(ops, "batch_norm_bwd_fused_local", no_small_plane)
    got = _run_function(d, DEV, dtype, channels_last)
    tol = {"y": 1e-5, "dx": 1e-4, "dw": 1e-3, "db": 1e-3, "rm": 1e-5,
           "rv": 1e-5}
    if dtype != F32:
        tol.update(y=2e-2, dx=2e-2)
    for k in want:
        if k == "dw" and dtype != F32:
            _, invstd = ops.batch_norm_stats(x, EPS)
            ref = ipo.backward(got["y"], d["dy"].to(dtype).to(DEV),
                               d["w"].to(DEV), d["b"].to(DEV), invstd,
                               slope=0.2)["grad_weight"]
            torch.testing.assert_close(got[k].double(), ref, atol=1e-3,
                                       rtol=1e-3)
            continue
        torch.testing.assert_close(got[k].float().cpu(), want[k],
                                   atol=tol[k], rtol=tol[k],
                                   msg=lambda m, k=k: f"{k}: {m}")


# =================================================================
# what the feature is for: one activation tensor less per layer
# =================================================================
def _blocks(inplace, K=3):
    torch.manual_seed(5)
    layers = []
    for _ in range(K):
        layers += [nn.Conv2d(16, 16, 1, bias=False),
                   SyncBatchNormAct2d(16, negative_slope=0.2,
                                      inplace=inplace)]
    return nn.Sequential(*layers).to(DEV).train()


@gpu
def test_inplace_saves_one_activation_per_layer():
    K, A = 3, 8 * 16 * 64 * 64 * 4
    assert A == 2 * 2 ** 20
    x = torch.randn(8, 16, 64, 64, device=DEV)
    held, grads = {}, {}
    for inplace in (False, True):
        net = _blocks(inplace, K)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = net(x)
        torch.cuda.synchronize()
        held[inplace] = torch.cuda.memory_allocated() - before
        y.square().mean().backward()
        grads[inplace] = [p.grad.clone() for p in net.parameters()]
        del y, net
    print(f"held after forward: out of place {held[False]} B, in place "
          f"{held[True]} B, saved {held[False] - held[True]} B")
    # the per-channel buffers round to 512 B each: 64 KiB of slack
    assert held[False] - held[True] >= K * A - 64 * 1024, held
    for a, b in zip(grads[False], grads[True]):
        torch.testing.assert_close(a, b, atol=1e-3, rtol=1e-3)
