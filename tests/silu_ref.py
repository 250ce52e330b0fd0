"""Inputs, fp64 reference and shared checks of the fused BN(+add)+SiLU tests.
The reference is the textbook formula in float64 on the ALREADY dtype-rounded
inputs; tolerances are those of tests/test_gpu_leaky_fused.py."""

import torch
import torch.nn.functional as F

from msbn import ops
from msbn.ops import _reference as ref

EPS = 1e-5
SUMS = {"atol": 1e-3, "rtol": 1e-3}  # sums, grad_weight, grad_bias


def tol(dtype, fp32_tol):
    t = fp32_tol if dtype == torch.float32 else 2e-2
    return {"atol": t, "rtol": t}


def close(got, want, **kw):
    torch.testing.assert_close(got.double().cpu(), want, **kw)


def draw(shape, dtype=torch.float32, gain=1.0):
    """x / res / dy rounded to ``dtype``, fp32 affine and running statistics;
    ``gain`` scales the weight (to push z out to where sigmoid saturates)."""
    g = torch.Generator().manual_seed(0)
    C = shape[1]
    x, res, dy = (torch.randn(shape, generator=g).to(dtype) for _ in "123")
    return {"x": x, "res": res, "dy": dy,
            "w": gain * (torch.randn(C, generator=g).abs() + 0.5),
            "b": torch.randn(C, generator=g),
            "rm": 0.5 * torch.randn(C, generator=g),
            "rv": torch.rand(C, generator=g) + 0.5}


def ops_ref(d, with_res, mean, invstd):
    """z, y = z*s, g = dy*s*(1 + z*(1 - s)) with s = sigmoid(z), and the
    BatchNorm backward algebra on g, for the statistics (mean, invstd)."""
    x, dy = d["x"].double(), d["dy"].double()
    cv = lambda t: t.double().reshape(1, -1, 1, 1)
    dims, n = [0, 2, 3], x.numel() // x.shape[1]
    m, istd = cv(mean), cv(invstd)
    scale = istd * cv(d["w"])
    z = (x - m) * scale + cv(d["b"]) + (d["res"].double() if with_res else 0)
    s = torch.sigmoid(z)
    g = dy * s * (1 + z * (1 - s))
    sdy, sdyx = g.sum(dims), (g * (x - m)).sum(dims)
    dx = (g - cv(sdy) / n - (x - m) * istd * istd * cv(sdyx) / n) * scale
    return dict(z=z, y=z * s, g=g, sum_dy=sdy, sum_dy_xmu=sdyx, n=n, dx=dx,
                gw=sdyx * invstd.double(), gb=sdy, frozen_dx=g * scale)


def check_ops(d, dtype, with_res, dev="cpu", cl=False, frozen=False):
    """The two-stage ops (or the frozen backward) with act="silu" on ``dev``
    against ops_ref; returns (y, gm, dx, z) of the two-stage ops."""
    fmt = torch.channels_last if cl else torch.contiguous_format
    x, dy, res = (d[k].to(dev).contiguous(memory_format=fmt)
                  for k in ("x", "dy", "res"))
    res = res if with_res else None
    w, b = d["w"].to(dev), d["b"].to(dev)
    if frozen:
        coefs = ref.bn_frozen_coefs(d["rm"], d["rv"], EPS, d["w"], d["b"])
        want = ops_ref(d, with_res, d["rm"], torch.rsqrt(d["rv"] + EPS))
        dx, dres = ops.batch_norm_frozen_backward_elemt(
            dy, x, res, coefs.to(dev), True, True, True, act="silu")
        close(dx, want["frozen_dx"], **tol(dtype, 1e-4))
        return close(dres, want["g"], **tol(dtype, 1e-5))
    mean, invstd = ref.batch_norm_stats(d["x"], EPS)
    want = ops_ref(d, with_res, mean, invstd)
    mean, invstd = mean.to(dev), invstd.to(dev)
    y = ops.batch_norm_elemt_act(x, res, w, b, mean, invstd, True,
                                 act="silu")
    close(y, want["y"], **tol(dtype, 1e-5))
    gm = torch.empty_like(dy)
    sums = ops.batch_norm_backward_reduce_act(
        dy, x, res, mean, invstd, w, b, True, True, True, True, None, gm,
        act="silu")
    for got, key in zip(sums, ("sum_dy", "sum_dy_xmu", "gw", "gb")):
        close(got, want[key], **SUMS)
    close(gm, want["g"], **tol(dtype, 1e-5))
    stats = (mean, invstd, w, b, sums[0], sums[1],
             torch.tensor([float(want["n"])], device=dev))
    dx, dres = ops.batch_norm_backward_elemt_act(dy, x, res, *stats, True,
                                                 True, act="silu")
    close(dx, want["dx"], **tol(dtype, 1e-4))
    # the residual gradient IS the reduce pass's gm (g rounded to T once),
    # and the derivative-free pass on gm gives dx (the gm route)
    assert torch.equal(dres, gm)
    dx_gm, _ = ops.batch_norm_backward_elemt_act(gm, x, None, *stats, False,
                                                 False)
    close(dx_gm, want["dx"], **tol(dtype, 1e-4))
    return y, gm, dx, want["z"]


def make_module(cls, d, training, dev="cpu"):
    m = cls(d["w"].numel(), eps=EPS, act="silu")
    with torch.no_grad():
        for name, key in (("weight", "w"), ("bias", "b"),
                          ("running_mean", "rm"), ("running_var", "rv")):
            getattr(m, name).copy_(d[key])
    return m.to(dev).train(training)


def check_module(m, d, dtype, with_res, dev="cpu", cl=False, fork=False):
    """``m`` against silu(bn(x) [+ res]) under fp64 autograd: output, input /
    residual / affine gradients, running statistics.  ``fork``: two consumers
    with gradients dy and 0.5*dy, which reach the layer as their sum in the
    activation dtype (one rounding)."""
    fmt = torch.channels_last if cl else torch.contiguous_format
    x, res = (d[k].clone().to(dev).contiguous(memory_format=fmt)
              .requires_grad_(True) for k in ("x", "res"))
    dy, args = d["dy"].to(dev), (x, res) if with_res else (x,)
    if fork:
        y, skip = m(*args, fork=True)
        torch.autograd.backward([y, skip], [dy, (0.5 * dy).to(dy.dtype)])
    else:
        y = m(*args)
        y.backward(dy)
    got = dict(y=y.detach(), dx=x.grad, rm=m.running_mean, rv=m.running_var)
    if m.weight.grad is not None:
        got.update(dw=m.weight.grad, db=m.bias.grad)
    if with_res:
        got["dres"] = res.grad
    x64, r64, w64, b64 = (d[k].double().requires_grad_(True)
                          for k in ("x", "res", "w", "b"))
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    z = F.batch_norm(x64, rm, rv, w64, b64, training=m.training,
                     momentum=0.1, eps=EPS)
    y64 = F.silu(z + r64 if with_res else z)
    dy = d["dy"] + (0.5 * d["dy"]).to(dtype) if fork else d["dy"]
    y64.backward(dy.double())
    want = dict(y=y64.detach(), dx=x64.grad, dres=r64.grad, dw=w64.grad,
                db=b64.grad, rm=rm, rv=rv)
    for k, v in got.items():
        fp32_tol = 1e-5 if k in ("y", "dres", "rm", "rv") else 1e-4
        kw = SUMS if k in ("dw", "db") else tol(dtype, fp32_tol)
        torch.testing.assert_close(v.double().cpu(), want[k], **kw,
                                   msg=lambda s, k=k: f"{k}: {s}")
