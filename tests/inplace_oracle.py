"""Float64 oracle for the in-place activated BatchNorm backward.

The in-place layer stores only its output ``y = act(scale*x + shift)`` (in
the activation dtype) and the backward starts from it.  The functions here
evaluate that backward in float64, in textbook form, from the same stored,
dtype-rounded ``y``:

    z      = y > 0 ? y : y/slope          (slope None: identity, z = y)
    g      = y > 0 ? dy : slope*dy
    x-mean = (z - bias) / (weight*invstd)
    sum_dy = sum g,  sum_dy_xmu = sum g*(x-mean)
    grad_weight = sum_dy_xmu*invstd,  grad_bias = sum_dy
    dx = (g - sum_dy/n - (x-mean)*invstd^2*sum_dy_xmu/n) * invstd*weight

The gate is ``sign(y)`` here and in the kernels, and ``y`` is data, not a
computed quantity: no gate can flip between the two, so inputs of any size
need no margin search.

A plain module, not a conftest: ``import inplace_oracle``.
"""

import torch


def _chan(t, ndim):
    return t.reshape([1, -1] + [1] * (ndim - 2))


def _red_dims(x):
    return [d for d in range(x.dim()) if d != 1]


def backward(y, dy, weight, bias, invstd, count=None, slope=None,
             sum_dy=None, sum_dy_xmu=None):
    """-> dict(sum_dy, sum_dy_xmu, grad_weight, grad_bias, dx, g, z,
    abs_dy, abs_xmu, abs_recon), all float64.

    ``count`` defaults to the elements per channel of ``y``; ``sum_dy`` /
    ``sum_dy_xmu`` override the sums ``dx`` is formed with (several ranks:
    the sums of the whole batch, ``count`` its size).  The last three are
    sums of magnitudes a rounding bound scales with:
      abs_dy    = sum |g|
      abs_xmu   = sum |t|,  t = g*(z - bias)/scale the terms of sum_dy_xmu
      abs_recon = sum |g|*(|z| + |bias|)/|scale|
    """
    f64 = torch.float64
    nd = y.dim()
    y64, g = y.to(f64), dy.to(f64)
    z = y64
    if slope is not None:
        pos = y64 > 0
        g = torch.where(pos, g, slope * g)
        z = torch.where(pos, y64, y64 / slope)
    w, b, istd = weight.to(f64), bias.to(f64), invstd.to(f64)
    scale = w * istd
    dims = _red_dims(y)
    xmu = (z - _chan(b, nd)) / _chan(scale, nd)
    t = g * xmu
    out = {
        "g": g, "z": z,
        "sum_dy": g.sum(dims), "sum_dy_xmu": t.sum(dims),
        "abs_dy": g.abs().sum(dims), "abs_xmu": t.abs().sum(dims),
        "abs_recon": (g.abs() * (z.abs() + _chan(b, nd).abs())
                      / _chan(scale, nd).abs()).sum(dims),
    }
    out["grad_weight"] = out["sum_dy_xmu"] * istd
    out["grad_bias"] = out["sum_dy"]
    n = float(count) if count is not None else float(y.numel() // y.shape[1])
    s1 = out["sum_dy"] if sum_dy is None else sum_dy.to(f64)
    s2 = out["sum_dy_xmu"] if sum_dy_xmu is None else sum_dy_xmu.to(f64)
    out["dx"] = (g - _chan(s1, nd) / n
                 - xmu * _chan(istd * istd * s2, nd) / n) * _chan(scale, nd)
    return out
