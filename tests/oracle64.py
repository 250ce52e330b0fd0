"""Float64 oracle for the BatchNorm op set, in the textbook form.

``msbn/ops/_reference.py`` is the CPU execution path and mirrors the kernels'
fp32 ``x*scale + shift`` arithmetic, so it shares their rounding.  The
functions here do not: everything is evaluated as ``(x - mean)*invstd*w + b``
in float64 (``dtype=`` exists only so a test can compare the float32
evaluation against the float64 one).  They are plain torch ops and run on
whatever device their inputs are on; per-channel arguments are ``[C]``
tensors, ``None`` weight / bias mean 1 / 0.

A plain module, not a conftest: import it as ``import oracle64``.
"""

import torch


def chan(t, ndim):
    """[C] -> broadcastable against an N,C,* tensor of ``ndim`` dims."""
    return t.reshape([1, -1] + [1] * (ndim - 2))


def _red_dims(x):
    return [d for d in range(x.dim()) if d != 1]


def _cast(t, dtype):
    return None if t is None else t.to(dtype)


def stats(x, eps, dtype=torch.float64):
    """Per-channel (mean, biased var, invstd) by the corrected two-pass
    algorithm (Chan, Golub & LeVeque): centre on a first mean m0, then
    mean = m0 + E[x-m0], var = E[(x-m0)^2] - E[x-m0]^2.  The correction terms
    vanish in exact arithmetic and absorb the rounding of m0 otherwise."""
    x = x.to(dtype)
    dims = _red_dims(x)
    m0 = x.mean(dims)
    d = x - chan(m0, x.dim())
    dm = d.mean(dims)
    var = ((d * d).mean(dims) - dm * dm).clamp_min(0)
    return m0 + dm, var, torch.rsqrt(var + eps)


def running_update(running_mean, running_var, mean, var, count, momentum,
                   dtype=torch.float64):
    """(new running_mean, new running_var); the variance is unbiased."""
    unbiased = var.to(dtype) * (count / (count - 1.0)) if count > 1 else var
    return ((1.0 - momentum) * running_mean.to(dtype) + momentum * mean.to(dtype),
            (1.0 - momentum) * running_var.to(dtype) + momentum * unbiased)


def gather(means, variances, counts, eps, dtype=torch.float64):
    """Combine per-rank (mean[C], biased var[C], count) -> the statistics of
    the union, by the pairwise-exact identity
    var = sum n_r (var_r + (mean_r - mean)^2) / n."""
    n = float(sum(counts))
    mean = sum(c * m.to(dtype) for m, c in zip(means, counts)) / n
    var = sum(c * (v.to(dtype) + (m.to(dtype) - mean) ** 2)
              for m, v, c in zip(means, variances, counts)) / n
    return mean, var, torch.rsqrt(var + eps)


def coefs(mean, invstd, weight, bias, dtype=torch.float64):
    """(scale, shift) of the fused-multiply form, from the textbook terms."""
    scale = invstd.to(dtype) * (1.0 if weight is None else weight.to(dtype))
    shift = -mean.to(dtype) * scale + (0.0 if bias is None else bias.to(dtype))
    return scale, shift


def pre_activation(x, mean, invstd, weight, bias, residual=None,
                   dtype=torch.float64):
    x = x.to(dtype)
    nd = x.dim()
    z = (x - chan(mean.to(dtype), nd)) * chan(invstd.to(dtype), nd)
    if weight is not None:
        z = z * chan(weight.to(dtype), nd)
    if bias is not None:
        z = z + chan(bias.to(dtype), nd)
    if residual is not None:
        z = z + residual.to(dtype)
    return z


def activation(z, act, slope=0.0):
    if not act:
        return z
    return torch.where(z > 0, z, slope * z)


def gate(dy, z, act, slope=0.0):
    """dy through the activation's derivative; z == 0 is the negative side."""
    if not act:
        return dy
    return torch.where(z > 0, dy, slope * dy)


def elemt(x, mean, invstd, weight, bias, residual=None, act=False, slope=0.0,
          dtype=torch.float64):
    """y = act((x - mean)*invstd*w + b [+ residual])"""
    return activation(
        pre_activation(x, mean, invstd, weight, bias, residual, dtype),
        act, slope)


def backward_reduce(dy, x, mean, invstd, weight, bias, residual=None,
                    act=False, slope=0.0, dtype=torch.float64):
    """-> dict(sum_dy, sum_dy_xmu, grad_weight, grad_bias, g, abs_dy, abs_xmu)
    with g the gated gradient; abs_* are the sums of term magnitudes (what a
    rounding bound of the kernel's summation scales with)."""
    x64, nd = x.to(dtype), x.dim()
    g = dy.to(dtype)
    if act:
        g = gate(g, pre_activation(x, mean, invstd, weight, bias, residual,
                                   dtype), act, slope)
    dims = _red_dims(x)
    t = g * (x64 - chan(mean.to(dtype), nd))
    sum_dy_xmu = t.sum(dims)
    return {
        "sum_dy": g.sum(dims), "sum_dy_xmu": sum_dy_xmu,
        "grad_weight": sum_dy_xmu * invstd.to(dtype), "grad_bias": g.sum(dims),
        "g": g, "abs_dy": g.abs().sum(dims), "abs_xmu": t.abs().sum(dims),
    }


def backward_elemt(dy, x, mean, invstd, weight, bias, sum_dy, sum_dy_xmu,
                   count, residual=None, act=False, slope=0.0,
                   dtype=torch.float64):
    """(dx, dres): dx = (g - sum_dy/n - (x-mean)*invstd^2*sum_dy_xmu/n)
    * invstd*w, dres = g."""
    x64, nd = x.to(dtype), x.dim()
    g = dy.to(dtype)
    if act:
        g = gate(g, pre_activation(x, mean, invstd, weight, bias, residual,
                                   dtype), act, slope)
    istd = chan(invstd.to(dtype), nd)
    xmu = x64 - chan(mean.to(dtype), nd)
    dx = (g - chan(sum_dy.to(dtype), nd) / count
          - xmu * istd * istd * chan(sum_dy_xmu.to(dtype), nd) / count) * istd
    if weight is not None:
        dx = dx * chan(weight.to(dtype), nd)
    return dx, g


def frozen_backward(dy, x, residual, running_mean, running_var, eps, weight,
                    bias, act=False, slope=0.0, dtype=torch.float64):
    """(dx, dres) of y = act((x - rm)*rsqrt(rv+eps)*w + b [+ res]) with the
    statistics held fixed: dx = g*rsqrt(rv+eps)*w, dres = g."""
    invstd = torch.rsqrt(running_var.to(dtype) + eps)
    g = dy.to(dtype)
    if act:
        g = gate(g, pre_activation(x, running_mean, invstd, weight, bias,
                                   residual, dtype), act, slope)
    scale = invstd if weight is None else invstd * weight.to(dtype)
    return g * chan(scale, dy.dim()), g
