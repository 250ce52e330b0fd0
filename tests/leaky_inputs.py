"""Inputs for the fused BN + LeakyReLU comparisons, drawn with a gate margin.

A sign flip of the pre-activation z between two arithmetics (CPU vs GPU,
fused vs composed) changes one gradient element by (1 - slope)*dy; no
tolerance absorbs that.  So every comparison draws its inputs here: the
pre-activation is computed in fp64 from the (already dtype-rounded) inputs,
with batch statistics AND with the drawn running statistics, without and with
the residual, and the draw is only accepted when min|z| >= MARGIN for all of
them.  fp32 evaluation of z = scale*x + shift (+ res) at these magnitudes
errs by ~1e-6, an order below the margin.

Keep shapes under ~20k elements: min|z| of N standard-normal-ish values is
~1/N, so a 1.2M-element tensor never clears the margin.
"""

import torch

MARGIN = 1e-5
EPS = 1e-5
SEEDS = range(20)


def _min_abs_preact(x, res, w, b, mean, var):
    shape = [1, -1] + [1] * (x.dim() - 2)
    z = (x - mean.reshape(shape)) * torch.rsqrt(var.reshape(shape) + EPS)
    z = z * w.reshape(shape) + b.reshape(shape)
    return min(z.abs().min().item(), (z + res).abs().min().item())


def _draw(shape, dtype, seed, batch, running):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    d = {
        "x": torch.randn(shape, generator=g).to(dtype),
        "res": torch.randn(shape, generator=g).to(dtype),
        "w": torch.randn(C, generator=g).abs() + 0.1,
        "b": torch.randn(C, generator=g),
        "dy": torch.randn(shape, generator=g).to(dtype),
        "rm": 0.5 * torch.randn(C, generator=g),
        "rv": torch.rand(C, generator=g) + 0.5,
    }
    x, res = d["x"].double(), d["res"].double()
    w, b = d["w"].double(), d["b"].double()
    dims = [0] + list(range(2, len(shape)))
    margin = float("inf")
    if batch:
        margin = _min_abs_preact(x, res, w, b, x.mean(dims),
                                 x.var(dims, unbiased=False))
    if running:
        margin = min(margin, _min_abs_preact(x, res, w, b, d["rm"].double(),
                                             d["rv"].double()))
    return d, margin


def gated_inputs(shape, dtype=torch.float32, batch=True, running=True):
    """dict(x, res, w, b, dy, rm, rv) from the first seed in 0..19 whose fp64
    pre-activations (with batch statistics if ``batch``, with the running
    statistics rm / rv if ``running``; each with and without res) all keep
    |z| >= MARGIN; fails the test when no seed does."""
    assert batch or running
    best = 0.0
    for seed in SEEDS:
        d, margin = _draw(tuple(shape), dtype, seed, batch, running)
        if margin >= MARGIN:
            d["seed"] = seed
            return d
        best = max(best, margin)
    raise AssertionError(
        f"no seed in 0..19 gives min|z| >= {MARGIN} for shape {tuple(shape)} "
        f"{dtype} (best {best:.3g})"
    )
