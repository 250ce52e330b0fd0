"""Pure-PyTorch reference implementations of the msbn BatchNorm op set.

These are the CPU execution path and the numerics oracle for the HIP kernels.
Semantics mirror the five ATen ops the stock SyncBatchNorm path calls
(signatures verified in SURVEY.md §2.3 against
/usr/local/lib/python3.10/dist-packages/torch/include/ATen/ops/batch_norm_*.h):

  batch_norm_stats                       -> per-channel (mean, invstd), biased var
  batch_norm_gather_stats_with_counts    -> combine per-rank moments (Chan merge),
                                            update running stats in-place (unbiased)
  batch_norm_elemt                       -> y = (x - mean) * invstd * w + b
  batch_norm_backward_reduce             -> (sum_dy, sum_dy_xmu, grad_weight, grad_bias)
  batch_norm_backward_elemt              -> grad_input with global count

All statistics accumulate in float32 (float64 internally for the reductions, to
serve as oracle), matching the fp32-accumulator rule of the stock kernels for
half/bf16 inputs (SURVEY.md §2.3 mixed-dtype rules).
"""

from typing import Optional, Tuple

import torch


def _flatten_to_ncs(input: torch.Tensor) -> torch.Tensor:
    """View (N, C, *spatial) as (N, C, S). 2-D input (N, C) becomes (N, C, 1)."""
    if input.dim() == 2:
        return input.unsqueeze(-1)
    return input.reshape(input.shape[0], input.shape[1], -1)


def batch_norm_stats(input: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-channel mean and inverse std (1/sqrt(biased_var + eps)) over N x spatial.

    Returns float32 tensors of shape [C].  Empty input (0 elements per channel)
    returns zeros for mean and invstd (the caller masks by count, matching the
    zero-count handling of the stock sync path).
    """
    x = _flatten_to_ncs(input)
    C = x.shape[1]
    n = x.shape[0] * x.shape[2]
    if n == 0:
        z = torch.zeros(C, dtype=torch.float32, device=input.device)
        return z, z.clone()
    xd = x.transpose(0, 1).reshape(C, -1).to(torch.float64)
    mean = xd.mean(dim=1)
    var = xd.var(dim=1, unbiased=False)
    invstd = torch.rsqrt(var + eps)
    return mean.to(torch.float32), invstd.to(torch.float32)


def batch_norm_gather_stats_with_counts(
    input: torch.Tensor,
    mean_all: torch.Tensor,
    invstd_all: torch.Tensor,
    running_mean: Optional[torch.Tensor],
    running_var: Optional[torch.Tensor],
    momentum: float,
    eps: float,
    counts: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Combine W rows of per-rank (mean, invstd, count) into global (mean, invstd).

    mean_all/invstd_all: [W, C] float32; counts: [W] (any float/int dtype).
    Zero-count rows are ignored.  Updates running_mean/running_var in-place with
    momentum and the UNBIASED global variance (n-1 divisor), matching
    batch_norm_gather_stats_with_counts.
    ``input`` is only consulted for dtype/device (as in ATen).
    """
    cnt = counts.to(torch.float64)
    m = mean_all.to(torch.float64)
    # var_r reconstructed from invstd: var = 1/invstd^2 - eps.
    # Guard zero-count ranks (invstd == 0) BEFORE the reciprocal.
    istd = invstd_all.to(torch.float64)
    safe = torch.where(istd == 0, torch.ones_like(istd), istd)
    var = torch.where(istd == 0, torch.zeros_like(istd), safe.pow(-2) - eps)
    mask = (cnt > 0).to(torch.float64)  # [W]
    n_tot = (cnt * mask).sum()
    if n_tot.item() == 0:
        C = mean_all.shape[1]
        z = torch.zeros(C, dtype=torch.float32, device=mean_all.device)
        return z, z.clone()
    w = (cnt * mask).unsqueeze(1)  # [W,1]
    mean_g = (m * w).sum(dim=0) / n_tot
    # Chan combine: E[x^2] based merge (biased variance over the union)
    ex2 = ((var + m * m) * w).sum(dim=0) / n_tot
    var_g = ex2 - mean_g * mean_g
    invstd_g = torch.rsqrt(var_g + eps)

    if running_mean is not None:
        running_mean.mul_(1 - momentum).add_(
            mean_g.to(running_mean.dtype), alpha=momentum
        )
    if running_var is not None:
        unbiased = var_g * (n_tot / (n_tot - 1.0)) if n_tot.item() > 1 else var_g
        running_var.mul_(1 - momentum).add_(
            unbiased.to(running_var.dtype), alpha=momentum
        )
    return mean_g.to(torch.float32), invstd_g.to(torch.float32)


def _chan_view(t: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Reshape per-channel [C] tensor for broadcast against (N, C, *spatial) ref."""
    shape = [1] * ref.dim()
    shape[1] = ref.shape[1]
    return t.reshape(shape)


def batch_norm_elemt(
    input: torch.Tensor,
    weight: Optional[torch.Tensor],
    bias: Optional[torch.Tensor],
    mean: torch.Tensor,
    invstd: torch.Tensor,
    eps: float,
) -> torch.Tensor:
    """y = (x - mean) * invstd * weight + bias, elementwise per channel.

    Output dtype == input dtype; math in float32.
    """
    xf = input.to(torch.float32)
    scale = invstd.to(torch.float32)
    if weight is not None:
        scale = scale * weight.to(torch.float32)
    shift = -mean.to(torch.float32) * scale
    if bias is not None:
        shift = shift + bias.to(torch.float32)
    y = xf * _chan_view(scale, input) + _chan_view(shift, input)
    return y.to(input.dtype)


def _act_coefs(mean, invstd, weight, bias):
    scale = invstd.to(torch.float32)
    if weight is not None:
        scale = scale * weight.to(torch.float32)
    shift = -mean.to(torch.float32) * scale
    if bias is not None:
        shift = shift + bias.to(torch.float32)
    return scale, shift


def batch_norm_elemt_act(
    input, residual, weight, bias, mean, invstd, relu: bool,
    negative_slope: float = 0.0,
):
    """y = act?(x*scale + shift [+ residual]) — fused epilogue reference.
    ``negative_slope`` (consulted only with ``relu``) selects LeakyReLU."""
    scale, shift = _act_coefs(mean, invstd, weight, bias)
    z = input.to(torch.float32) * _chan_view(scale, input) + _chan_view(
        shift, input
    )
    if residual is not None:
        z = z + residual.to(torch.float32)
    if relu:
        if negative_slope == 0.0:
            z = torch.relu(z)
        else:
            z = torch.where(z > 0, z, negative_slope * z)
    return z.to(input.dtype)


def _gate(z, g, negative_slope: float):
    """g through the activation's gate; z == 0 takes the negative branch."""
    if negative_slope == 0.0:
        return torch.where(z > 0, g, torch.zeros_like(g))
    return torch.where(z > 0, g, negative_slope * g)


def _masked_grad(grad_out, input, residual, mean, invstd, weight, bias,
                 relu_mask: bool, negative_slope: float = 0.0):
    g = grad_out.to(torch.float32)
    if relu_mask:
        scale, shift = _act_coefs(mean, invstd, weight, bias)
        z = input.to(torch.float32) * _chan_view(scale, input) + _chan_view(
            shift, input
        )
        if residual is not None:
            z = z + residual.to(torch.float32)
        g = _gate(z, g, negative_slope)
    return g


def batch_norm_backward_reduce_act(
    grad_out, input, residual, mean, invstd, weight, bias, relu_mask,
    input_g, weight_g, bias_g, gm_out=None, negative_slope: float = 0.0,
    grad_out2=None,
):
    if grad_out2 is not None:
        # the two gradients of a forked output: summed in the input dtype
        # first (one rounding), as autograd's own accumulation would
        grad_out = grad_out + grad_out2
    g = _masked_grad(grad_out, input, residual, mean, invstd, weight, bias,
                     relu_mask, negative_slope)
    if gm_out is not None:
        gm_out.copy_(g.to(grad_out.dtype))
    return batch_norm_backward_reduce(
        g, input, mean, invstd, weight, input_g, weight_g, bias_g
    )


def batch_norm_backward_elemt_act(
    grad_out, input, residual, mean, invstd, weight, bias, sum_dy,
    sum_dy_xmu, count, relu_mask, want_res_grad, negative_slope: float = 0.0,
):
    g = _masked_grad(grad_out, input, residual, mean, invstd, weight, bias,
                     relu_mask, negative_slope)
    dx = batch_norm_backward_elemt(
        g, input, mean, invstd, weight, sum_dy, sum_dy_xmu, count
    )
    dres = g.to(grad_out.dtype) if want_res_grad else None
    return dx, dres


# ---- stem pool fusion: bn + act + MaxPool2d(3, 2, 1) -----------------------
# Same code convention and rounding points as the kernels: the maximum is
# taken over y ROUNDED to the input dtype, scanning kh then kw ascending with
# `val > max or isnan(val)` (first maximum wins); the code of a pooled
# element is kh*3 + kw.  The backward gathers, per x element, the pooled
# gradient of every window whose code names it: fp32 sum in ascending
# (oh, ow) order, rounded to the input dtype once.

def pool_out_size(size: int) -> int:
    """Output length of the fixed kernel-3 / stride-2 / padding-1 pool."""
    return (size - 1) // 2 + 1


def _pooled_like(t: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    if ref.is_contiguous(memory_format=torch.channels_last):
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def batch_norm_elemt_act_pool(input, weight, bias, mean, invstd, relu: bool,
                              negative_slope: float = 0.0):
    """(pooled, codes) of maxpool_3_2_1(act?(x*scale + shift)); codes uint8."""
    y = batch_norm_elemt_act(input, None, weight, bias, mean, invstd, relu,
                             negative_slope)
    N, C, H, W = y.shape
    OH, OW = pool_out_size(H), pool_out_size(W)
    yp = torch.nn.functional.pad(y.to(torch.float32), (1, 1, 1, 1),
                                 value=float("-inf"))
    best = torch.full((N, C, OH, OW), float("-inf"), dtype=torch.float32,
                      device=y.device)
    # first window position inside the image (what an all -inf window keeps)
    first_h = torch.zeros(OH, dtype=torch.uint8, device=y.device)
    first_w = torch.zeros(OW, dtype=torch.uint8, device=y.device)
    first_h[0] = 3
    first_w[0] = 1
    codes = (first_h.reshape(1, 1, OH, 1) + first_w.reshape(1, 1, 1, OW)
             ).expand(N, C, OH, OW).clone()
    for kh in range(3):
        for kw in range(3):
            val = yp[:, :, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2]
            upd = (val > best) | torch.isnan(val)
            best = torch.where(upd, val, best)
            codes = torch.where(upd, torch.full_like(codes, kh * 3 + kw),
                                codes)
    return (_pooled_like(best.to(input.dtype), input),
            _pooled_like(codes, input))


def pool_codes_to_indices(codes: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """torch's max_pool2d indices (h*W + w of the chosen element, int64)."""
    OH, OW = codes.shape[2], codes.shape[3]
    c = codes.to(torch.int64)
    oh = torch.arange(OH, device=codes.device).reshape(1, 1, OH, 1)
    ow = torch.arange(OW, device=codes.device).reshape(1, 1, 1, OW)
    return (2 * oh - 1 + c // 3) * W + (2 * ow - 1 + c % 3)


def pool_gather_grad(grad_out, grad_out2, codes, input):
    """The full-size gradient the pool's backward stores, in the input
    dtype: zero where no window chose the element."""
    g = grad_out
    if grad_out2 is not None:
        g = grad_out + grad_out2  # one rounding, as the eager add
    g = g.to(torch.float32)
    N, C, H, W = input.shape
    OH, OW = codes.shape[2], codes.shape[3]
    full = torch.zeros((N, C, H, W), dtype=torch.float32,
                       device=input.device)
    # ascending (oh, ow) for a fixed element == descending (kh, kw)
    for kh in (2, 1, 0):
        lo_h = 1 if kh == 0 else 0
        hi_h = min(OH - 1, (H - kh) // 2)
        for kw in (2, 1, 0):
            lo_w = 1 if kw == 0 else 0
            hi_w = min(OW - 1, (W - kw) // 2)
            if hi_h < lo_h or hi_w < lo_w:
                continue
            sel = (slice(None), slice(None), slice(lo_h, hi_h + 1),
                   slice(lo_w, hi_w + 1))
            part = torch.where(codes[sel] == kh * 3 + kw, g[sel],
                               torch.zeros_like(g[sel]))
            h0, w0 = 2 * lo_h - 1 + kh, 2 * lo_w - 1 + kw
            dst = (slice(None), slice(None),
                   slice(h0, h0 + 2 * (hi_h - lo_h) + 1, 2),
                   slice(w0, w0 + 2 * (hi_w - lo_w) + 1, 2))
            full[dst] = full[dst] + part
    full = full.to(input.dtype)
    if input.is_contiguous(memory_format=torch.channels_last):
        full = full.contiguous(memory_format=torch.channels_last)
    return full


def batch_norm_backward_reduce_act_pool(
    grad_out, grad_out2, codes, input, mean, invstd, weight, bias, relu_mask,
    input_g, weight_g, bias_g, negative_slope: float = 0.0,
):
    g = pool_gather_grad(grad_out, grad_out2, codes, input)
    return batch_norm_backward_reduce_act(
        g, input, None, mean, invstd, weight, bias, relu_mask, input_g,
        weight_g, bias_g, None, negative_slope,
    )


def batch_norm_backward_elemt_act_pool(
    grad_out, grad_out2, codes, input, mean, invstd, weight, bias, sum_dy,
    sum_dy_xmu, count, relu_mask, negative_slope: float = 0.0,
):
    g = pool_gather_grad(grad_out, grad_out2, codes, input)
    return batch_norm_backward_elemt_act(
        g, input, None, mean, invstd, weight, bias, sum_dy, sum_dy_xmu,
        count, relu_mask, False, negative_slope,
    )[0]


# ---- in-place activated path ----------------------------------------------
# fp32 throughout, in the kernels' order of operations: these are the CPU
# execution path of the in-place ops, and they really overwrite ``input``.

def _check_invertible(act: bool, negative_slope: float, name: str):
    if act and not negative_slope > 0.0:
        raise RuntimeError(
            f"{name}: the in-place path needs an invertible activation "
            "(identity, or LeakyReLU with negative_slope > 0); got "
            f"negative_slope={negative_slope}"
        )


def _slope32(negative_slope: float):
    s = torch.tensor(negative_slope, dtype=torch.float32)
    return s, 1.0 / s


def _invert_act(grad_out, output, act: bool, negative_slope: float):
    """(g, z) in fp32 from the stored y: the gate and the pre-activation."""
    g = grad_out.to(torch.float32)
    z = output.to(torch.float32)
    if act:
        s, inv_s = _slope32(negative_slope)
        pos = z > 0
        g = torch.where(pos, g, s * g)
        z = torch.where(pos, z, z * inv_s)
    return g, z


def _rscale(invstd, weight):
    sc = invstd.to(torch.float32)
    if weight is not None:
        sc = sc * weight.to(torch.float32)
    safe = torch.where(sc != 0, sc, torch.ones_like(sc))
    return torch.where(sc != 0, 1.0 / safe, torch.zeros_like(sc))


def batch_norm_elemt_act_(input, weight, bias, mean, invstd, act: bool,
                          negative_slope: float = 0.0):
    """input <- act?(input*scale + shift), written over ``input``."""
    _check_invertible(act, negative_slope, "batch_norm_elemt_act_")
    if input.numel() > 0:
        input.copy_(batch_norm_elemt_act(input, None, weight, bias, mean,
                                         invstd, act, negative_slope))
    return input


def batch_norm_backward_reduce_inplace(grad_out, output, invstd, weight, bias,
                                       act: bool, input_g, weight_g, bias_g,
                                       negative_slope: float = 0.0):
    """The backward reductions from the stored output y:
    sum_dy = sum g, sum_dy_xmu = sum g*((z - bias)*(1/scale)), with the fp32
    terms the kernels form (summed in fp64)."""
    _check_invertible(act, negative_slope,
                      "batch_norm_backward_reduce_inplace")
    C = output.shape[1]
    wdtype = weight.dtype if weight is not None else output.dtype
    g, z = _invert_act(grad_out, output, act, negative_slope)
    rs = _rscale(invstd, weight)
    bi = (bias.to(torch.float32) if bias is not None
          else torch.zeros(C, dtype=torch.float32, device=output.device))
    t = g * ((z - _chan_view(bi, output)) * _chan_view(rs, output))
    s_dy = _flatten_to_ncs(g).to(torch.float64).sum(dim=(0, 2))
    s_dy_xmu = _flatten_to_ncs(t).to(torch.float64).sum(dim=(0, 2))
    combined = torch.cat([s_dy, s_dy_xmu]).to(torch.float32)
    grad_weight = ((s_dy_xmu * invstd.to(torch.float64)).to(wdtype)
                   if weight_g else None)
    grad_bias = s_dy.to(wdtype) if bias_g else None
    return combined[:C], combined[C:], grad_weight, grad_bias


def batch_norm_backward_elemt_inplace(grad_out, output, mean, invstd, weight,
                                      bias, sum_dy, sum_dy_xmu, count,
                                      act: bool, negative_slope: float = 0.0):
    """dx = a*g + (b/scale)*z + d' from the stored output y, with (a, b) of
    the out-of-place backward and d' = -a*sum_dy/n - (b/scale)*bias."""
    _check_invertible(act, negative_slope,
                      "batch_norm_backward_elemt_inplace")
    if output.numel() == 0:
        return torch.empty_like(grad_out)
    n = count.sum().to(torch.float32)
    g, z = _invert_act(grad_out, output, act, negative_slope)
    istd = invstd.to(torch.float32)
    f1 = istd * (weight.to(torch.float32) if weight is not None else 1.0)
    f3 = istd * istd * sum_dy_xmu.to(torch.float32) / n
    ca = f1
    cbz = (-f1 * f3) * _rscale(invstd, weight)
    cdz = -(ca * (sum_dy.to(torch.float32) / n))
    if bias is not None:
        cdz = cdz - cbz * bias.to(torch.float32)
    if not n > 0:
        ca, cbz, cdz = (torch.zeros_like(istd),) * 3
    dx = (_chan_view(ca, output) * g + _chan_view(cbz, output) * z
          + _chan_view(cdz, output))
    return dx.to(grad_out.dtype)


def bn_frozen_coefs(running_mean, running_var, eps: float, weight, bias):
    """Packed fp32 [scale(C) | shift(C)] from fixed running statistics:
    scale = weight / sqrt(running_var + eps), shift = bias - running_mean*scale."""
    invstd = torch.rsqrt(running_var.to(torch.float32) + eps)
    scale, shift = _act_coefs(running_mean, invstd, weight, bias)
    return torch.cat([scale, shift])


def batch_norm_frozen_backward_elemt(
    grad_out, input, residual, coefs, relu_mask: bool,
    want_input_grad: bool, want_res_grad: bool, negative_slope: float = 0.0,
):
    """Backward of y = act?(x*scale + shift [+ residual]) with FIXED scale /
    shift: dx = scale*g, dres = g, g = grad_out * 1[z > 0] (or
    negative_slope*grad_out where z <= 0).  ``input`` and ``residual`` are
    only consulted for the gate (relu_mask)."""
    C = grad_out.shape[1]
    scale = _chan_view(coefs[:C], grad_out)
    g = grad_out.to(torch.float32)
    if relu_mask:
        z = input.to(torch.float32) * scale + _chan_view(coefs[C:], grad_out)
        if residual is not None:
            z = z + residual.to(torch.float32)
        g = _gate(z, g, negative_slope)
    dx = (g * scale).to(grad_out.dtype) if want_input_grad else None
    dres = None
    if want_res_grad:
        dres = g.to(grad_out.dtype) if relu_mask else grad_out
    return dx, dres


def batch_norm_backward_reduce(
    grad_out: torch.Tensor,
    input: torch.Tensor,
    mean: torch.Tensor,
    invstd: torch.Tensor,
    weight: Optional[torch.Tensor],
    input_g: bool,
    weight_g: bool,
    bias_g: bool,
) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Per-channel reductions of the BN backward:
      sum_dy      = sum(dy)                      [float32, C]  (if input_g)
      sum_dy_xmu  = sum(dy * (x - mean))         [float32, C]  (if input_g)
      grad_weight = sum(dy * (x - mean)) * invstd  (dtype of weight, if weight_g)
      grad_bias   = sum(dy)                        (dtype of weight, if bias_g)
    """
    dy = _flatten_to_ncs(grad_out).to(torch.float64)
    x = _flatten_to_ncs(input).to(torch.float64)
    m = mean.to(torch.float64).reshape(1, -1, 1)
    s_dy = dy.sum(dim=(0, 2))
    s_dy_xmu = (dy * (x - m)).sum(dim=(0, 2))
    wdtype = weight.dtype if weight is not None else torch.float32
    sum_dy = s_dy.to(torch.float32) if input_g else None
    sum_dy_xmu = s_dy_xmu.to(torch.float32) if input_g else None
    grad_weight = (s_dy_xmu * invstd.to(torch.float64)).to(wdtype) if weight_g else None
    grad_bias = s_dy.to(wdtype) if bias_g else None
    return sum_dy, sum_dy_xmu, grad_weight, grad_bias


def batch_norm_backward_elemt(
    grad_out: torch.Tensor,
    input: torch.Tensor,
    mean: torch.Tensor,
    invstd: torch.Tensor,
    weight: Optional[torch.Tensor],
    sum_dy: torch.Tensor,
    sum_dy_xmu: torch.Tensor,
    count: torch.Tensor,
) -> torch.Tensor:
    """grad_input = (dy - sum_dy/n - (x-mean)*invstd^2*sum_dy_xmu/n) * invstd * w

    with n = count.sum() (global element count across ranks).  Output dtype ==
    grad_out dtype; math in float32.
    """
    n = count.sum().to(torch.float32)
    dy = grad_out.to(torch.float32)
    x = input.to(torch.float32)
    istd = invstd.to(torch.float32)
    f_scale = istd * (weight.to(torch.float32) if weight is not None else 1.0)
    mean_dy = sum_dy.to(torch.float32) / n
    proj = istd * istd * sum_dy_xmu.to(torch.float32) / n
    dx = (
        dy
        - _chan_view(mean_dy, input)
        - (x - _chan_view(mean.to(torch.float32), input)) * _chan_view(proj, input)
    ) * _chan_view(f_scale, input)
    return dx.to(grad_out.dtype)
