"""msbn.ops — the BatchNorm math op layer.

Dispatch policy:
  * CUDA (= HIP/MI355X) tensors -> the hand-written gfx950 kernels in the
    in-tree extension ``msbn._C`` (built by setup.py / __graft_entry__.build()).
    If the extension is missing on a GPU machine the ops raise — there is no
    silent eager fallback on the GPU path.
  * CPU tensors -> the pure-PyTorch reference implementations (used by the
    CPU/gloo plumbing config and as the numerics oracle in tests).

Op semantics: SURVEY.md §2.3 (the five stock SyncBatchNorm ATen ops).
"""

from typing import Optional

import torch

from msbn.ops import _reference as _ref

_C = None
_C_IMPORT_ERROR: Optional[BaseException] = None
try:  # built in-tree: msbn/_C*.so
    import os as _os

    if _os.environ.get("MSBN_AB_NONT", "0") == "1":
        # A/B measurement knob: route every op through the cached-access
        # build (no nontemporal bits).  Needs MSBN_BUILD_NONT=1 at setup.
        from msbn import _C_nont as _C  # type: ignore
    else:
        from msbn import _C as _C  # type: ignore
except Exception as e:  # pragma: no cover - exercised only when ext missing
    _C_IMPORT_ERROR = e


def hip_available() -> bool:
    """True when the gfx950 extension is importable."""
    return _C is not None


def _require_hip():
    if _C is None:
        raise RuntimeError(
            "msbn._C (the gfx950 HIP kernel extension) is not built, but a CUDA "
            "tensor reached msbn.ops. Build it with `python setup.py "
            "build_ext --inplace` (or __graft_entry__.build()). "
            f"Import error was: {_C_IMPORT_ERROR!r}"
        )
    return _C


def batch_norm_stats(input: torch.Tensor, eps: float):
    """Per-channel (mean, invstd) in fp32; invstd = 1/sqrt(biased_var + eps)."""
    if input.is_cuda:
        return _require_hip().batch_norm_stats(input, eps)
    return _ref.batch_norm_stats(input, eps)


def batch_norm_stats_packed(input: torch.Tensor, eps: float, out: torch.Tensor):
    """Fused variant: write [mean(C) | invstd(C) | count(1)] into ``out`` (2C+1 fp32).

    Saves the cat() + extra kernels of the stock path (SURVEY.md §2.2
    _functions.py:41-49) — the packed buffer is what the all_gather ships.
    Falls back to stats + copies on CPU.
    """
    C = input.shape[1]
    if input.is_cuda:
        _require_hip().batch_norm_stats_packed(input, eps, out)
        return out
    mean, invstd = _ref.batch_norm_stats(input, eps)
    out[:C] = mean
    out[C : 2 * C] = invstd
    n = input.numel() // C if C > 0 else 0
    out[2 * C] = float(n)
    return out


def batch_norm_gather_stats_with_counts(
    input: torch.Tensor,
    mean_all: torch.Tensor,
    invstd_all: torch.Tensor,
    running_mean: Optional[torch.Tensor],
    running_var: Optional[torch.Tensor],
    momentum: float,
    eps: float,
    counts: torch.Tensor,
):
    if input.is_cuda:
        return _require_hip().batch_norm_gather_stats_with_counts(
            mean_all, invstd_all, running_mean, running_var, momentum, eps, counts
        )
    return _ref.batch_norm_gather_stats_with_counts(
        input, mean_all, invstd_all, running_mean, running_var, momentum, eps, counts
    )


def batch_norm_gather_stats_packed(
    input: torch.Tensor,
    packed_all: torch.Tensor,  # [W, 2C+1] fp32: per-rank [mean | invstd | count]
    running_mean: Optional[torch.Tensor],
    running_var: Optional[torch.Tensor],
    momentum: float,
    eps: float,
):
    """Combine the all-gathered packed per-rank stats; returns (mean, invstd, count_sum).

    Zero-count ranks are masked INSIDE the kernel — no GPU->CPU sync (the stock
    path's mask at _functions.py:88-100 forces one per BN layer).
    count_sum is returned as a 1-element fp32 tensor on device.
    """
    W = packed_all.shape[0]
    C = (packed_all.shape[1] - 1) // 2
    if input.is_cuda:
        return _require_hip().batch_norm_gather_stats_packed(
            packed_all, running_mean, running_var, momentum, eps
        )
    mean_all = packed_all[:, :C]
    invstd_all = packed_all[:, C : 2 * C]
    counts = packed_all[:, 2 * C]
    mean, invstd = _ref.batch_norm_gather_stats_with_counts(
        input, mean_all, invstd_all, running_mean, running_var, momentum, eps, counts
    )
    return mean, invstd, counts.sum().reshape(1)


def batch_norm_elemt(
    input: torch.Tensor,
    weight: Optional[torch.Tensor],
    bias: Optional[torch.Tensor],
    mean: torch.Tensor,
    invstd: torch.Tensor,
    eps: float,
):
    if input.is_cuda:
        return _require_hip().batch_norm_elemt(input, weight, bias, mean, invstd, eps)
    return _ref.batch_norm_elemt(input, weight, bias, mean, invstd, eps)


def batch_norm_backward_reduce(
    grad_out: torch.Tensor,
    input: torch.Tensor,
    mean: torch.Tensor,
    invstd: torch.Tensor,
    weight: Optional[torch.Tensor],
    input_g: bool,
    weight_g: bool,
    bias_g: bool,
):
    if input.is_cuda:
        return _require_hip().batch_norm_backward_reduce(
            grad_out, input, mean, invstd, weight, input_g, weight_g, bias_g
        )
    return _ref.batch_norm_backward_reduce(
        grad_out, input, mean, invstd, weight, input_g, weight_g, bias_g
    )


def batch_norm_backward_elemt(
    grad_out: torch.Tensor,
    input: torch.Tensor,
    mean: torch.Tensor,
    invstd: torch.Tensor,
    weight: Optional[torch.Tensor],
    sum_dy: torch.Tensor,
    sum_dy_xmu: torch.Tensor,
    count: torch.Tensor,
):
    if input.is_cuda:
        return _require_hip().batch_norm_backward_elemt(
            grad_out, input, mean, invstd, weight, sum_dy, sum_dy_xmu, count
        )
    return _ref.batch_norm_backward_elemt(
        grad_out, input, mean, invstd, weight, sum_dy, sum_dy_xmu, count
    )


def bn_fused_local_eligible(input, weight, bias, running_mean, running_var):
    """True when the single-launch small-plane world-1 kernels apply
    (NCHW, plane <= 256K elems, C >= 64, fp32 stats/affine)."""
    if not input.is_cuda or _C is None:
        return False
    return _C.bn_fused_local_eligible(
        input, weight, bias, running_mean, running_var
    )


def batch_norm_fwd_fused_local(input, residual, weight, bias, eps, momentum,
                               running_mean, running_var, relu,
                               negative_slope: float = 0.0):
    """ONE kernel: local stats + running update + normalize(+res)(+relu,
    or LeakyReLU for a non-zero ``negative_slope``).
    Returns (y, mean, invstd, count[1], coefs[2C])."""
    return _require_hip().batch_norm_fwd_fused_local(
        input, residual, weight, bias, eps, momentum, running_mean,
        running_var, relu, negative_slope,
    )


def batch_norm_bwd_fused_local(grad_out, input, residual, mean, invstd,
                               weight, coefs, relu_mask, want_res_grad,
                               weight_g, bias_g, negative_slope: float = 0.0):
    """ONE kernel: whole local BN backward (reduce + coefs + dx(+dres))."""
    return _require_hip().batch_norm_bwd_fused_local(
        grad_out, input, residual, mean, invstd, weight, coefs, relu_mask,
        want_res_grad, weight_g, bias_g, negative_slope,
    )


def bn_make_coefs(mean, invstd, weight, bias):
    """Packed [scale | shift] fp32 per-channel affine (GPU); None on CPU."""
    if mean.is_cuda:
        return _require_hip().bn_make_coefs(mean, invstd, weight, bias)
    return None


def _act_name(relu: bool, negative_slope: float, act: Optional[str]) -> str:
    """The extension's spelling of ``act`` ("" for None), validated here so
    that CPU and GPU tensors raise alike."""
    if act is None:  # the common case, on every BN layer's hot path
        return ""
    return "silu" if _ref.check_act(relu, negative_slope, act) else ""


def gate_bits_empty(input: torch.Tensor) -> torch.Tensor:
    """An unwritten gate-bit tensor for ``input``: ``ceil(numel/8)`` uint8."""
    return torch.empty((input.numel() + 7) // 8, dtype=torch.uint8,
                       device=input.device)


def batch_norm_elemt_act(input, residual, weight, bias, mean, invstd,
                         relu: bool, coefs=None, negative_slope: float = 0.0,
                         gate_out=None, act: Optional[str] = None):
    """y = act(x*scale + shift [+ residual]); ``relu`` turns the activation
    on and ``negative_slope`` (only consulted then) makes it a LeakyReLU.
    ``act`` names an activation the pair cannot: ``None`` is ``(relu,
    negative_slope)`` as ever, ``"silu"`` (with ``relu`` true and a zero
    slope) is y = z*sigmoid(z).  SiLU has no branch, so it never writes gate
    bits.

    ``gate_out`` (``gate_bits_empty(input)``) asks the kernel to also store
    which branch the activation took, one bit per element: bit ``e & 7`` of
    byte ``e >> 3`` for the element at storage offset ``e``, set where the
    backward passes the gradient through (relu: ``not z <= 0``; leaky:
    ``z > 0``).  The call then returns ``(y, gate)`` with ``gate`` either
    ``gate_out``, written, or None: the kernels store bits only for an
    activated layer with a residual running 8 elements per thread (GPU,
    bf16 / half, C — or the plane, for NCHW — a multiple of 8, 16-byte
    aligned tensors), and the caller keeps the residual otherwise.  ``y`` is
    the same with and without ``gate_out``."""
    if input.is_cuda:
        y, wrote = _require_hip().batch_norm_elemt_act(
            input, residual, weight, bias, mean, invstd, relu, coefs,
            negative_slope, gate_out, _act_name(relu, negative_slope, act),
        )
        return y if gate_out is None else (y, gate_out if wrote else None)
    y = _ref.batch_norm_elemt_act(
        input, residual, weight, bias, mean, invstd, relu, negative_slope,
        act,
    )
    return y if gate_out is None else (y, None)


def batch_norm_backward_reduce_act(grad_out, input, residual, mean, invstd,
                                   weight, bias, relu_mask, input_g, weight_g,
                                   bias_g, coefs=None, gm_out=None,
                                   negative_slope: float = 0.0,
                                   grad_out2=None, gate=None,
                                   act: Optional[str] = None, *, dual=None):
    """First pass of the fused BN backward.  ``act`` as in
    ``batch_norm_elemt_act``; ``"silu"`` takes neither ``gate`` nor ``dual``,
    and its ``gm_out`` is g = dy*silu'(z) rounded to the input dtype (as
    LeakyReLU's, not exact).  ``grad_out2`` is the second
    gradient of a forked output, delivered unsummed: the incoming gradient is
    ``grad_out + grad_out2`` rounded to the input dtype once (the tensor an
    eager add would have produced), read inside the reduce kernel instead of
    in a pass of its own.  It requires ``gm_out``.

    ``gate``: the bits ``batch_norm_elemt_act(gate_out=)`` returned for this
    layer, passed INSTEAD of ``residual`` (which must be None): the kernel
    takes the activation's branch from them.  GPU only; requires
    ``relu_mask`` and ``gm_out``.  Same results as with the residual.

    ``dual=(input2, mean2, invstd2, weight2)`` (keyword only; dual BN,
    docs/KERNEL_DESIGN.md): the layer's residual was a second BatchNorm's
    output, ``bn2(input2)``, and the same kernel also forms that layer's
    sums over the gated gradient it writes to ``gm_out``.  Needs ``gate``,
    ``relu_mask`` with a zero slope and ``gm_out``; GPU only.  The call then
    returns ``(sum_dy, sum_dy_xmu, grad_weight, grad_bias, sum_dy_2,
    sum_dy_xmu_2, grad_weight_2, grad_bias_2)``, the four sums being views
    into ONE contiguous fp32 ``[4C]`` buffer in that order (one all_reduce
    for the pair).  ``weight_g`` / ``bias_g`` are the main layer's; the skip
    layer's affine gradients are formed whenever it has a weight (they are
    [C] vectors).  Inputs the dual kernel declines (a
    gradient off 16-byte alignment, ...) run the two single reduces; same
    results."""
    act_name = _act_name(relu_mask, negative_slope, act)
    if act_name and gate is not None:
        raise ValueError("act='silu' has no single-bit gate")
    if dual is not None:
        if not input.is_cuda:
            raise ValueError("the dual reduce exists on the GPU path only")
        if (gate is None or residual is not None or gm_out is None
                or not relu_mask or negative_slope != 0.0):
            raise ValueError(
                "dual needs gate, gm_out, relu_mask with a zero slope and no "
                "residual"
            )
        input2, mean2, invstd2, weight2 = dual
        sums, gw, gb, gw2, gb2 = (
            _require_hip().batch_norm_backward_reduce_act_dual(
                grad_out, input, input2, mean, mean2, invstd, invstd2,
                weight, weight2, weight_g, bias_g, weight2 is not None,
                weight2 is not None, gm_out, grad_out2, gate,
            )
        )
        C = input.shape[1]
        return (sums[:C], sums[C:2 * C], gw, gb, sums[2 * C:3 * C],
                sums[3 * C:], gw2, gb2)
    if input.is_cuda:
        return _require_hip().batch_norm_backward_reduce_act(
            grad_out, input, residual, mean, invstd, weight, bias, relu_mask,
            input_g, weight_g, bias_g, coefs, gm_out, negative_slope,
            grad_out2, gate, act_name,
        )
    if gate is not None:
        raise ValueError("gate bits exist on the GPU path only")
    return _ref.batch_norm_backward_reduce_act(
        grad_out, input, residual, mean, invstd, weight, bias, relu_mask,
        input_g, weight_g, bias_g, gm_out, negative_slope, grad_out2, act,
    )


def batch_norm_backward_elemt_act(grad_out, input, residual, mean, invstd,
                                  weight, bias, sum_dy, sum_dy_xmu, count,
                                  relu_mask, want_res_grad, coefs=None,
                                  negative_slope: float = 0.0,
                                  act: Optional[str] = None):
    """Second pass: dx = a*g + b*x + d, dres = g, with g = grad_out through
    the activation's derivative (``act`` as in ``batch_norm_elemt_act``)."""
    if input.is_cuda:
        dx, dres = _require_hip().batch_norm_backward_elemt_act(
            grad_out, input, residual, mean, invstd, weight, bias, sum_dy,
            sum_dy_xmu, count, relu_mask, want_res_grad, coefs,
            negative_slope, _act_name(relu_mask, negative_slope, act),
        )
        return dx, (dres if want_res_grad else None)
    return _ref.batch_norm_backward_elemt_act(
        grad_out, input, residual, mean, invstd, weight, bias, sum_dy,
        sum_dy_xmu, count, relu_mask, want_res_grad, negative_slope, act,
    )


def batch_norm_elemt_act_dual(input, input2, coefs, coefs2, relu: bool,
                              negative_slope: float, gate_out):
    """``relu(bn(input) + bn2(input2))`` in one kernel (dual BN,
    docs/KERNEL_DESIGN.md): ``coefs`` / ``coefs2`` are the two layers' packed
    ``[scale | shift]`` (``bn_make_coefs``) and ``gate_out``
    (``gate_bits_empty(input)``) receives the gate bits.  ``bn2``'s output is
    rounded to the input dtype in registers and never stored, so ``y`` and
    the bits are those of ``batch_norm_elemt`` followed by
    ``batch_norm_elemt_act(residual=, gate_out=)``.

    Returns ``(y, stored)``.  ``stored`` is False, ``y`` None and nothing is
    written when the kernel declines: anything but dense channels-last 4-D
    bf16 / half GPU tensors with C a multiple of 8 and 16-byte aligned
    pointers, and any activation but plain ReLU."""
    if not input.is_cuda:
        return None, False
    y, stored = _require_hip().batch_norm_elemt_act_dual(
        input, input2, coefs, coefs2, relu, negative_slope, gate_out
    )
    return (y if stored else None), stored


def batch_norm_backward_elemt_dual(gm, input, input2, mean, mean2, invstd,
                                   invstd2, weight, weight2, sums, count):
    """Second backward pass of a dual BN pair: ``(dx, dx2)`` from one read of
    ``gm``.  ``sums`` is the ``[4C]`` buffer the dual reduce returned (after
    its all_reduce).  Same bits as two ``batch_norm_backward_elemt`` calls.
    Takes what ``batch_norm_elemt_act_dual`` takes and raises otherwise."""
    return _require_hip().batch_norm_backward_elemt_dual(
        gm, input, input2, mean, mean2, invstd, invstd2, weight, weight2,
        sums, count,
    )


def batch_norm_elemt_act_pool(input, weight, bias, mean, invstd, relu: bool,
                              coefs=None, negative_slope: float = 0.0):
    """``max_pool2d(act(x*scale + shift), 3, 2, 1)`` without the activation
    tensor: returns ``(pooled, codes)``.  The maximum is taken over the values
    rounded to the input dtype (first maximum in kh, kw order; NaN wins, as
    in torch), and ``codes`` holds one uint8 ``kh*3 + kw`` per pooled
    element.  4-D channels-last input on the GPU."""
    if input.is_cuda:
        return _require_hip().batch_norm_elemt_act_pool(
            input, weight, bias, mean, invstd, relu, coefs, negative_slope
        )
    return _ref.batch_norm_elemt_act_pool(
        input, weight, bias, mean, invstd, relu, negative_slope
    )


def batch_norm_backward_reduce_act_pool(grad_out, grad_out2, codes, input,
                                        mean, invstd, weight, bias, relu_mask,
                                        input_g, weight_g, bias_g, coefs=None,
                                        negative_slope: float = 0.0):
    """``batch_norm_backward_reduce_act`` for a layer run through
    ``batch_norm_elemt_act_pool``: ``grad_out`` (and ``grad_out2``, the second
    gradient of a forked output, or None) are POOLED gradients; the gradient
    of each x element is gathered through ``codes`` inside the kernel, with
    the roundings of the eager add and of the pool's own backward."""
    if input.is_cuda:
        return _require_hip().batch_norm_backward_reduce_act_pool(
            grad_out, grad_out2, codes, input, mean, invstd, weight, bias,
            relu_mask, input_g, weight_g, bias_g, coefs, negative_slope,
        )
    return _ref.batch_norm_backward_reduce_act_pool(
        grad_out, grad_out2, codes, input, mean, invstd, weight, bias,
        relu_mask, input_g, weight_g, bias_g, negative_slope,
    )


def batch_norm_backward_elemt_act_pool(grad_out, grad_out2, codes, input,
                                       mean, invstd, weight, bias, sum_dy,
                                       sum_dy_xmu, count, relu_mask,
                                       coefs=None,
                                       negative_slope: float = 0.0):
    """Second backward pass of the pooled layer: gathers the same gradient
    again and returns ``dx`` (full size)."""
    if input.is_cuda:
        return _require_hip().batch_norm_backward_elemt_act_pool(
            grad_out, grad_out2, codes, input, mean, invstd, weight, bias,
            sum_dy, sum_dy_xmu, count, relu_mask, coefs, negative_slope,
        )
    return _ref.batch_norm_backward_elemt_act_pool(
        grad_out, grad_out2, codes, input, mean, invstd, weight, bias,
        sum_dy, sum_dy_xmu, count, relu_mask, negative_slope,
    )


def batch_norm_elemt_act_(input, weight, bias, mean, invstd, act: bool,
                          coefs=None, negative_slope: float = 0.0):
    """In place: ``input <- act(input*scale + shift)``; returns ``input``.
    Bit-identical to ``batch_norm_elemt_act`` on a copy.  ``act`` needs
    ``negative_slope > 0`` (LeakyReLU); ``act=False`` is the identity.  The
    backward of a layer run this way works from the stored output:
    ``batch_norm_backward_reduce_inplace`` /
    ``batch_norm_backward_elemt_inplace``."""
    if input.is_cuda:
        _require_hip().batch_norm_elemt_act_(
            input, weight, bias, mean, invstd, act, coefs, negative_slope
        )
        return input
    return _ref.batch_norm_elemt_act_(
        input, weight, bias, mean, invstd, act, negative_slope
    )


def batch_norm_backward_reduce_inplace(grad_out, output, invstd, weight, bias,
                                       act: bool, input_g, weight_g, bias_g,
                                       coefs=None,
                                       negative_slope: float = 0.0):
    """First backward pass from the stored OUTPUT ``y`` of an in-place layer:
    the gate is ``sign(y)``, the pre-activation ``z = y > 0 ? y : y/slope``
    and ``x - mean = (z - bias)/scale``.  Returns ``(sum_dy, sum_dy_xmu,
    grad_weight, grad_bias)`` with the meaning (and, on the GPU, the one
    ``[2C]`` buffer) of ``batch_norm_backward_reduce_act``.  Requires
    ``weight*invstd != 0`` in every channel."""
    if output.is_cuda:
        return _require_hip().batch_norm_backward_reduce_inplace(
            grad_out, output, invstd, weight, bias, act, input_g, weight_g,
            bias_g, coefs, negative_slope,
        )
    return _ref.batch_norm_backward_reduce_inplace(
        grad_out, output, invstd, weight, bias, act, input_g, weight_g,
        bias_g, negative_slope,
    )


def batch_norm_backward_elemt_inplace(grad_out, output, mean, invstd, weight,
                                      bias, sum_dy, sum_dy_xmu, count,
                                      act: bool, coefs=None,
                                      negative_slope: float = 0.0):
    """Second backward pass from the stored output ``y``:
    ``dx = a*g + (b/scale)*z + (d - b*shift/scale)`` with ``g`` / ``z``
    recovered from ``y`` as in ``batch_norm_backward_reduce_inplace``."""
    if output.is_cuda:
        return _require_hip().batch_norm_backward_elemt_inplace(
            grad_out, output, mean, invstd, weight, bias, sum_dy, sum_dy_xmu,
            count, act, coefs, negative_slope,
        )
    return _ref.batch_norm_backward_elemt_inplace(
        grad_out, output, mean, invstd, weight, bias, sum_dy, sum_dy_xmu,
        count, act, negative_slope,
    )


def bn_frozen_coefs(running_mean, running_var, eps: float, weight, bias):
    """Packed fp32 [scale(C) | shift(C)] from FIXED running statistics in one
    launch: scale = weight*rsqrt(running_var+eps), shift = bias -
    running_mean*scale.  The buffer is what ``batch_norm_elemt_act(coefs=)``
    and ``batch_norm_frozen_backward_elemt`` consume."""
    if running_mean.is_cuda:
        return _require_hip().bn_frozen_coefs(
            running_mean, running_var, eps, weight, bias
        )
    return _ref.bn_frozen_coefs(running_mean, running_var, eps, weight, bias)


def batch_norm_frozen_backward_elemt(grad_out, input, residual, coefs,
                                     relu_mask: bool, want_input_grad: bool,
                                     want_res_grad: bool,
                                     negative_slope: float = 0.0,
                                     act: Optional[str] = None):
    """Backward of the frozen BN(+add)(+ReLU) epilogue, one elementwise pass:
    dx = scale*g, dres = g, g = grad_out*1[z>0] (LeakyReLU for a non-zero
    ``negative_slope``: g = negative_slope*grad_out where z <= 0;
    ``act="silu"``: g = grad_out*silu'(z)).  ``input``
    / ``residual`` are only needed for the gate (``relu_mask``); without it
    ``dres`` is ``grad_out`` itself.  Returns (dx-or-None, dres-or-None)."""
    if grad_out.is_cuda:
        dx, dres = _require_hip().batch_norm_frozen_backward_elemt(
            grad_out, input, residual, coefs, relu_mask, want_input_grad,
            want_res_grad, negative_slope,
            _act_name(relu_mask, negative_slope, act),
        )
        return (dx if want_input_grad else None,
                dres if want_res_grad else None)
    return _ref.batch_norm_frozen_backward_elemt(
        grad_out, input, residual, coefs, relu_mask, want_input_grad,
        want_res_grad, negative_slope, act,
    )


def conv1x1_stats(input: torch.Tensor, weight: torch.Tensor):
    """A 1x1, stride-1, unpadded, ungrouped, bias-free convolution as one
    MFMA GEMM kernel that also forms the statistics of the BatchNorm that
    follows it (docs/KERNEL_DESIGN.md "Conv + statistics").

    Returns ``(y, partials, nchunks)``: ``y`` channels-last ``[N, Cout, H,
    W]``, accumulated in fp32 and rounded to the input dtype once;
    ``partials`` the fp64 ``[Cout][nchunks][2]`` workspace of per-channel
    ``{sum y, sum y^2}`` over the rounded values, which
    ``batch_norm_stats_local_from_partials`` /
    ``batch_norm_stats_packed_from_partials`` finalize.

    Returns ``(None, None, 0)`` and launches nothing for what the kernel
    does not take: anything but a non-empty dense channels-last 4-D bf16 /
    half GPU input with a contiguous ``[Cout, Cin, 1, 1]`` weight of the same
    dtype, ``Cin`` and ``Cout`` multiples of 8 (``Cin <= 2304``) and 16-byte
    aligned pointers.  The caller then runs the convolution it has."""
    if not input.is_cuda or not weight.is_cuda:
        return None, None, 0
    y, partials, nchunks = _require_hip().conv1x1_stats(input, weight)
    if y is None:
        return None, None, 0
    return y, partials, int(nchunks)


def dwconv3x3_stats(input: torch.Tensor, weight: torch.Tensor,
                    stride: int = 1):
    """A depthwise 3x3 convolution (padding 1, dilation 1, ``stride`` 1 or 2
    in both dimensions, ``groups == Cin == Cout``, no bias) as one streaming
    kernel that also forms the statistics of the BatchNorm that follows it
    (docs/KERNEL_DESIGN.md "Depthwise conv + statistics").

    Returns ``(y, partials, nchunks)`` as ``conv1x1_stats`` does: ``y``
    channels-last ``[N, C, OH, OW]`` with ``OH = (H - 1) // stride + 1``,
    accumulated in fp32 (``kh`` then ``kw`` ascending) and rounded to the
    input dtype once; ``partials`` the fp64 ``[C][nchunks][2]`` workspace of
    ``{sum y, sum y^2}`` over the rounded values.

    Returns ``(None, None, 0)`` and launches nothing for what the kernel
    does not take: anything but a non-empty dense channels-last 4-D bf16 /
    half GPU input with a contiguous ``[C, 1, 3, 3]`` weight of the same
    dtype and device, ``C`` a multiple of 8, 16-byte aligned pointers and a
    stride of 1 or 2.  The caller then runs the convolution it has."""
    if not input.is_cuda or not weight.is_cuda:
        return None, None, 0
    y, partials, nchunks = _require_hip().dwconv3x3_stats(
        input, weight, int(stride))
    if y is None:
        return None, None, 0
    return y, partials, int(nchunks)


def dwconv3x3_backward(grad_y: torch.Tensor, input: torch.Tensor,
                       weight: torch.Tensor, stride: int = 1,
                       want_dx: bool = True, want_dw: bool = True):
    """Both gradients of the depthwise 3x3 convolution ``dwconv3x3_stats``
    computes, as streaming kernels of this project (docs/KERNEL_DESIGN.md
    "Depthwise conv gradients").

    Returns ``(dx, dw)``, each ``None`` where not wanted.  ``dx`` is
    channels-last like ``input``: per element the taps inside ``grad_y`` in
    fp32, ``grad_y`` rows then columns ascending into one accumulator, rounded
    to the input dtype once.  ``dw`` is a contiguous ``[C, 1, 3, 3]``: fp32
    products summed for at most 64 terms, then in fp64 through a
    deterministic two-stage reduction, rounded once.

    Returns ``(None, None)`` and launches nothing for what the kernels do not
    take: everything ``dwconv3x3_stats`` declines, and a ``grad_y`` that is
    not a dense channels-last ``[N, C, OH, OW]`` of the input's dtype and
    device at a 16-byte aligned address.  Always ``(None, None)`` for CPU
    tensors.  The caller then runs the convolution backward it has."""
    if not (input.is_cuda and weight.is_cuda and grad_y.is_cuda):
        return None, None
    dx, dw = _require_hip().dwconv3x3_backward(
        grad_y, input, weight, int(stride), bool(want_dx), bool(want_dw))
    return dx, dw


def dwconv5x5_stats(input: torch.Tensor, weight: torch.Tensor,
                    stride: int = 1):
    """``dwconv3x3_stats`` at kernel 5x5, padding 2 (docs/KERNEL_DESIGN.md
    "Depthwise 5x5"): the input tile goes through LDS once, each thread holds
    a strip of fp32 accumulators.  ``(y, partials, nchunks)`` with the same
    arithmetic rules (fp32, ``kh`` then ``kw`` ascending, rounded once,
    statistics of the rounded values), and ``(None, None, 0)`` with nothing
    launched for what ``dwconv3x3_stats`` declines, the weight being a
    contiguous ``[C, 1, 5, 5]``."""
    if not input.is_cuda or not weight.is_cuda:
        return None, None, 0
    y, partials, nchunks = _require_hip().dwconv5x5_stats(
        input, weight, int(stride))
    if y is None:
        return None, None, 0
    return y, partials, int(nchunks)


def dwconv5x5_backward(grad_y: torch.Tensor, input: torch.Tensor,
                       weight: torch.Tensor, stride: int = 1,
                       want_dx: bool = True, want_dw: bool = True):
    """``dwconv3x3_backward`` at kernel 5x5, padding 2: ``(dx, dw)``, each
    ``None`` where not wanted, ``dw`` a contiguous ``[C, 1, 5, 5]``, under the
    3x3 op's rules (``dx``: ``grad_y`` rows then columns ascending in fp32,
    rounded once; ``dw``: at most 64 fp32 terms, then fp64, deterministic,
    rounded once).  ``(None, None)`` with nothing launched for what the
    kernels do not take, and always for CPU tensors."""
    if not (input.is_cuda and weight.is_cuda and grad_y.is_cuda):
        return None, None
    dx, dw = _require_hip().dwconv5x5_backward(
        grad_y, input, weight, int(stride), bool(want_dx), bool(want_dw))
    return dx, dw


def se_squeeze(y: torch.Tensor, coefs: torch.Tensor, mean: torch.Tensor):
    """First forward stage of squeeze-excite after BN+SiLU
    (docs/KERNEL_DESIGN.md "Squeeze-excite").  With ``z = scale*y + shift``
    (``coefs = [scale | shift]``, fp32) and ``a = silu(z)``, one read of ``y``
    gives per image and channel ``S = sum a``, ``Q1 = sum silu'(z)`` and
    ``Q2 = sum silu'(z)*(y - mean)``: fp64 partials ``[N, chunks, C, 3]``,
    which ``se_gate`` finalizes.

    Returns ``None`` and launches nothing for a GPU tensor the streaming
    kernels do not take: anything but a non-empty dense channels-last 4-D
    bf16 / half tensor with ``C`` a multiple of 8 at a 16-byte aligned
    address.  CPU tensors run the plain-PyTorch reference."""
    if y.is_cuda:
        return _require_hip().se_squeeze(y, coefs, mean, None)
    return _ref.se_squeeze(y, coefs, mean)


def se_gate(partials: torch.Tensor, hw: int, w1, b1, w2, b2):
    """The excite MLP, one block per image: ``(s, hpre, g, Q)`` with
    ``s[N, C] = S / hw``, ``hpre[N, Cr] = W1 s + b1``, ``g[N, C] =
    sigmoid(W2 silu(hpre) + b2)`` and ``Q[N, C, 2] = {Q1, Q2}`` (sums), all
    fp32.  ``w1`` is ``[Cr, C]`` or ``[Cr, C, 1, 1]``, ``w2`` ``[C, Cr(, 1,
    1)]``; the four parameters share one dtype (fp32, bf16 or half) and all
    arithmetic is fp32.

    Returns ``(None, None, None, None)`` and launches nothing for GPU tensors
    the kernel does not take: anything but ``se_squeeze``'s fp64 partials and
    contiguous parameters of one dtype on one device with ``C <= 4096`` and
    ``1 <= Cr <= 1024``."""
    if partials.is_cuda:
        return _require_hip().se_gate(partials, int(hw), w1, b1, w2, b2)
    return _ref.se_gate(partials, int(hw), w1, b1, w2, b2)


def se_scale(y: torch.Tensor, coefs: torch.Tensor, g: torch.Tensor):
    """``out = silu(scale*y + shift) * g[n, c]``, rounded to ``y``'s dtype
    once.  ``None`` where ``se_squeeze`` declines."""
    if y.is_cuda:
        return _require_hip().se_scale(y, coefs, g)
    return _ref.se_scale(y, coefs, g)


def se_backward_reduce(grad_out, y, coefs, mean):
    """First backward stage: one read of ``(grad_out, y)`` gives per image
    and channel ``R = sum dout*a``, ``P1 = sum dout*silu'(z)`` and ``P2 = sum
    dout*silu'(z)*(y - mean)``, as partials laid out like ``se_squeeze``'s.
    ``None`` where ``se_squeeze`` declines or ``grad_out`` is not a dense
    channels-last twin of ``y`` at a 16-byte aligned address."""
    if y.is_cuda:
        return _require_hip().se_squeeze(y, coefs, mean, grad_out)
    return _ref.se_squeeze(y, coefs, mean, grad_out)


def se_gate_backward(partials, hw: int, g, hpre, w1, w2):
    """The excite MLP's backward, one block per image: ``(dpool, dz2, dz1,
    P)`` with ``dz2[N, C] = R*g*(1 - g)``, ``dz1[N, Cr] = (W2^T dz2) *
    silu'(hpre)``, ``dpool[N, C] = (W1^T dz1) / hw`` (the gradient reaching
    every pixel of ``a`` through the pool) and ``P[N, C, 2] = {P1, P2}``.
    Four ``None`` with nothing launched where ``se_gate`` declines or ``g`` /
    ``hpre`` are not its fp32 outputs."""
    if partials.is_cuda:
        return _require_hip().se_gate_backward(partials, int(hw), g, hpre,
                                               w1, w2)
    return _ref.se_gate_backward(partials, int(hw), g, hpre, w1, w2)


def se_backward_finalize(g, dpool, p, q, invstd, weight_g: bool,
                         bias_g: bool):
    """The BatchNorm backward's per-channel sums without a second pass over
    the activation: the gradient entering BN+SiLU is ``(dout*g + dpool) *
    silu'(z)``, so ``sum_dy = sum_n g*P1 + dpool*Q1`` and ``sum_dy_xmu =
    sum_n g*P2 + dpool*Q2`` (fp64, fixed order).  Returns ``(sum_dy,
    sum_dy_xmu, grad_weight, grad_bias)``; on the GPU the two sums are views
    of one ``[2C]`` buffer (one all_reduce).  Four ``None`` with nothing
    launched for GPU tensors that are not the contiguous fp32 tables of one
    device."""
    if g.is_cuda:
        sum_dy, sum_dy_xmu, gw, gb = _require_hip().se_bn_finalize_backward(
            g, dpool, p, q, invstd, bool(weight_g), bool(bias_g))
        return (sum_dy, sum_dy_xmu, gw if weight_g else None,
                gb if bias_g else None)
    return _ref.se_backward_finalize(g, dpool, p, q, invstd, weight_g, bias_g)


def se_param_backward(dz2, dz1, hpre, s, w1, w2, want_w1: bool = True,
                      want_b1: bool = True, want_w2: bool = True,
                      want_b2: bool = True):
    """The SE block's own gradients ``(dW1, db1, dW2, db2)``, shaped and typed
    like the parameters, ``None`` where not wanted: ``dW2 = dz2^T silu(hpre)``,
    ``db2 = sum_n dz2``, ``dW1 = dz1^T s``, ``db1 = sum_n dz1``; fp64 over
    ``n`` ascending, rounded once.  Four ``None`` with nothing launched for
    GPU tensors the kernel does not take (``se_gate``'s rules for the
    weights, contiguous fp32 tables)."""
    wants = (bool(want_w1), bool(want_b1), bool(want_w2), bool(want_b2))
    if dz2.is_cuda:
        out = _require_hip().se_param_backward(dz2, dz1, hpre, s, w1, w2,
                                               *wants)
        return tuple(t if w else None for t, w in zip(out, wants))
    return _ref.se_param_backward(dz2, dz1, hpre, s, w1, w2, *wants)


def se_backward_elemt(grad_out, y, coefs, g, dpool, mean, invstd, weight,
                      sum_dy, sum_dy_xmu, count):
    """Last backward stage: ``dy = a*gz + b*y + d`` with ``gz = (grad_out*g +
    dpool) * silu'(z)`` recomputed per element and the coefficients of
    ``batch_norm_backward_elemt`` from ``sum_dy`` / ``sum_dy_xmu`` (summed
    over the ranks) and ``count``; rounded once.  ``weight`` is the
    BatchNorm's, fp32 or None.  ``None`` where ``se_backward_reduce``
    declines."""
    if y.is_cuda:
        return _require_hip().se_backward_elemt(
            grad_out, y, coefs, g, dpool, mean, invstd, weight, sum_dy,
            sum_dy_xmu, count)
    return _ref.se_backward_elemt(grad_out, y, coefs, g, dpool, mean, invstd,
                                  weight, sum_dy, sum_dy_xmu, count)


def batch_norm_stats_local_from_partials(partials, nchunks: int, count: int,
                                         eps: float, running_mean,
                                         running_var, momentum: float,
                                         weight, bias, want_coefs: bool):
    """``batch_norm_stats_local`` for statistics whose partial stage is done
    (``conv1x1_stats``): the finalize kernel alone, with the running-stat
    update and the ``[scale | shift]`` coefs.  ``count`` is the number of
    elements per channel.  Returns ``(mean, invstd, count[1], coefs|None)``."""
    mean, invstd, count_sum, coefs = (
        _require_hip().batch_norm_stats_local_from_partials(
            partials, nchunks, count, eps, running_mean, running_var,
            momentum, weight, bias, want_coefs,
        )
    )
    return mean, invstd, count_sum, (coefs if want_coefs else None)


def batch_norm_stats_packed_from_partials(partials, nchunks: int, count: int,
                                          eps: float, out: torch.Tensor):
    """``batch_norm_stats_packed`` from finished partials: writes
    ``[mean(C) | invstd(C) | count(1)]`` into ``out``."""
    _require_hip().batch_norm_stats_packed_from_partials(
        partials, nchunks, count, eps, out
    )
    return out


def batch_norm_stats_local_grouped(inputs, eps: float, running_mean,
                                   running_var, momentum: float, weight,
                                   bias):
    """Grouped BN (docs/KERNEL_DESIGN.md "Grouped BN"): the training
    statistics of S tensors that share one BatchNorm, each tensor
    ("segment") with its own, in one partial and one finalize launch.

    Returns ``(mean[S, C], invstd[S, C], count[S], coefs[S, 2C])``, ``coefs``
    holding each segment's ``[scale | shift]``.  The running statistics
    receive S successive momentum updates in segment order, each with that
    segment's unbiased variance: what S module calls leave.

    GPU only, and only what ``launch_plan("stats_grouped", ...)`` does not
    call ``"ineligible"``; weight, bias and running statistics fp32 or None."""
    return _require_hip().batch_norm_stats_local_grouped(
        list(inputs), eps, running_mean, running_var, momentum, weight, bias
    )


def batch_norm_stats_packed_grouped(inputs, eps: float, out: torch.Tensor):
    """The group's message for ONE all_gather: per segment ``[mean(C) |
    invstd(C) | count(1)]`` written into ``out`` (fp32 ``[S, 2C+1]``).  A
    group whose segments are all empty zero-fills ``out`` without a kernel
    of this project's."""
    _require_hip().batch_norm_stats_packed_grouped(list(inputs), eps, out)
    return out


def batch_norm_gather_stats_packed_grouped(packed_all, running_mean,
                                           running_var, momentum: float,
                                           eps: float, weight, bias):
    """Combine ``packed_all[world, S, 2C+1]`` per segment (count-weighted,
    zero-count ranks masked in the kernel), apply the S running updates in
    segment order and emit the coefs; returns what
    ``batch_norm_stats_local_grouped`` returns."""
    return _require_hip().batch_norm_gather_stats_packed_grouped(
        packed_all, running_mean, running_var, momentum, eps, weight, bias
    )


def batch_norm_elemt_act_grouped(inputs, coefs, relu: bool):
    """``[act(x_s * scale_s + shift_s) for s]`` in one launch; ``act`` is
    ReLU or the identity.  The outputs are views of one allocation."""
    return _require_hip().batch_norm_elemt_act_grouped(
        list(inputs), coefs, relu
    )


def batch_norm_backward_reduce_act_grouped(grad_outs, inputs, mean, invstd,
                                           coefs, relu: bool, weight_g: bool,
                                           bias_g: bool):
    """First backward pass of the group, one partial and one finalize
    launch: ``(sums[S, 2C], grad_weight[C] | None, grad_bias[C] | None)``
    with ``sums[s] = [sum_dy | sum_dy_xmu]`` of segment s (the buffer of the
    group's one all_reduce) and the affine gradients summed over the
    segments in ascending order.  The ReLU gate is recomputed from the
    inputs and ``coefs``."""
    sums, gw, gb = _require_hip().batch_norm_backward_reduce_act_grouped(
        list(grad_outs), list(inputs), mean, invstd, coefs, relu, weight_g,
        bias_g,
    )
    return sums, (gw if weight_g else None), (gb if bias_g else None)


def batch_norm_backward_elemt_act_grouped(grad_outs, inputs, mean, invstd,
                                          coefs, sums, count, relu: bool):
    """Second backward pass of the group in one launch: ``[dx_s]`` from
    ``sums[s]`` (summed over the ranks) and the total ``count[s]``."""
    return _require_hip().batch_norm_backward_elemt_act_grouped(
        list(grad_outs), list(inputs), mean, invstd, coefs, sums, count,
        relu,
    )


_GROUPED_KINDS = ("stats_grouped", "elemt_grouped", "bwd_reduce_grouped",
                  "bwd_elemt_grouped")


def launch_plan(kind: str, input: torch.Tensor, others=(), coefs=None) -> dict:
    """What a GPU op WOULD launch for these tensors — host-only, launches
    nothing.  The numbers come from the same host code the ops launch with.

    ``kind`` / tensors (pass only what the op itself would dereference):
      ``"stats"``             input = x
      ``"bwd_reduce"``        input = x, others = (grad_out, residual, gm_out,
                                                   grad_out2[, gate])
      ``"elemt"``             input = x, others = (residual[, gate]), coefs
      ``"bwd_elemt"``         input = x, others = (grad_out, residual), coefs
      ``"frozen_bwd_elemt"``  input = grad_out, others = (x, residual), coefs
      ``"fused_local"``       input = x, others = (residual,)
      ``"elemt_inplace"``       input = x, coefs
      ``"bwd_reduce_inplace"``  input = y, others = (grad_out,)
      ``"bwd_elemt_inplace"``   input = y, others = (grad_out,)
      ``"elemt_pool"``        input = x, others = (pooled, codes), coefs
      ``"bwd_reduce_pool"``   input = x, others = (grad_out, grad_out2, codes)
      ``"bwd_elemt_pool"``    input = x, others = (grad_out, grad_out2,
                                                   codes), coefs
      ``"elemt_dual"``        input = x, others = (x2[, coefs2]), coefs
      ``"bwd_reduce_dual"``   input = x, others = (grad_out, x2, gm_out,
                                                   grad_out2, gate)
      ``"bwd_elemt_dual"``    input = x, others = (gm, x2)
      ``"conv1x1_stats"``     input = x, others = (weight,)
    ``conv1x1_stats`` reports path ``"mfma"`` with ``nchunks``, ``row_tile``
    (rows of a tile), ``slab`` (output channels of a block), ``nslabs``,
    ``tiles_per_block`` (most row tiles one block visits), ``k_trips`` and
    ``lds_bytes``, or ``"ineligible"`` where the op declines (the device is
    not looked at: the plan of a CPU tensor is that of its GPU copy).
      ``"dwconv3x3_stats"``   input = x, others = (weight,)   (stride 1)
      ``"dwconv3x3s2_stats"`` input = x, others = (weight,)   (stride 2)
    They report path ``"dwconv"`` with ``V``, ``lpr`` (lanes across the
    channels), ``ctiles``, ``strip`` (output columns of a work item),
    ``items`` (work items), ``chunk_items``, ``nchunks``, ``trips`` (the most
    items one thread visits), ``flush_every`` and ``finalize_trips``, or
    ``"ineligible"`` where ``dwconv3x3_stats`` declines.
      ``"dwconv3x3_dgrad"`` / ``"dwconv3x3_wgrad"``      (stride 1)
      ``"dwconv3x3s2_dgrad"`` / ``"dwconv3x3s2_wgrad"``  (stride 2)
                              input = x, others = (weight, grad_y)
    The launches of ``dwconv3x3_backward``: path ``"dwconv"`` with the same
    numbers (``items`` are strips of ``dx`` for dgrad and of ``grad_y`` for
    wgrad, whose ``trips * strip <= flush_every`` holds by construction;
    ``finalize_trips`` for wgrad alone), or ``"ineligible"`` where the op
    declines.
      ``"dwconv5x5_stats"`` / ``"dwconv5x5_dgrad"`` / ``"dwconv5x5_wgrad"``
      ``"dwconv5x5s2_stats"`` / ``"dwconv5x5s2_dgrad"`` / ``"dwconv5x5s2_wgrad"``
    The 5x5 ops' launches, tensors as for their 3x3 namesakes: path
    ``"dwconv"`` with ``V``, ``lpr``, ``ctiles``, ``tile_h`` / ``tile_w`` (a
    work item is a tile of that many pixels of one image), ``strip``,
    ``items``, ``chunk_items``, ``nchunks``, ``trips`` (tiles a block visits;
    for wgrad the strips of one tile a thread visits before its fp32 sums
    move to fp64, so ``trips * strip <= flush_every``), ``flush_every``,
    ``lds_bytes`` and, but for dgrad, ``finalize_trips``; or ``"ineligible"``.
      ``"se_squeeze"`` / ``"se_scale"``        input = y
      ``"se_bwd_reduce"`` / ``"se_bwd_elemt"``  input = y, others = (grad_out,)
      ``"se_gate"`` / ``"se_gate_bwd"``         input = y, others = (w1, w2)
    The squeeze-excite ops' launches: path ``"se"`` (``"se_gate"`` for the
    gate kinds, which add ``Cr`` and ``lds_bytes``) with ``V``, ``lpr``,
    ``ctiles``, ``chunk_rows``, ``chunks_per_image`` (blocks per image and
    channel tile), ``trips``, ``flush_every`` and ``finalize_trips`` (the
    trips of the per-channel sum over the images), or ``"ineligible"``
    where the ops decline; empty and fp32 tensors are declined, not raised
    for.
    ``None`` entries of ``others`` are absent tensors.  The dual kinds
    report path ``"nhwc"`` with their single counterparts' numbers plus
    ``dual: True``, or ``"ineligible"`` where the dual kernels decline.

    Grouped BN, ``input`` the first segment and ``others`` the rest:
      ``"stats_grouped"``       input = x_0, others = (x_1, .., x_{S-1})
      ``"elemt_grouped"``       the same
      ``"bwd_reduce_grouped"``  others = (x_1, .., x_{S-1}, dy_0, .., dy_{S-1})
      ``"bwd_elemt_grouped"``   the same
    They report path ``"nhwc"`` with ``S`` and ``V``, or ``"ineligible"``
    where the grouped ops decline (S > 8, another layout, C not a multiple
    of the 16-byte pack, a pointer off 16-byte alignment, mixed dtypes or
    channel counts; the device is not looked at).  The reduction kinds add
    the group's ``chunk_rows``, ``lpr``, ``ctiles``, ``total_chunks``,
    ``trips``, ``flush_every``, ``finalize_trips`` and per segment the lists
    ``nchunks`` and ``first_block``; the elementwise kinds ``grid``,
    ``packs``, ``trips``, ``multi_trip`` and the lists ``blocks`` and
    ``first_block``.

    Returns a dict with ``path`` (``"nchw_vec"``, ``"nchw_flat"``, ``"nhwc"``,
    ``"small_plane"``, or ``"ineligible"`` for ``fused_local``), ``V`` and
    ``trips`` (the most loop iterations any one thread makes); reductions add
    ``nchunks``, ``flush_every``, ``finalize_trips`` and their chunk sizes,
    elementwise ops add ``grid``, ``packs`` and ``multi_trip``.  When the
    tuple has the trailing ``gate`` entry (a gate-bit tensor or None; never
    counted for alignment), ``gate`` tells whether the gate-bit kernel would
    run, the activation taken as on."""
    path, numbers = _require_hip().launch_plan(kind, input, list(others), coefs)
    plan = dict(numbers)
    plan["path"] = path
    if kind in _GROUPED_KINDS and path != "ineligible":
        # per-segment numbers arrive as name_<s>: fold them into lists
        for name in ("nchunks", "first_block", "blocks"):
            if f"{name}_0" in plan:
                plan[name] = [plan.pop(f"{name}_{s}")
                              for s in range(plan["S"])]
    for flag in ("multi_trip", "gate", "dual"):
        if flag in plan:
            plan[flag] = bool(plan[flag])
    return plan


__all__ = [
    "hip_available",
    "launch_plan",
    "gate_bits_empty",
    "conv1x1_stats",
    "dwconv3x3_stats",
    "dwconv3x3_backward",
    "dwconv5x5_stats",
    "dwconv5x5_backward",
    "se_squeeze",
    "se_gate",
    "se_scale",
    "se_backward_reduce",
    "se_gate_backward",
    "se_backward_finalize",
    "se_param_backward",
    "se_backward_elemt",
    "batch_norm_stats_local_from_partials",
    "batch_norm_stats_packed_from_partials",
    "batch_norm_stats_local_grouped",
    "batch_norm_stats_packed_grouped",
    "batch_norm_gather_stats_packed_grouped",
    "batch_norm_elemt_act_grouped",
    "batch_norm_backward_reduce_act_grouped",
    "batch_norm_backward_elemt_act_grouped",
    "bn_frozen_coefs",
    "batch_norm_frozen_backward_elemt",
    "batch_norm_elemt_act_dual",
    "batch_norm_backward_elemt_dual",
    "batch_norm_elemt_act_pool",
    "batch_norm_backward_reduce_act_pool",
    "batch_norm_backward_elemt_act_pool",
    "batch_norm_elemt_act_",
    "batch_norm_backward_reduce_inplace",
    "batch_norm_backward_elemt_inplace",
    "batch_norm_elemt_act",
    "bn_make_coefs",
    "batch_norm_backward_reduce_act",
    "batch_norm_backward_elemt_act",
    "batch_norm_stats",
    "batch_norm_stats_packed",
    "batch_norm_gather_stats_with_counts",
    "batch_norm_gather_stats_packed",
    "batch_norm_elemt",
    "batch_norm_backward_reduce",
    "batch_norm_backward_elemt",
]
