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


def gate_bits_empty(input: torch.Tensor) -> torch.Tensor:
    """An unwritten gate-bit tensor for ``input``: ``ceil(numel/8)`` uint8."""
    return torch.empty((input.numel() + 7) // 8, dtype=torch.uint8,
                       device=input.device)


def batch_norm_elemt_act(input, residual, weight, bias, mean, invstd,
                         relu: bool, coefs=None, negative_slope: float = 0.0,
                         gate_out=None):
    """y = act(x*scale + shift [+ residual]); ``relu`` turns the activation
    on and ``negative_slope`` (only consulted then) makes it a LeakyReLU.

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
            negative_slope, gate_out,
        )
        return y if gate_out is None else (y, gate_out if wrote else None)
    y = _ref.batch_norm_elemt_act(
        input, residual, weight, bias, mean, invstd, relu, negative_slope
    )
    return y if gate_out is None else (y, None)


def batch_norm_backward_reduce_act(grad_out, input, residual, mean, invstd,
                                   weight, bias, relu_mask, input_g, weight_g,
                                   bias_g, coefs=None, gm_out=None,
                                   negative_slope: float = 0.0,
                                   grad_out2=None, gate=None, *, dual=None):
    """First pass of the fused BN backward.  ``grad_out2`` is the second
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
            grad_out2, gate,
        )
    if gate is not None:
        raise ValueError("gate bits exist on the GPU path only")
    return _ref.batch_norm_backward_reduce_act(
        grad_out, input, residual, mean, invstd, weight, bias, relu_mask,
        input_g, weight_g, bias_g, gm_out, negative_slope, grad_out2,
    )


def batch_norm_backward_elemt_act(grad_out, input, residual, mean, invstd,
                                  weight, bias, sum_dy, sum_dy_xmu, count,
                                  relu_mask, want_res_grad, coefs=None,
                                  negative_slope: float = 0.0):
    if input.is_cuda:
        dx, dres = _require_hip().batch_norm_backward_elemt_act(
            grad_out, input, residual, mean, invstd, weight, bias, sum_dy,
            sum_dy_xmu, count, relu_mask, want_res_grad, coefs,
            negative_slope,
        )
        return dx, (dres if want_res_grad else None)
    return _ref.batch_norm_backward_elemt_act(
        grad_out, input, residual, mean, invstd, weight, bias, sum_dy,
        sum_dy_xmu, count, relu_mask, want_res_grad, negative_slope,
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
                                     negative_slope: float = 0.0):
    """Backward of the frozen BN(+add)(+ReLU) epilogue, one elementwise pass:
    dx = scale*g, dres = g, g = grad_out*1[z>0] (LeakyReLU for a non-zero
    ``negative_slope``: g = negative_slope*grad_out where z <= 0).  ``input``
    / ``residual`` are only needed for the gate (``relu_mask``); without it
    ``dres`` is ``grad_out`` itself.  Returns (dx-or-None, dres-or-None)."""
    if grad_out.is_cuda:
        dx, dres = _require_hip().batch_norm_frozen_backward_elemt(
            grad_out, input, residual, coefs, relu_mask, want_input_grad,
            want_res_grad, negative_slope,
        )
        return (dx if want_input_grad else None,
                dres if want_res_grad else None)
    return _ref.batch_norm_frozen_backward_elemt(
        grad_out, input, residual, coefs, relu_mask, want_input_grad,
        want_res_grad, negative_slope,
    )


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
    ``None`` entries of ``others`` are absent tensors.  The dual kinds
    report path ``"nhwc"`` with their single counterparts' numbers plus
    ``dual: True``, or ``"ineligible"`` where the dual kernels decline.

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
    for flag in ("multi_trip", "gate", "dual"):
        if flag in plan:
            plan[flag] = bool(plan[flag])
    return plan


__all__ = [
    "hip_available",
    "launch_plan",
    "gate_bits_empty",
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
