"""Fused SyncBatchNorm(+residual add)(+ReLU | LeakyReLU) — the msbn
epilogue-fusion path.

Mathematically identical to ``relu(bn(x) + residual)`` (or
``leaky_relu(bn(x) + residual, negative_slope)``) composed from separate
modules, but executed as ONE elementwise kernel forward and mask-recomputing
kernels backward (no clamp / add / threshold_backward kernels, no stored mask,
~3x fewer full-tensor round trips on the BN backward — see
profiles/r01_single_gpu.md for the measured eager-kernel cost this removes).
A layer with a residual may instead keep one bit per element for its gate
(``gate_bits``, profiles/r08_gate_bits.md): an eighth of a byte read back
where the backward re-read the whole residual.

``SyncBatchNormAct2d`` is used directly by the fused model variants
(msbn.models.resnet{18,50}(fused=True)); ``convert_sync_batchnorm`` leaves it
alone (it already IS a SyncBatchNorm subclass).
"""

from typing import Optional

import torch
import torch.distributed as dist

from msbn import ops
from msbn.nn.batchnorm import (SyncBatchNorm, _check_negative_slope,
                               _momentum_factor, _running_stats_forward)
from msbn.nn.functions import (_combined_view, _contig, _force_sync,
                               _match_layout, compute_sync_stats)


class SyncBatchNormActFunction(torch.autograd.Function):
    @staticmethod
    def forward(
        ctx,
        input: torch.Tensor,
        residual: Optional[torch.Tensor],
        weight: Optional[torch.Tensor],
        bias: Optional[torch.Tensor],
        running_mean: Optional[torch.Tensor],
        running_var: Optional[torch.Tensor],
        eps: float,
        momentum: float,
        process_group,
        world_size: int,
        relu: bool,
        negative_slope: float = 0.0,
        fork: bool = False,
        gate_bits: bool = False,
    ):
        """``fork=True`` returns the output twice — ``(y, y.detach())``, two
        tensor objects over one storage, no copy — for a result that feeds
        two consumers (a residual block's conv1 and its skip path).  Autograd
        sums gradients per output edge, so two outputs are what lets
        ``backward`` receive the two gradients UNSUMMED and read both inside
        the reduce kernel instead of paying for an eager add (read 2A, write
        1A) whose only reader is that kernel.

        ``gate_bits=True``: an activated layer whose residual needs its
        gradient keeps the activation's branch as one bit per element,
        stored by the forward kernel, instead of the residual tensor: the
        backward reduce reads numel/8 bytes where it read the residual, and
        the residual is not saved.  Only the two-stage GPU kernels do this,
        and only when the forward kernel reports that it stored the bits;
        every other case saves the residual as before.  Same results."""
        ctx.fork = fork
        ctx.gate_bits = gate_bits
        y = SyncBatchNormActFunction._forward(
            ctx, input, residual, weight, bias, running_mean, running_var,
            eps, momentum, process_group, world_size, relu, negative_slope,
        )
        if not fork:
            return y
        # an unused output then arrives as None, not as a full-size zero fill
        ctx.set_materialize_grads(False)
        return y, y.detach()

    @staticmethod
    def _forward(ctx, input, residual, weight, bias, running_mean,
                 running_var, eps, momentum, process_group, world_size, relu,
                 negative_slope):
        ctx.negative_slope = negative_slope
        ctx.has_res = residual is not None
        ctx.has_gate = False
        input = _contig(input)
        if residual is not None:
            residual = _match_layout(residual, input)
        if weight is not None:
            weight = weight.contiguous()
        if bias is not None:
            bias = bias.contiguous()

        use_sync = world_size > 1 or (
            process_group is not None and _force_sync()
        )
        if (
            not use_sync
            and input.numel() > 0
            and (residual is None or residual.is_contiguous())
            and ops.bn_fused_local_eligible(
                input, weight, bias, running_mean, running_var
            )
        ):
            # single-launch small-plane path: stats + running update +
            # normalize(+res)(+relu) in ONE kernel (K10-family)
            y, mean, invstd, count_sum, coefs = ops.batch_norm_fwd_fused_local(
                input, residual, weight, bias, eps, momentum,
                running_mean, running_var, relu, negative_slope,
            )
            ctx.save_for_backward(input, residual, weight, bias, mean,
                                  invstd, count_sum, coefs)
            ctx.has_coefs = True
            ctx.local_fused = True
            ctx.relu = relu
            ctx.process_group = process_group
            ctx.world_size = world_size
            return y
        ctx.local_fused = False

        # coefs ([scale|shift]) are emitted by the finalize/gather kernel in
        # the same launch and reused by forward elemt AND the two
        # mask-recomputing backward kernels.
        mean, invstd, count_sum, coefs = compute_sync_stats(
            input, eps, momentum, running_mean, running_var,
            process_group, world_size, weight, bias, want_coefs=True,
        )
        ctx.has_coefs = coefs is not None
        ctx.relu = relu
        ctx.process_group = process_group
        ctx.world_size = world_size
        ctx.use_sync = use_sync
        # Gate bits: asked for only where backward is certain to write gm
        # (use_gm there: an activation, and a residual that needs its
        # gradient), and kept only if the kernel stored them.
        gate = None
        if input.numel() == 0:
            y = torch.empty_like(input)
        elif (ctx.gate_bits and relu and residual is not None
                and ctx.needs_input_grad[1] and input.is_cuda):
            y, gate = ops.batch_norm_elemt_act(
                input, residual, weight, bias, mean, invstd, relu, coefs,
                negative_slope, ops.gate_bits_empty(input),
            )
        else:
            y = ops.batch_norm_elemt_act(
                input, residual, weight, bias, mean, invstd, relu, coefs,
                negative_slope,
            )
        ctx.has_gate = gate is not None
        saved = (input, None if ctx.has_gate else residual, weight, bias,
                 mean, invstd, count_sum)
        if ctx.has_coefs:
            saved += (coefs,)
        if ctx.has_gate:
            saved += (gate,)
        ctx.save_for_backward(*saved)
        return y

    @staticmethod
    def backward(ctx, grad_output, grad_skip=None):
        if grad_output is None:  # fork with only the second output used
            grad_output, grad_skip = grad_skip, None
        if grad_output is None:
            return (None,) * 14
        saved = ctx.saved_tensors
        input, residual, weight, bias, mean, invstd, count_sum = saved[:7]
        coefs = saved[7] if ctx.has_coefs else None
        # gate bits stand in for the residual, which was then not saved
        gate = saved[-1] if ctx.has_gate else None
        has_res = ctx.has_res
        # Both gradients of a forked output: the two-stage GPU path hands
        # them to the reduce kernel unsummed (grad_out2); every other path
        # (small-plane kernel, CPU, empty-input rank) starts with the eager
        # add autograd itself would have run.
        fold = (
            grad_skip is not None and input.is_cuda and input.numel() > 0
            and not getattr(ctx, "local_fused", False)
        )
        # The fold needs gm (below).  gm holds the gated gradient rounded to
        # the activation dtype: exact for none / relu (the gate passes or
        # zeroes a value that already is one), but slope*g is not, so a leaky
        # layer that would not have materialized gm anyway keeps the eager
        # add and its fp32 gate.
        if fold and ctx.relu and ctx.negative_slope != 0.0 and not (
            has_res and ctx.needs_input_grad[1]
        ):
            fold = False
        if grad_skip is not None and not fold:
            grad_output = grad_output + grad_skip
            grad_skip = None
        grad_output = _match_layout(grad_output, input)
        if fold:
            grad_skip = _match_layout(grad_skip, input)
        relu = ctx.relu
        slope = ctx.negative_slope
        process_group = ctx.process_group
        world_size = ctx.world_size
        need_input_g = ctx.needs_input_grad[0]
        need_res_g = has_res and ctx.needs_input_grad[1]
        need_weight_g = weight is not None and ctx.needs_input_grad[2]
        need_bias_g = bias is not None and ctx.needs_input_grad[3]

        C = int(input.shape[1])

        if getattr(ctx, "local_fused", False) and input.numel() > 0:
            # single-launch backward (mask recompute + reduce + coefs + dx
            # (+dres) in one kernel)
            grad_input, grad_weight, grad_bias, grad_res = (
                ops.batch_norm_bwd_fused_local(
                    grad_output, input, residual, mean, invstd, weight,
                    coefs, relu, need_res_g, need_weight_g, need_bias_g,
                    slope,
                )
            )
            return (
                grad_input if need_input_g else None,
                grad_res if need_res_g else None,
                grad_weight if need_weight_g else None,
                grad_bias if need_bias_g else None,
                None, None, None, None, None, None, None, None, None, None,
            )

        # Masked-grad materialization: when the residual branch needs its
        # gradient, the reduce pass writes gm = dy*1[z>0] (leaky: slope*dy
        # where z<=0) once; the elemt pass then reads gm instead of
        # (dy, residual) and gm itself IS the residual gradient -> one fewer
        # full-tensor read+write (8A -> 7A).
        # With both fork gradients (fold) gm is always written: the reduce
        # kernel is the only place their sum exists, and the elemt pass must
        # not read dy / dy2 again.
        use_gm = fold or (
            relu and has_res and need_res_g and input.is_cuda
            and input.numel() > 0
        )
        use_sync = getattr(ctx, "use_sync", world_size > 1)
        if input.numel() == 0:
            # empty-input rank (join): contribute zeros, keep peers unblocked
            if use_sync and (need_input_g or need_res_g):
                combined = torch.zeros(2 * C, dtype=torch.float32,
                                       device=grad_output.device)
                from msbn.utils import debug as _dbg
                if _dbg.enabled():  # peers verify; skipping would hang them
                    _dbg.verify_collective("syncbn.bwd.all_reduce", combined,
                                           process_group)
                dist.all_reduce(combined, dist.ReduceOp.SUM,
                                group=process_group)
            zg = torch.empty_like(grad_output)
            return (
                zg if need_input_g else None,
                torch.empty_like(grad_output) if need_res_g else None,
                torch.zeros_like(weight) if need_weight_g else None,
                torch.zeros_like(bias) if need_bias_g else None,
                None, None, None, None, None, None, None, None, None, None,
            )
        gm = torch.empty_like(grad_output) if use_gm else None
        if gate is not None:
            # the forward asked for bits only where use_gm was certain
            sum_dy, sum_dy_xmu, grad_weight, grad_bias = (
                ops.batch_norm_backward_reduce_act(
                    grad_output, input, None, mean, invstd, weight, bias,
                    relu, need_input_g, need_weight_g, need_bias_g, coefs, gm,
                    slope, grad_skip, gate=gate,
                )
            )
        else:
            sum_dy, sum_dy_xmu, grad_weight, grad_bias = (
                ops.batch_norm_backward_reduce_act(
                    grad_output, input, residual, mean, invstd, weight, bias,
                    relu, need_input_g, need_weight_g, need_bias_g, coefs, gm,
                    slope, grad_skip,
                )
            )
        grad_input = grad_res = None
        if need_input_g or need_res_g:
            if use_sync:
                combined, copied = _combined_view(sum_dy, sum_dy_xmu, C)
                from msbn.utils import debug as _dbg
                if _dbg.enabled():
                    _dbg.verify_collective("syncbn.bwd.all_reduce",
                                           combined, process_group)
                dist.all_reduce(combined, dist.ReduceOp.SUM, group=process_group)
                from msbn.utils.logging import comm_log
                comm_log.record("all_reduce", combined.numel() * 4,
                                f"syncbn bwd C={C}")
                if copied:
                    sum_dy, sum_dy_xmu = combined[:C], combined[C:]
            if use_gm:
                grad_input, _ = ops.batch_norm_backward_elemt_act(
                    gm, input, None, mean, invstd, weight, bias,
                    sum_dy, sum_dy_xmu, count_sum, False, False, coefs,
                )
                grad_res = gm if need_res_g else None
            else:
                grad_input, grad_res = ops.batch_norm_backward_elemt_act(
                    grad_output, input, residual, mean, invstd, weight, bias,
                    sum_dy, sum_dy_xmu, count_sum, relu, need_res_g, coefs,
                    slope,
                )
        return (
            grad_input if need_input_g else None,
            grad_res,
            grad_weight if need_weight_g else None,
            grad_bias if need_bias_g else None,
            None, None, None, None, None, None, None, None, None, None,
        )


class SyncBatchNormActPoolFunction(torch.autograd.Function):
    """``max_pool2d(act(bn(x)), 3, 2, 1)`` as one layer (the ResNet stem).

    The forward reads x once and writes the pooled output and one byte per
    pooled element (the window code); the full-size activation and the pool's
    int64 indices never exist.  The backward kernels gather each x element's
    gradient from the pooled gradient(s) through the codes, so neither the
    full-size pooled gradient nor (with ``fork``) the eager sum of the two
    consumers' gradients is materialised.  Saved for backward: x, the codes
    and per-channel vectors.  Statistics, their sync and the running update
    are those of SyncBatchNormActFunction; always the two-stage kernels.
    Results are bit-identical to the composition.  Callers check
    eligibility (``stem_pool_eligible``)."""

    @staticmethod
    def forward(
        ctx,
        input: torch.Tensor,
        weight: Optional[torch.Tensor],
        bias: Optional[torch.Tensor],
        running_mean: Optional[torch.Tensor],
        running_var: Optional[torch.Tensor],
        eps: float,
        momentum: float,
        process_group,
        world_size: int,
        relu: bool,
        negative_slope: float = 0.0,
        fork: bool = False,
    ):
        if weight is not None:
            weight = weight.contiguous()
        if bias is not None:
            bias = bias.contiguous()
        use_sync = world_size > 1 or (
            process_group is not None and _force_sync()
        )
        mean, invstd, count_sum, coefs = compute_sync_stats(
            input, eps, momentum, running_mean, running_var,
            process_group, world_size, weight, bias, want_coefs=True,
        )
        pooled, codes = ops.batch_norm_elemt_act_pool(
            input, weight, bias, mean, invstd, relu, coefs, negative_slope
        )
        ctx.has_coefs = coefs is not None
        saved = (input, codes, weight, bias, mean, invstd, count_sum)
        ctx.save_for_backward(*(saved + ((coefs,) if ctx.has_coefs else ())))
        ctx.relu = relu
        ctx.negative_slope = negative_slope
        ctx.process_group = process_group
        ctx.use_sync = use_sync
        if not fork:
            return pooled
        # an unused output then arrives as None, not as a zero fill
        ctx.set_materialize_grads(False)
        return pooled, pooled.detach()

    @staticmethod
    def backward(ctx, grad_output, grad_skip=None):
        if grad_output is None:  # fork with only the second output used
            grad_output, grad_skip = grad_skip, None
        if grad_output is None:
            return (None,) * 12
        saved = ctx.saved_tensors
        input, codes, weight, bias, mean, invstd, count_sum = saved[:7]
        coefs = saved[7] if ctx.has_coefs else None
        grad_output = _match_layout(grad_output, codes)
        if grad_skip is not None:
            grad_skip = _match_layout(grad_skip, codes)
        relu, slope = ctx.relu, ctx.negative_slope
        process_group = ctx.process_group
        need_input_g = ctx.needs_input_grad[0]
        need_weight_g = weight is not None and ctx.needs_input_grad[1]
        need_bias_g = bias is not None and ctx.needs_input_grad[2]
        C = int(input.shape[1])

        sum_dy, sum_dy_xmu, grad_weight, grad_bias = (
            ops.batch_norm_backward_reduce_act_pool(
                grad_output, grad_skip, codes, input, mean, invstd, weight,
                bias, relu, need_input_g, need_weight_g, need_bias_g, coefs,
                slope,
            )
        )
        grad_input = None
        if need_input_g:
            if ctx.use_sync:
                combined, copied = _combined_view(sum_dy, sum_dy_xmu, C)
                from msbn.utils import debug as _dbg
                if _dbg.enabled():
                    _dbg.verify_collective("syncbn.bwd.all_reduce",
                                           combined, process_group)
                dist.all_reduce(combined, dist.ReduceOp.SUM,
                                group=process_group)
                from msbn.utils.logging import comm_log
                comm_log.record("all_reduce", combined.numel() * 4,
                                f"syncbn bwd C={C}")
                if copied:
                    sum_dy, sum_dy_xmu = combined[:C], combined[C:]
            grad_input = ops.batch_norm_backward_elemt_act_pool(
                grad_output, grad_skip, codes, input, mean, invstd, weight,
                bias, sum_dy, sum_dy_xmu, count_sum, relu, coefs, slope,
            )
        return (
            grad_input,
            grad_weight if need_weight_g else None,
            grad_bias if need_bias_g else None,
            None, None, None, None, None, None, None, None, None,
        )


def stem_pool_eligible(bn, pool, input: torch.Tensor) -> bool:
    """True when ``pool(bn(input))`` can run as SyncBatchNormActPoolFunction:
    a training-mode out-of-place SyncBatchNormAct2d, MaxPool2d(3, 2, 1)
    (dilation 1, floor mode, no indices) and a non-empty dense channels-last
    CUDA input.  Everything else runs the composition, modules with hooks
    included (the fused route does not go through their ``__call__``)."""
    def _pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    def _hooked(m):
        return bool(m._forward_hooks or m._forward_pre_hooks
                    or m._backward_hooks or m._backward_pre_hooks)

    return (
        type(bn) is SyncBatchNormAct2d
        and not getattr(bn, "inplace", False)
        and not _hooked(bn) and not _hooked(pool)
        and (bn.training
             or (bn.running_mean is None and bn.running_var is None))
        and type(pool) is torch.nn.MaxPool2d
        and _pair(pool.kernel_size) == (3, 3)
        and _pair(pool.stride) == (2, 2)
        and _pair(pool.padding) == (1, 1)
        and _pair(pool.dilation) == (1, 1)
        and not pool.ceil_mode and not pool.return_indices
        and input.is_cuda and input.dim() == 4 and input.numel() > 0
        and input.is_contiguous(memory_format=torch.channels_last)
        and input.dtype in (torch.float32, torch.bfloat16, torch.float16)
    )


def bn_act_maxpool(bn, pool, input: torch.Tensor, fork: bool = False):
    """``pool(bn(input))`` for a SyncBatchNormAct2d ``bn`` and a MaxPool2d
    ``pool``, fused into SyncBatchNormActPoolFunction where eligible and the
    plain composition otherwise.  ``fork=True`` returns a ``(main, skip)``
    pair for a result with two consumers (see SyncBatchNormAct2d.forward);
    the composition's pair is the same tensor twice."""
    if not stem_pool_eligible(bn, pool, input):
        y = pool(bn(input))
        return (y, y) if fork else y
    bn._check_input_dim(input)
    bn._check_non_zero_input_channels(input)
    if bn.training and bn.track_running_stats:
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
    factor = _momentum_factor(bn) if bn.training else (
        bn.momentum if bn.momentum is not None else 0.0
    )
    process_group = None
    world_size = 1
    if dist.is_available() and dist.is_initialized():
        process_group = bn.process_group or dist.group.WORLD
        world_size = dist.get_world_size(process_group)
    running_mean = bn.running_mean if bn.track_running_stats else None
    running_var = bn.running_var if bn.track_running_stats else None
    return SyncBatchNormActPoolFunction.apply(
        input, bn.weight, bn.bias, running_mean, running_var, bn.eps, factor,
        process_group, world_size, bn.relu,
        getattr(bn, "negative_slope", 0.0), fork,
    )


def _combined4(parts, C: int):
    """The dual reduce returns its four sums as views of ONE contiguous
    ``[4C]`` buffer: all_reduce that buffer itself.  Anything else (the
    single ops' two ``[2C]`` buffers, CPU) is cat-copied."""
    first = parts[0]
    adjacent = all(
        p.is_contiguous() and p.numel() == C
        and p.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
        and p.data_ptr() == first.data_ptr() + i * C * first.element_size()
        for i, p in enumerate(parts)
    )
    if adjacent:
        base = first.new_empty(0)
        base.set_(first.untyped_storage(), first.storage_offset(), (4 * C,),
                  (1,))
        return base
    return torch.cat(parts)


class SyncBatchNormDualActFunction(torch.autograd.Function):
    """``relu(bn(x) + bn_skip(x_skip))`` as one layer: the first block of a
    ResNet stage, whose skip path has a BatchNorm of its own
    (docs/KERNEL_DESIGN.md "Dual BN").

    On the dual kernels the skip BN's output is never stored, the backward
    reads the gated gradient once per pass for both layers, and the saved
    tensors are x, x_skip, the gate bits and per-channel vectors.  Results
    are bit-identical to ``bn(x, residual=bn_skip(x_skip), fork=fork)``.

    The function fixes the collective schedule, whatever kernels run on this
    rank: forward statistics of the skip layer, then of the main layer;
    backward ONE all_reduce of ``[sum_dy | sum_dy_xmu | sum_dy_2 |
    sum_dy_xmu_2]`` (4C fp32).  The composition issues the same collectives
    in another order, so every rank of a group must be on the same route:
    callers choose it from properties that are equal on all ranks
    (``bn_add_bn_act``).  Whether the dual KERNELS run is decided here, per
    rank: an empty input, tensors that are not dense channels-last bf16 /
    half with C a multiple of 8 and 16-byte aligned, or a skip input that
    needs no gradient run the single-BN ops instead and pack their sums into
    the same message (CPU tensors included)."""

    @staticmethod
    def forward(ctx, input, input2, weight, bias, weight2, bias2,
                running_mean, running_var, running_mean2, running_var2,
                eps: float, eps2: float, momentum: float, momentum2: float,
                process_group, world_size: int, fork: bool = False):
        x = _contig(input)
        x2 = _contig(input2)
        weight, bias, weight2, bias2 = (
            None if t is None else t.contiguous()
            for t in (weight, bias, weight2, bias2)
        )
        use_sync = world_size > 1 or (
            process_group is not None and _force_sync()
        )
        mean2, invstd2, count2, coefs2 = compute_sync_stats(
            x2, eps2, momentum2, running_mean2, running_var2,
            process_group, world_size, weight2, bias2, want_coefs=True,
        )
        # x and x_skip have one shape on every rank, so the skip layer's
        # total count is the main layer's: one copy is kept, and this one is
        # released before anything else is allocated
        del count2
        mean, invstd, count, coefs = compute_sync_stats(
            x, eps, momentum, running_mean, running_var,
            process_group, world_size, weight, bias, want_coefs=True,
        )
        # what the composition's residual, bn_skip(x_skip), would require
        need_r = any(ctx.needs_input_grad[i] for i in (1, 4, 5))
        y = r = gate = None
        dual = False
        if x.numel() == 0:
            y = torch.empty_like(x)
        elif (x.is_cuda and ctx.needs_input_grad[1] and coefs is not None
                and coefs2 is not None and x2.stride() == x.stride()):
            bits = ops.gate_bits_empty(x)
            y, dual = ops.batch_norm_elemt_act_dual(
                x, x2, coefs, coefs2, True, 0.0, bits
            )
            if dual:
                gate = bits
        if y is None:
            # the composition's own two launches
            r = _match_layout(ops.batch_norm_elemt_act(
                x2, None, weight2, bias2, mean2, invstd2, False, coefs2), x)
            if need_r and x.is_cuda:
                y, gate = ops.batch_norm_elemt_act(
                    x, r, weight, bias, mean, invstd, True, coefs, 0.0,
                    ops.gate_bits_empty(x),
                )
            else:
                y = ops.batch_norm_elemt_act(
                    x, r, weight, bias, mean, invstd, True, coefs, 0.0
                )
            if gate is not None:
                r = None
        ctx.dual = dual
        ctx.need_r = need_r
        ctx.use_sync = use_sync
        ctx.process_group = process_group
        # Per-channel vectors: those of the composition's two layers, with
        # the skip layer's [scale | shift] in the place of its count on the
        # dual route.  The forward kernel reads that vector while y exists,
        # so releasing it afterwards could not lower the peak; keeping it
        # means that nothing is alive during the forward that is not held
        # after it, and the layer holds what the composition holds.
        ctx.save_for_backward(x, x2, r, gate, weight, bias, weight2, bias2,
                              mean, invstd, mean2, invstd2, count, coefs,
                              coefs2 if dual else None)
        if not fork:
            return y
        # an unused output then arrives as None, not as a full-size zero fill
        ctx.set_materialize_grads(False)
        return y, y.detach()

    @staticmethod
    def backward(ctx, grad_output, grad_skip=None):
        if grad_output is None:  # fork with only the second output used
            grad_output, grad_skip = grad_skip, None
        if grad_output is None:
            return (None,) * 17
        (x, x2, r, gate, weight, bias, weight2, bias2, mean, invstd, mean2,
         invstd2, count, coefs, _coefs2) = ctx.saved_tensors
        need_x, need_x2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = weight is not None and ctx.needs_input_grad[2]
        need_b = bias is not None and ctx.needs_input_grad[3]
        need_w2 = weight2 is not None and ctx.needs_input_grad[4]
        need_b2 = bias2 is not None and ctx.needs_input_grad[5]
        need_r = ctx.need_r
        process_group = ctx.process_group
        sync = ctx.use_sync and (need_x or need_r)
        C = int(x.shape[1])

        def all_reduce(combined):
            from msbn.utils import debug as _dbg
            if _dbg.enabled():  # peers verify; skipping would hang them
                _dbg.verify_collective("syncbn.bwd.all_reduce", combined,
                                       process_group)
            dist.all_reduce(combined, dist.ReduceOp.SUM, group=process_group)
            from msbn.utils.logging import comm_log
            comm_log.record("all_reduce", combined.numel() * 4,
                            f"syncbn bwd dual C={C}")

        def result(dx, dx2, gw, gb, gw2, gb2):
            return (
                dx if need_x else None, dx2 if need_x2 else None,
                gw if need_w else None, gb if need_b else None,
                gw2 if need_w2 else None, gb2 if need_b2 else None,
            ) + (None,) * 11

        # both gradients of a forked output reach the GPU reduce unsummed
        fold = grad_skip is not None and x.is_cuda and x.numel() > 0
        if grad_skip is not None and not fold:
            grad_output = grad_output + grad_skip
            grad_skip = None
        grad_output = _match_layout(grad_output, x)
        if fold:
            grad_skip = _match_layout(grad_skip, x)

        if x.numel() == 0:
            # empty-input rank (join): contribute zeros, keep peers unblocked
            if sync:
                all_reduce(torch.zeros(4 * C, dtype=torch.float32,
                                       device=grad_output.device))
            return result(
                torch.empty_like(grad_output), torch.empty_like(x2),
                None if weight is None else torch.zeros_like(weight),
                None if bias is None else torch.zeros_like(bias),
                None if weight2 is None else torch.zeros_like(weight2),
                None if bias2 is None else torch.zeros_like(bias2),
            )

        if ctx.dual:
            gm = torch.empty_like(grad_output)
            (sum_dy, sum_dy_xmu, gw, gb, sum_dy2, sum_dy_xmu2, gw2, gb2) = (
                ops.batch_norm_backward_reduce_act(
                    grad_output, x, None, mean, invstd, weight, bias, True,
                    need_x, need_w, need_b, coefs, gm, 0.0, grad_skip,
                    gate=gate, dual=(x2, mean2, invstd2, weight2),
                )
            )
            combined = _combined4(
                (sum_dy, sum_dy_xmu, sum_dy2, sum_dy_xmu2), C)
            if sync:
                all_reduce(combined)
            if need_x:
                dx, dx2 = ops.batch_norm_backward_elemt_dual(
                    gm, x, x2, mean, mean2, invstd, invstd2, weight, weight2,
                    combined, count,
                )
            else:
                dx = None
                dx2 = ops.batch_norm_backward_elemt(
                    gm, x2, mean2, invstd2, weight2, combined[2 * C:3 * C],
                    combined[3 * C:], count,
                )
            return result(dx, dx2, gw, gb, gw2, gb2)

        # the single-BN ops of the composition, their sums in one message
        use_gm = fold or need_r
        gm = torch.empty_like(grad_output) if use_gm else None
        sum_dy, sum_dy_xmu, gw, gb = ops.batch_norm_backward_reduce_act(
            grad_output, x, r, mean, invstd, weight, bias, True, need_x,
            need_w, need_b, coefs, gm, 0.0, grad_skip,
            **({} if gate is None else {"gate": gate}),
        )
        gw2 = gb2 = g2 = None
        if need_r:
            g2 = _match_layout(gm, x2)
            sum_dy2, sum_dy_xmu2, gw2, gb2 = ops.batch_norm_backward_reduce(
                g2, x2, mean2, invstd2, weight2, need_x2, need_w2, need_b2,
            )
        else:
            sum_dy2 = sum_dy_xmu2 = None
        # a layer whose input needs no gradient sends zeros (the CPU ops
        # then form no sums at all)
        zeros = torch.zeros(C, dtype=torch.float32, device=x.device)
        combined = torch.cat([
            zeros if s is None else s
            for s in (sum_dy, sum_dy_xmu, sum_dy2, sum_dy_xmu2)
        ])
        if sync:
            all_reduce(combined)
        dx = dx2 = None
        if need_x:
            if use_gm:
                dx, _ = ops.batch_norm_backward_elemt_act(
                    gm, x, None, mean, invstd, weight, bias, combined[:C],
                    combined[C:2 * C], count, False, False, coefs,
                )
            else:
                dx, _ = ops.batch_norm_backward_elemt_act(
                    grad_output, x, r, mean, invstd, weight, bias,
                    combined[:C], combined[C:2 * C], count, True, False,
                    coefs, 0.0,
                )
        if need_x2:
            dx2 = ops.batch_norm_backward_elemt(
                g2, x2, mean2, invstd2, weight2, combined[2 * C:3 * C],
                combined[3 * C:], count,
            )
        return result(dx, dx2, gw, gb, gw2, gb2)


def _hooked(m) -> bool:
    return bool(m._forward_hooks or m._forward_pre_hooks
                or m._backward_hooks or m._backward_pre_hooks)


def dual_bn_eligible(bn, bn_skip, x: torch.Tensor) -> bool:
    """True when ``bn(x, residual=bn_skip(x_skip))`` runs as
    SyncBatchNormDualActFunction.  The two routes issue their collectives in
    different orders, so this looks only at what is equal on every rank of a
    group by construction: the module types and flags (a training-mode
    out-of-place relu SyncBatchNormAct2d with gate bits, a training-mode
    SyncBatchNorm proper, no hooks, equal ``num_features`` and process
    group), and a 4-D bf16 / half input on a CUDA device.  Sizes, strides
    and addresses are the function's own business."""
    if not (
        type(bn) is SyncBatchNormAct2d and type(bn_skip) is SyncBatchNorm
        and bn.training and bn_skip.training
        and bn.relu and getattr(bn, "negative_slope", 0.0) == 0.0
        and getattr(bn, "gate_bits", False)
        and not getattr(bn, "inplace", False)
        and not _hooked(bn) and not _hooked(bn_skip)
        and bn.num_features == bn_skip.num_features
        and bn.process_group is bn_skip.process_group
        and x.is_cuda and x.dim() == 4
        and x.dtype in (torch.bfloat16, torch.float16)
    ):
        return False
    return True


def bn_add_bn_act(bn, bn_skip, x: torch.Tensor, x_skip: torch.Tensor,
                  fork: bool = False):
    """``bn(x, residual=bn_skip(x_skip), fork=fork)`` for the closing
    SyncBatchNormAct2d ``bn`` of a residual block and the SyncBatchNorm
    ``bn_skip`` of its downsample path: one dual layer where
    ``dual_bn_eligible``, exactly that composition otherwise (frozen or
    swapped modules, eval mode, fp32, CPU, hooks).  ``fork=True`` returns a
    ``(main, skip)`` pair (SyncBatchNormAct2d.forward).  Both modules'
    running statistics and ``num_batches_tracked`` move as their own
    ``forward`` would move them."""
    eligible = dual_bn_eligible(bn, bn_skip, x)
    process_group = None
    world_size = 1
    if eligible and dist.is_available() and dist.is_initialized():
        process_group = bn.process_group or dist.group.WORLD
        world_size = dist.get_world_size(process_group)
    if eligible and not (world_size > 1 or (
            process_group is not None and _force_sync())):
        # no collectives, so nothing to keep in step: small NCHW planes
        # stay on the composition's single-launch kernels
        eligible = not (
            ops.bn_fused_local_eligible(x, bn.weight, bn.bias,
                                        bn.running_mean, bn.running_var)
            or ops.bn_fused_local_eligible(x_skip, bn_skip.weight,
                                           bn_skip.bias, bn_skip.running_mean,
                                           bn_skip.running_var)
        )
    if not eligible:
        if fork:
            return bn(x, residual=bn_skip(x_skip), fork=True)
        return bn(x, residual=bn_skip(x_skip))
    for m, t in ((bn_skip, x_skip), (bn, x)):
        m._check_input_dim(t)
        m._check_non_zero_input_channels(t)
        if m.track_running_stats and m.num_batches_tracked is not None:
            m.num_batches_tracked.add_(1)

    def running(m):
        if m.track_running_stats:
            return m.running_mean, m.running_var
        return None, None

    return SyncBatchNormDualActFunction.apply(
        x, x_skip, bn.weight, bn.bias, bn_skip.weight, bn_skip.bias,
        *running(bn), *running(bn_skip), bn.eps, bn_skip.eps,
        _momentum_factor(bn), _momentum_factor(bn_skip), process_group,
        world_size, fork,
    )


class InPlaceSyncBatchNormActFunction(torch.autograd.Function):
    """In-Place Activated SyncBatchNorm (Rota Bulo et al., 2018): the output
    ``y = act(bn(x))`` is written over ``x`` and the backward works from ``y``
    alone, so the layer keeps no activation-sized tensor of its own (the next
    conv saves ``y`` anyway).  ``act`` is the identity or LeakyReLU with
    ``negative_slope > 0``; statistics, their sync and the running update are
    those of SyncBatchNormActFunction.  Always the two-stage kernels."""

    @staticmethod
    def forward(
        ctx,
        input: torch.Tensor,
        weight: torch.Tensor,
        bias: torch.Tensor,
        running_mean: Optional[torch.Tensor],
        running_var: Optional[torch.Tensor],
        eps: float,
        momentum: float,
        process_group,
        world_size: int,
        act: bool,
        negative_slope: float = 0.0,
    ):
        if act and not negative_slope > 0.0:
            raise ValueError(
                "in-place BN needs an invertible activation: identity, or "
                "LeakyReLU with negative_slope > 0"
            )
        if _contig(input) is not input:
            raise ValueError(
                "in-place BN needs a dense NCHW or channels-last input; a "
                "copy would leave the caller's tensor unwritten"
            )
        weight = weight.contiguous()
        bias = bias.contiguous()
        use_sync = world_size > 1 or (
            process_group is not None and _force_sync()
        )
        # the statistics are read before the overwrite (same stream)
        mean, invstd, count_sum, coefs = compute_sync_stats(
            input, eps, momentum, running_mean, running_var,
            process_group, world_size, weight, bias, want_coefs=True,
        )
        if input.numel() > 0:
            ops.batch_norm_elemt_act_(
                input, weight, bias, mean, invstd, act, coefs, negative_slope
            )
        ctx.mark_dirty(input)
        ctx.has_coefs = coefs is not None
        saved = (input, weight, bias, mean, invstd, count_sum)
        ctx.save_for_backward(*(saved + ((coefs,) if ctx.has_coefs else ())))
        ctx.act = act
        ctx.negative_slope = negative_slope
        ctx.process_group = process_group
        ctx.world_size = world_size
        ctx.use_sync = use_sync
        return input

    @staticmethod
    def backward(ctx, grad_output):
        saved = ctx.saved_tensors
        y, weight, bias, mean, invstd, count_sum = saved[:6]
        coefs = saved[6] if ctx.has_coefs else None
        grad_output = _match_layout(grad_output, y)
        act, slope = ctx.act, ctx.negative_slope
        process_group = ctx.process_group
        use_sync = ctx.use_sync
        need_input_g, need_weight_g, need_bias_g = ctx.needs_input_grad[:3]
        C = int(y.shape[1])

        if y.numel() == 0:
            # empty-input rank (join): contribute zeros, keep peers unblocked
            if use_sync and need_input_g:
                combined = torch.zeros(2 * C, dtype=torch.float32,
                                       device=grad_output.device)
                from msbn.utils import debug as _dbg
                if _dbg.enabled():  # peers verify; skipping would hang them
                    _dbg.verify_collective("syncbn.bwd.all_reduce", combined,
                                           process_group)
                dist.all_reduce(combined, dist.ReduceOp.SUM,
                                group=process_group)
            return (
                torch.empty_like(grad_output) if need_input_g else None,
                torch.zeros_like(weight) if need_weight_g else None,
                torch.zeros_like(bias) if need_bias_g else None,
                None, None, None, None, None, None, None, None,
            )
        sum_dy, sum_dy_xmu, grad_weight, grad_bias = (
            ops.batch_norm_backward_reduce_inplace(
                grad_output, y, invstd, weight, bias, act, need_input_g,
                need_weight_g, need_bias_g, coefs, slope,
            )
        )
        grad_input = None
        if need_input_g:
            if use_sync:
                combined, copied = _combined_view(sum_dy, sum_dy_xmu, C)
                from msbn.utils import debug as _dbg
                if _dbg.enabled():
                    _dbg.verify_collective("syncbn.bwd.all_reduce",
                                           combined, process_group)
                dist.all_reduce(combined, dist.ReduceOp.SUM, group=process_group)
                from msbn.utils.logging import comm_log
                comm_log.record("all_reduce", combined.numel() * 4,
                                f"syncbn bwd C={C}")
                if copied:
                    sum_dy, sum_dy_xmu = combined[:C], combined[C:]
            grad_input = ops.batch_norm_backward_elemt_inplace(
                grad_output, y, mean, invstd, weight, bias, sum_dy,
                sum_dy_xmu, count_sum, act, coefs, slope,
            )
        return (
            grad_input,
            grad_weight if need_weight_g else None,
            grad_bias if need_bias_g else None,
            None, None, None, None, None, None, None, None,
        )


class SyncBatchNormAct2d(SyncBatchNorm):
    """SyncBatchNorm with a fused (optional residual-add +) ReLU epilogue.

    forward(x, residual=None) == relu(bn(x) + residual) with identical math.
    ``relu=True, negative_slope=s`` makes the activation LeakyReLU(s):
    leaky_relu(bn(x) + residual, s).  The slope is a hyper-parameter, not
    state: state-dict keys are those of SyncBatchNorm.

    ``inplace=True`` (In-Place Activated BatchNorm) writes the output over
    the input in training mode and runs the backward from the output, so the
    layer keeps no activation-sized tensor alive: one activation tensor less
    per layer, at the byte traffic of the out-of-place path.  It needs
    ``affine=True`` and an invertible activation (``relu=False``, or
    ``relu=True`` with ``negative_slope > 0``; plain ReLU is rejected), and
    takes neither ``residual`` nor ``fork``.  Two preconditions the kernels
    cannot check:

    * ``weight != 0`` in every channel (the backward divides by
      ``weight*invstd``): a zero-initialised last BN of a residual block is
      incompatible; such a channel's gradients are finite but wrong.
    * the input must not be needed by its producer's backward (autograd's
      version counter raises if it is); conv outputs are fine.

    In-place layers always take the two-stage kernels (a known cost for
    planes <= 16K elements, where the out-of-place path has single-launch
    kernels).  In eval mode an ``inplace=True`` module takes the ordinary
    out-of-place running-statistics route, which saves nothing input-sized
    beyond what the gate needs.  State-dict keys are unchanged.
    """

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True,
                 track_running_stats=True, process_group=None, device=None,
                 dtype=None, relu: bool = True, negative_slope: float = 0.0,
                 inplace: bool = False, gate_bits: bool = True):
        super().__init__(num_features, eps, momentum, affine,
                         track_running_stats, process_group, device, dtype)
        # keep the activation's branch as one bit per element instead of the
        # residual where the kernels can (SyncBatchNormActFunction.forward);
        # False keeps the residual-recomputing route.  Same results.
        self.gate_bits = bool(gate_bits)
        self.relu = relu
        self.negative_slope = _check_negative_slope(relu, negative_slope)
        if inplace:
            if not affine:
                raise ValueError("inplace=True requires affine=True")
            if relu and not self.negative_slope > 0.0:
                raise ValueError(
                    "inplace=True needs an invertible activation: "
                    "relu=False, or relu=True with negative_slope > 0 "
                    "(plain ReLU cannot be inverted)"
                )
        self.inplace = bool(inplace)

    def extra_repr(self):
        s = super().extra_repr()
        slope = getattr(self, "negative_slope", 0.0)
        if slope != 0.0:
            s += f", negative_slope={slope}"
        if getattr(self, "inplace", False):
            s += ", inplace=True"
        return s

    def forward(self, input: torch.Tensor,
                residual: Optional[torch.Tensor] = None, fork: bool = False):
        """``fork=True`` returns the output as a ``(main, skip)`` pair of
        tensors over one storage, for a result with two consumers: their
        gradients then reach this layer's backward unsummed (see
        SyncBatchNormActFunction.forward).  Train and eval mode alike."""
        self._check_input_dim(input)
        self._check_non_zero_input_channels(input)
        # default: modules pickled before negative_slope existed
        slope = getattr(self, "negative_slope", 0.0)
        # likewise for inplace
        inplace = getattr(self, "inplace", False)
        if inplace and (residual is not None or fork):
            raise ValueError(
                "an inplace=True SyncBatchNormAct2d takes neither a residual "
                "nor fork=True"
            )

        bn_training = self.training or (
            self.running_mean is None and self.running_var is None
        )
        if self.training and self.track_running_stats:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked.add_(1)
        factor = _momentum_factor(self) if self.training else (
            self.momentum if self.momentum is not None else 0.0
        )

        if not bn_training:
            # the frozen kernels take one gradient: both consumers hang off
            # the same tensor and autograd sums for them, as ever
            y = _running_stats_forward(self, input, residual, self.relu,
                                       slope)
            return (y, y) if fork else y

        process_group = None
        world_size = 1
        if dist.is_available() and dist.is_initialized():
            process_group = self.process_group or dist.group.WORLD
            world_size = dist.get_world_size(process_group)

        running_mean = self.running_mean if self.track_running_stats else None
        running_var = self.running_var if self.track_running_stats else None
        if inplace:
            return InPlaceSyncBatchNormActFunction.apply(
                input, self.weight, self.bias, running_mean, running_var,
                self.eps, factor, process_group, world_size, self.relu, slope,
            )
        return SyncBatchNormActFunction.apply(
            input, residual, self.weight, self.bias, running_mean, running_var,
            self.eps, factor, process_group, world_size, self.relu, slope,
            fork,
            # default: modules pickled before gate_bits existed
            getattr(self, "gate_bits", False),
        )
