"""Frozen BatchNorm: normalize with FIXED running statistics, gradients flow.

The detection fine-tuning recipe (frozen backbone BN) and any BatchNorm in
``.eval()`` with autograd on share one code path here:

  forward   ``bn_frozen_coefs`` (one tiny launch: running stats + affine ->
            packed [scale | shift]) + ONE elemt launch
            y = relu?(x*scale + shift [+ residual]);
  backward  ONE elementwise kernel: dx = scale*g, dres = g, g = dy*1[z>0]
            with the ReLU gate recomputed in-kernel.  Without a ReLU the
            kernel never reads x, so the input is not kept alive.

A non-zero ``negative_slope`` turns the ReLU into LeakyReLU (forward
z>0 ? z : slope*z, gate z>0 ? dy : slope*dy) in the same kernels.

With fixed statistics there are no batch reductions.  Only when the affine
parameters themselves need a gradient (a trainable BN put in ``.eval()``)
does backward run the existing per-channel reduce kernel first.

``FrozenBatchNorm2d`` holds weight / bias / running stats as BUFFERS (zero
parameters: nothing for the optimizer or the DDP reducer), with state-dict
keys identical to ``BatchNorm2d``.  ``freeze_batchnorm`` converts a module
tree in place of the ``.eval()``-after-every-``.train()`` idiom.
"""

from typing import Optional

import torch
from torch.nn import Module

from msbn import ops
from msbn.nn.batchnorm import (_NormBase, _check_negative_slope,
                               _running_stats_forward)
from msbn.nn.functions import _contig, _match_layout


def _dense_format(t: torch.Tensor) -> torch.memory_format:
    """The memory format the kernels index ``t`` with (as _match_layout)."""
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return torch.channels_last
    if t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d):
        return torch.channels_last_3d
    return torch.contiguous_format


def _elemt(input, residual, coefs, relu: bool, negative_slope: float = 0.0):
    C = int(input.shape[1])
    scale, shift = coefs[:C], coefs[C:]
    if input.is_cuda:
        # mean / invstd / weight / bias are not consulted when coefs is given
        return ops.batch_norm_elemt_act(
            input, residual, None, None, scale, scale, relu, coefs,
            negative_slope,
        )
    # CPU reference takes (mean, invstd, weight, bias): mean=0, invstd=scale,
    # bias=shift reproduces x*scale + shift
    return ops.batch_norm_elemt_act(
        input, residual, None, shift, torch.zeros_like(scale), scale, relu,
        None, negative_slope,
    )


class FrozenBatchNormActFunction(torch.autograd.Function):
    """y = relu?(bn_running(x) [+ residual]) with fixed statistics.

    Host-sync free in both directions (hipGraph-capturable).
    """

    @staticmethod
    def forward(
        ctx,
        input: torch.Tensor,
        residual: Optional[torch.Tensor],
        weight: Optional[torch.Tensor],
        bias: Optional[torch.Tensor],
        running_mean: torch.Tensor,
        running_var: torch.Tensor,
        eps: float,
        relu: bool,
        negative_slope: float = 0.0,
    ):
        ctx.negative_slope = negative_slope
        input = _contig(input)
        if residual is not None:
            residual = _match_layout(residual, input)
        if weight is not None:
            weight = weight.contiguous()
        if bias is not None:
            bias = bias.contiguous()
        running_mean = running_mean.contiguous()
        running_var = running_var.contiguous()

        coefs = ops.bn_frozen_coefs(running_mean, running_var, eps, weight,
                                    bias)

        affine_g = (weight is not None and ctx.needs_input_grad[2]) or (
            bias is not None and ctx.needs_input_grad[3]
        )
        # save only what backward reads: the gate needs (input, residual),
        # the affine reduction needs (input, running stats)
        keep_x = relu or affine_g
        ctx.save_for_backward(
            coefs,
            input if keep_x else None,
            residual if relu else None,
            weight if affine_g else None,
            bias if affine_g else None,
            running_mean if affine_g else None,
            running_var if affine_g else None,
        )
        ctx.relu = relu
        ctx.eps = eps
        ctx.has_residual = residual is not None
        ctx.memory_format = _dense_format(input)
        if input.numel() == 0:
            return torch.empty_like(input)
        return _elemt(input, residual, coefs, relu, negative_slope)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        (coefs, input, residual, weight, bias, running_mean,
         running_var) = ctx.saved_tensors
        relu = ctx.relu
        slope = ctx.negative_slope
        grad_output = grad_output.contiguous(memory_format=ctx.memory_format) \
            if input is None else _match_layout(grad_output, input)
        need_input_g = ctx.needs_input_grad[0]
        need_res_g = ctx.has_residual and ctx.needs_input_grad[1]
        need_weight_g = weight is not None and ctx.needs_input_grad[2]
        need_bias_g = bias is not None and ctx.needs_input_grad[3]

        if grad_output.numel() == 0:
            return (
                torch.empty_like(grad_output) if need_input_g else None,
                torch.empty_like(grad_output) if need_res_g else None,
                torch.zeros_like(weight) if need_weight_g else None,
                torch.zeros_like(bias) if need_bias_g else None,
                None, None, None, None, None,
            )

        grad_weight = grad_bias = None
        if need_weight_g or need_bias_g:
            # trainable affine under fixed statistics: the existing reduce
            # kernel with mean=running_mean, invstd=rsqrt(running_var+eps)
            # gives grad_weight / grad_bias and writes the masked gradient
            # gm = dy*1[z>0]; the elementwise pass then runs gate-free on gm.
            want_elemt = need_input_g or need_res_g
            mean = running_mean.to(torch.float32)
            invstd = torch.rsqrt(running_var.to(torch.float32) + ctx.eps)
            gm = torch.empty_like(grad_output) if (relu and want_elemt) \
                else None
            _, _, grad_weight, grad_bias = ops.batch_norm_backward_reduce_act(
                grad_output, input, residual, mean, invstd, weight, bias,
                relu, False, need_weight_g, need_bias_g, coefs, gm, slope,
            )
            if gm is not None:
                grad_output, relu = gm, False

        grad_input = grad_res = None
        if need_input_g or need_res_g:
            grad_input, grad_res = ops.batch_norm_frozen_backward_elemt(
                grad_output, input if relu else None,
                residual if relu else None, coefs, relu, need_input_g,
                need_res_g, slope,
            )
        return (
            grad_input,
            grad_res,
            grad_weight if need_weight_g else None,
            grad_bias if need_bias_g else None,
            None, None, None, None, None,
        )


class FrozenBatchNorm2d(_NormBase):
    """BatchNorm with fixed statistics AND fixed affine (+ optional fused
    residual-add / ReLU epilogue): ``forward(x, residual=None)`` ==
    ``relu?(bn_eval(x) [+ residual])`` whatever ``.training`` says.
    ``relu=True, negative_slope=s`` makes the activation LeakyReLU(s).

    ``weight``, ``bias``, ``running_mean``, ``running_var`` and
    ``num_batches_tracked`` are buffers (zero parameters) under the same
    state-dict keys as ``BatchNorm2d``, so torch / msbn BN checkpoints load
    strict; the statistics are never updated.  Subclasses ``_NormBase`` so
    mixed-precision helpers keyed on it keep the module fp32.
    """

    _msbn_frozen = True

    def __init__(self, num_features: int, eps: float = 1e-5,
                 relu: bool = False, device=None, dtype=None,
                 negative_slope: float = 0.0) -> None:
        # buffers instead of _NormBase's parameters: no _NormBase.__init__
        Module.__init__(self)
        factory_kwargs = {"device": device, "dtype": dtype}
        self.num_features = num_features
        self.eps = eps
        self.momentum = 0.0
        self.affine = True
        self.track_running_stats = True
        self.relu = relu
        self.negative_slope = _check_negative_slope(relu, negative_slope)
        self.register_buffer("weight",
                             torch.ones(num_features, **factory_kwargs))
        self.register_buffer("bias",
                             torch.zeros(num_features, **factory_kwargs))
        self.register_buffer("running_mean",
                             torch.zeros(num_features, **factory_kwargs))
        self.register_buffer("running_var",
                             torch.ones(num_features, **factory_kwargs))
        self.register_buffer(
            "num_batches_tracked",
            torch.tensor(0, dtype=torch.long, device=device),
        )

    def reset_parameters(self) -> None:
        self.reset_running_stats()
        self.weight.fill_(1)
        self.bias.zero_()

    def _check_input_dim(self, input):
        if input.dim() < 2:
            raise ValueError(
                f"expected at least 2D input (got {input.dim()}D input)"
            )

    def extra_repr(self):
        s = f"{self.num_features}, eps={self.eps}, relu={self.relu}"
        slope = getattr(self, "negative_slope", 0.0)
        if slope != 0.0:
            s += f", negative_slope={slope}"
        return s

    def _load_from_state_dict(
        self, state_dict, prefix, local_metadata, strict,
        missing_keys, unexpected_keys, error_msgs,
    ):
        # frozen-BN checkpoints (torchvision style) carry no
        # num_batches_tracked whatever version they claim; run them through
        # the v1 -> v2 migration
        if prefix + "num_batches_tracked" not in state_dict:
            local_metadata = dict(local_metadata, version=1)
        super()._load_from_state_dict(
            state_dict, prefix, local_metadata, strict,
            missing_keys, unexpected_keys, error_msgs,
        )

    def forward(self, input: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_input_dim(input)
        # default: modules pickled before negative_slope existed
        return _running_stats_forward(
            self, input, residual, self.relu,
            getattr(self, "negative_slope", 0.0),
        )


def _frozen_from(bn, relu: bool,
                 negative_slope: float = 0.0) -> FrozenBatchNorm2d:
    """A FrozenBatchNorm2d sharing ``bn``'s tensors."""
    if not bn.track_running_stats or bn.running_mean is None:
        raise ValueError(
            "freeze_batchnorm: a BatchNorm with track_running_stats=False "
            "has no statistics to freeze"
        )
    out = FrozenBatchNorm2d(bn.num_features, bn.eps, relu=relu,
                            device=bn.running_mean.device,
                            dtype=bn.running_mean.dtype,
                            negative_slope=negative_slope)
    if bn.weight is not None:
        out.weight = bn.weight.detach()
    if bn.bias is not None:
        out.bias = bn.bias.detach()
    out.running_mean = bn.running_mean
    out.running_var = bn.running_var
    if bn.num_batches_tracked is not None:
        out.num_batches_tracked = bn.num_batches_tracked
    out.training = bn.training
    if hasattr(bn, "qconfig"):
        out.qconfig = bn.qconfig
    return out


def freeze_batchnorm(module: Module) -> Module:
    """Recursively replace every BatchNorm (torch.nn BatchNorm1d/2d/3d and
    SyncBatchNorm; msbn BatchNorm*, SyncBatchNorm and SyncBatchNormAct2d)
    with a ``FrozenBatchNorm2d`` that shares its tensors and keeps a fused
    ReLU / LeakyReLU epilogue.  ``affine=False`` becomes ones / zeros buffers; a source
    without running statistics raises."""
    out = module
    targets = (torch.nn.modules.batchnorm._BatchNorm, _NormBase)
    if isinstance(module, targets) and not isinstance(module,
                                                      FrozenBatchNorm2d):
        relu = bool(getattr(module, "relu", False))
        out = _frozen_from(
            module, relu,
            getattr(module, "negative_slope", 0.0) if relu else 0.0,
        )
    for name, child in module.named_children():
        out.add_module(name, freeze_batchnorm(child))
    return out
