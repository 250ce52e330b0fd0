"""fuse_bn_act: graph-free module-tree pass that merges adjacent
(BatchNorm2d | SyncBatchNorm, ReLU | LeakyReLU) pairs inside nn.Sequential
containers into a single SyncBatchNormAct2d (one-kernel epilogue, identical
math).  A LeakyReLU's ``negative_slope`` is carried into the fused module;
``inplace`` is irrelevant for either activation.  A (FrozenBatchNorm2d,
ReLU | LeakyReLU) pair becomes a FrozenBatchNorm2d(relu=True[,
negative_slope=s]).  ``fuse_bn_act(model, inplace=True)`` makes the
(BN, LeakyReLU) pairs in-place modules (the output overwrites the input, the
backward runs from the output; see SyncBatchNormAct2d).

Works on any model whose BN+activation pairs live in Sequentials (DCGAN
generator and discriminator, torchvision-style stems, custom CNNs).  Residual-add fusion requires the
block to call the module with ``residual=`` (see msbn.models.resnet's fused
blocks) and is not attempted here.

    model = msbn.nn.fuse_bn_act(msbn.convert_sync_batchnorm(model))
"""

import torch.nn as nn

from msbn.nn.batchnorm import SyncBatchNorm, _BatchNorm
from msbn.nn.frozen import FrozenBatchNorm2d, _frozen_from
from msbn.nn.fused import SyncBatchNormAct2d


_ACTS = (nn.ReLU, nn.LeakyReLU)


def _to_act(bn, act_module, inplace=False):
    relu = isinstance(act_module, _ACTS)
    slope = (float(act_module.negative_slope)
             if isinstance(act_module, nn.LeakyReLU) else 0.0)
    if isinstance(bn, FrozenBatchNorm2d):
        # frozen stays frozen: same tensors, activation folded into the
        # epilogue
        return _frozen_from(bn, relu=relu, negative_slope=slope)
    out = SyncBatchNormAct2d(
        bn.num_features, bn.eps, bn.momentum, bn.affine,
        bn.track_running_stats,
        getattr(bn, "process_group", None),
        relu=relu, negative_slope=slope,
        # only what the in-place backward can invert; the rest (plain ReLU,
        # no affine) fuses out of place as ever
        inplace=inplace and bn.affine and slope > 0.0,
    )
    if bn.affine:
        out.weight = bn.weight
        out.bias = bn.bias
    out.running_mean = bn.running_mean
    out.running_var = bn.running_var
    out.num_batches_tracked = bn.num_batches_tracked
    out.training = bn.training
    return out


def _fusable_bn(m) -> bool:
    if isinstance(m, SyncBatchNormAct2d):
        return False
    if isinstance(m, FrozenBatchNorm2d):
        return not m.relu
    return isinstance(m, (SyncBatchNorm, _BatchNorm, nn.modules.batchnorm._BatchNorm))


def fuse_bn_act(module: nn.Module, inplace: bool = False) -> nn.Module:
    """Recursively fuse (BN, ReLU) and (BN, LeakyReLU) pairs inside
    Sequential containers.

    ``inplace=True`` turns every (BN, LeakyReLU) pair with a positive slope
    and an affine BN into an in-place module
    (``SyncBatchNormAct2d(inplace=True)``: the output overwrites the input
    and the backward runs from the output, one activation tensor less per
    layer); (BN, ReLU) pairs are fused out of place as without it.  Two
    preconditions the kernels cannot check: every channel's ``weight`` must
    be non-zero (a zero-initialised BN is incompatible: finite but wrong
    gradients for that channel), and the BN's input must not be needed by its
    producer's backward (autograd's version counter raises if it is; conv
    outputs are fine)."""
    for name, child in module.named_children():
        fuse_bn_act(child, inplace)
        if isinstance(child, nn.Sequential):
            items = list(child._modules.items())
            new_items = []
            i = 0
            while i < len(items):
                k, m = items[i]
                if (
                    i + 1 < len(items)
                    and _fusable_bn(m)
                    and isinstance(items[i + 1][1], _ACTS)
                ):
                    new_items.append((k, _to_act(m, items[i + 1][1], inplace)))
                    i += 2
                else:
                    new_items.append((k, m))
                    i += 1
            if len(new_items) != len(items):
                child._modules.clear()
                for k, m in new_items:
                    child._modules[k] = m
    return module
