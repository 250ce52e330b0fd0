from msbn.models.simple import SimpleCNN  # noqa: F401
from msbn.models.resnet import resnet18, resnet50, ResNet  # noqa: F401
from msbn.models.dcgan import Generator, Discriminator  # noqa: F401
# imported up front: importing the submodule binds the package attribute
# ``retinanet`` to it, and the factory below has to be the last binding
from msbn.models.retinanet import RetinaNet  # noqa: F401

__all__ = [
    "SimpleCNN",
    "resnet18",
    "resnet50",
    "ResNet",
    "Generator",
    "Discriminator",
]


def retinanet(num_classes: int = 80, frozen_backbone: bool = False,
              fused_backbone: bool = False):
    """RetinaNet-R50-FPN.  ``fused_backbone`` builds the backbone with the
    fused BN(+add)+ReLU epilogues; ``frozen_backbone`` freezes every backbone
    BatchNorm (the detection fine-tuning recipe) — the heads keep trainable,
    sync-able BN.  The defaults give the plain trainable model."""
    return RetinaNet(num_classes, frozen_backbone=frozen_backbone,
                     fused_backbone=fused_backbone)


def convert_to_torch_batchnorm(module):
    """Recursively replace msbn BatchNorm/SyncBatchNorm modules with the
    stock ``torch.nn.BatchNorm1d/2d/3d`` equivalents, preserving parameters,
    running stats and training flag.  Used by the benchmarks' ``--stock``
    comparison lines: both impls then run the IDENTICAL architecture and
    initialization, differing only in the BN/DDP engine (the inverse of
    ``convert_sync_batchnorm``; cf. stock batchnorm.py:842-902).
    A ``FrozenBatchNorm2d`` becomes an eval-mode ``torch.nn.BatchNorm2d`` with
    non-trainable affine (same math); one with a fused ReLU raises."""
    import torch

    from msbn.nn.batchnorm import _NormBase, BatchNorm1d, BatchNorm3d

    out = module
    if getattr(out, "_msbn_frozen", False):
        # frozen -> eval-mode torch BN with non-trainable affine: same math
        if out.relu:
            raise ValueError(
                "convert_to_torch_batchnorm: FrozenBatchNorm2d(relu=True) has "
                "no torch.nn BatchNorm equivalent (the fused ReLU would be "
                "dropped); convert before fusing, or build the model unfused"
            )
        new = torch.nn.BatchNorm2d(out.num_features, out.eps)
        new.weight = torch.nn.Parameter(out.weight, requires_grad=False)
        new.bias = torch.nn.Parameter(out.bias, requires_grad=False)
        new.running_mean = out.running_mean
        new.running_var = out.running_var
        new.num_batches_tracked = out.num_batches_tracked
        new.training = False
        out = new
    elif isinstance(out, _NormBase):
        cls = torch.nn.BatchNorm2d
        if isinstance(out, BatchNorm1d):
            cls = torch.nn.BatchNorm1d
        elif isinstance(out, BatchNorm3d):
            cls = torch.nn.BatchNorm3d
        new = cls(
            out.num_features, out.eps, out.momentum, out.affine,
            out.track_running_stats,
        )
        if out.affine:
            with torch.no_grad():
                new.weight = out.weight
                new.bias = out.bias
        new.running_mean = out.running_mean
        new.running_var = out.running_var
        new.num_batches_tracked = out.num_batches_tracked
        new.training = out.training
        out = new
    for name, child in module.named_children():
        out.add_module(name, convert_to_torch_batchnorm(child))
    return out
