from msbn.nn.batchnorm import (  # noqa: F401
    BatchNorm1d,
    BatchNorm2d,
    BatchNorm3d,
    SyncBatchNorm,
    convert_sync_batchnorm,
)
from msbn.nn.functions import SyncBatchNormFunction  # noqa: F401
from msbn.nn.fused import (  # noqa: F401
    InPlaceSyncBatchNormActFunction,
    SyncBatchNormAct2d,
    SyncBatchNormActFunction,
)
from msbn.nn.frozen import (  # noqa: F401
    FrozenBatchNorm2d,
    FrozenBatchNormActFunction,
    freeze_batchnorm,
)
from msbn.nn.fuse_pass import fuse_bn_act  # noqa: F401

__all__ = [
    "FrozenBatchNorm2d",
    "FrozenBatchNormActFunction",
    "freeze_batchnorm",
    "BatchNorm1d",
    "BatchNorm2d",
    "BatchNorm3d",
    "SyncBatchNorm",
    "convert_sync_batchnorm",
    "SyncBatchNormFunction",
    "SyncBatchNormAct2d",
    "InPlaceSyncBatchNormActFunction",
    "fuse_bn_act",
]
