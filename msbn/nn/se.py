"""Squeeze-excite: the channel gate EfficientNet / MobileNetV3 blocks put
between the depthwise BN+SiLU layer and the 1x1 project convolution.

The module itself is the plain composition.  After a BatchNorm+SiLU layer of
this project it runs fused into that layer instead, through
``msbn.nn.fused.bn_silu_se`` (docs/KERNEL_DESIGN.md "Squeeze-excite").
"""

import torch
import torch.nn as nn
import torch.nn.functional as F


class SqueezeExcite(nn.Module):
    """``x * sigmoid(fc2(silu(fc1(mean_hw x))))`` with ``fc1`` / ``fc2`` 1x1
    convolutions with bias: the state-dict keys of torchvision's
    ``SqueezeExcitation``."""

    def __init__(self, channels: int, reduced: int):
        super().__init__()
        if channels < 1 or reduced < 1:
            raise ValueError("SqueezeExcite: channels and reduced must be >= 1")
        self.fc1 = nn.Conv2d(channels, reduced, 1)
        self.fc2 = nn.Conv2d(reduced, channels, 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.fc2(F.silu(self.fc1(s))))
