"""MBConv (inverted residual) blocks, the unit of EfficientNet / MobileNetV2
style backbones, with this project's BatchNorm+SiLU layers:

    1x1 expand -> BN+SiLU -> depthwise 3x3 | 5x5 (stride 1 | 2) -> BN+SiLU ->
    [squeeze-excite ->] 1x1 project -> BN (+ identity skip where the shapes
    allow)

``se_ratio`` (``None``: no squeeze-excite, and no module or state-dict key
for one) puts a ``SqueezeExcite`` with ``max(1, int(cin * se_ratio))`` hidden
channels after the depthwise BN+SiLU, as EfficientNet does (0.25).
``conv_stats=True`` runs the two 1x1 convolutions
through ``conv1x1_bn_act`` and the depthwise one through ``dwconv3x3_bn_act``
or, at kernel size 5, ``dwconv5x5_bn_act``:
the convolution kernels then emit the following BatchNorm's statistics and
its statistics pass does not run.  Whatever those routes do not take runs the
composition, so the flag changes neither modules nor state-dict keys.
Under ``conv_stats=True`` the squeeze-excite block runs fused into the
depthwise BN+SiLU layer (``bn_silu_se``: the activated tensor is never
stored); otherwise it is the module applied to the layer's output.
``dw_grad=True`` also runs the depthwise convolution's backward as this
project's gradient kernels (``ops.dwconv3x3_backward`` /
``ops.dwconv5x5_backward``); it is honoured only where ``conv_stats=True``.
"""

from typing import Optional, Sequence

import torch.nn as nn

from msbn.nn import SqueezeExcite, SyncBatchNorm
from msbn.nn.fused import (SyncBatchNormAct2d, conv1x1_bn_act,
                           dwconv3x3_bn_act, dwconv5x5_bn_act)


def _bn_silu(channels):
    return SyncBatchNormAct2d(channels, act="silu")


class MBConv(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int = 1, expand: int = 4,
                 conv_stats: bool = False, dw_grad: bool = False,
                 kernel_size: int = 3, se_ratio: Optional[float] = None):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError("MBConv: stride must be 1 or 2")
        if kernel_size not in (3, 5):
            raise ValueError("MBConv: kernel_size must be 3 or 5")
        mid = cin * expand
        self.conv_stats = conv_stats
        self.dw_grad = dw_grad  # honoured only where conv_stats
        self.skip = stride == 1 and cin == cout
        self.conv1 = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = _bn_silu(mid)
        self.conv2 = nn.Conv2d(mid, mid, kernel_size, stride,
                               kernel_size // 2, groups=mid, bias=False)
        self._dw_bn_act = dwconv3x3_bn_act if kernel_size == 3 else \
            dwconv5x5_bn_act
        self.bn2 = _bn_silu(mid)
        if se_ratio is not None:
            self.se = SqueezeExcite(mid, max(1, int(cin * se_ratio)))
        else:
            self.se = None
        self.conv3 = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = SyncBatchNorm(cout)

    def forward(self, x):
        if self.conv_stats:
            out = conv1x1_bn_act(self.conv1, self.bn1, x)
            out = self._dw_bn_act(self.conv2, self.bn2, out,
                                  grad_kernels=self.dw_grad, se=self.se)
            out = conv1x1_bn_act(self.conv3, self.bn3, out)
        else:
            out = self.bn1(self.conv1(x))
            out = self.bn2(self.conv2(out))
            if self.se is not None:
                out = self.se(out)
            out = self.bn3(self.conv3(out))
        return out + x if self.skip else out


class MBConvNet(nn.Module):
    def __init__(self, widths: Sequence[int], depths: Sequence[int],
                 num_classes: int = 1000, expand: int = 4,
                 conv_stats: bool = False, dw_grad: bool = False,
                 kernel_sizes: Optional[Sequence[int]] = None,
                 se_ratio: Optional[float] = None):
        super().__init__()
        if len(widths) != len(depths) or not widths:
            raise ValueError("mbconv_net: one depth per width")
        if kernel_sizes is None:
            kernel_sizes = (3,) * len(widths)
        if len(kernel_sizes) != len(widths):
            raise ValueError("mbconv_net: one kernel size per width")
        self.stem = nn.Conv2d(3, widths[0], 3, 2, 1, bias=False)
        self.stem_bn = _bn_silu(widths[0])
        blocks, cin = [], widths[0]
        for i, (width, depth, ksize) in enumerate(
                zip(widths, depths, kernel_sizes)):
            for j in range(depth):
                stride = 2 if j == 0 and i > 0 else 1
                blocks.append(MBConv(cin, width, stride, expand, conv_stats,
                                     dw_grad, ksize, se_ratio))
                cin = width
        self.blocks = nn.Sequential(*blocks)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        x = self.blocks(self.stem_bn(self.stem(x)))
        return self.fc(self.pool(x).flatten(1))


def mbconv_net(widths: Sequence[int] = (16, 24, 40, 80, 112, 192),
               depths: Sequence[int] = (1, 2, 2, 3, 3, 4),
               num_classes: int = 1000, expand: int = 4,
               conv_stats: bool = False, dw_grad: bool = False,
               kernel_sizes: Optional[Sequence[int]] = None,
               se_ratio: Optional[float] = None) -> MBConvNet:
    """A stack of MBConv stages (stage i > 0 opens with a stride-2 block)
    behind a plain 3x3/2 stem, with a pooled linear head.  The defaults are
    EfficientNet-B0's widths and depths up to its 192-channel stage.
    ``dw_grad=True`` runs the depthwise convolutions' backward as this
    project's gradient kernels; it is honoured only where
    ``conv_stats=True``.  ``kernel_sizes`` gives each stage's depthwise
    kernel size, 3 or 5 (``None``: 3 everywhere); EfficientNet-B0's are
    ``(3, 3, 5, 3, 5, 5)`` for the default widths.  ``se_ratio`` gives every
    block a squeeze-excite stage (EfficientNet: 0.25; ``None``: none)."""
    return MBConvNet(widths, depths, num_classes, expand, conv_stats,
                     dw_grad, kernel_sizes, se_ratio)
