"""ResNet family for the msbn benchmarks (BASELINE.json configs 2-3).

Hand-written (torchvision is not installed in this environment); standard
ResNet v1 architecture with msbn BatchNorm modules so that
``convert_sync_batchnorm`` swaps them for the RCCL-synced version.

``fused=True`` builds the same architecture with the fused
SyncBatchNormAct2d epilogues (bn+relu and bn+add+relu execute as single
kernels; identical math — msbn/nn/fused.py).  Fused models are already
sync-capable; convert_sync_batchnorm leaves them unchanged.
"""

from typing import List, Type, Union

import torch
import torch.nn as nn

from msbn.nn import BatchNorm2d, SyncBatchNorm
from msbn.nn.fused import (SyncBatchNormAct2d, bn_act_maxpool,
                           bn_add_bn_act)


def conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)


def conv1x1(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, 1, stride=stride, bias=False)


def _norm(planes, fused):
    # plain BN slot (no activation): sync-capable when fused, convertible else
    return SyncBatchNorm(planes) if fused else BatchNorm2d(planes)


def _split(x):
    # a block's input: a tensor, or the (main, skip) pair of a forking block
    return x if isinstance(x, tuple) else (x, x)


def _last_bn(bn, x, identity, fork):
    """A block's closing bn(+add)+relu.  ``fork``: the output feeds the next
    block twice (its conv1 and its skip path), so return it as a (main, skip)
    pair whose two gradients come back to this BN unsummed and are added
    inside its backward reduce kernel (msbn/nn/fused.py) instead of by an
    eager add over the whole tensor."""
    if not fork:
        return bn(x, residual=identity)
    if isinstance(bn, SyncBatchNormAct2d):
        return bn(x, residual=identity, fork=True)
    # slot was swapped for another module (freeze_batchnorm): one gradient
    y = bn(x, residual=identity)
    return y, y


def _dual_downsample(block):
    """True when the block's skip path is exactly (Conv2d, SyncBatchNorm)
    and the dual BN route is asked for: its BatchNorm then runs inside the
    closing BN's kernels (msbn/nn/fused.py bn_add_bn_act), which falls back
    to the composition itself for anything it does not take."""
    d = block.downsample
    return (
        block.fused and getattr(block, "dual_bn", False)
        and type(d) is nn.Sequential and len(d) == 2
        and type(d[0]) is nn.Conv2d and type(d[1]) is SyncBatchNorm
        and not (d._forward_hooks or d._forward_pre_hooks
                 or d._backward_hooks or d._backward_pre_hooks)
    )


def _skip_path(block, skip):
    """``(identity, x_d)`` of a block.  On the dual route the skip path stops
    after its conv (where it has always run, ahead of conv1): ``identity`` is
    None and ``x_d`` goes to ``_close`` unnormalised."""
    if _dual_downsample(block):
        return None, block.downsample[0](skip)
    if block.downsample is not None:
        return block.downsample(skip), None
    return skip, None


def _close(block, bn, x, identity, x_d):
    """The block's closing bn(+add)+relu over the conv output ``x``."""
    fork = getattr(block, "fork", False)
    if identity is None:
        if isinstance(bn, SyncBatchNormAct2d):
            return bn_add_bn_act(bn, block.downsample[1], x, x_d, fork)
        identity = block.downsample[1](x_d)
    return _last_bn(bn, x, identity, fork)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, planes, stride=1, downsample=None, fused=False,
                 fork=False, gate_bits=True, dual_bn=True):
        super().__init__()
        self.fused = fused
        # fused only: return the output as a (main, skip) pair (see _last_bn);
        # off by default, so a stand-alone block maps tensor -> tensor
        self.fork = fork and fused
        # fused, with a (Conv2d, SyncBatchNorm) downsample: its BatchNorm
        # runs inside bn2's kernels (_dual_downsample); needs the gate bits
        self.dual_bn = dual_bn and gate_bits and fused
        self.conv1 = conv3x3(cin, planes, stride)
        self.conv2 = conv3x3(planes, planes)
        self.downsample = downsample
        if fused:
            self.bn1 = SyncBatchNormAct2d(planes, relu=True)
            # takes the residual; gate_bits: its backward reads one stored
            # bit per element where it re-read the residual (fused.py)
            self.bn2 = SyncBatchNormAct2d(planes, relu=True,
                                          gate_bits=gate_bits)
        else:
            self.bn1 = BatchNorm2d(planes)
            self.bn2 = BatchNorm2d(planes)
            self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        x, skip = _split(x)
        identity, x_d = _skip_path(self, skip)
        if self.fused:
            out = self.bn1(self.conv1(x))
            return _close(self, self.bn2, self.conv2(out), identity, x_d)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, planes, stride=1, downsample=None, fused=False,
                 fork=False, gate_bits=True, dual_bn=True):
        super().__init__()
        self.fused = fused
        self.fork = fork and fused  # as in BasicBlock
        self.dual_bn = dual_bn and gate_bits and fused  # as in BasicBlock
        self.conv1 = conv1x1(cin, planes)
        self.conv2 = conv3x3(planes, planes, stride)
        self.conv3 = conv1x1(planes, planes * self.expansion)
        self.downsample = downsample
        if fused:
            self.bn1 = SyncBatchNormAct2d(planes, relu=True)
            self.bn2 = SyncBatchNormAct2d(planes, relu=True)
            self.bn3 = SyncBatchNormAct2d(planes * self.expansion, relu=True,
                                          gate_bits=gate_bits)  # as BasicBlock
        else:
            self.bn1 = BatchNorm2d(planes)
            self.bn2 = BatchNorm2d(planes)
            self.bn3 = BatchNorm2d(planes * self.expansion)
            self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        x, skip = _split(x)
        identity, x_d = _skip_path(self, skip)
        if self.fused:
            out = self.bn1(self.conv1(x))
            out = self.bn2(self.conv2(out))
            return _close(self, self.bn3, self.conv3(out), identity, x_d)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(
        self,
        block: Type[Union[BasicBlock, Bottleneck]],
        layers: List[int],
        num_classes: int = 1000,
        in_chans: int = 3,
        fused: bool = False,
        fork_grads: bool = True,
        gate_bits: bool = True,
        dual_bn: bool = True,
    ):
        super().__init__()
        self.fused = fused
        # fused models with gate bits: the first block of a stage runs its
        # downsample BatchNorm inside the closing BN's kernels (dual BN,
        # msbn/nn/fused.py bn_add_bn_act).  Same math either way; False
        # keeps the two layers apart.
        self.dual_bn = dual_bn and gate_bits and fused
        # fused models: each block's closing BN keeps its activation gate as
        # one bit per element instead of re-reading the residual in backward.
        # Same math either way; False keeps the recomputing route.
        self.gate_bits = gate_bits and fused
        # fused models: every block whose output feeds another block hands
        # it over as a (main, skip) pair (_last_bn).  Same math either way;
        # False keeps autograd's own gradient add at each fork.
        self.fork_grads = fork_grads and fused
        # fused models: bn1 + relu + maxpool run as one layer (_stem)
        self.stem_pool = fused
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_chans, 64, 7, stride=2, padding=3, bias=False)
        if fused:
            self.bn1 = SyncBatchNormAct2d(64, relu=True)
        else:
            self.bn1 = BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2,
                                       fork_last=False)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")

    def _make_layer(self, block, planes, blocks, stride=1, fork_last=True):
        # fork_last: the layer's last block feeds the next layer's first
        fork = [self.fork_grads] * (blocks - 1) + [self.fork_grads
                                                   and fork_last]
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                conv1x1(self.inplanes, planes * block.expansion, stride),
                _norm(planes * block.expansion, self.fused),
            )
        layers = [block(self.inplanes, planes, stride, downsample,
                        fused=self.fused, fork=fork[0],
                        gate_bits=self.gate_bits, dual_bn=self.dual_bn)]
        self.inplanes = planes * block.expansion
        for i in range(1, blocks):
            layers.append(block(self.inplanes, planes, fused=self.fused,
                                fork=fork[i], gate_bits=self.gate_bits))
        return nn.Sequential(*layers)

    def _stem(self, x):
        x = self.conv1(x)
        if self.fused:
            # bn1 + relu + maxpool as one layer where eligible (training-mode
            # SyncBatchNormAct2d, MaxPool2d(3, 2, 1), channels-last on the
            # GPU), else exactly maxpool(bn1(x)).  With fork_grads the result
            # goes to layer1[0] as a (main, skip) pair, so its conv1 and skip
            # gradients reach the stem's backward kernels unsummed.
            # stem_pool = False keeps the composition (same results).
            if (getattr(self, "stem_pool", True)
                    and isinstance(self.bn1, SyncBatchNormAct2d)):
                return bn_act_maxpool(self.bn1, self.maxpool, x,
                                      fork=getattr(self, "fork_grads", False))
            return self.maxpool(self.bn1(x))
        return self.maxpool(self.relu(self.bn1(x)))

    def forward_features(self, x):
        x = self._stem(x)
        # a forking layer hands its (main, skip) pair to the next layer; the
        # caller gets plain tensors (main: an extra consumer's gradient is
        # summed there by autograd as before)
        c2 = self.layer1(x)
        c3 = self.layer2(c2)
        c4 = self.layer3(c3)
        c5 = self.layer4(c4)
        return _split(c2)[0], _split(c3)[0], _split(c4)[0], _split(c5)[0]

    def forward(self, x):
        _, _, _, c5 = self.forward_features(x)
        out = self.avgpool(c5).flatten(1)
        return self.fc(out)


def resnet18(num_classes: int = 1000, fused: bool = False,
             fork_grads: bool = True, gate_bits: bool = True,
             dual_bn: bool = True) -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, fused=fused,
                  fork_grads=fork_grads, gate_bits=gate_bits,
                  dual_bn=dual_bn)


def resnet50(num_classes: int = 1000, fused: bool = False,
             fork_grads: bool = True, gate_bits: bool = True,
             dual_bn: bool = True) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, fused=fused,
                  fork_grads=fork_grads, gate_bits=gate_bits,
                  dual_bn=dual_bn)
