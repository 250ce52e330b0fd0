"""The 5x5 depthwise route off the GPU: the host-only launch plans, and the
MBConv kernel-size arguments on CPU tensors."""

import pytest
import torch

from msbn import ops
from msbn.models import mbconv_net
from msbn.models.mbconv import MBConv
from msbn.nn.fused import SyncBatchNormAct2d, dwconv5x5_bn_act

BF16 = torch.bfloat16
FIELDS = {"path", "V", "lpr", "ctiles", "tile_h", "tile_w", "strip", "items",
          "chunk_items", "nchunks", "trips", "flush_every", "lds_bytes"}


@pytest.mark.parametrize("kind,shape,want", [
    ("dwconv5x5_stats", (2, 240, 28, 28), dict(
        V=8, lpr=8, ctiles=4, tile_h=16, tile_w=16, strip=8, items=8,
        flush_every=64, finalize_trips=1)),
    ("dwconv5x5s2_stats", (2, 240, 28, 28), dict(
        lpr=8, tile_h=8, tile_w=8, strip=2, items=8, flush_every=16)),
    ("dwconv5x5_dgrad", (1, 1152, 7, 7), dict(
        lpr=16, ctiles=9, tile_h=8, tile_w=16, strip=8, items=1, nchunks=1)),
    ("dwconv5x5s2_dgrad", (1, 64, 20, 20), dict(
        lpr=8, tile_h=16, tile_w=16, items=4, flush_every=25)),
    ("dwconv5x5_wgrad", (1, 1152, 20, 20), dict(
        lpr=16, tile_h=8, tile_w=8, items=9, trips=3, flush_every=64)),
    ("dwconv5x5s2_wgrad", (1, 64, 20, 20), dict(
        lpr=8, tile_h=8, tile_w=8, strip=2, items=4, trips=6)),
])
def test_launch_plans_answer_for_cpu_tensors(kind, shape, want):
    n, c, h, w_ = shape
    s = 2 if "s2_" in kind else 1
    x = torch.zeros(shape, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    w = torch.zeros(c, 1, 5, 5, dtype=BF16)
    gy = torch.zeros(n, c, (h - 1) // s + 1, (w_ - 1) // s + 1, dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    plan = ops.launch_plan(kind, x, (w,) if kind.endswith("stats") else (w, gy))
    extra = set() if kind.endswith("dgrad") else {"finalize_trips"}
    assert plan["path"] == "dwconv" and set(plan) == FIELDS | extra, plan
    assert {k: plan[k] for k in want} == want, plan
    assert plan["nchunks"] == -(-plan["items"] // plan["chunk_items"])
    assert plan["tile_h"] * plan["tile_w"] // plan["strip"] <= \
        256 // plan["lpr"]
    assert 2 * plan["lds_bytes"] <= 160 * 1024  # two blocks per CU
    # a 3x3 weight is not this op's, a 5x5 weight not the 3x3 op's
    w3 = torch.zeros(c, 1, 3, 3, dtype=BF16)
    assert ops.launch_plan(kind, x, (w3, gy))["path"] == "ineligible"
    assert ops.launch_plan("dwconv3x3_stats", x, (w,))["path"] == "ineligible"


@pytest.mark.parametrize("stride", [1, 2])
def test_mbconv_kernel_size_5_runs_the_composition(stride):
    torch.manual_seed(0)
    block = MBConv(8, 8, stride, kernel_size=5, conv_stats=True, dw_grad=True)
    assert block.conv2.kernel_size == (5, 5) and block.conv2.padding == (2, 2)
    x = torch.randn(2, 8, 9, 7)
    y = block(x)
    assert y.shape == (2, 8, (9 - 1) // stride + 1, (7 - 1) // stride + 1)
    bn, ref_bn = (SyncBatchNormAct2d(32, act="silu") for _ in range(2))
    z = torch.randn(2, 32, 9, 7)
    assert torch.equal(dwconv5x5_bn_act(block.conv2, bn, z),
                       ref_bn(block.conv2(z)))
    assert ops.dwconv5x5_stats(z, block.conv2.weight, stride) == \
        (None, None, 0)
    assert ops.dwconv5x5_backward(y, z, block.conv2.weight, stride) == \
        (None, None)


def test_kernel_sizes_default_and_errors():
    plain = mbconv_net((8, 16), (1, 2), num_classes=5)
    same = mbconv_net((8, 16), (1, 2), num_classes=5, kernel_sizes=(3, 3))
    five = mbconv_net((8, 16), (1, 2), num_classes=5, kernel_sizes=(3, 5))
    shapes = {k: v.shape for k, v in plain.state_dict().items()}
    assert shapes == {k: v.shape for k, v in same.state_dict().items()}
    assert list(five.state_dict()) == list(shapes)
    assert plain.blocks[1].conv2.weight.shape[2:] == (3, 3)
    assert five.blocks[0].conv2.weight.shape[2:] == (3, 3)
    assert five.blocks[1].conv2.weight.shape[2:] == (5, 5)
    assert five(torch.randn(2, 3, 16, 16)).shape == (2, 5)
    with pytest.raises(ValueError):
        MBConv(8, 8, kernel_size=4)
    with pytest.raises(ValueError):
        mbconv_net((8, 16), (1, 2), kernel_sizes=(3,))
