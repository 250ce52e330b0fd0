"""Grouped BN off the GPU: the loop on CPU tensors, unchanged model structure
and the host-only launch plans."""

import pytest
import torch

from msbn import ops
from msbn.models.retinanet import RetinaNet
from msbn.nn import BatchNorm2d, SyncBatchNorm
from msbn.nn.fused import SyncBatchNormAct2d, bn_act_grouped

PLANES = [(13, 21), (7, 11), (4, 6), (2, 3), (1, 2)]


def _levels(dtype=torch.float32, n=2, c=16):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn((n, c, h, w), generator=g) + 3 * s).to(dtype)
            .contiguous(memory_format=torch.channels_last)
            for s, (h, w) in enumerate(PLANES)]


@pytest.mark.parametrize("make,relu", [(SyncBatchNorm, None),
                                       (SyncBatchNorm, True),
                                       (BatchNorm2d, True),
                                       (SyncBatchNormAct2d, None)])
def test_cpu_tensors_run_the_loop(make, relu):
    xs = _levels()
    bn, ref_bn = make(16), make(16)
    got = bn_act_grouped(bn, xs, relu=relu)
    want = [ref_bn(x) for x in xs]
    if relu and make is not SyncBatchNormAct2d:
        want = [torch.relu(y) for y in want]
    assert isinstance(got, list) and len(got) == len(xs)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(bn.running_mean, ref_bn.running_mean)
    assert torch.equal(bn.running_var, ref_bn.running_var)
    assert int(bn.num_batches_tracked) == len(xs)


def test_retinanet_structure_unchanged():
    plain, model = RetinaNet(), RetinaNet(grouped_heads=True)
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in model.named_modules()] == \
        [n for n, _ in plain.named_modules()]
    assert model.cls_head.grouped and model.box_head.grouped
    assert not plain.cls_head.grouped


def test_launch_plans_answer_for_cpu_tensors():
    xs = _levels(torch.bfloat16)
    dys = [torch.zeros_like(x) for x in xs]
    rows = [2 * h * w for h, w in PLANES]
    for kind in ("stats_grouped", "bwd_reduce_grouped"):
        others = xs[1:] + (dys if kind.startswith("bwd") else [])
        plan = ops.launch_plan(kind, xs[0], others)
        assert plan["path"] == "nhwc" and plan["S"] == 5 and plan["V"] == 8
        assert plan["chunk_rows"] == 128 and plan["ctiles"] == 1, plan
        assert plan["nchunks"] == [-(-r // 128) for r in rows] == \
            [5, 2, 1, 1, 1]
        assert plan["first_block"] == [0, 5, 7, 8, 9]
        assert plan["total_chunks"] == 10 and plan["trips"] == 4
    for kind in ("elemt_grouped", "bwd_elemt_grouped"):
        others = xs[1:] + (dys if kind.startswith("bwd") else [])
        plan = ops.launch_plan(kind, xs[0], others)
        assert plan["path"] == "nhwc" and not plan["multi_trip"]
        assert plan["blocks"] == [-(-r * 2 // 256) for r in rows]
        assert plan["grid"] == sum(plan["blocks"]) and plan["trips"] == 1
    assert ops.launch_plan("stats_grouped", xs[0].float(), xs[1:])["path"] \
        == "ineligible"
    assert ops.launch_plan("bwd_elemt_grouped", xs[0], xs[1:])["path"] \
        == "ineligible"  # the gradients are part of the launch
