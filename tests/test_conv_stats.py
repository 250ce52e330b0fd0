"""conv_stats off the GPU: the composition on CPU tensors, unchanged module
structure, and the host-only launch plan."""

import pytest
import torch

from msbn import ops
from msbn.models import resnet50
from msbn.nn import SyncBatchNorm
from msbn.nn.fused import SyncBatchNormAct2d, conv1x1_bn_act


@pytest.mark.parametrize("act", [True, False])
def test_cpu_tensors_run_the_composition(act):
    torch.manual_seed(0)
    x = torch.randn(2, 16, 5, 5).contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(16, 24, 1, bias=False)
    make = SyncBatchNormAct2d if act else SyncBatchNorm
    bn, ref_bn = make(24), make(24)
    assert torch.equal(conv1x1_bn_act(conv, bn, x), ref_bn(conv(x)))
    assert torch.equal(bn.running_mean, ref_bn.running_mean)
    assert int(bn.num_batches_tracked) == 1
    assert ops.conv1x1_stats(x, conv.weight) == (None, None, 0)


def test_state_dict_keys_unchanged():
    plain = resnet50(fused=True)
    model = resnet50(fused=True, conv_stats=True)
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in model.named_modules()] == \
        [n for n, _ in plain.named_modules()]
    assert model.layer1[0].conv_stats and not plain.layer1[0].conv_stats
    assert not resnet50(conv_stats=True).layer1[0].conv_stats  # needs fused


@pytest.mark.parametrize("cin,cout,rows,want", [
    (64, 256, 300, dict(path="mfma", slab=128, nslabs=2, k_trips=1,
                        row_tile=128, nchunks=3, tiles_per_block=1)),
    (2048, 512, 200, dict(path="mfma", slab=32, nslabs=16, k_trips=16)),
    (12, 16, 50, dict(path="ineligible")),
    (2312, 16, 50, dict(path="ineligible")),  # no 32-column slab fits the LDS
])
def test_launch_plan_answers_for_cpu_tensors(cin, cout, rows, want):
    x = torch.zeros(1, cin, 1, rows, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w = torch.zeros(cout, cin, 1, 1, dtype=torch.bfloat16)
    plan = ops.launch_plan("conv1x1_stats", x, (w,))
    assert {k: plan[k] for k in want} == want, plan
    assert ops.launch_plan("conv1x1_stats", x.float(), (w,))["path"] == \
        "ineligible"
