"""dwconv3x3_stats off the GPU: the host-only launch plan, and the
composition on CPU tensors (layer and mbconv_net)."""

import pytest
import torch

from msbn import ops
from msbn.models import mbconv_net
from msbn.nn import SyncBatchNorm
from msbn.nn.fused import SyncBatchNormAct2d, dwconv3x3_bn_act

BF16 = torch.bfloat16
FIELDS = {"path", "V", "lpr", "ctiles", "strip", "items", "chunk_items",
          "nchunks", "trips", "flush_every", "finalize_trips"}


def _xw(n, c, h, w, dtype=BF16, cw=None):
    x = torch.zeros(n, c, h, w, dtype=dtype) \
        .contiguous(memory_format=torch.channels_last)
    return x, torch.zeros(c if cw is None else cw, 1, 3, 3, dtype=dtype)


@pytest.mark.parametrize("kind,shape,want", [
    ("dwconv3x3_stats", (2, 64, 20, 20), dict(
        V=8, lpr=8, ctiles=1, strip=8, items=2 * 20 * 3, flush_every=64)),
    ("dwconv3x3s2_stats", (2, 64, 20, 20), dict(
        V=8, lpr=8, ctiles=1, strip=8, items=2 * 10 * 2)),
    ("dwconv3x3s2_stats", (1, 1152, 7, 7), dict(
        lpr=16, ctiles=9, items=4, nchunks=1, trips=1, finalize_trips=1)),
])
def test_launch_plan_answers_for_cpu_tensors(kind, shape, want):
    x, w = _xw(*shape)
    plan = ops.launch_plan(kind, x, (w,))
    assert plan["path"] == "dwconv" and set(plan) == FIELDS, plan
    assert {k: plan[k] for k in want} == want, plan
    rpi = 256 // plan["lpr"]
    assert plan["nchunks"] == -(-plan["items"] // plan["chunk_items"])
    assert plan["trips"] == -(-plan["chunk_items"] // rpi)


@pytest.mark.parametrize("kind", ["fp32", "nchw", "c_12", "multiplier_2",
                                  "kernel_5", "weight_dtype"])
def test_launch_plan_declines(kind):
    x, w = _xw(2, 12 if kind == "c_12" else 16, 5, 5,
               torch.float32 if kind == "fp32" else BF16,
               32 if kind == "multiplier_2" else None)
    if kind == "nchw":
        x = x.contiguous()
    if kind == "kernel_5":
        w = torch.zeros(16, 1, 5, 5, dtype=BF16)
    if kind == "weight_dtype":
        w = w.half()
    for k in ("dwconv3x3_stats", "dwconv3x3s2_stats"):
        assert ops.launch_plan(k, x, (w,))["path"] == "ineligible"


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("act", [True, False])
def test_cpu_tensors_run_the_composition(act, stride):
    torch.manual_seed(0)
    x = torch.randn(2, 16, 5, 7).contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(16, 16, 3, stride, 1, groups=16, bias=False)

    def make():
        return SyncBatchNormAct2d(16, act="silu") if act else SyncBatchNorm(16)

    bn, ref_bn = make(), make()
    assert torch.equal(dwconv3x3_bn_act(conv, bn, x), ref_bn(conv(x)))
    assert torch.equal(bn.running_var, ref_bn.running_var)
    assert int(bn.num_batches_tracked) == 1
    assert ops.dwconv3x3_stats(x, conv.weight, stride) == (None, None, 0)


def test_mbconv_net_flag_changes_nothing_on_the_cpu():
    torch.manual_seed(1)
    plain = mbconv_net((8, 16), (1, 2), num_classes=5)
    model = mbconv_net((8, 16), (1, 2), num_classes=5, conv_stats=True)
    assert list(model.state_dict()) == list(plain.state_dict())
    model.load_state_dict(plain.state_dict())
    x = torch.randn(2, 3, 16, 16)
    assert torch.equal(model(x), plain(x))
    assert model.blocks[0].skip and not model.blocks[1].skip
    assert model.blocks[1].conv2.stride == (2, 2)
