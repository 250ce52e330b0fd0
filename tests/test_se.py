"""Squeeze-excite on the CPU: the module, the factorised backward of
SyncBatchNormSiluSEFunction through the reference ops, and the routes that
must stay the composition."""

import pytest
import torch
import torch.nn.functional as F

from msbn.models import mbconv_net
from msbn.nn import SqueezeExcite
from msbn.nn.fused import (SyncBatchNormAct2d, SyncBatchNormSiluSEFunction,
                           bn_silu_se, bn_silu_se_eligible, dwconv3x3_bn_act)


def test_module_keys_and_formula():
    se = SqueezeExcite(12, 5).double()
    assert sorted(se.state_dict()) == ["fc1.bias", "fc1.weight", "fc2.bias",
                                      "fc2.weight"]
    assert se.fc1.weight.shape == (5, 12, 1, 1)
    x = torch.randn(3, 12, 4, 5, dtype=torch.float64)
    s = x.mean((2, 3))
    h = F.silu(s @ se.fc1.weight.view(5, 12).t() + se.fc1.bias)
    g = torch.sigmoid(h @ se.fc2.weight.view(12, 5).t() + se.fc2.bias)
    torch.testing.assert_close(se(x), x * g.view(3, 12, 1, 1))


def test_function_matches_autograd_of_the_composition():
    """fp64 CPU tensors through the reference stage ops: pins sum_dy =
    sum_n(g*P1 + dpool*Q1) (and sum_dy_xmu) independently of any kernel.
    The statistics ops hand mean / invstd over in fp32, hence 1e-5."""
    torch.manual_seed(3)
    N, C, Cr = 3, 8, 3
    lv = {k: v.double().requires_grad_(True) for k, v in dict(
        y=torch.randn(N, C, 5, 7) * 2 + 0.5, gamma=torch.rand(C) + 0.5,
        beta=torch.randn(C), w1=torch.randn(Cr, C, 1, 1) / 2,
        b1=torch.randn(Cr), w2=torch.randn(C, Cr, 1, 1), b2=torch.randn(C),
    ).items()}
    gout = torch.randn(N, C, 5, 7, dtype=torch.float64)

    def composition(y, gamma, beta, w1, b1, w2, b2):
        a = F.silu(F.batch_norm(y, None, None, gamma, beta, True, 0.0, 1e-5))
        s = a.mean((2, 3), keepdim=True)
        return a * torch.sigmoid(F.conv2d(F.silu(F.conv2d(s, w1, b1)), w2, b2))

    def fused(y, gamma, beta, w1, b1, w2, b2):
        return SyncBatchNormSiluSEFunction.apply(
            y, gamma, beta, None, None, 1e-5, 0.1, None, 1, w1, b1, w2, b2)

    want = composition(**lv)
    want_grads = torch.autograd.grad(want, list(lv.values()), gout)
    got = fused(**lv)
    got_grads = torch.autograd.grad(got, list(lv.values()), gout)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    for k, a, b in zip(lv, got_grads, want_grads):
        assert a.shape == b.shape and a.dtype == b.dtype, k
        torch.testing.assert_close(a, b, atol=1e-5, rtol=1e-5,
                                   msg=lambda m, k=k: k + ": " + m)


@pytest.mark.parametrize("case", ["fp32", "nchw", "eval", "hooks", "se_none"])
def test_ineligible_inputs_take_exactly_the_composition(case):
    torch.manual_seed(5)
    bn, ref_bn = (SyncBatchNormAct2d(8, act="silu") for _ in range(2))
    se = SqueezeExcite(8, 2)
    y = torch.randn(2, 8, 4, 4)
    if case != "nchw":
        y = y.contiguous(memory_format=torch.channels_last)
    if case == "eval":
        bn.eval(), ref_bn.eval()
    if case == "hooks":
        se.register_forward_hook(lambda m, i, o: None)
    if case == "se_none":
        conv = torch.nn.Conv2d(8, 8, 3, 1, 1, groups=8, bias=False)
        got, want = dwconv3x3_bn_act(conv, bn, y, se=None), ref_bn(conv(y))
    else:
        assert not bn_silu_se_eligible(bn, se, y)
        got, want = bn_silu_se(bn, se, y), se(ref_bn(y))
    assert torch.equal(got, want)
    assert torch.equal(bn.running_var, ref_bn.running_var)


def test_mbconv_net_keys():
    plain = mbconv_net((8, 16), (1, 1), num_classes=3)
    assert not any(".se." in k for k in plain.state_dict())
    assert len(plain.state_dict()) == 44
    with_se = mbconv_net((8, 16), (1, 1), num_classes=3, se_ratio=0.25)
    extra = sorted(set(with_se.state_dict()) - set(plain.state_dict()))
    assert extra == [f"blocks.{i}.se.fc{j}.{p}" for i in (0, 1)
                     for j in (1, 2) for p in ("bias", "weight")]
    assert with_se.blocks[1].se.fc1.out_channels == 2  # max(1, int(8 * .25))
    x = torch.randn(2, 3, 16, 16)
    assert with_se.train()(x).shape == (2, 3)
