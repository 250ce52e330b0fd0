"""GPU numerics of the fused BN(+add)+SiLU kernels (the kActSilu
instantiations of the two-stage and frozen families) against the fp64
formulas and shared checks of silu_ref.py."""

import functools

import pytest
import torch
import torch.nn as nn

import msbn
from msbn.nn import FrozenBatchNorm2d, SyncBatchNormAct2d, fuse_bn_act
from silu_ref import check_module, check_ops, close, draw, make_module, tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
draw = functools.lru_cache(maxsize=None)(draw)  # drawn once, never modified
layouts = pytest.mark.parametrize("channels_last", [False, True])
residual = pytest.mark.parametrize("with_res", [False, True])


@residual
@layouts
@pytest.mark.parametrize("shape,dtype", [
    ((4, 32, 9, 9), F32), ((4, 32, 9, 9), BF16),  # flat NCHW; vector NHWC
    ((2, 24, 8, 8), F32), ((2, 24, 8, 8), BF16),  # vectorised NCHW
    ((2, 24, 8, 8), torch.float16),
    ((3, 20, 7, 7), F32), ((3, 20, 7, 7), BF16),  # C % bf16 pack != 0
])
def test_silu_ops_vs_fp64(shape, dtype, channels_last, with_res):
    check_ops(draw(shape, dtype), dtype, with_res, DEV, channels_last)


@layouts
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_silu_saturation(dtype, channels_last):
    """z from -138 to 198, far past where exp(-z) overflows / underflows in
    fp32: the same tolerances, finite everywhere, y = z on the far positive
    side and 0 on the far negative."""
    y, gm, dx, z = check_ops(draw((2, 8, 4, 4), dtype, 20.0), dtype, False,
                             DEV, channels_last)
    assert all(torch.isfinite(t).all() for t in (y, gm, dx))
    hi, lo = (z > 100).to(DEV), (z < -100).to(DEV)
    assert hi.any() and lo.any()
    close(y[hi], z[hi.cpu()], **tol(dtype, 1e-5))
    assert (y[lo] == 0).all() and (gm[lo] == 0).all()


@residual
@layouts
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", [(3, 20, 7, 7), (2, 24, 8, 8)])
def test_silu_frozen_backward_kernel(shape, dtype, channels_last, with_res):
    check_ops(draw(shape, dtype), dtype, with_res, DEV, channels_last,
              frozen=True)


@pytest.mark.parametrize("cls,training,with_res,fork", [
    (SyncBatchNormAct2d, True, False, False),
    (SyncBatchNormAct2d, True, True, False),
    (SyncBatchNormAct2d, True, True, True),   # the fork fold
    (SyncBatchNormAct2d, False, False, False),
    (SyncBatchNormAct2d, False, True, True),
    (FrozenBatchNorm2d, False, True, False),
])
@pytest.mark.parametrize("dtype,channels_last", [(F32, False), (BF16, True)])
def test_silu_module_vs_fp64_autograd(dtype, channels_last, cls, training,
                                      with_res, fork):
    """Training and eval mode against F.silu(bn(x) [+ res]) under fp64
    autograd.  (4, 64, 8, 8) NCHW is a plane the single-launch kernels would
    take: SiLU must not."""
    d = draw((4, 64, 8, 8), dtype)
    check_module(make_module(cls, d, training, DEV), d, dtype, with_res, DEV,
                 channels_last, fork)


def test_fused_silu_stack_train_step():
    """fuse_bn_act on Conv, BN, SiLU stacks: one fused module per pair, and
    one bf16 channels-last train step that matches the unfused model."""
    def net():
        return msbn.convert_sync_batchnorm(nn.Sequential(*(
            nn.Sequential(nn.Conv2d(i, o, 3, padding=1, bias=False),
                          nn.BatchNorm2d(o), nn.SiLU(inplace=True))
            for i, o in ((3, 16), (16, 24)))))

    torch.manual_seed(5)
    a, b = net(), net()
    b.load_state_dict(a.state_dict())
    b = fuse_bn_act(b)
    fused = [m for m in b.modules() if isinstance(m, SyncBatchNormAct2d)]
    assert len(fused) == 2 and all(m.act == "silu" for m in fused)
    assert not any(isinstance(m, nn.SiLU) for m in b.modules())
    x = torch.randn(4, 3, 12, 12, device=DEV).bfloat16().contiguous(
        memory_format=torch.channels_last)
    outs = []
    for m in (a, b):
        m = m.to(DEV).bfloat16().to(memory_format=torch.channels_last)
        for bn in m.modules():  # bf16 activations, fp32 channel parameters
            if isinstance(bn, msbn.nn.SyncBatchNorm):
                bn.float()
        y = m.train()(x)
        y.float().square().mean().backward()
        outs.append([y] + [p.grad for p in m.parameters()])
    for p, q in zip(*outs):
        torch.testing.assert_close(p, q, atol=2e-2, rtol=2e-2)
