"""FrozenBatchNorm2d / freeze_batchnorm / frozen ops: CPU semantics.

The GPU kernels are covered by test_gpu_frozen_bn.py; here the module layer,
the converters and the pure-torch reference ops are checked against
torch.nn.BatchNorm2d in eval mode and against autograd of the composed
expression.
"""

import copy

import pytest
import torch
import torch.nn as nn

import msbn
from msbn.nn import FrozenBatchNorm2d, freeze_batchnorm
from msbn.nn.batchnorm import _NormBase
from msbn.nn.frozen import FrozenBatchNormActFunction
from msbn.ops import _reference as ref


def _torch_bn(C=8, seed=0):
    """An eval-mode torch BN with non-trivial stats and affine."""
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g).abs() + 0.1)
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(7)
    return bn.eval()


def _frozen_like(bn):
    m = FrozenBatchNorm2d(bn.num_features, bn.eps)
    m.load_state_dict(bn.state_dict(), strict=True)
    return m


def _fwd_dx(m, x):
    x = x.clone().requires_grad_(True)
    y = m(x)
    g = torch.arange(y.numel(), dtype=y.dtype).reshape(y.shape).cos()
    (dx,) = torch.autograd.grad(y, x, g)
    return y.detach(), dx


@pytest.mark.parametrize("train_mode", [False, True])
def test_matches_torch_eval_bn(train_mode):
    bn = _torch_bn()
    m = _frozen_like(bn)
    if train_mode:
        m.train()
    x = torch.randn(4, 8, 5, 5, generator=torch.Generator().manual_seed(1))
    y, dx = _fwd_dx(m, x)
    yref, dxref = _fwd_dx(bn, x)
    torch.testing.assert_close(y, yref, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(dx, dxref, atol=1e-6, rtol=1e-6)


def test_train_mode_never_updates_stats_and_has_no_parameters():
    bn = _torch_bn()
    m = _frozen_like(bn).train()
    before = copy.deepcopy(m.state_dict())
    m(torch.randn(4, 8, 5, 5) * 3 + 2)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert int(m.num_batches_tracked) == 7
    assert list(m.parameters()) == []
    assert isinstance(m, _NormBase)
    assert set(m.state_dict()) == set(bn.state_dict())


def test_state_dict_round_trips():
    bn = _torch_bn()
    m = _frozen_like(bn)  # strict load from torch.nn.BatchNorm2d
    for k, v in bn.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k

    # torchvision-style frozen-BN dict: no num_batches_tracked
    sd = {k: v.clone() for k, v in bn.state_dict().items()
          if k != "num_batches_tracked"}
    m2 = FrozenBatchNorm2d(8)
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.running_var, bn.running_var)
    assert torch.equal(m2.weight, bn.weight)
    # ... also as a child module with a prefix
    seq = nn.Sequential(nn.Conv2d(3, 8, 1), FrozenBatchNorm2d(8))
    sd_seq = {"0.weight": seq[0].weight.detach(), "0.bias": seq[0].bias.detach()}
    sd_seq.update({"1." + k: v for k, v in sd.items()})
    seq.load_state_dict(sd_seq, strict=True)
    assert torch.equal(seq[1].running_mean, bn.running_mean)

    # and back into a trainable msbn BatchNorm2d
    back = msbn.nn.BatchNorm2d(8)
    back.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(back.weight, bn.weight)
    assert torch.equal(back.running_mean, bn.running_mean)
    assert int(back.num_batches_tracked) == 7


def _randomize_bn(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    for mod in model.modules():
        if isinstance(mod, (_NormBase, nn.modules.batchnorm._BatchNorm)):
            with torch.no_grad():
                C = mod.num_features
                mod.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
                if mod.weight is not None:
                    mod.weight.copy_(torch.rand(C, generator=g) + 0.5)
                    mod.bias.copy_(torch.randn(C, generator=g) * 0.1)


@pytest.mark.parametrize("fused", [False, True])
def test_freeze_batchnorm_resnet18(fused):
    torch.manual_seed(0)
    model = msbn.models.resnet18(num_classes=10, fused=fused)
    _randomize_bn(model)
    model.eval()
    relu_before = {n: bool(getattr(m, "relu", False))
                   for n, m in model.named_modules()
                   if isinstance(m, _NormBase)}
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        want = model(x)
    frozen = freeze_batchnorm(model)
    bns = {n: m for n, m in frozen.named_modules()
           if isinstance(m, (_NormBase, nn.modules.batchnorm._BatchNorm))}
    assert set(bns) == set(relu_before) and len(bns) == 20
    for n, m in bns.items():
        assert isinstance(m, FrozenBatchNorm2d), n
        assert m.relu == relu_before[n], n
    assert any(relu_before.values()) == fused
    frozen.train()  # frozen BN ignores the mode
    with torch.no_grad():
        got = frozen(x)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    assert not any(isinstance(m, _NormBase) and list(m.parameters())
                   for m in frozen.modules())


def test_freeze_batchnorm_sources():
    # torch.nn family incl. 1d / 3d / SyncBatchNorm; tensors are shared
    for src, shape in [(nn.BatchNorm1d(6), (4, 6)),
                       (nn.BatchNorm3d(6), (2, 6, 3, 2, 2)),
                       (nn.SyncBatchNorm(6), (2, 6, 3, 3)),
                       (msbn.nn.SyncBatchNorm(6), (2, 6, 3, 3)),
                       (msbn.nn.SyncBatchNormAct2d(6), (2, 6, 3, 3))]:
        _randomize_bn(src)
        fz = freeze_batchnorm(src)
        assert isinstance(fz, FrozenBatchNorm2d)
        assert fz.running_mean is src.running_mean
        assert fz.weight.data_ptr() == src.weight.data_ptr()
        assert not fz.weight.requires_grad
        x = torch.randn(shape)
        want = torch.nn.functional.batch_norm(
            x, src.running_mean, src.running_var, src.weight, src.bias,
            False, 0.0, src.eps)
        if getattr(src, "relu", False):
            want = want.relu()
        torch.testing.assert_close(fz(x), want.detach(), atol=1e-6, rtol=1e-6)

    # affine=False -> ones / zeros buffers
    src = nn.BatchNorm2d(6, affine=False)
    _randomize_bn(src)
    fz = freeze_batchnorm(nn.Sequential(src))[0]
    assert torch.equal(fz.weight, torch.ones(6))
    assert torch.equal(fz.bias, torch.zeros(6))
    x = torch.randn(2, 6, 3, 3)
    torch.testing.assert_close(fz(x), src.eval()(x), atol=1e-6, rtol=1e-6)

    with pytest.raises(ValueError, match="track_running_stats"):
        freeze_batchnorm(nn.BatchNorm2d(6, track_running_stats=False))


def test_convert_sync_batchnorm_leaves_frozen():
    model = nn.Sequential(nn.Conv2d(3, 8, 1), FrozenBatchNorm2d(8),
                          nn.BatchNorm2d(8))
    frozen = model[1]
    out = msbn.convert_sync_batchnorm(model)
    assert out[1] is frozen
    assert isinstance(out[2], msbn.nn.SyncBatchNorm)
    assert msbn.convert_sync_batchnorm(frozen) is frozen


def test_fuse_bn_act_fuses_frozen_relu():
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), _frozen_like(_torch_bn()),
                        nn.ReLU())
    model = nn.Sequential(seq)
    x = torch.randn(2, 3, 6, 6)
    want = model(x)
    fused = msbn.nn.fuse_bn_act(model)
    assert len(fused[0]) == 2
    assert isinstance(fused[0][1], FrozenBatchNorm2d) and fused[0][1].relu
    torch.testing.assert_close(fused(x), want, atol=1e-6, rtol=1e-6)


def test_convert_to_torch_batchnorm_frozen():
    from msbn.models import convert_to_torch_batchnorm

    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 8, 1), _frozen_like(_torch_bn()))
    x = torch.randn(2, 3, 5, 5)
    want = model(x)
    stock = convert_to_torch_batchnorm(model)
    bn = stock[1]
    assert type(bn) is nn.BatchNorm2d
    assert not bn.training
    assert not bn.weight.requires_grad and not bn.bias.requires_grad
    torch.testing.assert_close(stock(x), want, atol=1e-6, rtol=1e-6)
    assert int(bn.num_batches_tracked) == 7  # eval: no update

    with pytest.raises(ValueError, match="relu=True"):
        convert_to_torch_batchnorm(
            nn.Sequential(FrozenBatchNorm2d(8, relu=True)))


def test_retinanet_frozen_backbone_build():
    torch.manual_seed(0)
    base = msbn.models.retinanet(num_classes=3)
    base_names = [n for n, _ in base.named_parameters()]
    # the default model is today's: backbone BN affine params are present
    assert "backbone.bn1.weight" in base_names
    assert "backbone.layer4.2.bn3.bias" in base_names
    n_bn = sum(isinstance(m, _NormBase) for m in base.backbone.modules())
    assert n_bn == 53
    assert len(base_names) == 3 * 53 + 2 * (3 + 3 + 2) + 2 * (3 * 4 + 2)

    for fused in (False, True):
        m = msbn.models.retinanet(num_classes=3, frozen_backbone=True,
                                  fused_backbone=fused)
        bbn = [x for x in m.backbone.modules() if isinstance(x, _NormBase)]
        assert len(bbn) == 53
        assert all(isinstance(x, FrozenBatchNorm2d) for x in bbn)
        assert not any(list(x.parameters()) for x in bbn)
        assert any(x.relu for x in bbn) == fused
        names = [n for n, _ in m.named_parameters()]
        # exactly the backbone BN weight/bias pairs are gone
        assert len(names) == len(base_names) - 2 * 53
        assert set(names) <= set(base_names)
        for head in (m.cls_head, m.box_head):
            hbn = [x for x in head.modules() if isinstance(x, _NormBase)]
            assert len(hbn) == 4
            assert all(not isinstance(x, FrozenBatchNorm2d) and
                       len(list(x.parameters())) == 2 for x in hbn)
        # sync conversion still reaches the heads and skips the backbone
        s = msbn.convert_sync_batchnorm(m)
        assert isinstance(s.cls_head.tower[1], msbn.nn.SyncBatchNorm)
        assert isinstance(s.backbone.bn1, FrozenBatchNorm2d)


def _composed(x, res, scale, shift, relu):
    shape = [1, -1] + [1] * (x.dim() - 2)
    z = x * scale.reshape(shape) + shift.reshape(shape)
    if res is not None:
        z = z + res
    return z.relu() if relu else z


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_reference_frozen_backward_matches_autograd(relu, with_res):
    g = torch.Generator().manual_seed(5)
    shape = (3, 6, 4, 5)
    C = shape[1]
    x = (torch.randn(shape, generator=g) * 2 + 0.5).requires_grad_(True)
    res = torch.randn(shape, generator=g).requires_grad_(True) \
        if with_res else None
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    w = torch.randn(C, generator=g).abs() + 0.1
    b = torch.randn(C, generator=g)
    dy = torch.randn(shape, generator=g)

    coefs = ref.bn_frozen_coefs(rm, rv, 1e-5, w, b)
    assert coefs.dtype == torch.float32 and coefs.shape == (2 * C,)
    scale = w / torch.sqrt(rv + 1e-5)
    torch.testing.assert_close(coefs[:C], scale, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(coefs[C:], b - rm * scale, atol=1e-6, rtol=1e-6)

    y = _composed(x, res, coefs[:C], coefs[C:], relu)
    grads = torch.autograd.grad(y, [x] + ([res] if with_res else []), dy)
    dx, dres = ref.batch_norm_frozen_backward_elemt(
        dy, x.detach() if relu else None,
        res.detach() if (relu and with_res) else None, coefs, relu, True,
        with_res)
    torch.testing.assert_close(dx, grads[0], atol=1e-6, rtol=1e-6)
    if with_res:
        torch.testing.assert_close(dres, grads[1], atol=1e-6, rtol=1e-6)
    else:
        assert dres is None
    only_res = ref.batch_norm_frozen_backward_elemt(
        dy, x.detach(), res.detach() if with_res else None, coefs, relu,
        False, True)
    assert only_res[0] is None
    torch.testing.assert_close(only_res[1],
                               grads[1] if with_res else only_res[1])


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("needs", ["all", "affine_only", "input_only"])
def test_function_matches_autograd_on_cpu(relu, with_res, needs):
    """The autograd function itself (every needs_input_grad combination,
    what it saves) against autograd of the composed expression."""
    g = torch.Generator().manual_seed(6)
    shape = (3, 6, 4, 5)
    C = shape[1]
    x = torch.randn(shape, generator=g) * 2 + 0.5
    res = torch.randn(shape, generator=g) if with_res else None
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    w = torch.randn(C, generator=g).abs() + 0.1
    b = torch.randn(C, generator=g)
    dy = torch.randn(shape, generator=g)
    x_g = needs != "affine_only"
    p_g = needs != "input_only"

    def run(fn):
        xs = x.clone().requires_grad_(x_g)
        rs = res.clone().requires_grad_(x_g) if with_res else None
        ws, bs = w.clone().requires_grad_(p_g), b.clone().requires_grad_(p_g)
        y = fn(xs, rs, ws, bs)
        leaves = [t for t in (xs, rs, ws, bs)
                  if t is not None and t.requires_grad]
        return y.detach(), torch.autograd.grad(y, leaves, dy)

    def composed(xs, rs, ws, bs):
        scale = ws * torch.rsqrt(rv + 1e-5)
        return _composed(xs, rs, scale, bs - rm * scale, relu)

    saved = []
    with torch.autograd.graph.saved_tensors_hooks(
            lambda t: (saved.append(t), t)[1], lambda t: t):
        y, grads = run(lambda xs, rs, ws, bs: FrozenBatchNormActFunction.apply(
            xs, rs, ws, bs, rm, rv, 1e-5, relu))
    yref, gref = run(composed)
    torch.testing.assert_close(y, yref, atol=1e-5, rtol=1e-5)
    assert len(grads) == len(gref)
    for a, r in zip(grads, gref):
        torch.testing.assert_close(a, r, atol=1e-4, rtol=1e-4)
    n_full = sum(t.numel() == x.numel() for t in saved)
    # bn alone with a frozen affine keeps no activation alive
    want_full = (1 if (relu or p_g) else 0) + (1 if (relu and with_res) else 0)
    assert n_full == want_full
