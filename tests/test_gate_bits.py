"""Gate bits, CPU side.  The bits exist on the two-stage GPU path only
(msbn/nn/fused.py): on the CPU ``gate_bits=True`` must change nothing — the
op declines, the residual is saved, no gate tensor reaches any op — and the
switch has to thread through the module and the models.  The kernels are
covered in test_gpu_gate_bits.py."""

import pytest
import torch

import msbn.nn.fused as fused_mod
from msbn import ops
from msbn.models import resnet18, resnet50
from msbn.nn.fused import SyncBatchNormAct2d

SHAPE = (4, 8, 5, 7)
ACTS = [(True, 0.0), (True, 0.1), (False, 0.0)]


def _inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(SHAPE, generator=g) for _ in range(4))


def _module(gate_bits, relu=True, slope=0.0):
    g = torch.Generator().manual_seed(0)
    m = SyncBatchNormAct2d(SHAPE[1], relu=relu, negative_slope=slope,
                           gate_bits=gate_bits).train()
    with torch.no_grad():
        m.weight.copy_(torch.randn(SHAPE[1], generator=g).abs() + 0.1)
        m.bias.copy_(torch.randn(SHAPE[1], generator=g))
    return m


def test_op_declines_on_cpu():
    x, res, _, _ = _inputs()
    w, b = torch.ones(8), torch.zeros(8)
    mean, invstd = ops.batch_norm_stats(x, 1e-5)
    y = ops.batch_norm_elemt_act(x, res, w, b, mean, invstd, True)
    bits = ops.gate_bits_empty(x)
    assert bits.dtype == torch.uint8 and bits.numel() == (x.numel() + 7) // 8
    y2, gate = ops.batch_norm_elemt_act(x, res, w, b, mean, invstd, True,
                                        None, 0.0, bits)
    assert gate is None and torch.equal(y, y2)
    with pytest.raises(ValueError):
        ops.batch_norm_backward_reduce_act(
            x, x, None, mean, invstd, w, b, True, True, True, True, None,
            torch.empty_like(x), 0.0, None, gate=bits)


@pytest.mark.parametrize("fork", [False, True], ids=["plain", "fork"])
@pytest.mark.parametrize("relu,slope", ACTS, ids=["relu", "leaky", "none"])
def test_cpu_module_gate_bits_on_equals_off(relu, slope, fork, monkeypatch):
    seen = []
    real = ops.batch_norm_backward_reduce_act

    def spy(*a, **kw):
        seen.append(kw.get("gate"))
        return real(*a, **kw)

    monkeypatch.setattr(fused_mod.ops, "batch_norm_backward_reduce_act", spy)
    x, res, g1, g2 = _inputs()
    outs = []
    for gate_bits in (True, False):
        m = _module(gate_bits, relu, slope)
        assert m.gate_bits is gate_bits
        xl = x.clone().requires_grad_(True)
        rl = res.clone().requires_grad_(True)
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda s: saved.append(s) or s, lambda s: s):
            out = m(xl, rl, fork=fork)
        # the residual is saved, and nothing byte-typed
        assert any(s.data_ptr() == rl.data_ptr() for s in saved)
        assert not any(s.dtype == torch.uint8 for s in saved)
        if fork:
            (out[0] * g1).sum().backward(retain_graph=True)
            (out[1] * g2).sum().backward()
            out = out[0]
        else:
            out.backward(g1)
        outs.append((out.detach(), xl.grad, rl.grad, m.weight.grad,
                     m.bias.grad, m.running_mean, m.running_var))
    assert seen and all(s is None for s in seen)
    for a, e in zip(*outs):
        assert torch.equal(a, e)


@pytest.mark.parametrize("factory", [resnet18, resnet50])
def test_model_switch_reaches_the_closing_bns(factory):
    on = factory(num_classes=4, fused=True)
    off = factory(num_classes=4, fused=True, gate_bits=False)
    plain = factory(num_classes=4)  # honoured only where fused is set
    assert on.gate_bits and not off.gate_bits and not plain.gate_bits
    last = "bn2" if factory is resnet18 else "bn3"
    for model, want in ((on, True), (off, False)):
        closing = [getattr(blk, last) for layer in
                   (model.layer1, model.layer2, model.layer3, model.layer4)
                   for blk in layer]
        assert len(closing) == (8 if factory is resnet18 else 16)
        assert all(bn.gate_bits is want for bn in closing)
    assert on.state_dict().keys() == off.state_dict().keys()


def test_cpu_model_gate_bits_on_equals_off():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 32, 32, generator=g)
    y = torch.randint(0, 4, (2,), generator=g)
    outs = []
    for gate_bits in (True, False):
        torch.manual_seed(0)
        m = resnet18(num_classes=4, fused=True, gate_bits=gate_bits).train()
        xg = x.clone().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(m(xg), y)
        loss.backward()
        outs.append([loss.detach(), xg.grad]
                    + [p.grad for p in m.parameters()])
    for a, e in zip(*outs):
        assert torch.equal(a, e)


def test_module_without_the_attribute_keeps_the_residual_route():
    """A module pickled before gate_bits existed has no such attribute."""
    m = _module(True)
    del m.gate_bits
    x, res, g1, _ = _inputs()
    m(x.requires_grad_(True), res.requires_grad_(True)).backward(g1)
    assert x.grad is not None and res.grad is not None
