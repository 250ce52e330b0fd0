"""Dual BN, CPU side: ``relu(bn(x) + bn_skip(x_skip))`` as one autograd
function (msbn/nn/fused.py, docs/KERNEL_DESIGN.md "Dual BN").  The dual
kernels exist on the GPU only (test_gpu_dual_bn.py); here

* ``bn_add_bn_act`` on CPU tensors must take the composition,
* ``SyncBatchNormDualActFunction`` applied directly runs its internal
  fallback, the single-BN ops, and equals the composition bytewise in fp32,
* the function's fixed collective schedule is run on two gloo ranks, one of
  them with an empty batch, and
* the model switch only takes the route for modules it is defined for.

The oracle throughout is the composition on the same inputs."""

import os
import sys

import pytest
import torch
import torch.distributed as dist

import msbn.models.resnet as resnet_mod
import msbn.nn.fused as fused_mod
from msbn.models import resnet18
from msbn.nn import SyncBatchNorm
from msbn.nn.batchnorm import _momentum_factor
from msbn.nn.fused import (SyncBatchNormAct2d, SyncBatchNormDualActFunction,
                           bn_add_bn_act)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPE = (4, 8, 5, 7)


def _same(a, b):
    """torch.equal that also holds for NaNs in the same places."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(
        a.contiguous().reshape(-1).view(torch.uint8),
        b.contiguous().reshape(-1).view(torch.uint8))


def _pair(seed=0, group=None):
    """A closing BN and a skip BN with different, off-centre parameters."""
    g = torch.Generator().manual_seed(seed)
    C = SHAPE[1]
    bn = SyncBatchNormAct2d(C, relu=True, process_group=group).train()
    bn_skip = SyncBatchNorm(C, process_group=group).train()
    with torch.no_grad():
        for m in (bn, bn_skip):
            m.weight.copy_(torch.randn(C, generator=g).abs() + 0.1)
            m.bias.copy_(torch.randn(C, generator=g))
            m.running_mean.copy_(torch.randn(C, generator=g))
            m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn, bn_skip


def _inputs(seed=1, n=SHAPE[0]):
    g = torch.Generator().manual_seed(seed)
    shape = (n,) + SHAPE[1:]
    x = torch.randn(shape, generator=g) + 1.0
    x_d = torch.randn(shape, generator=g) * 2.0 - 1.5
    g1, g2 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    return x, x_d, g1, g2


def _force_function(bn, bn_skip, x, x_d, fork, group=None, world=1):
    """What bn_add_bn_act does once it has chosen the dual route."""
    for m in (bn_skip, bn):
        m.num_batches_tracked.add_(1)
    return SyncBatchNormDualActFunction.apply(
        x, x_d, bn.weight, bn.bias, bn_skip.weight, bn_skip.bias,
        bn.running_mean, bn.running_var, bn_skip.running_mean,
        bn_skip.running_var, bn.eps, bn_skip.eps, _momentum_factor(bn),
        _momentum_factor(bn_skip), group, world, fork)


def _run(route, fork, used, x_d_grad=True, group=None, world=1, n=SHAPE[0]):
    bn, bn_skip = _pair(group=group)
    x, x_d, g1, g2 = _inputs(n=n)
    x.requires_grad_(True)
    x_d.requires_grad_(x_d_grad)
    if route == "function":
        out = _force_function(bn, bn_skip, x, x_d, fork, group, world)
    elif route == "entry":
        out = bn_add_bn_act(bn, bn_skip, x, x_d, fork)
    else:
        out = bn(x, residual=bn_skip(x_d), fork=True) if fork else \
            bn(x, residual=bn_skip(x_d))
    main, skip = out if fork else (out, None)
    loss = 0
    if used in ("main", "both"):
        loss = loss + (main * g1).sum()
    if used in ("skip", "both"):
        loss = loss + (skip * g2).sum()
    loss.backward()
    res = [main.detach(), x.grad, x_d.grad]
    for m in (bn, bn_skip):
        res += [m.weight.grad, m.bias.grad, m.running_mean, m.running_var,
                m.num_batches_tracked]
    return res


CASES = [(False, "main"), (True, "main"), (True, "skip"), (True, "both")]


@pytest.mark.parametrize("fork,used", CASES,
                         ids=[f"fork{int(f)}-{u}" for f, u in CASES])
@pytest.mark.parametrize("x_d_grad", [True, False], ids=["xd_grad", "xd_nograd"])
def test_cpu_function_fallback_equals_composition(fork, used, x_d_grad):
    want = _run("composition", fork, used, x_d_grad)
    got = _run("function", fork, used, x_d_grad)
    assert len(got) == len(want) == 13
    for i, (a, e) in enumerate(zip(got, want)):
        assert _same(a, e), i


def test_cpu_entry_takes_the_composition(monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the dual function ran on CPU tensors")

    monkeypatch.setattr(fused_mod.SyncBatchNormDualActFunction, "apply",
                        never)
    for fork, used in CASES:
        want = _run("composition", fork, used)
        got = _run("entry", fork, used)
        for a, e in zip(got, want):
            assert _same(a, e)


# ------------------------------------------------- two ranks, one empty batch
def schedule_case(rank, world, device, case):
    """Both ranks force the function; rank 1 has an empty batch.  Then both
    run the composition the same way.  The function issues skip stats, main
    stats, ONE [4C] all_reduce; a rank on the single-BN ops (rank 1: empty)
    must still meet that schedule or the group hangs."""
    fork, used = case
    n = SHAPE[0] if rank == 0 else 0
    group = dist.group.WORLD
    got = _run("function", fork, used, group=group, world=world, n=n)
    want = _run("composition", fork, used, group=group, world=world, n=n)
    fails = []
    if rank == 0:
        for i, (a, e) in enumerate(zip(got, want)):
            if not _same(a, e):
                fails.append(f"result {i} differs from the composition")
    return fails


def test_two_ranks_one_empty_batch_follow_the_schedule(tmp_path):
    import multirank_harness

    multirank_harness.run_cases(
        tmp_path, 2, "cpu", "test_dual_bn:schedule_case",
        [(False, "main"), (True, "both")])


# ------------------------------------------------------------------- models
def _spied_model_step(monkeypatch, prepare, **kw):
    calls = []
    real = fused_mod.SyncBatchNormDualActFunction.apply

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(fused_mod.SyncBatchNormDualActFunction, "apply", spy)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 32, 32, generator=g)
    outs = []
    for dual_bn in (True, False):
        torch.manual_seed(0)
        m = resnet18(num_classes=4, fused=True, dual_bn=dual_bn, **kw).train()
        m = prepare(m)
        xg = x.clone().requires_grad_(True)
        m(xg).sum().backward()
        outs.append([xg.grad] + [p.grad for p in m.parameters()])
    assert not calls
    for a, e in zip(*outs):
        assert _same(a, e)


def test_hooked_skip_bn_keeps_the_composition(monkeypatch):
    seen = []

    def prepare(m):
        m.layer2[0].downsample[1].register_forward_hook(
            lambda mod, i, o: seen.append(1))
        return m

    _spied_model_step(monkeypatch, prepare)
    assert len(seen) == 2  # the hook still fires, on both models


def test_frozen_model_keeps_the_composition(monkeypatch):
    from msbn.nn import freeze_batchnorm

    _spied_model_step(monkeypatch, lambda m: freeze_batchnorm(m) or m)


def test_eval_model_keeps_the_composition(monkeypatch):
    _spied_model_step(monkeypatch, lambda m: m.eval())


def test_model_without_gate_bits_keeps_the_composition(monkeypatch):
    _spied_model_step(monkeypatch, lambda m: m, gate_bits=False)


def test_switch_threads_through_and_state_dict_is_unchanged():
    on = resnet18(num_classes=4, fused=True)
    off = resnet18(num_classes=4, fused=True, dual_bn=False)
    nogate = resnet18(num_classes=4, fused=True, gate_bits=False)
    plain = resnet18(num_classes=4)
    assert on.dual_bn and not off.dual_bn
    assert not nogate.dual_bn and not plain.dual_bn
    first = [layer[0] for layer in (on.layer2, on.layer3, on.layer4)]
    assert all(resnet_mod._dual_downsample(b) for b in first)
    assert not resnet_mod._dual_downsample(on.layer1[0])  # no downsample
    assert not any(resnet_mod._dual_downsample(layer[0])
                   for layer in (off.layer2, nogate.layer2, plain.layer2))
    assert on.state_dict().keys() == off.state_dict().keys()
    assert list(on.state_dict()) == list(nogate.state_dict())
    # a block pickled before dual_bn existed has no such attribute
    blk = on.layer2[0]
    del blk.dual_bn
    assert not resnet_mod._dual_downsample(blk)
