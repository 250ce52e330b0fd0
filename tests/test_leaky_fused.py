"""Fused BN(+add)+LeakyReLU epilogue (negative_slope): CPU numerics against
the composed expression, the fusion pass on the DCGAN discriminator, module
validation / compatibility and a world-2 gloo run.  The GPU kernels are
covered in test_gpu_leaky_fused.
"""

import copy
import io
import pickle

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

import msbn
from leaky_inputs import EPS, gated_inputs
from msbn.nn import fuse_bn_act
from msbn.nn.frozen import (FrozenBatchNorm2d, FrozenBatchNormActFunction,
                            freeze_batchnorm)
from msbn.nn.fused import SyncBatchNormAct2d, SyncBatchNormActFunction

SHAPE = (6, 12, 7, 5)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


# --------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.2, 0.01, -0.5])
@pytest.mark.parametrize("with_res", [True, False])
def test_leaky_function_matches_composed(slope, with_res):
    d = gated_inputs(SHAPE)
    C = SHAPE[1]
    x, w, b = _leaf(d["x"]), _leaf(d["w"]), _leaf(d["b"])
    res = _leaf(d["res"]) if with_res else None
    rm, rv = torch.zeros(C), torch.ones(C)
    y = SyncBatchNormActFunction.apply(
        x, res, w, b, rm, rv, EPS, 0.1, None, 1, True, slope
    )

    x2, w2, b2 = _leaf(d["x"]), _leaf(d["w"]), _leaf(d["b"])
    res2 = _leaf(d["res"]) if with_res else None
    rm2, rv2 = torch.zeros(C), torch.ones(C)
    z = F.batch_norm(x2, rm2, rv2, w2, b2, training=True, momentum=0.1,
                     eps=EPS)
    if with_res:
        z = z + res2
    z = F.leaky_relu(z, slope)

    assert torch.allclose(y, z, atol=1e-5)
    assert torch.allclose(rm, rm2, atol=1e-6)
    assert torch.allclose(rv, rv2, atol=1e-5)
    y.backward(d["dy"])
    z.backward(d["dy"])
    assert torch.allclose(x.grad, x2.grad, atol=1e-4)
    assert torch.allclose(w.grad, w2.grad, atol=1e-4)
    assert torch.allclose(b.grad, b2.grad, atol=1e-4)
    if with_res:
        assert torch.allclose(res.grad, res2.grad, atol=1e-5)


def _composed_running(d, x, res, w, b, slope):
    z = F.batch_norm(x, d["rm"], d["rv"], w, b, training=False, eps=EPS)
    if res is not None:
        z = z + res
    return F.leaky_relu(z, slope)


def _load(m, d):
    with torch.no_grad():
        m.weight.copy_(d["w"])
        m.bias.copy_(d["b"])
        m.running_mean.copy_(d["rm"])
        m.running_var.copy_(d["rv"])
    return m


@pytest.mark.parametrize("grad", [True, False])
def test_leaky_module_eval_matches_composed(grad):
    d = gated_inputs(SHAPE)
    m = _load(SyncBatchNormAct2d(SHAPE[1], eps=EPS, relu=True,
                                 negative_slope=0.2), d).eval()
    want = _composed_running(d, d["x"], d["res"], d["w"], d["b"], 0.2)
    if not grad:
        with torch.no_grad():
            got = m(d["x"], d["res"])
        assert not got.requires_grad
        assert torch.allclose(got, want, atol=1e-5)
        return
    x, res = _leaf(d["x"]), _leaf(d["res"])
    got = m(x, res)
    assert torch.allclose(got, want, atol=1e-5)
    x2, res2 = _leaf(d["x"]), _leaf(d["res"])
    w2, b2 = _leaf(d["w"]), _leaf(d["b"])
    _composed_running(d, x2, res2, w2, b2, 0.2).backward(d["dy"])
    got.backward(d["dy"])
    assert torch.allclose(x.grad, x2.grad, atol=1e-4)
    assert torch.allclose(res.grad, res2.grad, atol=1e-5)
    assert torch.allclose(m.weight.grad, w2.grad, atol=1e-4)
    assert torch.allclose(m.bias.grad, b2.grad, atol=1e-4)


@pytest.mark.parametrize("via_freeze", [False, True])
def test_leaky_frozen_module_matches_composed(via_freeze):
    d = gated_inputs(SHAPE)
    C = SHAPE[1]
    if via_freeze:
        src = _load(SyncBatchNormAct2d(C, eps=EPS, relu=True,
                                       negative_slope=0.2), d)
        m = freeze_batchnorm(nn.Sequential(src))[0]
        assert isinstance(m, FrozenBatchNorm2d)
        assert m.relu and m.negative_slope == 0.2
    else:
        m = _load(FrozenBatchNorm2d(C, eps=EPS, relu=True,
                                    negative_slope=0.2), d)
    assert "negative_slope=0.2" in repr(m)
    m.train()  # frozen whatever .training says
    x, res = _leaf(d["x"]), _leaf(d["res"])
    got = m(x, res)
    x2, res2 = _leaf(d["x"]), _leaf(d["res"])
    want = _composed_running(d, x2, res2, d["w"], d["b"], 0.2)
    assert torch.allclose(got, want, atol=1e-5)
    got.backward(d["dy"])
    want.backward(d["dy"])
    assert torch.allclose(x.grad, x2.grad, atol=1e-4)
    assert torch.allclose(res.grad, res2.grad, atol=1e-5)
    assert torch.equal(m.running_mean, d["rm"])


def test_leaky_frozen_function_reference_path():
    """FrozenBatchNormActFunction (the GPU autograd path, here on the CPU
    reference ops) with a slope, trainable affine included."""
    d = gated_inputs(SHAPE)
    x, res = _leaf(d["x"]), _leaf(d["res"])
    w, b = _leaf(d["w"]), _leaf(d["b"])
    got = FrozenBatchNormActFunction.apply(
        x, res, w, b, d["rm"], d["rv"], EPS, True, 0.2
    )
    x2, res2 = _leaf(d["x"]), _leaf(d["res"])
    w2, b2 = _leaf(d["w"]), _leaf(d["b"])
    want = _composed_running(d, x2, res2, w2, b2, 0.2)
    assert torch.allclose(got, want, atol=1e-5)
    got.backward(d["dy"])
    want.backward(d["dy"])
    assert torch.allclose(x.grad, x2.grad, atol=1e-4)
    assert torch.allclose(res.grad, res2.grad, atol=1e-5)
    assert torch.allclose(w.grad, w2.grad, atol=1e-4)
    assert torch.allclose(b.grad, b2.grad, atol=1e-4)


# --------------------------------------------------------------------------
def _is_bn(m):
    return isinstance(m, (nn.modules.batchnorm._BatchNorm,
                          msbn.nn.batchnorm._NormBase))


def test_fuse_bn_act_pass_discriminator():
    """fuse_bn_act on the DCGAN discriminator: the three BN + LeakyReLU(0.2)
    pairs become SyncBatchNormAct2d(negative_slope=0.2), same function."""
    torch.manual_seed(3)
    d1 = msbn.convert_sync_batchnorm(msbn.models.Discriminator(ndf=16))
    d2 = msbn.models.Discriminator(ndf=16)
    d2.load_state_dict(d1.state_dict())
    d2 = fuse_bn_act(msbn.convert_sync_batchnorm(d2))

    acts = [m for m in d2.modules() if isinstance(m, SyncBatchNormAct2d)]
    assert len(acts) == 3
    assert all(m.relu and m.negative_slope == 0.2 for m in acts)
    seq = list(d2.main)
    assert not any(_is_bn(a) and isinstance(b, nn.LeakyReLU)
                   for a, b in zip(seq, seq[1:]))
    # the first LeakyReLU has no BN in front of it and stays
    assert sum(isinstance(m, nn.LeakyReLU) for m in seq) == 1

    # hyper-parameter, not state: identical keys, loads in both directions
    assert list(d1.state_dict()) == list(d2.state_dict())
    d2.load_state_dict(d1.state_dict())
    d1.load_state_dict(d2.state_dict())

    x = torch.randn(4, 3, 64, 64)
    t = torch.ones(4, 1)
    d1.train(), d2.train()
    y1, y2 = d1(x), d2(x)
    torch.testing.assert_close(y1, y2, atol=1e-4, rtol=1e-4)
    F.binary_cross_entropy_with_logits(y1, t).backward()
    F.binary_cross_entropy_with_logits(y2, t).backward()
    for (n1, p1), (n2, p2) in zip(d1.named_parameters(),
                                  d2.named_parameters()):
        assert n1 == n2
        torch.testing.assert_close(p1.grad, p2.grad, atol=1e-3, rtol=1e-3)
    for (n1, b1), (n2, b2) in zip(d1.named_buffers(), d2.named_buffers()):
        torch.testing.assert_close(b1, b2, atol=1e-5, rtol=1e-5)
    d1.eval(), d2.eval()
    with torch.no_grad():
        torch.testing.assert_close(d1(x), d2(x), atol=1e-4, rtol=1e-4)


def test_fuse_bn_act_pass_generator_unchanged():
    g = fuse_bn_act(msbn.convert_sync_batchnorm(msbn.models.Generator(ngf=16)))
    acts = [m for m in g.modules() if isinstance(m, SyncBatchNormAct2d)]
    assert len(acts) == 4
    assert all(m.relu and m.negative_slope == 0.0 for m in acts)
    assert all("negative_slope" not in repr(m) for m in acts)


def test_fuse_bn_act_frozen_and_torch_bn_leaky():
    seq = nn.Sequential(
        nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.LeakyReLU(0.1, inplace=True),
        nn.Conv2d(8, 8, 3), FrozenBatchNorm2d(8), nn.LeakyReLU(0.3),
    )
    out = fuse_bn_act(nn.Sequential(seq))[0]
    assert isinstance(out[1], SyncBatchNormAct2d)
    assert out[1].negative_slope == pytest.approx(0.1)
    assert isinstance(out[-1], FrozenBatchNorm2d) and out[-1].relu
    assert out[-1].negative_slope == pytest.approx(0.3)
    assert not any(isinstance(m, nn.LeakyReLU) for m in out)


# --------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [SyncBatchNormAct2d, FrozenBatchNorm2d])
def test_negative_slope_validation(cls):
    with pytest.raises(ValueError):
        cls(4, relu=False, negative_slope=0.2)
    with pytest.raises(ValueError):
        cls(4, relu=True, negative_slope=float("nan"))
    with pytest.raises(ValueError):
        cls(4, relu=True, negative_slope=float("inf"))
    cls(4, relu=False, negative_slope=0.0)
    assert cls(4, relu=True, negative_slope=-0.5).negative_slope == -0.5


@pytest.mark.parametrize("with_res", [True, False])
def test_zero_slope_is_todays_relu(with_res):
    d = gated_inputs(SHAPE)
    C = SHAPE[1]

    def run(*extra):
        x, w, b = _leaf(d["x"]), _leaf(d["w"]), _leaf(d["b"])
        res = _leaf(d["res"]) if with_res else None
        rm, rv = torch.zeros(C), torch.ones(C)
        y = SyncBatchNormActFunction.apply(
            x, res, w, b, rm, rv, EPS, 0.1, None, 1, True, *extra
        )
        y.backward(d["dy"])
        out = [y.detach(), x.grad, w.grad, b.grad, rm, rv]
        return out + ([res.grad] if with_res else [])

    for a, b in zip(run(), run(0.0)):
        assert torch.equal(a, b)


def test_leaky_module_copy_and_pickle_roundtrip():
    d = gated_inputs(SHAPE)
    m = _load(SyncBatchNormAct2d(SHAPE[1], eps=EPS, relu=True,
                                 negative_slope=0.2), d)
    f = _load(FrozenBatchNorm2d(SHAPE[1], eps=EPS, relu=True,
                                negative_slope=0.2), d)
    for mod in (m, f):
        mod.eval()
        want = mod(d["x"], d["res"])
        buf = io.BytesIO()
        torch.save(mod, buf)
        buf.seek(0)
        for clone in (copy.deepcopy(mod), pickle.loads(pickle.dumps(mod)),
                      torch.load(buf, weights_only=False)):
            assert clone.negative_slope == 0.2
            assert torch.equal(clone(d["x"], d["res"]), want)
        assert "negative_slope" not in mod.state_dict()


def test_module_pickled_before_negative_slope_still_runs():
    d = gated_inputs(SHAPE)
    m = _load(SyncBatchNormAct2d(SHAPE[1], eps=EPS, relu=True), d).eval()
    f = _load(FrozenBatchNorm2d(SHAPE[1], eps=EPS, relu=True), d)
    for mod in (m, f):
        want = mod(d["x"])
        del mod.__dict__["negative_slope"]  # as an old pickle restores it
        assert torch.equal(mod(d["x"]), want)
        assert "negative_slope" not in repr(mod)
    m.train()
    m(d["x"])
    assert freeze_batchnorm(nn.Sequential(m))[0].negative_slope == 0.0


# --------------------------------------------------------------------------
WORLD = 2


def _worker(rank, tmpdir, q):
    try:
        dist.init_process_group("gloo", init_method=f"file://{tmpdir}/pg",
                                rank=rank, world_size=WORLD)
        _gloo_body(rank)
        q.put((rank, None))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _gloo_body(rank):
    d = gated_inputs(SHAPE)
    C, half = SHAPE[1], SHAPE[0] // WORLD
    sl = slice(rank * half, (rank + 1) * half)

    m = SyncBatchNormAct2d(C, eps=EPS, relu=True, negative_slope=0.2)
    with torch.no_grad():
        m.weight.copy_(d["w"])
        m.bias.copy_(d["b"])
    m.train()
    x = _leaf(d["x"][sl])
    y = m(x)
    y.backward(d["dy"][sl])
    # the module's parameter grads are per-rank partial sums
    gw, gb = m.weight.grad.clone(), m.bias.grad.clone()
    dist.all_reduce(gw)
    dist.all_reduce(gb)

    # single-process full-batch composed oracle
    x2, w2, b2 = _leaf(d["x"]), _leaf(d["w"]), _leaf(d["b"])
    rm2, rv2 = torch.zeros(C), torch.ones(C)
    z = F.leaky_relu(
        F.batch_norm(x2, rm2, rv2, w2, b2, training=True, momentum=0.1,
                     eps=EPS), 0.2)
    z.backward(d["dy"])
    assert torch.allclose(y, z[sl], atol=1e-5)
    assert torch.allclose(x.grad, x2.grad[sl], atol=1e-4)
    assert torch.allclose(gw, w2.grad, atol=1e-4)
    assert torch.allclose(gb, b2.grad, atol=1e-4)
    assert torch.allclose(m.running_mean, rm2, atol=1e-6)
    assert torch.allclose(m.running_var, rv2, atol=1e-5)


def test_leaky_sync_world2_gloo(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    ps = [ctx.Process(target=_worker, args=(r, str(tmp_path), q))
          for r in range(WORLD)]
    for p in ps:
        p.start()
    errs = []
    for _ in range(WORLD):
        rank, err = q.get()
        if err:
            errs.append((rank, err))
    for p in ps:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
            errs.append((p.pid, "timeout"))
    assert not errs, "\n".join(f"rank {r}:\n{e}" for r, e in errs)
