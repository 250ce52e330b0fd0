"""GPU numerics for the fused BN(+add)+LeakyReLU kernels (the kActLeaky
instantiations) against the CPU reference ops, through every kernel family:
two-stage elemt / reduce / backward-elemt, the frozen backward kernel and the
small-plane single-launch pair, plus the running-statistics module routes
(eval with autograd, no_grad, FrozenBatchNorm2d) and one fused-discriminator
train step.

Inputs come from leaky_inputs.gated_inputs (min|z| >= 1e-5 in fp64), so no
gate can flip between the two arithmetics.  References are computed once per
key and never modified.  bf16 tolerances (2e-2) are the ones the existing
fused tests use for an 8-bit mantissa.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import msbn
from leaky_inputs import EPS, gated_inputs
from msbn import ops
from msbn.nn import fuse_bn_act
from msbn.nn.fused import SyncBatchNormActFunction
from msbn.ops import _reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

OP_SHAPES = [
    (4, 32, 9, 9),   # odd S: scalar NCHW (flat reduce); vectorised NHWC
    (2, 24, 8, 8),   # vectorised NCHW
    (3, 20, 7, 7),   # C not a multiple of the bf16 vector width
]
DTYPES = [torch.float32, torch.bfloat16]
SLOPES = [0.2, 0.01]


def _tol(dtype, fp32_tol):
    t = fp32_tol if dtype == torch.float32 else 2e-2
    return {"atol": t, "rtol": t}


SUMS = {"atol": 1e-3, "rtol": 1e-3}  # sums, grad_weight, grad_bias


def _dev(t, channels_last=False):
    if t is None:
        return None
    t = t.to(DEV)
    if channels_last and t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t


def _f(t):
    return None if t is None else t.float().cpu()


@functools.lru_cache(maxsize=None)
def _op_case(shape, dtype, slope, with_res):
    """Inputs + CPU reference of the three two-stage ops."""
    d = gated_inputs(shape, dtype, running=False)
    x, dy, w, b = d["x"], d["dy"], d["w"], d["b"]
    res = d["res"] if with_res else None
    C = shape[1]
    n = x.numel() // C
    mean, invstd = ref.batch_norm_stats(x, EPS)
    y = ref.batch_norm_elemt_act(x, res, w, b, mean, invstd, True, slope)
    gm = torch.empty_like(dy)
    sdy, sdyx, gw, gb = ref.batch_norm_backward_reduce_act(
        dy, x, res, mean, invstd, w, b, True, True, True, True, gm, slope
    )
    dx, dres = ref.batch_norm_backward_elemt_act(
        dy, x, res, mean, invstd, w, b, sdy, sdyx, torch.tensor([float(n)]),
        True, True, slope,
    )
    return dict(d=d, res=res, mean=mean, invstd=invstd, n=n, y=y, gm=gm,
                sdy=sdy, sdyx=sdyx, gw=gw, gb=gb, dx=dx, dres=dres)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_leaky_ops_vs_ref(shape, slope, dtype, channels_last, with_res):
    c = _op_case(shape, dtype, slope, with_res)
    d = c["d"]
    cl = channels_last
    x, dy, res = _dev(d["x"], cl), _dev(d["dy"], cl), _dev(c["res"], cl)
    w, b = d["w"].to(DEV), d["b"].to(DEV)
    mean, invstd = c["mean"].to(DEV), c["invstd"].to(DEV)

    y = ops.batch_norm_elemt_act(x, res, w, b, mean, invstd, True, None,
                                 slope)
    torch.testing.assert_close(_f(y), _f(c["y"]), **_tol(dtype, 1e-5))

    gm = torch.empty_like(dy)
    sdy, sdyx, gw, gb = ops.batch_norm_backward_reduce_act(
        dy, x, res, mean, invstd, w, b, True, True, True, True, None, gm,
        slope,
    )
    torch.testing.assert_close(sdy.cpu(), c["sdy"], **SUMS)
    torch.testing.assert_close(sdyx.cpu(), c["sdyx"], **SUMS)
    torch.testing.assert_close(gw.cpu(), c["gw"], **SUMS)
    torch.testing.assert_close(gb.cpu(), c["gb"], **SUMS)
    torch.testing.assert_close(_f(gm), _f(c["gm"]), **_tol(dtype, 1e-5))

    cnt = torch.tensor([float(c["n"])], device=DEV)
    dx, dres = ops.batch_norm_backward_elemt_act(
        dy, x, res, mean, invstd, w, b, sdy, sdyx, cnt, True, True, None,
        slope,
    )
    torch.testing.assert_close(_f(dx), _f(c["dx"]), **_tol(dtype, 1e-4))
    torch.testing.assert_close(_f(dres), _f(c["dres"]), **_tol(dtype, 1e-5))
    # the residual gradient IS the reduce pass's gm (same gate, same rounding)
    assert torch.equal(dres, gm)
    # ... and the gate-free elemt pass on gm gives the same dx (the gm
    # shortcut of the autograd function)
    dx_gm, _ = ops.batch_norm_backward_elemt_act(
        gm, x, None, mean, invstd, w, b, sdy, sdyx, cnt, False, False, None,
    )
    torch.testing.assert_close(_f(dx_gm), _f(c["dx"]), **_tol(dtype, 1e-4))


# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frozen_case(shape, dtype, slope, with_res):
    d = gated_inputs(shape, dtype, batch=False)
    res = d["res"] if with_res else None
    coefs = ref.bn_frozen_coefs(d["rm"], d["rv"], EPS, d["w"], d["b"])
    dx, dres = ref.batch_norm_frozen_backward_elemt(
        d["dy"], d["x"], res, coefs, True, True, True, slope
    )
    return dict(d=d, res=res, coefs=coefs, dx=dx, dres=dres)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("shape", [(2, 24, 8, 8), (4, 32, 9, 9)])
def test_leaky_frozen_backward_kernel(shape, slope, dtype, channels_last,
                                      with_res):
    c = _frozen_case(shape, dtype, slope, with_res)
    d = c["d"]
    cl = channels_last
    dx, dres = ops.batch_norm_frozen_backward_elemt(
        _dev(d["dy"], cl), _dev(d["x"], cl), _dev(c["res"], cl),
        c["coefs"].to(DEV), True, True, True, slope,
    )
    torch.testing.assert_close(_f(dx), _f(c["dx"]), **_tol(dtype, 1e-4))
    torch.testing.assert_close(_f(dres), _f(c["dres"]), **_tol(dtype, 1e-5))


# --------------------------------------------------------------------------
def _run_function(d, dev, with_res, slope_args, channels_last=False):
    C = d["x"].shape[1]

    def leaf(t):  # a copy: the cached inputs stay untouched
        return t.detach().clone().to(dev).requires_grad_(True)

    x = leaf(d["x"])
    r = leaf(d["res"]) if with_res else None
    xin, rin = x, r
    if channels_last:
        xin = x.contiguous(memory_format=torch.channels_last)
        rin = None if r is None else \
            r.contiguous(memory_format=torch.channels_last)
    w, b = leaf(d["w"]), leaf(d["b"])
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = SyncBatchNormActFunction.apply(
        xin, rin, w, b, rm, rv, EPS, 0.1, None, 1, True, *slope_args
    )
    y.backward(d["dy"].to(dev))
    out = dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)
    if with_res:
        out["dres"] = r.grad
    return out


@functools.lru_cache(maxsize=None)
def _function_case(shape, dtype, with_res):
    d = gated_inputs(shape, dtype, running=False)
    want = _run_function(d, "cpu", with_res, (0.2,))
    return d, {k: _f(v) for k, v in want.items()}


def _check_function(shape, dtype, with_res, channels_last, eligible):
    d, want = _function_case(shape, dtype, with_res)
    x = _dev(d["x"], channels_last)
    w, b = d["w"].to(DEV), d["b"].to(DEV)
    stat = torch.zeros(shape[1], device=DEV)
    assert ops.bn_fused_local_eligible(x, w, b, stat, stat) == eligible
    got = _run_function(d, DEV, with_res, (0.2,), channels_last)
    assert got.keys() == want.keys()
    for k in want:
        torch.testing.assert_close(_f(got[k]), want[k], **_tol(dtype, 1e-4),
                                   msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [
    (4, 64, 8, 8),     # vectorised packs
    (2, 64, 7, 7),     # scalar
    (128, 64, 4, 4),   # many rows per block
])
def test_leaky_small_plane_function_gpu_vs_cpu(shape, dtype, with_res):
    _check_function(shape, dtype, with_res, False, eligible=True)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_leaky_two_stage_function_gpu_vs_cpu(dtype, with_res):
    """channels_last is not eligible for the single-launch kernels: the
    two-stage local path (with the gm shortcut when the residual needs its
    gradient) at C >= 64."""
    _check_function((4, 64, 8, 8), dtype, with_res, True, eligible=False)


# --------------------------------------------------------------------------
@pytest.mark.parametrize("shape,channels_last", [((2, 64, 7, 7), False),
                                                 ((2, 24, 8, 8), False),
                                                 ((4, 64, 8, 8), True)])
def test_zero_slope_runs_the_relu_kernels(shape, channels_last):
    """negative_slope=0.0 dispatches to the unchanged relu instantiation:
    bit-identical to the call without the argument."""
    d = gated_inputs(shape, running=False)
    a = _run_function(d, DEV, True, (), channels_last)
    b = _run_function(d, DEV, True, (0.0,), channels_last)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    cl = channels_last
    x, res = _dev(d["x"], cl), _dev(d["res"], cl)
    mean, invstd = ops.batch_norm_stats(x, EPS)
    w, bb = d["w"].to(DEV), d["b"].to(DEV)
    assert torch.equal(
        ops.batch_norm_elemt_act(x, res, w, bb, mean, invstd, True),
        ops.batch_norm_elemt_act(x, res, w, bb, mean, invstd, True, None,
                                 0.0),
    )


# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _eval_case(shape, dtype):
    """Inputs + the composed CPU expression with running statistics."""
    d = gated_inputs(shape, dtype, batch=False)
    x = d["x"].detach().clone().requires_grad_(True)
    res = d["res"].detach().clone().requires_grad_(True)
    z = F.batch_norm(x.float(), d["rm"], d["rv"], d["w"], d["b"],
                     training=False, eps=EPS) + res.float()
    y = F.leaky_relu(z, 0.2).to(dtype)
    y.backward(d["dy"])
    return d, {"y": _f(y.detach()), "dx": _f(x.grad), "dres": _f(res.grad)}


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_leaky_eval_and_frozen_module_gpu(dtype, channels_last, frozen):
    """Running-statistics routes on the GPU: autograd on
    (FrozenBatchNormActFunction) and no_grad (one elemt launch), for the
    trainable module in eval mode and for FrozenBatchNorm2d."""
    shape = (2, 24, 8, 8)
    d, want = _eval_case(shape, dtype)
    cls = msbn.nn.FrozenBatchNorm2d if frozen else msbn.nn.SyncBatchNormAct2d
    m = cls(shape[1], eps=EPS, relu=True, negative_slope=0.2)
    with torch.no_grad():
        m.weight.copy_(d["w"])
        m.bias.copy_(d["b"])
        m.running_mean.copy_(d["rm"])
        m.running_var.copy_(d["rv"])
    m = m.to(DEV).eval().requires_grad_(False)
    cl = channels_last
    x = _dev(d["x"].clone(), cl).requires_grad_(True)
    res = _dev(d["res"].clone(), cl).requires_grad_(True)
    y = m(x, res)
    y.backward(_dev(d["dy"], cl))
    with torch.no_grad():
        y_ng = m(x, res)
    torch.testing.assert_close(_f(y), want["y"], **_tol(dtype, 1e-5))
    torch.testing.assert_close(_f(y_ng), want["y"], **_tol(dtype, 1e-5))
    torch.testing.assert_close(_f(x.grad), want["dx"], **_tol(dtype, 1e-4))
    torch.testing.assert_close(_f(res.grad), want["dres"],
                               **_tol(dtype, 1e-5))


# --------------------------------------------------------------------------
def test_fused_discriminator_step_gpu():
    """One train step of the fused DCGAN discriminator (three BN +
    LeakyReLU(0.2) pairs in one module each) against the unfused one."""
    torch.manual_seed(11)
    a = msbn.convert_sync_batchnorm(msbn.models.Discriminator(ndf=16))
    b = msbn.models.Discriminator(ndf=16)
    b.load_state_dict(a.state_dict())
    b = fuse_bn_act(msbn.convert_sync_batchnorm(b))
    assert sum(type(m).__name__ == "SyncBatchNormAct2d"
               for m in b.modules()) == 3
    a, b = a.to(DEV).train(), b.to(DEV).train()
    x = torch.randn(8, 3, 64, 64, device=DEV)
    t = torch.ones(8, 1, device=DEV)
    ya, yb = a(x), b(x)
    torch.testing.assert_close(ya, yb, atol=1e-3, rtol=1e-3)
    F.binary_cross_entropy_with_logits(ya, t).backward()
    F.binary_cross_entropy_with_logits(yb, t).backward()
    for (n1, p1), (n2, p2) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(p1.grad, p2.grad, atol=5e-3, rtol=5e-3,
                                   msg=lambda m, n=n1: f"{n}: {m}")
