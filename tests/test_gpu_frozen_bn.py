"""GPU numerics for the frozen-BN path: bn_frozen_coefs, the frozen backward
elementwise kernels, FrozenBatchNormActFunction / FrozenBatchNorm2d and the
eval-mode routing of the trainable BN modules.

Reference: autograd of the composed expression in fp64 on CPU, from the same
dtype-rounded inputs.  Inputs are nudged on CPU until no reference
pre-activation lies within |z| < 1e-3, so the ReLU gate is unambiguous and
every element is compared.
"""

import functools

import pytest
import torch

import msbn
from msbn import ops
from msbn.nn import FrozenBatchNorm2d

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
BAND = 1e-3

OP_SHAPES = [
    (4, 32, 9, 9),      # S=81 -> V=1 in NCHW; full-width packs in NHWC
    (2, 24, 4, 6),      # full-width NCHW packs
    (3, 20, 2, 2),      # S=4 and C=20 -> half-width packs
    (2, 100, 5, 5),     # C not a multiple of 8
    (8, 16),            # 2-D input
    (2, 24, 4, 6, 5),   # 5-D / channels_last_3d
    (2, 64, 56, 56),    # many blocks (1568 at V=1), still under the 4096-block
                        # cap: ONE trip each.  The grid-stride loop's second
                        # trip is covered in test_gpu_reduction_edges.py
]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (relu, with_res, want_res_grad)
COMBOS = [(False, False, False), (True, False, False), (True, True, False),
          (True, True, True), (False, True, True)]
LAYOUT_CASES = [(s, cl) for s in OP_SHAPES for cl in (False, True)
                if not (cl and len(s) < 4)]


def _tol(dtype):
    return {"atol": 1e-5, "rtol": 1e-5} if dtype == torch.float32 else \
        {"atol": 2e-2, "rtol": 2e-2}


PTOL = {"atol": 1e-3, "rtol": 1e-3}  # grad_weight / grad_bias


def _chan(t, ndim):
    return t.reshape([1, -1] + [1] * (ndim - 2))


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, relu, with_res):
    """Inputs (CPU, dtype-rounded) + fp64 reference of forward and every
    gradient.  Computed once per key and never modified."""
    seed = (sum((i + 1) * 7919 * s for i, s in enumerate(shape))
            + 31 * DTYPES.index(dtype) + 2 * int(relu) + int(with_res))
    g = torch.Generator().manual_seed(seed % (2 ** 31))
    C = shape[1]
    x = (torch.randn(shape, generator=g) * 2 + 0.5).to(dtype)
    res = torch.randn(shape, generator=g).to(dtype) if with_res else None
    dy = torch.randn(shape, generator=g).to(dtype)
    w = torch.randn(C, generator=g).abs() + 0.1
    b = torch.randn(C, generator=g)
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5

    def pre(xv, w64, b64):
        scale = w64 * torch.rsqrt(rv.double() + EPS)
        z = xv * _chan(scale, len(shape)) + _chan(b64 - rm.double() * scale,
                                                  len(shape))
        return z + res.double() if with_res else z

    # nudge: move x by 1 (>= 0.08 in z) wherever |z| < BAND, re-round, repeat
    for _ in range(64):
        near = pre(x.double(), w.double(), b.double()).abs() < BAND
        if not near.any():
            break
        x = torch.where(near, x.float() + 1.0, x.float()).to(dtype)
    assert not (pre(x.double(), w.double(), b.double()).abs() < BAND).any()

    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if with_res else None
    if with_res:
        scale = w64 * torch.rsqrt(rv.double() + EPS)
        z = x64 * _chan(scale, len(shape)) + _chan(
            b64 - rm.double() * scale, len(shape)) + r64
    else:
        z = pre(x64, w64, b64)
    y = torch.relu(z) if relu else z
    leaves = [x64, w64, b64] + ([r64] if with_res else [])
    grads = torch.autograd.grad(y, leaves, dy.double())
    scale = (w.double() * torch.rsqrt(rv.double() + EPS))
    return {
        "x": x, "res": res, "dy": dy, "w": w, "b": b, "rm": rm, "rv": rv,
        "coefs": torch.cat([scale, b.double() - rm.double() * scale]),
        "y": y.detach(), "dx": grads[0], "gw": grads[1], "gb": grads[2],
        "dres": grads[3] if with_res else None,
    }


def _dev(t, channels_last=False):
    if t is None:
        return None
    t = t.to(DEV)
    if channels_last and t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    elif channels_last and t.dim() == 5:
        t = t.contiguous(memory_format=torch.channels_last_3d)
    return t


def _close(got, want, **tol):
    torch.testing.assert_close(got.double().cpu(), want, **tol)


# --------------------------------------------------------------- op level
@pytest.mark.parametrize("wdtype", DTYPES)
@pytest.mark.parametrize("sdtype", DTYPES)
@pytest.mark.parametrize("C", [20, 100, 2048])
def test_frozen_coefs_op(C, sdtype, wdtype):
    g = torch.Generator().manual_seed(C)
    rm = torch.randn(C, generator=g).to(sdtype)
    rv = (torch.rand(C, generator=g) + 0.5).to(sdtype)
    w = (torch.randn(C, generator=g).abs() + 0.1).to(wdtype)
    b = torch.randn(C, generator=g).to(wdtype)
    scale = w.double() * torch.rsqrt(rv.double() + EPS)
    for ww, bb in [(w, b), (None, None), (w, None)]:
        coefs = ops.bn_frozen_coefs(rm.to(DEV), rv.to(DEV), EPS, _dev(ww),
                                    _dev(bb))
        assert coefs.dtype == torch.float32 and coefs.shape == (2 * C,)
        sc = scale if ww is not None else torch.rsqrt(rv.double() + EPS)
        sh = -rm.double() * sc + (bb.double() if bb is not None else 0.0)
        _close(coefs, torch.cat([sc, sh]), atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("relu,with_res,want_res", COMBOS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,channels_last", LAYOUT_CASES)
def test_frozen_backward_elemt_op(shape, channels_last, dtype, relu, with_res,
                                  want_res):
    c = _case(shape, dtype, relu, with_res)
    C = shape[1]
    coefs = ops.bn_frozen_coefs(c["rm"].to(DEV), c["rv"].to(DEV), EPS,
                                c["w"].to(DEV), c["b"].to(DEV))
    _close(coefs, c["coefs"], atol=1e-5, rtol=1e-5)
    dy = _dev(c["dy"], channels_last)
    x = _dev(c["x"], channels_last) if relu else None
    res = _dev(c["res"], channels_last) if relu else None
    dx, dres = ops.batch_norm_frozen_backward_elemt(
        dy, x, res, coefs, relu, True, want_res)
    assert dx.dtype == dtype and dx.shape == dy.shape
    assert dx.stride() == dy.stride()
    _close(dx, c["dx"], **_tol(dtype))
    if not want_res:
        assert dres is None
    else:
        _close(dres, c["dres"], **_tol(dtype))
        if not relu:  # no gate: the residual gradient IS grad_out
            assert dres.data_ptr() == dy.data_ptr()
        # residual branch alone
        dx2, dres2 = ops.batch_norm_frozen_backward_elemt(
            dy, x, res, coefs, relu, False, True)
        assert dx2 is None
        assert torch.equal(dres2, dres)
    # forward through the same coefs (the frozen forward launch)
    y = ops.batch_norm_elemt_act(
        _dev(c["x"], channels_last), _dev(c["res"], channels_last), None,
        None, coefs[:C], coefs[:C], relu, coefs)
    _close(y, c["y"], **_tol(dtype))


# ----------------------------------------------------------- module level
def _frozen_module(c, relu):
    C = c["w"].numel()
    m = FrozenBatchNorm2d(C, EPS, relu=relu)
    m.load_state_dict({"weight": c["w"], "bias": c["b"],
                       "running_mean": c["rm"], "running_var": c["rv"]})
    return m.to(DEV).train()  # frozen whatever the mode


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("shape", [(4, 32, 9, 9), (2, 24, 4, 6)])
def test_frozen_module(shape, channels_last, dtype, with_res, relu):
    c = _case(shape, dtype, relu, with_res)
    m = _frozen_module(c, relu)
    x = _dev(c["x"], channels_last).requires_grad_(True)
    res = _dev(c["res"], channels_last)
    if with_res:
        res.requires_grad_(True)
    y = m(x, res)
    assert y.dtype == dtype
    _close(y, c["y"], **_tol(dtype))
    # grad_output arrives in the OTHER layout
    dy = _dev(c["dy"], not channels_last)
    grads = torch.autograd.grad(y, [x] + ([res] if with_res else []), dy)
    _close(grads[0], c["dx"], **_tol(dtype))
    if with_res:
        _close(grads[1], c["dres"], **_tol(dtype))
    assert torch.equal(m.running_mean.cpu(), c["rm"])
    assert int(m.num_batches_tracked) == 0

    # non-contiguous input (a strided view of a wider tensor)
    wide = torch.zeros(shape[:3] + (2 * shape[3],), dtype=dtype, device=DEV)
    wide[..., ::2] = _dev(c["x"])
    xs = wide[..., ::2].requires_grad_(True)
    assert not xs.is_contiguous()
    y2 = m(xs, res)
    _close(y2, c["y"], **_tol(dtype))
    (dx2,) = torch.autograd.grad(y2, xs, _dev(c["dy"], channels_last))
    _close(dx2, c["dx"], **_tol(dtype))


# ----------------------------------------------------------- eval routing
def _eval_module(kind, c):
    C = c["w"].numel()
    if kind == "bn":
        m = msbn.nn.BatchNorm2d(C, EPS)
    elif kind == "sync":
        m = msbn.nn.SyncBatchNorm(C, EPS)
    else:
        m = msbn.nn.SyncBatchNormAct2d(C, EPS, relu=True)
    m.load_state_dict({"weight": c["w"], "bias": c["b"],
                       "running_mean": c["rm"], "running_var": c["rv"],
                       "num_batches_tracked": torch.tensor(3)})
    return m.to(DEV).eval()


@pytest.mark.parametrize("kind,with_res", [("bn", False), ("sync", False),
                                           ("act", False), ("act", True)])
@pytest.mark.parametrize("input_grad", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("shape", [(4, 32, 9, 9), (3, 20, 2, 2)])
def test_eval_routing_trainable_affine(shape, channels_last, dtype,
                                       input_grad, kind, with_res):
    relu = kind == "act"
    c = _case(shape, dtype, relu, with_res)
    m = _eval_module(kind, c)
    x = _dev(c["x"], channels_last).requires_grad_(input_grad)
    res = _dev(c["res"], channels_last)
    if with_res:
        res.requires_grad_(input_grad)
    y = m(x, res) if with_res else m(x)
    _close(y, c["y"], **_tol(dtype))
    leaves = [m.weight, m.bias]
    if input_grad:
        leaves += [x] + ([res] if with_res else [])
    grads = torch.autograd.grad(y, leaves, _dev(c["dy"], channels_last))
    assert grads[0].dtype == torch.float32
    _close(grads[0], c["gw"], **PTOL)
    _close(grads[1], c["gb"], **PTOL)
    if input_grad:
        _close(grads[2], c["dx"], **_tol(dtype))
        if with_res:
            _close(grads[3], c["dres"], **_tol(dtype))
    # eval mode: the statistics are untouched
    assert torch.equal(m.running_var.cpu(), c["rv"])
    assert int(m.num_batches_tracked) == 3


# ------------------------------------------------- not the composed path
@pytest.mark.parametrize("relu", [False, True])
def test_saves_no_fp32_copies(relu):
    shape = (2, 24, 4, 6)
    c = _case(shape, torch.bfloat16, relu, False)
    m = _frozen_module(c, relu)
    x = _dev(c["x"]).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(
            lambda t: (saved.append(t), t)[1], lambda t: t):
        y = m(x)
    n = x.numel()
    if relu:
        assert not any(t.numel() == n and t.dtype == torch.float32
                       for t in saved)
    else:
        assert not any(t.numel() == n for t in saved)
    (dx,) = torch.autograd.grad(y, x, _dev(c["dy"]))
    _close(dx, c["dx"], **_tol(torch.bfloat16))


# ------------------------------------------------------------ edge cases
@pytest.mark.parametrize("relu", [False, True])
def test_empty_input(relu):
    m = FrozenBatchNorm2d(16, relu=relu).to(DEV)
    x = torch.empty(0, 16, 4, 4, device=DEV, requires_grad=True)
    res = torch.empty(0, 16, 4, 4, device=DEV, requires_grad=True)
    y = m(x, res)
    assert y.shape == x.shape
    dx, dres = torch.autograd.grad(y, (x, res), torch.empty_like(y))
    assert dx.shape == x.shape and dres.shape == x.shape
    # trainable affine in eval mode: zero parameter gradients
    bn = msbn.nn.SyncBatchNormAct2d(16, relu=relu).to(DEV).eval()
    y = bn(x, res)
    gw, gb, dx = torch.autograd.grad(y, (bn.weight, bn.bias, x),
                                     torch.empty_like(y))
    assert dx.shape == x.shape
    assert torch.equal(gw, torch.zeros_like(gw))
    assert torch.equal(gb, torch.zeros_like(gb))
    torch.cuda.synchronize()


def test_hipgraph_capture_forward_backward():
    shape = (4, 16, 6, 6)
    c1 = _case(shape, torch.float32, True, True)
    m = _frozen_module(c1, True)
    sx = torch.zeros(shape, device=DEV, requires_grad=True)
    sr = torch.zeros(shape, device=DEV, requires_grad=True)
    sg = torch.zeros(shape, device=DEV)

    def step():
        y = m(sx, sr)
        dx, dr = torch.autograd.grad(y, (sx, sr), sg)
        return y, dx, dr

    def load(seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            sx.copy_(torch.randn(shape, generator=g) * 2 + 0.5)
            sr.copy_(torch.randn(shape, generator=g))
            sg.copy_(torch.randn(shape, generator=g))

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    for seed in (1, 2):
        load(seed)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = step()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert got[0].abs().sum().item() > 0
