"""Fork-gradient fold, CPU side: a fused BN whose output feeds two consumers
returns it as a (main, skip) pair, so its backward receives the two
gradients unsummed (msbn/nn/fused.py).  On the CPU the backward starts with
the one add autograd itself would have run, so everything here is bit-exact
against the unforked wiring.  The GPU kernels that read both gradients are
covered in test_gpu_grad_fork.py."""

import pytest
import torch

from msbn import ops
from msbn.models import resnet18, resnet50
from msbn.nn.fused import SyncBatchNormAct2d

SHAPE = (4, 6, 5, 7)
# (relu, negative_slope)
ACTS = [(False, 0.0), (True, 0.0), (True, 0.1)]


def _pair(relu, slope, seed=0):
    """Two modules with the same (non-trivial) affine parameters."""
    C = SHAPE[1]
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, generator=g).abs() + 0.1
    b = torch.randn(C, generator=g)
    out = []
    for _ in range(2):
        m = SyncBatchNormAct2d(C, relu=relu, negative_slope=slope).train()
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        out.append(m)
    return out


def _inputs(with_res, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(SHAPE, generator=g) * 2 + 0.5
    res = torch.randn(SHAPE, generator=g) if with_res else None
    g1 = torch.randn(SHAPE, generator=g)
    g2 = torch.randn(SHAPE, generator=g)
    return x, res, g1, g2


def _leaves(x, res):
    xl = x.clone().requires_grad_(True)
    rl = res.clone().requires_grad_(True) if res is not None else None
    return xl, rl


def _grads(m, xl, rl):
    out = [xl.grad, m.weight.grad, m.bias.grad]
    if rl is not None:
        out.append(rl.grad)
    return out


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu,slope", ACTS, ids=["none", "relu", "leaky"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_forked_module_matches_unforked(mode, relu, slope, with_res):
    forked, plain = _pair(relu, slope)
    getattr(forked, mode)()
    getattr(plain, mode)()
    x, res, g1, g2 = _inputs(with_res)

    xa, ra = _leaves(x, res)
    main, skip = forked(xa, ra, fork=True)
    assert main.untyped_storage().data_ptr() == \
        skip.untyped_storage().data_ptr()
    assert main.shape == skip.shape and main.stride() == skip.stride()
    assert main.grad_fn is not None and skip.grad_fn is not None
    if mode == "train":  # both are outputs of the one Function, not views
        assert main.grad_fn is skip.grad_fn
        assert not main._is_view() and not skip._is_view()
    (main * g1 + skip * g2).sum().backward()

    xb, rb = _leaves(x, res)
    y = plain(xb, rb)                  # the same tensor, consumed twice
    assert isinstance(y, torch.Tensor)
    (y * g1 + y * g2).sum().backward()

    assert torch.equal(main, y) and torch.equal(skip, y)
    for a, b in zip(_grads(forked, xa, ra), _grads(plain, xb, rb)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("used", [0, 1], ids=["main_only", "skip_only"])
def test_one_output_unused(used):
    forked, plain = _pair(True, 0.0)
    x, res, g1, _ = _inputs(True)
    xa, ra = _leaves(x, res)
    (forked(xa, ra, fork=True)[used] * g1).sum().backward()
    xb, rb = _leaves(x, res)
    (plain(xb, rb) * g1).sum().backward()
    for a, b in zip(_grads(forked, xa, ra), _grads(plain, xb, rb)):
        assert torch.equal(a, b)


def test_default_returns_a_tensor():
    m, _ = _pair(True, 0.0)
    x, res, _, _ = _inputs(True)
    assert isinstance(m(x, res), torch.Tensor)
    assert isinstance(m.eval()(x, res), torch.Tensor)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("make", [resnet18, resnet50],
                         ids=["resnet18", "resnet50"])
def test_forked_resnet_matches_unforked(make, mode):
    torch.manual_seed(0)
    forked = make(num_classes=10, fused=True)
    torch.manual_seed(0)
    plain = make(num_classes=10, fused=True, fork_grads=False)
    torch.manual_seed(0)
    unfused = make(num_classes=10)
    assert list(forked.state_dict()) == list(plain.state_dict())
    assert list(forked.state_dict()) == list(unfused.state_dict())
    assert [n for n, _ in forked.named_modules()] == \
        [n for n, _ in plain.named_modules()]
    # every block forks but the last of layer4
    blocks = [b for layer in (forked.layer1, forked.layer2, forked.layer3,
                              forked.layer4) for b in layer]
    assert [b.fork for b in blocks] == [True] * (len(blocks) - 1) + [False]
    assert not any(b.fork for layer in (plain.layer1, plain.layer4)
                   for b in layer)

    getattr(forked, mode)()
    getattr(plain, mode)()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    ya, yb = forked(xa), plain(xb)
    assert torch.equal(ya, yb)
    feats = forked.forward_features(x)
    assert len(feats) == 4 and all(isinstance(f, torch.Tensor) for f in feats)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    for (n, p), (_, q) in zip(forked.named_parameters(),
                              plain.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_reference_sums_in_the_input_dtype():
    """The CPU op: grad_out2 is added in the input dtype first (one
    rounding), like the eager add the GPU kernel replaces."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(SHAPE, generator=g) * 2).to(torch.bfloat16)
    g1 = torch.randn(SHAPE, generator=g).to(torch.bfloat16)
    g2 = torch.randn(SHAPE, generator=g).to(torch.bfloat16)
    C = SHAPE[1]
    mean = torch.randn(C, generator=g)
    invstd = torch.rand(C, generator=g) + 0.5
    w = torch.rand(C, generator=g) + 0.1
    b = torch.randn(C, generator=g)
    gm_a, gm_b = torch.empty_like(x), torch.empty_like(x)
    got = ops.batch_norm_backward_reduce_act(
        g1, x, None, mean, invstd, w, b, True, True, True, True, None, gm_a,
        0.0, g2)
    want = ops.batch_norm_backward_reduce_act(
        g1 + g2, x, None, mean, invstd, w, b, True, True, True, True, None,
        gm_b, 0.0)
    assert torch.equal(gm_a, gm_b)
    for a, bb in zip(got, want):
        assert torch.equal(a, bb)


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["float32", "bfloat16"])
def test_launch_plan_sees_a_misaligned_dy2(dtype, cl):
    """dy2 is one more pointer the kernel loads V-wide packs from: one
    element off an aligned address and the whole launch drops to V = 1.
    launch_plan is host-only, so CPU tensors do."""
    shape = (4, 8, 4, 16)
    vmax = 16 // torch.empty((), dtype=dtype).element_size()
    fmt = torch.channels_last if cl else torch.contiguous_format
    x = torch.empty(shape, dtype=dtype).contiguous(memory_format=fmt)
    dy, res, gm = (torch.empty_like(x) for _ in range(3))
    n = x.numel()
    flat = torch.empty(n + 64, dtype=dtype)[1:1 + n]
    if cl:
        N, C, H, W = shape
        dy2 = flat.view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        dy2 = flat.view(shape)
    assert dy2.stride() == x.stride()
    assert dy2.data_ptr() % 16 == x.element_size()
    aligned = ops.launch_plan("bwd_reduce", x,
                              (dy, res, gm, torch.empty_like(x)))
    assert aligned["V"] == vmax, aligned
    off = ops.launch_plan("bwd_reduce", x, (dy, res, gm, dy2))
    assert off["V"] == 1, off
    assert off["path"] == ("nhwc" if cl else "nchw_flat"), off
