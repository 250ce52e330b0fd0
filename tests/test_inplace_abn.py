"""In-place activated SyncBatchNorm (``SyncBatchNormAct2d(inplace=True)``)
on the CPU: storage, errors, equivalence with the out-of-place module, the
fuse pass, pickling, and two gloo ranks against the float64 oracle of the
whole batch.

The world-2 case follows tests/test_sync_oracle.py: every rank builds the
same global batch, runs its slice, and is held to the float64 statistics of
the whole batch (``oracle64``, that file's ``_check_*`` bounds) and, for the
gradients, to ``inplace_oracle`` evaluated on the whole batch's STORED output
(the ranks exchange their y): the in-place backward is a function of y, and a
float64 oracle that started from x instead would differ from it by the
rounding of y itself, which no summation bound describes.  Bounds (u = 2^-24):

* y, fp32: 4*2^-23 * (|x*scale| + |shift|) (test_sync_oracle._y_bound).
* sums of one rank: RED_K*abs_dy, and RED_K*abs_xmu + RECON_K*abs_recon
  (derived in tests/test_gpu_inplace_abn.py) + rtol*|sum| for the fp32
  statistics the kernel's 1/scale is formed from.
* dx, fp32: 4*2^-23 * (|a*g| + |bz*z| + |dz|), the three fp32 terms the
  in-place kernel adds, plus the propagated error of the two global sums as
  in test_sync_oracle._dx_bound; bf16: ``_tol(bf16)``.
"""

import copy
import io
import pickle

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

import inplace_oracle as ipo
import msbn
import multirank_harness as harness
import oracle64 as o64
from leaky_inputs import EPS, gated_inputs
from msbn.nn import fuse_bn_act
from msbn.nn.fused import SyncBatchNormAct2d
from test_gpu_reduction_edges import (RED_K, U, _check_coefs, _check_running,
                                      _check_stats, _stat_bounds, _tol,
                                      _within)

F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(4, 32, 9, 9), (2, 24, 8, 8), (3, 20, 7, 7)]
# (relu, negative_slope)
ACTS = [(True, 0.2), (True, 0.01), (False, 0.0)]
ACT_IDS = ["leaky0.2", "leaky0.01", "identity"]
# roundings of the reconstruction of x - mean from y, see the derivation in
# tests/test_gpu_inplace_abn.py
RECON_K = 7 * U


def _module(C, relu, slope, inplace, d=None):
    m = SyncBatchNormAct2d(C, eps=EPS, relu=relu, negative_slope=slope,
                           inplace=inplace)
    if d is not None:
        with torch.no_grad():
            m.weight.copy_(d["w"])
            m.bias.copy_(d["b"])
    return m.train()


def _nonleaf(t):
    """(leaf, a fresh non-leaf tensor the in-place layer may overwrite)"""
    leaf = t.detach().clone().requires_grad_(True)
    return leaf, leaf * 1.0


def _run(d, relu, slope, inplace, dtype=F32):
    m = _module(d["x"].shape[1], relu, slope, inplace, d)
    leaf, xin = _nonleaf(d["x"].to(dtype))
    y = m(xin)
    same = y.data_ptr() == xin.data_ptr()
    yv = y.detach().clone()
    y.backward(d["dy"].to(dtype))
    return dict(y=yv, dx=leaf.grad, dw=m.weight.grad, db=m.bias.grad,
                rm=m.running_mean, rv=m.running_var,
                nbt=m.num_batches_tracked, same=same, m=m)


# ------------------------------------------------------------------ storage
def test_output_is_the_input_storage_and_nothing_else_is_saved():
    d = gated_inputs(SHAPES[1])
    m = _module(SHAPES[1][1], True, 0.2, True, d)
    _, xin = _nonleaf(d["x"])
    ptr, version = xin.data_ptr(), xin._version
    y = m(xin)
    assert y.data_ptr() == ptr
    assert xin._version > version
    assert type(y.grad_fn).__name__.startswith(
        "InPlaceSyncBatchNormActFunction")
    big = [t for t in y.grad_fn.saved_tensors if t.numel() == y.numel()]
    assert len(big) == 1 and big[0].data_ptr() == y.data_ptr()
    # the out-of-place module keeps x next to y
    m2 = _module(SHAPES[1][1], True, 0.2, False, d)
    _, xin2 = _nonleaf(d["x"])
    y2 = m2(xin2)
    assert y2.data_ptr() != xin2.data_ptr()


# ------------------------------------------------------------------- errors
def test_constructor_and_forward_errors():
    with pytest.raises(ValueError):
        SyncBatchNormAct2d(8, relu=True, negative_slope=0.0, inplace=True)
    with pytest.raises(ValueError):
        SyncBatchNormAct2d(8, relu=True, negative_slope=0.2, affine=False,
                           inplace=True)
    SyncBatchNormAct2d(8, relu=False, inplace=True)   # identity is fine
    d = gated_inputs(SHAPES[1])
    m = _module(SHAPES[1][1], True, 0.2, True, d)
    with pytest.raises(ValueError):
        m(_nonleaf(d["x"])[1], d["res"])
    with pytest.raises(ValueError):
        m(_nonleaf(d["x"])[1], fork=True)
    leaf = d["x"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="in-place"):
        m(leaf)


def test_reference_ops_reject_plain_relu():
    x = torch.randn(2, 4, 3, 3)
    z, o = torch.zeros(4), torch.ones(4)
    with pytest.raises(RuntimeError):
        msbn.ops.batch_norm_elemt_act_(x, o, z, z, o, True, None, 0.0)
    with pytest.raises(RuntimeError):
        msbn.ops.batch_norm_backward_reduce_inplace(
            x, x, o, o, z, True, True, True, True, None, 0.0)


# ------------------------------------------------------- forward equivalence
@pytest.mark.parametrize("relu,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_equals_out_of_place(shape, relu, slope):
    d = gated_inputs(shape)
    a = _run(d, relu, slope, False)
    b = _run(d, relu, slope, True)
    assert b["same"] and not a["same"]
    for k in ("y", "rm", "rv", "nbt"):
        assert torch.equal(a[k], b[k]), k


def test_eval_mode_takes_the_out_of_place_route():
    d = gated_inputs(SHAPES[1])
    a = _module(SHAPES[1][1], True, 0.2, False, d).eval()
    b = _module(SHAPES[1][1], True, 0.2, True, d).eval()
    x = d["x"].clone()
    y = b(x)
    assert y.data_ptr() != x.data_ptr() and torch.equal(x, d["x"])
    assert torch.equal(y, a(d["x"]))


# ------------------------------------------------------ backward equivalence
@pytest.mark.parametrize("relu,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_matches_out_of_place_fp32(shape, relu, slope):
    d = gated_inputs(shape)
    a = _run(d, relu, slope, False)
    b = _run(d, relu, slope, True)
    for k, tol in (("dx", 1e-4), ("dw", 1e-3), ("db", 1e-3)):
        err = (a[k] - b[k]).abs().max().item()
        print(f"{shape} {relu} {slope} {k}: max|err| {err:.3e}")
        torch.testing.assert_close(b[k], a[k], atol=tol, rtol=tol,
                                   msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("relu,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_matches_out_of_place_bf16(shape, relu, slope):
    """grad_weight is held to the in-place oracle, not to the out-of-place
    module: recovering x - mean from a bf16 y and dividing by weight >= 0.1
    moves sum_dy_xmu by up to 1.2e-1 on these draws, which is the method's
    own cost, not an error of the arithmetic."""
    d = gated_inputs(shape, BF16)
    a = _run(d, relu, slope, False, BF16)
    b = _run(d, relu, slope, True, BF16)
    for k, tol in (("dx", 2e-2), ("db", 1e-3)):
        err = (a[k].float() - b[k].float()).abs().max().item()
        print(f"{shape} {relu} {slope} {k}: max|err| {err:.3e}")
        torch.testing.assert_close(b[k].float(), a[k].float(), atol=tol,
                                   rtol=tol, msg=lambda m, k=k: f"{k}: {m}")
    _, invstd = msbn.ops.batch_norm_stats(d["x"], EPS)
    want = ipo.backward(b["y"], d["dy"], d["w"], d["b"], invstd,
                        slope=slope if relu else None)
    err = (b["dw"].double() - want["grad_weight"]).abs().max().item()
    print(f"{shape} {relu} {slope} dw vs oracle: max|err| {err:.3e}")
    torch.testing.assert_close(b["dw"].double(), want["grad_weight"],
                               atol=1e-3, rtol=1e-3)


# ------------------------------------------------------------- the fuse pass
def test_fuse_bn_act_inplace_discriminator_step():
    torch.manual_seed(11)
    a = msbn.convert_sync_batchnorm(msbn.models.Discriminator(ndf=16))
    b = msbn.models.Discriminator(ndf=16)
    b.load_state_dict(a.state_dict())
    b = fuse_bn_act(msbn.convert_sync_batchnorm(b), inplace=True)
    acts = [m for m in b.modules() if isinstance(m, SyncBatchNormAct2d)]
    assert len(acts) == 3 and all(m.inplace for m in acts)
    assert list(a.state_dict()) == list(b.state_dict())
    a.train(), b.train()
    x = torch.randn(8, 3, 64, 64)
    t = torch.ones(8, 1)
    ya, yb = a(x), b(x)
    torch.testing.assert_close(ya, yb, atol=1e-3, rtol=1e-3)
    F.binary_cross_entropy_with_logits(ya, t).backward()
    F.binary_cross_entropy_with_logits(yb, t).backward()
    for (n1, p1), (n2, p2) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(p1.grad, p2.grad, atol=5e-3, rtol=5e-3,
                                   msg=lambda m, n=n1: f"{n}: {m}")


def test_fuse_bn_act_inplace_leaves_relu_pairs_out_of_place():
    net = nn.Sequential(nn.Conv2d(3, 8, 1), nn.BatchNorm2d(8), nn.ReLU(),
                        nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8),
                        nn.LeakyReLU(0.1),
                        nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8, affine=False),
                        nn.LeakyReLU(0.1))
    net = fuse_bn_act(nn.Sequential(net), inplace=True)
    acts = [m for m in net.modules() if isinstance(m, SyncBatchNormAct2d)]
    assert [m.inplace for m in acts] == [False, True, False]
    assert not any(m.inplace for m in fuse_bn_act(nn.Sequential(nn.Sequential(
        nn.BatchNorm2d(8), nn.LeakyReLU(0.1)))).modules()
        if isinstance(m, SyncBatchNormAct2d))


# ------------------------------------------------------ pickle / state dict
def test_inplace_module_pickle_and_state_dict():
    d = gated_inputs(SHAPES[1])
    C = SHAPES[1][1]
    m = _module(C, True, 0.2, True, d)
    want = m(_nonleaf(d["x"])[1]).detach().clone()
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)),
                  torch.load(io.BytesIO(_saved(m)), weights_only=False)):
        assert clone.inplace is True and "inplace=True" in repr(clone)
        _, xin = _nonleaf(d["x"])
        y = clone(xin)
        assert y.data_ptr() == xin.data_ptr() and torch.equal(y, want)
    assert "inplace" not in m.state_dict()
    plain = msbn.nn.SyncBatchNorm(C, eps=EPS)
    plain.load_state_dict(m.state_dict())
    assert list(plain.state_dict()) == list(m.state_dict())
    # a module pickled before the attribute existed is out of place
    old = _module(C, True, 0.2, False, d)
    del old.__dict__["inplace"]
    _, xin = _nonleaf(d["x"])
    assert old(xin).data_ptr() != xin.data_ptr()
    assert "inplace" not in repr(old)


def _saved(mod):
    buf = io.BytesIO()
    torch.save(mod, buf)
    return buf.getvalue()


# --------------------------------------------------------- two ranks, gloo
C2 = 8
PLANE = (5, 5)
SLOPE = 0.2
MOMENTUM = 0.1
# name -> per-rank batch sizes; the second has an empty rank
RANK_SIZES = {"uneven": (3, 2), "empty": (5, 0)}


def global_batch(sizes, C2, plane, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    H, W = plane
    x = torch.cat([torch.randn(n, C2, H, W, generator=g) * (1 + r) + 3 * r
                   for r, n in enumerate(sizes)]).to(dtype)
    return {
        "x": x,
        "dy": torch.randn(N, C2, H, W, generator=g).to(dtype),
        "w": 8 * (torch.randn(C2, generator=g).abs() + 0.1),
        "b": -torch.randn(C2, generator=g).abs(),
        "rm0": torch.randn(C2, generator=g),
        "rv0": torch.rand(C2, generator=g) + 0.5,
    }


def _cl(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) \
        if channels_last else t.contiguous()


def run_rank_case(rank, world, device, case):
    """One in-place layer on one rank (harness case function): run every
    collective, then check; returns the failures."""
    name, sizes, C2, plane, dtype, cl, seed = case
    d = global_batch(sizes, C2, plane, dtype, seed)
    off, n_loc = sum(sizes[:rank]), sizes[rank]
    n = sum(sizes) * plane[0] * plane[1]
    tag = f"[{name} r{rank}]"
    on_gpu = device != "cpu"

    m = SyncBatchNormAct2d(C2, EPS, MOMENTUM, relu=True, negative_slope=SLOPE,
                           inplace=True).to(device).train()
    with torch.no_grad():
        m.weight.copy_(d["w"])
        m.bias.copy_(d["b"])
        m.running_mean.copy_(d["rm0"])
        m.running_var.copy_(d["rv0"])
    leaf = _cl(d["x"][off:off + n_loc].to(device), cl).requires_grad_(True)
    xin = leaf * 1.0
    xs = xin.detach().clone()
    dys = _cl(d["dy"][off:off + n_loc].to(device), cl)
    y = m(xin)
    same = y.data_ptr() == xin.data_ptr()
    node = y.grad_fn
    mean, invstd, count_sum = node.saved_tensors[3:6]
    coefs = node.saved_tensors[6] if node.has_coefs else None
    y_loc = y.detach().clone()
    dx, dw, db = torch.autograd.grad(y, (leaf, m.weight, m.bias), dys)
    ys = [None] * world
    dist.all_gather_object(ys, y_loc.cpu())
    running = torch.cat([m.running_mean, m.running_var]).detach().clone()
    everyone = [torch.empty_like(running) for _ in range(world)]
    dist.all_gather(everyone, running)
    if on_gpu:
        torch.cuda.synchronize()

    failures = []

    def ck(fn, *a):
        try:
            fn(*a)
        except AssertionError as e:
            failures.append(str(e))

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {what}")

    expect(same, "the output does not live in the input's storage")
    expect(node.has_coefs == on_gpu, f"has_coefs {node.has_coefs}")
    X, DY = d["x"].to(device), d["dy"].to(device)
    w, b = d["w"].to(device), d["b"].to(device)
    mean64, var64, invstd64 = o64.stats(X, EPS)
    rtol, matol = _stat_bounds(mean64, var64)
    expect(count_sum.numel() == 1 and count_sum.item() == float(n),
           f"count_sum {count_sum.tolist()} != {n}")
    ck(_check_stats, tag, mean, invstd, mean64, var64)
    if coefs is not None:
        ck(_check_coefs, tag, coefs, mean64, var64, w, b)
    ck(_check_running, tag, m.running_mean, m.running_var,
       d["rm0"].to(device), d["rv0"].to(device), mean64, var64, n, MOMENTUM)
    expect(all(torch.equal(e, running) for e in everyone),
           "running statistics differ between ranks")
    expect(dx is not None and dx.shape == xs.shape and dx.dtype == dtype,
           "dx: wrong shape or dtype")
    if n_loc == 0:
        expect(not dw.any().item() and not db.any().item(),
               "empty rank: grad_weight / grad_bias are not zeros")
        return failures

    # forward, against the textbook float64 expression of the whole batch
    nd = xs.dim()
    want_y = o64.elemt(xs, mean64, invstd64, w, b, None, True, SLOPE)
    if dtype == F32:
        scale, shift = o64.coefs(mean64, invstd64, w, b)
        y_bound = 4 * 2.0 ** -23 * ((xs.double() * o64.chan(scale, nd)).abs()
                                    + o64.chan(shift, nd).abs())
    else:
        t = _tol(dtype)
        y_bound = t["atol"] + t["rtol"] * want_y.abs()
    ck(_within, f"{tag} y", y_loc, want_y, y_bound)

    # backward, against the in-place oracle of the whole batch's stored y
    Y = torch.cat([t for t in ys]).to(device)
    RED = ipo.backward(Y, DY, w, b, invstd64, n, SLOPE)
    LOC = ipo.backward(y_loc, dys, w, b, invstd64, n, SLOPE,
                       RED["sum_dy"], RED["sum_dy_xmu"])
    xmu_bound = RED_K * LOC["abs_xmu"] + RECON_K * LOC["abs_recon"]
    ck(_within, f"{tag} grad_bias", db, LOC["grad_bias"],
       RED_K * LOC["abs_dy"])
    ck(_within, f"{tag} grad_weight", dw, LOC["grad_weight"],
       xmu_bound * invstd64 + (rtol + 2 * U) * LOC["grad_weight"].abs())
    if dtype == F32:
        g, z = LOC["g"], LOC["z"]
        f1 = invstd64 * w.double()
        f3 = invstd64 * invstd64 * RED["sum_dy_xmu"] / n
        ca, cbz = f1, -f3          # b/scale with scale == f1
        cdz = -ca * RED["sum_dy"] / n - cbz * b.double()
        terms = ((o64.chan(ca, nd) * g).abs() + (o64.chan(cbz, nd) * z).abs()
                 + o64.chan(cdz, nd).abs())
        xmu = ((z - o64.chan(b.double(), nd)) / o64.chan(f1, nd)).abs()
        red_xmu = (RED_K * RED["abs_xmu"] + RECON_K * RED["abs_recon"]
                   + rtol * RED["sum_dy_xmu"].abs())
        red_err = o64.chan(f1.abs(), nd) * (
            o64.chan(RED_K * RED["abs_dy"] / n, nd)
            + xmu * o64.chan(invstd64 * invstd64 * red_xmu / n, nd))
        dx_bound = 4 * 2.0 ** -23 * terms + red_err
    else:
        t = _tol(dtype)
        dx_bound = t["atol"] + t["rtol"] * LOC["dx"].abs()
    ck(_within, f"{tag} dx", dx, LOC["dx"], dx_bound)
    return failures


def test_inplace_sync_world2_gloo(tmp_path):
    cases = [(name, sizes, C2, PLANE, F32, False, 40 + i)
             for i, (name, sizes) in enumerate(RANK_SIZES.items())]
    outputs = harness.run_cases(tmp_path, 2, "cpu",
                                "test_inplace_abn:run_rank_case", cases)
    assert sorted(outputs) == [0, 1]
    for rank, per_case in outputs.items():
        for _, text in per_case:
            print(text, end="")
