"""GPU edges of the BatchNorm kernels the small-tensor suite never reaches.

Every case first asserts, through ``ops.launch_plan`` (host-only, same code
the ops launch with), the property it exists for — more than 64 chunks into
the finalize kernel, a loop that runs past the accumulator's flush period,
a grid-stride loop that takes a second trip, a reduced vector width — so a
retuned heuristic makes the test fail instead of silently losing coverage.

Reference: ``oracle64`` (float64, textbook ``(x-mean)*invstd*w+b`` form),
evaluated on the device, from the same dtype-rounded inputs.

Tolerances are derived, not tuned (u = 2^-24, fp32 unit roundoff):

* statistics: a correct fp64 combine of {sum x, sum x^2} has conditioning
  cond = mean^2/(var+eps), the outputs are fp32:
    invstd  rtol = max(1e-5, 64 * 2^-53 * cond)   per channel
    mean    atol = 1e-6 * max(|mean|, std)
  scale/shift and the running statistics inherit them (propagated through
  scale = invstd*w, shift = b - mean*scale; running bound scaled by the
  momentum, plus 4u of the fp32 blend (1-m)*old + m*new the kernels do).
* backward reductions: each fp32 partial sum holds at most MSBN_ACC_FLUSH =
  64 terms before it is flushed to fp64, so its error is at most
  63u * sum|t|; a term g*(x-mean) carries two more roundings and the fp32
  result one:  |err| <= 68u * sum|t|.
* elementwise ops: the suite's existing ``_tol(dtype)``.
"""

import pytest
import torch

import msbn
import oracle64 as o64
from msbn import ops

gpu = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
U = 2.0 ** -24
RED_K = 68 * U
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GRID_CAP_THREADS = 4096 * 256


def _tol(dtype):
    return {"atol": 1e-5, "rtol": 1e-5} if dtype == torch.float32 else \
        {"atol": 2e-2, "rtol": 2e-2}


def _cl(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) \
        if channels_last else t.contiguous()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, dtype=F32):
    return torch.randn(shape, generator=g, device=DEV).to(dtype)


def _ordinary(shape, dtype, channels_last, seed):
    """The suite's usual data (randn*2 + 0.5), x / dy / res, on the device."""
    g = _gen(seed)
    x = _cl((_randn(shape, g) * 2 + 0.5).to(dtype), channels_last)
    dy = _cl(_randn(shape, g, dtype), channels_last)
    res = _cl(_randn(shape, g, dtype), channels_last)
    return x, dy, res


def _affine(C, seed):
    g = _gen(seed + 1)
    return (torch.randn(C, generator=g, device=DEV).abs() + 0.1,
            torch.randn(C, generator=g, device=DEV))


def _within(name, got, want, bound):
    """|got - want| <= bound elementwise; prints the figures first."""
    err = (got.double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64,
                            device=err.device).expand_as(err)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300),
                        torch.zeros_like(err))
    print(f"{name}: max|err| {err.max().item():.3e}  "
          f"max err/bound {ratio.max().item():.3e}")
    bad = err > bound
    assert not bad.any().item(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; worst "
        f"err/bound {ratio.max().item():.3e} at flat index "
        f"{int(ratio.flatten().argmax())}")


# ------------------------------------------------------------ stat bounds
def _stat_bounds(mean, var):
    """(invstd rtol[C], mean atol[C]) from the oracle's float64 statistics."""
    cond = mean * mean / (var + EPS)
    rtol = torch.clamp(64 * 2.0 ** -53 * cond, min=1e-5)
    matol = 1e-6 * torch.maximum(mean.abs(), var.sqrt())
    return rtol, matol


def _check_stats(tag, got_mean, got_invstd, mean, var):
    rtol, matol = _stat_bounds(mean, var)
    invstd = torch.rsqrt(var + EPS)
    _within(tag + " mean", got_mean, mean, matol)
    _within(tag + " invstd", got_invstd, invstd, rtol * invstd)


def _check_coefs(tag, coefs, mean, var, w, b):
    C = mean.numel()
    rtol, matol = _stat_bounds(mean, var)
    scale, shift = o64.coefs(mean, torch.rsqrt(var + EPS), w, b)
    scale_b = (rtol + 2 * U) * scale.abs()
    shift_b = (mean.abs() * scale_b + matol * scale.abs()
               + 2 * U * ((mean * scale).abs() + b.double().abs()))
    _within(tag + " scale", coefs[:C], scale, scale_b)
    _within(tag + " shift", coefs[C:], shift, shift_b)


def _check_running(tag, rm, rv, rm0, rv0, mean, var, count, momentum):
    rtol, matol = _stat_bounds(mean, var)
    want_m, want_v = o64.running_update(rm0, rv0, mean, var, count, momentum)
    unb = var * (count / (count - 1.0))
    blend_m = 4 * U * ((1 - momentum) * rm0.double().abs()
                       + momentum * mean.abs())
    blend_v = 4 * U * ((1 - momentum) * rv0.double().abs() + momentum * unb)
    _within(tag + " running_mean", rm, want_m, momentum * matol + blend_m)
    # d var / var = 2 d invstd / invstd (of var + eps)
    _within(tag + " running_var", rv, want_v,
            momentum * 2 * rtol * (unb + EPS) + blend_v)


# --------------------------------------------------- backward-reduce check
def _nudge(x, res, mean, invstd, w, b, offcentre=False):
    """Move x by +1 wherever the pre-activation is too close to zero for the
    gate to be unambiguous between fp32 fused-multiply and textbook fp64."""
    for _ in range(64):
        z = o64.pre_activation(x, mean, invstd, w, b, res)
        band = 1e-3
        if offcentre:
            sc, sh = o64.coefs(mean, invstd, w, b)
            mag = (x.double() * o64.chan(sc, x.dim())).abs() \
                + o64.chan(sh, x.dim()).abs()
            band = 1e-3 + 32 * U * mag
        near = z.abs() < band
        if not near.any().item():
            return x
        x = torch.where(near, x.float() + 1.0, x.float()).to(x.dtype)
    raise AssertionError("could not separate the pre-activations from zero")


# (act, slope, with_res, want_gm)
BWD_COMBOS = [(False, 0.0, False, False), (True, 0.0, False, False),
              (True, 0.25, True, True)]


def _check_bwd_reduce(tag, x, dy, res, mean32, invstd32, w, b, combo,
                      offcentre=False):
    act, slope, with_res, want_gm = combo
    r = res if with_res else None
    if act:
        xn = _nudge(x, r, mean32, invstd32, w, b, offcentre)
        # keep the memory format of x
        x = xn.contiguous(memory_format=torch.channels_last) \
            if (x.dim() == 4 and not x.is_contiguous()) else xn.contiguous()
    gm = torch.empty_like(x) if want_gm else None
    sum_dy, sum_dy_xmu, gw, gb = ops.batch_norm_backward_reduce_act(
        dy, x, r, mean32, invstd32, w, b, act, True, True, True, None, gm,
        slope)
    want = o64.backward_reduce(dy, x, mean32, invstd32, w, b, r, act, slope)
    name = f"{tag} act={act} slope={slope} res={with_res}"
    _within(name + " sum_dy", sum_dy, want["sum_dy"],
            RED_K * want["abs_dy"])
    _within(name + " sum_dy_xmu", sum_dy_xmu, want["sum_dy_xmu"],
            RED_K * want["abs_xmu"])
    _within(name + " grad_bias", gb, want["grad_bias"],
            RED_K * want["abs_dy"])
    _within(name + " grad_weight", gw, want["grad_weight"],
            RED_K * want["abs_xmu"] * invstd32.double()
            + 2 * U * want["grad_weight"].abs())
    if want_gm:  # slope 0.25 scales exactly: the gated gradient is bit-exact
        assert torch.equal(gm, want["g"].to(x.dtype))


def _stats32(x):
    mean, var, invstd = o64.stats(x, EPS)
    return mean, var, mean.float(), invstd.float()


# =================================================================
# finalize with > 64 chunks (count not a multiple of 64), and loops
# that run past the flush period
# =================================================================
# (path, shape, dtype, channels_last, V)
FINALIZE_CASES = [
    ("nchw_vec", (100, 4, 4, 4), F32, False, 4),
    ("nchw_vec", (100, 4, 4, 4), BF16, False, 8),
    ("nchw_flat", (70, 2, 31, 31), F32, False, 1),
    ("nhwc", (3, 8, 53, 53), F32, True, 4),
    ("nhwc", (2, 2048, 42, 50), BF16, True, 8),   # channel-tiled: ctiles 16
]
LOOP_CASES = [
    ("nchw_vec", (1030, 256, 2, 2), F32, False, 4),
    ("nchw_vec", (1030, 256, 2, 4), BF16, False, 8),
    ("nchw_flat", (130, 2048, 1, 127), F32, False, 1),
    ("nhwc", (4, 3, 1030, 1030), BF16, True, 1),
]
MULTI_S_CASE = ("nchw_vec", (2, 8, 72, 72), F32, False, 4)


def _assert_property(kind, plan, case):
    path, shape, _, _, V = case
    assert plan["path"] == path and plan["V"] == V, plan
    if kind == "finalize":
        assert plan["nchunks"] > 64 and plan["nchunks"] % 64 != 0, plan
        assert plan["finalize_trips"] >= 2, plan
        if shape[1] == 2048:
            assert plan["ctiles"] == 16, plan
    elif kind == "loop":
        assert plan["trips"] > plan["flush_every"], plan
        assert plan["trips"] % plan["flush_every"] != 0, plan
    else:  # several S-chunks, and a last trip only part of the block joins
        S = shape[2] * shape[3]
        assert plan["nchunkS"] > 1 and plan["chunkS"] < S, plan
        assert (S // V) % 256 != 0, plan


REDUCTION_CASES = ([("finalize", c) for c in FINALIZE_CASES]
                   + [("loop", c) for c in LOOP_CASES]
                   + [("multi_s", MULTI_S_CASE)])


def _case_id(p):
    kind, (path, shape, dtype, cl, _) = p
    return f"{kind}-{path}-{'x'.join(map(str, shape))}-{str(dtype)[6:]}"


def test_launch_plan_is_host_only():
    """launch_plan only looks at shapes, strides and pointers: it answers for
    CPU tensors too, so the properties the GPU cases rely on are checked on
    machines without a GPU as well (uninitialised memory, nothing touched)."""
    for kind, case in REDUCTION_CASES:
        _, shape, dtype, cl, _ = case
        x = _cl(torch.empty(shape, dtype=dtype), cl)
        _assert_property(kind, ops.launch_plan("stats", x), case)
        _assert_property(
            kind, ops.launch_plan("bwd_reduce", x, (x, None, None)), case)
    for shape, dtype, cl, V in GRID_CASES:
        x = _cl(torch.empty(shape, dtype=dtype), cl)
        for kind in ("elemt", "bwd_elemt", "frozen_bwd_elemt"):
            _assert_grid(ops.launch_plan(kind, x), V)
    # the small-plane kernels are GPU-only
    assert ops.launch_plan("fused_local",
                           torch.empty(4, 64, 16, 16))["path"] == "ineligible"
    with pytest.raises(RuntimeError):
        ops.launch_plan("no_such_op", torch.empty(2, 4, 4, 4))


@gpu
@pytest.mark.parametrize("kind,case", REDUCTION_CASES,
                         ids=[_case_id(p) for p in REDUCTION_CASES])
def test_stats_reduction_edges(kind, case):
    _, shape, dtype, cl, _ = case
    x, _, _ = _ordinary(shape, dtype, cl, seed=sum(shape))
    _assert_property(kind, ops.launch_plan("stats", x), case)
    mean, var, _, _ = _stats32(x)
    got_mean, got_invstd = ops.batch_norm_stats(x, EPS)
    _check_stats("stats", got_mean, got_invstd, mean, var)


@gpu
@pytest.mark.parametrize("combo", BWD_COMBOS,
                         ids=["plain", "relu", "leaky_res_gm"])
@pytest.mark.parametrize("kind,case", REDUCTION_CASES,
                         ids=[_case_id(p) for p in REDUCTION_CASES])
def test_backward_reduction_edges(kind, case, combo):
    _, shape, dtype, cl, _ = case
    x, dy, res = _ordinary(shape, dtype, cl, seed=sum(shape))
    others = (dy, res if combo[2] else None,
              torch.empty_like(x) if combo[3] else None)
    _assert_property(kind, ops.launch_plan("bwd_reduce", x, others), case)
    _, _, mean32, invstd32 = _stats32(x)
    w, b = _affine(shape[1], sum(shape))
    _check_bwd_reduce("bwd", x, dy, res, mean32, invstd32, w, b, combo)


# =================================================================
# off-centre and degenerate statistics, on every reduction path
# =================================================================
SPECS32 = [(100.0, 1.0), (1000.0, 1.0), (1000.0, 0.1), (-4096.0, 1.0),
           "const", "zero", "outlier"]
SPECS16 = [(100.0, 1.0), (-60.0, 0.5), "const", "zero", "outlier"]


def _offcentre(shape, dtype, seed=0):
    """CPU fp32 -> rounded to dtype.  Channel c follows spec c % len(specs):
    mean + std*randn, constant 100.1, constant 0, or an ordinary channel
    whose very first element is +1000."""
    specs = SPECS32 if dtype == F32 else SPECS16
    g = torch.Generator().manual_seed(seed + 17 * sum(shape))
    x = torch.randn(shape, generator=g)
    for c in range(shape[1]):
        s = specs[c % len(specs)]
        if s == "const":
            x[:, c] = 100.1
        elif s == "zero":
            x[:, c] = 0.0
        elif s == "outlier":
            x[:, c] = x[:, c] * 2 + 0.5
            x[0, c].view(-1)[0] = 1000.0
        else:
            x[:, c] = s[0] + s[1] * x[:, c]
    dy = torch.randn(shape, generator=g)
    res = torch.randn(shape, generator=g)
    return x.to(dtype), dy.to(dtype), res.to(dtype)


# path -> (plane ~1K shape, plane ~16K shape, channels_last)
OFFCENTRE_SHAPES = {
    "nchw_vec": ((4, 8, 16, 16), (16, 8, 32, 32), False),
    "nchw_flat": ((4, 8, 15, 17), (16, 8, 31, 33), False),
    "nhwc": ((4, 8, 16, 16), (16, 8, 32, 32), True),
    "small_plane": ((4, 64, 16, 16), (16, 64, 32, 32), False),
}
OFFCENTRE_CASES = [(path, shp[i], dtype)
                   for path, shp in OFFCENTRE_SHAPES.items()
                   for i in (0, 1) for dtype in (F32, BF16, F16)]
MOMENTUM = 0.1


def _running0(C):
    g = _gen(C)
    return (torch.randn(C, generator=g, device=DEV),
            torch.rand(C, generator=g, device=DEV) + 0.5)


@gpu
@pytest.mark.parametrize(
    "path,shape,dtype", OFFCENTRE_CASES,
    ids=[f"{p}-{'x'.join(map(str, s))}-{str(d)[6:]}"
         for p, s, d in OFFCENTRE_CASES])
def test_offcentre_statistics(path, shape, dtype):
    cl = OFFCENTRE_SHAPES[path][2]
    xc, dyc, resc = _offcentre(shape, dtype)
    x, dy, res = (_cl(t.to(DEV), cl) for t in (xc, dyc, resc))
    N, C = shape[0], shape[1]
    count = x.numel() // C
    mean, var, mean32, invstd32 = _stats32(x)
    w, b = _affine(C, C)
    _C = ops._require_hip()

    if path == "small_plane":
        plan = ops.launch_plan("fused_local", x)
        assert plan["path"] == "small_plane" and plan["V"] > 1, plan
        rm0, rv0 = _running0(C)
        rm, rv = rm0.clone(), rv0.clone()
        assert ops.bn_fused_local_eligible(x, w, b, rm, rv)
        y, gm, gi, cnt, coefs = ops.batch_norm_fwd_fused_local(
            x, None, w, b, EPS, MOMENTUM, rm, rv, False)
        assert cnt.item() == count
        _check_stats("fused_local", gm, gi, mean, var)
        _check_coefs("fused_local", coefs, mean, var, w, b)
        _check_running("fused_local", rm, rv, rm0, rv0, mean, var, count,
                       MOMENTUM)
        # the single-launch backward's reductions
        for act, slope, with_res, _ in BWD_COMBOS:
            r = res if with_res else None
            xb = _nudge(x, r, mean32, invstd32, w, b, True) if act else x
            fc = ops.bn_make_coefs(mean32, invstd32, w, b)
            _, gw, gb, _ = ops.batch_norm_bwd_fused_local(
                dy, xb, r, mean32, invstd32, w, fc, act, False, True, True,
                slope)
            want = o64.backward_reduce(dy, xb, mean32, invstd32, w, b, r,
                                       act, slope)
            _within(f"fused_local act={act} grad_bias", gb,
                    want["grad_bias"], RED_K * want["abs_dy"])
            _within(f"fused_local act={act} grad_weight", gw,
                    want["grad_weight"],
                    RED_K * want["abs_xmu"] * invstd32.double()
                    + 2 * U * want["grad_weight"].abs())
        return

    plan = ops.launch_plan("stats", x)
    assert plan["path"] == path, plan
    assert ops.launch_plan("fused_local", x)["path"] == "ineligible"

    # two-stage stats
    got_mean, got_invstd = ops.batch_norm_stats(x, EPS)
    _check_stats("stats", got_mean, got_invstd, mean, var)

    # fused local finalize: running statistics + coefs in the same launch
    rm0, rv0 = _running0(C)
    rm, rv = rm0.clone(), rv0.clone()
    lm, li, lc, coefs = _C.batch_norm_stats_local(x, EPS, rm, rv, MOMENTUM,
                                                  w, b, True)
    assert lc.item() == count
    _check_stats("stats_local", lm, li, mean, var)
    _check_coefs("stats_local", coefs, mean, var, w, b)
    _check_running("stats_local", rm, rv, rm0, rv0, mean, var, count,
                   MOMENTUM)

    # cross-rank combine: two ranks of unequal count (1/4 and 3/4 of N)
    n1 = N // 4
    packed = torch.empty(2, 2 * C + 1, device=DEV)
    ops.batch_norm_stats_packed(x[:n1], EPS, packed[0])
    ops.batch_norm_stats_packed(x[n1:], EPS, packed[1])
    assert packed[0, 2 * C].item() != packed[1, 2 * C].item()
    rm, rv = rm0.clone(), rv0.clone()
    gmean, ginvstd, gcount, gcoefs = _C.batch_norm_gather_stats_packed_coefs(
        packed, rm, rv, MOMENTUM, EPS, w, b, True)
    assert gcount.item() == count
    _check_stats("gather", gmean, ginvstd, mean, var)
    _check_coefs("gather", gcoefs, mean, var, w, b)
    _check_running("gather", rm, rv, rm0, rv0, mean, var, count, MOMENTUM)

    # backward reductions at these inputs (centred terms: must stay sound)
    for combo in BWD_COMBOS:
        _check_bwd_reduce("bwd", x, dy, res, mean32, invstd32, w, b, combo,
                          offcentre=True)


def test_oracle_float32_agrees_with_float64():
    """The oracle's own float32 evaluation meets the statistic bounds (CPU):
    they are reachable by plain two-pass fp32 arithmetic."""
    for dtype in (F32, BF16, F16):
        for shape in ((4, 8, 16, 16), (16, 8, 32, 32)):
            x, _, _ = _offcentre(shape, dtype)
            mean, var, _ = o64.stats(x, EPS)
            m32, v32, i32 = o64.stats(x, EPS, dtype=torch.float32)
            assert m32.dtype == torch.float32
            _check_stats(f"oracle32 {shape} {dtype}", m32, i32, mean, var)


@gpu
def test_syncbn_module_two_stage_offcentre():
    """msbn.nn.SyncBatchNorm (world size 1, two-stage path) on channels at
    (100, 1) against torch.nn.functional.batch_norm in float64.

    y and dx are held to 4 * 2^-23 * (sum of magnitudes of the fp32 terms
    the kernel adds): |x*scale| + |shift| forward, |a*dy| + |b*x| + |d|
    backward.  That is the known cost of the fused-multiply form — at
    mean 100 the forward adds two terms of magnitude ~100*scale to produce
    an output of magnitude ~1 — and this test documents it."""
    shape, C = (8, 32, 24, 24), 32
    g = torch.Generator().manual_seed(5)
    x = (100.0 + torch.randn(shape, generator=g)).to(DEV)
    dy = torch.randn(shape, generator=g).to(DEV)
    w, b = _affine(C, 3)
    rm0, rv0 = _running0(C)
    n = x.numel() // C

    assert ops.launch_plan("fused_local", x)["path"] == "ineligible"
    assert ops.launch_plan("stats", x)["path"] == "nchw_vec"

    m = msbn.nn.SyncBatchNorm(C, EPS, MOMENTUM).to(DEV).train()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        m.running_mean.copy_(rm0)
        m.running_var.copy_(rv0)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    dx, dw, db = torch.autograd.grad(y, (xg, m.weight, m.bias), dy)

    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    rm64, rv64 = rm0.double(), rv0.double()
    y64 = torch.nn.functional.batch_norm(x64, rm64, rv64, w64, b64, True,
                                         MOMENTUM, EPS)
    dx64, dw64, db64 = torch.autograd.grad(y64, (x64, w64, b64), dy.double())

    mean, var, invstd = o64.stats(x, EPS)
    rtol, matol = _stat_bounds(mean, var)
    scale, shift = o64.coefs(mean, invstd, w, b)
    nd = x.dim()
    xd, dyd = x.double(), dy.double()
    fwd_terms = (xd * o64.chan(scale, nd)).abs() + o64.chan(shift, nd).abs()
    _within("module y", y, y64.detach(), 4 * 2.0 ** -23 * fwd_terms)

    red = o64.backward_reduce(dy, x, mean, invstd, w, b)
    f1 = invstd * w.double()
    f2 = red["sum_dy"] / n
    f3 = invstd * invstd * red["sum_dy_xmu"] / n
    ca, cb, cd = f1, -f1 * f3, f1 * (f3 * mean - f2)
    bwd_terms = ((o64.chan(ca, nd) * dyd).abs() + (o64.chan(cb, nd) * xd).abs()
                 + o64.chan(cd, nd).abs())
    _within("module dx", dx, dx64, 4 * 2.0 ** -23 * bwd_terms)

    _within("module db", db, db64, RED_K * red["abs_dy"] + U * db64.abs())
    # dw = invstd * sum dy*(x - mean): the kernel's mean / invstd carry the
    # statistic bounds into it
    _within("module dw", dw, dw64,
            invstd * (RED_K * red["abs_xmu"] + matol * red["sum_dy"].abs())
            + (rtol + 2 * U) * dw64.abs())
    _check_running("module", m.running_mean, m.running_var, rm0, rv0, mean,
                   var, n, MOMENTUM)
    torch.testing.assert_close(rm64, o64.running_update(
        rm0, rv0, mean, var, n, MOMENTUM)[0])


# =================================================================
# grid-stride loops of the elementwise kernels
# =================================================================
# (shape, dtype, channels_last, V)
GRID_CASES = [
    ((3, 37, 97, 99), F32, False, 1),       # 1.07M elements, S and C odd
    ((3, 37, 97, 99), F32, True, 1),
    ((1, 8, 4, 131076), F32, False, 4),     # just past 4096*256*V elements
    ((1, 8, 4, 262152), BF16, True, 8),
]
# (act, slope, with_res, want_res_grad)
ELEMT_COMBOS = [(False, 0.0, False, False), (True, 0.0, True, True),
                (True, 0.1, True, False)]


def _assert_grid(plan, V):
    assert plan["V"] == V, plan
    assert plan["grid"] == 4096 and plan["multi_trip"], plan
    assert plan["trips"] >= 2 and plan["packs"] > GRID_CAP_THREADS, plan
    if V > 1:
        assert plan["packs"] % GRID_CAP_THREADS != 0, plan


def _close(got, want, dtype):
    torch.testing.assert_close(got.double(), want, **_tol(dtype))


@gpu
@pytest.mark.parametrize("combo", ELEMT_COMBOS,
                         ids=["plain", "relu_res_dres", "leaky_res"])
@pytest.mark.parametrize(
    "shape,dtype,cl,V", GRID_CASES,
    ids=[f"{'x'.join(map(str, s))}-{str(d)[6:]}-{'nhwc' if c else 'nchw'}"
         for s, d, c, _ in GRID_CASES])
def test_grid_stride_elementwise(shape, dtype, cl, V, combo):
    act, slope, with_res, want_res = combo
    C = shape[1]
    n = 1
    for s in shape:
        n *= s
    n //= C
    x, dy, res = _ordinary(shape, dtype, cl, seed=sum(shape))
    r = res if with_res else None
    g = _gen(C + 11)
    mean = torch.randn(C, generator=g, device=DEV)
    invstd = torch.rsqrt(torch.rand(C, generator=g, device=DEV) + 0.5)
    sum_dy = torch.randn(C, generator=g, device=DEV) * n ** 0.5
    sum_dy_xmu = torch.randn(C, generator=g, device=DEV) * 2 * n ** 0.5
    count = torch.full((1,), float(n), device=DEV)
    w, b = _affine(C, C)
    if act:
        x = _cl(_nudge(x, r, mean, invstd, w, b), cl)

    # forward
    _assert_grid(ops.launch_plan("elemt", x, (r,)), V)
    y = ops.batch_norm_elemt_act(x, r, w, b, mean, invstd, act, None, slope)
    _close(y, o64.elemt(x, mean, invstd, w, b, r, act, slope), dtype)

    # backward
    _assert_grid(ops.launch_plan("bwd_elemt", x, (dy, r)), V)
    dx, dres = ops.batch_norm_backward_elemt_act(
        dy, x, r, mean, invstd, w, b, sum_dy, sum_dy_xmu, count, act,
        want_res, None, slope)
    want_dx, want_g = o64.backward_elemt(
        dy, x, mean, invstd, w, b, sum_dy, sum_dy_xmu, float(n), r, act,
        slope)
    _close(dx, want_dx, dtype)
    if want_res:
        _close(dres, want_g, dtype)

    # frozen backward: the statistics are fixed running stats
    rv = invstd.double().pow(-2).float()   # arbitrary positive variances
    coefs = ops.bn_frozen_coefs(mean, rv, EPS, w, b)
    if act:
        x = _cl(_nudge(x, r, mean, torch.rsqrt(rv.double() + EPS).float(),
                       w, b), cl)
    _assert_grid(ops.launch_plan("frozen_bwd_elemt", dy,
                                 (x, r) if act else (), coefs), V)
    fdx, fdres = ops.batch_norm_frozen_backward_elemt(
        dy, x if act else None, r if act else None, coefs, act, True,
        want_res, slope)
    want_fdx, want_fg = o64.frozen_backward(dy, x, r, mean, rv, EPS, w, b,
                                            act, slope)
    _close(fdx, want_fdx, dtype)
    if want_res:
        _close(fdres, want_fg, dtype)


# =================================================================
# misaligned views: the vector-width fallback
# =================================================================
# Data here is small integers (and power-of-two statistics), so every sum
# and every product the kernels form is exact in fp32 whatever the order or
# the vector width: equal bits between the aligned and the misaligned run
# is then a fair demand of the reductions too.
MIS_SHAPE = (4, 8, 4, 16)   # S = 64, C = 8, N*S = 256


def _ints(shape, g, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=g).float()


def _offset_view(t, k, channels_last):
    """A copy of t living k ELEMENTS past an aligned allocation."""
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=t.device)
    flat = buf[k:k + t.numel()]
    if channels_last:
        N, C, H, W = t.shape
        v = flat.view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        v = flat.view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + k * t.element_size()
    assert v.stride() == t.stride()
    return v


def _mis_inputs(dtype, cl):
    g = torch.Generator().manual_seed(99)
    C = MIS_SHAPE[1]
    t = {k: _cl(_ints(MIS_SHAPE, g).to(dtype).to(DEV), cl)
         for k in ("x", "dy", "res")}
    t["mean"] = _ints((C,), g, -2, 3).to(DEV)
    t["invstd"] = torch.tensor([0.5, 1.0, 2.0, 1.0, 0.5, 2.0, 1.0, 0.25],
                               device=DEV)
    t["w"] = torch.tensor([1.0, 2.0, 0.5, 1.0, 2.0, 1.0, 0.5, 1.0],
                          device=DEV)
    t["b"] = (_ints((C,), g, -3, 4) + 0.5).to(DEV)
    t["sum_dy"] = (_ints((C,), g) * 256).to(DEV)
    t["sum_dy_xmu"] = (_ints((C,), g) * 256).to(DEV)
    t["count"] = torch.full((1,), 256.0, device=DEV)
    t["coefs"] = ops.bn_make_coefs(t["mean"], t["invstd"], t["w"], t["b"])
    return t


def _run_all(t, gm_like):
    """Every op that takes caller tensors; returns all results + plans."""
    x, dy, res, coefs = t["x"], t["dy"], t["res"], t["coefs"]
    gm = gm_like(torch.empty_like(x))
    out, plans = {}, {}
    plans["stats"] = ops.launch_plan("stats", x)
    out["stats"] = ops.batch_norm_stats(x, EPS)
    plans["bwd_reduce"] = ops.launch_plan("bwd_reduce", x, (dy, res, gm))
    out["bwd_reduce"] = ops.batch_norm_backward_reduce_act(
        dy, x, res, t["mean"], t["invstd"], t["w"], t["b"], True, True, True,
        True, coefs, gm, 0.25)
    out["gm"] = (gm,)
    plans["elemt"] = ops.launch_plan("elemt", x, (res,), coefs)
    out["elemt"] = (ops.batch_norm_elemt_act(
        x, res, t["w"], t["b"], t["mean"], t["invstd"], True, coefs, 0.25),)
    plans["bwd_elemt"] = ops.launch_plan("bwd_elemt", x, (dy, res), coefs)
    out["bwd_elemt"] = ops.batch_norm_backward_elemt_act(
        dy, x, res, t["mean"], t["invstd"], t["w"], t["b"], t["sum_dy"],
        t["sum_dy_xmu"], t["count"], True, True, coefs, 0.25)
    plans["frozen"] = ops.launch_plan("frozen_bwd_elemt", dy, (x, res), coefs)
    out["frozen"] = ops.batch_norm_frozen_backward_elemt(
        dy, x, res, coefs, True, True, True, 0.25)
    return out, plans


# which plans must report the reduced V when this tensor is the offset one
MIS_AFFECTS = {
    "x": ("stats", "bwd_reduce", "elemt", "bwd_elemt", "frozen"),
    "dy": ("bwd_reduce", "bwd_elemt", "frozen"),
    "res": ("bwd_reduce", "elemt", "bwd_elemt", "frozen"),
    "gm_out": ("bwd_reduce",),
    # only the NHWC elementwise kernels load the coefficients as packs
    "coefs": ("elemt", "bwd_elemt", "frozen"),
}


@gpu
@pytest.mark.parametrize("which", list(MIS_AFFECTS))
@pytest.mark.parametrize("offset", ["one_element", "eight_bytes"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_misaligned_views(dtype, cl, offset, which):
    vmax = 16 // torch.empty((), dtype=dtype).element_size()
    esize = 4 if which == "coefs" else 16 // vmax
    k = 1 if offset == "one_element" else 8 // esize
    t = _mis_inputs(dtype, cl)
    base, base_plans = _run_all(t, lambda e: e)
    assert all(p["V"] == vmax for p in base_plans.values()), base_plans

    m = dict(t)
    gm_like = lambda e: e
    if which == "gm_out":
        gm_like = lambda e: _offset_view(e, k, cl)
    elif which == "coefs":
        m["coefs"] = _offset_view(t["coefs"], k, False)
    else:
        m[which] = _offset_view(t[which], k, cl)
    got, plans = _run_all(m, gm_like)

    if which == "coefs":
        # a pack of V floats needs V*4 bytes: any of these offsets -> V = 1
        want_v = 1 if cl else vmax
    else:
        want_v = 1 if offset == "one_element" else vmax // 2
    for name, p in plans.items():
        assert p["V"] == (want_v if name in MIS_AFFECTS[which] else vmax), \
            (name, p)
    for name in base:
        for a, bb in zip(base[name], got[name]):
            if a is None or not isinstance(a, torch.Tensor) or \
                    a.numel() == 0:
                continue
            assert torch.equal(a, bb), (name, which)
