"""Multi-rank SyncBatchNorm against the float64 oracle of the WHOLE batch.

The kernels are held to ``oracle64`` one by one elsewhere; this file holds
the composition that makes them a synchronized BatchNorm — the Python of
``msbn/nn/functions.py`` and ``msbn/nn/fused.py`` that runs when
``world_size > 1`` — to the same oracle, with ranks that differ in count,
mean and variance, so that a local count, an un-reduced sum, equal rank
weights or a variance merge without its between-rank term cannot pass.

Every rank builds the same global batch (CPU generator, one seed per case),
takes its slice, runs the module, and compares its slice of the oracle of
the whole batch.  Rank r's samples are ``randn*(1+r) + 3r``; batch sizes are
unequal and one rank of the 4-rank world is empty.  The GPU tier (2 and 4
ranks on cuda:0) also records the arguments of the backward reduce op and of
the forward elemt op, so that each case is known to run the branch it is
there for; the CPU tier (2, 3, 4 ranks) runs the same checks on the reference
ops and validates harness, oracle wiring and bounds without a GPU.

Bounds (u = 2^-24; all from test_gpu_reduction_edges.py):

* mean / invstd / coefs / running statistics: ``_check_*`` with the global
  count; ``count_sum`` is exact.
* y, fp32: 4*2^-23 * (|x*scale| + |shift| [+ |res|]); bf16: ``_tol(bf16)``.
* dres: bit-equal to the oracle's gated gradient rounded to the input dtype
  (a fork's incoming gradient is dy1 + dy2 rounded once to that dtype).
* dx, fp32: 4*2^-23 * (|a*g| + |b*x| + |d|) plus the propagated error of the
  two global sums, f1*(RED_K*ABS_DY/n + |x-mean|*invstd^2*RED_K*ABS_XMU/n);
  bf16: ``_tol(bf16)``.
* grad_weight / grad_bias are this rank's contribution (the DDP reducer sums
  them): RED_K*abs_dy, and RED_K*abs_xmu*invstd + (rtol+2u)*|dw|
  + invstd*matol*|sum_dy|, of the rank's slice with the global statistics.
"""

import inspect
import re

import pytest
import torch
import torch.distributed as dist

import msbn
import multirank_harness as harness
import oracle64 as o64
from msbn import ops
from msbn.nn.fused import SyncBatchNormAct2d
from test_gpu_reduction_edges import (EPS, RED_K, U, _check_coefs,
                                      _check_running, _check_stats, _nudge,
                                      _stat_bounds, _tol, _within)

gpu = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
C = 24                       # < 64: the small-plane kernels stay out
MOMENTUM = 0.1
SIZES = {2: (1, 3), 3: (3, 1, 0), 4: (2, 0, 1, 5)}
# S = 35: vector width 1.  S = 48: vectorised.
PLANES = [(5, 7), (6, 8)]
# (dtype, channels_last)
TIERS = [(F32, False), (BF16, True)]

# name -> (fused, act, slope, residual, fork, affine, want gm_out,
#          want grad_out2); the last two are what the GPU path must hand to
# the backward reduce op
CONFIGS = {
    "a": (False, False, 0.0, False, False, True, False, False),
    "b": (True, True, 0.0, False, False, True, False, False),
    "c": (True, True, 0.0, True, False, True, True, False),
    "d": (True, True, 0.25, True, True, True, True, True),
    "e": (True, True, 0.0, False, True, True, True, True),
    "f": (True, True, 0.25, False, True, True, False, False),
    "g": (True, True, 0.0, True, False, False, True, False),
}
CASES = [(name, plane, ti) for name in CONFIGS for plane in PLANES
         for ti in range(len(TIERS))]


def _cl(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) \
        if channels_last else t.contiguous()


def _seed(case):
    name, plane, ti = case
    return 1000 * (ord(name) - ord("a")) + 10 * plane[0] + ti


# ------------------------------------------------------------------- data
def _global_batch(case, sizes):
    """The whole batch on the CPU, identical on every rank: x, res, dy1, dy2
    (rounded to the case dtype), w, b, rm0, rv0 (fp32).  For activation
    cases x is nudged until no pre-activation of the WHOLE batch lies inside
    the gate's ambiguity band; the statistics depend on x, so iterate."""
    name, (H, W_), ti = case
    fused, act, slope, with_res, fork, affine, _, _ = CONFIGS[name]
    dtype, _ = TIERS[ti]
    g = torch.Generator().manual_seed(_seed(case))
    N = sum(sizes)
    x = torch.cat([torch.randn(n, C, H, W_, generator=g) * (1 + r) + 3 * r
                   for r, n in enumerate(sizes)]).to(dtype)
    d = {"res": None, "dy2": None, "w": None, "b": None}
    if with_res:
        d["res"] = torch.randn(N, C, H, W_, generator=g).to(dtype)
    d["dy1"] = torch.randn(N, C, H, W_, generator=g).to(dtype)
    if fork:
        d["dy2"] = torch.randn(N, C, H, W_, generator=g).to(dtype)
    if affine:
        # invstd is about 1/4 .. 1/2 here; weights of several units keep dx
        # of order one, where the bf16 tier's atol of 2e-2 is not most of
        # its bound (test_wrong_compositions_violate_the_bounds)
        d["w"] = 8 * (torch.randn(C, generator=g).abs() + 0.1)
        # The y bound counts shift = b - mean*scale as ONE fp32 term.  The
        # mean is an fp32 number, so shift carries u*|mean*scale| whatever
        # forms it, which |shift| covers only where the two do not cancel:
        # every channel's global mean is positive here (asserted below), so
        # the bias is drawn negative.  test_gpu_reduction_edges._check_coefs
        # is where a cancelling shift is held to its own bound.
        d["b"] = -torch.randn(C, generator=g).abs()
    d["rm0"] = torch.randn(C, generator=g)
    d["rv0"] = torch.rand(C, generator=g) + 0.5
    if act:
        for _ in range(16):
            mean, _, invstd = o64.stats(x, EPS)
            moved = _nudge(x, d["res"], mean, invstd, d["w"], d["b"], True)
            if moved is x:
                break
            x = moved
        else:
            raise AssertionError(
                "could not separate the pre-activations from zero")
    assert (o64.stats(x, EPS)[0] > 0.25).all().item(), \
        "a channel's global mean is not clearly positive"
    d["x"] = x
    return d


def _incoming(dy1, dy2):
    """The gradient that reaches the layer: a fork's two, summed in the input
    dtype (one rounding), as autograd or the reduce kernel does."""
    return dy1 if dy2 is None else dy1 + dy2


# ----------------------------------------------------------------- bounds
def _elementwise_bound(dtype, want):
    t = _tol(dtype)
    return t["atol"] + t["rtol"] * want.abs()


def _y_bound(dtype, x, res, mean, invstd, w, b, want):
    if dtype != F32:
        return _elementwise_bound(dtype, want)
    nd = x.dim()
    scale, shift = o64.coefs(mean, invstd, w, b)
    terms = (x.double() * o64.chan(scale, nd)).abs() \
        + o64.chan(shift, nd).abs().expand_as(x)
    if res is not None:
        terms = terms + res.double().abs()
    return 4 * 2.0 ** -23 * terms


def _dx_bound(dtype, x, g, mean, invstd, w, red, n, want):
    """``red`` is the oracle's backward_reduce of the whole batch, ``g`` the
    gated gradient of the slice ``x``."""
    if dtype != F32:
        return _elementwise_bound(dtype, want)
    nd = x.dim()
    xd = x.double()
    f1 = invstd if w is None else invstd * w.double()
    f2 = red["sum_dy"] / n
    f3 = invstd * invstd * red["sum_dy_xmu"] / n
    ca, cb, cd = f1, -f1 * f3, f1 * (f3 * mean - f2)
    terms = ((o64.chan(ca, nd) * g).abs() + (o64.chan(cb, nd) * xd).abs()
             + o64.chan(cd, nd).abs())
    xmu = (xd - o64.chan(mean, nd)).abs()
    red_err = o64.chan(f1.abs(), nd) * (
        o64.chan(RED_K * red["abs_dy"] / n, nd)
        + xmu * o64.chan(invstd * invstd * RED_K * red["abs_xmu"] / n, nd))
    return 4 * 2.0 ** -23 * terms + red_err


def _dw_bound(loc, invstd, rtol, matol):
    return (RED_K * loc["abs_xmu"] * invstd
            + (rtol + 2 * U) * loc["grad_weight"].abs()
            + invstd * matol * loc["sum_dy"].abs())


# ------------------------------------------------------------ the worker
class _Recorder:
    """Wraps ops.<name> while a case runs and keeps each call's arguments by
    parameter name."""

    def __init__(self, *names):
        self.names = names
        self.calls = {n: [] for n in names}
        self._real = {}

    def __enter__(self):
        for n in self.names:
            real = getattr(ops, n)
            sig = inspect.signature(real)

            def wrapped(*a, _real=real, _sig=sig, _n=n, **kw):
                bound = _sig.bind(*a, **kw)
                bound.apply_defaults()
                self.calls[_n].append(dict(bound.arguments))
                return _real(*a, **kw)

            self._real[n] = real
            setattr(ops, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, real in self._real.items():
            setattr(ops, n, real)


def _checked(failures, fn, *args):
    try:
        fn(*args)
    except AssertionError as e:
        failures.append(str(e))


def run_case(rank, world, device, case):
    """One case on one rank: run (every collective), then check.  Returns
    the failures; raises only if the run itself broke."""
    name, plane, ti = case
    fused, act, slope, with_res, fork, affine, want_gm, want_dy2 = \
        CONFIGS[name]
    dtype, cl = TIERS[ti]
    sizes = SIZES[world]
    on_gpu = device != "cpu"
    d = _global_batch(case, sizes)
    off, n_loc = sum(sizes[:rank]), sizes[rank]
    n = sum(sizes) * plane[0] * plane[1]
    tag = f"[{name} W{world} r{rank}]"

    def dev(t):
        return None if t is None else t.to(device)

    def loc(t, grad=False):
        if t is None:
            return None
        t = _cl(t[off:off + n_loc].to(device), cl)
        return t.requires_grad_(True) if grad else t

    # ------------------------------------------------------------ run
    if fused:
        m = SyncBatchNormAct2d(C, EPS, MOMENTUM, affine, relu=act,
                               negative_slope=slope)
    else:
        m = msbn.nn.SyncBatchNorm(C, EPS, MOMENTUM, affine)
    m = m.to(device).train()
    with torch.no_grad():
        if affine:
            m.weight.copy_(d["w"])
            m.bias.copy_(d["b"])
        m.running_mean.copy_(d["rm0"])
        m.running_var.copy_(d["rv0"])
    x = loc(d["x"], grad=True)
    res = loc(d["res"], grad=True)
    dy1, dy2 = loc(d["dy1"]), loc(d["dy2"])

    with _Recorder("batch_norm_elemt_act", "batch_norm_backward_reduce",
                   "batch_norm_backward_reduce_act") as rec:
        if not fused:
            out = (m(x),)
        elif fork:
            out = m(x, res, fork=True)
        else:
            out = (m(x, res),)
        node = out[0].grad_fn
        saved = node.saved_tensors
        if fused:
            mean, invstd, count_sum = saved[4:7]
            coefs = saved[7] if node.has_coefs else None
        else:
            mean, invstd, count_sum = saved[2:5]
            fwd = rec.calls["batch_norm_elemt_act"]
            coefs = fwd[0]["coefs"] if fwd else None
        loss = (out[0] * dy1).sum()
        if fork:
            loss = loss + (out[1] * dy2).sum()
        wanted = [x] + ([res] if with_res else []) \
            + ([m.weight, m.bias] if affine else [])
        grads = list(torch.autograd.grad(loss, wanted, allow_unused=True))
    dx = grads.pop(0)
    dres = grads.pop(0) if with_res else None
    dw, db = grads if affine else (None, None)

    running = torch.cat([m.running_mean, m.running_var]).detach().clone()
    everyone = [torch.empty_like(running) for _ in range(world)]
    dist.all_gather(everyone, running)
    if on_gpu:
        torch.cuda.synchronize()

    # ---------------------------------------------------------- check
    failures = []
    ck = lambda fn, *a: _checked(failures, fn, *a)   # noqa: E731

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {what}")

    # which branch ran
    fwd = rec.calls["batch_norm_elemt_act"]
    red = rec.calls["batch_norm_backward_reduce"]
    red_act = rec.calls["batch_norm_backward_reduce_act"]
    if n_loc == 0:
        expect(not fwd and not red and not red_act,
               "the empty rank launched an elementwise or reduce op")
    else:
        expect(len(fwd) == 1, f"{len(fwd)} forward elemt calls")
        expect(all((c["coefs"] is not None) == on_gpu for c in fwd),
               "coefs reach the forward elemt op on the GPU only")
        if fused:
            expect(len(red_act) == 1 and not red,
                   f"reduce calls: {len(red)} plain, {len(red_act)} act")
            for c in red_act:
                expect((c["gm_out"] is not None) == (want_gm and on_gpu),
                       f"gm_out passed: {c['gm_out'] is not None}")
                expect((c["grad_out2"] is not None) == (want_dy2 and on_gpu),
                       f"grad_out2 passed: {c['grad_out2'] is not None}")
                expect((c["coefs"] is not None) == on_gpu,
                       "coefs reach the reduce op on the GPU only")
                if with_res and on_gpu and c["gm_out"] is not None:
                    expect(dres is not None
                           and dres.data_ptr() == c["gm_out"].data_ptr(),
                           "dres is not the gm the reduce pass wrote")
        else:
            expect(len(red) == 1 and not red_act,
                   f"reduce calls: {len(red)} plain, {len(red_act)} act")
    if fused:
        expect(node.has_coefs == on_gpu, f"has_coefs {node.has_coefs}")
    expect((coefs is not None) == (on_gpu and (fused or n_loc > 0)),
           f"saved coefs present: {coefs is not None}")

    # statistics of the whole batch
    X = dev(d["x"])
    w, b = dev(d["w"]), dev(d["b"])
    RES = dev(d["res"])
    mean64, var64, invstd64 = o64.stats(X, EPS)
    expect(count_sum.numel() == 1 and count_sum.item() == float(n),
           f"count_sum {count_sum.tolist()} != {n}")
    ck(_check_stats, tag, mean, invstd, mean64, var64)
    if coefs is not None:
        ck(_check_coefs, tag, coefs, mean64, var64,
           w if affine else torch.ones(C, device=device),
           b if affine else torch.zeros(C, device=device))
    ck(_check_running, tag, m.running_mean, m.running_var, dev(d["rm0"]),
       dev(d["rv0"]), mean64, var64, n, MOMENTUM)
    expect(all(torch.equal(e, running) for e in everyone),
           "running statistics differ between ranks")
    expect(m.num_batches_tracked.item() == 1,
           f"num_batches_tracked {m.num_batches_tracked.item()}")

    # the oracle of the whole batch, compared on this rank's slice
    DY = _incoming(dev(d["dy1"]), dev(d["dy2"]))
    RED = o64.backward_reduce(DY, X, mean64, invstd64, w, b, RES, act, slope)
    sl = slice(off, off + n_loc)
    xs, dys = X[sl], DY[sl]
    rs = None if RES is None else RES[sl]
    rtol, matol = _stat_bounds(mean64, var64)

    for i, y in enumerate(out):
        expect(y.shape == xs.shape and y.dtype == dtype,
               f"y{i}: {tuple(y.shape)} {y.dtype}")
    expect(dx is not None and dx.shape == xs.shape and dx.dtype == dtype,
           "dx: wrong shape or dtype")
    if n_loc > 0:
        want_y = o64.elemt(xs, mean64, invstd64, w, b, rs, act, slope)
        y_bound = _y_bound(dtype, xs, rs, mean64, invstd64, w, b, want_y)
        for i, y in enumerate(out):
            ck(_within, f"{tag} y{i}", y.detach(), want_y, y_bound)
        want_dx, want_g = o64.backward_elemt(
            dys, xs, mean64, invstd64, w, b, RED["sum_dy"],
            RED["sum_dy_xmu"], float(n), rs, act, slope)
        ck(_within, f"{tag} dx", dx, want_dx,
           _dx_bound(dtype, xs, want_g, mean64, invstd64, w, RED, float(n),
                     want_dx))
        if with_res:
            expect(dres is not None and torch.equal(dres, want_g.to(dtype)),
                   "dres is not the gated gradient, bit for bit")
        if affine:
            LOC = o64.backward_reduce(dys, xs, mean64, invstd64, w, b, rs,
                                      act, slope)
            ck(_within, f"{tag} grad_bias", db, LOC["grad_bias"],
               RED_K * LOC["abs_dy"])
            ck(_within, f"{tag} grad_weight", dw, LOC["grad_weight"],
               _dw_bound(LOC, invstd64, rtol, matol))
    else:
        if with_res:
            expect(dres is not None and dres.shape == xs.shape,
                   "empty rank: dres")
        if affine and fused:    # the fused function returns zeros ...
            expect(dw is not None and not dw.any().item()
                   and db is not None and not db.any().item(),
                   "empty rank: fused grad_weight / grad_bias are not zeros")
        elif affine:            # ... the plain one nothing
            expect(dw is None and db is None,
                   "empty rank: plain grad_weight / grad_bias are not None")
    return failures


# --------------------------------------------------------------- the tests
_RATIO = re.compile(r"^\[(\w) W\d r\d\] (.+?): .*max err/bound (\S+)$")


def _report(world, device, outputs):
    """Worst err/bound that ``_within`` printed, per configuration and per
    quantity, over ranks, shapes and dtypes."""
    worst = {}
    for rank, per_case in outputs.items():
        for _, text in per_case:
            for line in text.splitlines():
                mt = _RATIO.match(line)
                if mt:
                    key = (mt.group(1), mt.group(2))
                    worst[key] = max(worst.get(key, 0.0), float(mt.group(3)))
    for name in CONFIGS:
        row = ", ".join(f"{q} {v:.2f}" for (c, q), v in sorted(worst.items())
                        if c == name)
        print(f"worst err/bound, W={world} {device}, case {name}: {row}")
    return worst


def _run(tmp_path, world, device):
    outputs = harness.run_cases(tmp_path, world, device,
                                "test_sync_oracle:run_case", CASES)
    assert sorted(outputs) == list(range(world))
    worst = _report(world, device, outputs)
    # every configuration was measured on y, dx and the statistics
    for name in CONFIGS:
        for q in ("y0", "dx", "mean", "invstd", "running_var"):
            assert (name, q) in worst, (name, q)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sync_oracle_cpu(world, tmp_path):
    _run(tmp_path, world, "cpu")


@gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sync_oracle_gpu(world, tmp_path):
    _run(tmp_path, world, "cuda:0")


def test_harness_reports_every_failure_and_times_out(tmp_path):
    """Failures of all cases and ranks arrive together; a deadline that has
    run out (here: at once, nothing is waited for) ends in the word
    "timeout" with the workers terminated, not in a hang."""
    with pytest.raises(AssertionError) as e:
        harness.run_cases(tmp_path, 2, "cpu", "test_sync_oracle:_failing_case",
                          ["p", "q"])
    msg = str(e.value)
    for rank in (0, 1):
        for c in ("p", "q"):
            assert f"rank {rank}, case '{c}':\nbad {c}" in msg, msg
    with pytest.raises(AssertionError, match="timeout"):
        harness.run_cases(tmp_path, 2, "cpu",
                          "test_sync_oracle:_failing_case", ["p"],
                          deadline_s=0.0)


def _failing_case(rank, world, device, case):
    t = torch.ones(1)
    dist.all_reduce(t)
    return [f"bad {case}"] if t.item() == world else ["all_reduce is broken"]


# ------------------------------------------------- can the data tell?
def test_wrong_compositions_violate_the_bounds():
    """Oracle only, CPU, the 4-rank batch sizes, both dtypes: five wrong ways
    to compose the synchronized statistics and gradients each miss the bound
    above by at least 10x on some non-empty rank.  If one did not, the data
    or the bounds would be too weak to notice that mistake.  The first four
    are tried on the plain configuration (a), the fork's on (d)."""
    sizes = SIZES[4]
    for ti, (dtype, _) in enumerate(TIERS):
        for name in ("a", "d"):
            case = (name, PLANES[0], ti)
            _, act, slope, with_res, fork, _, _, _ = CONFIGS[name]
            d = _global_batch(case, sizes)
            X, RES, w, b = d["x"], d["res"], d["w"], d["b"]
            n = float(X.numel() // C)
            mean, var, invstd = o64.stats(X, EPS)
            rtol, matol = _stat_bounds(mean, var)
            DY = _incoming(d["dy1"], d["dy2"])
            RED = o64.backward_reduce(DY, X, mean, invstd, w, b, RES, act,
                                      slope)
            offs = [sum(sizes[:r]) for r in range(len(sizes))]
            ranks = [(slice(o, o + k), k) for o, k in zip(offs, sizes) if k]

            def worst_dx(wrong):
                """max err/bound of wrong(slice, n_r) -> dx over the ranks"""
                worst = 0.0
                for sl, k in ranks:
                    rs = None if RES is None else RES[sl]
                    want, g = o64.backward_elemt(
                        DY[sl], X[sl], mean, invstd, w, b, RED["sum_dy"],
                        RED["sum_dy_xmu"], n, rs, act, slope)
                    bound = _dx_bound(dtype, X[sl], g, mean, invstd, w, RED,
                                      n, want)
                    got = wrong(sl, k)
                    worst = max(worst, ((got - want).abs() / bound).max()
                                .item())
                return worst

            def elemt_with(dy, sum_dy, sum_dy_xmu, count):
                def f(sl, k):
                    rs = None if RES is None else RES[sl]
                    s1 = sum_dy(sl) if callable(sum_dy) else sum_dy
                    s2 = sum_dy_xmu(sl) if callable(sum_dy_xmu) \
                        else sum_dy_xmu
                    cnt = count(sl) if callable(count) else count
                    return o64.backward_elemt(
                        dy[sl], X[sl], mean, invstd, w, b, s1, s2, cnt, rs,
                        act, slope)[0]
                return f

            def local(key):
                def f(sl):
                    rs = None if RES is None else RES[sl]
                    return o64.backward_reduce(DY[sl], X[sl], mean, invstd,
                                               w, b, rs, act, slope)[key]
                return f

            plane = float(PLANES[0][0] * PLANES[0][1])
            tagd = f"{name} {dtype}"
            if fork:
                # 5. one of a fork's two gradients alone
                r5 = worst_dx(elemt_with(d["dy1"], RED["sum_dy"],
                                         RED["sum_dy_xmu"], n))
                print(f"{tagd}: dy1 alone {r5:.3g}")
                assert r5 >= 10, (tagd, r5)
                continue
            # 1. the local count instead of the global one
            r1 = worst_dx(elemt_with(
                DY, RED["sum_dy"], RED["sum_dy_xmu"],
                lambda sl: (sl.stop - sl.start) * plane))
            # 2. rank-local sums: the all-reduce left out
            r2 = worst_dx(elemt_with(DY, local("sum_dy"),
                                     local("sum_dy_xmu"), n))
            print(f"{tagd}: local count {r1:.3g}, local sums {r2:.3g}")
            assert r1 >= 10 and r2 >= 10, (tagd, r1, r2)

            # 3. / 4. the statistics' merge
            per = [o64.stats(X[sl], EPS) for sl, _ in ranks]
            counts = [k * plane for _, k in ranks]
            good_mean, good_var, _ = o64.gather(
                [p[0] for p in per], [p[1] for p in per], counts, EPS)
            _check_stats(tagd + " merge", good_mean, torch.rsqrt(
                good_var + EPS), mean, var)
            flat_mean = sum(p[0] for p in per) / len(per)
            within_var = sum(c * p[1] for p, c in zip(per, counts)) / n
            r3 = ((flat_mean - mean).abs() / matol).max().item()
            r4 = ((torch.rsqrt(within_var + EPS) - invstd).abs()
                  / (rtol * invstd)).max().item()
            print(f"{tagd}: unweighted mean {r3:.3g}, no between-rank "
                  f"term {r4:.3g}")
            assert r3 >= 10 and r4 >= 10, (tagd, r3, r4)
