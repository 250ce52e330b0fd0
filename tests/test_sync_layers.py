"""The layers added since test_sync_oracle.py, at ``world_size > 1``.

Grouped BN, the stem pool, dual BN, the SiLU epilogue and the conv-fed
BatchNorms each have a ``use_sync`` branch of their own in
``msbn/nn/fused.py``.  At world size 1 every collective is the identity, so a
dropped all_reduce, a count or mean taken from the wrong rank or segment, or
a local count where the global one belongs pass every single-process test.
Here W ranks that differ in batch size (one of four is empty), mean and
variance run one process group (``multirank_harness``), as in
test_sync_oracle.py: rank r's samples are ``randn*(1+r) + 3r``, the whole
batch is built on every rank from one CPU generator, each rank takes its
slice and compares its slice of the reference of the WHOLE batch.

1. Grouped BN (``bn_act_grouped``): ``oracle64`` per segment over the
   concatenation of that segment across ranks, with the bounds of
   test_sync_oracle.py (fp32: ``_y_bound`` / ``_dx_bound``; bf16: ``_tol``),
   ``_check_stats`` / ``_check_coefs`` with the global statistics, and the
   running statistics after S updates under the summed single-update bounds
   (``test_gpu_grouped_bn._running_chain``).  The rank-local affine gradients
   are the sum over the segments of each segment's contribution, held to the
   sum of the per-segment bounds.  A group may hold a segment that is empty
   on one rank only ("ragged"): the plan gives it no chunk and no block,
   ``find_segment`` steps over it and the finalize stages emit zeros for it.
2. Stem pool and dual BN: bit-equal to their composition run in the same
   group right after, on clones of the inputs and twin modules.  The
   composition's pieces are held to the oracle by test_sync_oracle.py.
3. SiLU and the conv-fed layers: float64 autograd of the whole batch, the
   tolerances of ``silu_ref`` and of test_gpu_conv_stats.py.  The affine and
   conv-weight gradients are rank-local (the DDP reducer sums them); their
   reference is formed from the whole-batch reference's gradient at the
   BatchNorm's output / at the convolution's output, over the rank's slice.
4. Depthwise 5x5 (``dw5``) and squeeze-excite (``se``, alone and behind the
   3x3 and 5x5 depthwise kernels): as 3., ``_tol(dtype)`` throughout.  SE's
   BatchNorm backward sums are factorised through per-image tables and then
   all_reduced, so dx, the rank-local affine and conv-weight gradients and
   the block's own parameter gradients (float64 autograd of the block alone
   on the rank's slice of the activated tensor) are each held on every
   non-empty rank, the running statistics on all.  The empty rank runs the
   composition beside peers on the fused Function: every rank's collectives
   (op, numel, dtype, in order) are recorded and compared across the group.
5. On the CPU: wrong compositions of the grouped statistics and gradients
   miss the bounds of 1. by 10x or more, the comparison of 2. reports a
   dropped all_reduce (two gloo ranks on the reference ops), the rank-local
   references of 4. add up to the whole-batch gradients, and the SE Function
   on gloo ranks passes the checker of 4. and reports dx on every non-empty
   rank once all_reduce is dropped.
"""

import contextlib
import functools
import re

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

import multirank_harness as harness
import oracle64 as o64
import silu_ref
import test_dual_bn as dual_cpu
import test_gpu_conv_stats as cs
import test_gpu_dwconv_stats as dws
import test_gpu_grouped_bn as gbn
import test_sync_oracle as so
from msbn import ops
from msbn.nn import SqueezeExcite, SyncBatchNorm
from msbn.nn.batchnorm import _momentum_factor
from msbn.nn.fused import (SyncBatchNormAct2d, SyncBatchNormActPoolFunction,
                           SyncBatchNormSiluSEFunction, bn_act_grouped,
                           bn_act_maxpool, bn_add_bn_act, bn_silu_se,
                           conv1x1_bn_act, dwconv3x3_bn_act,
                           dwconv5x5_bn_act)
from test_gpu_reduction_edges import (EPS, RED_K, _check_coefs,
                                      _check_running, _check_stats, _nudge,
                                      _stat_bounds, _tol, _within)

gpu = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
MOM = 0.1
SIZES = so.SIZES
CL = torch.channels_last


def _cl(t):
    return t.contiguous(memory_format=CL)


def _rank_batch(shape_of, world, g):
    """cat over the ranks of ``randn(shape_of(r)) * (1 + r) + 3r``."""
    return torch.cat([torch.randn(shape_of(r), generator=g) * (1 + r) + 3 * r
                      for r in range(world)])


def _one_thread(fn):
    """Run ``fn`` with one intra-op thread.  The float64 convolution
    references are tiny, and W ranks that each wake a whole thread pool for
    them on shared cores wait seconds per case for one another."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*a, **kw)
        finally:
            torch.set_num_threads(n)
    return wrapped


def _close(name, got, want, kw):
    """assert_close's inequality through ``_within``, which prints the
    worst err/bound first."""
    want = want.double()
    _within(name, got.detach().double().cpu(), want.cpu(),
            kw["atol"] + kw["rtol"] * want.cpu().abs())


@contextlib.contextmanager
def _all_reduce_dropped(on):
    """``dist.all_reduce`` leaves its argument untouched (every rank alike,
    so the ranks stay in step)."""
    if not on:
        yield
        return
    real = dist.all_reduce
    dist.all_reduce = lambda tensor, *a, **kw: None
    try:
        yield
    finally:
        dist.all_reduce = real


# =================================================================== grouped
PYRAMID = [(5, 7), (3, 4), (1, 2)]
EIGHT = [(2, 3), (1, 2), (2, 2), (1, 1), (1, 3), (3, 1), (1, 5), (2, 1)]
# n[rank][segment]; every segment's global count is at least 2
RAGGED = {2: [(1, 0, 2), (3, 2, 0)],
          4: [(1, 0, 2), (3, 2, 0), (0, 0, 0), (2, 1, 1)]}
# name -> (C, planes, module): "fold" a SyncBatchNorm with the ReLU after it
# folded in, "act" a SyncBatchNormAct2d, "plain" a SyncBatchNorm alone
GROUPS = {
    "pyramid_fold": (16, PYRAMID, "fold"),
    "pyramid_act": (16, PYRAMID, "act"),
    # 72 channels: two channel tiles (fp32: three); the gather kernel's full
    # s loop and running-statistics chain
    "eight": (72, EIGHT, "plain"),
    "ragged": (16, PYRAMID, "act"),
    "layout": (16, PYRAMID, "fold"),
}
GROUPED_OPS = ("batch_norm_stats_packed_grouped",
               "batch_norm_gather_stats_packed_grouped",
               "batch_norm_elemt_act_grouped",
               "batch_norm_backward_reduce_act_grouped",
               "batch_norm_backward_elemt_act_grouped")


def _counts(name, world):
    if name == "ragged":
        return RAGGED[world]
    return [(n,) * len(GROUPS[name][1]) for n in SIZES[world]]


def _grouped_batch(name, world, ti):
    """The whole group on the CPU, identical on every rank: per segment
    (x, dy) rounded to the dtype, and fp32 w, b, rm0, rv0.  With a ReLU x is
    nudged as in test_sync_oracle._global_batch.  ``_y_bound`` counts
    shift = b - mean*scale as one fp32 term, which covers the rounding of
    mean*scale only where the two do not cancel: the bias is negative, so
    they cannot where the mean is positive; a segment that only the rank
    centred on zero holds (ragged) can have either sign, and the draw is
    repeated with the next seed until |shift| >= (|mean*scale| + |b|) / 4."""
    C, planes, kind = GROUPS[name]
    dtype, relu = DTYPES[ti], kind != "plain"
    counts = _counts(name, world)
    base = 100 * sorted(GROUPS).index(name) + 10 * world + ti
    for attempt in range(64):
        g = torch.Generator().manual_seed(base + 7919 * attempt)
        w = 8 * (torch.randn(C, generator=g).abs() + 0.1)
        b = -torch.randn(C, generator=g).abs()
        rm0 = torch.randn(C, generator=g)
        rv0 = torch.rand(C, generator=g) + 0.5
        segs, safe = [], True
        for s, (H, W_) in enumerate(planes):
            x = _rank_batch(lambda r: (counts[r][s], C, H, W_), world,
                            g).to(dtype)
            dy = torch.randn(x.shape, generator=g).to(dtype)
            for _ in range(16 if relu else 0):
                mean, _, invstd = o64.stats(x, EPS)
                moved = _nudge(x, None, mean, invstd, w, b, True)
                if moved is x:
                    break
                x = moved
            else:
                assert not relu, \
                    "could not separate the pre-activations from zero"
            mean, _, invstd = o64.stats(x, EPS)
            scale, shift = o64.coefs(mean, invstd, w, b)
            safe = safe and (shift.abs() >= 0.25 * (
                (mean * scale).abs() + b.double().abs())).all().item()
            segs.append((x, dy))
        if safe:
            return {"w": w, "b": b, "rm0": rm0, "rv0": rv0, "segs": segs}
    raise AssertionError("no draw without a cancelling shift")


def _grouped_oracle(d, relu):
    """Per segment the float64 statistics and backward sums of the whole
    batch: (mean, var, invstd, n, RED)."""
    out = []
    for X, DY in d["segs"]:
        mean, var, invstd = o64.stats(X, EPS)
        red = o64.backward_reduce(DY, X, mean, invstd, d["w"], d["b"], None,
                                  relu)
        out.append((mean, var, invstd, float(X.numel() // X.shape[1]), red))
    return out


def _segment_wants(dtype, X, DY, orc, sl, w, b, relu):
    """What rank-slice ``sl`` of a segment must see, with the bounds:
    (y, y_bound, dx, dx_bound, LOC, grad_weight bound, grad_bias bound)."""
    mean, var, invstd, n, red = orc
    xs, dys = X[sl], DY[sl]
    want_y = o64.elemt(xs, mean, invstd, w, b, None, relu)
    y_bound = so._y_bound(dtype, xs, None, mean, invstd, w, b, want_y)
    want_dx, g = o64.backward_elemt(dys, xs, mean, invstd, w, b,
                                    red["sum_dy"], red["sum_dy_xmu"], n, None,
                                    relu)
    dx_bound = so._dx_bound(dtype, xs, g, mean, invstd, w, red, n, want_dx)
    loc = o64.backward_reduce(dys, xs, mean, invstd, w, b, None, relu)
    rtol, matol = _stat_bounds(mean, var)
    return (want_y, y_bound, want_dx, dx_bound, loc,
            so._dw_bound(loc, invstd, rtol, matol), RED_K * loc["abs_dy"])


def _dense_aligned(t):
    return t.numel() == 0 or (t.is_contiguous(memory_format=CL)
                              and t.data_ptr() % 16 == 0)


def _run_grouped(rank, world, device, case):
    _, name, ti = case
    C, planes, kind = GROUPS[name]
    dtype, relu, S = DTYPES[ti], kind != "plain", len(planes)
    counts = _counts(name, world)
    d = _grouped_batch(name, world, ti)
    tag = f"[grouped W{world} r{rank}]"
    offs = [sum(counts[r][s] for r in range(rank)) for s in range(S)]
    sls = [slice(offs[s], offs[s] + counts[rank][s]) for s in range(S)]
    all_empty = not any(counts[rank])

    # ------------------------------------------------------------ run
    bn = (SyncBatchNormAct2d(C, EPS, MOM) if kind == "act"
          else SyncBatchNorm(C, EPS, MOM)).to(device).train()
    with torch.no_grad():
        bn.weight.copy_(d["w"])
        bn.bias.copy_(d["b"])
        bn.running_mean.copy_(d["rm0"])
        bn.running_var.copy_(d["rv0"])
    xs = [_cl(X[sl].to(device)) for (X, _), sl in zip(d["segs"], sls)]
    dys = [_cl(DY[sl].to(device)) for (_, DY), sl in zip(d["segs"], sls)]
    odd = name == "layout" and rank == 0
    if odd:
        # one tensor NCHW, one off the 16-byte boundary by one element
        xs[0] = xs[0].contiguous()
        n1, (h1, w1) = counts[0][1], planes[1]
        buf = torch.empty(xs[1].numel() + 1, dtype=dtype, device=device)
        v = buf[1:].view(n1, h1, w1, C).permute(0, 3, 1, 2)
        xs[1] = v.copy_(xs[1])
    for x in xs:
        x.requires_grad_(True)
    odd_plan = ops.launch_plan("stats_grouped", xs[0], xs[1:])["path"] \
        if odd else None

    with so._Recorder(*GROUPED_OPS) as rec:
        ys = bn_act_grouped(bn, xs, relu=True if kind == "fold" else None)
        node = ys[0].grad_fn
        node_name = type(node).__name__
        mean, invstd, count, coefs = node.saved_tensors[2:6]
        loss = sum((y * dy).sum() for y, dy in zip(ys, dys))
        grads = torch.autograd.grad(loss, xs + [bn.weight, bn.bias],
                                    allow_unused=True)
    dxs, (dw, db) = grads[:S], grads[S:]
    running = torch.cat([bn.running_mean, bn.running_var]).detach().clone()
    everyone = [torch.empty_like(running) for _ in range(world)]
    dist.all_gather(everyone, running)
    torch.cuda.synchronize()

    # ---------------------------------------------------------- check
    failures = []

    def ck(fn, *a):
        so._checked(failures, fn, *a)

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {name}: {what}")

    # the route: every rank on the grouped function, whatever it holds
    expect(node_name.startswith("SyncBatchNormGroupedActFunction"),
           f"output made by {node_name}")
    calls = {k: len(v) for k, v in rec.calls.items()}
    fwd = rec.calls["batch_norm_elemt_act_grouped"]
    expect(calls["batch_norm_elemt_act_grouped"] == 1
           and calls["batch_norm_stats_packed_grouped"] == 1
           and calls["batch_norm_gather_stats_packed_grouped"] == 1
           and calls["batch_norm_backward_elemt_act_grouped"] == 1,
           f"grouped ops called {calls}")
    given = list(fwd[0]["inputs"]) if fwd else []
    expect(len(given) == S and all(_dense_aligned(t) for t in given),
           "the grouped kernels were handed a tensor they cannot read")
    if odd:
        expect(odd_plan == "ineligible", f"plan of the odd group {odd_plan}")
        same = [t.data_ptr() == x.data_ptr() for t, x in zip(given, xs)]
        expect(same == [False, False, True],
               f"copies: exactly the two odd tensors, not {same}")
    if all_empty:
        # the ops run their host side only: no chunk, no block, no reduce
        expect(calls["batch_norm_backward_reduce_act_grouped"] == 0,
               "the all-empty rank ran the backward reduce")
        red_plan = ops.launch_plan("stats_grouped", given[0], given[1:])
        elt_plan = ops.launch_plan("elemt_grouped", given[0], given[1:])
        expect(red_plan["total_chunks"] == 0 and elt_plan["grid"] == 0,
               f"the all-empty rank has work: {red_plan} {elt_plan}")
    else:
        expect(calls["batch_norm_backward_reduce_act_grouped"] == 1,
               f"backward reduce calls {calls}")

    # statistics of the whole batch, per segment
    dev = lambda t: t.to(device)   # noqa: E731
    w, b = dev(d["w"]), dev(d["b"])
    segs = [(dev(X), dev(DY)) for X, DY in d["segs"]]
    orcs = _grouped_oracle({"segs": segs, "w": w, "b": b}, relu)
    expect(count.tolist() == [o[3] for o in orcs],
           f"count {count.tolist()} != {[o[3] for o in orcs]}")
    for s, (m64, v64, _, _, _) in enumerate(orcs):
        ck(_check_stats, tag, mean[s], invstd[s], m64, v64)
        ck(_check_coefs, tag, coefs[s], m64, v64, w, b)
    want_m, want_v, bound_m, bound_v = gbn._running_chain(
        dev(d["rm0"]), dev(d["rv0"]), [o[:3] for o in orcs],
        [o[3] for o in orcs], MOM)
    ck(_within, f"{tag} running_mean", bn.running_mean, want_m, bound_m)
    ck(_within, f"{tag} running_var", bn.running_var, want_v, bound_v)
    expect(all(torch.equal(e, running) for e in everyone),
           "running statistics differ between ranks")
    expect(bn.num_batches_tracked.item() == S,
           f"num_batches_tracked {bn.num_batches_tracked.item()}")

    # this rank's slices
    want_dw = want_db = bound_dw = bound_db = 0.0
    for s, ((X, DY), sl) in enumerate(zip(segs, sls)):
        shape = tuple(X[sl].shape)
        expect(tuple(ys[s].shape) == shape and ys[s].dtype == dtype
               and dxs[s] is not None and tuple(dxs[s].shape) == shape
               and dxs[s].dtype == dtype,
               f"segment {s}: shape or dtype of y / dx")
        if sl.stop == sl.start:
            continue
        wy, by, wdx, bdx, loc, bdw, bdb = _segment_wants(
            dtype, X, DY, orcs[s], sl, w, b, relu)
        ck(_within, f"{tag} y", ys[s].detach(), wy, by)
        ck(_within, f"{tag} dx", dxs[s], wdx, bdx)
        want_dw, bound_dw = want_dw + loc["grad_weight"], bound_dw + bdw
        want_db, bound_db = want_db + loc["grad_bias"], bound_db + bdb
    if all_empty:
        expect(dw is not None and not dw.any().item() and db is not None
               and not db.any().item(),
               "all-empty rank: grad_weight / grad_bias are not zeros")
    else:
        ck(_within, f"{tag} grad_weight", dw, want_dw, bound_dw)
        ck(_within, f"{tag} grad_bias", db, want_db, bound_db)
    return [f if f.startswith(tag + " " + name) else f"{name}: {f}"
            for f in failures]


# ============================================ pool and dual: the composition
# (relu, slope)
POOL_ACTS = {"relu": (True, 0.0), "leaky": (True, 0.25),
             "none": (False, 0.0)}
POOL_C, POOL_PLANE = 8, (7, 9)
DUAL_C, DUAL_PLANE = 16, (5, 7)


def _force_pool(bn, x, fork, group, world):
    """What bn_act_maxpool does once it has chosen the fused route."""
    bn.num_batches_tracked.add_(1)
    return SyncBatchNormActPoolFunction.apply(
        x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
        _momentum_factor(bn), group, world, bn.relu, bn.negative_slope, fork)


def _equal_batch(case, world):
    family, act, fork, ti, _ = case
    C, (H, W_) = (POOL_C, POOL_PLANE) if family == "pool" \
        else (DUAL_C, DUAL_PLANE)
    sizes = SIZES[world]
    g = torch.Generator().manual_seed(
        7 + 100 * sorted(POOL_ACTS).index(act or "relu") + 10 * fork + ti)
    N, dtype = sum(sizes), DTYPES[ti]
    d = {"x": _rank_batch(lambda r: (sizes[r], C, H, W_), world,
                          g).to(dtype)}
    if family == "dual":
        d["x2"] = _rank_batch(lambda r: (sizes[r], C, H, W_), world,
                              g).to(dtype)
        out = (N, C, H, W_)
    else:
        out = (N, C, (H - 1) // 2 + 1, (W_ - 1) // 2 + 1)
    d["dy1"] = torch.randn(out, generator=g).to(dtype)
    d["dy2"] = torch.randn(out, generator=g).to(dtype)
    for k in ("w", "w2"):
        d[k] = torch.randn(C, generator=g).abs() + 0.1
    for k in ("b", "b2", "rm", "rm2"):
        d[k] = torch.randn(C, generator=g)
    for k in ("rv", "rv2"):
        d[k] = torch.rand(C, generator=g) + 0.5
    return d


def _run_equal(rank, world, device, case):
    """The fused entry point (CPU: the function, forced), then the
    composition, both in this group; everything must be the same bits."""
    family, act, fork, ti, drop = case
    dtype, on_gpu = DTYPES[ti], device != "cpu"
    sizes = SIZES[world]
    off, n_loc = sum(sizes[:rank]), sizes[rank]
    d = _equal_batch(case, world)
    tag = f"[{family} W{world} r{rank}]"
    group = dist.group.WORLD

    def modules():
        if family == "pool":
            relu, slope = POOL_ACTS[act]
            ms = [SyncBatchNormAct2d(POOL_C, EPS, MOM, relu=relu,
                                     negative_slope=slope)]
        else:
            ms = [SyncBatchNormAct2d(DUAL_C, EPS, MOM),
                  SyncBatchNorm(DUAL_C, EPS, MOM)]
        for m, sfx in zip(ms, ("", "2")):
            with torch.no_grad():
                m.weight.copy_(d["w" + sfx])
                m.bias.copy_(d["b" + sfx])
                m.running_mean.copy_(d["rm" + sfx])
                m.running_var.copy_(d["rv" + sfx])
        return [m.to(device).train() for m in ms]

    def loc(key, grad=False):
        t = _cl(d[key][off:off + n_loc].to(device))
        return t.requires_grad_(True) if grad else t

    def run(fused):
        ms = modules()
        x = loc("x", True)
        ins = [x] + ([loc("x2", True)] if family == "dual" else [])
        pool = torch.nn.MaxPool2d(3, 2, 1)
        if family == "pool":
            if not fused:
                y = pool(ms[0](x))
                out = (y, y) if fork else y
            elif on_gpu:
                out = bn_act_maxpool(ms[0], pool, x, fork)
            else:
                out = _force_pool(ms[0], x, fork, group, world)
        else:
            if not fused:
                out = ms[0](x, residual=ms[1](ins[1]), fork=True) if fork \
                    else ms[0](x, residual=ms[1](ins[1]))
            elif on_gpu:
                out = bn_add_bn_act(ms[0], ms[1], x, ins[1], fork)
            else:
                out = dual_cpu._force_function(ms[0], ms[1], x, ins[1], fork,
                                               group, world)
        main, skip = out if fork else (out, None)
        node = main.grad_fn
        info = (type(node).__name__, getattr(node, "dual", None))
        loss = (main * loc("dy1")).sum()
        if fork:   # both outputs are used
            loss = loss + (skip * loc("dy2")).sum()
        params = [p for m in ms for p in (m.weight, m.bias)]
        grads = torch.autograd.grad(loss, ins + params, allow_unused=True)
        res = {"y": main.detach()}
        if fork:
            res["y_skip"] = skip.detach()
        names = ["dx", "dx_skip"][:len(ins)] + [
            f"{g}{sfx}" for sfx in ("", "_skip")[:len(ms)]
            for g in ("grad_weight", "grad_bias")]
        res.update(zip(names, grads))
        for m, sfx in zip(ms, ("", "_skip")):
            res["running_mean" + sfx] = m.running_mean.detach().clone()
            res["running_var" + sfx] = m.running_var.detach().clone()
            res["num_batches_tracked" + sfx] = m.num_batches_tracked.clone()
        return res, info

    spied = "batch_norm_elemt_act_pool" if family == "pool" \
        else "batch_norm_elemt_act_dual"
    with so._Recorder(spied) as rec, _all_reduce_dropped(drop):
        got, (node_name, dual_flag) = run(True)
    want, _ = run(False)
    if on_gpu:
        torch.cuda.synchronize()

    failures = []

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {what}")

    launched = len(rec.calls[spied])
    fn = "SyncBatchNormActPoolFunction" if family == "pool" \
        else "SyncBatchNormDualActFunction"
    if family == "pool":
        # an empty input is not eligible: that rank runs the composition
        expect(node_name.startswith(fn) == (n_loc > 0),
               f"output made by {node_name}")
        expect(launched == (1 if n_loc > 0 else 0),
               f"{launched} calls of {spied}")
    else:
        # the function on every rank; its kernels where there is an input
        expect(node_name.startswith(fn), f"output made by {node_name}")
        if on_gpu:
            expect(launched == (1 if n_loc > 0 else 0)
                   and bool(dual_flag) == (n_loc > 0),
                   f"{launched} calls of {spied}, dual {dual_flag}")
    expect(sorted(got) == sorted(want), "different result sets")
    if n_loc == 0:
        # An empty rank has no gradient for the parameters.  The dual
        # function says so with zeros (as SyncBatchNormActFunction does), the
        # plain SyncBatchNormFunction of the composition's skip layer with
        # None: the same gradient, so None is read as zeros here.
        for res in (got, want):
            for k in [k for k in res if k.startswith("grad_")]:
                if res[k] is None:
                    res[k] = torch.zeros(DUAL_C if family == "dual"
                                         else POOL_C, device=device)
    for k in want:
        expect(got[k] is not None or want[k] is None, f"{k} is missing")
        expect(dual_cpu._same(got[k], want[k]),
               f"{k} differs from the composition")
    return failures


# ====================================================================== SiLU
SILU_C = 24


def _silu_batch(case, world):
    _, with_res, fork, (H, W_), ti = case
    sizes, dtype = SIZES[world], DTYPES[ti]
    g = torch.Generator().manual_seed(
        500 + 100 * with_res + 50 * fork + 10 * H + ti)
    shape = (sum(sizes), SILU_C, H, W_)
    d = {"x": _rank_batch(lambda r: (sizes[r], SILU_C, H, W_), world,
                          g).to(dtype)}
    for k in ("res", "dy1", "dy2"):
        d[k] = torch.randn(shape, generator=g).to(dtype)
    d["w"] = torch.randn(SILU_C, generator=g).abs() + 0.5
    d["b"] = torch.randn(SILU_C, generator=g)
    d["rm"] = 0.5 * torch.randn(SILU_C, generator=g)
    d["rv"] = torch.rand(SILU_C, generator=g) + 0.5
    return d


def _silu_reference(d, with_res, fork):
    """float64 F.batch_norm + F.silu over the whole batch (what
    silu_ref.check_module builds), differentiated with the whole upstream
    gradient; ``g`` is the gradient at the BatchNorm's output."""
    x64, r64, w64, b64 = (d[k].double().requires_grad_(True)
                          for k in ("x", "res", "w", "b"))
    z = F.batch_norm(x64, None, None, w64, b64, True, 0.0, silu_ref.EPS)
    z.retain_grad()
    y64 = F.silu(z + r64 if with_res else z)
    dy = d["dy1"] + d["dy2"] if fork else d["dy1"]   # one rounding
    y64.backward(dy.double())
    return {"y": y64.detach(), "dx": x64.grad, "dres": r64.grad,
            "g": z.grad}


def _run_silu(rank, world, device, case):
    _, with_res, fork, plane, ti = case
    sizes, dtype = SIZES[world], DTYPES[ti]
    off, n_loc = sum(sizes[:rank]), sizes[rank]
    sl = slice(off, off + n_loc)
    n = float(sum(sizes) * plane[0] * plane[1])
    d = _silu_batch(case, world)
    tag = f"[silu W{world} r{rank}]"

    m = silu_ref.make_module(SyncBatchNormAct2d, d, True, device)
    x = _cl(d["x"][sl].to(device)).requires_grad_(True)
    res = _cl(d["res"][sl].to(device)).requires_grad_(True)
    args = (x, res) if with_res else (x,)
    if fork:
        y, skip = m(*args, fork=True)
        loss = (y * _cl(d["dy1"][sl].to(device))).sum() \
            + (skip * _cl(d["dy2"][sl].to(device))).sum()
    else:
        y = m(*args)
        loss = (y * _cl(d["dy1"][sl].to(device))).sum()
    node = y.grad_fn
    mean, invstd, count_sum = node.saved_tensors[4:7]
    grads = torch.autograd.grad(loss, list(args) + [m.weight, m.bias],
                                allow_unused=True)
    dx, dres = grads[0], grads[1] if with_res else None
    dw, db = grads[-2:]
    torch.cuda.synchronize()

    failures = []

    def ck(fn, *a):
        so._checked(failures, fn, *a)

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {what}")

    mean64, var64, invstd64 = o64.stats(d["x"], silu_ref.EPS)
    expect(count_sum.item() == n, f"count_sum {count_sum.tolist()} != {n}")
    ck(_check_stats, tag, mean.cpu(), invstd.cpu(), mean64, var64)
    ck(_check_running, tag, m.running_mean.cpu(), m.running_var.cpu(),
       d["rm"], d["rv"], mean64, var64, n, MOM)
    expect(tuple(y.shape) == tuple(d["x"][sl].shape) and y.dtype == dtype
           and dx is not None and dx.shape == y.shape,
           "y / dx: wrong shape or dtype")
    if n_loc == 0:
        expect(not dw.any().item() and not db.any().item(),
               "empty rank: grad_weight / grad_bias are not zeros")
        return failures
    want = _silu_reference(d, with_res, fork)
    ck(_close, f"{tag} y", y, want["y"][sl], silu_ref.tol(dtype, 1e-5))
    ck(_close, f"{tag} dx", dx, want["dx"][sl], silu_ref.tol(dtype, 1e-4))
    if with_res:
        ck(_close, f"{tag} dres", dres, want["dres"][sl],
           silu_ref.tol(dtype, 1e-5))
    g = want["g"][sl]
    xhat = (d["x"][sl].double() - o64.chan(mean64, 4)) * o64.chan(invstd64, 4)
    ck(_close, f"{tag} grad_weight", dw, (g * xhat).sum((0, 2, 3)),
       silu_ref.SUMS)
    ck(_close, f"{tag} grad_bias", db, g.sum((0, 2, 3)), silu_ref.SUMS)
    return failures


# ================================================================== conv-fed
CONV_KINDS = ("conv1x1", "dw_plain", "dw_grad_kernels", "dw_s1_grad_kernels")
CONV_PLANE = (7, 9)
MASK_LIMIT = 0.25


def _dw_stride(kind):
    """The depthwise 3x3 kinds run stride 2 but for the one named ``s1``."""
    return 1 if "_s1_" in kind else 2


@_one_thread
def _conv_batch(kind, world):
    """bf16 inputs of the whole batch and the float64 reference of the whole
    batch (CPU).  ``g`` is the gradient at the BatchNorm's output, ``keep``
    the gradient mask (conv1x1: ReLU gates the conv output's rounding could
    flip carry no upstream gradient; the SiLU layers need none)."""
    sizes = SIZES[world]
    N, (H, W_) = sum(sizes), CONV_PLANE
    gen = torch.Generator().manual_seed(11 + CONV_KINDS.index(kind))
    d = {}
    if kind == "conv1x1":
        cin, cout, oh, ow = 24, 40, H, W_
        d["cw"] = (torch.randn(cout, cin, 1, 1, generator=gen)
                   / cin ** 0.5).to(BF16)
    else:
        cin = cout = 16
        stride = _dw_stride(kind)
        oh, ow = (H - 1) // stride + 1, (W_ - 1) // stride + 1
        d["cw"] = (torch.randn(cout, 1, 3, 3, generator=gen) / 3).to(BF16)
    d["x"] = _rank_batch(lambda r: (sizes[r], cin, H, W_), world,
                         gen).to(BF16)
    d["gamma"] = torch.randn(cout, generator=gen).abs() + 0.1
    d["beta"] = torch.randn(cout, generator=gen)
    d["res"] = torch.randn(N, cout, oh, ow, generator=gen).to(BF16)
    d["gout"] = torch.randn(N, cout, oh, ow, generator=gen).to(BF16)
    if kind == "conv1x1":
        ref, keep = cs._layer_reference(d["x"], d["cw"], d["res"], d["gamma"],
                                        d["beta"], None, None, None, None,
                                        d["gout"])
        ref = {"y": ref["y"], "dx": ref["dx"], "dres": ref["dres"],
               "dw": ref["dw"], "dgamma": ref["dgamma"],
               "dbeta": ref["dbeta"], "running_mean": ref["rm_x"],
               "running_var": ref["rv_x"], "conv": ref["conv_x"],
               "dconv": ref["dconv_x"], "g": ref["dres"]}
    else:
        ref = dws._layer_reference(d["x"], d["cw"], d["gamma"], d["beta"],
                                   stride, True, d["gout"])
        ref["g"] = ref["dz"]
        keep = torch.ones_like(d["gout"])
    d["ref"], d["keep"] = ref, keep
    return d


def _conv_local(kind, d, sl):
    """This slice's contribution to the conv weight and affine gradients,
    from the whole-batch reference's gradients at the convolution's output
    and at the BatchNorm's output."""
    kw = {} if kind == "conv1x1" else dict(stride=_dw_stride(kind), padding=1,
                                           groups=d["cw"].shape[0])
    return _local_grads(d, sl, kw)


@_one_thread
def _local_grads(d, sl, conv_kw):
    """Slice ``sl``'s share of the gradients the DDP reducer sums, from the
    whole-batch reference ``d["ref"]``: the affine gradients from the
    gradient at the BatchNorm's output and the global statistics of its
    input, and with ``conv_kw`` (not None) the weight gradient of that
    convolution from the gradient at its output."""
    ref = d["ref"]
    mean, _, invstd = o64.stats(ref["conv"], cs.EPS)
    xhat = (ref["conv"][sl] - o64.chan(mean, 4)) * o64.chan(invstd, 4)
    g = ref["g"][sl]
    out = {"dgamma": (g * xhat).sum((0, 2, 3)), "dbeta": g.sum((0, 2, 3))}
    if conv_kw is not None:
        w64 = d["cw"].double().requires_grad_(True)
        (out["dw"],) = torch.autograd.grad(
            F.conv2d(d["x"][sl].double(), w64, **conv_kw), w64,
            ref["dconv"][sl])
    return out


def _mask_removed(d, sizes):
    """Fraction of elements the mask removes: of the whole batch and of
    every non-empty rank's slice."""
    offs = [sum(sizes[:r]) for r in range(len(sizes))]
    parts = [d["keep"]] + [d["keep"][o:o + k] for o, k in zip(offs, sizes)
                           if k]
    return [1.0 - p.float().mean().item() for p in parts]


def _run_conv(rank, world, device, case):
    _, kind = case
    sizes = SIZES[world]
    off, n_loc = sum(sizes[:rank]), sizes[rank]
    sl = slice(off, off + n_loc)
    d = _conv_batch(kind, world)
    tag = f"[conv W{world} r{rank}]"

    def loc(key, grad=False):
        t = _cl(d[key][sl].to(device))
        return t.requires_grad_(True) if grad else t

    if kind == "conv1x1":
        conv = torch.nn.Conv2d(24, 40, 1, bias=False)
        bn = SyncBatchNormAct2d(40)
    else:
        conv = torch.nn.Conv2d(16, 16, 3, _dw_stride(kind), 1, groups=16,
                               bias=False)
        bn = SyncBatchNormAct2d(16, act="silu")
    conv, bn = conv.to(device, BF16), bn.to(device).train()
    with torch.no_grad():
        conv.weight.copy_(d["cw"])
        bn.weight.copy_(d["gamma"])
        bn.bias.copy_(d["beta"])
    x = loc("x", True)
    res = loc("res", True) if kind == "conv1x1" else None
    gout = _cl((d["gout"] * d["keep"])[sl].to(device))
    with so._Recorder("batch_norm_stats_packed_from_partials",
                      "batch_norm_stats_packed", "dwconv3x3_backward") as rec:
        if kind == "conv1x1":
            y = conv1x1_bn_act(conv, bn, x, residual=res)
        else:
            y = dwconv3x3_bn_act(conv, bn, x,
                                 grad_kernels=kind.endswith("grad_kernels"))
        wanted = [x, conv.weight, bn.weight, bn.bias] \
            + ([res] if res is not None else [])
        grads = torch.autograd.grad((y * gout).sum(), wanted,
                                    allow_unused=True)
    got = dict(zip(("dx", "dw", "dgamma", "dbeta", "dres"), grads))
    torch.cuda.synchronize()

    failures = []

    def ck(fn, *a):
        so._checked(failures, fn, *a)

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {kind}: {what}")

    removed = _mask_removed(d, sizes)
    expect(max(removed) <= MASK_LIMIT, f"the mask removes {removed}")
    # the partials branch where the conv kernel ran; the empty rank is
    # declined by it and reads (nothing of) its input
    calls = {k: len(v) for k, v in rec.calls.items()}
    expect(calls["batch_norm_stats_packed_from_partials"]
           == (1 if n_loc else 0)
           and calls["batch_norm_stats_packed"] == 0, f"statistics {calls}")
    expect(calls["dwconv3x3_backward"]
           == (1 if n_loc and kind.endswith("grad_kernels") else 0),
           f"gradient kernels {calls}")
    ref, tol = d["ref"], _tol(BF16)
    expect(tuple(y.shape) == tuple(ref["y"][sl].shape)
           and got["dx"] is not None and got["dx"].shape == x.shape,
           "y / dx: wrong shape")
    ck(_close, f"{tag} running_mean", bn.running_mean, ref["running_mean"],
       tol)
    ck(_close, f"{tag} running_var", bn.running_var, ref["running_var"], tol)
    if n_loc == 0:
        return failures
    ck(_close, f"{tag} y", y, ref["y"][sl], tol)
    ck(_close, f"{tag} dx", got["dx"], ref["dx"][sl], tol)
    if res is not None:
        ck(_close, f"{tag} dres", got["dres"], ref["dres"][sl], tol)
    for k, v in _conv_local(kind, d, sl).items():
        ck(_close, f"{tag} {k}", got[k], v, tol)
    return [f if f.startswith(f"{tag} {kind}") else f"{kind}: {f}"
            for f in failures]


# ================================== depthwise 5x5 and squeeze-excite (dw5, se)
DWSE_C, DWSE_CR = 16, 4
# family -> kind -> (kernel size or 0 for no convolution, stride,
# grad_kernels); with se ``dx`` of ``bn_se`` is the gradient at the
# BatchNorm's input y
DWSE_KINDS = {
    "dw5": {"s1_plain": (5, 1, False), "s2_grad_kernels": (5, 2, True)},
    "se": {"bn_se": (0, 1, False), "dw3_se": (3, 1, True),
           "dw5_se": (5, 2, True)},
}
SE_PARAMS = ("w1", "b1", "w2", "b2")
DWSE_OPS = ("batch_norm_stats_packed_from_partials",
            "batch_norm_stats_packed", "dwconv3x3_backward",
            "dwconv5x5_backward", "se_squeeze", "se_scale",
            "se_backward_elemt")


class _Collectives:
    """Every ``dist.all_reduce`` / ``dist.all_gather*`` this rank issues
    while it is entered, in order, as (op, numel of the payload, dtype); the
    calls go through.  Entered inside ``_all_reduce_dropped`` it records the
    dropped calls too."""

    NAMES = ("all_reduce", "all_gather", "all_gather_into_tensor")

    def __enter__(self):
        self.calls, self._real = [], {}
        for n in self.NAMES:
            real = getattr(dist, n)

            def wrapped(*a, _real=real, _n=n, **kw):
                # all_reduce(tensor, ...); all_gather*(output, input, ...)
                t = a[0] if _n == "all_reduce" else a[1]
                self.calls.append((_n, t.numel(), str(t.dtype)))
                return _real(*a, **kw)

            self._real[n] = real
            setattr(dist, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, real in self._real.items():
            setattr(dist, n, real)


def _se64(a, w1, b1, w2, b2):
    """SqueezeExcite.forward on float64 tensors."""
    s = a.mean((2, 3), keepdim=True)
    return a * torch.sigmoid(F.conv2d(F.silu(F.conv2d(s, w1, b1)), w2, b2))


@_one_thread
def _dwse_batch(family, kind, world, dtype):
    """Inputs of the whole batch rounded to ``dtype`` (fp32 gamma, beta) and
    the float64 reference of the whole batch on the CPU: autograd of conv
    (its output stored in ``dtype``, ``cs._Stored``), batch_norm, silu and,
    for ``se``, the squeeze-excite block.  Kept besides the outputs and the
    leaves' gradients: ``conv`` / ``dconv`` the BatchNorm's input and the
    gradient at the convolution's output, ``g`` the gradient at the
    BatchNorm's output, ``a`` the activated tensor."""
    k, stride, _ = DWSE_KINDS[family][kind]
    sizes, C, Cr = SIZES[world], DWSE_C, DWSE_CR
    N, (H, W_) = sum(sizes), CONV_PLANE
    gen = torch.Generator().manual_seed(
        31 + 10 * sorted(DWSE_KINDS[family]).index(kind)
        + 100 * (family == "se"))
    oh, ow = (H - 1) // stride + 1, (W_ - 1) // stride + 1
    d = {"x": _rank_batch(lambda r: (sizes[r], C, H, W_), world,
                          gen).to(dtype)}
    if k:
        d["cw"] = (torch.randn(C, 1, k, k, generator=gen) / k).to(dtype)
    d["gamma"] = torch.randn(C, generator=gen).abs() + 0.1
    d["beta"] = torch.randn(C, generator=gen)
    d["gout"] = torch.randn(N, C, oh, ow, generator=gen).to(dtype)
    if family == "dw5":
        ref = dws._layer_reference(d["x"], d["cw"], d["gamma"], d["beta"],
                                   stride, True, d["gout"], k=5)
        ref["g"] = ref["dz"]
        d["ref"] = ref
        return d
    for name, shape in zip(SE_PARAMS, ((Cr, C, 1, 1), (Cr,), (C, Cr, 1, 1),
                                       (C,))):
        d[name] = (torch.randn(shape, generator=gen) / 2).to(dtype)
    lv = {n: d[n].double().requires_grad_(True)
          for n in ("x", "gamma", "beta") + SE_PARAMS + (("cw",) if k else ())}
    if k:
        raw = F.conv2d(lv["x"], lv["cw"], stride=stride, padding=k // 2,
                       groups=C)
        raw.retain_grad()
        yc = cs._Stored.apply(raw, dtype)
    else:
        yc = lv["x"]
    mean, var, _ = o64.stats(yc.detach(), cs.EPS)
    count = yc.numel() // C
    z = F.batch_norm(yc, None, None, lv["gamma"], lv["beta"], True, 0.0,
                     cs.EPS)
    z.retain_grad()
    a = F.silu(z)
    out = _se64(a, *(lv[n] for n in SE_PARAMS))
    out.backward(d["gout"].double())
    ref = {"out": out.detach(), "dx": lv["x"].grad, "g": z.grad,
           "a": a.detach(), "conv": yc.detach(),
           "dgamma": lv["gamma"].grad, "dbeta": lv["beta"].grad,
           "running_mean": 0.1 * mean,
           "running_var": 0.9 + 0.1 * var * count / (count - 1.0)}
    ref.update(("d" + n, lv[n].grad) for n in SE_PARAMS)
    if k:
        ref["dw"], ref["dconv"] = lv["cw"].grad, raw.grad
    d["ref"] = ref
    return d


@_one_thread
def _dwse_local(family, kind, d, sl):
    """``_local_grads`` of the slice and, for ``se``, the block's own
    parameter gradients: SE is per image, so they are float64 autograd of
    the block alone on the slice of the activated tensor."""
    k, stride, _ = DWSE_KINDS[family][kind]
    out = _local_grads(d, sl, dict(stride=stride, padding=k // 2,
                                   groups=DWSE_C) if k else None)
    if family == "se":
        ps = [d[n].double().requires_grad_(True) for n in SE_PARAMS]
        grads = torch.autograd.grad(_se64(d["ref"]["a"][sl], *ps), ps,
                                    d["gout"][sl].double())
        out.update(zip(("d" + n for n in SE_PARAMS), grads))
    return out


def _force_se(bn, se, y, group, world):
    """What bn_silu_se does once it has chosen the fused route."""
    bn.num_batches_tracked.add_(1)
    return SyncBatchNormSiluSEFunction.apply(
        y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
        _momentum_factor(bn), group, world, se.fc1.weight, se.fc1.bias,
        se.fc2.weight, se.fc2.bias)


def _run_dwse(rank, world, device, case):
    """``(family, kind, dtype name, drop)``.  On the CPU (``bn_se`` only)
    the non-empty ranks apply SyncBatchNormSiluSEFunction themselves, the
    empty one calls bn_silu_se as on the GPU."""
    family, kind, dtype_name, drop = case
    k, stride, grad_kernels = DWSE_KINDS[family][kind]
    dtype, on_gpu, with_se = getattr(torch, dtype_name), device != "cpu", \
        family == "se"
    sizes, C = SIZES[world], DWSE_C
    off, n_loc = sum(sizes[:rank]), sizes[rank]
    sl = slice(off, off + n_loc)
    d = _dwse_batch(family, kind, world, dtype)
    ref, tol = d["ref"], _tol(dtype)
    tag = f"[{family} W{world} r{rank}]"
    out_name = "out" if with_se else "y"

    # ------------------------------------------------------------ run
    conv = se = None
    if k:
        conv = torch.nn.Conv2d(C, C, k, stride, k // 2, groups=C,
                               bias=False).to(device, dtype)
    bn = SyncBatchNormAct2d(C, act="silu").to(device).train()
    with torch.no_grad():
        if k:
            conv.weight.copy_(d["cw"])
        bn.weight.copy_(d["gamma"])
        bn.bias.copy_(d["beta"])
    params = {"dgamma": bn.weight, "dbeta": bn.bias}
    if k:
        params["dw"] = conv.weight
    if with_se:
        se = SqueezeExcite(C, DWSE_CR).to(device, dtype)
        se_params = (se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias)
        with torch.no_grad():
            for p, n in zip(se_params, SE_PARAMS):
                p.copy_(d[n])
        params.update(zip(("d" + n for n in SE_PARAMS), se_params))
    x = _cl(d["x"][sl].to(device)).requires_grad_(True)
    gout = _cl(d["gout"][sl].to(device))
    with _all_reduce_dropped(drop), _Collectives() as col, \
            so._Recorder(*DWSE_OPS) as rec:
        if family == "dw5":
            y = dwconv5x5_bn_act(conv, bn, x, grad_kernels=grad_kernels)
        elif k:
            layer = dwconv3x3_bn_act if k == 3 else dwconv5x5_bn_act
            y = layer(conv, bn, x, grad_kernels=grad_kernels, se=se)
        elif on_gpu or not n_loc:
            y = bn_silu_se(bn, se, x)
        else:
            y = _force_se(bn, se, x, dist.group.WORLD, world)
        node_name = type(y.grad_fn).__name__
        grads = torch.autograd.grad((y * gout).sum(),
                                    [x] + list(params.values()),
                                    allow_unused=True)
    got = dict(zip(["dx"] + list(params), grads))
    running = torch.cat([bn.running_mean, bn.running_var]).detach().clone()
    everyone = [torch.empty_like(running) for _ in range(world)]
    dist.all_gather(everyone, running)
    schedules = [None] * world
    dist.all_gather_object(schedules, col.calls)
    if on_gpu:
        torch.cuda.synchronize()

    # ---------------------------------------------------------- check
    failures = []

    def ck(fn, *a):
        so._checked(failures, fn, *a)

    def expect(cond, what):
        if not cond:
            failures.append(f"{tag} {kind}: {what}")

    # one all_gather forward and one [2C] all_reduce backward, fp32, on
    # every rank, whichever autograd Function it runs
    want_calls = [("all_gather", 2 * C + 1, "torch.float32"),
                  ("all_reduce", 2 * C, "torch.float32")]
    expect(col.calls == want_calls, f"collectives {col.calls}")
    expect(all(s == schedules[0] for s in schedules),
           f"collectives differ between ranks: {schedules}")
    calls = {n: len(v) for n, v in rec.calls.items()}
    kernels = bool(n_loc and k and on_gpu)
    expect(calls["batch_norm_stats_packed_from_partials"] == int(kernels)
           and calls["batch_norm_stats_packed"] == int(bool(n_loc and not k)),
           f"statistics {calls}")
    expect(calls["dwconv3x3_backward"]
           == int(kernels and k == 3 and grad_kernels)
           and calls["dwconv5x5_backward"]
           == int(kernels and k == 5 and grad_kernels),
           f"gradient kernels {calls}")
    fused = int(bool(with_se and n_loc))
    expect(all(calls[n] == fused for n in ("se_squeeze", "se_scale",
                                           "se_backward_elemt")),
           f"squeeze-excite ops {calls}")
    if with_se:
        expect(node_name.startswith("SyncBatchNormSiluSEFunction")
               == (n_loc > 0), f"output made by {node_name}")
    expect(tuple(y.shape) == tuple(ref[out_name][sl].shape)
           and y.dtype == dtype and got["dx"] is not None
           and got["dx"].shape == x.shape and got["dx"].dtype == dtype,
           f"{out_name} / dx: wrong shape or dtype")
    ck(_close, f"{tag} running_mean", bn.running_mean, ref["running_mean"],
       tol)
    ck(_close, f"{tag} running_var", bn.running_var, ref["running_var"], tol)
    expect(all(torch.equal(e, running) for e in everyone),
           "running statistics differ between ranks")
    expect(bn.num_batches_tracked.item() == 1,
           f"num_batches_tracked {bn.num_batches_tracked.item()}")
    if n_loc == 0:
        # no sample, no gradient: None is read as zeros (see _run_equal)
        for n, p in params.items():
            expect(got[n] is None or (got[n].shape == p.shape
                                      and not got[n].any().item()),
                   f"empty rank: {n} is not zeros")
    else:
        ck(_close, f"{tag} {out_name}", y, ref[out_name][sl], tol)
        ck(_close, f"{tag} dx", got["dx"], ref["dx"][sl], tol)
        for n, v in _dwse_local(family, kind, d, sl).items():
            expect(got[n] is not None and got[n].shape == params[n].shape,
                   f"{n} is missing or misshapen")
            if got[n] is not None:
                ck(_close, f"{tag} {n}", got[n], v, tol)
    return [f if f.startswith(f"{tag} {kind}") else f"{kind}: {f}"
            for f in failures]


# ============================================================ the GPU tier
RUNNERS = {"grouped": _run_grouped, "pool": _run_equal, "dual": _run_equal,
           "silu": _run_silu, "conv": _run_conv, "dw5": _run_dwse,
           "se": _run_dwse}
# the quantities every family must have been measured on
MEASURED = {"grouped": ("y", "dx", "mean", "invstd", "scale", "shift",
                        "running_mean", "running_var", "grad_weight",
                        "grad_bias"),
            "silu": ("y", "dx", "dres", "mean", "invstd", "running_var",
                     "grad_weight", "grad_bias"),
            "conv": ("y", "dx", "dres", "dw", "dgamma", "dbeta",
                     "running_var"),
            "dw5": ("y", "dx", "dw", "dgamma", "dbeta", "running_mean",
                    "running_var"),
            "se": ("out", "dx", "dw", "dgamma", "dbeta", "dw1", "db1", "dw2",
                   "db2", "running_mean", "running_var")}


def run_case(rank, world, device, case):
    """One case on one rank: run (every collective), then check.  Returns
    the failures; raises only if the run itself broke."""
    return RUNNERS[case[0]](rank, world, device, case)


def _gpu_cases():
    cases = [("grouped", name, ti) for name in GROUPS for ti in (0, 1)]
    cases += [("pool", act, fork, ti, False) for act in POOL_ACTS
              for fork in (False, True) for ti in (0, 1)]
    # fp32 is not eligible for the dual route: bf16 only
    cases += [("dual", None, fork, 1, False) for fork in (False, True)]
    cases += [("silu", with_res, fork, plane, ti)
              for with_res in (False, True) for fork in (False, True)
              for plane in so.PLANES for ti in (0, 1)]
    cases += [("conv", kind) for kind in CONV_KINDS]
    cases += [(family, kind, "bfloat16", False) for family in DWSE_KINDS
              for kind in DWSE_KINDS[family]]
    cases += [("se", "bn_se", "float16", False)]
    return cases


_RATIO = re.compile(r"^\[(\w+) W\d r\d\] (.+?): .*max err/bound (\S+)$")


def _report(world, device, outputs):
    """Worst err/bound that ``_within`` printed, per layer family and per
    quantity, over ranks and cases (the format of test_sync_oracle)."""
    worst = {}
    for per_case in outputs.values():
        for _, text in per_case:
            for line in text.splitlines():
                mt = _RATIO.match(line)
                if mt:
                    key = (mt.group(1), mt.group(2))
                    worst[key] = max(worst.get(key, 0.0), float(mt.group(3)))
    for family in MEASURED:
        row = ", ".join(f"{q} {v:.2f}" for (c, q), v in sorted(worst.items())
                        if c == family)
        print(f"worst err/bound, W={world} {device}, case {family}: {row}")
    return worst


@gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sync_layers_gpu(world, tmp_path):
    """Measured on an MI355X (worst err/bound; 5 s at W = 2, 5 s at W = 4,
    the float64 references on one thread; the dw5 and se cases take 0.01 s
    each):

    W=2 grouped: dx 0.18, grad_bias 0.02, grad_weight 0.03, invstd 0.01,
      mean 0.10, running_mean 0.11, running_var 0.01, scale 0.01, shift 0.02,
      y 0.36
    W=2 silu: dres 0.14, dx 0.22, grad_bias 0.00, grad_weight 0.00,
      invstd 0.01, mean 0.09, running_mean 0.25, running_var 0.01, y 0.16
    W=2 conv: dbeta 0.00, dgamma 0.00, dres 0.00, dw 0.17, dx 0.12,
      running_mean 0.00, running_var 0.00, y 0.15
    W=2 dw5: dbeta 0.00, dgamma 0.00, dw 0.17, dx 0.11, running_mean 0.00,
      running_var 0.00, y 0.13
    W=2 se: db1 0.10, db2 0.16, dbeta 0.00, dgamma 0.00, dw 0.16, dw1 0.14,
      dw2 0.14, dx 0.08, out 0.12, running_mean 0.00, running_var 0.00
    W=4 grouped: dx 0.16, grad_bias 0.02, grad_weight 0.01, invstd 0.01,
      mean 0.09, running_mean 0.11, running_var 0.01, scale 0.01, shift 0.02,
      y 0.35
    W=4 silu: dres 0.14, dx 0.15, grad_bias 0.00, grad_weight 0.00,
      invstd 0.01, mean 0.08, running_mean 0.13, running_var 0.01, y 0.16
    W=4 conv: dbeta 0.00, dgamma 0.00, dres 0.00, dw 0.18, dx 0.09,
      running_mean 0.00, running_var 0.00, y 0.15
    W=4 dw5: dbeta 0.00, dgamma 0.00, dw 0.17, dx 0.06, running_mean 0.00,
      running_var 0.00, y 0.15
    W=4 se: db1 0.09, db2 0.13, dbeta 0.00, dgamma 0.00, dw 0.16, dw1 0.15,
      dw2 0.13, dx 0.06, out 0.14, running_mean 0.00, running_var 0.00
    """
    outputs = harness.run_cases(tmp_path, world, "cuda:0",
                                "test_sync_layers:run_case", _gpu_cases())
    assert sorted(outputs) == list(range(world))
    worst = _report(world, "cuda:0", outputs)
    for family, quantities in MEASURED.items():
        for q in quantities:
            assert (family, q) in worst, (family, q)


# ======================================================= can the data tell?
def test_conv_masks_and_rank_local_references():
    """The gradient mask of the conv-fed cases is a condition on the data:
    it removes at most a quarter of the whole batch and of every rank's
    slice (float64 reference alone).  And the rank-local references are what
    they claim: summed over the ranks they are the whole-batch gradients."""
    for world in (2, 4):
        sizes = SIZES[world]
        offs = [sum(sizes[:r]) for r in range(world)]
        for kind in CONV_KINDS[:2]:
            d = _conv_batch(kind, world)
            removed = _mask_removed(d, sizes)
            print(f"{kind} W={world}: mask removes "
                  + ", ".join(f"{r:.3f}" for r in removed))
            assert max(removed) <= MASK_LIMIT, (kind, world, removed)
            parts = [_conv_local(kind, d, slice(o, o + k))
                     for o, k in zip(offs, sizes) if k]
            for key in ("dw", "dgamma", "dbeta"):
                torch.testing.assert_close(sum(p[key] for p in parts),
                                           d["ref"][key], rtol=1e-9,
                                           atol=1e-9)


def test_wrong_grouped_compositions_violate_the_bounds():
    """Oracle only, the 4-rank sizes, both dtypes: seven wrong ways to
    compose the grouped statistics and gradients each miss the bounds of the
    GPU tier by at least 10x (the dx ones on some non-empty rank).  The
    pyramid's per-rank counts are proportional from one segment to the next,
    so taking the neighbour's counts changes nothing there: that mistake is
    shown on the ragged group, whose counts are not."""
    world = 4
    for name in ("pyramid_act", "ragged"):
        C, planes, _ = GROUPS[name]
        S, counts = len(planes), _counts(name, world)
        for ti, dtype in enumerate(DTYPES):
            d = _grouped_batch(name, world, ti)
            w, b = d["w"], d["b"]
            orcs = _grouped_oracle(d, True)
            r = dict.fromkeys(("neighbour counts", "no between-rank term",
                               "unweighted mean", "local sums",
                               "local count"), 0.0)
            for s, ((X, DY), (mean, var, invstd, n, red)) in enumerate(
                    zip(d["segs"], orcs)):
                plane = float(planes[s][0] * planes[s][1])
                rtol, matol = _stat_bounds(mean, var)
                offs = [sum(counts[q][s] for q in range(k))
                        for k in range(world)]
                ranks = [(k, slice(offs[k], offs[k] + counts[k][s]))
                         for k in range(world) if counts[k][s]]
                per = [o64.stats(X[sl], EPS) for _, sl in ranks]
                cnt = [counts[k][s] * plane for k, _ in ranks]
                good = o64.gather([p[0] for p in per], [p[1] for p in per],
                                  cnt, EPS)
                _check_stats(f"{name} seg{s} merge", good[0], good[2], mean,
                             var)

                def stat_miss(m, i):
                    return max(((m - mean).abs() / matol).max().item(),
                               ((i - invstd).abs() / (rtol * invstd)).max()
                               .item())

                # 1. segment s merged with segment s+1's per-rank counts
                nxt = (s + 1) % S
                wrong = [counts[k][nxt] * float(planes[nxt][0]
                                                * planes[nxt][1])
                         for k, _ in ranks]
                if sum(wrong) > 0:
                    m, _, i = o64.gather([p[0] for p in per],
                                         [p[1] for p in per], wrong, EPS)
                    r["neighbour counts"] = max(r["neighbour counts"],
                                                stat_miss(m, i))
                if len(ranks) > 1:
                    # 2. the merge without its between-rank variance term
                    within = sum(c * p[1] for p, c in zip(per, cnt)) / n
                    r["no between-rank term"] = max(
                        r["no between-rank term"],
                        stat_miss(mean, torch.rsqrt(within + EPS)))
                    # 3. an unweighted mean over the ranks
                    flat = sum(p[0] for p in per) / len(per)
                    r["unweighted mean"] = max(r["unweighted mean"],
                                               stat_miss(flat, invstd))
                for k, sl in ranks:
                    _, _, want, bound, loc, _, _ = _segment_wants(
                        dtype, X, DY, orcs[s], sl, w, b, True)

                    def dx_miss(sum_dy, sum_dy_xmu, count):
                        got = o64.backward_elemt(
                            DY[sl], X[sl], mean, invstd, w, b, sum_dy,
                            sum_dy_xmu, count, None, True)[0]
                        return ((got - want).abs() / bound).max().item()

                    if len(ranks) > 1:
                        # 4. rank-local sums: the all_reduce left out
                        r["local sums"] = max(r["local sums"], dx_miss(
                            loc["sum_dy"], loc["sum_dy_xmu"], n))
                        # 5. the local count in dx
                        r["local count"] = max(r["local count"], dx_miss(
                            red["sum_dy"], red["sum_dy_xmu"],
                            counts[k][s] * plane))
            # 6. / 7. the running statistics' chain
            stats = [o[:3] for o in orcs]
            ns = [o[3] for o in orcs]
            want_m, want_v, bound_m, bound_v = gbn._running_chain(
                d["rm0"], d["rv0"], stats, ns, MOM)

            def chain_miss(stats, ns):
                m, v, _, _ = gbn._running_chain(d["rm0"], d["rv0"], stats,
                                                ns, MOM)
                return max(((m - want_m).abs() / bound_m).max().item(),
                           ((v - want_v).abs() / bound_v).max().item())

            r["one running update"] = chain_miss(stats[-1:], ns[-1:])
            r["reverse segment order"] = chain_miss(stats[::-1], ns[::-1])
            print(f"{name} {dtype}: " + ", ".join(
                f"{k} {v:.3g}" for k, v in r.items()))
            for k, v in r.items():
                if name == "pyramid_act" and k == "neighbour counts":
                    continue
                assert v >= 10, (name, dtype, k, v)


CPU_EQUAL = [("pool", "relu", True, 0), ("pool", "leaky", False, 0),
             ("dual", None, False, 0), ("dual", None, True, 0)]


def run_cpu_equal_case(rank, world, device, case):
    return _run_equal(rank, world, device, case)


def test_equality_tier_notices_a_dropped_all_reduce(tmp_path):
    """Two gloo ranks on the reference ops, the pool and dual functions
    forced: the comparison with the composition passes; with all_reduce a
    no-op while the functions run, every case reports a difference."""
    spec = "test_sync_layers:run_cpu_equal_case"
    harness.run_cases(tmp_path, 2, "cpu", spec,
                      [c + (False,) for c in CPU_EQUAL])
    with pytest.raises(AssertionError) as e:
        harness.run_cases(tmp_path, 2, "cpu", spec,
                          [c + (True,) for c in CPU_EQUAL])
    msg = str(e.value)
    print(msg)
    assert "timeout" not in msg and harness.NOT_RUN not in msg \
        and "Traceback" not in msg, msg
    for case in CPU_EQUAL:
        for rank in (0, 1):
            assert f"rank {rank}, case {case + (True,)!r}:\n" \
                f"[{case[0]} W2 r{rank}] dx differs" in msg, (rank, case)


# ============================== dw5 and se: can the references, the test tell?
def test_dwse_rank_local_references_add_up():
    """Reference only, both worlds, every kind this file adds for the
    depthwise 5x5 and squeeze-excite layers (and the stride-1 3x3 kind): the
    rank-local references of the conv weight, affine and SE parameter
    gradients, summed over the non-empty ranks, are the whole-batch float64
    gradients."""
    for world in (2, 4):
        sizes = SIZES[world]
        sls = [slice(sum(sizes[:r]), sum(sizes[:r + 1]))
               for r in range(world) if sizes[r]]
        todo = [("conv", "dw_s1_grad_kernels", "bfloat16", False)] + [
            c for c in _gpu_cases() if c[0] in DWSE_KINDS]
        for family, kind, dtype_name, _ in todo:
            if family == "conv":
                d = _conv_batch(kind, world)
                parts = [_conv_local(kind, d, sl) for sl in sls]
            else:
                d = _dwse_batch(family, kind, world,
                                getattr(torch, dtype_name))
                parts = [_dwse_local(family, kind, d, sl) for sl in sls]
            want = {"conv": 3, "dw5": 3, "se": 7 if kind != "bn_se" else 6}
            assert len(parts[0]) == want[family], (kind, sorted(parts[0]))
            for key in parts[0]:
                torch.testing.assert_close(
                    sum(p[key] for p in parts), d["ref"][key], rtol=1e-9,
                    atol=1e-9, msg=lambda m: f"{family} {kind} W={world} "
                    f"{key}: {m}")


CPU_SE = ("se", "bn_se", "float32")
_DX_MISS = r"\[se W{w} r{r}\] dx: .*worst err/bound (\S+) at"


def run_cpu_dwse_case(rank, world, device, case):
    return _run_dwse(rank, world, device, case)


@pytest.mark.parametrize("world", [2, 4])
def test_se_function_on_gloo_and_a_dropped_all_reduce(world, tmp_path):
    """gloo ranks on the reference ops, fp32 CPU tensors:
    SyncBatchNormSiluSEFunction applied on the non-empty ranks, bn_silu_se
    (the composition) on the empty one of W = 4, held to the whole-batch
    float64 reference by the checker of the GPU tier, collective parity
    included.  With all_reduce a no-op while the layer runs, every non-empty
    rank reports dx: it misses ``_tol(float32)`` against the float64
    reference by 4.2e3x / 1.5e3x (W = 2, ranks 0 / 1) and 1.6e3x / 1.7e3x /
    1.0e3x (W = 4, ranks 0 / 2 / 3).

    Why fp32: the reference SE ops work at the wider of fp32 and the tensors'
    dtype, so on fp64 tensors the Function's ``[2C]`` backward all_reduce
    carries fp64 sums, while the empty rank's composition
    (SyncBatchNormActFunction.backward) sends fp32 zeros; gloo aborts on the
    size mismatch.  That pairing exists only where the Function is applied by
    hand as here: bn_silu_se takes the Function for CUDA bf16 / half tensors
    alone, whose kernels emit fp32 sums, and every BatchNorm reduce op, HIP
    or reference, returns fp32 sums whatever the input dtype.  The forward
    all_gather is packed fp32 on every route."""
    spec = "test_sync_layers:run_cpu_dwse_case"
    outputs = harness.run_cases(tmp_path, world, "cpu", spec,
                                [CPU_SE + (False,)])
    worst = _report(world, "cpu", outputs)
    for q in MEASURED["se"]:
        assert q == "dw" or ("se", q) in worst, q
    with pytest.raises(AssertionError) as e:
        harness.run_cases(tmp_path, world, "cpu", spec, [CPU_SE + (True,)])
    msg = str(e.value)
    print(msg)
    assert "timeout" not in msg and harness.NOT_RUN not in msg \
        and "Traceback" not in msg and "collectives" not in msg, msg
    for rank, n_loc in enumerate(SIZES[world]):
        miss = re.search(_DX_MISS.format(w=world, r=rank), msg)
        assert (miss is not None) == (n_loc > 0), (rank, n_loc)
        if miss:
            print(f"W={world} rank {rank}: a dropped all_reduce misses the "
                  f"dx bound {float(miss.group(1)):.3g}x")
            assert float(miss.group(1)) >= 10, (rank, miss.group(1))
