#!/usr/bin/env python3
"""Stem pool fusion, kernel by kernel, at the benchmark's stem shape
(512x64x112x112 bf16 channels-last): each fused kernel next to the stock
kernels it replaces, timed with hipEvents, three alternated runs.

    python benchmarks/bench_stem_pool.py [--iters 30] [--runs 3] [--impl nt]

Achieved GB/s is (bytes the kernel must move) / time, with A the bytes of the
full-size activation: the byte counts of docs/KERNEL_DESIGN.md "Stem pool
fusion".  ``--impl nont`` runs the cached-access A/B build (MSBN_BUILD_NONT=1
at setup time): plain instead of nontemporal window / gather loads.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from msbn import ops


def bench(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1000.0 / iters  # us


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--shape", type=int, nargs=4, default=[512, 64, 112, 112])
    p.add_argument("--impl", default="nt", choices=["nt", "nont"])
    p.add_argument("--json", action="store_true")
    args = p.parse_args()

    if args.impl == "nont":
        import msbn._C_nont as C_nont
        import msbn.ops as _ops_mod

        _ops_mod._C = C_nont

    dev, dt = "cuda", torch.bfloat16
    N, C, H, W = args.shape
    cl = torch.channels_last
    x = torch.randn(N, C, H, W, device=dev, dtype=dt).to(memory_format=cl)
    w = torch.randn(C, device=dev).abs() + 0.1
    b = torch.randn(C, device=dev)
    mean, invstd = ops.batch_norm_stats(x, 1e-5)
    coefs = ops.bn_make_coefs(mean, invstd, w, b)
    cnt = torch.full((1,), float(x.numel() // C), device=dev)
    A = x.numel() * x.element_size()

    y = ops.batch_norm_elemt_act(x, None, w, b, mean, invstd, True, coefs)
    pooled, idx = F.max_pool2d(y, 3, 2, 1, return_indices=True)
    pooled_f, codes = ops.batch_norm_elemt_act_pool(x, w, b, mean, invstd,
                                                    True, coefs)
    assert torch.equal(pooled, pooled_f)
    dy1 = torch.randn_like(pooled)
    dy2 = torch.randn_like(pooled)
    dy = dy1 + dy2

    def pool_bwd():
        return torch.ops.aten.max_pool2d_with_indices_backward(
            dy, y, [3, 3], [2, 2], [1, 1], [1, 1], False, idx)

    g_full = pool_bwd()
    red = ops.batch_norm_backward_reduce_act(
        g_full, x, None, mean, invstd, w, b, True, True, True, True, coefs)
    red_f = ops.batch_norm_backward_reduce_act_pool(
        dy1, dy2, codes, x, mean, invstd, w, b, True, True, True, True, coefs)
    assert all(torch.equal(a, e) for a, e in zip(red_f, red))
    sum_dy, sum_dy_xmu = red[0], red[1]

    cases = {
        # name: (fn, bytes in units of A)
        "stock bn_elemt+relu": (
            lambda: ops.batch_norm_elemt_act(x, None, w, b, mean, invstd,
                                             True, coefs), 2.0),
        "stock max_pool fwd": (
            lambda: F.max_pool2d(y, 3, 2, 1, return_indices=True), 2.25),
        "fused elemt_pool": (
            lambda: ops.batch_norm_elemt_act_pool(x, w, b, mean, invstd, True,
                                                  coefs), 1.375),
        "stock add(dy1,dy2)": (lambda: torch.add(dy1, dy2), 0.75),
        "stock max_pool bwd": (pool_bwd, 2.25),
        "stock bwd_reduce+relu": (
            lambda: ops.batch_norm_backward_reduce_act(
                g_full, x, None, mean, invstd, w, b, True, True, True, True,
                coefs), 2.0),
        "fused bwd_reduce_pool+dy2": (
            lambda: ops.batch_norm_backward_reduce_act_pool(
                dy1, dy2, codes, x, mean, invstd, w, b, True, True, True,
                True, coefs), 1.625),
        "stock bwd_elemt+relu": (
            lambda: ops.batch_norm_backward_elemt_act(
                g_full, x, None, mean, invstd, w, b, sum_dy, sum_dy_xmu, cnt,
                True, False, coefs), 3.0),
        "fused bwd_elemt_pool+dy2": (
            lambda: ops.batch_norm_backward_elemt_act_pool(
                dy1, dy2, codes, x, mean, invstd, w, b, sum_dy, sum_dy_xmu,
                cnt, True, coefs), 2.625),
    }
    rows = []
    for run in range(args.runs):
        for name, (fn, units) in cases.items():
            us = bench(fn, args.iters)
            rows.append({"run": run + 1, "kernel": name, "us": round(us, 1),
                         "GBps": round(units * A / (us * 1e-6) / 1e9, 1)})
    if args.json:
        print(json.dumps(rows))
        return
    print(f"shape {N}x{C}x{H}x{W} bf16 channels_last, impl {args.impl}")
    print(f"{'kernel':>28} " + " ".join(f"{'us run' + str(r + 1):>10}"
                                        for r in range(args.runs))
          + "   GB/s (per run)")
    for name in cases:
        rs = [r for r in rows if r["kernel"] == name]
        print(f"{name:>28} " + " ".join(f"{r['us']:>10}" for r in rs)
              + "   " + " / ".join(str(r["GBps"]) for r in rs))


if __name__ == "__main__":
    main()
