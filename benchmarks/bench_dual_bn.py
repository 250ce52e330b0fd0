#!/usr/bin/env python3
"""Dual BN, kernel by kernel, at the four downsample-block shapes of the
ResNet-50 benchmark (bf16 channels-last, batch 512): the composition's five
kernels next to the dual three.  hipEvent timing, alternated runs.

    python benchmarks/bench_dual_bn.py [--iters 30] [--runs 3] [--json]

Before timing, every shape checks that the dual route reproduces the
composition bit for bit (y, the gate bits, gm, all four sums, both layers'
affine gradients, dx and dx_d).

Achieved GB/s is (bytes the kernels must move) / time with A the bytes of
one activation tensor, gate bits and per-channel vectors left out: forward
5A composed (2A + 3A) / 3A dual; backward reduce 6A (4A + 2A) / 5A; backward
elemt 6A (3A + 3A) / 5A (the traffic table of docs/KERNEL_DESIGN.md
"Dual BN").  Each row's time includes its tiny per-channel kernels
(finalize, coefficient) as the ops launch them.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from msbn import ops

SHAPES = [
    (512, 256, 56, 56),
    (512, 512, 28, 28),
    (512, 1024, 14, 14),
    (512, 2048, 7, 7),
]


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


def one_shape(shape, iters, runs):
    dev, dt = "cuda", torch.bfloat16
    N, C, H, W = shape
    cl = torch.channels_last

    def rand(scale=1.0, shift=0.0):
        t = torch.randn(N, C, H, W, device=dev) * scale + shift
        return t.to(dt).to(memory_format=cl)

    x, x_d, dy1, dy2 = rand(1.0, 1.0), rand(2.0, -1.5), rand(), rand()
    w, w2 = (torch.randn(C, device=dev).abs() + 0.1 for _ in range(2))
    b, b2 = (torch.randn(C, device=dev) for _ in range(2))
    mean, invstd = ops.batch_norm_stats(x, 1e-5)
    mean2, invstd2 = ops.batch_norm_stats(x_d, 1e-5)
    coefs = ops.bn_make_coefs(mean, invstd, w, b)
    coefs2 = ops.bn_make_coefs(mean2, invstd2, w2, b2)
    count = torch.full((1,), float(N * H * W), device=dev)
    A = x.numel() * x.element_size()
    bits_c, bits_d = ops.gate_bits_empty(x), ops.gate_bits_empty(x)
    gm_c, gm_d = torch.empty_like(x), torch.empty_like(x)

    def fwd_composed():
        r = ops.batch_norm_elemt_act(x_d, None, w2, b2, mean2, invstd2,
                                     False, coefs2)
        return ops.batch_norm_elemt_act(x, r, w, b, mean, invstd, True,
                                        coefs, 0.0, bits_c)

    def fwd_dual():
        return ops.batch_norm_elemt_act_dual(x, x_d, coefs, coefs2, True,
                                             0.0, bits_d)

    def red_composed():
        main = ops.batch_norm_backward_reduce_act(
            dy1, x, None, mean, invstd, w, b, True, True, True, True, coefs,
            gm_c, 0.0, dy2, gate=bits_c)
        skip = ops.batch_norm_backward_reduce(gm_c, x_d, mean2, invstd2, w2,
                                              True, True, True)
        return tuple(main) + tuple(skip)

    def red_dual():
        return ops.batch_norm_backward_reduce_act(
            dy1, x, None, mean, invstd, w, b, True, True, True, True, coefs,
            gm_d, 0.0, dy2, gate=bits_d, dual=(x_d, mean2, invstd2, w2))

    y_c, wrote = fwd_composed()
    assert wrote is bits_c, "the composed forward declined to store the bits"
    y_d, stored = fwd_dual()
    assert stored, "the dual forward declined"
    assert torch.equal(y_c, y_d) and torch.equal(bits_c, bits_d)
    for kind, others in (("bwd_reduce_dual", (dy1, x_d, gm_d, dy2, bits_d)),
                         ("bwd_elemt_dual", (gm_d, x_d))):
        assert ops.launch_plan(kind, x, others)["dual"], kind
    want, got = red_composed(), red_dual()
    assert torch.equal(gm_c, gm_d)
    assert all(torch.equal(a, e) for a, e in zip(got, want))
    sums = torch.cat([got[0], got[1], got[4], got[5]])

    def elemt_composed():
        return (
            ops.batch_norm_backward_elemt(gm_c, x, mean, invstd, w,
                                          sums[:C], sums[C:2 * C], count),
            ops.batch_norm_backward_elemt(gm_c, x_d, mean2, invstd2, w2,
                                          sums[2 * C:3 * C], sums[3 * C:],
                                          count),
        )

    def elemt_dual():
        return ops.batch_norm_backward_elemt_dual(
            gm_d, x, x_d, mean, mean2, invstd, invstd2, w, w2, sums, count)

    assert all(torch.equal(a, e)
               for a, e in zip(elemt_dual(), elemt_composed()))

    cases = {
        "elemt composed (2)": (fwd_composed, 5.0),
        "elemt dual": (fwd_dual, 3.0),
        "reduce composed (2)": (red_composed, 6.0),
        "reduce dual": (red_dual, 5.0),
        "bwd elemt composed (2)": (elemt_composed, 6.0),
        "bwd elemt dual": (elemt_dual, 5.0),
    }
    rows = []
    for run in range(runs):
        for name, (fn, units) in cases.items():
            us = bench(fn, iters)
            rows.append({"shape": "x".join(map(str, shape)), "run": run + 1,
                         "kernel": name, "us": round(us, 1),
                         "GBps": round(units * A / (us * 1e-6) / 1e9, 1)})
    return list(cases), rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--json", action="store_true")
    args = p.parse_args()

    all_rows = []
    for shape in SHAPES:
        names, rows = one_shape(shape, args.iters, args.runs)
        all_rows += rows
        if args.json:
            continue
        print(f"shape {'x'.join(map(str, shape))} bf16 channels_last "
              "(bit-equal to the composition: yes)")
        print(f"{'kernels':>24} " + " ".join(f"{'us run' + str(r + 1):>10}"
                                             for r in range(args.runs))
              + "   GB/s (per run)")
        for name in names:
            rs = [r for r in rows if r["kernel"] == name]
            print(f"{name:>24} " + " ".join(f"{r['us']:>10}" for r in rs)
                  + "   " + " / ".join(str(r["GBps"]) for r in rs))
        med = {n: sorted(r["us"] for r in rows if r["kernel"] == n)
               [args.runs // 2] for n in names}
        old = sum(med[n] for n in names[0::2])
        new = sum(med[n] for n in names[1::2])
        print(f"{'five -> three (median)':>24} {old:10.1f} -> {new:10.1f} us"
              f"  ({old - new:+.1f}, {100.0 * (old - new) / old:+.1f}%)")
        sys.stdout.flush()
    if args.json:
        print(json.dumps(all_rows))


if __name__ == "__main__":
    main()
