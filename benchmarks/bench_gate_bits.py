#!/usr/bin/env python3
"""Gate bits, kernel by kernel, at the closing-BN shapes of the ResNet-50
benchmark (bf16 channels-last, batch 512): the bit-storing forward next to
the plain one, and the fork-folding backward reduce that reads the bits next
to the one that reads the residual.  hipEvent timing, alternated runs.

    python benchmarks/bench_gate_bits.py [--iters 30] [--runs 3] [--json]

Before timing, every shape checks that the gate route reproduces the residual
route bit for bit (y, gm, both sums, both affine gradients).

Achieved GB/s is (bytes the kernel must move) / time with A the bytes of one
activation tensor: 3A / 3.0625A for the forward without / with the bit store,
5A / 4.0625A for the reduce with the residual / with the bits (the traffic
table of docs/KERNEL_DESIGN.md "Gate bits").
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from msbn import ops

SHAPES = [
    (512, 64, 112, 112),
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

    def rand():
        return torch.randn(N, C, H, W, device=dev, dtype=dt).to(
            memory_format=cl)

    x, res, dy1, dy2 = rand(), rand(), rand(), rand()
    w = torch.randn(C, device=dev).abs() + 0.1
    b = torch.randn(C, device=dev)
    mean, invstd = ops.batch_norm_stats(x, 1e-5)
    coefs = ops.bn_make_coefs(mean, invstd, w, b)
    A = x.numel() * x.element_size()
    bits = ops.gate_bits_empty(x)
    gm_r, gm_g = torch.empty_like(x), torch.empty_like(x)

    def fwd():
        return ops.batch_norm_elemt_act(x, res, w, b, mean, invstd, True,
                                        coefs)

    def fwd_gate():
        return ops.batch_norm_elemt_act(x, res, w, b, mean, invstd, True,
                                        coefs, 0.0, bits)

    def red_res():
        return ops.batch_norm_backward_reduce_act(
            dy1, x, res, mean, invstd, w, b, True, True, True, True, coefs,
            gm_r, 0.0, dy2)

    def red_gate():
        return ops.batch_norm_backward_reduce_act(
            dy1, x, None, mean, invstd, w, b, True, True, True, True, coefs,
            gm_g, 0.0, dy2, gate=bits)

    y = fwd()
    y_g, wrote = fwd_gate()
    assert wrote is bits, "the forward declined to store the bits"
    assert torch.equal(y, y_g)
    assert ops.launch_plan("bwd_reduce", x,
                           (dy1, None, gm_g, dy2, bits))["gate"]
    want, got = red_res(), red_gate()
    assert torch.equal(gm_r, gm_g)
    assert all(torch.equal(a, e) for a, e in zip(got, want))

    cases = {
        "elemt relu,RES": (fwd, 3.0),
        "elemt relu,RES +bits": (fwd_gate, 3.0625),
        "reduce RES,GM,DY2": (red_res, 5.0),
        "reduce GATE,GM,DY2": (red_gate, 4.0625),
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
              "(bit-equal to the residual route: yes)")
        print(f"{'kernel':>22} " + " ".join(f"{'us run' + str(r + 1):>10}"
                                            for r in range(args.runs))
              + "   GB/s (per run)")
        for name in names:
            rs = [r for r in rows if r["kernel"] == name]
            print(f"{name:>22} " + " ".join(f"{r['us']:>10}" for r in rs)
                  + "   " + " / ".join(str(r["GBps"]) for r in rs))
        med = {n: sorted(r["us"] for r in rows if r["kernel"] == n)
               [len(rows) // len(names) // 2] for n in names}
        pair_old = med[names[0]] + med[names[2]]
        pair_new = med[names[1]] + med[names[3]]
        print(f"{'pair (median)':>22} {pair_old:10.1f} -> {pair_new:10.1f} us"
              f"  ({pair_old - pair_new:+.1f})")
    if args.json:
        print(json.dumps(all_rows))


if __name__ == "__main__":
    main()
