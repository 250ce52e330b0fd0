#!/usr/bin/env python3
"""Per-layer forward+backward micro-benchmark of the fused BN + LeakyReLU
epilogue at the DCGAN discriminator's three BN stages (batch 128).

    python benchmarks/bench_bn_leaky.py [--iters 10 --rounds 5]

Training-mode BatchNorm (batch statistics, world size 1) followed by
LeakyReLU(0.2), gradients for the input and the affine parameters.  Four
arms, alternated round-robin inside ONE process after every shape has been
warmed (so clocks / allocator state are shared):

    fused     msbn.nn.SyncBatchNormAct2d(relu=True, negative_slope=0.2)
    inplace   the same module with inplace=True: y overwrites x, the
              backward runs from y (always the two-stage kernels; the fused
              arm takes the single-launch small-plane kernels where they
              apply).  Its input is a non-leaf tensor over a fixed buffer
              (no copy is timed), so each iteration normalises the previous
              iteration's output: same bytes, same kernels, other values
    composed  msbn.nn.SyncBatchNorm + nn.LeakyReLU(0.2, inplace=True): what
              the discriminator ran before the leaky epilogue
    torch     torch.nn.BatchNorm2d + nn.LeakyReLU(0.2, inplace=True); fp32
              NCHW only: stock torch-ROCm is known to crash on bf16 +
              channels_last BN on this stack (profiles/r02_kernel_polish.md
              section 6), so that arm is not run for the channels-last rows

Two configurations: fp32 NCHW (the recorded DCGAN configuration) and bf16
channels_last.  Timing is by device events around ``iters`` forward+backward
pairs; every arm gets ``rounds`` such samples and the median / min / max
per-iteration time is reported with the achieved bytes/s against the arm's
own traffic count (see ``traffic_bytes``).  Needs a GPU: no CPU fallback.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn as nn

import msbn

# (N, C, H, W): the discriminator's BN inputs at batch 128, 64x64 images
SHAPES = [(128, 128, 32, 32), (128, 256, 16, 16), (128, 512, 8, 8)]
CONFIGS = [("fp32", torch.float32, False), ("bf16", torch.bfloat16, True)]
ARMS = ["fused", "inplace", "composed", "torch"]
SLOPE = 0.2


def traffic_bytes(numel: int, itemsize: int, arm: str) -> int:
    """Full-tensor traffic of one forward+backward, A = numel*itemsize per
    tensor pass (per-channel vectors and reduction workspaces ignored):

      BN forward     stats read x; normalize read x, write y          3A
      BN backward    reduce read dy, x; elemt read dy, x, write dx    5A
      LeakyReLU      forward read + write (in place)                  2A
                     backward read dy, y; write                       3A

    fused = 8A: the activation rides in the BN normalize / reduce / elemt
    kernels (the gate is recomputed from x).  composed / torch = 13A.
    inplace = 8A as well: stats read x, normalize read x + write y over it
    (3A); reduce read dy, y (2A); elemt read dy, y, write dx (3A).
    """
    a = numel * itemsize
    return (8 if arm in ("fused", "inplace") else 13) * a


class _Fresh(torch.autograd.Function):
    """A non-leaf tensor that requires grad over a fixed buffer, at no
    memory traffic: what an in-place layer may overwrite.  ``knob`` only
    carries requires_grad; the incoming dx is dropped."""

    @staticmethod
    def forward(ctx, knob, buf):
        return buf.detach()

    @staticmethod
    def backward(ctx, grad):
        return torch.zeros((), device=grad.device), None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10,
                   help="forward+backward pairs per timed sample")
    p.add_argument("--rounds", type=int, default=5,
                   help="timed samples per arm (arms alternate each round)")
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_bn_leaky.py needs a GPU (no CPU fallback)")
    assert msbn.ops.hip_available(), "msbn._C (gfx950 HIP extension) missing"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    configs = [(s, c) for c in CONFIGS for s in SHAPES]

    def build(shape, config):
        _, dtype, cl = config
        C = shape[1]
        mods = {
            "fused": msbn.nn.SyncBatchNormAct2d(C, relu=True,
                                                negative_slope=SLOPE),
            "composed": nn.Sequential(msbn.nn.SyncBatchNorm(C),
                                      nn.LeakyReLU(SLOPE, inplace=True)),
        }
        if not cl:
            mods["torch"] = nn.Sequential(nn.BatchNorm2d(C),
                                          nn.LeakyReLU(SLOPE, inplace=True))
        fmt = torch.channels_last if cl else torch.contiguous_format

        def rnd():
            return torch.randn(*shape, device=dev,
                               dtype=dtype).contiguous(memory_format=fmt)

        x = rnd().requires_grad_(True)
        dy = rnd()
        fns = {}
        for arm, m in mods.items():
            m = m.to(dev).train()
            leaves = [x] + list(m.parameters())
            fns[arm] = (lambda m=m, leaves=leaves:
                        torch.autograd.grad(m(x), leaves, dy))
        ip = msbn.nn.SyncBatchNormAct2d(C, relu=True, negative_slope=SLOPE,
                                        inplace=True).to(dev).train()
        buf = rnd()
        knob = torch.zeros((), device=dev, requires_grad=True)
        ip_leaves = [knob] + list(ip.parameters())
        fns["inplace"] = (lambda: torch.autograd.grad(
            ip(_Fresh.apply(knob, buf)), ip_leaves, dy))
        fns = {arm: fns[arm] for arm in ARMS if arm in fns}
        return fns, x.numel(), x.element_size()

    # warm every shape / config / arm before any timing
    for cfg in configs:
        fns, _, _ = build(*cfg)
        for arm in fns:
            for _ in range(args.warmup):
                fns[arm]()
        del fns
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    rows = []
    for shape, config in configs:
        fns, numel, itemsize = build(shape, config)
        for arm in fns:
            fns[arm]()
        torch.cuda.synchronize()
        samples = {arm: [] for arm in fns}
        for _ in range(args.rounds):
            for arm in fns:
                start = torch.cuda.Event(enable_timing=True)
                stop = torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.iters):
                    fns[arm]()
                stop.record()
                stop.synchronize()
                samples[arm].append(start.elapsed_time(stop) / args.iters)
        for arm in fns:
            med = statistics.median(samples[arm])
            nbytes = traffic_bytes(numel, itemsize, arm)
            row = {
                "shape": "x".join(str(s) for s in shape),
                "dtype": config[0],
                "layout": "channels_last" if config[2] else "nchw",
                "arm": arm,
                "ms": round(med, 4),
                "ms_min": round(min(samples[arm]), 4),
                "ms_max": round(max(samples[arm]), 4),
                "bytes": nbytes,
                "GBps": round(nbytes / (med * 1e-3) / 1e9, 1),
                "timed_iters": args.iters * args.rounds,
            }
            rows.append(row)
            print(json.dumps(row), flush=True)
        del fns
        torch.cuda.empty_cache()

    def total(arm, dtype):
        return round(sum(r["ms"] for r in rows
                         if r["arm"] == arm and r["dtype"] == dtype), 4)

    print(json.dumps({
        "metric": "BN+LeakyReLU(0.2) fwd+bwd, sum of per-layer medians over "
                  "the three discriminator stages",
        "unit": "ms",
        "fp32_nchw": {a: total(a, "fp32") for a in ARMS},
        "bf16_channels_last": {a: total(a, "bf16") for a in ARMS[:3]},
    }))


if __name__ == "__main__":
    main()
