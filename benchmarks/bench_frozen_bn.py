#!/usr/bin/env python3
"""Per-layer forward+backward micro-benchmark of the frozen-BN path at the
RetinaNet-R50 backbone's real activation shapes (batch 2 at 800x1344, bf16).

    python benchmarks/bench_frozen_bn.py [--iters 10 --rounds 5]

Three arms, alternated round-robin inside ONE process after every shape has
been warmed (so clocks / allocator state are shared):

    frozen    msbn.nn.FrozenBatchNorm2d (coefs kernel + one elemt launch
              forward, one elementwise kernel backward)
    composed  the eager differentiable expression the GPU eval path used
              before the frozen kernels (MSBN_FROZEN_COMPOSED=1)
    torch     torch.nn.BatchNorm2d.eval() with frozen affine (+ add + relu);
              NCHW only: stock torch-ROCm is known to crash on bf16 +
              channels_last at detection shapes on this stack
              (profiles/r02_kernel_polish.md section 6), so that arm is not
              run for the channels-last rows

Timing is by device events around ``iters`` forward+backward pairs; every
arm gets ``rounds`` such samples (>= 50 timed iterations per arm by default)
and the median / min / max per-iteration time is reported together with the
achieved bytes/s against the MINIMAL traffic of the layer (see
``minimal_bytes``).  Needs a GPU: there is no CPU fallback.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import msbn
from msbn.nn.batchnorm import _composed_running_stats_forward

# (C, H, W) of every distinct BN input in the R50 backbone, batch 2 at 800x1344
SHAPES = [
    (64, 400, 672),
    (64, 200, 336), (256, 200, 336),
    (128, 100, 168), (512, 100, 168),
    (256, 50, 84), (1024, 50, 84),
    (512, 25, 42), (2048, 25, 42),
]
VARIANTS = ["bn", "bn+relu", "bn+add+relu"]
ARMS = ["frozen", "composed", "torch"]


def minimal_bytes(numel: int, itemsize: int, variant: str) -> int:
    """Bytes a forward+backward of the layer must move at the very least,
    A = numel*itemsize per full tensor (per-channel vectors ignored):

      forward   read x (+ residual), write y              2A / 2A / 3A
      backward  bn          read dy, write dx             2A
                bn+relu     + read x for the gate         3A
                bn+add+relu + read residual, write dres   5A
    """
    a = numel * itemsize
    fwd = {"bn": 2, "bn+relu": 2, "bn+add+relu": 3}[variant]
    bwd = {"bn": 2, "bn+relu": 3, "bn+add+relu": 5}[variant]
    return (fwd + bwd) * a


def make_arm(arm, variant, frozen, stock):
    relu = variant != "bn"

    if arm == "frozen":
        def fwd(x, res):
            return frozen(x, res)
    elif arm == "composed":
        def fwd(x, res):
            return _composed_running_stats_forward(
                x, res, frozen.weight, frozen.bias, frozen.running_mean,
                frozen.running_var, frozen.eps, relu)
    else:
        def fwd(x, res):
            y = stock(x)
            if res is not None:
                y = y + res
            return torch.relu(y) if relu else y
    return fwd


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch-size", type=int, default=2)
    p.add_argument("--iters", type=int, default=10,
                   help="forward+backward pairs per timed sample")
    p.add_argument("--rounds", type=int, default=5,
                   help="timed samples per arm (arms alternate each round)")
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_frozen_bn.py needs a GPU (no CPU fallback)")
    assert msbn.ops.hip_available(), "msbn._C (gfx950 HIP extension) missing"
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    torch.manual_seed(0)

    configs = []
    for C, H, W in SHAPES:
        for cl in (False, True):
            for variant in VARIANTS:
                configs.append((C, H, W, cl, variant))

    def build(C, H, W, cl, variant):
        relu = variant != "bn"
        frozen = msbn.nn.FrozenBatchNorm2d(C, relu=relu).to(dev)
        frozen.weight.uniform_(0.5, 1.5)
        frozen.bias.normal_()
        frozen.running_mean.normal_()
        frozen.running_var.uniform_(0.5, 1.5)
        stock = torch.nn.BatchNorm2d(C).to(dev).eval()
        stock.load_state_dict(frozen.state_dict())
        stock.requires_grad_(False)
        fmt = torch.channels_last if cl else torch.contiguous_format

        def rnd():
            return torch.randn(args.batch_size, C, H, W, device=dev,
                               dtype=dtype).contiguous(memory_format=fmt)

        x = rnd().requires_grad_(True)
        res = rnd().requires_grad_(True) if variant == "bn+add+relu" else None
        dy = rnd()
        leaves = [x] + ([res] if res is not None else [])
        fns = {}
        for arm in (ARMS[:2] if cl else ARMS):
            f = make_arm(arm, variant, frozen, stock)
            fns[arm] = (lambda f=f: torch.autograd.grad(f(x, res), leaves, dy))
        return fns, x.numel()

    # warm every shape / variant / arm before any timing
    for cfg in configs:
        fns, _ = build(*cfg)
        for arm in fns:
            for _ in range(args.warmup):
                fns[arm]()
        del fns
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    rows = []
    for cfg in configs:
        C, H, W, cl, variant = cfg
        fns, numel = build(*cfg)
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
        nbytes = minimal_bytes(numel, 2, variant)
        for arm in fns:
            med = statistics.median(samples[arm])
            row = {
                "shape": f"{args.batch_size}x{C}x{H}x{W}",
                "layout": "channels_last" if cl else "nchw",
                "variant": variant,
                "arm": arm,
                "ms": round(med, 4),
                "ms_min": round(min(samples[arm]), 4),
                "ms_max": round(max(samples[arm]), 4),
                "min_bytes": nbytes,
                "GBps": round(nbytes / (med * 1e-3) / 1e9, 1),
                "timed_iters": args.iters * args.rounds,
            }
            rows.append(row)
            print(json.dumps(row), flush=True)
        del fns
        torch.cuda.empty_cache()

    def total(arm, layout=None):
        return sum(r["ms"] for r in rows if r["arm"] == arm
                   and layout in (None, r["layout"]))

    print(json.dumps({
        "metric": "frozen-BN fwd+bwd, sum of per-layer medians over all "
                  "shapes/layouts/variants",
        "unit": "ms",
        "dtype": "bf16",
        "frozen": round(total("frozen"), 3),
        "composed": round(total("composed"), 3),
        "frozen_nchw": round(total("frozen", "nchw"), 3),
        "composed_nchw": round(total("composed", "nchw"), 3),
        "torch_nchw": round(total("torch", "nchw"), 3),
    }))


if __name__ == "__main__":
    main()
