"""conv1x1_stats against the route it replaces, on one GPU.

Per layer: the distinct (M, Cin, Cout) of ResNet-50's 33 1x1 stride-1
conv -> BatchNorm sites at the flagship batch, bf16 channels-last.
  fused  : ops.conv1x1_stats + batch_norm_stats_local_from_partials
  parent : the stock convolution (MIOpen, the shipped find-db) +
           batch_norm_stats_local
Both sides are timed in one process, alternating, with device events around
blocks of launches after a warm-up per shape.  The fused kernel's achieved
bytes/s uses the shape-derived byte count 2*M*(Cin + Cout).

End to end: the flagship configuration (ResNet-50, bf16, channels-last, fused
SGD, as bench.py builds it) with conv_stats off and on, alternating blocks of
steps; the spread of the repeats is printed next to the difference.

    python benchmarks/bench_conv_stats.py [--batch-size 512] [--skip-e2e]

Prints one JSON line per measurement.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_db = os.path.join(ROOT, "miopen_db")
if os.path.isdir(_db) and os.listdir(_db):
    os.environ.setdefault("MIOPEN_USER_DB_PATH", _db)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import msbn  # noqa: E402
from msbn import ops  # noqa: E402

# (spatial side, Cin, Cout, number of sites)
SITES = [
    (56, 64, 64, 1), (56, 64, 256, 4), (56, 256, 64, 2), (56, 256, 128, 1),
    (28, 128, 512, 4), (28, 512, 128, 3), (28, 512, 256, 1),
    (14, 256, 1024, 6), (14, 1024, 256, 5), (14, 1024, 512, 1),
    (7, 512, 2048, 3), (7, 2048, 512, 2),
]
EPS = 1e-5


def _time_blocks(fns, iters, repeats):
    """Median and spread (ms per call) of each fn, blocks alternating."""
    times = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            stop.synchronize()
            times[i].append(start.elapsed_time(stop) / iters)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def per_layer(batch, iters, repeats):
    dev = torch.device("cuda:0")
    for side, cin, cout, sites in SITES:
        x = torch.randn(batch, cin, side, side, device=dev,
                        dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cout, cin, 1, 1, device=dev) / cin ** 0.5) \
            .to(torch.bfloat16)
        gamma = torch.ones(cout, device=dev)
        beta = torch.zeros(cout, device=dev)
        rm = torch.zeros(cout, device=dev)
        rv = torch.ones(cout, device=dev)
        rows = x.numel() // cin
        hip = ops._require_hip()

        def fused():
            _, partials, nchunks = ops.conv1x1_stats(x, w)
            ops.batch_norm_stats_local_from_partials(
                partials, nchunks, rows, EPS, rm, rv, 0.1, gamma, beta, True)

        def conv_only():
            ops.conv1x1_stats(x, w)

        def parent():
            y = F.conv2d(x, w)
            hip.batch_norm_stats_local(y, EPS, rm, rv, 0.1, gamma, beta, True)

        for fn in (fused, parent, fused, parent):  # warm-up per shape
            fn()
        torch.cuda.synchronize()
        (f, fmin, fmax), (p, pmin, pmax), (k, _, _) = _time_blocks(
            [fused, parent, conv_only], iters, repeats)
        plan = ops.launch_plan("conv1x1_stats", x, (w,))
        print(json.dumps({
            "kind": "layer", "rows": rows, "cin": cin, "cout": cout,
            "sites": sites, "fused_ms": round(f, 4),
            "fused_ms_range": [round(fmin, 4), round(fmax, 4)],
            "parent_ms": round(p, 4),
            "parent_ms_range": [round(pmin, 4), round(pmax, 4)],
            "kernel_ms": round(k, 4),
            "kernel_tb_per_s": round(2 * rows * (cin + cout) / k / 1e9, 3),
            "slab": plan["slab"], "nslabs": plan["nslabs"],
            "nchunks": plan["nchunks"],
            "tiles_per_block": plan["tiles_per_block"],
        }), flush=True)
        del x, w


def end_to_end(batch, steps, repeats):
    sys.path.insert(0, ROOT)
    import bench  # the flagship's own model construction

    dev = torch.device("cuda:0")
    runs = []
    for conv_stats in (False, True):
        torch.manual_seed(1234)
        model = msbn.models.resnet50(fused=True, conv_stats=conv_stats)
        model = bench.cast_bf16_keep_bn_fp32(model.to(dev)) \
            .to(memory_format=torch.channels_last)
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                              weight_decay=1e-4, fused=True)
        runs.append((model, opt))
    x = torch.randn(batch, 3, 224, 224, device=dev, dtype=torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (batch,), device=dev)
    loss_fn = torch.nn.CrossEntropyLoss()

    def stepper(model, opt):
        def step():
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(model(x).float(), y)
            loss.backward()
            opt.step()
        return step

    fns = [stepper(*r) for r in runs]
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    (off, offmin, offmax), (on, onmin, onmax) = _time_blocks(
        fns, steps, repeats)
    print(json.dumps({
        "kind": "end_to_end", "batch": batch, "steps_per_block": steps,
        "repeats": repeats, "off_ms": round(off, 3),
        "off_ms_range": [round(offmin, 3), round(offmax, 3)],
        "on_ms": round(on, 3), "on_ms_range": [round(onmin, 3),
                                               round(onmax, 3)],
        "on_minus_off_ms": round(on - off, 3),
    }), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch-size", type=int, default=512)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--skip-layers", action="store_true")
    p.add_argument("--skip-e2e", action="store_true")
    args = p.parse_args()
    if not args.skip_layers:
        per_layer(args.batch_size, args.iters, args.repeats)
    if not args.skip_e2e:
        end_to_end(args.batch_size, args.steps, args.repeats)


if __name__ == "__main__":
    main()
