"""dwconv3x3_stats against the route it replaces, on one GPU.

Per layer: the 3x3 depthwise conv -> BatchNorm sites of an EfficientNet-B0
like net (224x224 input, expansion 6) at a training batch, bf16
channels-last, both strides.
  fused  : ops.dwconv3x3_stats + batch_norm_stats_local_from_partials
  parent : the stock grouped convolution (MIOpen, the shipped find-db) +
           batch_norm_stats_local
Both sides are timed in one process, alternating, with device events around
blocks of launches after a warm-up per shape.  The fused kernel's achieved
bytes/s uses the shape-derived byte count 2*(N*H*W*C + N*OH*OW*C).

End to end: mbconv_net (bf16, channels-last, fused SGD) with conv_stats off
and on, alternating blocks of steps; the spread of the repeats is printed
next to the difference.

    python benchmarks/bench_dwconv_stats.py [--batch-size 128] [--skip-e2e]

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

# (input side, C, stride, number of sites)
SITES = [
    (112, 32, 1, 1), (112, 96, 2, 1), (56, 144, 1, 1), (56, 144, 2, 1),
    (28, 240, 1, 1), (28, 240, 2, 1), (14, 480, 1, 2), (14, 672, 1, 1),
    (14, 672, 2, 1), (7, 1152, 1, 1),
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
    hip = ops._require_hip()
    for side, c, stride, sites in SITES:
        x = torch.randn(batch, c, side, side, device=dev,
                        dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(c, 1, 3, 3, device=dev) / 3).to(torch.bfloat16)
        gamma = torch.ones(c, device=dev)
        beta = torch.zeros(c, device=dev)
        rm = torch.zeros(c, device=dev)
        rv = torch.ones(c, device=dev)
        oside = (side - 1) // stride + 1
        count = batch * oside * oside

        def fused():
            _, partials, nchunks = ops.dwconv3x3_stats(x, w, stride)
            ops.batch_norm_stats_local_from_partials(
                partials, nchunks, count, EPS, rm, rv, 0.1, gamma, beta, True)

        def conv_only():
            ops.dwconv3x3_stats(x, w, stride)

        def parent():
            y = F.conv2d(x, w, stride=stride, padding=1, groups=c)
            hip.batch_norm_stats_local(y, EPS, rm, rv, 0.1, gamma, beta, True)

        def parent_conv_only():
            F.conv2d(x, w, stride=stride, padding=1, groups=c)

        for fn in (fused, parent, fused, parent):  # warm-up per shape
            fn()
        torch.cuda.synchronize()
        (f, fmin, fmax), (p, pmin, pmax), (k, _, _), (pc, _, _) = \
            _time_blocks([fused, parent, conv_only, parent_conv_only],
                         iters, repeats)
        kind = "dwconv3x3_stats" if stride == 1 else "dwconv3x3s2_stats"
        plan = ops.launch_plan(kind, x, (w,))
        nbytes = 2 * (x.numel() + count * c)
        print(json.dumps({
            "kind": "layer", "side": side, "c": c, "stride": stride,
            "sites": sites, "fused_ms": round(f, 4),
            "fused_ms_range": [round(fmin, 4), round(fmax, 4)],
            "parent_ms": round(p, 4),
            "parent_ms_range": [round(pmin, 4), round(pmax, 4)],
            "kernel_ms": round(k, 4),
            "kernel_tb_per_s": round(nbytes / k / 1e9, 3),
            "parent_conv_ms": round(pc, 4),
            "lpr": plan["lpr"], "ctiles": plan["ctiles"],
            "nchunks": plan["nchunks"], "trips": plan["trips"],
        }), flush=True)
        del x, w


def end_to_end(batch, steps, repeats):
    import bench  # the flagship's own bf16 cast

    dev = torch.device("cuda:0")
    runs = []
    for conv_stats in (False, True):
        torch.manual_seed(1234)
        model = msbn.models.mbconv_net(conv_stats=conv_stats)
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
    p.add_argument("--batch-size", type=int, default=128)
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
