#!/usr/bin/env python3
"""The two RetinaNet heads alone, per-level loop against grouped BN, one GPU.

Inputs: the five FPN levels of the benchmark shape (2 x 3 x 800 x 1333 padded
to 800 x 1344: 100x168, 50x84, 25x42, 13x21, 7x11 at C = 256), bf16
channels-last, BatchNorm parameters fp32.  One step is forward plus backward
of both heads.
  loop    : Head(grouped=False) applied level by level (the parent route)
  grouped : Head(grouped=True), the same weights, layer-major
Both sides run in one process in alternating blocks after a warm-up per side;
the median and the min..max of the repeats are printed, with the kernel
launches of one step counted by the profiler.  Collectives per step are
stated from the structure (a one-GPU run issues none): 8 BatchNorm layers x 5
levels x 2 directions against 8 x 2.

    python benchmarks/bench_grouped_heads.py [--iters 10 --repeats 7]

Prints one JSON line per side and one for the comparison.
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

import msbn  # noqa: E402
from msbn.models.retinanet import Head  # noqa: E402
from msbn.nn.batchnorm import _NormBase  # noqa: E402

PLANES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def build(grouped, dev):
    torch.manual_seed(3)
    heads = torch.nn.ModuleList([Head(256, 80, grouped=grouped),
                                 Head(256, 4, grouped=grouped)])
    heads = msbn.convert_sync_batchnorm(heads).to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last).train()
    for m in heads.modules():
        if isinstance(m, _NormBase):
            m.float()
    return heads


def make_step(heads, feats, grouped):
    def step():
        for f in feats:
            f.grad = None
        for p in heads.parameters():
            p.grad = None
        loss = 0.0
        for head in heads:
            outs = head(feats) if grouped else [head(f) for f in feats]
            for o in outs:
                loss = loss + o.float().square().mean()
        loss.backward()
    return step


def count_launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events()
                   if str(e.device_type).endswith("CUDA")
                   and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:  # the count is a by-product, the timing is not
        print(f"[bench_grouped_heads] launch count unavailable: {e!r}",
              file=sys.stderr)
        return None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    feats = [torch.randn((2, 256, h, w), generator=g, device=dev)
             .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
             .requires_grad_(True) for h, w in PLANES]
    loop, grouped = build(False, dev), build(True, dev)
    grouped.load_state_dict(loop.state_dict())
    steps = {"loop": make_step(loop, feats, False),
             "grouped": make_step(grouped, feats, True)}
    for step in steps.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(args.repeats):
        for name, step in steps.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                step()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / args.iters)
    out = {}
    for name, step in steps.items():
        t = times[name]
        out[name] = {"side": name, "ms_per_step": round(statistics.median(t), 4),
                     "min": round(min(t), 4), "max": round(max(t), 4),
                     "kernel_launches_per_step": count_launches(step),
                     "collectives_per_step_multi_gpu":
                         80 if name == "loop" else 16}
        print(json.dumps(out[name]))
    print(json.dumps({
        "metric": "two RetinaNet heads fwd+bwd, loop / grouped",
        "ratio_of_medians": round(out["loop"]["ms_per_step"]
                                  / out["grouped"]["ms_per_step"], 4),
        "ranges_overlap": not (out["grouped"]["max"] < out["loop"]["min"]
                               or out["loop"]["max"] < out["grouped"]["min"]),
        "iters": args.iters, "repeats": args.repeats,
    }))


if __name__ == "__main__":
    main()
