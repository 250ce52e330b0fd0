"""bn_silu_se (squeeze-excite fused into the depthwise BN+SiLU layer) against
the composition se(bn(y)), on one GPU.

Per site: every distinct (side, C, Cr) at which mbconv_net's defaults with
se_ratio=0.25 apply an SE block at 224x224 input, bf16 channels-last, forward
+ backward of the layer from a given y and output gradient.  Both sides run in
one process, alternating, timed with device events around blocks of calls
after a warm-up (bench_dwconv_stats._time_blocks: median and range).  Bytes
are shape-derived: from a given y the fused route moves 9A (one statistics
pass, 3 forward, 5 backward), A = N*H*W*C elements of 2 bytes; the rate is
given against the 6.3 TB/s ceiling.

End to end: mbconv_net(kernel_sizes=(3, 3, 5, 3, 5, 5), se_ratio=0.25,
conv_stats=True, dw_grad=True) (bf16, channels-last, fused SGD) with the SE
route on and forced off, alternating blocks of steps.

    python benchmarks/bench_se.py [--batch-size 128] [--skip-e2e]

Prints one JSON line per measurement.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dwconv_stats import _time_blocks  # noqa: E402  (sets the db)

import torch  # noqa: E402

import msbn  # noqa: E402
from msbn.nn import SqueezeExcite  # noqa: E402
from msbn.nn import fused  # noqa: E402

# (output side of the depthwise conv, C = 4 * cin, Cr = cin / 4)
SITES = [(112, 64, 4), (56, 64, 4), (56, 96, 6), (28, 96, 6), (28, 160, 10),
         (14, 160, 10), (14, 320, 20), (7, 320, 20), (7, 448, 28),
         (4, 448, 28), (4, 768, 48)]
B0_KERNELS = (3, 3, 5, 3, 5, 5)
CEILING = 6.3e12


def _r(t):
    med, lo, hi = t
    return {"ms": round(med, 4), "range": [round(lo, 4), round(hi, 4)]}


def per_site(batch, iters, repeats):
    dev = torch.device("cuda:0")
    for side, c, cr in SITES:
        y = torch.randn(batch, c, side, side, device=dev,
                        dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gout = torch.randn_like(y)
        bn = fused.SyncBatchNormAct2d(c, act="silu").to(dev)
        se = SqueezeExcite(c, cr).to(dev, torch.bfloat16)
        assert fused.bn_silu_se_eligible(bn, se, y)

        def run(fn):
            def step():
                y.grad = None
                fn().backward(gout)
            return step

        fns = [run(lambda: fused.bn_silu_se(bn, se, y)),
               run(lambda: se(bn(y)))]
        for fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ours, comp = _time_blocks(fns, iters, repeats)
        a_bytes = y.numel() * 2
        print(json.dumps({
            "kind": "site", "side": side, "C": c, "Cr": cr, "batch": batch,
            "fused": _r(ours), "composition": _r(comp),
            "fused_over_composition": round(ours[0] / comp[0], 3),
            "fused_tb_s": round(9 * a_bytes / (ours[0] * 1e-3) / 1e12, 3),
            "fraction_of_ceiling": round(
                9 * a_bytes / (ours[0] * 1e-3) / CEILING, 3),
        }), flush=True)


def end_to_end(batch, steps, repeats):
    import bench  # the flagship's own bf16 cast

    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = msbn.models.mbconv_net(kernel_sizes=B0_KERNELS, se_ratio=0.25,
                                   conv_stats=True, dw_grad=True)
    model = bench.cast_bf16_keep_bn_fp32(model.to(dev)) \
        .to(memory_format=torch.channels_last).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                          weight_decay=1e-4, fused=True)
    x = torch.randn(batch, 3, 224, 224, device=dev, dtype=torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    t = torch.randint(0, 1000, (batch,), device=dev)
    loss_fn = torch.nn.CrossEntropyLoss()
    eligible = fused.bn_silu_se_eligible

    def stepper(route_on):
        def step():
            # forced off: every SE site then runs the composition
            fused.bn_silu_se_eligible = eligible if route_on else \
                (lambda *a: False)
            opt.zero_grad(set_to_none=True)
            loss_fn(model(x).float(), t).backward()
            opt.step()
            fused.bn_silu_se_eligible = eligible
        return step

    fns = [stepper(False), stepper(True)]
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    off, on = _time_blocks(fns, steps, repeats)
    print(json.dumps({
        "kind": "end_to_end", "batch": batch, "steps_per_block": steps,
        "repeats": repeats, "off": _r(off), "on": _r(on),
        "on_minus_off_ms": round(on[0] - off[0], 3),
    }), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--skip-sites", action="store_true")
    p.add_argument("--skip-e2e", action="store_true")
    args = p.parse_args()
    if not args.skip_sites:
        per_site(args.batch_size, args.iters, args.repeats)
    if not args.skip_e2e:
        end_to_end(args.batch_size, args.steps, args.repeats)


if __name__ == "__main__":
    main()
