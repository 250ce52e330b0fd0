"""ops.dwconv3x3_backward against the route it replaces, on one GPU.

Per layer: the 3x3 depthwise conv sites of an EfficientNet-B0 like net
(224x224 input, expansion 6) at a training batch, bf16 channels-last, both
strides (the SITES of bench_dwconv_stats.py).
  ours   : ops.dwconv3x3_backward
  parent : aten.convolution_backward with groups = C (MIOpen, the shipped
           find-db), the stock route at the same commit
Both gradients together, and each one alone.  Both sides are timed in one
process, alternating, with device events around blocks of launches after a
warm-up per shape.  Achieved bytes/s use shape-derived byte counts: with
X = N*H*W*C and A = N*OH*OW*C elements of 2 bytes, dgrad moves A + X (reads
dy, writes dx) and wgrad A + X (reads dy and x).

End to end: mbconv_net(conv_stats=True) (bf16, channels-last, fused SGD) with
dw_grad off and on, alternating blocks of steps; the spread of the repeats is
printed next to the difference.

    python benchmarks/bench_dwconv_grad.py [--batch-size 128] [--skip-e2e]

Prints one JSON line per measurement.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dwconv_stats import SITES, _time_blocks  # noqa: E402  (sets the db)

import torch  # noqa: E402

import msbn  # noqa: E402
from msbn import ops  # noqa: E402


def _r(t):
    med, lo, hi = t
    return {"ms": round(med, 4), "range": [round(lo, 4), round(hi, 4)]}


def per_layer(batch, iters, repeats):
    dev = torch.device("cuda:0")
    for side, c, stride, sites in SITES:
        x = torch.randn(batch, c, side, side, device=dev,
                        dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(c, 1, 3, 3, device=dev) / 3).to(torch.bfloat16)
        oside = (side - 1) // stride + 1
        gy = torch.randn(batch, c, oside, oside, device=dev,
                         dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)

        def ours(dx, dw):
            return lambda: ops.dwconv3x3_backward(gy, x, w, stride, dx, dw)

        def parent(dx, dw):
            return lambda: torch.ops.aten.convolution_backward(
                gy, x, w, None, [stride] * 2, [1, 1], [1, 1], False, [0, 0],
                c, [dx, dw, False])

        masks = [(True, True), (True, False), (False, True)]
        fns = [f(*m) for m in masks for f in (ours, parent)]
        assert ours(True, True)()[0] is not None
        for fn in fns + fns:  # warm-up per shape
            fn()
        torch.cuda.synchronize()
        t = _time_blocks(fns, iters, repeats)
        nbytes = 2 * (x.numel() + gy.numel())
        kinds = ("dwconv3x3_dgrad", "dwconv3x3_wgrad") if stride == 1 else \
            ("dwconv3x3s2_dgrad", "dwconv3x3s2_wgrad")
        pd, pw = (ops.launch_plan(k, x, (w, gy)) for k in kinds)
        print(json.dumps({
            "kind": "layer", "side": side, "c": c, "stride": stride,
            "sites": sites,
            "both_ours": _r(t[0]), "both_parent": _r(t[1]),
            "dgrad_ours": _r(t[2]), "dgrad_parent": _r(t[3]),
            "wgrad_ours": _r(t[4]), "wgrad_parent": _r(t[5]),
            "dgrad_tb_per_s": round(nbytes / t[2][0] / 1e9, 3),
            "wgrad_tb_per_s": round(nbytes / t[4][0] / 1e9, 3),
            "lpr": pd["lpr"], "ctiles": pd["ctiles"],
            "dgrad_nchunks": pd["nchunks"], "dgrad_trips": pd["trips"],
            "wgrad_nchunks": pw["nchunks"], "wgrad_trips": pw["trips"],
        }), flush=True)
        del x, w, gy


def end_to_end(batch, steps, repeats):
    import bench  # the flagship's own bf16 cast

    dev = torch.device("cuda:0")
    runs = []
    for dw_grad in (False, True):
        torch.manual_seed(1234)
        model = msbn.models.mbconv_net(conv_stats=True, dw_grad=dw_grad)
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
    off, on = _time_blocks(fns, steps, repeats)
    print(json.dumps({
        "kind": "end_to_end", "batch": batch, "steps_per_block": steps,
        "repeats": repeats, "off": _r(off), "on": _r(on),
        "on_minus_off_ms": round(on[0] - off[0], 3),
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
