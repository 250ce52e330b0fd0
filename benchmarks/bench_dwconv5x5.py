"""ops.dwconv5x5_stats / ops.dwconv5x5_backward against the routes they
replace, on one GPU.

Per layer: the 5x5 depthwise conv sites of EfficientNet-B0 (224x224 input,
expansion 6) at a training batch, bf16 channels-last.
  forward ours   : ops.dwconv5x5_stats + batch_norm_stats_local_from_partials
  forward parent : F.conv2d(groups=C) + ops.batch_norm_stats_local
  dgrad / wgrad  : ops.dwconv5x5_backward against aten.convolution_backward
                   with groups = C, one gradient at a time
Both sides are timed in one process, alternating, with device events around
blocks of launches after a warm-up per shape (bench_dwconv_stats._time_blocks:
median and range).  Achieved bytes/s use shape-derived byte counts, X =
N*H*W*C and A = N*OH*OW*C elements of 2 bytes: X + A for each kernel.  The FMA
rate is 25 (forward, dgrad at stride 1, wgrad) FMAs per output element; the
stride-2 dgrad issues 25/4 per dx element.

End to end: mbconv_net(kernel_sizes=(3, 3, 5, 3, 5, 5)) (bf16, channels-last,
fused SGD) with conv_stats / dw_grad off and on, alternating blocks of steps.

    python benchmarks/bench_dwconv5x5.py [--batch-size 128] [--skip-e2e]

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
import torch.nn.functional as F  # noqa: E402

import msbn  # noqa: E402
from msbn import ops  # noqa: E402

# (input side, C, stride): B0's 5x5 blocks
SITES = [(28, 240, 1), (28, 240, 2), (14, 672, 1), (14, 672, 2), (7, 1152, 1)]
B0_KERNELS = (3, 3, 5, 3, 5, 5)


def _r(t):
    med, lo, hi = t
    return {"ms": round(med, 4), "range": [round(lo, 4), round(hi, 4)]}


def per_layer(batch, iters, repeats):
    dev = torch.device("cuda:0")
    for side, c, stride in SITES:
        x = torch.randn(batch, c, side, side, device=dev,
                        dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(c, 1, 5, 5, device=dev) / 5).to(torch.bfloat16)
        oside = (side - 1) // stride + 1
        gy = torch.randn(batch, c, oside, oside, device=dev,
                         dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        count = batch * oside * oside
        gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        hip = ops._require_hip()

        def fwd_ours():
            _, partials, nchunks = ops.dwconv5x5_stats(x, w, stride)
            ops.batch_norm_stats_local_from_partials(
                partials, nchunks, count, 1e-5, rm, rv, 0.1, gamma, beta, True)

        def fwd_parent():
            y = F.conv2d(x, w, stride=stride, padding=2, groups=c)
            hip.batch_norm_stats_local(y, 1e-5, rm, rv, 0.1, gamma, beta, True)

        def ours(dx, dw):
            return lambda: ops.dwconv5x5_backward(gy, x, w, stride, dx, dw)

        def parent(dx, dw):
            return lambda: torch.ops.aten.convolution_backward(
                gy, x, w, None, [stride] * 2, [2, 2], [1, 1], False, [0, 0],
                c, [dx, dw, False])

        fns = [fwd_ours, fwd_parent, ours(True, False), parent(True, False),
               ours(False, True), parent(False, True)]
        assert ops.dwconv5x5_stats(x, w, stride)[0] is not None
        for fn in fns + fns:  # warm-up per shape
            fn()
        torch.cuda.synchronize()
        t = _time_blocks(fns, iters, repeats)
        nbytes = 2 * (x.numel() + gy.numel())
        fma = 25 * gy.numel()
        rec = {"kind": "layer", "side": side, "c": c, "stride": stride}
        for i, name in enumerate(("fwd", "dgrad", "wgrad")):
            rec[name + "_ours"] = _r(t[2 * i])
            rec[name + "_parent"] = _r(t[2 * i + 1])
            rec[name + "_tb_per_s"] = round(nbytes / t[2 * i][0] / 1e9, 3)
            rec[name + "_tfma_per_s"] = round(fma / t[2 * i][0] / 1e9, 3)
        plan = ops.launch_plan(
            "dwconv5x5_stats" if stride == 1 else "dwconv5x5s2_stats", x, (w,))
        rec.update(lpr=plan["lpr"], ctiles=plan["ctiles"],
                   tile=[plan["tile_h"], plan["tile_w"]],
                   nchunks=plan["nchunks"], trips=plan["trips"])
        print(json.dumps(rec), flush=True)
        del x, w, gy


def end_to_end(batch, steps, repeats):
    import bench  # the flagship's own bf16 cast

    dev = torch.device("cuda:0")
    runs = []
    for flag in (False, True):
        torch.manual_seed(1234)
        model = msbn.models.mbconv_net(kernel_sizes=B0_KERNELS,
                                       conv_stats=flag, dw_grad=flag)
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
    p.add_argument("--skip-layers", action="store_true")
    p.add_argument("--skip-e2e", action="store_true")
    args = p.parse_args()
    if not args.skip_layers:
        per_layer(args.batch_size, args.iters, args.repeats)
    if not args.skip_e2e:
        end_to_end(args.batch_size, args.steps, args.repeats)


if __name__ == "__main__":
    main()
