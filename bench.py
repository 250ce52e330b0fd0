#!/usr/bin/env python3
"""msbn flagship benchmark: ResNet-50 + SyncBatchNorm, bf16, synthetic 224x224
ImageNet-shaped data (BASELINE.json config 3 — the headline metric:
images/sec whole-node at 1/2/4/8 MI355X).

Single GPU:      python bench.py --gpus 1 --steps 30 --warmup 10
Multi GPU (driver): python -m torch.distributed.run --nnodes=1
                    --nproc-per-node N --master-addr 127.0.0.1 bench.py
                    --gpus N --steps K --warmup W

One JSON line is printed by rank 0 (contract in the project brief).

A plain run does only what the headline figure needs: set up, warm up, time
`--steps` train steps, print the line.  `--full` is where any measurement
beyond the headline figure belongs; today there is none, so it adds nothing.

`--dump-outputs DIR` additionally writes what the last timed step computed
(rank 0) as DIR/<name>.npy, so two builds can be compared output for output.
Seeds, model init and the synthetic batch are fixed by the arguments, but
that alone does not make the last step repeatable.  Measured on one MI355X:
between identical iterations the forward pass, every BatchNorm gradient and
the whole dx chain are bit-identical, while the weight gradient of each of
the 53 convolutions varies in its last bf16 bit (MIOpen's tuned
backward-weights solvers add split-K partial sums atomically, in arrival
order; the deterministic solvers cost 28 s per step against 0.055 s).  bf16
SGD on one repeated batch turns that into loss 3.6-4.0 and logits apart by
hundreds after 40 steps.  So a dumping run puts the model and optimizer back
to their seeded initial state just before the last timed step (one foreach
copy inside the timed window): that step runs the same kernels as every
other, from the same weights in every run, and what is dumped are its
results that no varying sum feeds: loss, logits, and the stem BatchNorm and
classifier state after the update (the stem's affine gradient is the end of
the backward chain through every BN kernel and every conv's dx).
"""

import argparse
import contextlib
import json
import os
import sys
import time

import torch
import torch.distributed as dist

import msbn


def cast_bf16_keep_bn_fp32(model):
    """bf16 weights everywhere except BatchNorm affine params + running stats
    (standard mixed-precision practice; msbn kernels take bf16 activations
    with fp32 channel parameters)."""
    from msbn.nn.batchnorm import _NormBase

    model.to(torch.bfloat16)
    for m in model.modules():
        if isinstance(m, (_NormBase, torch.nn.modules.batchnorm._BatchNorm)):
            m.float()
    return model


def build_model(name, memory_format, dtype, device, sync, fused=True):
    if name == "resnet50":
        model = msbn.models.resnet50(fused=fused)
    elif name == "resnet18":
        model = msbn.models.resnet18(fused=fused)
    else:
        raise ValueError(name)
    if sync:
        model = msbn.convert_sync_batchnorm(model)
    model = model.to(device)
    if dtype == torch.bfloat16:
        model = cast_bf16_keep_bn_fp32(model)
    if memory_format == torch.channels_last:
        model = model.to(memory_format=torch.channels_last)
    return model


DUMP_MAX_BYTES = 64 << 20  # whole --dump-outputs directory
# Model state the last step updated, dumped next to the step's own results.
# No conv weight: its gradient is the one thing that varies from run to run
# (module docstring).
DUMP_STATE = ("bn1.weight", "bn1.bias", "bn1.running_mean",
              "bn1.running_var", "fc.weight")


def dump_outputs(dirname, arrays):
    """Write {name: tensor} as dirname/<name>.npy (float32, or float64 for
    float64 tensors).  Each array gets an equal share of DUMP_MAX_BYTES; a
    larger one is cut down to a fixed, seeded sample of its flat elements."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    cap = DUMP_MAX_BYTES // max(len(arrays), 1)
    for name, t in arrays.items():
        t = t.detach()
        t = t.to("cpu", torch.float64 if t.dtype == torch.float64
                 else torch.float32).contiguous()
        a = t.numpy()
        if a.nbytes > cap:
            idx = np.random.default_rng(0).choice(
                a.size, size=cap // a.itemsize, replace=False)
            idx.sort()
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=512,
                   help="per-GPU batch (weak scaling)")
    p.add_argument("--model", type=str, default="resnet50")
    # channels_last default: fastest measured path on gfx950 (MIOpen igemm
    # kernels are NHWC-native -> no transposes; msbn NHWC BN kernels are
    # C-vectorized). See profiles/r01_single_gpu.md.
    p.add_argument("--memory-format", type=str, default="channels_last",
                   choices=["channels_last", "contiguous"])
    p.add_argument("--dtype", type=str, default="bf16",
                   choices=["bf16", "fp32"])
    p.add_argument("--stock", action="store_true",
                   help="use stock torch SyncBatchNorm+DDP (comparison line)")
    p.add_argument("--benchmark", action="store_true",
                   help="enable MIOpen conv autotune (cudnn.benchmark): "
                        "minutes of find cost in every process; only for "
                        "configs the shipped find-db does not cover")
    p.add_argument("--graph", action="store_true",
                   help="capture the train step in a hipGraph (single GPU)")
    p.add_argument("--no-fused", action="store_true",
                   help="disable the fused BN(+add)+ReLU epilogue modules")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write the last step's loss "
                        "and logits and the model state it updated as "
                        "DIR/<name>.npy (rank 0)")
    p.add_argument("--full", action="store_true",
                   help="also run every measurement beyond the headline "
                        "figure (none today: same as a plain run)")
    p.add_argument("--local_rank", "--local-rank", type=int,
                   default=int(os.environ.get("LOCAL_RANK", 0)),
                   dest="local_rank")
    args = p.parse_args()

    # In-tree MIOpen find-db (miopen_db/, exported by
    # tools/export_miopen_finddb.sh after a --benchmark run): tuned conv
    # solver choices ship with the repo.  MIOpen's immediate mode (the
    # default, cudnn.benchmark off) picks each conv's solver from this db, so
    # the tuned config (resnet50 bf16 CL bs512 — the headline bench) runs the
    # tuned solvers from its first step.  Autotune is NOT auto-enabled: the
    # find re-measures every solver of every conv in each new process even
    # when the db has the record (~120 s before the first step, measured)
    # and rewrites the db files, for the same steady-state step time
    # (A/B in profiles/r02_kernel_polish.md §9).  --benchmark opts in, to
    # tune another config or to refresh the db.
    _db = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "miopen_db")
    if os.path.isdir(_db) and os.listdir(_db):
        os.environ.setdefault("MIOPEN_USER_DB_PATH", _db)
    if args.benchmark:
        torch.backends.cudnn.benchmark = True  # MIOpen conv autotune

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    distributed = world_size > 1
    use_cuda = torch.cuda.is_available()
    device = torch.device(f"cuda:{args.local_rank}" if use_cuda else "cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    if distributed:
        dist.init_process_group(
            backend="nccl" if use_cuda else "gloo", init_method="env://",
            world_size=world_size, rank=rank,
        )

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    mem_fmt = (torch.channels_last if args.memory_format == "channels_last"
               else torch.contiguous_format)

    torch.manual_seed(1234)
    # Whole-step hipGraph capture (single OR multi GPU; msbn impl only —
    # stock DDP needs static_graph for capture).  The model, DDP wrapper,
    # data, warmup AND capture must share ONE side stream: the reducer's
    # autograd hooks live on AccumulateGrad nodes created at DDP-construction
    # time, and the engine replays them on their creation-time stream — a
    # default-stream accumulator would launch the bucket all-reduce outside
    # the capture (tools/nccl_world1_check.py case `graph`).
    use_graph = (args.graph or os.environ.get("MSBN_GRAPH", "0") == "1") \
        and use_cuda and not args.stock
    side_stream = torch.cuda.Stream() if use_graph else None
    stream_ctx = (
        torch.cuda.stream(side_stream) if use_graph else contextlib.nullcontext()
    )
    with stream_ctx:
        if args.stock:
            model = msbn.models.resnet50() if args.model == "resnet50" else \
                msbn.models.resnet18()
            if distributed:
                model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
            model = model.to(device)
            if dtype == torch.bfloat16:
                model = cast_bf16_keep_bn_fp32(model)
            if mem_fmt == torch.channels_last:
                model = model.to(memory_format=torch.channels_last)
            if distributed:
                model = torch.nn.parallel.DistributedDataParallel(
                    model, device_ids=[args.local_rank] if use_cuda else None,
                    output_device=args.local_rank if use_cuda else None,
                )
        else:
            model = build_model(args.model, mem_fmt, dtype, device, sync=True,
                                fused=not args.no_fused)
            if distributed:
                model = msbn.parallel.DistributedDataParallel(
                    model,
                    device_ids=[args.local_rank] if use_cuda else None,
                    output_device=args.local_rank if use_cuda else None,
                    gradient_as_bucket_view=True,
                    bucket_cap_mb=float(os.environ.get("MSBN_BUCKET_MB", "25")),
                )
        model.train()

        # --dump-outputs: the seeded initial state, put back before the last
        # timed step so that step starts from the same weights in every run
        restore = None
        if args.dump_outputs:
            core = getattr(model, "module", model)
            live = list(core.parameters()) + list(core.buffers())
            init = [t.detach().clone() for t in live]

            def restore():
                with torch.no_grad():
                    torch._foreach_copy_(live, init)
                    # zeroed momentum == no momentum yet: buf = 0.9*0 + grad
                    bufs = [st["momentum_buffer"] for st in opt.state.values()
                            if st.get("momentum_buffer") is not None]
                    if bufs:
                        torch._foreach_zero_(bufs)

        try:  # fused foreach SGD (works on ROCm; identical for both impls)
            opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                                  weight_decay=1e-4, fused=True)
        except (RuntimeError, TypeError):
            opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                                  weight_decay=1e-4)
        loss_fn = torch.nn.CrossEntropyLoss()

        bs = args.batch_size
        x = torch.randn(bs, 3, 224, 224, device=device, dtype=dtype)
        if mem_fmt == torch.channels_last:
            x = x.to(memory_format=torch.channels_last)
        y = torch.randint(0, 1000, (bs,), device=device)

        def step():
            opt.zero_grad(set_to_none=True)
            out = model(x)
            loss = loss_fn(out.float(), y)
            loss.backward()
            opt.step()
            return loss.detach(), out.detach()

        # warmup (on the side stream when graphing: allocator steady state,
        # MIOpen finds, RCCL communicator creation)
        for _ in range(max(args.warmup, 3) if use_graph else args.warmup):
            step()
        if use_graph:
            opt.zero_grad(set_to_none=False)

    graph = None
    if use_graph:
        # hipGraph-captured whole train step (fwd+bwd+optimizer+collectives):
        # kills the ~500 per-step kernel-launch round trips AND the per-layer
        # collective launch latency.  msbn's BN ops are capture-safe by
        # design (no host syncs; zero-count masking is in-kernel).  Falls
        # back to eager on any capture failure.
        torch.cuda.synchronize()
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side_stream):
                out = model(x)
                loss = loss_fn(out.float(), y)
                loss.backward()
                opt.step()
                # zero grads IN-GRAPH so replays are self-contained
                torch._foreach_zero_([p.grad for p in model.parameters()
                                      if p.grad is not None])
            for _ in range(args.warmup):
                graph.replay()
        except Exception as e:  # capture unsupported for this config
            print(f"[bench] hipGraph capture failed ({e!r}); "
                  "falling back to eager", file=sys.stderr)
            graph = None
            torch.cuda.synchronize()

    if distributed:
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    if graph is not None:
        for i in range(args.steps):
            if restore is not None and i == args.steps - 1:
                restore()
            graph.replay()  # rewrites the captured `loss` and `out` in place
    else:
        for i in range(args.steps):
            if restore is not None and i == args.steps - 1:
                restore()
            loss, out = step()
    if use_cuda:
        torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # MAX elapsed over ranks decides whole-job throughput
    if distributed:
        t = torch.tensor([elapsed], device=device if use_cuda else "cpu",
                         dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    n_gpus = world_size
    images_per_sec = bs * n_gpus * args.steps / elapsed
    ms_per_step = 1000.0 * elapsed / args.steps

    if args.dump_outputs and rank == 0:
        state = getattr(model, "module", model).state_dict()
        arrays = {"loss": loss.reshape(1), "logits": out}
        arrays.update((k.replace(".", "_"), state[k]) for k in DUMP_STATE)
        dump_outputs(args.dump_outputs, arrays)

    if rank == 0:
        print(json.dumps({
            "metric": f"images/sec (whole node) {args.model} SyncBN",
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": bs * n_gpus,
                "per_gpu_batch": bs,
                "image": "3x224x224",
                "memory_format": args.memory_format,
                "parallelism": f"dp{n_gpus}",
                "impl": "stock" if args.stock else "msbn",
                "hip_graph": graph is not None,
                "conv_autotune": args.benchmark,
                "fused_bn_act": not (args.stock or args.no_fused),
            },
        }))

    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
