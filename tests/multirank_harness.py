"""Run a list of cases on W ranks of one machine, inside ONE process group.

W spawned processes join a gloo group over a ``file://`` store (the mechanism
of test_gpu_multirank.py).  For ``device="cuda:0"`` every rank shares that
device (gloo moves CUDA tensors; RCCL forbids two ranks on one device), for
``device="cpu"`` every rank works on CPU tensors.  The worker loops over all
cases, so process start-up and HIP initialisation are paid once per world
size, not once per case.

A case function is named as ``"module:function"`` and is called as
``fn(rank, world, device, case) -> list of failure strings``.  It must finish
every collective of the case before it returns, on every rank, whatever its
checks find: failures are returned, not raised.  An exception is taken to mean
that the ranks are no longer in step; the worker then stops, reports the
remaining cases as not run, and its peers run into the group's 60 s timeout
instead of waiting for ever.  Whatever a case prints is captured and handed
back to the parent.

Nothing here waits without a bound: the group has a timeout, the parent a
deadline, a worker that dies is noticed through its sentinel.  Nothing is
tried twice.

A plain module, not a conftest: ``import multirank_harness``.
"""

import contextlib
import importlib
import io
import os
import tempfile
import time
import traceback
from datetime import timedelta
from multiprocessing import connection as mpc

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

MAX_WORLD = 4
GROUP_TIMEOUT_S = 60
DEADLINE_S = 150.0
NOT_RUN = "not run: an earlier case left the ranks out of step"


def _resolve(spec):
    mod, _, name = spec.partition(":")
    return getattr(importlib.import_module(mod), name)


def _worker(rank, world, device, fn_spec, cases, store, conn):
    results = []          # (case index, [failure, ...], captured output)
    fatal = None
    try:
        dist.init_process_group(
            "gloo", init_method=f"file://{store}", rank=rank,
            world_size=world, timeout=timedelta(seconds=GROUP_TIMEOUT_S),
        )
        if device != "cpu":
            torch.cuda.set_device(torch.device(device))
        fn = _resolve(fn_spec)
        for i, case in enumerate(cases):
            out = io.StringIO()
            try:
                with contextlib.redirect_stdout(out):
                    failures = list(fn(rank, world, device, case))
            except Exception:
                results.append((i, [traceback.format_exc()], out.getvalue()))
                results.extend((j, [NOT_RUN], "")
                               for j in range(i + 1, len(cases)))
                break
            results.append((i, failures, out.getvalue()))
    except Exception:
        fatal = traceback.format_exc()
    finally:
        try:
            conn.send((results, fatal))
        finally:
            conn.close()
            if dist.is_initialized():
                dist.destroy_process_group()


def _stop(procs):
    for p in procs:
        if p.is_alive():
            p.terminate()
    for p in procs:
        p.join(timeout=10)
        if p.is_alive():
            p.kill()
            p.join(timeout=10)


def run_cases(tmp_path, world, device, fn_spec, cases, deadline_s=DEADLINE_S):
    """Spawn ``world`` ranks, run every case on all of them, fail with every
    failure of every rank.  Returns {rank: [(case index, output), ...]}."""
    assert 1 <= world <= MAX_WORLD, world
    cases = list(cases)
    ctx = mp.get_context("spawn")
    # a store of its own for every group, however often a test calls this
    store = os.path.join(tempfile.mkdtemp(dir=str(tmp_path)), "pg")
    pending, procs = {}, []
    for rank in range(world):
        recv, send = ctx.Pipe(duplex=False)
        p = ctx.Process(target=_worker, args=(rank, world, device, fn_spec,
                                              cases, store, send))
        p.start()
        send.close()
        pending[rank] = (recv, p)
        procs.append(p)

    errs, outputs, broken = [], {}, False
    end = time.monotonic() + deadline_s
    try:
        while pending and not broken:
            left = end - time.monotonic()
            ready = left > 0 and mpc.wait(
                [c for c, _ in pending.values()]
                + [p.sentinel for _, p in pending.values()], timeout=left)
            if not ready:
                errs.append(
                    f"timeout: ranks {sorted(pending)} gave no result within "
                    f"{deadline_s:.0f} s; workers terminated")
                broken = True
                break
            for rank, (recv, p) in list(pending.items()):
                if recv.poll():
                    try:
                        results, fatal = recv.recv()
                    except EOFError:
                        p.join(timeout=10)
                        errs.append(f"rank {rank}: died without a result, "
                                    f"exit code {p.exitcode}")
                        broken = True
                        del pending[rank]
                        continue
                    if fatal:
                        errs.append(f"rank {rank}:\n{fatal}")
                    outputs[rank] = [(i, out) for i, _, out in results]
                    for i, failures, _ in results:
                        errs.extend(f"rank {rank}, case {cases[i]!r}:\n{f}"
                                    for f in failures)
                    # out of step: the peers can only run into the timeout
                    broken = broken or bool(fatal) or any(
                        NOT_RUN in f for _, f, _ in results)
                    del pending[rank]
                elif not p.is_alive():
                    errs.append(f"rank {rank}: died without a result, "
                                f"exit code {p.exitcode}")
                    broken = True
                    del pending[rank]
        if not broken:
            for p in procs:
                p.join(timeout=max(0.0, end - time.monotonic()))
                if p.is_alive():
                    errs.append(f"timeout: worker {p.pid} did not exit; "
                                "terminated")
    finally:
        _stop(procs)
    # every rank that reported is heard, also when another one broke
    for rank, (recv, _) in pending.items():
        try:
            if recv.poll():
                results, fatal = recv.recv()
                outputs[rank] = [(i, out) for i, _, out in results]
                if fatal:
                    errs.append(f"rank {rank}:\n{fatal}")
                for i, failures, _ in results:
                    errs.extend(f"rank {rank}, case {cases[i]!r}:\n{f}"
                                for f in failures if f != NOT_RUN)
        except (EOFError, OSError):
            pass
    assert not errs, f"{len(errs)} failure(s):\n" + "\n".join(errs)
    return outputs
