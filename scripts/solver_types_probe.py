#!/usr/bin/env python3
"""Solver-type probe: ms per training iteration of C4 (cifar10_full, batch
100, gaussian failure pattern + threshold strategy, fused_update=True) for
each solver type, all in one process.

Per type: a warm-up, `--repeats` timed repeats of `--iters` iterations each
(device synchronised around each), the median ms per iteration and the spread
((max - min) / median) of the repeats.  Then the tail timer: the one-launch
fused tail alone (one kernel for all types; SGD goes in through
rram_fused_update_fail_batched, so that a build from before the other types
is measured through the same entry, the others through
rram_fused_opt_update_fail_batched) on scratch blobs of the
net's own learnable shapes and fault state, between two device events, and
the bytes it moves (9 floats per faultable element, 5 per other element, 2
more per element with a second history), so its GB/s.  One JSON line per
type is appended to profiles/solver_types.jsonl and printed.

`--types SGD` is the yardstick: it touches nothing but the SGD entries, so the
same script runs on a build that predates the other types.  Every type after
the first reports its difference to the first one's iteration and whether it
exceeds that one's whole fused-tail time (a type that lost its fusion).

Each type runs under a time limit of its own (`--step-timeout` seconds, a
SIGALRM watchdog): a step that overruns ends the probe with a non-zero status
instead of starting the next type."""
import argparse
import json
import signal
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "rram-caffe-simulation_amd" / "python",):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

BATCH = 100
KIND_IDS = {"SGD": 0, "Nesterov": 1, "AdaGrad": 2, "RMSProp": 3, "AdaDelta": 4, "Adam": 5}
TWO_HISTORIES = ("AdaDelta", "Adam")


class StepTimeout(Exception):
    pass


def _alarm(_sig, _frm):
    raise StepTimeout()


def solver_text(kind):
    from rramsim import models
    mom = 0.0 if kind in ("AdaGrad", "RMSProp") else (0.95 if kind == "AdaDelta" else 0.9)
    sp = models.solver(base_lr=0.001, momentum=mom, weight_decay=0.004, lr_policy="fixed", max_iter=100000,
                       failure_mean=5e4, failure_std=1.5e4, failure_prob=(5, 90, 5), threshold=0.001)
    return sp if kind == "SGD" else sp + f'type: "{kind}"\n'


def tail_timer(kind, s, repeats):
    """The fused tail alone on copies of the solver's blobs: median ms, bytes moved."""
    import torch
    from rramsim import ops
    ps = s.net.params()
    fault = {f["data"].data_ptr(): i for i, f in enumerate(s.net.failure_params())}
    fs = s.fail_state()
    two = kind in TWO_HISTORIES
    segs, nbytes = [], 0
    for p in ps:
        w = p["data"].detach().clone().reshape(-1)
        g = torch.randn_like(w) * 1e-3
        h = torch.rand_like(w) * 1e-3
        h2 = torch.rand_like(w) * 1e-3 if two else None
        fi = fault.get(p["data"].data_ptr())
        e = fs[fi][0].detach().clone() if fi is not None else None
        v = fs[fi][1].detach().clone() if fi is not None else None
        faulty = e is not None
        nbytes += 4 * w.numel() * ((9 if faulty else 5) + (2 if two else 0))
        if kind == "SGD":
            segs.append((w, g, h, e, v, 0.004, 0.001, faulty, 1e-6, None))
        else:
            segs.append((w, g, h, h2, e, v, 0.004, 0.001, faulty, 1e-6, None))
    if kind == "SGD":
        run = lambda: ops.fused_update_fail_batched(segs, 0.9)                     # noqa: E731
    else:
        hy = ops.solver_hyper(0.0 if kind in ("AdaGrad", "RMSProp") else 0.9, 0.999, 1e-8)
        run = lambda: ops.fused_opt_update_fail_batched(KIND_IDS[kind], hy, segs)  # noqa: E731
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(repeats, 5) * 4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), nbytes


def measure(kind, iters, repeats, warmup):
    import torch
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    s = caffe.Solver(solver_text(kind), models.cifar10_full(train_batch=BATCH, test_batch=BATCH),
                     dict(models.net_options("cifar10_full"), fused_update=True))
    s.step(warmup)
    torch.cuda.synchronize()
    per_iter = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        s.step(iters)
        torch.cuda.synchronize()
        per_iter.append((time.perf_counter() - t0) * 1e3 / iters)
    med = statistics.median(per_iter)
    rec = dict(type=kind, batch=BATCH, iters_per_repeat=iters, repeats=repeats, ms_per_iter=round(med, 4),
               ms_per_iter_min=round(min(per_iter), 4), ms_per_iter_max=round(max(per_iter), 4),
               spread=round((max(per_iter) - min(per_iter)) / med, 4), history_blobs=len(s.history()),
               params=len(s.net.params()))
    tail_ms, nbytes = tail_timer(kind, s, repeats)
    rec.update(tail_ms=round(tail_ms, 5), tail_bytes=nbytes, tail_gbps=round(nbytes / (tail_ms * 1e-3) / 1e9, 1))
    s.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--types", default="SGD,Nesterov,AdaGrad,RMSProp,AdaDelta,Adam")
    ap.add_argument("--iters", type=int, default=50, help="iterations per timed repeat")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=90, help="seconds per solver type")
    ap.add_argument("--label", default="", help="recorded with every line (e.g. the commit measured)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "solver_types.jsonl"))
    args = ap.parse_args()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    signal.signal(signal.SIGALRM, _alarm)
    base = None
    for kind in args.types.split(","):
        signal.alarm(args.step_timeout)
        try:
            rec = measure(kind, args.iters, args.repeats, args.warmup)
        except StepTimeout:
            print(json.dumps(dict(type=kind, error=f"no result within {args.step_timeout} s")), flush=True)
            sys.exit(3)
        finally:
            signal.alarm(0)
        if args.label:
            rec["label"] = args.label
        if base is None:
            base = rec
        else:
            rec["delta_ms_to_" + base["type"]] = round(rec["ms_per_iter"] - base["ms_per_iter"], 4)
            rec["tail_bytes_ratio_to_" + base["type"]] = round(rec["tail_bytes"] / base["tail_bytes"], 4)
            rec["slower_by_more_than_the_tail"] = bool(rec["ms_per_iter"] - base["ms_per_iter"] > base["tail_ms"])
        line = json.dumps(rec)
        print(line, flush=True)
        with out.open("a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
