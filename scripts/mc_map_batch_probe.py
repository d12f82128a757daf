#!/usr/bin/env python3
"""Monte-Carlo map batching probe: maps/s of C2 (cifar10_quick, B = 100,
quant16 + lognormal 0.1, p = 0.01) and LeNet MC (B = 100, stuck-at p = 0.01)
at map_batch K in {1, 4, 16, 32}, all in one process.  K = 1 is the baseline:
the untouched sequential driver on the batch-B net.  K > 1 builds the net at
batch K x B, tiles the first B images over the K slices and runs K maps per
forward (rramsim.caffe.MonteCarlo(map_batch=K)).

Per (workload, K): a warm-up, `--repeats` timed repeats of `--maps` maps each
(device synchronised around each), the median maps/s and the spread
((max - min) / median) of the repeats.  Then one more pass with the hipEvent
layer timers on: the time in the Convolution and InnerProduct layers per map,
their TF/s from the algorithmic FLOPs per map, and the layer forwards per map
(Forward calls of all layers plus injection launches, divided by the maps:
the host-side count that shrinks by K; kernel launches inside a layer are not
counted).  One JSON line per (workload, K) is appended to
profiles/mc_map_batch.jsonl and printed.

A K that set_map_batch refuses (a batch-dependent plan of a prefix layer) is
recorded with its message instead of numbers."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "rram-caffe-simulation_amd" / "python",):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

B = 100


def build(workload, k):
    from rramsim import caffe, make_inject_cfg, models
    if workload == "c2":
        net = caffe.Net(models.cifar10_quick(test_batch=k * B), "test", models.net_options("cifar10_quick"))
        cfgs = []
        for f in net.failure_params():
            gmax = float(f["data"].abs().max().item()) or 1.0
            cfgs.append(make_inject_cfg(0.01, 10, 20, 10, quant_levels=16, g_max=gmax, var_sigma=0.1,
                                        stuck_scale=gmax))
    else:
        net = caffe.Net(models.lenet(test_batch=k * B), "test", models.net_options("lenet"))
        cfgs = [make_inject_cfg(0.01, 5, 90, 5)]
    return net, cfgs


def measure(workload, k, maps, repeats, seed):
    import torch
    from rramsim import caffe
    from rramsim._kernels import RramError
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    net, cfgs = build(workload, k)
    rec = dict(workload=workload, map_batch=k, images_per_map=B, maps_per_repeat=maps, repeats=repeats)
    try:
        mc = caffe.MonteCarlo(net, cfgs, seed=seed, max_maps=8, map_batch=k)
    except RramError as e:
        net.close()
        return dict(rec, refused=str(e))
    mc.tile_inputs()
    mc.run(0, 2 * max(k, 8))                       # warm-up: every buffer allocated, tables built
    torch.cuda.synchronize()
    rates = []
    for r in range(repeats):
        t0 = time.perf_counter()
        mc.run((r + 1) * maps, maps)
        torch.cuda.synchronize()
        rates.append(maps / (time.perf_counter() - t0))
    med = statistics.median(rates)
    rec.update(maps_per_s=round(med, 1), maps_per_s_min=round(min(rates), 1), maps_per_s_max=round(max(rates), 1),
               spread=round((max(rates) - min(rates)) / med, 4))
    # the layer timers: one pass of `maps` maps with events around every layer
    con = net.contractions()
    net.layer_times(reset=True)
    mc.inject_times(reset=True)
    net.set_timing(1)
    mc.set_timing(True)
    mc.run((repeats + 1) * maps, maps)
    torch.cuda.synchronize()
    net.set_timing(0)
    mc.set_timing(False)
    lt = net.layer_times()
    _, inj_launches, _ = mc.inject_times()
    rec["layer_forwards_per_map"] = round((sum(c for _, _, _, c in lt) + inj_launches) / maps, 2)
    for typ, key in (("Convolution", "conv"), ("InnerProduct", "ip")):
        ms = sum(m for name, t, m, _ in lt if t == typ) / maps            # per map
        flops = sum(f for name, (f, e) in con.items() if any(n == name and t == typ for n, t, _, _ in lt)) / k
        rec[key + "_ms_per_map"] = round(ms, 5)
        rec[key + "_tflops"] = round(flops / (ms * 1e-3) / 1e12, 3) if ms > 0 else None
    mc.close()
    net.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ks", default="1,4,16,32")
    ap.add_argument("--workloads", default="c2,lenet")
    ap.add_argument("--maps", type=int, default=320, help="maps per timed repeat (a multiple of every K)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1701)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mc_map_batch.jsonl"))
    args = ap.parse_args()
    ks = [int(x) for x in args.ks.split(",")]
    assert all(args.maps % k == 0 for k in ks), "--maps must be a multiple of every K"
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for w in args.workloads.split(","):
        base = None
        for k in ks:
            rec = measure(w, k, args.maps, args.repeats, args.seed)
            if k == 1 and "maps_per_s" in rec:
                base = rec
            if base and "maps_per_s" in rec:
                rec["ratio_to_k1"] = round(rec["maps_per_s"] / base["maps_per_s"], 3)
                # faster than K = 1 by more than the run-to-run spread either side reports
                rec["faster_than_k1_beyond_spread"] = bool(rec["maps_per_s_min"] > base["maps_per_s_max"])
            line = json.dumps(rec)
            print(line, flush=True)
            with out.open("a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
