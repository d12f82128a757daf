#!/usr/bin/env python3
"""BatchNorm probe: on the VGG11's BatchNorm shapes at batch 100
(64x32x32, 128x16x16, 256x8x8, 512x4x4, 512x2x2, 1024x1x1) the time of

  train_fwd   rram_bn_stats_train + rram_norm_apply (gamma, beta, ReLU, x^ stored)
  fold_bwd    rram_norm_bwd_reduce + rram_norm_bwd_apply (ReLU mask, dgamma, dbeta)
  test_apply  rram_bn_stats_global + rram_norm_apply (gamma, beta, ReLU)

against rram_relu_fwd on the same tensor in the same run (the stream yardstick:
one read and one write of the tensor).  Per entry: bytes the launches move
(`moved`), the algorithmic bytes (`algo`: every tensor the result depends on
read once, every result written once), the achieved GB/s over `moved` and its
fraction of the ReLU stream's GB/s.  Each figure is the median of `--repeats`
timings of `--iters` back-to-back calls between two device events, after a
warm-up; the clocks are whatever the device runs at (not pinned), so compare
fractions within one run, not GB/s across runs.

Then one VGG11 batch-100 training iteration (fault-aware SGD, fused update)
with the BatchNorm + Scale + ReLU fold on and off, and the TEST net's
Monte-Carlo maps per second.  One JSON line per record is printed and written
to profiles/norm_probe.jsonl.

`--trace-train on|off` only runs four such training iterations with the fold
on or off and exits: run it under `rocprofv3 --kernel-trace -d DIR --` and give
DIR to scripts/kernel_sequence.py for the iteration's kernel sequence and
launch count (profiles/norm_kernel_sequence.txt)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rram-caffe-simulation_amd" / "python"))

BATCH = 100
SHAPES = [(64, 32, 32), (128, 16, 16), (256, 8, 8), (512, 4, 4), (512, 2, 2), (1024, 1, 1)]


def timed(fn, iters, repeats):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), (max(out) - min(out)) / statistics.median(out)


def kernels(args, emit):
    import torch
    from rramsim import ops
    for c, h, w in SHAPES:
        shape = (BATCH, c, h, w)
        n, inner = BATCH * c * h * w, h * w
        x = torch.randn(shape, device="cuda")
        y, xh, dy, dx = (torch.empty_like(x) for _ in range(4))
        dy.normal_()
        g, b = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda")
        mean, rstd, dg, db = (torch.zeros(c, device="cuda") for _ in range(4))
        rm, rv, f = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"), torch.ones(1, device="cuda")
        nws = ops.norm_workspace_floats(BATCH, c, inner)
        ws = torch.empty(nws, device="cuda")
        part, coef = ws[:nws - 3 * c], ws[nws - 3 * c:]

        def train_fwd():
            ops.bn_stats_train(x, mean, rstd, part, run_mean=rm, run_var=rv, factor=f)
            ops.norm_apply(x, y, mean, rstd, g, b, True, xhat_out=xh)

        def fold_bwd():
            ops.norm_bwd_reduce(dy, xh, part, relu_y=y, gamma=g, rstd=rstd, dgamma=dg, dbeta=db, coef=coef)
            ops.norm_bwd_apply(dy, dx, relu_y=y, xhat=xh, coef=coef)

        def test_apply():
            ops.bn_stats_global(rm, rv, f, mean, rstd)
            ops.norm_apply(x, y, mean, rstd, g, b, True)

        relu_ms, _ = timed(lambda: ops.relu_fwd(x, y), args.iters, args.repeats)
        relu_gbs = 2 * 4 * n / relu_ms / 1e6
        # tensor passes: (moved, algorithmic) in units of the tensor's bytes
        passes = {"train_fwd": (4, 3), "fold_bwd": (7, 4), "test_apply": (2, 2)}
        for name, fn in (("train_fwd", train_fwd), ("fold_bwd", fold_bwd), ("test_apply", test_apply)):
            ms, spread = timed(fn, args.iters, args.repeats)
            moved, algo = (p * 4 * n for p in passes[name])
            gbs = moved / ms / 1e6
            emit(dict(record="kernel", shape=[BATCH, c, h, w], entry=name, us=round(ms * 1e3, 2),
                      spread=round(spread, 3), moved_bytes=moved, algo_bytes=algo, moved_over_algo=round(moved / algo, 2),
                      gbs=round(gbs, 1), relu_us=round(relu_ms * 1e3, 2), relu_gbs=round(relu_gbs, 1),
                      frac_of_relu_stream=round(gbs / relu_gbs, 3)))


def nets(args, emit):
    import torch
    from rramsim import caffe, make_inject_cfg, models
    for fuse in (True, False):
        caffe.set_stream_from_torch()
        caffe.set_random_seed(1701)
        sp = models.solver(base_lr=0.005, momentum=0.9, weight_decay=0.004, max_iter=100000, failure_mean=5e6,
                           failure_std=1e6)
        opts = dict(models.net_options("cifar10_vgg11"), fused_update=True, fuse_bn_scale=fuse)
        s = caffe.Solver(sp, models.cifar10_vgg11(train_batch=BATCH, test_batch=BATCH), opts)
        s.step(3)
        ms, spread = timed(lambda: s.step(1), 5, args.repeats)
        s.close()
        net = caffe.Net(models.cifar10_vgg11(test_batch=BATCH), "test", opts)
        mc = caffe.MonteCarlo(net, make_inject_cfg(0.05), seed=7, max_maps=4096)
        mc.run(0, 4)
        mps, _ = timed(lambda: mc.run(4, 16), 1, args.repeats)
        mc.close()
        net.close()
        torch.cuda.synchronize()
        emit(dict(record="vgg11_b100", fuse_bn_scale=fuse, train_iter_ms=round(ms, 3), spread=round(spread, 3),
                  mc_maps_per_s=round(16 / (mps / 1e3), 1)))


def trace_train(fuse):
    import torch
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    sp = models.solver(base_lr=0.005, momentum=0.9, weight_decay=0.004, max_iter=100000, failure_mean=5e6,
                       failure_std=1e6)
    opts = dict(models.net_options("cifar10_vgg11"), fused_update=True, fuse_bn_scale=fuse)
    s = caffe.Solver(sp, models.cifar10_vgg11(train_batch=BATCH, test_batch=BATCH), opts)
    s.step(4)
    torch.cuda.synchronize()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "norm_probe.jsonl"))
    ap.add_argument("--skip-nets", action="store_true")
    ap.add_argument("--trace-train", choices=["on", "off"])
    args = ap.parse_args()
    if args.trace_train:
        trace_train(args.trace_train == "on")
        return
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(json.dumps(d))

    kernels(args, emit)
    if not args.skip_nets:
        nets(args, emit)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
