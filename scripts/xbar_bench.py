"""Times the crossbar-tiled forwards beside the plain forwards of the same
shapes (the same MFMA count without the per-tile rounding): rram_ip_fwd_xbar
beside rram_ip_fwd on the fc6 / fc7 / CIFAR ip1 shapes, or with --conv
rram_conv2d_fwd_xbar beside rram_conv2d_fwd on AlexNet conv2 / conv3, VGG11
conv2 / conv8 and a GoogLeNet 1x1, or with --serial the bit-serial
rram_ip_fwd_xbar_bs beside rram_ip_fwd_xbar with the same DAC (dac_bits 4 and 8)
on the InnerProduct shapes, or with --sliced the bit-sliced-weight
rram_ip_fwd_xbar_ws (weight_bits 8, cell_bits 2 and 1) beside rram_ip_fwd_xbar
with the same 8-bit DAC, or with --serial-sliced the digit-serial
rram_ip_fwd_xbar_ss (digit_bits 1 and 2, cell_bits 2) beside rram_ip_fwd_xbar_ws
at cell_bits 2, or with --backward the transposed read-out
rram_ip_bwd_data_xbar beside rram_ip_bwd with only dx wanted and beside
rram_ip_fwd_xbar on the mirrored shape.  Call times from device events (every
launch of the call included), the two alternated in one process, the median and
range of REPS windows of ITERS calls each.

    python scripts/xbar_bench.py [--conv | --serial | --sliced | --serial-sliced | --backward] [out.txt]

--sliced --shape=fc6 --cells=2 keeps one shape and one cell width, so that a
kernel trace of the run (per-kernel totals) gives the weight pack's share of
that call.
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rram-caffe-simulation_amd" / "python"))

import torch  # noqa: E402

from rramsim import ops  # noqa: E402

ROOF = 2.5e15 / 6          # bf16 dense peak over the six products, FLOP/s of fp32-equivalent work
SHAPES = [("fc6", 256, 4096, 9216, 128, 8), ("fc7", 256, 4096, 4096, 128, 8), ("cifar ip1", 100, 64, 1024, 64, 8)]
# name, x shape, Cout, kernel, pad, group, R, B
CONVS = [("alexnet conv2 b256", (256, 96, 27, 27), 256, 5, 2, 2, 128, 8),
         ("alexnet conv3 b256", (256, 256, 13, 13), 384, 3, 1, 1, 128, 8),
         ("vgg11 conv2 b100", (100, 64, 16, 16), 128, 3, 1, 1, 128, 8),
         ("vgg11 conv8 b100", (100, 512, 2, 2), 512, 3, 1, 1, 128, 8),
         ("googlenet 3a 1x1 b128", (128, 192, 28, 28), 64, 1, 0, 1, 128, 8)]
ITERS, REPS = 50, 7


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3   # us per call


def row(head, fx, fp, idx, idp, flops):
    """One result line: fx (crossbar) and fp (plain) warmed up, then timed in alternating windows."""
    for f in (fx, fp):
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    tx, tp = [], []
    for _ in range(REPS):
        tx.append(window(fx))
        tp.append(window(fp))
    mx, mp = sorted(tx)[REPS // 2], sorted(tp)[REPS // 2]
    return (f"{head} | {mx:.1f} ({min(tx):.1f}..{max(tx):.1f}) {','.join(idx)} | "
            f"{mp:.1f} ({min(tp):.1f}..{max(tp):.1f}) {','.join(idp)} | {mx / mp:.2f} | {flops / (mx * 1e-6) / ROOF:.3f}")


def ip_rows():
    lines = ["shape  M x N x K  R B | xbar us (min..max) ids | plain us (min..max) ids | ratio | xbar share of 416.7 TFLOP/s"]
    for name, M, N, K, R, B in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(M, K, device="cuda", generator=g)
        w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
        bias = torch.randn(N, device="cuda", generator=g)
        y = torch.empty(M, N, device="cuda")
        cfg = ops.xbar_cfg(R, B, 4.0)
        wsx = torch.empty(max(1, ops.ip_fwd_xbar_workspace(M, N, K, cfg)), dtype=torch.uint8, device="cuda")
        wsp = torch.empty(min(16 * M * N * 4, 256 << 20), dtype=torch.uint8, device="cuda")
        fx = lambda: ops.ip_fwd_xbar(x, w, bias, y, M, N, K, cfg, relu=True, workspace=wsx)  # noqa: E731
        fp = lambda: ops.ip_fwd(x, w, bias, y, M, N, K, relu=True, workspace=wsp)            # noqa: E731
        lines.append(row(f"{name}  {M} x {N} x {K}  {R} {B}", fx, fp,
                         ops.ip_fwd_xbar_kernel_ids(M, N, K, cfg, ws_bytes=wsx.numel()),
                         ops.ip_fwd_kernel_ids(M, N, K, relu=True, ws_bytes=wsp.numel()), 2.0 * M * N * K))
    return lines


def serial_rows():
    lines = ["shape  M x N x K  R B b | bit-serial us (min..max) ids | parallel xbar us (min..max) ids | ratio | "
             "MFMA count ratio (b - 1) / 2 | bit-serial share of 416.7 TFLOP/s"]
    for name, M, N, K, R, B in SHAPES:
        for b in (4, 8):
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(M, K, device="cuda", generator=g)
            w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
            bias = torch.randn(N, device="cuda", generator=g)
            y = torch.empty(M, N, device="cuda")
            cfg = ops.xbar_cfg(R, B, 4.0, b, 4.0)
            wss = torch.empty(max(1, ops.ip_fwd_xbar_bs_workspace(M, N, K, cfg)), dtype=torch.uint8, device="cuda")
            wsx = torch.empty(max(1, ops.ip_fwd_xbar_workspace(M, N, K, cfg)), dtype=torch.uint8, device="cuda")
            fs = lambda: ops.ip_fwd_xbar_bs(x, w, bias, y, M, N, K, cfg, relu=True, workspace=wss)  # noqa: E731
            fx = lambda: ops.ip_fwd_xbar(x, w, bias, y, M, N, K, cfg, relu=True, workspace=wsx)     # noqa: E731
            line = row(f"{name}  {M} x {N} x {K}  {R} {B} {b}", fs, fx,
                       ops.ip_fwd_xbar_bs_kernel_ids(M, N, K, cfg, ws_bytes=wss.numel()),
                       ops.ip_fwd_xbar_kernel_ids(M, N, K, cfg, ws_bytes=wsx.numel()), 2.0 * M * N * K)
            head, share = line.rsplit(" | ", 1)
            lines.append(f"{head} | {(b - 1) / 2:.1f} | {share}")
    return lines


def sliced_rows(shape=None, cells=None):
    lines = ["shape  M x N x K  R B b wb cb | sliced us (min..max) ids | parallel xbar us (min..max) ids | ratio | "
             "MFMA count ratio Ns / 6 | sliced share of 416.7 TFLOP/s"]
    for name, M, N, K, R, B in SHAPES:
        for cb in (2, 1):
            if (shape and shape not in name) or (cells and cells != cb):
                continue
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(M, K, device="cuda", generator=g)
            w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
            bias = torch.randn(N, device="cuda", generator=g)
            y = torch.empty(M, N, device="cuda")
            cfg, sl = ops.xbar_cfg(R, B, 4.0, 8, 4.0), ops.xbar_slices(8, cb, 4.0 * K ** -0.5)
            wss = torch.empty(ops.ip_fwd_xbar_ws_workspace(M, N, K, cfg, sl), dtype=torch.uint8, device="cuda")
            wsx = torch.empty(max(1, ops.ip_fwd_xbar_workspace(M, N, K, cfg)), dtype=torch.uint8, device="cuda")
            fs = lambda: ops.ip_fwd_xbar_ws(x, w, bias, y, M, N, K, cfg, sl, relu=True, workspace=wss)  # noqa: E731
            fx = lambda: ops.ip_fwd_xbar(x, w, bias, y, M, N, K, cfg, relu=True, workspace=wsx)         # noqa: E731
            line = row(f"{name}  {M} x {N} x {K}  {R} {B} 8 8 {cb}", fs, fx,
                       ops.ip_fwd_xbar_ws_kernel_ids(M, N, K, cfg, sl, ws_bytes=wss.numel()),
                       ops.ip_fwd_xbar_kernel_ids(M, N, K, cfg, ws_bytes=wsx.numel()), 2.0 * M * N * K)
            head, share = line.rsplit(" | ", 1)
            lines.append(f"{head} | {-(-7 // cb) / 6:.2f} | {share}")
    return lines


def serial_sliced_rows():
    lines = ["shape  M x N x K  R B b wb db cb | serial-sliced us (min..max) ids | sliced xbar_ws us (min..max) ids | "
             "ratio | MFMA count ratio Nd | ratio per MFMA"]
    for name, M, N, K, R, B in SHAPES:
        for db in (1, 2):
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(M, K, device="cuda", generator=g)
            w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
            bias = torch.randn(N, device="cuda", generator=g)
            y = torch.empty(M, N, device="cuda")
            cfg, sl = ops.xbar_cfg(R, B, 4.0, 8, 4.0), ops.xbar_slices(8, 2, 4.0 * K ** -0.5)
            wsd = torch.empty(ops.ip_fwd_xbar_ss_workspace(M, N, K, cfg, sl, db), dtype=torch.uint8, device="cuda")
            wss = torch.empty(ops.ip_fwd_xbar_ws_workspace(M, N, K, cfg, sl), dtype=torch.uint8, device="cuda")
            fd = lambda: ops.ip_fwd_xbar_ss(x, w, bias, y, M, N, K, cfg, sl, db, relu=True, workspace=wsd)  # noqa: E731
            fs = lambda: ops.ip_fwd_xbar_ws(x, w, bias, y, M, N, K, cfg, sl, relu=True, workspace=wss)      # noqa: E731
            line = row(f"{name}  {M} x {N} x {K}  {R} {B} 8 8 {db} 2", fd, fs,
                       ops.ip_fwd_xbar_ss_kernel_ids(M, N, K, cfg, sl, db, ws_bytes=wsd.numel()),
                       ops.ip_fwd_xbar_ws_kernel_ids(M, N, K, cfg, sl, ws_bytes=wss.numel()), 2.0 * M * N * K)
            head, ratio, _ = line.rsplit(" | ", 2)
            nd = -(-7 // db)
            lines.append(f"{head} | {ratio} | {nd} | {float(ratio) / nd:.2f}")
    return lines


def conv_rows():
    lines = ["shape  x -> Cout k/pad/group  R B | xbar us (min..max) ids | plain us (min..max) ids | ratio | "
             "xbar share of 416.7 TFLOP/s"]
    for name, xs, cout, k, pad, group, R, B in CONVS:
        d = ops.conv_desc(xs, cout, k, 1, pad, 1, group)
        kg = xs[1] // group * k * k
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(*xs, device="cuda", generator=g)
        w = torch.randn(cout, xs[1] // group, k, k, device="cuda", generator=g) * kg ** -0.5
        bias = torch.randn(cout, device="cuda", generator=g)
        y = torch.empty(xs[0], cout, d.out_h, d.out_w, device="cuda")
        cfg = ops.xbar_cfg(R, B, 4.0)
        wsx = torch.empty(max(1, ops.conv_fwd_xbar_workspace(d, cfg)), dtype=torch.uint8, device="cuda")
        fx = lambda: ops.conv_fwd_xbar(d, x, w, bias, y, cfg, relu=True, workspace=wsx)      # noqa: E731
        fp = lambda: ops.conv2d_fwd(d, x, w, bias, y, relu=True)                             # noqa: E731
        lines.append(row(f"{name}  {'x'.join(map(str, xs))} -> {cout} {k}/{pad}/{group}  {R} {B}", fx, fp,
                         ops.conv_fwd_xbar_kernel_ids(d, cfg, ws_bytes=wsx.numel()), ops.conv_fwd_kernel_ids(d),
                         2.0 * xs[0] * d.out_h * d.out_w * cout * kg))
    return lines


def backward_rows():
    """rram_ip_bwd_data_xbar (dx from dy [M][N] and w [N][K], tiles of C columns over N) beside (a) rram_ip_bwd
    with only dx wanted and (b) rram_ip_fwd_xbar on the mirrored shape (M, N' = K, K' = N): the same MFMAs,
    the weights staged as they lie.  The three alternated window by window."""
    lines = ["shape  M x N x K  C B | transposed xbar us (min..max) ids | (a) plain dx us (min..max) ids | "
             "(b) mirrored forward xbar us (min..max) ids | ratio to (a) | ratio to (b)"]
    for name, M, N, K, C, B in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        dy = torch.randn(M, N, device="cuda", generator=g)
        w = torch.randn(N, K, device="cuda", generator=g) * N ** -0.5
        wm = w.t().contiguous()                                      # [K][N]: (b)'s weight rows run along N
        x, dx = torch.randn(M, K, device="cuda", generator=g), torch.empty(M, K, device="cuda")
        cfg = ops.xbar_cfg(C, B, 4.0)
        wst = torch.empty(max(1, ops.ip_bwd_data_xbar_workspace(M, N, K, cfg)), dtype=torch.uint8, device="cuda")
        wsf = torch.empty(max(1, ops.ip_fwd_xbar_workspace(M, K, N, cfg)), dtype=torch.uint8, device="cuda")
        fns = [lambda: ops.ip_bwd_data_xbar(dy, w, dx, M, N, K, cfg, workspace=wst),
               lambda: ops.ip_bwd(x, w, dy, None, None, dx, M, N, K),
               lambda: ops.ip_fwd_xbar(dy, wm, None, dx, M, K, N, cfg, workspace=wsf)]
        ids = [ops.ip_bwd_data_xbar_kernel_ids(M, N, K, cfg, ws_bytes=wst.numel()),
               ops.ip_bwd_kernel_ids(M, N, K, dw=False, db=False),
               ops.ip_fwd_xbar_kernel_ids(M, K, N, cfg, ws_bytes=wsf.numel())]
        for f in fns:
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t = [[], [], []]
        for _ in range(REPS):
            for i, f in enumerate(fns):
                t[i].append(window(f))
        med = [sorted(v)[REPS // 2] for v in t]
        cols = [f"{med[i]:.1f} ({min(t[i]):.1f}..{max(t[i]):.1f}) {','.join(ids[i])}" for i in range(3)]
        lines.append(f"{name}  {M} x {N} x {K}  {C} {B} | " + " | ".join(cols) +
                     f" | {med[0] / med[1]:.2f} | {med[0] / med[2]:.2f}")
    return lines


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if a not in flags]
    opt = dict(f[2:].split("=", 1) for f in flags if "=" in f)
    rows = conv_rows if "--conv" in flags else serial_rows if "--serial" in flags else ip_rows
    if "--backward" in flags:
        rows = backward_rows
    if "--serial-sliced" in flags:
        rows = serial_sliced_rows
    if "--sliced" in flags:
        rows = lambda: sliced_rows(opt.get("shape"), int(opt.get("cells", 0)))  # noqa: E731
    text = "\n".join(rows()) + "\n"
    print(text, end="")
    if args:
        Path(args[0]).write_text(text)


if __name__ == "__main__":
    main()
