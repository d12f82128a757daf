"""Times rram_ip_fwd_xbar beside rram_ip_fwd (the same MFMA count without the
per-tile rounding) on the fc6 / fc7 / CIFAR ip1 shapes: call times from device
events (pack, GEMM and finish / split-K reduce included), the two alternated
in one process, the median and range of REPS windows of ITERS calls each.

    python scripts/xbar_bench.py [out.txt]
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rram-caffe-simulation_amd" / "python"))

import torch  # noqa: E402

from rramsim import ops  # noqa: E402

ROOF = 2.5e15 / 6          # bf16 dense peak over the six products, FLOP/s of fp32-equivalent work
SHAPES = [("fc6", 256, 4096, 9216, 128, 8), ("fc7", 256, 4096, 4096, 128, 8), ("cifar ip1", 100, 64, 1024, 64, 8)]
ITERS, REPS = 50, 7


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3   # us per call


def main():
    assert torch.cuda.is_available(), "needs a GPU"
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
        for f in (fx, fp):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        tx, tp = [], []
        for _ in range(REPS):
            tx.append(window(fx))
            tp.append(window(fp))
        mx, mp = sorted(tx)[REPS // 2], sorted(tp)[REPS // 2]
        idx = ",".join(ops.ip_fwd_xbar_kernel_ids(M, N, K, cfg, ws_bytes=wsx.numel()))
        idp = ",".join(ops.ip_fwd_kernel_ids(M, N, K, relu=True, ws_bytes=wsp.numel()))
        lines.append(f"{name}  {M} x {N} x {K}  {R} {B} | {mx:.1f} ({min(tx):.1f}..{max(tx):.1f}) {idx} | "
                     f"{mp:.1f} ({min(tp):.1f}..{max(tp):.1f}) {idp} | {mx / mp:.2f} | "
                     f"{2.0 * M * N * K / (mx * 1e-6) / ROOF:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)


if __name__ == "__main__":
    main()
