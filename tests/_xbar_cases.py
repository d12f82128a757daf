"""What the crossbar read-out tests (test_gpu_xbar.py, test_gpu_xbar_conv.py,
test_gpu_xbar_bs.py) share: exact-grid operands, aligned and one-float-off
device copies, the float64 DAC and ADC arithmetic of their references, the
InnerProduct entry-point runner and the three-layer net runner."""
import numpy as np


def grid(shape, seed, lo=-7, hi=7, scale=2.0 ** -3):
    return (np.random.default_rng(seed).integers(lo, hi + 1, shape) * scale).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev(a, unaligned=False):
    """a on the GPU; unaligned: as a view one float past an aligned allocation."""
    import torch
    t = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = t[1:] if unaligned else t[:-1]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    return v.view(*a.shape)


def dac_codes(x, xs, cmax):
    """The DAC's integer codes clamp(rint(x / xs), +-cmax), as float64."""
    return np.clip(np.rint(x / xs), -cmax, cmax)


def adc_tile(a, wt, step, qmax):
    """One crossbar tile's column sums a @ wt.T through the ADC: (codes int64, per-element 1 where the sum is
    within 1e-6 sum|a w| / step of a rounding tie below the clamp, whether any code clipped)."""
    r = (a @ wt.T) / step
    margin = 1e-6 * (np.abs(a) @ np.abs(wt).T) / step
    near = (np.abs(np.abs(r) % 1.0 - 0.5) <= margin) & (np.abs(r) < qmax + 1)
    clipped = bool((np.abs(np.rint(r)) > qmax).any())
    return np.clip(np.rint(r), -qmax, qmax).astype(np.int64), near, clipped


def run_ip(fn, x, w, bias, cfg_args, relu=False, split_k=0, unaligned=False):
    """ops.<fn> (fn = "ip_fwd_xbar" or "ip_fwd_xbar_bs") on device copies of the operands, y as numpy."""
    import torch
    from rramsim import ops
    M, K = x.shape
    N = w.shape[0]
    cfg = ops.xbar_cfg(*cfg_args)
    y = torch.full((M, N), float("nan"), device="cuda")
    ws = torch.empty(max(1, getattr(ops, fn + "_workspace")(M, N, K, cfg, split_k)), dtype=torch.uint8, device="cuda")
    getattr(ops, fn)(dev(x, unaligned), dev(w, unaligned), None if bias is None else dev(bias), y, M, N, K, cfg,
                     relu=relu, split_k=split_k, workspace=ws)
    torch.cuda.synchronize()
    return y.cpu().numpy()


IP_NET = ('force_backward: true\n'
          'layer {{ name: "x" type: "Input" top: "x" input_param {{ shape {{ dim: 37 dim: 100 }} }} }}\n'
          'layer {{ name: "ip" type: "InnerProduct" bottom: "x" top: "y" {xbar} inner_product_param {{ num_output: 45 '
          'weight_filler {{ type: "uniform" }} bias_filler {{ type: "uniform" }} }} }}\n'
          'layer {{ name: "relu" type: "ReLU" bottom: "y" top: "y" }}\n')


def run_net(proto, options, x, w, b, dy):
    """(y, dx, dw, db) of a net x -> one layer with weights and bias -> y on the given blobs."""
    import torch
    from rramsim import caffe
    caffe.set_stream_from_torch()
    net = caffe.Net(proto, "train", options)
    ps = net.params()
    for t, a in ((net.blob("x"), x), (ps[0]["data"], w), (ps[1]["data"], b)):
        t.copy_(torch.from_numpy(a).reshape(t.shape))
    net.clear_param_diffs()
    net.forward()
    y = net.blob("y").cpu().numpy()
    net.blob("y", diff=True).copy_(torch.from_numpy(dy))
    net.backward()
    out = (y, net.blob("x", diff=True).cpu().numpy(), ps[0]["diff"].cpu().numpy(), ps[1]["diff"].cpu().numpy())
    net.close()
    return out
