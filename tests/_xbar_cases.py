"""What the crossbar read-out tests (test_gpu_xbar*.py and the case matrix of
_xbar_matrix.py) share: exact-grid operands, aligned and one-float-off device
copies, the six numpy references (loops over crossbar tiles, planes, slices and
digits in float64 or int64 that know nothing of the kernels' layouts), the
InnerProduct entry-point runner and the three-layer net runner."""
import numpy as np

f32 = np.float32


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


def xbar_out(S, step, bias, relu=False):
    """The output stage every read-out documents: fl32(fl32(float32(S) * step) + bias), then ReLU (S int64)."""
    y = S.astype(f32) * f32(step)
    if bias is not None:
        y = y + bias.astype(f32)
    return (np.maximum(y, f32(0)) if relu else y).astype(f32)


def ref_xbar(x, w, bias, R, bits, rng, relu=False, dac=None):
    """(y float32, S int64, per-element count of tiles near a rounding tie, clipped anywhere)."""
    x, w = x.astype(np.float64), w.astype(np.float64)
    if dac:
        q = 2 ** (dac[0] - 1) - 1
        x = dac_codes(x, dac[1] / q, q) * (dac[1] / q)
    qmax = 2 ** (bits - 1) - 1
    step = float(np.float32(rng)) / qmax
    S = np.zeros((x.shape[0], w.shape[0]), np.int64)
    near = np.zeros(S.shape, np.int64)
    clipped = False
    for k0 in range(0, x.shape[1], R):
        q, n, c = adc_tile(x[:, k0:k0 + R], w[:, k0:k0 + R], step, qmax)
        S, near, clipped = S + q, near + n, clipped | c
    return xbar_out(S, step, bias, relu), S, near, clipped


def ref_bs(x, w, bias, R, B, A, b, X, relu=False):
    """(y float32, S int64, per-element count of near-tie (tile, plane) pairs, clipped anywhere)."""
    cmax, qmax = 2 ** (b - 1) - 1, 2 ** (B - 1) - 1
    xs, step = float(np.float32(X)) / cmax, float(np.float32(A)) / qmax
    c = np.clip(np.rint(x.astype(f32) / f32(xs)), -cmax, cmax).astype(np.int64)   # the header's float32 division
    w = w.astype(np.float64)
    S = np.zeros((x.shape[0], w.shape[0]), np.int64)
    near = np.zeros(S.shape, np.int64)
    clipped = False
    for k0 in range(0, x.shape[1], R):
        ct, wt = c[:, k0:k0 + R], w[:, k0:k0 + R]
        for j in range(b - 1):
            q, n, cl = adc_tile((np.sign(ct) * ((np.abs(ct) >> j) & 1)).astype(np.float64), wt, step, qmax)
            S, near, clipped = S + (q << j), near + n, clipped | cl
    return xbar_out(S, step * xs, bias, relu), S, near, clipped


def ref_ws(x, w, bias, cfg, sl, relu=False):
    """(y float32, whether any ADC code clipped, max |p|)."""
    (R, B, A, b, X), (wb, cb, Wr) = cfg, sl
    cmax, dmax, qmax = 2 ** (b - 1) - 1, 2 ** (wb - 1) - 1, 2 ** (B - 1) - 1
    A, X, Wr = float(f32(A)), float(f32(X)), float(f32(Wr))
    kf, out = f32(X / cmax * (Wr / dmax) / (A / qmax)), f32(A / qmax)
    c = np.clip(np.rint(x / f32(X / cmax)), -cmax, cmax).astype(np.int64)
    d = np.clip(np.rint(w / f32(Wr / dmax)), -dmax, dmax).astype(np.int64)
    S = np.zeros((x.shape[0], w.shape[0]), np.int64)
    clipped, pmax = False, 0
    for k0 in range(0, x.shape[1], R):
        ct, dt = c[:, k0:k0 + R], d[:, k0:k0 + R]
        for s in range(-(-(wb - 1) // cb)):
            p = ct @ (np.sign(dt) * ((np.abs(dt) >> (s * cb)) & (2 ** cb - 1))).T
            r = np.rint(p.astype(f32) * kf)
            clipped, pmax = clipped or bool((np.abs(r) > qmax).any()), max(pmax, int(np.abs(p).max()))
            S += np.clip(r, -qmax, qmax).astype(np.int64) << (s * cb)
    return xbar_out(S, out, bias, relu), clipped, pmax


def ref_ss(x, w, bias, cfg, sl, db, relu=False):
    """(y float32, whether any ADC code clipped, max |p|)."""
    (R, B, A, b, X), (wb, cb, Wr) = cfg, sl
    cmax, dmax, qmax = 2 ** (b - 1) - 1, 2 ** (wb - 1) - 1, 2 ** (B - 1) - 1
    A, X, Wr = float(f32(A)), float(f32(X)), float(f32(Wr))
    kf, out = f32(X / cmax * (Wr / dmax) / (A / qmax)), f32(A / qmax)
    c = np.clip(np.rint(x / f32(X / cmax)), -cmax, cmax).astype(np.int64)
    d = np.clip(np.rint(w / f32(Wr / dmax)), -dmax, dmax).astype(np.int64)
    S = np.zeros((x.shape[0], w.shape[0]), np.int64)
    clipped, pmax = False, 0
    for k0 in range(0, x.shape[1], R):
        ct, dt = c[:, k0:k0 + R], d[:, k0:k0 + R]
        for j in range(-(-(b - 1) // db)):
            cj = np.sign(ct) * ((np.abs(ct) >> (j * db)) & (2 ** db - 1))
            for s in range(-(-(wb - 1) // cb)):
                p = cj @ (np.sign(dt) * ((np.abs(dt) >> (s * cb)) & (2 ** cb - 1))).T
                r = np.rint(p.astype(f32) * kf)
                clipped, pmax = clipped or bool((np.abs(r) > qmax).any()), max(pmax, int(np.abs(p).max()))
                S += np.clip(r, -qmax, qmax).astype(np.int64) << (j * db + s * cb)
    assert np.abs(S).max() < 2 ** 31
    return xbar_out(S, out, bias, relu), clipped, pmax


def ref_bwd(dy, w, C, bits, rng, dac=None):
    """(dx float32, S int64, per-element count of tiles near a rounding tie, clipped anywhere)."""
    dy, w = dy.astype(np.float64), w.astype(np.float64)
    if dac:
        q = 2 ** (dac[0] - 1) - 1
        dy = dac_codes(dy, dac[1] / q, q) * (dac[1] / q)
    qmax = 2 ** (bits - 1) - 1
    step = float(np.float32(rng)) / qmax
    S = np.zeros((dy.shape[0], w.shape[1]), np.int64)
    near, clipped = np.zeros(S.shape, np.int64), False
    for n0 in range(0, dy.shape[1], C):
        q, n, c = adc_tile(dy[:, n0:n0 + C], w[n0:n0 + C].T, step, qmax)
        S, near, clipped = S + q, near + n, clipped | c
    return xbar_out(S, step, None), S, near, clipped


def im2col(x, g, geom):
    """[num * Ho * Wo][Kg] float64 columns of group g, k = (ci * kh + i) * kw + j; and (Ho, Wo)."""
    num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group = geom[:14]
    Cg = C // group
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    xp = np.zeros((num, Cg, H + 2 * ph, W + 2 * pw))
    xp[:, :, ph:ph + H, pw:pw + W] = x[:, g * Cg:(g + 1) * Cg]
    taps = [xp[:, :, i * dh:i * dh + (Ho - 1) * sh + 1:sh, j * dw:j * dw + (Wo - 1) * sw + 1:sw]
            for i in range(kh) for j in range(kw)]
    cols = np.stack(taps, axis=2)                                   # [num][Cg][kh*kw][Ho][Wo]
    return cols.transpose(0, 3, 4, 1, 2).reshape(num * Ho * Wo, Cg * kh * kw), (Ho, Wo)


def ref_conv(x, w, bias, geom, bits, rng, relu=False, dac=None):
    """(y float32 NCHW, S, per-output count of near-tie tiles, clipped anywhere, the plain float64 convolution)."""
    num, Cout, group, R = geom[0], geom[4], geom[13], geom[14]
    Ng = Cout // group
    out = [[], [], [], []]
    clipped = False
    for g in range(group):
        cols, (Ho, Wo) = im2col(x, g, geom)
        wg = w[g * Ng:(g + 1) * Ng].reshape(Ng, -1)
        y, S, near, c = ref_xbar(cols, wg, None if bias is None else bias[g * Ng:(g + 1) * Ng], R, bits, rng, relu, dac)
        clipped |= c
        for o, a in zip(out, (y, S, near, cols @ wg.astype(np.float64).T)):
            o.append(a.reshape(num, Ho, Wo, Ng).transpose(0, 3, 1, 2))
    return tuple(np.concatenate(o, axis=1) for o in out[:3]) + (clipped, np.concatenate(out[3], axis=1))


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
