"""The digit-serial read-out of the bit-sliced crossbar (rram_ip_fwd_xbar_ss) against a numpy loop
over crossbar tiles, input digits and weight slices, bit for bit: integers plus three rounded float operations
per output, so there is no tolerance anywhere.  xs and ws are powers of two and kf = 2^h / 3; with an 8-bit ADC
no pair clips while R (2^db - 1) (2^cb - 1) 2^h / 3 <= 127.5, which is where each case's h comes from."""
import numpy as np
import pytest
from _xbar_cases import IP_NET, dev, grid, ref_ss, run_net, same_bits

gpu = pytest.mark.gpu
f32 = np.float32


def cfgs(R, B, b, wb, cb, h, e=-5, f=-5):
    """((rows, adc_bits, adc_range, dac_bits, dac_range), (weight_bits, cell_bits, weight_range)): xs = 2^e,
    ws = 2^f, kf = 2^h / 3."""
    qmax = 2 ** (B - 1) - 1
    return ((R, B, qmax * 3.0 * 2.0 ** (e + f - h), b, (2 ** (b - 1) - 1) * 2.0 ** e),
            (wb, cb, (2 ** (wb - 1) - 1) * 2.0 ** f))


def run(x, w, bias, cfg, sl, db, relu=False, split_k=0, unaligned=False):
    import torch
    from rramsim import ops
    (M, K), N = x.shape, w.shape[0]
    c, s = ops.xbar_cfg(*cfg), ops.xbar_slices(*sl)
    y = torch.full((M, N), float("nan"), device="cuda")
    ws = torch.empty(ops.ip_fwd_xbar_ss_workspace(M, N, K, c, s, db, split_k), dtype=torch.uint8, device="cuda")
    ops.ip_fwd_xbar_ss(dev(x, unaligned), dev(w, unaligned), None if bias is None else dev(bias), y, M, N, K, c, s,
                       db, relu=relu, split_k=split_k, workspace=ws)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def operands(M, N, K, kind, seed=1):
    g = np.random.default_rng(seed)
    if kind == "gauss":
        return g.standard_normal((M, K)).astype(f32), g.standard_normal((N, K)).astype(f32)
    if kind == "grid":       # half-code points: ties of both quantisers, their clamps, zero digits under a minus sign
        return grid((M, K), seed, -260, 260, 2.0 ** -6), grid((N, K), seed + 1, -260, 260, 2.0 ** -6)
    x, w = np.where(g.random((M, K)) < 0.5, f32(-8), f32(8)), np.where(g.random((N, K)) < 0.5, f32(-8), f32(8))
    x[0], w[0] = 8, 8                                    # "max": every code at +-max, |p[0][0]| = K cmax dmax
    return x, w


TWO, BIG = (70, 130, 100, 32), (40, 130, 1056, 32)
# (M, N, K, R), adc_bits, dac_bits, digit_bits, weight_bits, cell_bits, log2(3 kf), bias + relu, unaligned, operands
CASES = [((5, 3, 32, 32), 8, 4, 3, 3, 2, -1, False, False, "gauss"),      # one digit, one slice, one tile
         (TWO, 8, 8, 2, 8, 2, 0, True, False, "gauss"),                   # 2 x 2 tiles, short last tile, digits 2,2,2,1
         (TWO, 8, 8, 2, 8, 2, 0, True, False, "grid"),
         (BIG, 8, 8, 1, 8, 1, 3, True, False, "gauss"),                   # 7 x 7 pairs: 3 x 2 chunks, finish, 33 tiles
         ((40, 130, 1055, 32), 8, 8, 1, 8, 1, 3, True, True, "gauss"),    # ... the scalar packs
         (TWO, 4, 8, 2, 8, 2, 0, True, False, "gauss"),                   # the ADC clips
         ((33, 40, 1024, 1024), 16, 8, 7, 8, 7, -9, False, False, "max")]  # |p| reaches 1024 * 127 * 127


@gpu
@pytest.mark.parametrize("shape,B,b,db,wb,cb,h,full,unaligned,kind", CASES)
def test_bit_exact(device, shape, B, b, db, wb, cb, h, full, unaligned, kind):
    from rramsim import ops
    M, N, K, R = shape
    x, w = operands(M, N, K, kind)
    bias = grid((N,), 3) if full else None
    cfg, sl = cfgs(R, B, b, wb, cb, h)
    ref, clipped, pmax = ref_ss(x, w, bias, cfg, sl, db, full)
    assert clipped == (B == 4) and np.abs(ref).max() > 0
    assert kind != "max" or pmax == 1024 * 127 * 127
    got = run(x, w, bias, cfg, sl, db, full, unaligned=unaligned)
    assert same_bits(got, ref), np.abs(got - ref).max()
    if db == b - 1:                                      # one digit: the parallel DAC of rram_ip_fwd_xbar_ws
        import torch
        c, s, y = ops.xbar_cfg(*cfg), ops.xbar_slices(*sl), torch.full((M, N), float("nan"), device="cuda")
        ws = torch.empty(ops.ip_fwd_xbar_ws_workspace(M, N, K, c, s), dtype=torch.uint8, device="cuda")
        ops.ip_fwd_xbar_ws(dev(x), dev(w), None if bias is None else dev(bias), y, M, N, K, c, s, relu=full,
                           workspace=ws)
        assert same_bits(got, y.cpu().numpy())


@gpu
def test_split_independence(device):
    from rramsim import ops
    M, N, K, R = BIG
    x, w = operands(M, N, K, "gauss", 4)
    bias = grid((N,), 6)
    cfg, sl = cfgs(R, 8, 8, 8, 1, 3)
    ref = ref_ss(x, w, bias, cfg, sl, 1)[0]
    for split in (1, 2, 5, 33, 64):
        assert same_bits(run(x, w, bias, cfg, sl, 1, split_k=split), ref), split
        ids = ops.ip_fwd_xbar_ss_kernel_ids(M, N, K, ops.xbar_cfg(*cfg), ops.xbar_slices(*sl), 1, split_k=split,
                                            ws_bytes=1 << 30)
        assert ids == ["xbar:pack_sm8<vec>", "xbar:pack_wslices<vec>", "xbar:ip_ss<d3;p4>/s%d/c6" % min(split, 33),
                       "xbar:finish"], ids


MSG = ("crossbar_param { rows: 32 adc_bits: %d adc_range: %r dac_bits: 4 dac_range: 0.875 %s"
       "weight_slices { weight_bits: 4 cell_bits: 2 weight_range: 0.875 input_digit_bits: 2 } }")


@gpu
def test_layer_option_backward(device):
    x, w, b, dy = grid((37, 100), 7), grid((45, 100), 8), grid((45,), 9), grid((37, 45), 10)
    net = lambda xbar, opts=None: run_net(IP_NET.format(xbar=xbar), opts, x, w, b, dy)  # noqa: E731
    cfg, sl = (32, 6, 31 * 3 * 2.0 ** -4, 4, 0.875), (4, 2, 0.875)       # xs = ws = 2^-3, kf = 2^-2 / 3
    y = net(MSG % (cfg[1], cfg[2], ""))[0]
    assert same_bits(y, run(x, w, b, cfg, sl, 2, relu=True))
    assert same_bits(y, ref_ss(x, w, b, cfg, sl, 2, True)[0])
    opts = {"crossbar": "32,6,%r,4,0.875" % cfg[2], "crossbar_slices": "4,2,0.875,2"}
    assert same_bits(y, net("", opts)[0])
    plain = net("")
    assert not same_bits(y, plain[0])                                     # the ADC does round here
    # kf = 1 with 12 bits: the codes are the grids, nothing rounds or clips, so the plain net's y and diffs
    fine = net(MSG % (12, 2047 * 2.0 ** -6, ""))
    for a, p in zip(fine, plain):
        assert same_bits(a, p) and np.abs(a).max() > 0


CONV = ('layer { name: "x" type: "Input" top: "x" input_param { shape { dim: 4 dim: 5 dim: 6 dim: 6 } } }\n'
        'layer { name: "conv" type: "Convolution" bottom: "x" top: "y" %s convolution_param { num_output: 9 '
        'kernel_size: 3 pad: 1 } }\n')


def test_refusals_host_only():
    """No device is touched: the checks, the plan query and the layers' set-up are host code."""
    from rramsim import _kernels as K, caffe, ops
    ok_c, ok_s = (64, 8, 4.0, 8, 1.0), (8, 2, 1.0)

    def ids(c, s, db, Kdim=256, **kw):
        return ops.ip_fwd_xbar_ss_kernel_ids(8, 16, Kdim, ops.xbar_cfg(*c), ops.xbar_slices(*s), db, **kw)

    need = ops.ip_fwd_xbar_ss_workspace(8, 16, 256, ops.xbar_cfg(*ok_c), ops.xbar_slices(*ok_s), 2, 1)
    assert need == 8 * 4 * 4096 + 2 * 8 * 16 * 4         # the slice planes + two digit chunks' slabs
    assert ids(ok_c, ok_s, 2, split_k=1, ws_bytes=need) == ["xbar:pack_sm8<vec>", "xbar:pack_wslices<vec>",
                                                            "xbar:ip_ss<d2;p4>/s1/c2", "xbar:finish"]
    assert ids(ok_c, ok_s, 7, split_k=1, ws_bytes=need)[2] == "xbar:ip_ss<d2;p4>/s1/c1"
    for db in (0, 8, -1):
        with pytest.raises(K.RramError, match="digit_bits"):
            ids(ok_c, ok_s, db, ws_bytes=need)
    for c, s in [((64, 8, 4.0, 9, 1.0), ok_s), (ok_c, (8, 8, 1.0)), (ok_c, (8, 2, 0.0))]:   # what _ws refuses
        with pytest.raises(K.RramError):
            ids(c, s, 2, ws_bytes=need)
    with pytest.raises(K.RramError, match="workspace"):
        ids(ok_c, ok_s, 2, split_k=1, ws_bytes=need - 1)
    big = ((32, 16, 4.0, 8, 1.0), (8, 1, 1.0), 1)        # 4 * 32767 * 127 * 127 < 2^31 <= 5 * 32767 * 127 * 127
    assert ids(*big, Kdim=128, ws_bytes=1 << 30)
    with pytest.raises(K.RramError, match="overflows int32"):
        ids(*big, Kdim=160, ws_bytes=1 << 30)
    with pytest.raises(K.RramError, match="weight_slices with bit_serial is not served"):
        caffe.Net(IP_NET.format(xbar=MSG % (8, 4.0, "bit_serial: true ")), "train", None)
    with pytest.raises(K.RramError, match="weight_slices is not served for Convolution"):
        caffe.Net(CONV % (MSG % (8, 4.0, "")), "train", None)
    with pytest.raises(K.RramError, match="digit_bits"):
        caffe.Net(IP_NET.format(xbar=""), "train", {"crossbar": "32,8,4.0,4,1.0", "crossbar_slices": "4,2,1.0,4"})
