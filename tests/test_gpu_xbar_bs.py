"""The bit-serial crossbar read-out (rram_ip_fwd_xbar_bs) against a
float64 loop over crossbar tiles and input bit planes: bit-exact on exact grids,
equal to the parallel read-out under an ADC that changes nothing, identical
under every split and chunking, within the near-tie count on Gaussian inputs,
through the InnerProduct layer, and refused where the header says so."""
import numpy as np
import pytest
from _xbar_cases import IP_NET, grid, ref_bs, run_ip as run, run_net, same_bits

gpu = pytest.mark.gpu


def cfg_of(R, B, e, b, ex):
    """(rows, adc_bits, adc_range, dac_bits, dac_range) with step = 2^e and xs = 2^ex."""
    return (R, B, (2 ** (B - 1) - 1) * 2.0 ** e, b, (2 ** (b - 1) - 1) * 2.0 ** ex)


def half_codes(shape, seed, b, ex):
    """x on half-code points i xs / 2, i in [-2 cmax - 4, 2 cmax + 4]: DAC ties and the clamp both occur."""
    n = 2 * (2 ** (b - 1) - 1) + 4
    return grid(shape, seed, -n, n, 2.0 ** (ex - 1))


MID, BIG = (33, 130, 96, 32), (40, 300, 2068, 64)
# (M, N, K, R), adc_bits, log2(step), dac_bits, bias + relu, unaligned
EXACT = [((1, 1, 1, 32), 8, -3, 2, False, False),       # one plane
         (MID, 8, -2, 8, True, False),                  # ragged M and N, one chunk of 7 planes
         (MID, 4, -2, 4, True, False),                  # the ADC clips
         ((5, 10, 50, 32), 8, -2, 3, False, True),      # short last tile, scalar loads
         ((70, 200, 300, 128), 12, -3, 5, False, False),
         (BIG, 8, -2, 12, True, False),                 # 33 tiles, two plane chunks, the finish kernel
         ((5, 10, 50, 32), 8, -2, 8, False, True)]      # short last tile, scalar loads, the 7-plane chunk
                                                        # (<scalar; p7>); last, so the ids above stay


@gpu
@pytest.mark.parametrize("shape,B,e,b,full,unaligned", EXACT)
def test_exact_grid_bit_exact(device, shape, B, e, b, full, unaligned):
    M, N, K, R = shape
    x, w, bias = half_codes((M, K), 1, b, -4), grid((N, K), 2), (grid((N,), 3) if full else None)
    cfg = cfg_of(R, B, e, b, -4)
    ref, S, _, clipped = ref_bs(x, w, bias, R, B, cfg[2], b, cfg[4], full)
    assert clipped == (B == 4) and np.abs(S).max() < 2 ** 24
    got = run("ip_fwd_xbar_bs", x, w, bias, cfg, full, unaligned=unaligned)
    assert same_bits(got, ref), np.abs(got - ref).max()


@gpu
def test_equals_parallel_readout_under_a_fine_adc(device):
    M, N, K, R = MID
    x, w, bias = half_codes((M, K), 1, 8, -4), grid((N, K), 2), grid((N,), 3)
    for B, same in ((16, True), (4, False)):
        bs = cfg_of(R, B, -3, 8, -4)
        par = cfg_of(R, B, -3 - 4, 8, -4)               # step' = step * xs
        a, p = run("ip_fwd_xbar_bs", x, w, bias, bs), run("ip_fwd_xbar", x, w, bias, par)
        assert same_bits(a, p) == same, B                # 4 bits: the per-plane ADC is in the path


@gpu
def test_split_and_chunk_independence(device):
    from rramsim import ops
    M, N, K, R = BIG
    x, w, bias = half_codes((M, K), 4, 12, -4), grid((N, K), 5), grid((N,), 6)
    cfg = cfg_of(R, 8, -2, 12, -4)
    ref = ref_bs(x, w, bias, R, 8, cfg[2], 12, cfg[4])[0]
    for split in (1, 2, 5, 33, 64):
        assert same_bits(run("ip_fwd_xbar_bs", x, w, bias, cfg, split_k=split), ref), split
        ids = ops.ip_fwd_xbar_bs_kernel_ids(M, N, K, ops.xbar_cfg(*cfg), split_k=split, ws_bytes=1 << 30)
        assert ids == ["xbar:pack_codes<vec>", "xbar:ip_bs<vec;p7>/s%d/c2" % min(split, 33), "xbar:finish"], ids


@gpu
@pytest.mark.parametrize("shape,B,e,b", [((64, 96, 1024, 64), 10, -2, 8), ((17, 40, 2304, 128), 8, 0, 6)])
def test_gaussian_boundary_aware(device, shape, B, e, b):
    M, N, K, R = shape
    g = np.random.default_rng(11)
    x, w = g.standard_normal((M, K)).astype(np.float32), g.standard_normal((N, K)).astype(np.float32)
    cfg = cfg_of(R, B, e, b, -5)
    _, S, near, clipped = ref_bs(x, w, None, R, B, cfg[2], b, cfg[4])
    assert (near > 0).mean() <= 0.05 and not clipped     # a condition on the inputs, from the reference alone
    Sg = run("ip_fwd_xbar_bs", x, w, None, cfg).astype(np.float64) / 2.0 ** (e - 5)
    assert np.array_equal(Sg, np.rint(Sg))
    print("max |S_gpu - S_ref|", np.abs(Sg - S).max(), "near share", (near > 0).mean())
    assert (np.abs(Sg - S) <= 2 ** (b - 2) * near).all()  # a tie on the highest plane moves S by 2^(b-2); none: equal


CONV = ('layer {{ name: "x" type: "Input" top: "x" input_param {{ shape {{ dim: 4 dim: 5 dim: 6 dim: 6 }} }} }}\n'
        'layer {{ name: "conv" type: "Convolution" bottom: "x" top: "y" {xbar} convolution_param {{ num_output: 9 '
        'kernel_size: 3 pad: 1 }} }}\n')


def _net(xbar, options, x, w, b, dy):
    return run_net(IP_NET.format(xbar=xbar), options, x, w, b, dy)


@gpu
def test_layer_forward_option_backward(device):
    x, w, b, dy = grid((37, 100), 7), grid((45, 100), 8), grid((45,), 9), grid((37, 45), 10)
    cfg = (32, 8, 31.75, 4, 0.875)
    msg = "crossbar_param { rows: 32 adc_bits: 8 adc_range: 31.75 dac_bits: 4 dac_range: 0.875 %s}"
    y = _net(msg % "bit_serial: true ", None, x, w, b, dy)[0]
    assert same_bits(y, run("ip_fwd_xbar_bs", x, w, b, cfg, relu=True))
    assert same_bits(y, _net("", {"crossbar": "32,8,31.75,4,0.875,1"}, x, w, b, dy)[0])
    par = _net(msg % "", None, x, w, b, dy)[0]
    assert same_bits(par, run("ip_fwd_xbar", x, w, b, cfg, relu=True)) and not same_bits(par, y)
    # step 2^-3 with 12 bits and xs 2^-3 change nothing here: the plain net's y, so the plain net's diffs
    fine = _net("crossbar_param { rows: 32 adc_bits: 12 adc_range: %r dac_bits: 4 dac_range: 0.875 bit_serial: true }"
                % (2047 * 2.0 ** -3), None, x, w, b, dy)
    for a, p in zip(fine, _net("", None, x, w, b, dy)):
        assert same_bits(a, p) and np.abs(a).max() > 0


def test_refusals_host_only():
    """No device is touched: the checks and the plan query are host code."""
    import ctypes as C
    from rramsim import _kernels as K, caffe, ops
    lib = K.load()
    p = C.c_void_p(1 << 20)

    def call(cfg, Kdim=256, transpose=0, split_k=0, ws_bytes=0):
        return lib.rram_ip_fwd_xbar_bs(p, p, None, p, 8, 16, Kdim, transpose, C.byref(ops.xbar_cfg(*cfg)), 0, split_k,
                                       p if ws_bytes else None, ws_bytes, None)

    ok = (64, 8, 4.0, 4, 1.0)
    bad = [(64, 8, 4.0), (48,) + ok[1:], (0,) + ok[1:], (2048,) + ok[1:], (64, 1, 4.0, 4, 1.0), (64, 17, 4.0, 4, 1.0),
           (64, 8, 0.0, 4, 1.0), (64, 8, float("nan"), 4, 1.0), (64, 8, 4.0, 1, 1.0), (64, 8, 4.0, 4, 0.0),
           (64, 8, 4.0, 17, 1.0)]
    for cfg in bad:
        assert call(cfg) == K.RRAM_EINVAL, cfg
    assert call(ok, transpose=1) == K.RRAM_EINVAL
    assert call((32, 16, 4.0, 16, 1.0), Kdim=96) == K.RRAM_EINVAL       # 3 * 32767^2 >= 2^31
    wide = ops.xbar_cfg(64, 8, 4.0, 12, 1.0)                            # 11 planes: two chunks
    assert ops.ip_fwd_xbar_bs_workspace(8, 16, 256, ops.xbar_cfg(*ok), 1) == 0
    need = ops.ip_fwd_xbar_bs_workspace(8, 16, 256, wide, 4)
    assert need == 4 * 2 * 8 * 16 * 4
    assert call((64, 8, 4.0, 12, 1.0), split_k=4, ws_bytes=need - 1) == K.RRAM_EINVAL
    assert ops.ip_fwd_xbar_bs_kernel_ids(8, 16, 256, ops.xbar_cfg(*ok)) == \
        ["xbar:pack_codes<vec>", "xbar:ip_bs<vec;p4>/s1/c1"]
    assert ops.ip_fwd_xbar_bs_kernel_ids(8, 16, 250, wide, split_k=9, ws_bytes=need) == \
        ["xbar:pack_codes<scalar>", "xbar:ip_bs<scalar;p7>/s4/c2", "xbar:finish"]
    flag = "crossbar_param { rows: 32 adc_bits: 8 adc_range: 4.0 dac_bits: 4 dac_range: 1.0 bit_serial: true }"
    with pytest.raises(K.RramError, match="bit_serial is not served for Convolution"):
        caffe.Net(CONV.format(xbar=flag), "train", None)
    with pytest.raises(K.RramError, match="bit_serial is not served for Convolution"):
        caffe.Net(CONV.format(xbar=""), "train", {"crossbar_conv": "32,8,4.0,4,1.0,1"})
