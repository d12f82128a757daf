"""The transposed crossbar read-out of the InnerProduct input gradient
(rram_ip_bwd_data_xbar) against a float64 loop over tiles of C
array columns: bit for bit on exact grids, identical bits under every split
over N, within the near-tie count on Gaussian operands, through the layer
message and the Net option, and the refusals without a device."""
import numpy as np
import pytest
from _xbar_cases import IP_NET, dev, grid, ref_bwd, run_net, same_bits

gpu = pytest.mark.gpu


def run_bwd(dy, w, cfg_args, split_k=0, unaligned=False):
    import torch
    from rramsim import ops
    (M, N), K = dy.shape, w.shape[1]
    cfg = ops.xbar_cfg(*cfg_args)
    dx = torch.full((M, K), float("nan"), device="cuda")
    ws = torch.empty(max(1, ops.ip_bwd_data_xbar_workspace(M, N, K, cfg, split_k)), dtype=torch.uint8, device="cuda")
    ops.ip_bwd_data_xbar(dev(dy, unaligned), dev(w, unaligned), dx, M, N, K, cfg, split_k=split_k, workspace=ws)
    torch.cuda.synchronize()
    return dx.cpu().numpy()


BIG = (40, 2068, 300, 64)     # 33 tiles of 64 columns, the last short; three column tiles of k
# (M, N, K, C), adc_bits, log2(step), unaligned, dac
EXACT = [((1, 1, 1, 32), 8, -2, False, None),
         ((33, 96, 130, 32), 8, -3, False, (4, 7 * 2.0 ** -3)),
         ((130, 300, 200, 128), 8, -2, False, None),
         ((5, 50, 10, 32), 4, -3, False, None),
         ((40, 2068, 301, 64), 8, -2, True, None),
         (BIG, 8, -2, False, None)]


@gpu
@pytest.mark.parametrize("shape,bits,e,unaligned,dac", EXACT)
def test_exact_grid_bit_exact(device, shape, bits, e, unaligned, dac):
    M, N, K, C = shape
    dy = grid((M, N), 1, -64, 64, 2.0 ** -6) if dac else grid((M, N), 1)
    w = grid((N, K), 2)                            # [N][K], never square beyond 1 x 1: a missed transpose cannot pass
    rng = (2 ** (bits - 1) - 1) * 2.0 ** e
    ref, _, _, clipped = ref_bwd(dy, w, C, bits, rng, dac)
    assert clipped == (bits == 4)                  # the 4-bit ADC must saturate somewhere
    got = run_bwd(dy, w, (C, bits, rng) + (dac or ()), unaligned=unaligned)
    assert same_bits(got, ref), np.abs(got - ref).max()


@gpu
def test_split_independence(device):
    from rramsim import ops
    M, N, K, C = BIG
    dy, w = grid((M, N), 4), grid((N, K), 5)
    cfg = (C, 8, 127 * 0.25)
    ref = ref_bwd(dy, w, C, 8, cfg[2])[0]
    for split in (1, 2, 5, 33, 64):
        assert same_bits(run_bwd(dy, w, cfg, split_k=split), ref), split
        ids = ops.ip_bwd_data_xbar_kernel_ids(M, N, K, ops.xbar_cfg(*cfg), split_k=split, ws_bytes=1 << 30)
        assert ids == ["xbar:pack<vec>", "xbar:ip_t<vec>/s%d" % min(split, 33)] + ["xbar:finish"] * (split > 1), ids


@gpu
def test_gaussian_boundary_aware(device):
    M, N, K, C, bits, step = 64, 1024, 96, 64, 10, 2.0 ** -2
    g = np.random.default_rng(11)
    dy, w = g.standard_normal((M, N)).astype(np.float32), g.standard_normal((N, K)).astype(np.float32)
    rng = (2 ** (bits - 1) - 1) * step
    _, S, near, clipped = ref_bwd(dy, w, C, bits, rng)
    assert (near > 0).mean() <= 0.02 and not clipped, ((near > 0).mean(), clipped)   # on the inputs, reference alone
    Sg = run_bwd(dy, w, (C, bits, rng)).astype(np.float64) / step
    assert np.array_equal(Sg, np.rint(Sg))
    bad = np.abs(Sg - S) > near
    assert not bad.any(), (int(bad.sum()), float(np.abs(Sg - S).max()))


BWD = "backward { cols: 32 adc_bits: 8 adc_range: 31.75 }"
# forwards that neither round nor clip these operands (test_gpu_xbar.py, test_gpu_xbar_bs.py): the plain net's y
FINE = "rows: 32 adc_bits: 12 adc_range: %r " % (2047 * 2.0 ** -6)
FINE_BS = "rows: 32 adc_bits: 12 adc_range: %r dac_bits: 4 dac_range: 0.875 bit_serial: true " % (2047 * 2.0 ** -3)


@gpu
def test_layer_message_option_bit_serial(device):
    x, w, b, dy = grid((37, 100), 7), grid((45, 100), 8), grid((45,), 9), grid((37, 45), 10)
    net = lambda xbar, opts=None: run_net(IP_NET.format(xbar=xbar), opts, x, w, b, dy)  # noqa: E731
    plain, got = net(""), net("crossbar_param { %s%s }" % (FINE, BWD))
    for i in (0, 2, 3):                                                   # y, dw, db: the plain net's
        assert same_bits(got[i], plain[i]) and np.abs(got[i]).max() > 0
    direct = run_bwd(dy * (got[0] > 0), w, (32, 8, 31.75))                # the in-place ReLU's backward, then the read
    assert same_bits(got[1], direct) and not same_bits(got[1], plain[1])  # the ADC does round here
    for other in (net("crossbar_param { %s}" % FINE, {"crossbar_backward": "32,8,31.75"}),
                  net("crossbar_param { %s%s }" % (FINE_BS, BWD))):
        for a, g in zip(other, got):
            assert same_bits(a, g)


CONV = ('layer { name: "x" type: "Input" top: "x" input_param { shape { dim: 4 dim: 5 dim: 6 dim: 6 } } }\n'
        'layer { name: "conv" type: "Convolution" bottom: "x" top: "y" %s convolution_param { num_output: 9 '
        'kernel_size: 3 pad: 1 } }\n')


def test_refusals_host_only():
    """No device is touched: the checks, the plan query and the layers' set-up are host code."""
    import ctypes as C
    from rramsim import _kernels as K, caffe, ops
    lib, p = K.load(), C.c_void_p(1 << 20)

    def call(cfg, shape=(8, 256, 16), split_k=0, ws_bytes=0):
        return lib.rram_ip_bwd_data_xbar(p, p, p, *shape, C.byref(ops.xbar_cfg(*cfg)), split_k, p if ws_bytes else None,
                                         ws_bytes, None)

    ok = (64, 8, 4.0)
    for cfg in [(48, 8, 4.0), (0, 8, 4.0), (2048, 8, 4.0), (64, 1, 4.0), (64, 17, 4.0), (64, 8, 0.0),
                (64, 8, float("nan")), (64, 8, 4.0, 1, 1.0), (64, 8, 4.0, 4, 0.0)]:
        assert call(cfg) == K.RRAM_EINVAL, cfg
    assert call(ok, (8, 0, 16)) == K.RRAM_EINVAL                          # nothing to sum over
    assert call((32, 16, 4.0), (1, 32 * 65539, 1)) == K.RRAM_EINVAL       # 65539 tiles x 32767 >= 2^31
    assert ops.ip_bwd_data_xbar_kernel_ids(1, 32 * 65538, 1, ops.xbar_cfg(32, 16, 4.0))[1] == "xbar:ip_t<scalar>/s1"
    assert call(ok, (65536, 32, 32768)) == K.RRAM_EINVAL                  # M K = 2^31
    assert call(ok, (0, 256, 16)) == K.RRAM_OK and call(ok, (8, 256, 0)) == K.RRAM_OK
    need = ops.ip_bwd_data_xbar_workspace(8, 256, 16, ops.xbar_cfg(*ok), 4)
    assert need == 4 * 8 * 16 * 4
    assert call(ok, split_k=4, ws_bytes=need - 1) == K.RRAM_EINVAL and call(ok, split_k=-1) == K.RRAM_EINVAL
    assert ops.ip_bwd_data_xbar_kernel_ids(8, 256, 16, ops.xbar_cfg(*ok)) == ["xbar:pack<vec>", "xbar:ip_t<vec>/s1"]
    assert ops.ip_bwd_data_xbar_kernel_ids(8, 250, 18, ops.xbar_cfg(*ok), split_k=9, ws_bytes=4 * 8 * 18 * 4) == \
        ["xbar:pack<scalar>", "xbar:ip_t<scalar>/s4", "xbar:finish"]
    xbar = "crossbar_param { rows: 32 adc_bits: 8 adc_range: 4.0 %s }"
    with pytest.raises(K.RramError, match="ip: crossbar_param backward: ip_bwd_data_xbar: rows 48"):
        caffe.Net(IP_NET.format(xbar=xbar % "backward { cols: 48 adc_bits: 8 adc_range: 4.0 }"), "train", None)
    with pytest.raises(K.RramError, match="backward is not served for Convolution"):
        caffe.Net(CONV % (xbar % BWD), "train", None)
    with pytest.raises(K.RramError, match="backward is not served for Convolution"):
        caffe.Net(CONV % "", "train", {"crossbar_conv": "32,8,4.0", "crossbar_backward": "32,8,4.0"})
