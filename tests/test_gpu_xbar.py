"""The crossbar-tiled InnerProduct forward (rram_ip_fwd_xbar)
against a float64 loop over crossbar tiles: bit-exact on inputs whose every
product, partial sum and p / step is exact in fp32; within the number of
near-tie tiles on Gaussian inputs; identical bits under every split over K;
and through the InnerProduct layer, the Net option and the Monte-Carlo driver."""
import numpy as np
import pytest
from _xbar_cases import IP_NET, grid, ref_xbar, run_ip, run_net

gpu = pytest.mark.gpu


def run_xbar(x, w, bias, cfg_args, relu=False, split_k=0, unaligned=False):
    return run_ip("ip_fwd_xbar", x, w, bias, cfg_args, relu, split_k, unaligned)


BIG = (40, 300, 2068, 64)     # 33 tiles, the last short; several workgroup tiles
# (M, N, K, R), adc_bits, log2(step), bias, relu, unaligned, dac
EXACT = [((1, 1, 1, 32), 8, -2, True, False, False, None),
         ((33, 130, 96, 32), 8, -2, False, True, False, None),
         ((33, 130, 96, 32), 4, -3, True, True, False, None),
         ((33, 130, 96, 32), 8, -3, True, False, False, (4, 7 * 2.0 ** -3)),
         ((70, 200, 300, 128), 8, -2, True, False, False, None),
         ((70, 200, 300, 128), 12, -6, False, False, True, None),
         ((5, 10, 50, 32), 8, -2, True, True, False, None),
         (BIG, 8, -2, True, True, False, None),
         (BIG, 8, -2, False, False, True, None)]


@gpu
@pytest.mark.parametrize("shape,bits,e,bias,relu,unaligned,dac", EXACT)
def test_exact_grid_bit_exact(device, shape, bits, e, bias, relu, unaligned, dac):
    M, N, K, R = shape
    x = grid((M, K), 1, -64, 64, 2.0 ** -6) if dac else grid((M, K), 1)
    w, b = grid((N, K), 2), (grid((N,), 3) if bias else None)
    rng = (2 ** (bits - 1) - 1) * 2.0 ** e
    ref, _, _, clipped = ref_xbar(x, w, b, R, bits, rng, relu, dac)
    assert clipped == (bits == 4)                  # the 4-bit ADC must saturate somewhere
    got = run_xbar(x, w, b, (R, bits, rng) + (dac or ()), relu, unaligned=unaligned)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()


@gpu
def test_split_independence(device):
    from rramsim import ops
    M, N, K, R = BIG
    x, w, b = grid((M, K), 4), grid((N, K), 5), grid((N,), 6)
    cfg = (R, 8, 127 * 0.25)
    ref = ref_xbar(x, w, b, R, 8, cfg[2])[0]
    for split in (1, 2, 5, 33, 64):
        got = run_xbar(x, w, b, cfg, split_k=split)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), split
        ids = ops.ip_fwd_xbar_kernel_ids(M, N, K, ops.xbar_cfg(*cfg), split_k=split, ws_bytes=1 << 30)
        assert ("xbar:finish" in ids) == (split > 1), ids
        assert any(i.startswith("xbar:ip<vec>/s%d" % min(split, 33)) for i in ids), ids


@gpu
@pytest.mark.parametrize("shape,bits,e", [((64, 96, 1024, 64), 10, -2), ((17, 40, 9216, 128), 8, 1)])
def test_gaussian_boundary_aware(device, shape, bits, e):
    M, N, K, R = shape
    g = np.random.default_rng(11)
    x, w = g.standard_normal((M, K)).astype(np.float32), g.standard_normal((N, K)).astype(np.float32)
    step = 2.0 ** e
    rng = (2 ** (bits - 1) - 1) * step
    _, S, near, _ = ref_xbar(x, w, None, R, bits, rng)
    assert (near > 0).mean() <= 0.02, (near > 0).mean()     # a condition on the inputs, from the reference alone
    Sg = run_xbar(x, w, None, (R, bits, rng)).astype(np.float64) / step
    assert np.array_equal(Sg, np.rint(Sg))
    bad = np.abs(Sg - S) > near
    assert not bad.any(), (int(bad.sum()), float(np.abs(Sg - S).max()))


def _net(xbar="", options=None, x=None, w=None, b=None, dy=None):
    return run_net(IP_NET.format(xbar=xbar), options, x, w, b, dy)


@gpu
def test_layer_forward_option_backward(device):
    x, w, b, dy = grid((37, 100), 7), grid((45, 100), 8), grid((45,), 9), grid((37, 45), 10)
    ref = ref_xbar(x, w, b, 32, 8, 127 * 0.25, relu=True)[0]
    msg = "crossbar_param { rows: 32 adc_bits: 8 adc_range: 31.75 }"
    y = _net(msg, None, x, w, b, dy)[0]
    assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(y, run_xbar(x, w, b, (32, 8, 31.75), relu=True))
    assert not np.array_equal(y, _net("", None, x, w, b, dy)[0])           # the ADC does round here
    assert np.array_equal(y, _net("", {"crossbar": "32,8,31.75"}, x, w, b, dy)[0])
    # step 2^-6 with 12 bits neither rounds nor clips these inputs: the same y, so the
    # straight-through backward must give the plain net's diffs
    fine = _net("crossbar_param { rows: 32 adc_bits: 12 adc_range: %r }" % (2047 * 2.0 ** -6), None, x, w, b, dy)
    plain = _net("", None, x, w, b, dy)
    for a, p in zip(fine, plain):
        assert np.array_equal(a.view(np.uint32), p.view(np.uint32)) and np.abs(a).max() > 0


@gpu
def test_map_batch_equals_sequential(device):
    import torch
    from rramsim import caffe, make_inject_cfg, models
    caffe.set_stream_from_torch()
    B, K, MAPS = 20, 2, 3
    opts = models.net_options("lenet", crossbar="64,8,8.0")

    def stats(net, **kw):
        mc = caffe.MonteCarlo(net, make_inject_cfg(0.05), seed=5, max_maps=8, **kw)
        if kw:
            mc.tile_inputs()
        mc.run(0, MAPS)
        st = mc.stats()
        mc.close()
        return st

    caffe.set_random_seed(1701)
    seq = caffe.Net(models.lenet(test_batch=B), "test", opts)
    caffe.set_random_seed(1701)
    plain = caffe.Net(models.lenet(test_batch=B), "test", models.net_options("lenet"))
    caffe.set_random_seed(1701)
    bat = caffe.Net(models.lenet(test_batch=K * B), "test", opts)
    for p, q in zip(bat.params(), seq.params()):
        p["data"].copy_(q["data"])
    for k in ("data", "label"):
        bat.blob(k)[:B].copy_(seq.blob(k))
    want, got, base = stats(seq), stats(bat, map_batch=K), stats(plain)
    assert got["per_map"] == want["per_map"] and got["broken"] == want["broken"]
    assert want["per_map"] != base["per_map"]                # the read-out is in the path
    for n in (seq, plain, bat):
        n.close()


def test_invalid_configurations_host_only():
    """No device is touched: the checks and the plan query are host code."""
    import ctypes as C
    from rramsim import _kernels as K, ops
    lib = K.load()
    p = C.c_void_p(1 << 20)

    def call(cfg, transpose=0, split_k=0, ws_bytes=0):
        return lib.rram_ip_fwd_xbar(p, p, None, p, 8, 16, 256, transpose, C.byref(ops.xbar_cfg(*cfg)), 0, split_k,
                                    p if ws_bytes else None, ws_bytes, None)

    bad = [(48, 8, 4.0), (0, 8, 4.0), (2048, 8, 4.0), (64, 1, 4.0), (64, 17, 4.0), (64, 8, 0.0), (64, 8, float("nan")),
           (64, 8, 4.0, 1, 1.0), (64, 8, 4.0, 4, 0.0)]
    for cfg in bad:
        assert call(cfg) == K.RRAM_EINVAL, cfg
    assert call((64, 8, 4.0), transpose=1) == K.RRAM_EINVAL
    need = ops.ip_fwd_xbar_workspace(8, 16, 256, ops.xbar_cfg(64, 8, 4.0), 4)
    assert need == 4 * 8 * 16 * 4
    assert call((64, 8, 4.0), split_k=4, ws_bytes=need - 1) == K.RRAM_EINVAL
    assert ops.ip_fwd_xbar_kernel_ids(8, 16, 256, ops.xbar_cfg(64, 8, 4.0)) == ["xbar:pack<vec>", "xbar:ip<vec>/s1"]
    assert ops.ip_fwd_xbar_kernel_ids(8, 16, 250, ops.xbar_cfg(64, 8, 4.0), split_k=9, ws_bytes=need) == \
        ["xbar:pack<scalar>", "xbar:ip<scalar>/s4", "xbar:finish"]
