"""The crossbar-tiled Convolution forward (rram_conv2d_fwd_xbar)
against a float64 reference: a zero-padded strided-slice im2col per group, then
the loop over crossbar tiles of test_gpu_xbar.ref_xbar.  Bit-exact on inputs
whose every product, partial sum and p / step is exact in fp32; identical bits
under every split over K and every batch size; within the number of near-tie
tiles on Gaussian inputs; and through the Convolution layer and the Net option."""
import numpy as np
import pytest
from _xbar_cases import dev, grid, ref_conv, run_net

gpu = pytest.mark.gpu


def desc_of(geom):
    from rramsim import ops
    num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group = geom[:14]
    return ops.conv_desc((num, C, H, W), Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), group)


def run_conv(x, w, bias, geom, cfg_args, relu=False, split_k=0, unaligned=False):
    import torch
    from rramsim import ops
    d, cfg = desc_of(geom), ops.xbar_cfg(*cfg_args)
    y = torch.full((geom[0], geom[4], d.out_h, d.out_w), float("nan"), device="cuda")
    ws = torch.empty(max(1, ops.conv_fwd_xbar_workspace(d, cfg, split_k)), dtype=torch.uint8, device="cuda")
    ops.conv_fwd_xbar(d, dev(x, unaligned), dev(w, unaligned), None if bias is None else dev(bias), y, cfg,
                      relu=relu, split_k=split_k, workspace=ws)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def operands(geom, seeds, dac=False):
    num, C, H, W, Cout, kh, kw = geom[:7]
    x = grid((num, C, H, W), seeds[0], -64, 64, 2.0 ** -6) if dac else grid((num, C, H, W), seeds[0])
    return x, grid((Cout, C // geom[13], kh, kw), seeds[1]), grid((Cout,), seeds[0] + 2)


# (num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group, R)
ONE = (1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 32)
K45 = (3, 5, 7, 5, 33, 3, 3, 1, 1, 1, 1, 1, 1, 1, 32)        # tile boundary inside a channel's taps, 13-row last tile
GRP = (2, 8, 9, 11, 6, 5, 5, 2, 2, 2, 2, 1, 1, 2, 32)        # two groups, stride 2, Kg = 100
DIL = (2, 6, 10, 9, 10, 3, 2, 0, 1, 2, 1, 2, 2, 1, 32)       # non-square, mixed stride / pad, dilation 2
PW = (5, 70, 3, 3, 20, 1, 1, 0, 0, 1, 1, 1, 1, 1, 64)        # 1x1, a position tile spans images, Kg % 4 != 0
T12 = (2, 40, 12, 12, 130, 3, 3, 1, 1, 1, 1, 1, 1, 1, 32)    # 12 tiles, several position and channel tiles
# geom, adc_bits, log2(step), bias, relu, unaligned, dac
EXACT = [(ONE, 8, -2, True, False, False, None),
         (K45, 8, -2, False, True, False, None),
         (K45, 4, -3, True, True, False, None),
         (GRP, 8, -2, True, False, True, None),
         (DIL, 8, -2, False, False, False, None),
         (PW, 8, -2, True, True, True, None),
         (T12, 8, -2, True, True, False, None),
         (T12[:14] + (128,), 12, -6, False, False, True, None),
         (K45, 8, -2, True, False, False, (4, 7 * 2.0 ** -3))]


@gpu
@pytest.mark.parametrize("geom,bits,e,bias,relu,unaligned,dac", EXACT)
def test_exact_grid_bit_exact(device, geom, bits, e, bias, relu, unaligned, dac):
    x, w, b = operands(geom, (1, 2), dac)
    b = b if bias else None
    rng = (2 ** (bits - 1) - 1) * 2.0 ** e
    ref, _, _, clipped, plain = ref_conv(x, w, b, geom, bits, rng, relu, dac)
    assert clipped == (bits == 4)                  # the 4-bit ADC must saturate somewhere, no other case does
    if bits == 12:                                 # neither rounds nor clips: the plain float64 convolution
        assert np.array_equal(ref, plain.astype(np.float32))
    got = run_conv(x, w, b, geom, (geom[14], bits, rng) + (dac or ()), relu, unaligned=unaligned)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()


@gpu
def test_split_independence(device):
    from rramsim import ops
    x, w, b = operands(T12, (4, 5))
    cfg = (32, 8, 127 * 0.25)
    ref = ref_conv(x, w, b, T12, 8, cfg[2])[0]
    for split in (1, 2, 5, 12, 64):
        got = run_conv(x, w, b, T12, cfg, split_k=split)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), split
        ids = ops.conv_fwd_xbar_kernel_ids(desc_of(T12), ops.xbar_cfg(*cfg), split_k=split, ws_bytes=1 << 30)
        per = -(-12 // min(split, 12))                               # whole tiles per split: 5 asked -> 3 each, 4 splits
        assert ("xbar:finish" in ids) == (split > 1), ids
        assert ids[0] == "xbar:conv<vec>/s%d" % -(-12 // per) and (split < 64 or ids[0].endswith("/s12")), ids
    one = run_conv(x[:1], w, b, (1,) + T12[1:], cfg)                 # the first image alone
    assert np.array_equal(one.view(np.uint32), ref[:1].view(np.uint32))


@gpu
@pytest.mark.parametrize("geom,bits,e", [((2, 24, 10, 10, 40, 3, 3, 1, 1, 1, 1, 1, 1, 1, 64), 10, -2),
                                         ((4, 16, 13, 13, 24, 5, 5, 2, 2, 1, 1, 1, 1, 2, 128), 8, 0)])
def test_gaussian_boundary_aware(device, geom, bits, e):
    num, C, H, W, Cout, kh, kw = geom[:7]
    g = np.random.default_rng(11)
    x = g.standard_normal((num, C, H, W)).astype(np.float32)
    w = g.standard_normal((Cout, C // geom[13], kh, kw)).astype(np.float32)
    step = 2.0 ** e
    rng = (2 ** (bits - 1) - 1) * step
    _, S, near, _, _ = ref_conv(x, w, None, geom, bits, rng)
    assert (near > 0).mean() <= 0.02, (near > 0).mean()     # a condition on the inputs, from the reference alone
    Sg = run_conv(x, w, None, geom, (geom[14], bits, rng)).astype(np.float64) / step
    assert np.array_equal(Sg, np.rint(Sg))
    bad = np.abs(Sg - S) > near
    assert not bad.any(), (int(bad.sum()), float(np.abs(Sg - S).max()))


LAYER = (4, 5, 6, 6, 9, 3, 3, 1, 1, 1, 1, 1, 1, 1, 32)
NET = ('force_backward: true\n'
       'layer {{ name: "x" type: "Input" top: "x" input_param {{ shape {{ dim: 4 dim: 5 dim: 6 dim: 6 }} }} }}\n'
       'layer {{ name: "conv" type: "Convolution" bottom: "x" top: "y" {xbar} convolution_param {{ num_output: 9 '
       'kernel_size: 3 pad: 1 weight_filler {{ type: "uniform" }} bias_filler {{ type: "uniform" }} }} }}\n'
       'layer {{ name: "relu" type: "ReLU" bottom: "y" top: "y" }}\n')


def _net(xbar, options, x, w, b, dy):
    return run_net(NET.format(xbar=xbar), options, x, w, b, dy)


@gpu
def test_layer_option_backward(device):
    (x, w, b), dy = operands(LAYER, (7, 8)), grid((4, 9, 6, 6), 10)
    ref = ref_conv(x, w, b, LAYER, 8, 127 * 0.25, relu=True)[0]
    y = _net("crossbar_param { rows: 32 adc_bits: 8 adc_range: 31.75 }", None, x, w, b, dy)[0]
    assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(y, run_conv(x, w, b, LAYER, (32, 8, 31.75), relu=True))
    plain = _net("", None, x, w, b, dy)
    assert not np.array_equal(y, plain[0])                                 # the ADC does round here
    assert np.array_equal(y, _net("", {"crossbar_conv": "32,8,31.75"}, x, w, b, dy)[0])
    assert np.array_equal(plain[0], _net("", {"crossbar": "32,8,31.75"}, x, w, b, dy)[0])   # InnerProduct only
    # step 2^-6 with 12 bits neither rounds nor clips these inputs: the same y, so the
    # straight-through backward must give the plain net's diffs
    fine = _net("crossbar_param { rows: 32 adc_bits: 12 adc_range: %r }" % (2047 * 2.0 ** -6), None, x, w, b, dy)
    for a, p in zip(fine, plain):
        assert np.array_equal(a.view(np.uint32), p.view(np.uint32)) and np.abs(a).max() > 0


@gpu
def test_concat_and_pool_folds_decline(device):
    """TEST phase: max pool -> two sibling 1x1 crossbar convolutions -> Concat; the layer declines the
    Concat fold and the octet companions, so the Concat top is the two references side by side."""
    import torch
    from rramsim import caffe
    conv = ('layer {{ name: "{n}" type: "Convolution" bottom: "p" top: "{n}" convolution_param {{ num_output: {o} '
            'kernel_size: 1 weight_filler {{ type: "uniform" }} bias_filler {{ type: "uniform" }} }} }}\n')
    proto = ('layer { name: "x" type: "Input" top: "x" input_param { shape { dim: 2 dim: 8 dim: 8 dim: 8 } } }\n'
             'layer { name: "p" type: "Pooling" bottom: "x" top: "p" pooling_param { pool: MAX kernel_size: 2 '
             'stride: 2 } }\n' + conv.format(n="a", o=16) + conv.format(n="b", o=8) +
             'layer { name: "c" type: "Concat" bottom: "a" bottom: "b" top: "c" }\n')
    caffe.set_stream_from_torch()
    net = caffe.Net(proto, "test", {"crossbar_conv": "32,8,31.75"})
    x = grid((2, 8, 8, 8), 12)
    blobs = [grid((16, 8, 1, 1), 13), grid((16,), 14), grid((8, 8, 1, 1), 15), grid((8,), 16)]
    for t, a in [(net.blob("x"), x)] + [(p["data"], a) for p, a in zip(net.params(), blobs)]:
        t.copy_(torch.from_numpy(a).reshape(t.shape))
    net.forward()
    got = net.blob("c").cpu().numpy()
    net.close()
    pooled = x.reshape(2, 8, 4, 2, 4, 2).max(axis=(3, 5))
    want = [ref_conv(pooled, blobs[2 * i], blobs[2 * i + 1], (2, 8, 4, 4, o, 1, 1, 0, 0, 1, 1, 1, 1, 1, 32), 8, 31.75)[0]
            for i, o in enumerate((16, 8))]
    assert np.array_equal(got.view(np.uint32), np.concatenate(want, axis=1).view(np.uint32))


def test_invalid_configurations_host_only():
    """No device is touched: the checks and the plan query are host code."""
    import ctypes as C
    from rramsim import _kernels as K, caffe, ops
    lib = K.load()
    p = C.c_void_p(1 << 20)
    d = desc_of(K45)

    def call(cfg, desc=d, split_k=0, ws_bytes=0):
        return lib.rram_conv2d_fwd_xbar(C.byref(desc), p, p, None, p, C.byref(ops.xbar_cfg(*cfg)), 0, split_k,
                                        p if ws_bytes else None, ws_bytes, None)

    bad = [(48, 8, 4.0), (0, 8, 4.0), (2048, 8, 4.0), (64, 1, 4.0), (64, 17, 4.0), (64, 8, 0.0), (64, 8, float("nan")),
           (64, 8, 4.0, 1, 1.0), (64, 8, 4.0, 4, 0.0)]
    for cfg in bad:
        assert call(cfg) == K.RRAM_EINVAL, cfg
    big = K.ConvDesc(1, 3, 4, 4, 2, 7, 7, 1, 1, 1, 1, 1, 1, 1, 0, 0)            # kernel 7 > padded input 6
    assert call((64, 8, 4.0), desc=big) == K.RRAM_EINVAL
    need = ops.conv_fwd_xbar_workspace(d, ops.xbar_cfg(32, 8, 4.0), 2)
    assert need == 2 * 3 * 33 * 7 * 5 * 4
    assert call((32, 8, 4.0), split_k=2, ws_bytes=need - 1) == K.RRAM_EINVAL
    assert ops.conv_fwd_xbar_kernel_ids(desc_of(T12), ops.xbar_cfg(128, 8, 4.0), split_k=1) == ["xbar:conv<vec>/s1"]
    assert ops.conv_fwd_xbar_kernel_ids(d, ops.xbar_cfg(32, 8, 4.0), split_k=9, ws_bytes=need) == \
        ["xbar:conv<scalar>/s2", "xbar:finish"]
    with pytest.raises(K.RramError, match="rows 48"):
        caffe.Net(NET.format(xbar="crossbar_param { rows: 48 adc_bits: 8 adc_range: 4.0 }"), "train", None)
