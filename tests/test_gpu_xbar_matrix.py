"""Every case of tests/_xbar_matrix.py (every crossbar kernel instantiation and
plan branch, see tests/test_xbar_kernel_coverage.py) on the GPU against its
numpy reference, bit for bit, with guards around the output and the workspace:

  y (dx) is a view in the middle of a larger buffer of sentinel words, itself
  pre-filled with NaN: afterwards no sentinel has changed and no NaN is left;
  the workspace is exactly the *_workspace query's byte count inside a larger
  sentinel-filled allocation (16-byte aligned for ws / ss, which require it, 4
  bytes past that otherwise): the bytes before and after it are unchanged.

Two cross-checks need no reference: ss with one digit equals ws, and bs equals
ip under an ADC that changes nothing."""
import numpy as np
import pytest
from _xbar_cases import dev, f32, ref_bs, same_bits
from _xbar_matrix import (LABELS, WIDE_DELTA, XBAR_CASES, _adc, _desc, counts, query, reference, taps, wide,
                          wide_ok)

gpu = pytest.mark.gpu
GUARD = 1 << 16                 # sentinel floats on either side of y: more than 128 rows of the widest case
WS_GUARD = 1 << 12              # sentinel bytes on either side of the workspace
SENTINEL = -0x21524111          # 0xDEADBEEF as int32: no NaN, no value a read-out produces


def run_case(c, x, w, bias, entry=None):
    """The case through its entry point (or through `entry`, for the cross-checks), y as numpy; the guards are
    asserted here."""
    import torch
    from rramsim import ops
    e = entry or c["entry"]
    c = dict(c, entry=e)
    cfg = ops.xbar_cfg(*c["cfg"])
    if e == "conv":
        d = _desc(c["geom"])
        shape = (c["geom"][0], c["geom"][4], d.out_h, d.out_w)
    else:
        M, N, K = c["shape"]
        shape = (M, K) if e == "bwd" else (M, N)
    total = int(np.prod(shape))
    buf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    y = buf[GUARD:GUARD + total].view(torch.float32)
    y.fill_(float("nan"))
    need = query(c, "workspace")
    off = WS_GUARD + (0 if e in ("ws", "ss") else 4)
    wbuf = torch.full((need + 2 * WS_GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = wbuf[off:off + need] if need else None
    assert wbuf.data_ptr() % 16 == 0
    xd, wd = dev(np.array(x), not c["xa"]), dev(np.array(w), not c["wa"])    # copies: the cached operands are read-only
    bd = None if bias is None else dev(np.array(bias))
    kw = dict(split_k=c["split"], workspace=ws)
    yv = y.view(*shape)
    if e == "conv":
        ops.conv_fwd_xbar(d, xd, wd, bd, yv, cfg, relu=c["relu"], **kw)
    elif e == "bwd":
        ops.ip_bwd_data_xbar(xd, wd, yv, M, N, K, cfg, **kw)
    elif e in ("ws", "ss"):
        sl = ops.xbar_slices(*c["sl"])
        if e == "ws":
            ops.ip_fwd_xbar_ws(xd, wd, bd, yv, M, N, K, cfg, sl, relu=c["relu"], **kw)
        else:
            ops.ip_fwd_xbar_ss(xd, wd, bd, yv, M, N, K, cfg, sl, c["db"], relu=c["relu"], **kw)
    else:
        getattr(ops, "ip_fwd_xbar" + ("_bs" if e == "bs" else ""))(xd, wd, bd, yv, M, N, K, cfg, relu=c["relu"], **kw)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + total:] == SENTINEL).all()), \
        "a store outside y"
    assert bool((wbuf[:off] == 0xA5).all()) and bool((wbuf[off + need:] == 0xA5).all()), "a store outside the workspace"
    got = y.cpu().numpy().reshape(shape)
    assert not np.isnan(got).any(), "an output was not written"
    return got


@gpu
@pytest.mark.parametrize("label", LABELS)
def test_case_bit_exact(device, label):
    c = XBAR_CASES[LABELS.index(label)]
    x, w, bias, ref = reference(label)          # asserts the case's reference-side conditions first
    got = run_case(c, x, w, bias)
    assert same_bits(got, ref), (int((got.view(np.uint32) != ref.view(np.uint32)).sum()), np.abs(got - ref).max())
    if c["entry"] == "ss" and counts(c)[1] == 1:                  # one digit: the parallel DAC of rram_ip_fwd_xbar_ws
        assert same_bits(got, run_case(c, x, w, bias, entry="ws"))


@gpu
@pytest.mark.parametrize("shape,R,b,cmax,pairs,aligned", [((33, 130, 96), 32, 3, 3, 3, True),
                                                          ((66, 70, 213), 32, 6, 15, 1, False),
                                                          ((5, 10, 600), 256, 6, 15, 1, True)])
def test_bit_serial_equals_parallel_under_a_fine_adc(device, shape, R, b, cmax, pairs, aligned):
    """bs = ip when neither ADC rounds or clips, on the wide_w operand: w = n 2^-18 with |n| in [2^16, 2^19) and
    the codes +c, -c on pairs of neighbouring weights that differ by at most 2^11 quanta.  Both ADCs run 16 bits at
    their sums' quantum (2^-18 per plane; times xs for the parallel read-out), so a tile may hold pairs |c| 2^11
    <= 32767 steps, and the parallel read-out's partial sums stay fp32 numbers while 1.02 sum |c| |n| <= 2^24: 3 pairs
    of codes up to 3 on <p4>, one pair of codes up to 15 (of 31) on <p7>."""
    M, N, K = shape
    x = taps((M, K), 4, R, tuple(v * 2.0 ** -4 for v in range(1, cmax + 1)), pairs)
    w = wide((N, K), 5)
    bias = (np.random.default_rng(3).integers(-7, 8, N) * 0.125).astype(f32)
    assert pairs * cmax * WIDE_DELTA <= 32767 and wide_ok(x, w, R, 2.0 ** -22)
    base = dict(label="fine", shape=shape, sl=None, db=0, split=1, xa=aligned, wa=aligned, bias=True, relu=False)
    cb = dict(base, entry="bs", cfg=(R, 16, _adc(16, -18), b, _adc(b, -4)))
    cp = dict(base, entry="ip", cfg=(R, 16, _adc(16, -22), b, _adc(b, -4)))      # step' = step * xs
    a, p = run_case(cb, x, w, bias), run_case(cp, x, w, bias)
    y, _, _, clipped = ref_bs(x, w, bias, *cb["cfg"])
    assert not clipped and same_bits(a, y) and same_bits(a, p) and (a != bias).mean() > 0.5
    coarse = run_case(dict(cb, cfg=(R, 4, _adc(4, -18), b, _adc(b, -4))), x, w, bias)
    assert not same_bits(coarse, a)                      # the per-plane ADC is in the path
