"""Every reachable bf16x6 convolution kernel instantiation against fp64.

tests/_x6_cases.py holds, per kernel id (ops.conv_fwd_kernel_id: template
arguments, K-tile parity, tiling kind), the cheapest shape that selects it.
Each is run here with the id asserted again before the launch, so a broken
template form, a wrong parity epilogue, a short last tile or a lost product
term of one instantiation cannot hide behind the networks' own shapes.

Per case and relu in (False, True):
  canaries    y lies between 4096 sentinel floats on either side (bit-unchanged
              afterwards) and starts as NaN (none may remain);
  accuracy    |y - fp64| <= 1e-6 Σ|a·b| (the fp32-level bound of
              tests/test_gpu_fp32_guard.py; a lost bf16 term is ~2^-16), and
              _ref64.x6_guard_failures against the fp32-MFMA engine on the
              same data (<= 2 x its max and mean error);
  companions  channel-octet and 1x1 ids: conv2d_fwd_octets with and without
              the input companion gives y bit-identical to conv2d_fwd and the
              output companion equals octets_ref(y); with y = None (where
              ops.conv_output_octets_only) the same companion;
  strided     one case per family into a channel slice of a wider NCHW
              tensor: the slice equals y's bits, the rest is untouched;
  weight pack conv2d_fwd_cached, w_pack_valid False then True: y's bits.
"""
import numpy as np
import pytest

from _x6_cases import X6_CASES, desc, family
from test_gpu_octets import N, T, _as_u16, _oct_buf, octets_ref

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0x5A5AC3C3          # bit pattern of the canary floats (a finite value)
TOL = 1e-6                     # _ref64.X6_GUARD_MAX
OCTET_FAMILIES = ("cb", "cb16", "c1x1", "c1x1_dma")
# the first case of each family also runs the strided (Concat-fold) form
STRIDED = {}
for _i, _c in enumerate(X6_CASES):
    STRIDED.setdefault(family(_c["id"]), _i)

_DATA = {}


def _data(i):
    """Inputs and the fp64 reference of case i, computed once (shared by both relu runs)."""
    if i not in _DATA:
        from _ref64 import conv64
        cs = X6_CASES[i]
        rng = np.random.default_rng(1000 + i)
        x = rng.standard_normal(cs["x"]).astype(np.float32)
        w = (0.1 * rng.standard_normal((cs["cout"], cs["x"][1] // cs["g"], cs["k"], cs["k"]))).astype(np.float32)
        b = rng.standard_normal(cs["cout"]).astype(np.float32)
        ref, scale = conv64(x, w, b, cs["s"], cs["p"], cs["g"])
        _DATA[i] = (x, w, b, ref, scale)
    return _DATA[i]


def _guarded(shape, device, lead=0):
    """A NaN tensor of `shape` inside a sentinel buffer: (whole buffer as int32, the tensor)."""
    import torch
    n = int(np.prod(shape))
    big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
    y = big[GUARD:GUARD + n].view(torch.float32).view(shape)
    y.fill_(float("nan"))
    return big, y


def _sentinels_intact(big, what):
    import torch
    torch.cuda.synchronize()
    head, tail = big[:GUARD], big[-GUARD:]
    assert bool((head == SENTINEL).all()), f"{what}: wrote before y"
    assert bool((tail == SENTINEL).all()), f"{what}: wrote past y"


def _errs(got, ref, scale, relu):
    if relu:
        ref = np.maximum(ref, 0.0)
    r = np.abs(got.astype(np.float64) - ref) / np.maximum(scale, 1e-300)
    return float(r.max()), float(r.mean())


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("i", range(len(X6_CASES)), ids=[c["id"] for c in X6_CASES])
def test_kernel_instantiation(device, i, relu):
    import torch
    from rramsim import ops
    from _ref64 import assert_scaled, x6_guard_failures
    cs = X6_CASES[i]
    kid, fam = cs["id"], family(cs["id"])
    x, w, b, ref, scale = _data(i)
    d = desc(cs)
    yshape = (cs["x"][0], cs["cout"], d.out_h, d.out_w)
    # x on a 16-byte boundary, or 4 bytes past one
    xbuf = torch.empty(x.size + 4, device=device)
    off = 0 if cs["align16"] else 1
    xd = xbuf[off:off + x.size].view(cs["x"])
    xd.copy_(T(x, device))
    assert (xd.data_ptr() % 16 == 0) == cs["align16"] and xd.data_ptr() % 4 == 0
    wd, bd = T(w, device), T(b, device)

    assert ops.get_f32_engine() == ops.ENGINE_BF16X6
    assert ops.conv_fwd_kernel_id(d, xd.data_ptr() % 16 == 0) == kid        # the kernel this launch runs
    big, y = _guarded(yshape, device)
    ops.conv2d_fwd(d, xd, wd, bd, y, relu=relu)
    _sentinels_intact(big, kid)
    got = N(y)
    assert not np.isnan(got).any(), f"{kid}: {int(np.isnan(got).sum())} outputs left unwritten"

    # accuracy: fp32 level, and against the fp32-MFMA engine on the same data
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        assert ops.conv_fwd_kernel_id(d, cs["align16"]) == "f32"
        yf = torch.empty(yshape, device=device)
        ops.conv2d_fwd(d, xd, wd, bd, yf, relu=relu)
        got_f32 = N(yf)
    finally:
        ops.set_f32_engine(prev)
    e6, e32 = _errs(got, ref, scale, relu), _errs(got_f32, ref, scale, relu)
    print(f"X6MATRIX {kid} relu={int(relu)} err/scale max x6 {e6[0]:.3e} f32 {e32[0]:.3e} "
          f"mean x6 {e6[1]:.3e} f32 {e32[1]:.3e}")
    assert_scaled(got, ref, scale, kid, tol=TOL, relu=relu)
    bad = x6_guard_failures(e6, e32)
    assert not bad, f"{kid}: bf16x6 " + "; ".join(bad)

    # companions
    if fam in OCTET_FAMILIES:
        with_yo = cs["cout"] % 8 == 0
        xo = _oct_buf(cs["x"], device)
        ops.pack_octets(xd, xo, *cs["x"])
        yo_ref = octets_ref(got) if with_yo else None
        for use_xo in (False, True):
            big1, y1 = _guarded(yshape, device)
            yo = _oct_buf(yshape, device) if with_yo else None
            ops.conv2d_fwd_octets(d, xd, xo if use_xo else None, wd, bd, y1, yo, relu=relu)
            _sentinels_intact(big1, f"{kid} octets")
            np.testing.assert_array_equal(N(y1).view(np.uint32), got.view(np.uint32))
            if with_yo:
                np.testing.assert_array_equal(_as_u16(yo, yshape), yo_ref)
        if ops.conv_output_octets_only(d) == 1:
            yo2 = _oct_buf(yshape, device)
            ops.conv2d_fwd_octets(d, xd, xo, wd, bd, None, yo2, relu=relu)
            np.testing.assert_array_equal(_as_u16(yo2, yshape), yo_ref)

    # strided output: a channel slice of a wider NCHW tensor
    if STRIDED[fam] == i:
        n, cout, hw = yshape[0], yshape[1], d.out_h * d.out_w
        lo, ctot = 3, cout + 8
        top = torch.full((n, ctot, d.out_h, d.out_w), SENTINEL, dtype=torch.int32, device=device)
        ops.conv2d_fwd_strided(d, xd, wd, bd, top[:, lo:].view(torch.float32), ctot * hw, relu=relu)
        t = N(top)
        np.testing.assert_array_equal(t[:, lo:lo + cout].view(np.uint32), got.view(np.uint32))
        assert (t[:, :lo] == SENTINEL).all() and (t[:, lo + cout:] == SENTINEL).all(), f"{kid}: wrote outside its slice"

    # weight pack: packed by the call, then reused
    nb = ops.conv_weight_pack_bytes(d)
    assert nb > 0, kid
    wp = torch.zeros(nb, dtype=torch.uint8, device=device)
    for valid in (False, True):
        big2, y2 = _guarded(yshape, device)
        ops.conv2d_fwd_cached(d, xd, None, wd, wp, valid, bd, y2, None, relu=relu)
        _sentinels_intact(big2, f"{kid} cached")
        np.testing.assert_array_equal(N(y2).view(np.uint32), got.view(np.uint32))
