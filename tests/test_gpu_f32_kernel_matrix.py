"""Every reachable fp32-MFMA kernel instantiation against fp64.

tests/_f32_cases.py holds, per kernel id and K split (ops.gemm_kernel_ids and
its siblings), the cheapest shape that selects it through a public entry
point.  Each case runs here with its id lines asserted again before the
launch, in two passes:

  exact     operands, bias, C0, dw0 and db0 are integer-valued floats in
            {-3..3}, alpha and beta in {1, 0.5, 2, 0}.  Then every product and
            every partial sum is an integer (or a half) far below 2^24
            (9 K + |beta C0| + |bias| < 2^24, asserted per case on the CPU by
            _f32_cases.exact_ok), so any fp32 summation order, any split-K and
            any reduce kernel gives the float64 result bit for bit:
            np.array_equal.  One dropped, duplicated or misplaced product
            fails, which a scale-relative bound can hide at long K.
  gaussian  standard-normal inputs, weights x 0.1, _ref64.assert_scaled at the
            project's TOL against float64.

Outputs the kernels write start as NaN; outputs they accumulate into start
from known values.  Dense cases run with lda, ldb and ldc above their minimum,
NaN guard elements between the rows of A, B and C: those of C must still be
NaN afterwards and those of A and B must not reach the result.
"""
import numpy as np
import pytest

from _f32_cases import F32_CASES, LD_PAD, conv_desc, epilogue, ids_of, label, ld

pytestmark = pytest.mark.gpu

IDS = [label(i) for i in range(len(F32_CASES))]
PASSES = ["exact", "gaussian"]


@pytest.fixture(autouse=True)
def _f32_engine():
    from rramsim import ops
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    yield
    ops.set_f32_engine(prev)


def _draw(rng, shape, exact, scale=1.0):
    if exact:
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def _dev(a, device, align16=True):
    """a on the device, 16-byte aligned or 4 bytes past a 16-byte boundary."""
    import torch
    a = np.array(a, dtype=np.float32, order="C", copy=True)      # (a flipped view has negative strides)
    buf = torch.empty(a.size + 4, device=device)
    off = 0 if align16 else 1
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert (t.data_ptr() % 16 == 0) == align16
    return t


def _ws(nbytes, device):
    import torch
    return torch.empty(nbytes // 4, device=device) if nbytes else None


def _check(got, ref, scale, exact, what, relu=False):
    from _ref64 import assert_scaled
    got = np.asarray(got)
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} outputs left unwritten"
    if relu:
        ref = np.maximum(ref, 0.0)
    if exact:
        diff = int((got.astype(np.float64).reshape(ref.shape) != ref).sum())
        assert np.array_equal(got.astype(np.float64).reshape(ref.shape), ref), f"{what}: {diff} elements differ"
    else:
        assert_scaled(got, ref, scale, what)


def _padded(op, ldx):
    """Row-major matrix `op` stored with row stride ldx, NaN in the padding."""
    out = np.full((op.shape[0], ldx), np.nan, np.float32)
    out[:, :op.shape[1]] = op
    return out


def _run_gemm(i, cs, exact, device, alpha=None):
    from rramsim import ops
    rng = np.random.default_rng(7000 + i)
    M, N, K, ta, tb = cs["M"], cs["N"], cs["K"], cs["ta"], cs["tb"]
    alpha0, beta, bias_mode, relu = epilogue(i)
    alpha = alpha0 if alpha is None else alpha
    lda, ldb = ld(cs)
    ldc = N + LD_PAD + 1
    A = _draw(rng, (M, K), exact)
    B = _draw(rng, (K, N), exact, 0.1)
    C0 = _draw(rng, (M, N), exact)
    bias = _draw(rng, (M if bias_mode == 1 else N,), exact) if bias_mode else None
    Ad = _dev(_padded(A.T if ta else A, lda), device, cs["a16"])
    Bd = _dev(_padded(B.T if tb else B, ldb), device, cs["b16"])
    Cd = _dev(_padded(C0 if beta != 0.0 else np.full((M, N), np.nan, np.float32), ldc), device)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = alpha * (A64 @ B64) + (beta * C0.astype(np.float64) if beta != 0.0 else 0.0)
    scale = abs(alpha) * (np.abs(A64) @ np.abs(B64)) + abs(beta) * np.abs(C0)
    if bias_mode:
        b64 = bias.astype(np.float64)[:, None] if bias_mode == 1 else bias.astype(np.float64)[None, :]
        ref, scale = ref + b64, scale + np.abs(b64)
    ops.gemm_ex(ta, tb, M, N, K, alpha, Ad, lda, Bd, ldb, beta, Cd, ldc, None if bias is None else _dev(bias, device),
                bias_mode, relu, _ws(cs["ws"], device))
    got = Cd.cpu().numpy()
    assert np.isnan(got[:, N:]).all(), "the guard elements between the rows of C were written"
    _check(got[:, :N], ref, scale, exact, "C", relu)


def _run_ip_fwd(i, cs, exact, device, G=1, bias_on=None, relu=None):
    import torch
    from rramsim import ops
    rng = np.random.default_rng(7000 + i)
    M, N, K, t = cs["M"], cs["N"], cs["K"], cs["t"]
    bias_on, relu = cs.get("bias", bias_on), cs.get("relu", relu)
    x = _draw(rng, (G, M, K), exact)
    w = _draw(rng, (G, N, K), exact, 0.1)
    b = _draw(rng, (G, N), exact) if bias_on else None
    y = torch.full((G, M, N), float("nan"), device=device)
    wd = _dev(np.swapaxes(w, 1, 2) if t else w, device)
    bd = None if b is None else _dev(b, device)
    if cs["entry"] == "ip_groups":
        ops.ip_fwd_groups(_dev(x, device), wd, N * K, bd, N if bias_on else 0, y, G, M, N, K, bool(t), relu,
                          _ws(cs["ws"], device))
    else:
        ops.ip_fwd(_dev(x[0], device), wd, bd, y, M, N, K, bool(t), relu, _ws(cs["ws"], device))
    from _ref64 import ip64
    got = y.cpu().numpy()
    for g in range(G):
        ref, scale = ip64(x[g], w[g], None if b is None else b[g])
        _check(got[g], ref, scale, exact, f"y[{g}]", relu)


def _run_ip_bwd(i, cs, exact, device):
    import torch
    from rramsim import ops
    rng = np.random.default_rng(7000 + i)
    M, N, K, t = cs["M"], cs["N"], cs["K"], cs["t"]
    x, w, dy = _draw(rng, (M, K), exact), _draw(rng, (N, K), exact, 0.1), _draw(rng, (M, N), exact)
    dw0, db0 = _draw(rng, (N, K), exact), _draw(rng, (N,), exact)
    dwd = _dev(dw0.T if t else dw0, device) if cs["dw"] else None
    dbd = _dev(db0, device) if cs["db"] else None
    dxd = torch.full((M, K), float("nan"), device=device) if cs["dx"] else None
    ops.ip_bwd(_dev(x, device), _dev(w.T if t else w, device), _dev(dy, device), dwd, dbd, dxd, M, N, K, bool(t))
    x64, w64, dy64 = (a.astype(np.float64) for a in (x, w, dy))
    if cs["dw"]:
        got = dwd.cpu().numpy()
        _check(got.T if t else got, dw0 + dy64.T @ x64, np.abs(dw0) + np.abs(dy64).T @ np.abs(x64), exact, "dW")
    if cs["db"]:
        _check(dbd.cpu().numpy(), db0 + dy64.sum(0), np.abs(db0) + np.abs(dy64).sum(0), exact, "db")
    if cs["dx"]:
        _check(dxd.cpu().numpy(), dy64 @ w64, np.abs(dy64) @ np.abs(w64), exact, "dX")


def _conv_data(i, cs, exact):
    rng = np.random.default_rng(7000 + i)
    n, c, h, wd_ = cs["x"]
    x = _draw(rng, cs["x"], exact)
    w = _draw(rng, (cs["cout"], c // cs["g"], cs["k"], cs["k"]), exact, 0.1)
    b = _draw(rng, (cs["cout"],), exact)
    return rng, x, w, b


def _run_conv_fwd(i, cs, exact, device):
    import torch
    from _ref64 import conv64
    from rramsim import ops
    _, x, w, b = _conv_data(i, cs, exact)
    d = conv_desc(cs)
    ref, scale = conv64(x, w, b, cs["s"], cs["p"], cs["g"], cs["d"])
    xd, wd, bd = _dev(x, device), _dev(w, device, cs["w16"]), _dev(b, device)
    for relu in (False, True):
        y = torch.full(ref.shape, float("nan"), device=device)
        ops.conv2d_fwd(d, xd, wd, bd, y, relu=relu)
        _check(y.cpu().numpy(), ref, scale, exact, f"y relu={relu}", relu)


def _run_conv_bwd(i, cs, exact, device):
    import torch
    from rramsim import ops
    F = torch.nn.functional
    rng, x, w, b = _conv_data(i, cs, exact)
    d = conv_desc(cs)
    dy = _draw(rng, (cs["x"][0], cs["cout"], d.out_h, d.out_w), exact)
    dw0, db0 = _draw(rng, w.shape, exact), _draw(rng, b.shape, exact)

    def grads(absolute):
        f = (lambda a: torch.from_numpy(a).double().abs()) if absolute else (lambda a: torch.from_numpy(a).double())
        xs = [f(a).clone().requires_grad_(True) for a in (x, w, b)]
        F.conv2d(*xs, cs["s"], cs["p"], cs["d"], cs["g"]).backward(f(dy))
        return [t.grad.numpy() for t in xs]

    (gx, gw, gb), (sx, sw, sb) = grads(False), grads(True)
    xd, wd, dyd = _dev(x, device), _dev(w, device, cs["w16"]), _dev(dy, device)
    wf = None
    if cs["wflip"]:     # rot180 of each group's kernel with in <-> out channels swapped (k_flip_kernel's layout)
        g, cg, og = cs["g"], cs["x"][1] // cs["g"], cs["cout"] // cs["g"]
        wf = _dev(np.flip(w.reshape(g, og, cg, cs["k"], cs["k"]).transpose(0, 2, 1, 3, 4), (3, 4)), device)
    dxs = []
    for flip in ([wf, None] if cs["wflip"] else [None]):
        dwd = _dev(dw0, device) if cs["dw"] else None
        dbd = _dev(db0, device) if cs["db"] else None
        dxd = torch.full(cs["x"], float("nan"), device=device) if cs["dx"] else None
        # the run without the caller's copy gets room for the flipped kernel, so both take the forward form
        wsb = cs["ws"] if flip is not None or not cs["wflip"] else max(cs["ws"], w.size * 4)
        ops.conv2d_bwd_ex(d, xd, wd, flip, dyd, dwd, dbd, dxd, _ws(wsb, device))
        if cs["dw"]:
            _check(dwd.cpu().numpy(), dw0 + gw, np.abs(dw0) + sw, exact, "dW")
        if cs["db"]:
            _check(dbd.cpu().numpy(), db0 + gb, np.abs(db0) + sb, exact, "db")
        if cs["dx"]:
            dxs.append(dxd.cpu().numpy())
            _check(dxs[-1], gx, sx, exact, "dX")
    assert len(dxs) == (2 if cs["wflip"] and cs["dx"] else 1 if cs["dx"] else 0)
    if len(dxs) == 2:
        assert np.array_equal(dxs[0].view(np.uint32), dxs[1].view(np.uint32)), "dX differs with the caller's w_flipped"


def _run_ip_groups(i, cs, exact, device):
    """The grouped forward's launches do not depend on bias or ReLU: plain, then per-group bias with ReLU."""
    _run_ip_fwd(i, cs, exact, device, cs["G"], False, False)
    _run_ip_fwd(i, cs, exact, device, cs["G"], True, True)


RUN = {"gemm": _run_gemm, "ip_fwd": _run_ip_fwd, "ip_bwd": _run_ip_bwd, "conv_fwd": _run_conv_fwd,
       "conv_bwd": _run_conv_bwd, "ip_groups": _run_ip_groups}


@pytest.mark.parametrize("mode", PASSES)
@pytest.mark.parametrize("i", range(len(F32_CASES)), ids=IDS)
def test_kernel_instantiation(device, i, mode):
    cs = F32_CASES[i]
    assert ids_of(cs) == cs["ids"]          # the kernels this call launches
    RUN[cs["entry"]](i, cs, mode == "exact", device)


@pytest.mark.parametrize("mode", PASSES)
@pytest.mark.parametrize("ws", [0, 64 << 20], ids=["unsplit", "split"])
def test_gemm_alpha_zero(device, ws, mode):
    """alpha = 0 (no table case has it): C = beta C0 + bias whatever A and B hold, unsplit and split."""
    cs = dict(entry="gemm", ta=0, tb=1, M=100, N=500, K=1027, a16=False, b16=True, ws=ws)
    assert any("/s1 " in ln for ln in ids_of(cs)) == (ws == 0)
    for i in range(6):                      # row and column bias, beta zero and not
        _run_gemm(i, cs, mode == "exact", device, alpha=0.0)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("outs", [1, 5, 8200])       # 8200 > 4 waves x 2048 blocks: the grid-stride loop runs
@pytest.mark.parametrize("red", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("trans", [0, 1])
def test_gemv_direct(device, trans, red, outs, beta):
    """rram_gemv_f32 at the lengths where its lane loop and grid-stride loop
    change behaviour; integer data, so float64 bit for bit.  beta = 0 must not
    read y (NaN-filled)."""
    import torch
    from rramsim import ops
    rng = np.random.default_rng(red * 10 + outs + trans)
    M, Nn = (red, outs) if trans else (outs, red)
    A, x = _draw(rng, (M, Nn), True), _draw(rng, (red,), True)
    y0 = _draw(rng, (outs,), True)
    y = _dev(y0, device) if beta else torch.full((outs,), float("nan"), device=device)
    ops.gemv(trans, M, Nn, 2.0, _dev(A, device), _dev(x, device), beta, y)
    A64 = A.astype(np.float64)
    ref = 2.0 * ((A64.T if trans else A64) @ x.astype(np.float64)) + (beta * y0 if beta else 0.0)
    assert 2 * 9 * red + 3 < 2 ** 23
    _check(y.cpu().numpy(), ref, None, True, "y")


@pytest.mark.parametrize("mode", PASSES)
@pytest.mark.parametrize("want", [(1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0)], ids=["all", "no-db", "no-dx", "db"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 130, 66), (64, 500, 800)])
def test_ip_bwd_transposed_direct(device, shape, want, mode):
    """rram_ip_bwd with transpose = 1 (W, dW stored [K][N]), db or dx NULL."""
    M, N, K = shape
    cs = dict(entry="ip_bwd", M=M, N=N, K=K, t=1, dw=want[0], db=want[1], dx=want[2])
    _run_ip_bwd(M + N + K, cs, mode == "exact", device)
